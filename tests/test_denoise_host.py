"""Host-side checks of the denoiser (include/trg_denoise.h, toyraygun_amd/denoise.py): exported surface, the files it must leave alone, and the
float64 reference the GPU tests compare the kernels with.  No GPU."""
import json
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_denoise.h")


def test_library_exports_and_python_binds_every_declared_symbol(built):
    from toyraygun_amd import capi, denoise
    declared = sorted(set(denoise.header_symbols(HEADER)))
    assert len(declared) >= 5 and {"trg_guides_render", "trg_denoise", "trg_render_denoised", "trg_denoise_release",
                                   "trg_denoise_default_params"} <= set(declared)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(denoise.SYMBOL_NAMES) == declared      # the Python module covers the whole header
    L = denoise.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None
    p = denoise.default_params()
    assert (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth, p.demodulate) == (5, 4.0, 128.0, 1.0, 1)


def test_render_abi_and_hashed_kernel_sources_are_untouched(built):
    """The denoiser lives beside the render path: trg.h names none of it, capi.SYMBOL_NAMES is still trg.h, and the kernel-source hash is the
    one the committed profiler counters were measured on."""
    from toyraygun_amd import capi, denoise
    from toyraygun_amd.srchash import kernel_source_hash
    trg_h = open(os.path.join(ROOT, "include", "trg.h")).read()
    for name in denoise.SYMBOL_NAMES + ["trg_denoise_params"]:
        assert name not in trg_h, name
        assert name not in capi.SYMBOL_NAMES
    with open(os.path.join(ROOT, "profiles", "r05", "c2_counters.json")) as f:
        assert json.load(f)["kernel_source_hash"] == kernel_source_hash()


# ---- the float64 reference --------------------------------------------------------------------------------------------------------------------
def _flat_guides(h, w, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=(0.5, 0.6, 0.7)):
    g0 = np.zeros((h, w, 4), np.float32)
    g1 = np.zeros((h, w, 4), np.float32)
    g0[..., :3] = normal; g0[..., 3] = depth
    g1[..., :3] = albedo
    g1[..., 3] = np.zeros((h, w), np.int32).view(np.float32)
    return g0, g1


def test_reference_keeps_a_constant_image_constant():
    from toyraygun_amd.denoise import reference_denoise
    g0, g1 = _flat_guides(23, 31)
    g0[..., 3] = 1.0 + 0.01 * np.arange(31, dtype=np.float32)[None, :]      # a depth ramp changes weights, not a constant
    c = np.empty((23, 31, 4), np.float32)
    c[...] = (0.3, 1.7, 0.9, 0.5)
    for demod in (0, 1):
        out = reference_denoise(c, g0, g1, iterations=5, demodulate=demod)
        assert np.abs(out - c.astype(np.float64)).max() <= 1e-12


def test_reference_zero_iterations_is_the_identity():
    from toyraygun_amd.denoise import reference_denoise
    rng = np.random.default_rng(3)
    g0, g1 = _flat_guides(9, 11)
    c = rng.uniform(0, 4, (9, 11, 4)).astype(np.float32)
    assert np.array_equal(reference_denoise(c, g0, g1, iterations=0), c.astype(np.float64))


def test_reference_does_not_filter_across_orthogonal_normals():
    from toyraygun_amd.denoise import reference_denoise
    h, w = 20, 40
    g0, g1 = _flat_guides(h, w, albedo=(1.0, 1.0, 1.0))
    g0[:, w // 2:, :3] = (1.0, 0.0, 0.0)                                    # n . n = 0 across the edge: w_n = 0
    c = np.zeros((h, w, 4), np.float32)
    c[:, w // 2:, :3] = 1.0
    c[..., 3] = 1.0
    out = reference_denoise(c, g0, g1, iterations=5)
    assert np.array_equal(out, c.astype(np.float64))


def test_reference_weights_of_an_interior_pixel_sum_to_one():
    """Flat guides and a constant image: every w_n = w_z = w_c = 1, so the weights of a pixel whose 25 taps are all inside are the B3 kernel,
    which sums to 1; a corner pixel sees 9 of them, (3/8 + 1/4 + 1/16)^2."""
    from toyraygun_amd.denoise import atrous_weights
    g0, _ = _flat_guides(16, 16)
    I = np.full((16, 16, 3), 0.8)
    W = atrous_weights(I, g0.astype(np.float64), 2, 4.0, 128.0, 1.0)
    assert abs(W[:, :, 8, 8].sum() - 1.0) <= 1e-12
    assert abs(W[:, :, 0, 0].sum() - (3 / 8 + 1 / 4 + 1 / 16) ** 2) <= 1e-12
    assert (W[:2, :, 0, 0] == 0).all() and (W[:, :2, 0, 0] == 0).all()      # taps outside the image are skipped


def test_reference_keeps_emitters_out_of_the_filter():
    """A bright block whose first hit is an emissive primitive on a surface of the same normal and depth: with the scene's material ids it
    keeps its input and its neighbours do not brighten; without a scene it is filtered like everything else."""
    from toyraygun_amd.denoise import emitter_mask, reference_denoise
    h, w = 24, 24
    g0, g1 = _flat_guides(h, w, albedo=(1.0, 1.0, 1.0))
    ids = np.zeros((h, w), np.int32)
    ids[10:14, 10:14] = 1
    g1[..., 3] = ids.view(np.float32)
    c = np.full((h, w, 4), 0.2, np.float32)
    c[10:14, 10:14, :3] = 1.5
    mats = np.array([1, 2], np.uint32)
    assert emitter_mask(g1, mats).sum() == 16
    out = reference_denoise(c, g0, g1, iterations=3, material_ids=mats)
    assert np.abs(out - c.astype(np.float64)).max() <= 1e-12
    assert np.abs(reference_denoise(c, g0, g1, iterations=3) - c).max() > 0.1
