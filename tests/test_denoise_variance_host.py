"""Host-side checks of the variance-guided filter from two half-sample buffers (include/trg_denoise.h, toyraygun_amd/denoise.py): the exported
surface, the float64 reference on synthetic inputs, and its quality on the Cornell box from the CPU oracle alone.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_denoise.h")
f32 = np.float32

NEW_SYMBOLS = {"trg_render_halves", "trg_render_halves_read", "trg_denoise_variance", "trg_denoise_variance_host", "trg_render_denoised_variance",
               "trg_render_denoised_variance_read", "trg_render_denoised_variance_own", "trg_denoise_var_default_params"}


def test_header_exports_and_python_agree_on_the_variance_entry_points(built):
    from toyraygun_amd import capi, denoise
    declared = set(denoise.header_symbols(HEADER))
    assert NEW_SYMBOLS <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(denoise.SYMBOL_NAMES) == sorted(declared)
    p = denoise.make_var_params()
    assert (p.iterations, p.sigma_lum, p.sigma_normal, p.sigma_depth, p.demodulate, p.prefilter) == (5, 4.0, 128.0, 1.0, 1, 1)
    assert {k: getattr(p, k) for k, _ in denoise.VarParams._fields_} == denoise._VAR_DEFAULTS      # the reference's defaults are the library's
    q = denoise.default_params()                                                                     # trg_denoise_params keeps its layout
    assert [f for f, _ in denoise.Params._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_depth", "demodulate"]
    assert (q.iterations, q.sigma_color, q.demodulate) == (5, 4.0, 1)


def _flat_guides(h, w, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=(0.5, 0.6, 0.7)):
    g0 = np.zeros((h, w, 4), f32)
    g1 = np.zeros((h, w, 4), f32)
    g0[..., :3] = normal; g0[..., 3] = depth
    g1[..., :3] = albedo
    g1[..., 3] = np.zeros((h, w), np.int32).view(f32)
    return g0, g1


def test_reference_zero_iterations_is_the_mean_of_the_halves():
    from toyraygun_amd.denoise import reference_denoise_variance
    rng = np.random.default_rng(3)
    g0, g1 = _flat_guides(9, 11)
    h1, h2 = (rng.uniform(0, 4, (9, 11, 4)).astype(f32) for _ in range(2))
    for pre in (0, 1):
        out = reference_denoise_variance(h1, h2, g0, g1, iterations=0, prefilter=pre)
        assert np.array_equal(out[..., :3], 0.5 * (h1[..., :3].astype(np.float64) + h2[..., :3]))
        assert np.array_equal(out[..., 3], h1[..., 3].astype(np.float64))


def test_reference_with_equal_halves_has_no_variance_and_stays_finite():
    """H1 == H2: V_0 = 0 everywhere, every w_l has the bare 1e-3 in its denominator; the result is finite, V stays 0, and a constant image stays
    what it was."""
    from toyraygun_amd.denoise import reference_denoise_variance
    rng = np.random.default_rng(4)
    g0, g1 = _flat_guides(21, 27)
    g0[..., 3] = 1.0 + 0.01 * np.arange(27, dtype=f32)[None, :]
    h = rng.uniform(0, 4, (21, 27, 4)).astype(f32)
    for demod in (0, 1):
        out, v = reference_denoise_variance(h, h, g0, g1, demodulate=demod, return_variance=True)
        assert np.isfinite(out).all() and (v == 0).all()
        assert np.array_equal(out[..., 3], h[..., 3].astype(np.float64))
    c = np.empty((21, 27, 4), f32)
    c[...] = (0.3, 1.7, 0.9, 0.5)
    assert np.abs(reference_denoise_variance(c, c, g0, g1) - c.astype(np.float64)).max() <= 1e-12


def test_reference_keeps_a_luminance_step_better_than_the_spatial_variance_filter():
    """A step edge in luminance on ONE flat surface (normals, depth and albedo tell nothing), low noise: the 3 x 3 spatial variance of
    reference_denoise is large exactly at the edge, which opens w_c there; the per-pixel variance of the samples stays small, so w_l keeps the
    edge.  Measured as the error against the noise-free step in the band of +-8 pixels around it, after 5 iterations at default parameters."""
    from toyraygun_amd.denoise import reference_denoise, reference_denoise_variance
    h, w = 32, 48
    rng = np.random.default_rng(5)
    g0, g1 = _flat_guides(h, w, albedo=(1.0, 1.0, 1.0))
    clean = np.full((h, w, 4), 0.2)
    clean[:, w // 2:, :3] = 1.0
    clean[..., 3] = 1.0
    h1 = (clean + np.concatenate([rng.normal(0, 0.02, (h, w, 3)), np.zeros((h, w, 1))], -1)).astype(f32)
    h2 = (clean + np.concatenate([rng.normal(0, 0.02, (h, w, 3)), np.zeros((h, w, 1))], -1)).astype(f32)
    mean = (0.5 * (h1.astype(np.float64) + h2)).astype(f32)
    band = (slice(None), slice(w // 2 - 8, w // 2 + 8), slice(0, 3))
    err = lambda a: float(np.sqrt(((a[band] - clean[band]) ** 2).mean()))
    old = err(reference_denoise(mean, g0, g1))
    new = err(reference_denoise_variance(h1, h2, g0, g1))
    print("step edge, band rmse: raw %.5f, reference_denoise %.5f, reference_denoise_variance %.5f" % (err(mean.astype(np.float64)), old, new))
    assert new < old
    assert new < err(mean.astype(np.float64))          # and it did remove noise there


# ---- quality, from the oracle alone ----------------------------------------------------------------------------------------------------------
def oracle_halves(O, scene, w, h, b, n, bounces, offsets):
    """The procedure of trg_render_halves on the oracle: two renders from zeroed buffers, one fp32 multiply per channel, alpha copied."""
    half = n // 2
    a, _ = O.render(scene, w, h, half, bounces, frame_begin=b, offsets=offsets, want_stats=False)
    c, _ = O.render(scene, w, h, half, bounces, frame_begin=b + half, offsets=offsets, want_stats=False)
    f1, f2 = f32(np.float64(b + half) / np.float64(half)), f32(np.float64(b + n) / np.float64(half))
    h1, h2 = a.copy(), c.copy()
    h1[..., :3] = a[..., :3] * f1
    h2[..., :3] = c[..., :3] * f2
    return np.stack([h1, h2])


def oracle_guides(O, scene, w, h, frame, offsets):
    """[2, h, w, 4] guide planes from the oracle's primary rays, as tests/test_gpu_denoise.py builds its reference guides."""
    from tests.test_gpu_denoise import _reference_guides
    _, prim, dist, nrm, alb = _reference_guides(O, scene, scene.buffers(), w, h, frame, offsets=offsets)
    g = np.zeros((2, h, w, 4), f32)
    g[0, ..., :3] = nrm
    g[0, ..., 3] = np.where(prim >= 0, dist, f32(-1.0))
    g[1, ..., :3] = alb
    g[1, ..., 3] = prim.astype(np.int32).view(f32)
    return g


def test_quality_on_the_cornell_box_from_the_oracle(O, cornell):
    """Cornell box, 128 x 96, 3 bounces; halves b = 0, n = 4 and guides of frame 0 from the oracle; target: the oracle's 256 spp.  The
    variance-guided reference at default parameters must beat the raw 4-spp mean.  Printed beside it: reference_denoise on the same mean for
    1 / 3 / 5 iterations and the new filter for the same counts (NOTEBOOK.md, "Denoiser", has the table)."""
    from toyraygun_amd import denoise as dn
    w, h = 128, 96
    off = O.pixel_offsets(w, h)
    target, _ = O.render(cornell, w, h, 256, 3, offsets=off, want_stats=False)
    hv = oracle_halves(O, cornell, w, h, 0, 4, 3, off)
    g = oracle_guides(O, cornell, w, h, 0, off)
    mats = cornell.buffers()["material_ids"]
    rmse = lambda a: float(np.sqrt(((np.asarray(a)[..., :3].astype(np.float64) - target[..., :3]) ** 2).mean()))
    mean = dn.reference_denoise_variance(hv[0], hv[1], g[0], g[1], iterations=0)
    plain4, _ = O.render(cornell, w, h, 4, 3, offsets=off, want_stats=False)
    print("rmse against 256 spp: mean of the halves %.5f (one 4-spp render %.5f)" % (rmse(mean), rmse(plain4)))
    for it in (1, 3, 5):
        old = dn.reference_denoise(mean.astype(f32), g[0], g[1], iterations=it, material_ids=mats)
        new = dn.reference_denoise_variance(hv[0], hv[1], g[0], g[1], iterations=it, material_ids=mats)
        print("  %d iterations: reference_denoise %.5f   reference_denoise_variance %.5f" % (it, rmse(old), rmse(new)))
    assert it == 5 and rmse(new) < rmse(mean)              # (5 iterations = the default parameters)
