"""GPU tests (-m gpu) of trg_guides_render where tests/test_gpu_denoise.py does not reach: triangles whose three corners carry different normals
and colours, trees deep enough for the guide pass's own stack scratch, leaf orders of the device builders, duplicate / degenerate / emissive
triangles, ray counts that are no multiple of 256, images smaller than a tile, and one state serving scenes of different sizes in turn.
Everything is compared with the CPU oracle through _reference_guides / _check_guides, in the strict and the shipped setting."""
import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _check_guides, _close, _reference_guides, _grazing, _shipped_attr_bars
from tests.test_gpu_parity import _random_soup, _uv_sphere
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 50, 37            # 1,850 rays: seven full workgroups of the tracer and 58 rays of an eighth


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def dn(capi):
    from toyraygun_amd import denoise
    denoise.load()
    return denoise


def _ref_with_margin(O, scene, b, w, h, frame, off):
    """(oracle guides, the pixels fp32 cannot decide): those whose float64 margin is below 1e-5 (the set rule of test_intersector) and those
    whose first hit is grazing (_grazing: the distance's own conditioning puts one rounding above the 3e-6 rule).  The callers hold the share
    of both together under the existing caps; the oracle counts 3 and 1 grazing pixels on the fine sphere, 0 and 1 in the soup, none on
    the coarse sphere or in the Cornell box."""
    ref = _reference_guides(O, scene, b, w, h, frame, offsets=off)
    _, _, margin = O.nearest_f64(scene, ref[0])
    return ref, (margin < 1e-5).reshape(h, w) | _grazing(b, ref)


def _check_both_settings(capi, dn, c, b, frame, ref, undecidable):
    """guides of `frame` in the strict and the shipped setting against the oracle; returns the two results."""
    out = []
    for strict in (1, 0):
        c.set_option(capi.OPT_STRICT, strict)
        g = dn.guides(c, frame)
        _check_guides(g, ref, strict, undecidable, attr_bars=None if strict else _shipped_attr_bars(b, ref[1]))
        out.append(g)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- 1. varying attributes
@pytest.mark.parametrize("nu,nv,in_lds", [(8, 5, 1), (40, 24, 0)])
def test_guides_interpolate_per_corner_attributes(capi, dn, O, nu, nv, in_lds):
    """The Cornell box plus a tessellated sphere with per-vertex normals and colours (Scene::addMesh), LDS-resident (64 + 36 triangles) and
    HBM-resident (1,840 + 36), 50 x 37.  The sphere (radius 0.7 around (0, 1, 0.4)) is the first hit of at least 300 pixels on at least 20
    different triangles.  Strict: ids equal, distances bit-equal, normal and albedo within 1e-6.  Shipped: on the pixels float64 geometry can
    decide, the bar derived from the 2e-5 its barycentrics are allowed (_shipped_attr_bars).  And the comparison can fail: against a reference
    whose mesh corners are rotated (v0 <- v1 <- v2 <- v0, positions untouched) the same guides are refused."""
    from toyraygun_amd import host
    v, n, col, tris = _uv_sphere(nu, nv, 0.7, (0.0, 1.0, 0.4))
    hs = host.Scene.cornell_box()
    hs.add_mesh(v, n, tris, np.eye(4, dtype=f32), col, 1)
    b = hs.buffers()
    assert b["material_ids"].shape[0] == 36 + tris.shape[0]
    mesh_n, mesh_c = b["normals"][108:].reshape(-1, 3, 3), b["colors"][108:].reshape(-1, 3, 3)
    assert (np.abs(mesh_n[:, 0] - mesh_n[:, 1]).max(-1) > 1e-3).mean() > 0.9 and (np.abs(mesh_c[:, 0] - mesh_c[:, 2]).max(-1) > 1e-3).mean() > 0.9
    scene = O.OracleScene()
    scene.add_raw(b["positions"], b["normals"], b["colors"], b["material_ids"])
    off = O.pixel_offsets(W, H)
    c = capi.Context(W, H)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        assert c.stats().scene_in_lds == in_lds
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(W, H)))
        c.set_pixel_offsets(off)
        for frame in (0, 7):
            ref, undecidable = _ref_with_margin(O, scene, b, W, H, frame, off)
            on_mesh = ref[1] >= 36
            assert on_mesh.sum() >= 300 and len(np.unique(ref[1][on_mesh])) >= 20
            assert undecidable.mean() < 0.05
            strict_g, shipped_g = _check_both_settings(capi, dn, c, b, frame, ref, undecidable)
            # the interpolated values really vary inside the triangles: far more distinct normals than triangles
            assert len(np.unique(_bits(strict_g[0, ..., :3][on_mesh]), axis=0)) >= 0.9 * on_mesh.sum()
            rot = dict(b)
            for k in ("normals", "colors"):
                a = b[k].copy()
                a[108:] = a[108:].reshape(-1, 3, 3)[:, [1, 2, 0]].reshape(-1, 3)
                rot[k] = a
            wrong = _reference_guides(O, scene, rot, W, H, frame, offsets=off)
            assert np.array_equal(wrong[1], ref[1])
            wrong_bars = _shipped_attr_bars(rot, wrong[1])
            for g, strict in ((strict_g, 1), (shipped_g, 0)):
                with pytest.raises(AssertionError, match="guide normals differ"):      # ids, distances and misses pass: the attributes fail
                    _check_guides(g, wrong, strict, undecidable, attr_bars=None if strict else wrong_bars)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 2. deep trees
@pytest.fixture(scope="module")
def soup(O):
    """_random_soup(O, 3000, 5): exact duplicates, coplanar overlapping pairs, zero-area and needle triangles, emissive and masked ones; its
    oracle guides of frames 0 and 7 at 50 x 37."""
    scene = _random_soup(O, 3000, 5)
    b = scene.buffers()
    off = O.pixel_offsets(W, H)
    refs = {frame: _ref_with_margin(O, scene, b, W, H, frame, off) for frame in (0, 7)}
    return scene, b, off, refs


def _check_soup(capi, dn, c, b, refs, frames=(0, 7)):
    mats = b["material_ids"]
    for frame in frames:
        ref, undecidable = refs[frame]
        # the duplicate and coplanar triangles of the soup are ties by construction: 0.0449 of the pixels in both frames
        assert undecidable.mean() < 0.06
        prim = ref[1]
        emissive = (prim >= 0) & (mats[np.where(prim >= 0, prim, 0)] == 2)
        assert emissive.sum() >= 150
        ref_g1 = np.concatenate([ref[4], np.ascontiguousarray(prim).view(f32)[..., None]], -1)
        for g, strict in zip(_check_both_settings(capi, dn, c, b, frame, ref, undecidable), (1, 0)):
            ok = np.ones(prim.shape, bool) if strict else ~undecidable
            assert np.array_equal(_bits(g[1, ..., :3][emissive & ok]), _bits(np.ones((int((emissive & ok).sum()), 3), f32)))   # an emitter's albedo is (1, 1, 1)
            assert np.array_equal(dn.emitter_mask(g[1], mats)[ok], dn.emitter_mask(ref_g1, mats)[ok])


@pytest.mark.parametrize("builder,levels", [(0, 2), (0, 12), (2, 2), (2, 12), (1, 12), (3, 12)])
def test_guides_of_a_hostile_soup_with_every_builder_and_the_stack_in_scratch(capi, dn, O, soup, builder, levels):
    """3,036 triangles kept in HBM, 50 x 37, frames 0 and 7; the host SAH tree and the device builders' trees (binned SAH, LBVH, PLOC: other
    leaf orders for the record map); with TRG_OPT_STACK_LDS_LEVELS 2 everything but the sentinel of every traversal stack lives in the
    denoiser's own overflow scratch.  Strict: ids and distances bit for bit everywhere -- of exact duplicates the lower original index
    wins.  Shipped: the set rule.  Emissive first hits carry albedo (1, 1, 1) and are what the filter will keep out."""
    scene, b, off, refs = soup
    c = capi.Context(W, H)
    try:
        c.set_option(capi.OPT_GPU_BUILD, builder)
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        assert c.stats().scene_in_lds == 0
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(W, H)))
        c.set_pixel_offsets(off)
        c.set_option(capi.OPT_STACK_LDS_LEVELS, levels)
        _check_soup(capi, dn, c, b, refs)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. tiny images
@pytest.mark.parametrize("force_global", [0, 1])
@pytest.mark.parametrize("size", [(33, 17), (5, 3)], ids=lambda s: "%dx%d" % s)
def test_guides_of_an_image_smaller_than_a_workgroup(capi, dn, O, cornell, size, force_global):
    """The Cornell box at 33 x 17 (561 rays: two full workgroups and 49 rays) and 5 x 3 (15 rays), staged in LDS and kept in HBM."""
    w, h = size
    b = cornell.buffers()
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
        for frame in (0, 7):
            ref, undecidable = _ref_with_margin(O, cornell, b, w, h, frame, off)
            assert undecidable.mean() < 0.05
            _check_both_settings(capi, dn, c, b, frame, ref, undecidable)
        assert c.stats().scene_in_lds == (0 if force_global else 1)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. a grown state
def test_one_state_serves_deep_and_shallow_stacks_and_a_reloaded_scene(capi, dn, O, cornell, soup):
    """One context, one denoise state: the soup with 12 stack levels in LDS (a small overflow scratch), then with 2 (the scratch regrows), then
    the context reloaded with the 36-triangle Cornell box (the record map shrinks inside its allocation and is rebuilt) -- every result is
    still the oracle's."""
    scene, b, off, refs = soup
    c = capi.Context(W, H)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(W, H)))
        c.set_pixel_offsets(off)
        for levels in (12, 2):
            c.set_option(capi.OPT_STACK_LDS_LEVELS, levels)
            _check_soup(capi, dn, c, b, refs, frames=(0,))
        cb = cornell.buffers()
        c.load_scene(cb["positions"], cb["normals"], cb["colors"], cb["indices"], cb["material_ids"])
        assert c.stats().scene_in_lds == 1
        ref, undecidable = _ref_with_margin(O, cornell, cb, W, H, 0, off)
        assert undecidable.mean() < 0.05
        _check_both_settings(capi, dn, c, cb, 0, ref, undecidable)
        c.set_option(capi.OPT_FORCE_GLOBAL, 1)
        _check_both_settings(capi, dn, c, cb, 0, ref, undecidable)
    finally:
        _close(c, dn)
