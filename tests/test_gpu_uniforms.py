"""The render path under cameras and lights other than the default (-m gpu): the table of tests/util.py (CAMERAS x LIGHTS; what the cases are
for and that they deliver it is checked on the CPU in tests/test_uniforms_host.py) through every schedule of the megakernel and through the
stage-level entry points, against the CPU oracle.

Bars as in tests/test_gpu_parity.py: the strict build bit for bit against the oracle in its portable-trig mode, with the four ray counters;
the shipped build against the libm oracle with RMSE <= TOL_RMSE and no more outlier pixels than tests/util.py edge_flip_allowance gives the
image's rays.  Shapes: 72 x 40 (9 x 5 whole 8 x 8 tiles) and 33 x 17 (partial tiles both ways); strict runs at 3 spp, 5 bounces.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import CAMERAS, FAST_RUNS, LIGHTS, REDUCED_PAIRS, UNIFORM_SHAPES, box_zoo, fast_bar, make_ctx, uniform_pairs, uniforms_case

pytestmark = pytest.mark.gpu
SPP, BNC = 3, 5


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counts(st):
    return (st.primary_rays, st.bounce_rays, st.shadow_rays, st.shaded_hits)


def _portable(O, fn):
    O.set_trig_mode(O.TRIG_PORTABLE)
    try:
        return fn()
    finally:
        O.set_trig_mode(O.TRIG_LIBM)


@pytest.fixture(scope="module")
def strict_refs(O, cornell):
    """(w, h, cam, light) -> (image, stats): the portable-trig oracle at SPP x BNC, every pair at both shapes, rendered once."""
    def run():
        return {(w, h, cam, light): O.render(cornell, w, h, SPP, BNC, offsets=O.pixel_offsets(w, h), uniforms=uniforms_case(O, w, h, cam, light))
                for (w, h) in UNIFORM_SHAPES for cam, light in uniform_pairs()}
    return _portable(O, run)


def _strict_ctx(capi, O, scene, w, h, **options):
    c = make_ctx(O, scene, w, h, offsets=O.pixel_offsets(w, h))
    c.set_option(capi.OPT_STRICT, 1)
    for k, v in options.items():
        c.set_option(getattr(capi, "OPT_" + k), v)
    return c


def _check_pairs(c, O, refs, w, h, pairs, tag, expect=None):
    """Every pair on context c: the accumulation buffer and the four ray counters equal the oracle's; `expect`: fields of the stats that say
    which schedule really ran."""
    for cam, light in pairs:
        ref, rst = refs[(w, h, cam, light)]
        c.set_uniforms(O.uniforms_bytes(uniforms_case(O, w, h, cam, light)))
        c.reset_stats()
        c.render(0, SPP, BNC)
        img, st = c.read_accum(), c.stats()
        assert np.array_equal(_bits(img), _bits(ref)), (tag, w, h, cam, light, int((_bits(img) != _bits(ref)).any(-1).sum()))
        assert _counts(st) == _counts(rst), (tag, w, h, cam, light, _counts(st), _counts(rst))
        for k, v in (expect or {}).items():
            assert getattr(st, k) == v, (tag, w, h, cam, light, k, getattr(st, k))


# ------------------------------------------------------------------ strict, every pair
@pytest.mark.parametrize("force_global", [0, 1])
@pytest.mark.parametrize("w,h", UNIFORM_SHAPES)
def test_strict_every_pair(capi, O, cornell, strict_refs, w, h, force_global):
    """All 7 x 5 pairs on the default schedule, scene in LDS and in HBM."""
    c = _strict_ctx(capi, O, cornell, w, h, FORCE_GLOBAL=force_global)
    try:
        _check_pairs(c, O, strict_refs, w, h, uniform_pairs(), "default schedule", {"scene_in_lds": 0 if force_global else 1})
    finally:
        c.close()


# ------------------------------------------------------------------ strict, every schedule
SCHEDULES = {
    "lds_fp1": dict(FRAME_SPLIT=1, TAIL_BOUNCE=0), "lds_fp2": dict(FRAME_SPLIT=2), "lds_fp4": dict(FRAME_SPLIT=4),
    "hbm_fp1": dict(FORCE_GLOBAL=1, FRAME_SPLIT=1, REGEN=0), "hbm_fp2": dict(FORCE_GLOBAL=1, FRAME_SPLIT=2, REGEN=0),
    "hbm_fp4": dict(FORCE_GLOBAL=1, FRAME_SPLIT=4, REGEN=0),
    "tail1": dict(FRAME_SPLIT=1, TAIL_BOUNCE=1, TAIL_LEVELS=0), "tail1_once": dict(FRAME_SPLIT=1, TAIL_BOUNCE=1, TAIL_LEVELS=1),
    "tail2": dict(FRAME_SPLIT=1, TAIL_BOUNCE=2, TAIL_LEVELS=0), "tail2_once": dict(FRAME_SPLIT=1, TAIL_BOUNCE=2, TAIL_LEVELS=1),
    "hbm_regen": dict(FORCE_GLOBAL=1, FRAME_SPLIT=1, REGEN=1),
}
EXPECT = {
    "lds_fp1": dict(scene_in_lds=1, last_frame_split=1, last_tail_bounce=0), "lds_fp2": dict(scene_in_lds=1, last_frame_split=2),
    "lds_fp4": dict(scene_in_lds=1, last_frame_split=4),
    "hbm_fp1": dict(scene_in_lds=0, last_frame_split=1, last_regen=0), "hbm_fp2": dict(scene_in_lds=0, last_frame_split=2, last_regen=0),
    "hbm_fp4": dict(scene_in_lds=0, last_frame_split=4, last_regen=0),
    "tail1": dict(scene_in_lds=1, last_tail_bounce=1), "tail1_once": dict(scene_in_lds=1, last_tail_bounce=1),
    "tail2": dict(scene_in_lds=1, last_tail_bounce=2), "tail2_once": dict(scene_in_lds=1, last_tail_bounce=2),
    "hbm_regen": dict(scene_in_lds=0, last_regen=1),
}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_strict_every_schedule(capi, O, cornell, strict_refs, schedule):
    """Frame lanes 1 / 2 / 4 in LDS and in HBM, tail compaction from bounce 1 and 2 with and without re-compaction, HBM lock step and path
    regeneration: each fetches the uniform block its own way (TRG_U, TRG_RG_U, the tail's kernarg-segment pointer)."""
    for (w, h) in UNIFORM_SHAPES:
        c = _strict_ctx(capi, O, cornell, w, h, **SCHEDULES[schedule])
        try:
            _check_pairs(c, O, strict_refs, w, h, REDUCED_PAIRS, schedule, EXPECT[schedule])
        finally:
            c.close()


@pytest.mark.parametrize("builder", [1, 2, 3])
def test_strict_device_built_trees(capi, O, cornell, strict_refs, builder):
    b = cornell.buffers()
    for (w, h) in UNIFORM_SHAPES:
        c = capi.Context(w, h)
        try:
            c.set_option(capi.OPT_GPU_BUILD, builder)
            c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            c.set_pixel_offsets(O.pixel_offsets(w, h))
            c.set_option(capi.OPT_STRICT, 1)
            _check_pairs(c, O, strict_refs, w, h, REDUCED_PAIRS, "builder %d" % builder, {"gpu_built": 1, "scene_in_lds": 0})
        finally:
            c.close()


def test_strict_every_kernel_of_the_loaded_library(capi, O, cornell, strict_refs):
    """TRG_KERNEL_DIRECT in the product library; the pool and wavefront schedules too when the experiments library is loaded."""
    for (w, h) in UNIFORM_SHAPES:
        for kernel in ([0, 1, 2] if capi.has_experiments() else [0]):
            for force_global in (0, 1):
                c = _strict_ctx(capi, O, cornell, w, h, KERNEL=kernel, FORCE_GLOBAL=force_global)
                try:
                    _check_pairs(c, O, strict_refs, w, h, REDUCED_PAIRS, "kernel %d" % kernel, {"last_kernel": 0} if kernel == 0 else None)
                finally:
                    c.close()


@pytest.mark.parametrize("schedule", ["lds_fp1", "tail2", "hbm_fp1", "hbm_regen"])
def test_strict_interleaved_bands_of_three_ranks(capi, O, cornell, strict_refs, schedule):
    """trg_render_bands for ranks 0..2 into a compact buffer, trg_unpack_bands: the oracle's frame and the oracle's ray counts."""
    import torch
    n = 3
    for (w, h) in UNIFORM_SHAPES:
        _, stride = capi.microband_rows(h, n, 0)
        c = _strict_ctx(capi, O, cornell, w, h, **SCHEDULES[schedule])
        try:
            compact = torch.zeros((n * stride, w, 4), dtype=torch.float32, device="cuda")
            image = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
            c.bind_accum(compact.data_ptr())
            for cam, light in REDUCED_PAIRS:
                ref, rst = strict_refs[(w, h, cam, light)]
                c.set_uniforms(O.uniforms_bytes(uniforms_case(O, w, h, cam, light)))
                c.reset_stats()
                for r in range(n):
                    c.render_bands(0, SPP, BNC, n, r, r * stride)
                c.unpack_bands(compact.data_ptr(), image.data_ptr(), n)
                c.sync()
                assert np.array_equal(_bits(image.cpu().numpy()), _bits(ref)), (schedule, w, h, cam, light)
                assert _counts(c.stats()) == _counts(rst), (schedule, w, h, cam, light)
            c.bind_accum(None)
        finally:
            c.close()


@pytest.mark.parametrize("force_global", [0, 1])
def test_strict_group_of_two_contexts(capi, O, cornell, strict_refs, force_global, monkeypatch):
    """trg_group_set_uniforms hands the block to every rank: two contexts on one device, each rendering its band, gathered to both."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")
    b = cornell.buffers()
    for (w, h) in UNIFORM_SHAPES:
        g = capi.Group([0, 0], w, h)
        try:
            g.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            g.set_pixel_offsets_seed()
            g.set_option(capi.OPT_STRICT, 1)
            g.set_option(capi.OPT_FORCE_GLOBAL, force_global)
            for cam, light in REDUCED_PAIRS:
                ref, rst = strict_refs[(w, h, cam, light)]
                g.set_uniforms(O.uniforms_bytes(uniforms_case(O, w, h, cam, light)))
                g.reset_stats()
                g.render(0, SPP, BNC, gather=capi.GATHER_ALL)
                g.sync()
                assert _counts(g.stats()) == _counts(rst), (w, h, cam, light)
                for r in range(2):
                    assert np.array_equal(_bits(g.read_accum(r)), _bits(ref)), (w, h, cam, light, r)
        finally:
            g.close()


def test_strict_box_zoo_from_a_foreign_viewpoint(capi, O):
    """Box leaves (tests/util.py box_zoo: rotated, sheared, mirrored, nested cubes) seen from inside_low under tilted_coloured."""
    scene, n_boxes = box_zoo(O)
    for (w, h) in UNIFORM_SHAPES:
        u = uniforms_case(O, w, h, "inside_low", "tilted_coloured")
        off = O.pixel_offsets(w, h)
        ref, rst = _portable(O, lambda: O.render(scene, w, h, SPP, BNC, offsets=off, uniforms=u))
        c = make_ctx(O, scene, w, h, offsets=off, uniforms=u)
        try:
            c.set_option(capi.OPT_STRICT, 1)
            for force_global in (0, 1):
                c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
                c.reset_stats()
                c.render(0, SPP, BNC)
                st = c.stats()
                assert np.array_equal(_bits(c.read_accum()), _bits(ref)) and _counts(st) == _counts(rst), (w, h, force_global)
                assert st.bvh_boxes == n_boxes and st.scene_in_lds == 1 - force_global
        finally:
            c.close()


# ------------------------------------------------------------------ uniforms changed between launches
@pytest.mark.parametrize("schedule", ["lds_fp1", "tail2", "hbm_fp1", "hbm_regen"])
def test_uniforms_changed_between_launches(capi, O, cornell, schedule):
    """One context, frames [0, 2) under pair A, [2, 5) under pair B, [5, 7) under A again: the accumulation continued across launches
    equals the oracle doing the same, bit for bit -- synchronously, and with TRG_OPT_TIMING 0 and nothing between trg_set_uniforms and the
    next trg_render (the block travels with the launch, so an enqueued launch keeps the one it was given)."""
    a, b = ("inside_low", "tilted_coloured"), ("outside_back", "sideways")
    steps = ((a, 0, 2), (b, 2, 3), (a, 5, 2))
    for (w, h) in UNIFORM_SHAPES:
        off = O.pixel_offsets(w, h)

        def oracle():
            acc, counts = np.zeros((h, w, 4), np.float32), np.zeros(4, np.int64)
            for pair, f0, n in steps:
                _, st = O.render(cornell, w, h, n, BNC, frame_begin=f0, accum=acc, offsets=off, uniforms=uniforms_case(O, w, h, *pair))
                counts += _counts(st)
            return acc, tuple(int(v) for v in counts)
        ref, rcounts = _portable(O, oracle)
        c = _strict_ctx(capi, O, cornell, w, h, **SCHEDULES[schedule])
        try:
            for timing in (1, 0):
                c.set_option(capi.OPT_TIMING, timing)
                c.reset_stats()
                for pair, f0, n in steps:
                    c.set_uniforms(O.uniforms_bytes(uniforms_case(O, w, h, *pair)))
                    c.render(f0, n, BNC)
                c.sync()
                st = c.stats()
                assert np.array_equal(_bits(c.read_accum()), _bits(ref)), (schedule, w, h, timing)
                assert _counts(st) == rcounts, (schedule, w, h, timing)
                for k, v in EXPECT[schedule].items():
                    assert getattr(st, k) == v, (schedule, k)
        finally:
            c.close()


# ------------------------------------------------------------------ the shipped build
@pytest.mark.parametrize("schedule", ["default", "hbm_regen"])
@pytest.mark.parametrize("w,h", UNIFORM_SHAPES)
def test_fast_build_every_pair(capi, O, cornell, w, h, schedule):
    """The shipped build (FMA contraction, v_rcp / v_rsq / v_sin / v_cos) on every pair against the libm oracle, runs of FAST_RUNS: RMSE and
    outlier pixels inside the project's small-image bar, the ray total within 1e-4.  Every pair's figures are printed; all pairs are run
    before the first failure is raised."""
    spp, bnc = FAST_RUNS[(w, h)]
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    failed = []
    try:
        if schedule == "hbm_regen":
            c.set_option(capi.OPT_FORCE_GLOBAL, 1)
            c.set_option(capi.OPT_REGEN, 1)
        for cam, light in uniform_pairs():
            u = uniforms_case(O, w, h, cam, light)
            ref, rst = O.render(cornell, w, h, spp, bnc, offsets=off, uniforms=u)
            c.set_uniforms(O.uniforms_bytes(u))
            c.reset_stats()
            c.render(0, spp, bnc)
            img, st = c.read_accum(), c.stats()
            ok, rmse, outliers, allowed = fast_bar(img, ref, rst.rays)
            rays_ok = abs(st.rays - rst.rays) <= 1e-4 * rst.rays
            print("fast %-9s %dx%d %-12s x %-15s rmse %.3e  outliers %d (allowed %d)  rays %d / %d%s"
                  % (schedule, w, h, cam, light, rmse, outliers, allowed, st.rays, rst.rays, "" if ok and rays_ok else "   <-- FAILS"))
            assert np.isfinite(img).all() and (img[..., 3] == 1.0).all()
            if not (ok and rays_ok):
                failed.append((cam, light, rmse, outliers, allowed, st.rays, rst.rays))
            if schedule == "hbm_regen":
                assert st.last_regen == 1 and st.scene_in_lds == 0
    finally:
        c.close()
    assert not failed, failed


# ------------------------------------------------------------------ trg_raygen
@pytest.mark.parametrize("w,h", UNIFORM_SHAPES)
def test_raygen_every_camera(capi, O, cornell, w, h):
    """Every pixel, every camera, frames 0 and 2^32 - 1 (offset + frameIndex wraps): strict byte for byte; shipped build directions to 3e-7,
    origins exact."""
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        for cam in CAMERAS:
            for f in (0, 2 ** 32 - 1):
                u = uniforms_case(O, w, h, cam, "tilted_coloured", f)
                ref = O.raygen(w, h, f, offsets=off, uniforms=u)
                c.set_uniforms(O.uniforms_bytes(u))
                c.set_option(capi.OPT_STRICT, 1)
                got = c.raygen(f)
                assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (cam, f)
                c.set_option(capi.OPT_STRICT, 0)
                got = c.raygen(f)
                np.testing.assert_allclose(got["direction"], ref["direction"], rtol=0, atol=3e-7, err_msg="%s %d" % (cam, f))
                assert np.array_equal(got["origin"], ref["origin"]) and (got["mask"] == 3).all() and np.isinf(got["maxDistance"]).all()
                assert np.array_equal(got["color"], ref["color"])
    finally:
        c.close()


# ------------------------------------------------------------------ trg_sample
K_AXIS = np.array([0.0072, 1.0, 0.0034], np.float32)       # align_hemisphere's helper axis
ROW_CLASSES = ("random", "at", "near", "axis")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def sample_inputs(light_fields, seed):
    """(p, n, r4, row class) for one light: 4,096 random points in and around the room with random unit normals, and planted rows --
    p at the sampled point, at 1e-4 and at 2e-3 from it (either side of the 1e-3 clamp on the distance), p behind the light, n facing away
    from it, n within 1e-5 .. 1e-3 of +-the helper axis of align_hemisphere (never ON it: there the frame is 0 / 0)."""
    rng = np.random.default_rng(seed)
    lp, lf, lr, lu, _ = (np.asarray(v, np.float32).astype(np.float64) for v in light_fields)
    n_rand, n_plant = 4096, 8
    p = rng.uniform((-1.5, -0.5, -1.5), (1.5, 2.5, 3.5), (n_rand, 3))
    n = _unit(rng.normal(size=(n_rand, 3)))
    kind = ["random"] * n_rand
    r4 = rng.random((n_rand + 8 * n_plant, 4)).astype(np.float32)
    one = 1.0 - 2.0 ** -24                                                          # the largest fp32 below 1: Halton numbers are in [0, 1)
    r4[n_rand:n_rand + 4] = [[0, 0, 0, 0], [one, one, one, one], [0.5, 0.5, 0.25, one], [0.5, 0.5, 0.75, 0.0]]      # (corners of the random square)
    rp = r4[n_rand:].astype(np.float64)
    sp = lp + lr * (rp[:, :1] * 2.0 - 1.0) + lu * (rp[:, 1:2] * 2.0 - 1.0)        # the sampled points of the planted rows
    P, N = [], []
    for j, (dist, cls) in enumerate(((0.0, "at"), (1e-4, "near"), (2e-3, "near"))):
        s = sp[j * n_plant:(j + 1) * n_plant]
        P.append(s + dist * _unit(rng.normal(size=s.shape))); N.append(_unit(rng.normal(size=s.shape))); kind += [cls] * n_plant
    s = sp[3 * n_plant:4 * n_plant]                                                 # behind the light: -d . forward <= 0
    P.append(s - _unit(lf) * rng.uniform(0.2, 0.9, (n_plant, 1)) + rng.normal(0, 0.03, s.shape)); N.append(_unit(rng.normal(size=s.shape)))
    kind += ["random"] * n_plant
    s = sp[4 * n_plant:5 * n_plant]                                                 # n facing away from the light
    q = s + _unit(lf) * rng.uniform(0.3, 1.2, (n_plant, 1)) + rng.normal(0, 0.2, s.shape)
    P.append(q); N.append(_unit(-(s - q) + rng.normal(0, 0.05, s.shape))); kind += ["random"] * n_plant
    k = _unit(K_AXIS.astype(np.float64))
    for j, sign in enumerate((1.0, -1.0, 1.0)):                                     # n near +-the helper axis
        P.append(rng.uniform((-0.9, 0.1, -0.9), (0.9, 1.9, 0.9), (n_plant, 3)))
        off = _unit(np.cross(rng.normal(size=(n_plant, 3)), k)) * 10.0 ** rng.uniform(-5, -3, (n_plant, 1))      # at right angles to the axis
        N.append(_unit(sign * k + off)); kind += ["axis"] * n_plant
    p, n = np.concatenate([p] + P).astype(np.float32), np.concatenate([n] + N).astype(np.float32)
    assert p.shape == n.shape == (r4.shape[0], 3)
    ang = np.linalg.norm(np.cross(_unit(n.astype(np.float64)), k), axis=1)      # sine of the angle to the axis
    kind = np.array(kind)
    kind[(ang < 1e-3) & (kind == "random")] = "axis"        # (a random normal that close to the axis: one in a million)
    assert (ang[kind == "axis"] < 1.1e-3).all() and (ang[kind == "axis"] > 5e-6).all()
    return p, n, r4, kind


def sample_f64(light_fields, p, n, r4):
    """sample_area_light, sample_cosine_hemisphere and align_hemisphere (the shaders' common.h) restated in float64 on the fp32 inputs and
    the fp32 constants: (light dir, light dist, light colour, colour magnitude before the two cosines, bounce dir)."""
    lp, lf, lr, lu, lc = (np.asarray(v, np.float32).astype(np.float64) for v in light_fields)
    p, n, r = p.astype(np.float64), n.astype(np.float64), r4.astype(np.float64)
    sp = lp + lr * (r[:, :1] * 2.0 - 1.0) + lu * (r[:, 1:2] * 2.0 - 1.0)
    d = sp - p
    dist = np.sqrt((d * d).sum(1))
    inv = 1.0 / np.maximum(dist, float(np.float32(1e-3)))
    d = d * inv[:, None]
    k1 = np.clip((-d * lf).sum(1), 0.0, 1.0)
    k2 = np.clip((n * d).sum(1), 0.0, 1.0)
    scale = np.abs(lc).max() * inv * inv
    col = lc * (inv * inv * k1 * k2)[:, None]
    phi = 2.0 * float(np.float32(3.1415926535898)) * r[:, 2]
    ct = np.sqrt(r[:, 3])
    st = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
    s = np.stack([st * np.cos(phi), ct, st * np.sin(phi)], 1)
    right = _unit(np.cross(n, K_AXIS.astype(np.float64)))
    fwd = np.cross(right, n)
    return d, dist, col, scale, s[:, :1] * right + s[:, 1:2] * n + s[:, 2:3] * fwd


def sample_errors(out12, f64, kind):
    """Per row class, the worst error of an fp32 result [n, 12] (trg_sample's layout) against the float64 restatement, per output group:
      dir     light direction, absolute (the direction is a unit vector, shorter inside the clamp);
      dist    light distance, relative to the distance;
      colour  light colour relative to its own magnitude -- floored at 1e-4 of the magnitude it has before the two cosines: below that the
              cosines (differences of products of numbers near 1) are beyond what fp32's 6e-8 can hold to any relative precision;
      bounce  bounce direction, absolute."""
    d, dist, col, scale, bd = f64
    o = out12.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = {"dir": np.abs(o[:, 0:3] - d).max(1),
             "dist": np.where(dist > 0, np.abs(o[:, 3] - dist) / dist, np.abs(o[:, 3])),
             "colour": np.abs(o[:, 4:7] - col).max(1) / np.maximum(np.abs(col).max(1), 1e-4 * scale),
             "bounce": np.abs(o[:, 8:11] - bd).max(1)}
    return {(cls, g): float(v[kind == cls].max()) for cls in ROW_CLASSES for g, v in e.items()}


def oracle_sample(O, u, p, n, r4):
    """orc_sample_area_light and orc_sample_cosine_hemisphere + orc_align_hemisphere row by row, in trg_sample's layout."""
    L = O.lib()
    vp = C.c_void_p
    area = C.CFUNCTYPE(None, vp, vp, vp, vp, vp, vp, vp)(("orc_sample_area_light", L))
    hemi = C.CFUNCTYPE(None, vp, vp)(("orc_sample_cosine_hemisphere", L))
    align = C.CFUNCTYPE(None, vp, vp, vp)(("orc_align_hemisphere", L))
    out = np.zeros((p.shape[0], 12), np.float32)
    h = np.zeros(3, np.float32)
    up, pp, pn, pr, po, ph = C.addressof(u), p.ctypes.data, n.ctypes.data, r4.ctypes.data, out.ctypes.data, h.ctypes.data
    for k in range(p.shape[0]):
        o = po + 48 * k
        area(up, pr + 16 * k, pp + 12 * k, pn + 12 * k, o, o + 16, o + 12)
        hemi(pr + 16 * k + 8, ph)
        align(ph, pn + 12 * k, o + 32)
    return out


@pytest.mark.parametrize("light", list(LIGHTS))
def test_sample_every_light(capi, O, cornell, light):
    """trg_sample under every light of the table, 4,096 random rows plus the planted ones of sample_inputs.

    Strict build: the oracle's bits (portable trig for the bounce direction).  Shipped build: judged against the ORACLE, by errors against a
    float64 restatement of the formulas: the oracle's own fp32 error is measured on these same inputs, per row class and per output group
    (sample_errors), floored at half an ulp (2^-24), and the shipped build may have 4 x that -- its chain has at most four approximate
    operations (v_rsq, v_rcp, v_sqrt, v_sin / v_cos) of about an ulp each where the oracle has correctly rounded ones.

    The oracle's envelopes (libm trig) measured on these inputs, worst over the five lights, and the shipped build's errors on an MI355X:
      random rows                                   dir 3.3e-7 (shipped 5.7e-7), dist 6.5e-7 (3.3e-7), colour 8.1e-5 (1.4e-4), bounce 1.7e-6 (1.1e-6)
      p at the sampled point (dist < 1e-6)          dir 6.0e-5 (6.0e-5), dist 1.7 (1.7: a distance of 1e-8 is rounding noise on both sides),
                                                    colour 9.2e-6 (9.3e-6), bounce 1.0e-4 (the rows with r3 one ulp below 1)
      p at 1e-4 / 2e-3 from it                      dir 5.4e-5 (5.4e-5), dist 4.3e-4 (4.3e-4), colour 2.5e-3 (2.5e-3), bounce 3.0e-7 (1.9e-7)
      n within 1e-3 of the helper axis              dir 1.6e-7 (1.1e-7), dist 1.1e-7 (1.3e-7), colour 6.9e-5 (8.0e-5), bounce 9.8e-6 (6.1e-7)
    (near the sampled point the difference sp - p cancels: what is left of the fp32 rounding of sp is 1e-7 of a length of 1e-4.)"""
    u = uniforms_case(O, 72, 40, "default", light)
    fields = [list(getattr(u, f))[0:3] for f in ("light_pos", "light_forward", "light_right", "light_up", "light_color")]
    p, n, r4, kind = sample_inputs(fields, 40 + list(LIGHTS).index(light))
    f64 = sample_f64(fields, p, n, r4)
    ref_libm = oracle_sample(O, u, p, n, r4)
    ref_portable = _portable(O, lambda: oracle_sample(O, u, p, n, r4))
    assert np.isfinite(ref_libm).all() and np.isfinite(ref_portable).all()
    # the planted rows are what they claim to be
    at, near = np.flatnonzero(kind == "at"), np.flatnonzero(kind == "near")
    assert (ref_libm[at, 3] < 1e-6).all() and (ref_libm[near[:8], 3] < 1e-3).all() and (ref_libm[near[8:], 3] > 1e-3).all()
    if light == "point_dim":
        assert (ref_libm[at, 3] == 0).all()           # zero extent: the sampled point is light_pos itself, dist = 0 exactly
    assert (ref_libm[4096 + 24:4096 + 40, 4:7] == 0).all()  # behind the light / facing away: no light
    assert (ref_libm[:4096, 4:7].max(1) > 0).mean() > 0.05
    envelope = sample_errors(ref_libm, f64, kind)
    c = make_ctx(O, cornell, 72, 40, uniforms=u)
    try:
        c.set_option(capi.OPT_STRICT, 1)
        got = c.sample(p, n, r4)
        assert np.array_equal(_bits(got[:, 0:8]), _bits(ref_libm[:, 0:8])), "strict light sample differs from the oracle"
        assert np.array_equal(_bits(got[:, 8:12]), _bits(ref_portable[:, 8:12])), "strict bounce direction differs from the oracle"
        c.set_option(capi.OPT_STRICT, 0)
        fast = c.sample(p, n, r4)
    finally:
        c.close()
    assert np.isfinite(fast).all()
    err = sample_errors(fast, f64, kind)
    bad = []
    for key in sorted(envelope):
        allowed = 4.0 * max(envelope[key], 2.0 ** -24)
        print("sample %-15s %-6s %-6s oracle %.3e  shipped %.3e  allowed %.3e%s"
              % (light, key[0], key[1], envelope[key], err[key], allowed, "" if err[key] <= allowed else "   <-- FAILS"))
        if not err[key] <= allowed:
            bad.append((key, envelope[key], err[key], allowed))
    assert not bad, bad


# ------------------------------------------------------------------ trg_postprocess
def _check_postprocess(c, O, acc):
    for flip in (True, False):
        got, want = c.postprocess(flip_y=flip), O.postprocess(acc, flip_y=flip)
        diff = np.abs(got.astype(int) - want.astype(int))
        assert diff.max() <= 1, (flip, int(diff.max()), np.argwhere(diff > 1)[:5].tolist())
        assert (got[..., 3] == 255).all()


def test_postprocess_bright_and_coloured_frames(capi, O, cornell):
    """Frames with radiance far above 1 (sideways: 1 / d^2 near the light) and with unequal channels (tilted_coloured), 33 x 17, both flips."""
    w, h = 33, 17
    for cam, light, least in (("nearly_up", "sideways", 20.0), ("inside_low", "tilted_coloured", 4.0)):
        c = make_ctx(O, cornell, w, h, offsets=O.pixel_offsets(w, h), uniforms=uniforms_case(O, w, h, cam, light))
        try:
            c.render(0, SPP, BNC)
            acc = c.read_accum()
            assert np.isfinite(acc).all() and acc[..., :3].max() > least, acc[..., :3].max()
            _check_postprocess(c, O, acc)
        finally:
            c.close()


def test_postprocess_synthetic_buffer(capi, O, cornell):
    """A bound buffer of chosen texels: 0, 1e-8, the sRGB knee 0.0031308 +- 1 ulp as a texel and as the tone-mapped value (the texel whose
    ACES value is the knee, +- 1 ulp), 0.5, 1, 5, 67, 1e18, 1e30 (finite, but x * x overflows inside the tone curve: both sides then clamp
    a NaN to 0) and small negatives; a third channel that numbers the pixels, so that a flip or a stride error shows.  Finite texels only:
    the project defines nothing for the others."""
    import torch
    w, h = 33, 17
    knee = np.float32(0.0031308)
    a, b, cc, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
    k = float(knee)                                             # ACES(x) = k  <=>  (a - k c) x^2 + (b - k d) x - k e = 0
    qa, qb, qc = a - k * cc, b - k * d, -k * e
    x_knee = np.float32((-qb + np.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa))
    ulp = lambda v, s: np.nextafter(np.float32(v), np.float32(s * np.inf), dtype=np.float32)
    specials = np.array([0.0, 1e-8, ulp(knee, -1), knee, ulp(knee, 1), ulp(x_knee, -1), x_knee, ulp(x_knee, 1), 0.5, 1.0, 5.0, 67.0, 1e18, 1e30,
                         -1e-8, -1e-3, -0.5, 0.18, 0.01], np.float32)
    assert np.isfinite(specials).all() and 0.002 < x_knee < 0.05
    yy, xx = np.mgrid[0:h, 0:w]
    acc = np.empty((h, w, 4), np.float32)
    acc[..., 0] = specials[(xx + 5 * yy) % len(specials)]
    acc[..., 1] = specials[(2 * xx + yy + 1) % len(specials)]
    acc[..., 2] = (xx + w * yy + 1).astype(np.float32) / np.float32(w * h)       # the pixel's number
    acc[..., 3] = 1.0
    c = make_ctx(O, cornell, w, h)
    try:
        buf = torch.from_numpy(acc).to("cuda")
        c.bind_accum(buf.data_ptr())
        _check_postprocess(c, O, acc)
        want = O.postprocess(acc, flip_y=False)
        # the expected picture tells every row from every other row and every column from every other column: no flip, shift or stride slips by
        assert len({want[y].tobytes() for y in range(h)}) == h and len({want[:, x].tobytes() for x in range(w)}) == w
        assert not np.array_equal(want, O.postprocess(acc, flip_y=True))
        c.bind_accum(None)
    finally:
        c.close()
