"""Every render schedule on scenes whose triangles carry three different normals, colours and texture coordinates (-m gpu), and the LDS tier
up to its edge.  The scenes are those of tests/schedule_scenes.py; tests/test_schedule_scenes_host.py shows on the oracle alone that a kernel
which drops the texture descriptor, ignores the barycentric weights or permutes the corners changes their pictures.

Every case loads scene A with its textures, sets a schedule's options, asserts through trg_get_stats that THIS schedule ran, and is held to
three bars at both shapes of schedule_scenes.SHAPES (48 x 40 at 5 spp and 33 x 17 at 18 spp, 5 bounces: partial 16 x 16 tiles, the second
crossing the 16-frame chunk of the tail and regeneration kernels):
  A  strict build: the accumulation buffer is the portable-trig oracle's bit for bit, and so are the four ray counters;
  B  shipped build: tests/util.py fast_bar against the libm oracle and the ray total within 1e-4 (figures printed);
  C  textures removed (trg_load_textures with no images): the strict image is the UNTEXTURED oracle's bit for bit -- the descriptor is gone in
     that kernel too -- and the shipped build is inside fast_bar on it.
"""
import numpy as np
import pytest

from tests import schedule_scenes as S
from tests.test_gpu_parity import _rays
from tests.test_gpu_uniforms import EXPECT, SCHEDULES
from tests.util import fast_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counts(st):
    return (int(st.primary_rays), int(st.bounce_rays), int(st.shadow_rays), int(st.shaded_hits))


def _set(c, capi, options):
    for k, v in options.items():
        c.set_option(getattr(capi, "OPT_" + k), v)


def _load(c, O, scene, w, h, textured=True):
    b, uvs, ids, imgs = scene
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    if textured:
        c.load_textures(uvs, ids, list(imgs))
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
    c.set_pixel_offsets(O.pixel_offsets(w, h))


# ---- how a case draws its frame: (context, first frame, frames, bounces) -> image
def _draw_plain(c, spp, bnc):
    c.render(0, spp, bnc)
    return c.read_accum()


def _draw_continued(c, spp, bnc):
    """Two launches that continue one accumulation: 7 + 11 of the 18 frames, 2 + 3 of the 5."""
    first = 7 if spp == 18 else 2
    c.render(0, first, bnc)
    c.render(first, spp - first, bnc)
    return c.read_accum()


def _draw_bands(n):
    def draw(c, spp, bnc):
        import torch
        from toyraygun_amd import capi
        _, stride = capi.microband_rows(c.h, n, 0)
        compact = torch.zeros((n * stride, c.w, 4), dtype=torch.float32, device="cuda")
        image = torch.full((c.h, c.w, 4), -1.0, dtype=torch.float32, device="cuda")
        c.bind_accum(compact.data_ptr())
        try:
            for r in range(n):
                c.render_bands(0, spp, bnc, n, r, r * stride)
            c.unpack_bands(compact.data_ptr(), image.data_ptr(), n)
            c.sync()
            return image.cpu().numpy()
        finally:
            c.bind_accum(None)
    return draw


def _strict(c, capi, ref, expect, tag, draw, spp, bnc):
    img_ref, counts, _ = ref
    c.set_option(capi.OPT_STRICT, 1)
    c.reset_stats()
    img = draw(c, spp, bnc)
    st = c.stats()
    assert np.array_equal(_bits(img), _bits(img_ref)), (tag, "pixels that differ: %d of %d" % (int((_bits(img) != _bits(img_ref)).any(-1).sum()), img.shape[0] * img.shape[1]))
    assert _counts(st) == counts, (tag, _counts(st), counts)
    for k, v in expect.items():
        assert getattr(st, k) == v, (tag, k, getattr(st, k), v)
    return img


def _shipped(c, capi, ref, expect, tag, draw, spp, bnc):
    img_ref, _, rays = ref
    c.set_option(capi.OPT_STRICT, 0)
    c.reset_stats()
    img = draw(c, spp, bnc)
    st = c.stats()
    ok, rmse, outliers, allowed = fast_bar(img, img_ref, rays)
    rays_ok = abs(int(st.rays) - rays) <= 1e-4 * rays
    print("shipped %-40s rmse %.3e  outliers %d (allowed %d)  rays %d / %d%s" % (tag, rmse, outliers, allowed, st.rays, rays, "" if ok and rays_ok else "   <-- FAILS"))
    assert np.isfinite(img).all() and (img[..., 3] == 1.0).all(), tag
    assert ok and rays_ok, (tag, rmse, outliers, allowed, int(st.rays), rays)
    for k, v in expect.items():
        assert getattr(st, k) == v, (tag, k, getattr(st, k), v)


def _bars(c, capi, name, shape, expect, tag, draw=_draw_plain, variant="base"):
    """Bars A to C on a context that holds scene `name` with its textures; the textures are loaded again before it returns."""
    w, h, spp, bnc = S.SHAPES[shape]
    tag = "%s %s %dx%d" % (tag, name, w, h)
    _, uvs, ids, imgs = S.scene(name, variant)
    _strict(c, capi, S.reference(name, variant, True, shape, "TRIG_PORTABLE"), expect, tag + " textured", draw, spp, bnc)
    _shipped(c, capi, S.reference(name, variant, True, shape, "TRIG_LIBM"), expect, tag + " textured", draw, spp, bnc)
    c.load_textures(uvs, ids, [])
    _strict(c, capi, S.reference(name, variant, False, shape, "TRIG_PORTABLE"), expect, tag + " textures removed", draw, spp, bnc)
    _shipped(c, capi, S.reference(name, variant, False, shape, "TRIG_LIBM"), expect, tag + " textures removed", draw, spp, bnc)
    c.load_textures(uvs, ids, list(imgs))


# ---------------------------------------------------------------------------------------------------------------------------- the schedules
def _cases():
    """name -> (options, what trg_get_stats must say afterwards, how the frame is drawn)."""
    cases = {k: (SCHEDULES[k], EXPECT[k], _draw_plain) for k in SCHEDULES}
    for sort in (1, 2, 3):
        cases["tail2_sort%d" % sort] = (dict(SCHEDULES["tail2"], TAIL_SORT=sort), EXPECT["tail2"], _draw_plain)
    for lanes in (2, 4):
        cases["hbm_regen_fp%d" % lanes] = (dict(SCHEDULES["hbm_regen"], FRAME_SPLIT=lanes), dict(EXPECT["hbm_regen"], last_frame_split=lanes), _draw_plain)
    cases["hbm_regen_queues66"] = (dict(SCHEDULES["hbm_regen"], TILE_ORDER=66), dict(EXPECT["hbm_regen"], last_tile_order=66), _draw_plain)
    for order in (1, 8, 17, 32):
        cases["lds_fp1_order%d" % order] = (dict(SCHEDULES["lds_fp1"], TILE_ORDER=order), dict(EXPECT["lds_fp1"], last_tile_order=order), _draw_plain)
    cases["hbm_fp1_stack2"] = (dict(SCHEDULES["hbm_fp1"], STACK_LDS_LEVELS=2), EXPECT["hbm_fp1"], _draw_plain)
    for k in ("tail1", "hbm_regen"):
        cases[k + "_continued"] = (SCHEDULES[k], EXPECT[k], _draw_continued)
    for k in ("lds_fp1", "tail2", "hbm_fp1", "hbm_regen"):
        cases[k + "_bands3"] = (SCHEDULES[k], EXPECT[k], _draw_bands(3))
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def torch_cuda():
    """torch with its device runtime up (the band cases bind a torch buffer): brought up once, outside any case's own time."""
    import torch
    torch.zeros(1, device="cuda")
    return torch


@pytest.mark.parametrize("schedule", list(CASES))
def test_every_schedule_on_scene_a(capi, O, torch_cuda, schedule):
    """Frame lanes 1 / 2 / 4 in LDS and in HBM, tail compaction from bounce 1 and 2 with and without re-compaction and with the three sorts,
    HBM lock step with two stack levels in LDS, path regeneration with frame lanes and with per-XCD job queues, the XCD-aware tile orders, an
    accumulation continued across two launches, and three ranks' interleaved bands unpacked into one frame."""
    options, expect, draw = CASES[schedule]
    for shape, (w, h, _, _) in enumerate(S.SHAPES):
        c = capi.Context(w, h)
        try:
            _load(c, O, S.scene("A"), w, h)
            _set(c, capi, options)
            _bars(c, capi, "A", shape, expect, schedule, draw)
        finally:
            c.close()


@pytest.mark.parametrize("options", [dict(FRAME_SPLIT=1, REGEN=0), dict(FRAME_SPLIT=1, REGEN=1), dict(FRAME_SPLIT=2, REGEN=1)], ids=["lock_step", "regen", "regen_fp2"])
def test_scene_b_host_built(capi, O, options):
    """1,878 triangles: in HBM by itself, no TRG_OPT_FORCE_GLOBAL."""
    w, h, _, _ = S.SHAPES[0]
    c = capi.Context(w, h)
    try:
        _load(c, O, S.scene("B"), w, h)
        _set(c, capi, options)
        _bars(c, capi, "B", 0, dict(scene_in_lds=0, gpu_built=0, last_regen=options["REGEN"], last_frame_split=options["FRAME_SPLIT"]), "host-built")
    finally:
        c.close()


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("builder", [1, 2, 3])
def test_device_built_trees(capi, O, builder, name):
    """TRG_OPT_GPU_BUILD 1 / 2 / 3: each builder writes the 128-byte leaf records (geometry, nine normal and nine colour floats) itself.  The
    lock-step kernel and path regeneration on one context."""
    for shape in ((0, 1) if name == "A" else (0,)):
        w, h, _, _ = S.SHAPES[shape]
        c = capi.Context(w, h)
        try:
            c.set_option(capi.OPT_GPU_BUILD, builder)
            _load(c, O, S.scene(name), w, h)
            for regen in (0, 1):
                _set(c, capi, dict(FRAME_SPLIT=1, REGEN=regen))
                _bars(c, capi, name, shape, dict(gpu_built=1, scene_in_lds=0, last_regen=regen), "builder %d regen %d" % (builder, regen))
        finally:
            c.close()


@pytest.mark.parametrize("force_global", [0, 1])
@pytest.mark.parametrize("bands", ["contiguous", "interleaved"])
def test_group_of_two_contexts(capi, O, bands, force_global, monkeypatch):
    """trg_group_load_textures hands the descriptor to every rank: two contexts on one device, each rendering its band (contiguous rows, or
    interleaved 8-row micro-bands through trg_render_bands), gathered to both.  Bars A to C on both ranks' frames."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")
    b, uvs, ids, imgs = S.scene("A")
    for shape, (w, h, spp, bnc) in enumerate(S.SHAPES):
        g = capi.Group([0, 0], w, h)
        try:
            g.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            g.load_textures(uvs, ids, list(imgs))
            g.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
            g.set_pixel_offsets_seed()
            g.set_option(capi.OPT_FORCE_GLOBAL, force_global)
            g.set_bands(capi.BANDS_INTERLEAVED if bands == "interleaved" else capi.BANDS_CONTIGUOUS)
            assert g.n == 2 and g.exchange == capi.EXCHANGE_COPY and g.bands == (capi.BANDS_INTERLEAVED if bands == "interleaved" else capi.BANDS_CONTIGUOUS)
            for textured in (True, False):
                if not textured:
                    g.load_textures(uvs, ids, [])
                for strict in (1, 0):
                    tag = "group %s fg%d %dx%d %s %s" % (bands, force_global, w, h, "textured" if textured else "textures removed", "strict" if strict else "shipped")
                    ref, counts, rays = S.reference("A", "base", textured, shape, "TRIG_PORTABLE" if strict else "TRIG_LIBM")
                    g.set_option(capi.OPT_STRICT, strict)
                    g.reset_stats()
                    g.render(0, spp, bnc, gather=capi.GATHER_ALL)
                    g.sync()
                    st = g.stats()
                    for r in range(2):
                        img = g.read_accum(r)
                        assert g.rank_stats(r).scene_in_lds == 1 - force_global and g.rank_stats(r).rays > 0, (tag, r)
                        if strict:
                            assert np.array_equal(_bits(img), _bits(ref)), (tag, r)
                        else:
                            ok, rmse, outliers, allowed = fast_bar(img, ref, rays)
                            print("shipped %-60s rank %d rmse %.3e  outliers %d (allowed %d)" % (tag, r, rmse, outliers, allowed))
                            assert ok, (tag, r, rmse, outliers, allowed)
                    if strict:
                        assert _counts(st) == counts, (tag, _counts(st), counts)
                    else:
                        assert abs(int(st.rays) - rays) <= 1e-4 * rays, (tag, int(st.rays), rays)
        finally:
            g.close()


# ---------------------------------------------------------------------------------------------------------------------------- corner rotation
ROTATION_FAMILIES = {"lds_fp1": (0, "lds_fp1"), "lds_fp4": (0, "lds_fp4"), "tail1": (0, "tail1"), "hbm_fp1": (0, "hbm_fp1"), "hbm_regen": (0, "hbm_regen"),
                     "builder2": (2, None)}


@pytest.mark.parametrize("family", list(ROTATION_FAMILIES))
def test_rotated_corners_per_kernel_family(capi, O, family):
    """The mesh corners' normals, colours and uv moved on by one corner, the positions left alone: every kernel family draws the oracle's image of
    THAT scene bit for bit -- which is not the image of scene A -- so no family reads a leaf record's corners, or the weights, in another order."""
    builder, schedule = ROTATION_FAMILIES[family]
    options = SCHEDULES[schedule] if schedule else dict(FRAME_SPLIT=1, REGEN=0)
    expect = EXPECT[schedule] if schedule else dict(gpu_built=1, scene_in_lds=0)
    for shape, (w, h, spp, bnc) in enumerate(S.SHAPES):
        c = capi.Context(w, h)
        try:
            c.set_option(capi.OPT_GPU_BUILD, builder)
            _load(c, O, S.scene("A", "rotated"), w, h)
            _set(c, capi, options)
            for textured in (True, False):
                if not textured:
                    c.load_textures(S.scene("A", "rotated")[1], S.scene("A", "rotated")[2], [])
                img = _strict(c, capi, S.reference("A", "rotated", textured, shape, "TRIG_PORTABLE"), expect, "%s rotated %dx%d textured %d" % (family, w, h, textured),
                              _draw_plain, spp, bnc)
                assert S.differ(img, S.reference("A", "base", textured, shape, "TRIG_PORTABLE")[0]).mean() >= 0.01
        finally:
            c.close()


# ---------------------------------------------------------------------------------------------------------------------------- the LDS tier's edge
EDGE_SLOTS = ("resident_4th_largest", "resident_3rd_largest", "resident_2nd_largest", "resident_largest", "first_not_resident")


@pytest.fixture(scope="module")
def lds_edge(capi, O):
    """n -> (scene_in_lds, lds_bytes) for every member of the edge family, as trg_get_stats reports it after trg_load_scene."""
    w, h, _, _ = S.EDGE_SHAPE
    c = capi.Context(w, h)
    out = {}
    try:
        for n in S.EDGE_N:
            b = S.edge_scene(n)[0]
            c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            st = c.stats()
            out[n] = (int(st.scene_in_lds), int(st.lds_bytes))
    finally:
        c.close()
    return out


def _edge_n(lds_edge, slot):
    resident = sorted(n for n, (r, _) in lds_edge.items() if r)
    away = sorted(n for n, (r, _) in lds_edge.items() if not r)
    assert len(resident) >= 4 and away, (resident, away)
    return away[0] if slot == "first_not_resident" else resident[-4 + EDGE_SLOTS.index(slot)]


def test_lds_tier_has_an_edge_inside_the_family(lds_edge):
    resident = sorted(n for n, (r, _) in lds_edge.items() if r)
    away = sorted(n for n, (r, _) in lds_edge.items() if not r)
    assert resident and away
    assert all(lds_edge[n][1] <= 65536 for n in resident)
    top = resident[-1]
    print("LDS tier: largest resident scene of the family has %d triangles, lds_bytes %d; resident sizes %d..%d (%d of them), first not resident %d"
          % (top, lds_edge[top][1], resident[0], top, len(resident), away[0]))
    print("the sizes tested: " + ", ".join("%s = %d (lds_bytes %d)" % (s, _edge_n(lds_edge, s), lds_edge[_edge_n(lds_edge, s)][1]) for s in EDGE_SLOTS))


def _trace_bar(c, capi, O, s, seed):
    """Strict trg_trace of 5,000 random rays: the brute-force oracle's records byte for byte, the any-hit answers identical."""
    rays = _rays(O, 5000, seed)
    ref, ref_any = O.intersect_nearest(s, rays, brute=True), O.intersect_any(s, rays, brute=True)
    assert (ref["primitiveIndex"] >= 36).mean() > 0.05             # (the rays meet the added triangles, not the room alone)
    c.set_option(capi.OPT_STRICT, 1)
    got = c.trace(rays)
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "records that differ: %d" % int((got != ref).sum())
    assert np.array_equal(c.trace(rays, any_hit=True) >= 0, ref_any >= 0)


def _render_bars(c, capi, refs, schedules, tag):
    w, h, spp, bnc = S.EDGE_SHAPE
    for name, options, expect in schedules:
        _set(c, capi, options)
        _strict(c, capi, refs("TRIG_PORTABLE"), expect, "%s %s" % (tag, name), _draw_plain, spp, bnc)
        _shipped(c, capi, refs("TRIG_LIBM"), expect, "%s %s" % (tag, name), _draw_plain, spp, bnc)


@pytest.mark.parametrize("slot", EDGE_SLOTS)
def test_lds_tier_at_its_edge(capi, O, lds_edge, slot):
    """The four largest scenes of the family that are staged in LDS and the smallest that is not: consecutive sizes move the staged byte count by
    126 per triangle plus whole 208-byte nodes, so the Halton tables behind the attributes and the stacks behind the staged bytes fall on
    different alignments.  Intersector and whole path, every corner with its own normal and colour, every third triangle textured."""
    n = _edge_n(lds_edge, slot)
    resident = lds_edge[n][0]
    assert resident == (0 if slot == "first_not_resident" else 1)
    scene = S.edge_scene(n)
    w, h, _, _ = S.EDGE_SHAPE
    c = capi.Context(w, h)
    try:
        _load(c, O, scene, w, h)
        st = c.stats()
        assert (int(st.scene_in_lds), int(st.lds_bytes)) == lds_edge[n]
        _trace_bar(c, capi, O, S.oracle_scene(O, scene[0]), 700 + n)
        if resident:
            schedules = (("frame-serial", dict(FRAME_SPLIT=1, TAIL_BOUNCE=0), dict(scene_in_lds=1, last_frame_split=1, last_tail_bounce=0)),
                         ("frame lanes 4", dict(FRAME_SPLIT=4, TAIL_BOUNCE=0), dict(scene_in_lds=1, last_frame_split=4)),
                         ("tail from bounce 1", dict(FRAME_SPLIT=1, TAIL_BOUNCE=1), dict(scene_in_lds=1, last_tail_bounce=1)))
        else:
            schedules = (("hbm_fp1", SCHEDULES["hbm_fp1"], EXPECT["hbm_fp1"]),)
        _render_bars(c, capi, lambda trig: S.edge_reference(n, trig), schedules, "edge %s n=%d" % (slot, n))
    finally:
        c.close()


def test_small_scene_with_a_deep_tree_stays_in_hbm(capi, O):
    """plan_lds, second branch: tests/schedule_scenes.py deep_scene has fewer than 40 KiB to stage, but its host tree is so deep that the staged
    bytes and the traversal stacks together pass 64 KiB (tests/test_schedule_scenes_host.py).  It is rendered from HBM without
    TRG_OPT_FORCE_GLOBAL; tail compaction, which needs the scene in LDS, gives way to the lock-step kernel."""
    b = S.deep_scene()
    nt = b["material_ids"].shape[0]
    scene = (b,) + S.random_textures(nt, 4)
    w, h, _, _ = S.EDGE_SHAPE
    c = capi.Context(w, h)
    try:
        _load(c, O, scene, w, h)
        st = c.stats()
        print("deep scene: %d triangles, bvh_depth %d, bvh_nodes %d, scene_in_lds %d, lds_bytes %d" % (nt, st.bvh_depth, st.bvh_nodes, st.scene_in_lds, st.lds_bytes))
        assert st.scene_in_lds == 0 and st.lds_bytes <= 65536 and st.gpu_built == 0
        # half of the rays at random, half aimed at the fan's triangles, the small ones at the bottom of the tree as often as the large ones
        rays = np.concatenate([_rays(O, 2500, 99, lo=(-0.5, -0.2, -0.5), hi=(1.6, 1.6, 2.5)), S.aimed_rays(O, b, np.arange(4, nt), 2500, 98)])
        s = S.oracle_scene(O, b)
        ref, ref_any = O.intersect_nearest(s, rays, brute=True), O.intersect_any(s, rays, brute=True)
        assert (ref["primitiveIndex"] >= 4).mean() > 0.2 and len(np.unique(ref["primitiveIndex"])) > 30
        c.set_option(capi.OPT_STRICT, 1)
        got = c.trace(rays)
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "records that differ: %d" % int((got != ref).sum())
        assert np.array_equal(c.trace(rays, any_hit=True) >= 0, ref_any >= 0)
        schedules = (("frame-serial", dict(FRAME_SPLIT=1, TAIL_BOUNCE=0), dict(scene_in_lds=0, last_frame_split=1, last_tail_bounce=0, last_regen=0)),
                     ("frame lanes 4", dict(FRAME_SPLIT=4, TAIL_BOUNCE=0), dict(last_frame_split=4)),
                     ("tail asked for", dict(FRAME_SPLIT=1, TAIL_BOUNCE=1), dict(scene_in_lds=0, last_frame_split=1, last_tail_bounce=0)))
        _render_bars(c, capi, S.deep_reference, schedules, "deep tree")
    finally:
        c.close()
