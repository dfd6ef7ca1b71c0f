"""GPU tests (-m gpu) of the skin unit (include/trg_skin.h): a loaded scene skinned on the device -- four bones per vertex, blended -- against
skin_reference (bit for bit), against the CPU oracle's render of the read-back geometry (bit for bit in the strict build; inside the shipped build's
bar otherwise), against a fresh trg_load_scene and against trg_pose_apply for one-hot weights.  Images 32 x 24, 2 spp, 3 bounces; traces 4,096
random rays -- the sizes of tests/test_gpu_refit.py, whose bars these are.  The bones keep every box and quad leaf of scene A:
tests/test_skin_host.py checks that on the CPU.  Nothing here provokes a fault: every refusal is decided on the host or from flag words before
anything is written."""
import os
import subprocess

import numpy as np
import pytest

from tests import pose_scenes as PS
from tests import refit_scenes as RS
from tests import skin_scenes as SS
from tests.test_gpu_pose import RAY_HI, RAY_LO, _device_bytes, _fresh_trace_equal
from tests.test_gpu_refit import BOUNCES, H, HBM_KERNELS, SPP, W, _bits, _close, _ctx, _rays, _shipped_bars, _strict_bars, _textures

pytestmark = pytest.mark.gpu
NT = 706


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def refit(built):
    from toyraygun_amd import refit as r
    r.load()
    return r


@pytest.fixture(scope="module")
def skin(built):
    from toyraygun_amd import skin as s
    s.load()
    return s


@pytest.fixture(scope="module")
def pose(built):
    from toyraygun_amd import pose as p
    p.load()
    return p


@pytest.fixture(scope="module")
def dn(built):
    from toyraygun_amd import denoise
    denoise.load()
    return denoise


@pytest.fixture(scope="module")
def rest():
    """Scene A as loaded -- per corner and indexed -- with its binding; shared and left unchanged."""
    a, i = RS.scene_a(0), RS.scene_a_indexed(0)
    return (a, SS.scene_a_binding(a)), (i, SS.scene_a_binding(i))


def _bind(skin, c, b, binding, normals=True, n_bones=SS.N_BONES):
    skin.bind(c, b["positions"], b["normals"] if normals else None, b["indices"], binding[0], binding[1], n_bones)


def _skinned(skin, c, b, binding, bones, normals=True):
    """apply + read, checked against skin_reference bit for bit; returns the buffer dict of the read-back geometry."""
    skin.apply(c, bones)
    pos, nrm = skin.read(c)
    ref_pos, ref_nrm = skin.skin_reference(b["positions"], b["normals"] if normals else None, b["indices"], binding[0], binding[1], bones)
    assert np.array_equal(_bits(pos), _bits(ref_pos))
    assert (nrm is None and ref_nrm is None) if not normals else np.array_equal(_bits(nrm), _bits(ref_nrm))
    return SS.posed_buffers(b, pos, nrm)


# ---------------------------------------------------------------------------------------------------------------------------- scene A skinned
@pytest.mark.parametrize("gpu_build", [0, 1, 2, 3], ids=["host-built", "binned", "lbvh", "ploc"])
def test_scene_a_skinned(capi, refit, skin, O, rest, gpu_build):
    """706 triangles in HBM; 2,118 vertices = 8 blocks of 256 + 70, then 6,354 corner normals = 24 blocks + 210.  Host-built (box leaves: every
    cube and the floor must survive the refit's checks) and the three device builders."""
    b, binding = rest[0]
    rays = _rays(O, 151 + gpu_build, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, gpu_build)
    try:
        assert c.stats().scene_in_lds == 0
        _bind(skin, c, b, binding)
        pos, nrm = skin.read(c)
        assert np.array_equal(_bits(pos), _bits(b["positions"])) and np.array_equal(_bits(nrm), _bits(b["normals"]))   # bound: the rest pose
        assert refit.refit_last(c)["path"] == refit.NONE                                                                 # bind does not refit
        moved = _skinned(skin, c, b, binding, SS.scene_a_bones(1 + gpu_build % 3))
        info = refit.refit_last(c)
        assert info["path"] == refit.DEVICE and info["n_records"] == NT
        if gpu_build == 0:
            assert info["n_boxes"] == RS.N_CUBES + 1 and info["n_quads"] == 1 + 6 * RS.N_CUBES
        assert np.array_equal(np.array(info["lo"], np.float32), moved["positions"].min(0)) and np.array_equal(np.array(info["hi"], np.float32), moved["positions"].max(0))
        scene = RS.oracle_scene(O, moved)
        what = "skinned scene A, builder %d" % gpu_build
        _strict_bars(capi, O, c, scene, rays, what)
        _fresh_trace_equal(capi, O, c, moved, rays, gpu_build, what)
        _shipped_bars(capi, O, c, scene, moved, rays, what, gpu_build)
    finally:
        skin.release(c)
        _close(c, refit)


@pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no-normals"])
def test_per_corner_and_indexed_with_and_without_normals(capi, refit, skin, O, rest, indexed, normals):
    """2,118 and 424 vertices: a block boundary plus a remainder in both ranges of the launch (424 = 256 + 168; the corner range is 6,354 either
    way, and absent without normals).  Indexed: a corner's matrix is that of the vertex its INDEX names, in a shuffled vertex buffer, and the two
    vertices no triangle names are skinned like any other.  Without normals the loaded ones stay."""
    b, binding = rest[1] if indexed else rest[0]
    assert b["positions"].shape[0] == (424 if indexed else 2118)
    rays = _rays(O, 161, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b)
    try:
        _bind(skin, c, b, binding, normals)
        moved = _skinned(skin, c, b, binding, SS.scene_a_bones(2), normals)
        unnamed = SS._objects(b) < 0
        assert int(unnamed.sum()) == (2 if indexed else 0) and (moved["positions"][unnamed] != b["positions"][unnamed]).any(1).all()
        if not normals:
            assert moved["normals"] is b["normals"]
            pos, nrm = np.empty((b["positions"].shape[0], 3), np.float32), np.empty((3 * NT, 3), np.float32)
            assert skin.load().trg_skin_read(c.h_ctx, pos.ctypes.data, nrm.ctypes.data) == -22      # bound without normals: none to read
            assert skin.buffers(c)["nrm"] is None and skin.buffers(c)["prev_nrm"] is None
        flat = RS.unindexed(moved)
        _strict_bars(capi, O, c, RS.oracle_scene(O, flat), rays, "skinned scene A indexed %d normals %d" % (indexed, normals), kernels=HBM_KERNELS[:1])
    finally:
        skin.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- against the pose unit
@pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
def test_one_hot_weights_are_trg_pose_apply(capi, refit, skin, pose, O, rest, indexed):
    """Weights (1, 0, 0, 0) on the bone of the vertex's object -- the other three ids naming arbitrary bones -- against trg_pose_apply on a twin
    context with the same matrices: read-back positions and normals equal under ==, strict frames and traces bit-identical."""
    b = (rest[1] if indexed else rest[0])[0]
    ids, w, nb = SS.one_hot(b)
    ids[:, 1:] = np.random.default_rng(5).integers(0, nb, (ids.shape[0], 3))
    x = PS.scene_a_xforms(3)
    rays = _rays(O, 171, RAY_LO, RAY_HI)
    s, p = _ctx(capi, O, b), _ctx(capi, O, b)
    try:
        skin.bind(s, b["positions"], b["normals"], b["indices"], ids, w, nb)
        skin.apply(s, np.concatenate([x, PS.identity(1)]))
        pose.bind(p, b["positions"], b["normals"], b["indices"], PS.scene_a_first())
        pose.apply(p, x)
        (s_pos, s_nrm), (p_pos, p_nrm) = skin.read(s), pose.read(p)
        assert (s_pos == p_pos).all() and (s_nrm == p_nrm).all()
        for c in (s, p):
            c.set_option(capi.OPT_STRICT, 1)
            c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(s.read_accum()), _bits(p.read_accum()))
        assert np.array_equal(s.trace(rays).view(np.uint8), p.trace(rays).view(np.uint8))
    finally:
        skin.release(s)
        pose.release(p)
        _close(s, refit)
        _close(p, refit)


# ---------------------------------------------------------------------------------------------------------------------------- sequences
def test_skins_apply_to_the_rest_geometry_and_the_previous_pose_is_kept(capi, refit, skin, O, rest):
    """P1 then P2: the current pose is skin(rest, P2), not skin(skin(rest, P1), P2); the previous buffers -- read through trg_skin_buffers and a
    device copy -- hold P1 bit for bit, the current ones P2, the indices are the bound ones.  A third apply rotates again."""
    b, binding = rest[1]
    nv = b["positions"].shape[0]
    P1, P2, P3 = SS.scene_a_bones(1), SS.scene_a_bones(2), SS.scene_a_bones(3)
    ref = [skin.skin_reference(b["positions"], b["normals"], b["indices"], binding[0], binding[1], P) for P in (P1, P2, P3)]
    c = _ctx(capi, O, b)
    try:
        _bind(skin, c, b, binding)
        rest_addr = skin.buffers(c)
        skin.apply(c, P1)
        skin.apply(c, P2)
        p = skin.buffers(c)
        c.sync()
        pos, nrm = skin.read(c)
        assert np.array_equal(_bits(pos), _bits(ref[1][0])) and np.array_equal(_bits(nrm), _bits(ref[1][1]))
        assert np.array_equal(_device_bytes(p["prev_pos"], nv * 12), ref[0][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["prev_nrm"], NT * 36), ref[0][1].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["pos"], nv * 12), ref[1][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["nrm"], NT * 36), ref[1][1].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["idx"], NT * 12), b["indices"].view(np.uint8).reshape(-1))
        assert len({p["pos"], p["prev_pos"]}) == 2 and p["idx"] == rest_addr["idx"]
        skin.apply(c, P3)
        q = skin.buffers(c)
        c.sync()
        assert q["prev_pos"] == p["pos"] and q["pos"] not in (p["pos"], p["prev_pos"])
        assert np.array_equal(_device_bytes(q["prev_pos"], nv * 12), ref[1][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(q["pos"], nv * 12), ref[2][0].view(np.uint8).reshape(-1))
    finally:
        skin.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_bind_refusals_are_the_validators_cases(capi, refit, skin, O, rest):
    b, binding = rest[0]
    nv = b["positions"].shape[0]
    c = _ctx(capi, O, b)
    try:
        L = skin.load()
        assert L.trg_skin_apply(c.h_ctx, SS.identity().ctypes.data) == -22       # apply without bind
        assert b"trg_skin_bind" in L.trg_last_error(c.h_ctx)
        with pytest.raises(capi.TrgError):
            skin.apply(c, SS.identity())
        for name, (ids, w, vert, word) in SS.bad_bindings(b).items():
            if vert is None:
                continue
            with pytest.raises(capi.TrgError) as e:
                skin.bind(c, b["positions"], b["normals"], b["indices"], ids, w, SS.N_BONES)
            print("%s: %s" % (name, e.value))
            assert e.value.code == -22 and "vertex %d " % vert in str(e.value) and word in str(e.value), (name, str(e.value))
        bad = b["positions"].copy()
        bad[1234, 1] = np.inf
        with pytest.raises(capi.TrgError) as e:
            skin.bind(c, bad, b["normals"], b["indices"], binding[0], binding[1], SS.N_BONES)
        assert e.value.code == -22 and "vertex 1234" in str(e.value)
        bad_idx = b["indices"].copy()
        bad_idx[3 * 400 + 1] = nv
        with pytest.raises(capi.TrgError) as e:
            skin.bind(c, b["positions"], b["normals"], bad_idx, binding[0], binding[1], SS.N_BONES)
        assert e.value.code == -22 and "triangle 400" in str(e.value)
        with pytest.raises(capi.TrgError) as e:
            skin.bind(c, b["positions"], b["normals"], b["indices"], binding[0], binding[1], SS.N_BONES, n_tris=705)
        assert e.value.code == -22 and "706" in str(e.value)
        with pytest.raises(capi.TrgError):                                       # still nothing bound
            skin.buffers(c)
        assert refit.refit_last(c)["path"] == refit.NONE
        ids, w, _, _ = SS.bad_bindings(b)["a sum off by 1e-6"]                   # within 1e-4: bound, and used as given
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, w, SS.N_BONES)
        _skinned(skin, c, b, (ids, w), SS.scene_a_bones(1))
    finally:
        skin.release(c)
        _close(c, refit)


def test_refused_applies_leave_scene_and_poses_as_they_were(capi, refit, skin, O, rest):
    """On the host-built tree, with cube 9's corners split between two bones.  While those two bones are equal the cube stays a box; under
    scene_a_bones(1) it is none: TRG_ERR_RANGE, decided from the refit's flag words before anything is written.  Non-finite bones: refused on the
    host, nothing enqueued.  After a trg_load_scene: "bind again".  Each leaves the strict frame, the trace, the current and the previous pose
    bit for bit what they were."""
    b = rest[0][0]
    binding = SS.scene_a_binding(b, split_cube=9)
    nv = b["positions"].shape[0]
    rays = _rays(O, 181, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, 0)
    try:
        _bind(skin, c, b, binding)
        skin.apply(c, SS.scene_a_bones(2, share=(10, 11)))
        _skinned(skin, c, b, binding, SS.scene_a_bones(3, share=(10, 11)))
        good = refit.refit_last(c)
        assert good["path"] == refit.DEVICE and good["n_boxes"] == RS.N_CUBES + 1

        def state():
            c.set_option(capi.OPT_STRICT, 1)
            c.render(0, SPP, BOUNCES)
            img, tr = c.read_accum(), c.trace(rays)
            c.set_option(capi.OPT_STRICT, 0)
            p = skin.buffers(c)
            c.sync()
            mem = [_device_bytes(p[k], n) for k, n in (("pos", nv * 12), ("nrm", NT * 36), ("prev_pos", nv * 12), ("prev_nrm", NT * 36))]
            return img, tr, p, mem, skin.read(c)
        before = state()
        nan = SS.scene_a_bones(3, share=(10, 11))
        nan[20, 7] = np.nan
        for name, x, code, text in (("split cube", SS.scene_a_bones(1), -34, "triangle"), ("nan", nan, -22, "bone 20")):
            with pytest.raises(capi.TrgError) as e:
                skin.apply(c, x)
            print("%s: %s" % (name, e.value))
            assert e.value.code == code and text in str(e.value), (name, str(e.value))
            after = state()
            assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8)), name
            assert after[2] == before[2] and all(np.array_equal(m, n) for m, n in zip(after[3], before[3])), name
            assert all(np.array_equal(_bits(m), _bits(n)) for m, n in zip(after[4], before[4])), name
            if code == -22:
                assert refit.refit_last(c) == good
        moved = _skinned(skin, c, b, binding, SS.scene_a_bones(2, share=(10, 11)))   # the next valid call works
        _strict_bars(capi, O, c, RS.oracle_scene(O, moved), rays, "after the refusals", kernels=HBM_KERNELS[:1])
        b2 = RS.scene_a(1)
        c.load_scene(b2["positions"], b2["normals"], b2["colors"], b2["indices"], b2["material_ids"])      # a load makes the binding stale
        c.set_option(capi.OPT_STRICT, 1)
        c.render(0, SPP, BOUNCES)
        loaded = c.read_accum()
        for call in (lambda: skin.apply(c, SS.identity()), lambda: skin.read(c), lambda: skin.buffers(c)):
            with pytest.raises(capi.TrgError) as e:
                call()
            assert e.value.code == -22 and "bind again" in str(e.value)
        c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(c.read_accum()), _bits(loaded))
        c.set_option(capi.OPT_STRICT, 0)
        _bind(skin, c, b, binding)
        skin.apply(c, SS.identity())
        skin.release(c)                                                          # release unbinds, and only that
        with pytest.raises(capi.TrgError):
            skin.buffers(c)
        assert refit.refit_last(c)["path"] == refit.DEVICE
    finally:
        skin.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- the LDS tier
def test_small_scene_is_skinned_through_the_rebuild_and_keeps_its_textures(capi, refit, skin, O):
    """The Cornell box, LDS-resident, its short box TWISTED: the top turns, the bottom stays, the side faces are no plane quads any more -- the
    buffers are downloaded and the host builder runs (REBUILD); strict frames are the oracle's of the read-back geometry bit for bit, in the LDS
    kernel and with TRG_OPT_FORCE_GLOBAL; textures on the short box and the floor survive."""
    rays = _rays(O, 191, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0))
    b = RS.cornell_moved(O, 0)
    ids, w, nb, axis = SS.cornell_binding(b)
    for tex in (None, _textures(36, 0, 14, 6)):
        c = _ctx(capi, O, b)
        try:
            assert c.stats().scene_in_lds == 1
            if tex:
                c.load_textures(*tex)
            skin.bind(c, b["positions"], b["normals"], b["indices"], ids, w, nb)
            for s in (1, 2):
                moved = _skinned(skin, c, b, (ids, w), SS.twist_bones(axis, 12.0 * s))
                assert refit.refit_last(c)["path"] == refit.REBUILD and c.stats().scene_in_lds == 1
                top = w[:36, 1] == 1
                assert top.sum() == 18 and (w[:36, 1][~top] == 0).all()
                assert (moved["positions"][36:] == b["positions"][36:]).all() and (moved["positions"][:36][~top] == b["positions"][:36][~top]).all()
                assert (moved["positions"][:36][top] != b["positions"][:36][top]).any(1).all()
                scene = RS.oracle_scene(O, moved, tex)
                for force_global in (0, 1):
                    c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
                    _strict_bars(capi, O, c, scene, rays, "twisted cornell step %d global %d" % (s, force_global), kernels=(("direct", 0, 1),))
                    if force_global == 0:                                    # the shipped LDS kernels test the room ahead of the tree: the strict build does not know it
                        assert c.stats().bvh_room == 5
                        _shipped_bars(capi, O, c, scene, moved, rays, "twisted cornell step %d" % s)
                c.set_option(capi.OPT_FORCE_GLOBAL, 0)
        finally:
            skin.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- temporal
def _cornell_ctx(capi, O, b, w, h):
    c = capi.Context(w, h)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
    c.set_pixel_offsets(O.pixel_offsets(w, h))
    return c


def test_previous_scene_from_the_skin_units_buffers_gives_the_host_forms_motion_planes(capi, refit, skin, dn, O):
    """Two skins of the Cornell box; the unit's PREVIOUS buffers handed to trg_temporal_set_previous_scene_device: M0 and M1 of
    trg_guides_render_motion bit for bit those after the host form with the read-back arrays of the first skin."""
    w, h = 64, 48
    b = RS.cornell_moved(O, 0)
    ids, wts, nb, axis = SS.cornell_binding(b)
    c = _cornell_ctx(capi, O, b, w, h)
    try:
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, wts, nb)
        skin.apply(c, SS.twist_bones(axis, 10.0))
        first = skin.read(c)
        skin.apply(c, SS.twist_bones(axis, 25.0))
        dn.temporal_set_previous_scene(c, first[0], first[1], b["indices"])
        want = dn.guides_motion(c, 0)
        dn.temporal_set_previous_scene(c, None, None, None)                      # forgotten: the next planes can only come from the device form
        p = skin.buffers(c)
        dn.temporal_set_previous_scene_device(c, p["prev_pos"], p["prev_nrm"], p["idx"], n_verts=108, n_tris=36)
        got = dn.guides_motion(c, 0)
        for a, e in zip(got, want):
            assert np.array_equal(_bits(a), _bits(e))
        assert (got[2][0, ..., 3] == 1).any()
    finally:
        skin.release(c)
        dn.release(c)
        _close(c, refit)


def test_temporal_history_follows_the_skins_without_a_host_copy(capi, refit, skin, dn, O):
    """The short box twisting over three calls, as HipRenderer::poseSkin drives the C ABI: trg_skin_apply, the unit's PREVIOUS buffers to
    trg_temporal_set_previous_scene_device, trg_render_temporal -- against the same calls with the read-back arrays through trg_refit_scene and the
    host form: every step's output bit for bit."""
    w, h, bounces = 64, 48, 3
    b = RS.cornell_moved(O, 0)
    ids, wts, nb, axis = SS.cornell_binding(b)
    P, Q = _cornell_ctx(capi, O, b, w, h), _cornell_ctx(capi, O, b, w, h)
    try:
        skin.bind(P, b["positions"], b["normals"], b["indices"], ids, wts, nb)
        read = [(b["positions"], b["normals"])]
        for k in range(3):
            if k:
                skin.apply(P, SS.twist_bones(axis, 8.0 * k))
                p = skin.buffers(P)
                dn.temporal_set_previous_scene_device(P, p["prev_pos"], p["prev_nrm"], p["idx"], n_verts=108, n_tris=36)
                read.append(skin.read(P))
                refit.refit_scene(Q, read[k][0], read[k][1], b["indices"])
                dn.temporal_set_previous_scene(Q, read[k - 1][0], read[k - 1][1], b["indices"])
            got, want = dn.render_temporal(P, k, 1, bounces, iterations=3), dn.render_temporal(Q, k, 1, bounces, iterations=3)
            assert np.array_equal(_bits(got), _bits(want)), k
        assert (read[2][0][:36] != read[1][0][:36]).any()
    finally:
        skin.release(P)
        for c in (P, Q):
            dn.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- group, plugin
def test_group_skins_match_the_single_context(capi, refit, skin, O, rest, monkeypatch):
    """Two contexts on one device, each rendering its band of the skinned scene, gathered: the single context's frame."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    b, binding = rest[0]
    u = O.uniforms_bytes(O.make_uniforms(W, H))
    c = capi.Context(W, H)
    g = capi.Group([0, 0], W, H)
    try:
        for x in (c, g):
            x.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            x.set_uniforms(u)
            x.set_pixel_offsets_seed()
            _bind(skin, x, b, binding)
            skin.apply(x, SS.scene_a_bones(2))
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.DEVICE
        c.render(0, SPP, BOUNCES)
        g.render(0, SPP, BOUNCES)
        g.sync()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(c.read_accum()))
        bad = SS.scene_a_bones(2)
        bad[3, 0] = np.inf
        with pytest.raises(capi.TrgError) as e:
            skin.apply(g, bad)
        assert e.value.code == -22 and "bone 3" in str(e.value)
    finally:
        skin.release(g)
        refit.release(g)
        g.close()
        skin.release(c)
        _close(c, refit)


def test_plugin_skin_option(capi, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png twist=5 skin: HipRenderer::bindSkin once, poseSkin before every call but the first, plain and with
    denoise=5,temporal: exit 0, "3 skins applied" as the last line, a picture that differs from the untwisted one.  twist=0: the picture without
    the option, in both modes; and IDENTITY bones applied before every call through the C ABI write that picture too (plain mode; in temporal mode an
    apply arms the previous-position planes, another reprojection path).  Together with refit or pose: refused."""
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 64, 48, 4, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba(), r.stdout
    still = {False: run("still.png"), True: run("still_t.png", "denoise=5,temporal")}
    for temporal in (False, True):
        extra = ("denoise=5,temporal",) if temporal else ()
        pic, out = run("skin%d.png" % temporal, *extra, "twist=5", "skin")
        assert out.strip().splitlines()[-1] == "%d skins applied" % (frames - 1) and "refused" not in out
        assert not np.array_equal(pic, still[temporal][0])
        zero, out = run("zero%d.png" % temporal, *extra, "twist=0", "skin")       # no twist: bound, nothing applied (as slide=0 under pose)
        assert out.strip().splitlines()[-1] == "0 skins applied"
        assert np.array_equal(zero, still[temporal][0])
    assert "skins" not in still[False][1]
    b = host.Scene.cornell_box().buffers()
    ids, wts, nb, axis = SS.cornell_binding(b)
    c = capi.Context(w, h)
    try:
        from toyraygun_amd import skin
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, wts, nb)
        for k in range(frames):
            if k:
                skin.apply(c, SS.twist_bones(axis, 0.0))
            c.render(k, 1, bounces)
        c.sync()
        assert np.array_equal(c.postprocess(flip_y=True), still[False][0])
    finally:
        skin.release(c)
        c.close()
    for other in ("pose", "refit"):
        assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "twist=5", "skin", other], capture_output=True, timeout=120).returncode != 0
