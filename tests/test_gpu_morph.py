"""GPU tests (-m gpu) of the morph unit (include/trg_morph.h): a loaded scene morphed on the device -- blend shapes, optionally in front of a skin
-- against morph_reference (bit for bit), against the CPU oracle's render of the read-back geometry (bit for bit in the strict build; inside the
shipped build's bar otherwise), against a fresh trg_load_scene and against trg_skin_apply for zero target weights.  Images 32 x 24, 2 spp,
3 bounces; traces 4,096 random rays -- the sizes of tests/test_gpu_refit.py, whose bars these are.  The targets, weights and bones keep every box
and quad leaf of scene A: tests/test_morph_host.py checks that on the CPU.  Nothing here provokes a fault: every refusal is decided on the host or
from flag words before anything is written."""
import os
import subprocess

import numpy as np
import pytest

from tests import morph_scenes as MS
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
def morph(built):
    from toyraygun_amd import morph as m
    m.load()
    return m


@pytest.fixture(scope="module")
def skin(built):
    from toyraygun_amd import skin as s
    s.load()
    return s


@pytest.fixture(scope="module")
def dn(built):
    from toyraygun_amd import denoise
    denoise.load()
    return denoise


@pytest.fixture(scope="module")
def rest():
    """Scene A as loaded -- per corner and indexed -- with its targets and its skin binding; shared and left unchanged."""
    a, i = MS.scene(False), MS.scene(True)
    return (a, MS.targets(a), SS.scene_a_binding(a)), (i, MS.targets(i), SS.scene_a_binding(i))


def _bind(morph, c, b, t, binding=None, normals=True, deltas=True):
    skin_args = {} if binding is None else dict(bone_ids=binding[0], bone_weights=binding[1], n_bones=SS.N_BONES)
    morph.bind(c, b["positions"], b["normals"] if normals else None, b["indices"], t[0], t[1], t[2], t[3] if deltas else None, **skin_args)


def _reference(morph, b, t, tw, binding=None, bones=None, normals=True, deltas=True):
    skin_args = {} if binding is None else dict(bone_ids=binding[0], bone_weights=binding[1], bones=bones)
    return morph.morph_reference(b["positions"], b["normals"] if normals else None, b["indices"], t[0], t[1], t[2], t[3] if deltas else None, tw, **skin_args)


def _morphed(morph, c, b, t, tw, binding=None, bones=None, normals=True, deltas=True):
    """apply + read, checked against morph_reference bit for bit; returns the buffer dict of the read-back geometry."""
    morph.apply(c, tw, bones)
    pos, nrm = morph.read(c)
    ref_pos, ref_nrm = _reference(morph, b, t, tw, binding, bones, normals, deltas)
    assert np.array_equal(_bits(pos), _bits(ref_pos))
    assert (nrm is None and ref_nrm is None) if not normals else np.array_equal(_bits(nrm), _bits(ref_nrm))
    return SS.posed_buffers(b, pos, nrm)


# ---------------------------------------------------------------------------------------------------------------------------- scene A morphed
@pytest.mark.parametrize("gpu_build", [0, 1, 2, 3], ids=["host-built", "binned", "lbvh", "ploc"])
def test_scene_a_morphed(capi, refit, morph, O, rest, gpu_build):
    """706 triangles in HBM; 2,118 vertices = 8 blocks of 256 + 70, then 6,354 corner normals = 24 blocks + 210; no bones.  Host-built (box
    leaves: every cube and the floor must survive the refit's checks) and the three device builders."""
    b, t, _ = rest[0]
    rays = _rays(O, 251 + gpu_build, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, gpu_build)
    try:
        assert c.stats().scene_in_lds == 0
        _bind(morph, c, b, t)
        pos, nrm = morph.read(c)
        assert np.array_equal(_bits(pos), _bits(b["positions"])) and np.array_equal(_bits(nrm), _bits(b["normals"]))   # bound: the rest pose
        assert refit.refit_last(c)["path"] == refit.NONE                                                                 # bind does not refit
        moved = _morphed(morph, c, b, t, MS.weights("abc"[gpu_build % 3]))
        info = refit.refit_last(c)
        assert info["path"] == refit.DEVICE and info["n_records"] == NT
        if gpu_build == 0:
            assert info["n_boxes"] == RS.N_CUBES + 1 and info["n_quads"] == 1 + 6 * RS.N_CUBES
        assert np.array_equal(np.array(info["lo"], np.float32), moved["positions"].min(0)) and np.array_equal(np.array(info["hi"], np.float32), moved["positions"].max(0))
        scene = RS.oracle_scene(O, moved)
        what = "morphed scene A, builder %d" % gpu_build
        _strict_bars(capi, O, c, scene, rays, what)
        _fresh_trace_equal(capi, O, c, moved, rays, gpu_build, what)
        _shipped_bars(capi, O, c, scene, moved, rays, what, gpu_build)
    finally:
        morph.release(c)
        _close(c, refit)


@pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
@pytest.mark.parametrize("form", ["normal-deltas", "normals", "no-normals"])
def test_per_corner_and_indexed_in_every_normals_form(capi, refit, morph, O, rest, indexed, form):
    """2,118 and 424 vertices: a block boundary plus a remainder in both ranges of the launch.  Indexed: a corner walks the records of the vertex
    its INDEX names, in a shuffled vertex buffer, and the two vertices no triangle names are morphed like any other.  With normals but without
    normal deltas the corner range is not launched and the loaded normals are kept bit for bit; without normals there are none to read."""
    b, t, _ = rest[1] if indexed else rest[0]
    normals, deltas = form != "no-normals", form == "normal-deltas"
    rays = _rays(O, 261, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b)
    try:
        _bind(morph, c, b, t, normals=normals, deltas=deltas)
        moved = _morphed(morph, c, b, t, MS.weights("a"), normals=normals, deltas=deltas)
        unnamed = SS._objects(b) < 0
        assert int(unnamed.sum()) == (2 if indexed else 0) and (moved["positions"][unnamed] != b["positions"][unnamed]).any(1).all()
        if form == "normals":
            assert np.array_equal(_bits(moved["normals"]), _bits(b["normals"]))
        if not normals:
            assert moved["normals"] is b["normals"]
            pos, nrm = np.empty((b["positions"].shape[0], 3), np.float32), np.empty((3 * NT, 3), np.float32)
            assert morph.load().trg_morph_read(c.h_ctx, pos.ctypes.data, nrm.ctypes.data) == -22     # bound without normals: none to read
            assert morph.buffers(c)["nrm"] is None and morph.buffers(c)["prev_nrm"] is None
        flat = RS.unindexed(moved)
        _strict_bars(capi, O, c, RS.oracle_scene(O, flat), rays, "morphed scene A indexed %d %s" % (indexed, form), kernels=HBM_KERNELS[:1])
    finally:
        morph.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- with bones
@pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
@pytest.mark.parametrize("deltas", [True, False], ids=["normal-deltas", "no-deltas"])
def test_with_bones_is_the_fused_reference(capi, refit, morph, O, rest, indexed, deltas):
    """Targets in front of scene A's 38 bones, all four template forms of the kernel between this test and the one above: the read-back equals
    the fused reference -- skin_reference of the bone-free morph -- bit for bit, and the strict frame is the oracle's."""
    b, t, binding = rest[1] if indexed else rest[0]
    rays = _rays(O, 271, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b)
    try:
        _bind(morph, c, b, t, binding, deltas=deltas)
        _morphed(morph, c, b, t, MS.weights("b"), binding, SS.scene_a_bones(1), deltas=deltas)
        moved = _morphed(morph, c, b, t, MS.weights("c"), binding, SS.scene_a_bones(2), deltas=deltas)
        assert refit.refit_last(c)["path"] == refit.DEVICE
        _strict_bars(capi, O, c, RS.oracle_scene(O, RS.unindexed(moved)), rays, "morphed and skinned scene A indexed %d deltas %d" % (indexed, deltas), kernels=HBM_KERNELS[:1])
    finally:
        morph.release(c)
        _close(c, refit)


@pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
def test_zero_target_weights_with_bones_are_trg_skin_apply(capi, refit, morph, skin, O, rest, indexed):
    """All-zero target weights (zeros of either sign) under bones against trg_skin_apply on a twin context: read-back positions and normals, strict
    frame and trace bit for bit.  And one-hot identity bones under weights: the bone-free morph -- positions under ==; normals within one ulp of a
    unit component, 2^-23: under bones a corner goes through pose::normal, which normalises once more (the reference shows 294 corners of 6,354
    one ulp off, and the device equals the reference bit for bit)."""
    b, t, binding = rest[1] if indexed else rest[0]
    bones = SS.scene_a_bones(3)
    rays = _rays(O, 281, RAY_LO, RAY_HI)
    m, s = _ctx(capi, O, b), _ctx(capi, O, b)
    try:
        _bind(morph, m, b, t, binding)
        morph.apply(m, MS.weights(MS.ZERO), bones)
        skin.bind(s, b["positions"], b["normals"], b["indices"], binding[0], binding[1], SS.N_BONES)
        skin.apply(s, bones)
        (m_pos, m_nrm), (s_pos, s_nrm) = morph.read(m), skin.read(s)
        assert np.array_equal(_bits(m_pos), _bits(s_pos)) and np.array_equal(_bits(m_nrm), _bits(s_nrm))
        for c in (m, s):
            c.set_option(capi.OPT_STRICT, 1)
            c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(m.read_accum()), _bits(s.read_accum()))
        assert np.array_equal(m.trace(rays).view(np.uint8), s.trace(rays).view(np.uint8))
        for c in (m, s):
            c.set_option(capi.OPT_STRICT, 0)
        # one-hot identity bones: M is the identity (1 x = x, 0 x = 0, x + 0 = x), so the skin behind the morph changes nothing under ==
        ids, w, nb = SS.one_hot(b)
        morph.bind(m, b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], bone_ids=ids, bone_weights=w, n_bones=nb)
        morph.apply(m, MS.weights("a"), SS.identity(nb))
        pos, nrm = morph.read(m)
        free_pos, free_nrm = _reference(morph, b, t, MS.weights("a"))
        assert (pos == free_pos).all() and np.abs(nrm.astype(np.float64) - free_nrm).max() <= 2.0 ** -23
        untouched = (nrm == b["normals"]).all(1) & (free_nrm == b["normals"]).all(1)
        assert untouched.any()
    finally:
        morph.release(m)
        skin.release(s)
        _close(m, refit)
        _close(s, refit)


# ---------------------------------------------------------------------------------------------------------------------------- zero weights, sequences
def test_zero_weights_return_the_rest_pose_bit_for_bit(capi, refit, morph, O, rest):
    """No bones, all weights zero (of either sign): every target is skipped.  The rest pose comes back bit for bit -- the -0.0 coordinate as -0.0,
    compared as bits -- and T5's 1e6 reached nothing.  After a morph that moved everything: apply starts from the rest geometry."""
    b, t, _ = rest[1]
    c = _ctx(capi, O, b)
    try:
        _bind(morph, c, b, t)
        morph.apply(c, MS.weights("a"))
        assert (morph.read(c)[0] != b["positions"]).any()
        morph.apply(c, MS.weights(MS.ZERO))
        pos, nrm = morph.read(c)
        assert np.array_equal(_bits(pos), _bits(b["positions"])) and np.array_equal(_bits(nrm), _bits(b["normals"]))
        v = MS.minus_zero_vertex(b)
        assert _bits(pos)[v, 1] == 0x80000000
        assert refit.refit_last(c)["path"] == refit.DEVICE
    finally:
        morph.release(c)
        _close(c, refit)


def test_morphs_apply_to_the_rest_geometry_and_the_previous_pose_is_kept(capi, refit, morph, O, rest):
    """w1 then w2: the current pose is morph(rest, w2), not a morph of the morph; the previous buffers -- read through trg_morph_buffers and a
    device copy -- hold w1's result bit for bit, the current ones w2's, the indices are the bound ones.  A third apply rotates again."""
    b, t, _ = rest[1]
    nv = b["positions"].shape[0]
    ref = [_reference(morph, b, t, MS.weights(k)) for k in "abc"]
    c = _ctx(capi, O, b)
    try:
        _bind(morph, c, b, t)
        rest_addr = morph.buffers(c)
        morph.apply(c, MS.weights("a"))
        morph.apply(c, MS.weights("b"))
        p = morph.buffers(c)
        c.sync()
        pos, nrm = morph.read(c)
        assert np.array_equal(_bits(pos), _bits(ref[1][0])) and np.array_equal(_bits(nrm), _bits(ref[1][1]))
        assert np.array_equal(_device_bytes(p["prev_pos"], nv * 12), ref[0][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["prev_nrm"], NT * 36), ref[0][1].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["pos"], nv * 12), ref[1][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["nrm"], NT * 36), ref[1][1].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["idx"], NT * 12), b["indices"].view(np.uint8).reshape(-1))
        assert len({p["pos"], p["prev_pos"]}) == 2 and p["idx"] == rest_addr["idx"]
        morph.apply(c, MS.weights("c"))
        q = morph.buffers(c)
        c.sync()
        assert q["prev_pos"] == p["pos"] and q["pos"] not in (p["pos"], p["prev_pos"])
        assert np.array_equal(_device_bytes(q["prev_pos"], nv * 12), ref[1][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(q["pos"], nv * 12), ref[2][0].view(np.uint8).reshape(-1))
    finally:
        morph.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_bind_refusals_are_the_validators_cases(capi, refit, morph, O, rest):
    b, t, binding = rest[0]
    nv = b["positions"].shape[0]
    c = _ctx(capi, O, b)
    try:
        L = morph.load()
        assert L.trg_morph_apply(c.h_ctx, MS.weights("a").ctypes.data, None) == -22      # apply without bind
        assert b"trg_morph_bind" in L.trg_last_error(c.h_ctx)
        for name, (first, ev, dp, dnrm, ne, _, words) in MS.bad_targets(b).items():
            with pytest.raises(capi.TrgError) as e:
                morph.bind(c, b["positions"], b["normals"], b["indices"], first, ev, dp, dnrm, n_entries=ne)
            print("%s: %s" % (name, e.value))
            assert e.value.code == -22 and all(w in str(e.value) for w in words), (name, str(e.value))
        with pytest.raises(capi.TrgError) as e:                                  # normal deltas without normals
            morph.bind(c, b["positions"], None, b["indices"], *t)
        assert e.value.code == -22 and "without normals" in str(e.value)
        for ids, w, n in ((binding[0], None, SS.N_BONES), (None, binding[1], SS.N_BONES), (binding[0], binding[1], 0), (None, None, 3)):
            with pytest.raises(capi.TrgError) as e:                              # half-given bones
                morph.bind(c, b["positions"], b["normals"], b["indices"], *t, bone_ids=ids, bone_weights=w, n_bones=n)
            assert e.value.code == -22 and "all three or none" in str(e.value)
        for name, (ids, w, vert, word) in SS.bad_bindings(b).items():            # the skin unit's checks, with its texts
            if vert is None:
                continue
            with pytest.raises(capi.TrgError) as e:
                morph.bind(c, b["positions"], b["normals"], b["indices"], *t, bone_ids=ids, bone_weights=w, n_bones=SS.N_BONES)
            assert e.value.code == -22 and "vertex %d " % vert in str(e.value) and word in str(e.value), (name, str(e.value))
        with pytest.raises(capi.TrgError) as e:                                  # no targets
            morph.bind(c, b["positions"], b["normals"], b["indices"], np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))
        assert e.value.code == -22 and "no targets" in str(e.value)
        bad = b["positions"].copy()
        bad[1234, 1] = np.inf
        with pytest.raises(capi.TrgError) as e:
            morph.bind(c, bad, b["normals"], b["indices"], *t)
        assert e.value.code == -22 and "vertex 1234" in str(e.value)
        bad_idx = b["indices"].copy()
        bad_idx[3 * 400 + 1] = nv
        with pytest.raises(capi.TrgError) as e:
            morph.bind(c, b["positions"], b["normals"], bad_idx, *t)
        assert e.value.code == -22 and "triangle 400" in str(e.value)
        with pytest.raises(capi.TrgError) as e:
            morph.bind(c, b["positions"], b["normals"], b["indices"], *t, n_tris=705)
        assert e.value.code == -22 and "706" in str(e.value)
        with pytest.raises(capi.TrgError):                                       # still nothing bound
            morph.buffers(c)
        assert refit.refit_last(c)["path"] == refit.NONE
        # a binding whose targets are ALL empty is legal, and every apply of it gives the rest pose
        morph.bind(c, b["positions"], b["normals"], b["indices"], np.zeros(3, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))
        morph.apply(c, np.array([2.0, -1.0], np.float32))
        assert np.array_equal(_bits(morph.read(c)[0]), _bits(b["positions"]))
    finally:
        morph.release(c)
        _close(c, refit)


@pytest.mark.parametrize("with_bones", [False, True], ids=["no-bones", "bones"])
def test_refused_applies_leave_scene_and_poses_as_they_were(capi, refit, morph, O, rest, with_bones):
    """On the host-built tree, with the one-corner target in T3's place.  At weight 0 cube 9 is the box it was; at weight 1 it is none:
    TRG_ERR_RANGE, decided from the refit's flag words before anything is written.  Weights that are not finite, bones missing or given against
    the binding or not finite: refused on the host, nothing enqueued.  After a trg_load_scene: "bind again".  Each leaves the strict frame, the
    trace, the current and the previous pose and trg_refit_last bit for bit what they were."""
    b, _, binding = rest[0]
    if not with_bones:
        binding = None
    t = MS.targets(b, one_corner=True)
    nv = b["positions"].shape[0]
    bones = [SS.scene_a_bones(s) if with_bones else None for s in (1, 2, 3)]
    rays = _rays(O, 291, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, 0)
    try:
        _bind(morph, c, b, t, binding)
        morph.apply(c, MS.weights("a"), bones[0])
        _morphed(morph, c, b, t, MS.weights("b"), binding, bones[1])
        good = refit.refit_last(c)
        assert good["path"] == refit.DEVICE and good["n_boxes"] == RS.N_CUBES + 1

        def state():
            c.set_option(capi.OPT_STRICT, 1)
            c.render(0, SPP, BOUNCES)
            img, tr = c.read_accum(), c.trace(rays)
            c.set_option(capi.OPT_STRICT, 0)
            p = morph.buffers(c)
            c.sync()
            mem = [_device_bytes(p[k], n) for k, n in (("pos", nv * 12), ("nrm", NT * 36), ("prev_pos", nv * 12), ("prev_nrm", NT * 36))]
            return img, tr, p, mem, morph.read(c)
        before = state()
        one = MS.weights("c").copy()
        one[MS.EMPTY] = 1.0
        nan, inf = MS.weights("c").copy(), MS.weights("c").copy()
        nan[4], inf[MS.LAST] = np.nan, -np.inf
        cases = [("one corner", one, bones[2], -34, "triangle"), ("nan", nan, bones[2], -22, "target 4"), ("inf", inf, bones[2], -22, "target %d" % MS.LAST)]
        if with_bones:
            bad = bones[2].copy()
            bad[20, 7] = np.nan
            cases += [("null bones", MS.weights("c"), None, -22, "null bones"), ("nan bone", MS.weights("c"), bad, -22, "bone 20")]
        else:
            cases += [("bones against the binding", MS.weights("c"), SS.scene_a_bones(1), -22, "has none")]
        for name, tw, x, code, text in cases:
            with pytest.raises(capi.TrgError) as e:
                morph.apply(c, tw, x)
            print("%s: %s" % (name, e.value))
            assert e.value.code == code and text in str(e.value), (name, str(e.value))
            after = state()
            assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8)), name
            assert after[2] == before[2] and all(np.array_equal(m, n) for m, n in zip(after[3], before[3])), name
            assert all(np.array_equal(_bits(m), _bits(n)) for m, n in zip(after[4], before[4])), name
            assert refit.refit_last(c) == good, name
        moved = _morphed(morph, c, b, t, MS.weights("c"), binding, bones[2])      # the next valid call works
        _strict_bars(capi, O, c, RS.oracle_scene(O, moved), rays, "after the refusals", kernels=HBM_KERNELS[:1])
        b2 = RS.scene_a(1)
        c.load_scene(b2["positions"], b2["normals"], b2["colors"], b2["indices"], b2["material_ids"])      # a load makes the binding stale
        c.set_option(capi.OPT_STRICT, 1)
        c.render(0, SPP, BOUNCES)
        loaded = c.read_accum()
        for call in (lambda: morph.apply(c, MS.weights("a"), bones[0]), lambda: morph.read(c), lambda: morph.buffers(c)):
            with pytest.raises(capi.TrgError) as e:
                call()
            assert e.value.code == -22 and "bind again" in str(e.value)
        c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(c.read_accum()), _bits(loaded))
        c.set_option(capi.OPT_STRICT, 0)
        _bind(morph, c, b, t, binding)
        morph.apply(c, MS.weights(MS.ZERO), bones[0])
        morph.release(c)                                                         # release unbinds, and only that
        with pytest.raises(capi.TrgError):
            morph.buffers(c)
        assert refit.refit_last(c)["path"] == refit.DEVICE
    finally:
        morph.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- the LDS tier
def test_small_scene_is_morphed_through_the_rebuild_and_keeps_its_textures(capi, refit, morph, O):
    """The Cornell box, LDS-resident, the top of its short box BULGED (and, second binding, twisted behind that): the side faces are no
    parallelograms any more -- the buffers are downloaded and the host builder runs (REBUILD); strict frames are the oracle's of the read-back
    geometry bit for bit, in the LDS kernel and with TRG_OPT_FORCE_GLOBAL; textures on the short box and the floor survive."""
    rays = _rays(O, 301, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0))
    b = RS.cornell_moved(O, 0)
    first, ev, dp = MS.cornell_bulge(b)
    ids, w, nb, axis = SS.cornell_binding(b)
    assert ev.shape[0] == 18
    for tex, with_bones in ((None, False), (_textures(36, 0, 14, 6), False), (_textures(36, 0, 14, 6), True)):
        c = _ctx(capi, O, b)
        try:
            assert c.stats().scene_in_lds == 1
            if tex:
                c.load_textures(*tex)
            skin_args = dict(bone_ids=ids, bone_weights=w, n_bones=nb) if with_bones else {}
            morph.bind(c, b["positions"], b["normals"], b["indices"], first, ev, dp, None, **skin_args)
            for s in (1, 2):
                tw, bones = np.array([0.15 * s], np.float32), SS.twist_bones(axis, 12.0 * s) if with_bones else None
                morph.apply(c, tw, bones)
                pos, nrm = morph.read(c)
                ref = morph.morph_reference(b["positions"], b["normals"], b["indices"], first, ev, dp, None, tw, **(dict(bone_ids=ids, bone_weights=w, bones=bones) if with_bones else {}))
                assert np.array_equal(_bits(pos), _bits(ref[0])) and np.array_equal(_bits(nrm), _bits(ref[1]))
                moved = SS.posed_buffers(b, pos, nrm)
                assert refit.refit_last(c)["path"] == refit.REBUILD and c.stats().scene_in_lds == 1
                assert (pos[36:] == b["positions"][36:]).all() and (pos[ev] != b["positions"][ev]).any(1).all()
                scene = RS.oracle_scene(O, moved, tex)
                for force_global in (0, 1):
                    c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
                    _strict_bars(capi, O, c, scene, rays, "bulged cornell step %d global %d bones %d" % (s, force_global, with_bones), kernels=(("direct", 0, 1),))
                    if force_global == 0:                                    # the shipped LDS kernels test the room ahead of the tree: the strict build does not know it
                        assert c.stats().bvh_room == 5
                        _shipped_bars(capi, O, c, scene, moved, rays, "bulged cornell step %d bones %d" % (s, with_bones))
                c.set_option(capi.OPT_FORCE_GLOBAL, 0)
        finally:
            morph.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- temporal
def _cornell_ctx(capi, O, b, w, h):
    c = capi.Context(w, h)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
    c.set_pixel_offsets(O.pixel_offsets(w, h))
    return c


def test_temporal_history_follows_the_morphs_without_a_host_copy(capi, refit, morph, dn, O):
    """The short box bulging over three calls, as HipRenderer::poseMorph drives the C ABI: trg_morph_apply, the unit's PREVIOUS buffers to
    trg_temporal_set_previous_scene_device, trg_render_temporal -- against the same calls with the read-back arrays through trg_refit_scene and the
    host form: the motion planes of the second step and every step's output bit for bit."""
    w, h, bounces = 64, 48, 3
    b = RS.cornell_moved(O, 0)
    first, ev, dp = MS.cornell_bulge(b)
    P, Q = _cornell_ctx(capi, O, b, w, h), _cornell_ctx(capi, O, b, w, h)
    try:
        morph.bind(P, b["positions"], b["normals"], b["indices"], first, ev, dp)
        read = [(b["positions"], b["normals"])]
        for k in range(3):
            if k:
                morph.apply(P, np.array([0.1 * k], np.float32))
                p = morph.buffers(P)
                dn.temporal_set_previous_scene_device(P, p["prev_pos"], p["prev_nrm"], p["idx"], n_verts=108, n_tris=36)
                read.append(morph.read(P))
                refit.refit_scene(Q, read[k][0], read[k][1], b["indices"])
                dn.temporal_set_previous_scene(Q, read[k - 1][0], read[k - 1][1], b["indices"])
            if k == 2:
                got, want = dn.guides_motion(P, 0), dn.guides_motion(Q, 0)
                for a, e in zip(got, want):
                    assert np.array_equal(_bits(a), _bits(e))
                assert (got[2][0, ..., 3] == 1).any()
            got, want = dn.render_temporal(P, k, 1, bounces, iterations=3), dn.render_temporal(Q, k, 1, bounces, iterations=3)
            assert np.array_equal(_bits(got), _bits(want)), k
        assert (read[2][0][:36] != read[1][0][:36]).any()
    finally:
        morph.release(P)
        for c in (P, Q):
            dn.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- group, plugin
def test_group_morphs_match_the_single_context(capi, refit, morph, O, rest, monkeypatch):
    """Two contexts on one device, each rendering its band of the morphed and skinned scene, gathered: the single context's frame."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    b, t, binding = rest[0]
    u = O.uniforms_bytes(O.make_uniforms(W, H))
    c = capi.Context(W, H)
    g = capi.Group([0, 0], W, H)
    try:
        for x in (c, g):
            x.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            x.set_uniforms(u)
            x.set_pixel_offsets_seed()
            _bind(morph, x, b, t, binding)
            morph.apply(x, MS.weights("b"), SS.scene_a_bones(2))
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.DEVICE
        c.render(0, SPP, BOUNCES)
        g.render(0, SPP, BOUNCES)
        g.sync()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(c.read_accum()))
        bad = MS.weights("b").copy()
        bad[2] = np.inf
        with pytest.raises(capi.TrgError) as e:
            morph.apply(g, bad, SS.scene_a_bones(2))
        assert e.value.code == -22 and "target 2" in str(e.value)
    finally:
        morph.release(g)
        refit.release(g)
        g.close()
        morph.release(c)
        _close(c, refit)


def test_plugin_morph_option(capi, morph, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png bulge=0.05 morph, and the same with twist=5: HipRenderer::bindMorph once, poseMorph before every call but
    the first -- exit 0, "3 morphs applied" as the last line, and the picture the same sequence through the C ABI writes.  bulge=0 morph: nothing
    applied, the plain run's picture.  Together with refit, pose or skin: refused."""
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 64, 48, 4, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba(), r.stdout
    still = run("still.png")
    zero, out = run("zero.png", "bulge=0", "morph")
    assert out.strip().splitlines()[-1] == "0 morphs applied" and np.array_equal(zero, still[0]) and "morphs" not in still[1]
    b = host.Scene.cornell_box().buffers()
    first, ev, dp = MS.cornell_bulge(b)
    ids, wts, nb, axis = SS.cornell_binding(b)
    for twist in (None, 5.0):
        extra = () if twist is None else ("twist=%g" % twist,)
        pic, out = run("morph%d.png" % (twist is not None), "bulge=0.05", *extra, "morph")
        assert out.strip().splitlines()[-1] == "%d morphs applied" % (frames - 1) and "refused" not in out
        assert not np.array_equal(pic, still[0])
        c = capi.Context(w, h)
        try:
            c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            c.set_uniforms(host.uniforms(w, h)[0])
            c.set_pixel_offsets_seed()
            skin_args = {} if twist is None else dict(bone_ids=ids, bone_weights=wts, n_bones=nb)
            morph.bind(c, b["positions"], b["normals"], b["indices"], first, ev, dp, None, **skin_args)
            for k in range(frames):
                if k:
                    morph.apply(c, np.array([np.float32(k) * np.float32(0.05)], np.float32), None if twist is None else MS.cornell_app_bones(b, twist * k))
                c.render(k, 1, bounces)
            c.sync()
            assert np.array_equal(c.postprocess(flip_y=True), pic)
        finally:
            morph.release(c)
            c.close()
    for other in ("pose", "refit", "skin"):
        assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "bulge=0.05", "morph", other], capture_output=True, timeout=120).returncode != 0
