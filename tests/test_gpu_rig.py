"""GPU tests (-m gpu) of the rig unit (include/trg_rig.h): a keyframed joint forest evaluated on the device -- against rig_reference bit for bit --,
and its bones fed to the skin and morph bindings without leaving the device -- against trg_skin_apply / trg_morph_apply given the read-back bones on
a twin context (positions, normals, trg_refit_last, strict frames and traces bit for bit), against skin_reference, the CPU oracle and the shipped
build's bars.  Images 32 x 24 (64 x 48 for the Cornell box), 2 spp, 3 bounces; traces 4,096 random rays -- the sizes and bars of
tests/test_gpu_refit.py.  Rig A keeps every box and quad leaf of scene A: tests/test_rig_host.py checks that on the CPU.  Nothing here provokes a
fault: every refusal is decided on the host or from the refit's flag words before anything is written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import morph_scenes as MS
from tests import refit_scenes as RS
from tests import rig_scenes as GS
from tests import skin_scenes as SS
from tests.test_gpu_pose import RAY_HI, RAY_LO, _device_bytes, _fresh_trace_equal
from tests.test_gpu_refit import BOUNCES, H, HBM_KERNELS, SPP, W, _bits, _close, _ctx, _rays, _shipped_bars, _strict_bars

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
def morph(built):
    from toyraygun_amd import morph as m
    m.load()
    return m


@pytest.fixture(scope="module")
def rig(built):
    from toyraygun_amd import rig as r
    r.load()
    return r


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


@pytest.fixture(scope="module")
def rig_a():
    """Rig A and its bones under every clock vector (rig_reference); shared and left unchanged."""
    r = GS.rig_a()
    return r, {name: GS.reference(r, clocks)[0] for name, clocks in GS.CLOCKS_A.items()}


def _bind_skin(skin, c, b, binding):
    skin.bind(c, b["positions"], b["normals"], b["indices"], binding[0], binding[1], SS.N_BONES)


def _strict_state(capi, c, rays):
    c.set_option(capi.OPT_STRICT, 1)
    c.render(0, SPP, BOUNCES)
    img, tr = c.read_accum(), c.trace(rays)
    c.set_option(capi.OPT_STRICT, 0)
    return img, tr


def _same_state(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def _last(refit, c):
    info = dict(refit.refit_last(c))
    info.pop("ms")
    return info


def _through_torch(address, n_floats):
    """Device memory at `address` copied into a torch tensor on the device, then to the host."""
    import torch
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    t = torch.empty(n_floats, dtype=torch.float32, device="cuda:0")
    assert hip.hipMemcpy(t.data_ptr(), address, n_floats * 4, 3) == 0          # hipMemcpyDeviceToDevice
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------- 1. evaluation
def test_rig_b_evaluates_to_the_bits_of_rig_reference(capi, rig):
    """700 joints on 12 levels -- launches of 5, 257 (a block and one thread), 300 (two blocks), ..., 1 joints --, no scene loaded: bones and world
    after every clock vector are rig_reference's bit for bit, a second evaluation gives the same bits, and the device buffers hold those bytes."""
    r = GS.rig_b()
    c = capi.Context(W, H)
    try:
        L = rig.load()
        assert L.trg_rig_evaluate(c.h_ctx, np.zeros(5, np.float32).ctypes.data) == -22       # evaluate without bind
        assert b"trg_rig_bind" in L.trg_last_error(c.h_ctx)
        rig.bind(c, *GS.args(r))
        with pytest.raises(capi.TrgError) as e:                                  # bound, never evaluated: nothing to read
            rig.read(c)
        assert e.value.code == -22 and "evaluated" in str(e.value)
        for name, clocks in GS.clocks_b(r).items():
            want_b, want_w = GS.reference(r, clocks)
            for again in range(2):
                rig.evaluate(c, clocks)
                bones, world = rig.read(c)
                assert np.array_equal(_bits(bones), _bits(want_b)), (name, again)
                assert np.array_equal(_bits(world), _bits(want_w)), (name, again)
            p = rig.buffers(c)
            assert p["bones"] % 16 == 0 and p["world"] % 16 == 0
            assert np.array_equal(_bits(_through_torch(p["bones"], 700 * 12)), _bits(want_b).reshape(-1)), name
            assert np.array_equal(_bits(_through_torch(p["world"], 700 * 12)), _bits(want_w).reshape(-1)), name
        no_inv = dict(r, inv_bind=None)                                          # without inverse binds the bones are the world's bits
        rig.bind(c, *GS.args(no_inv))
        rig.evaluate(c, GS.clocks_b(r)["mixed"])
        bones, world = rig.read(c)
        assert np.array_equal(_bits(bones), _bits(world)) and np.array_equal(_bits(world), _bits(GS.reference(no_inv, GS.clocks_b(r)["mixed"])[1]))
    finally:
        rig.release(c)
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------- 2. scene A animated
@pytest.mark.parametrize("gpu_build, indexed", [(0, False), (0, True), (1, False)], ids=["host-built", "host-built-indexed", "binned"])
def test_scene_a_animated(capi, refit, skin, rig, O, rest, rig_a, gpu_build, indexed):
    """Scene A's 38 bones from rig A: trg_skin_read after skin_apply(clocks) is skin_reference of rig_reference's bones; a twin context given the
    READ-BACK bones through plain trg_skin_apply agrees on everything; then the oracle's bars."""
    b, binding = rest[1] if indexed else rest[0]
    r, bones_of = rig_a
    rays = _rays(O, 251 + gpu_build, RAY_LO, RAY_HI)
    P, Q = _ctx(capi, O, b, gpu_build), _ctx(capi, O, b, gpu_build)
    try:
        rig.bind(P, *GS.args(r))
        for c in (P, Q):
            _bind_skin(skin, c, b, binding)
        for name in ("on a key", "between"):
            rig.skin_apply(P, GS.CLOCKS_A[name])
            bones, _ = rig.read(P)
            assert np.array_equal(_bits(bones), _bits(bones_of[name])), name
            pos, nrm = skin.read(P)
            ref_pos, ref_nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], binding[0], binding[1], bones_of[name])
            assert np.array_equal(_bits(pos), _bits(ref_pos)) and np.array_equal(_bits(nrm), _bits(ref_nrm)), name
            skin.apply(Q, bones)
            q_pos, q_nrm = skin.read(Q)
            assert np.array_equal(_bits(pos), _bits(q_pos)) and np.array_equal(_bits(nrm), _bits(q_nrm)), name
            assert _last(refit, P) == _last(refit, Q) and refit.refit_last(P)["path"] == refit.DEVICE
            assert _same_state(_strict_state(capi, P, rays), _strict_state(capi, Q, rays)), name
        if gpu_build == 0:
            info = refit.refit_last(P)
            assert info["n_boxes"] == RS.N_CUBES + 1 and info["n_quads"] == 1 + 6 * RS.N_CUBES
        moved = RS.unindexed(SS.posed_buffers(b, pos, nrm)) if indexed else SS.posed_buffers(b, pos, nrm)
        scene = RS.oracle_scene(O, moved)
        what = "animated scene A, builder %d indexed %d" % (gpu_build, indexed)
        _strict_bars(capi, O, P, scene, rays, what, kernels=HBM_KERNELS if not indexed else HBM_KERNELS[:1])
        if not indexed:
            _fresh_trace_equal(capi, O, P, moved, rays, gpu_build, what)
            _shipped_bars(capi, O, P, scene, moved, rays, what, gpu_build)
    finally:
        rig.release(P)
        for c in (P, Q):
            skin.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 3. morph
def test_morph_apply_from_the_rig_is_trg_morph_apply_with_the_read_back_bones(capi, refit, morph, rig, O, rest, rig_a):
    """tests/morph_scenes.py's binding (seven targets, normal deltas, scene A's bones behind them): morph_apply(weights, clocks) against
    trg_morph_apply with the bones trg_rig_read returns -- positions, normals, trg_refit_last, strict frame and trace."""
    b, binding = rest[0]
    r, bones_of = rig_a
    t = MS.targets(b)
    rays = _rays(O, 261, RAY_LO, RAY_HI)
    P, Q = _ctx(capi, O, b, 1), _ctx(capi, O, b, 1)
    try:
        rig.bind(P, *GS.args(r))
        for c in (P, Q):
            morph.bind(c, b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], bone_ids=binding[0], bone_weights=binding[1], n_bones=SS.N_BONES)
        for tw, name in (("a", "between"), ("b", "mixed")):
            rig.morph_apply(P, MS.weights(tw), GS.CLOCKS_A[name])
            bones, _ = rig.read(P)
            assert np.array_equal(_bits(bones), _bits(bones_of[name]))
            morph.apply(Q, MS.weights(tw), bones)
            (pos, nrm), (q_pos, q_nrm) = morph.read(P), morph.read(Q)
            assert np.array_equal(_bits(pos), _bits(q_pos)) and np.array_equal(_bits(nrm), _bits(q_nrm))
            assert (pos != b["positions"]).any() and _last(refit, P) == _last(refit, Q)
            assert _same_state(_strict_state(capi, P, rays), _strict_state(capi, Q, rays))
        # a morph binding WITHOUT bones has nothing a rig could drive
        morph.bind(P, b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3])
        with pytest.raises(capi.TrgError) as e:
            rig.morph_apply(P, MS.weights("a"), GS.CLOCKS_A["between"])
        assert e.value.code == -22 and "no bones" in str(e.value)
    finally:
        rig.release(P)
        for c in (P, Q):
            morph.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 4. caller-owned bones
def test_device_forms_equal_the_host_forms_and_refuse_what_is_no_device_memory(capi, refit, skin, morph, rig, O, rest, rig_a):
    """Bones in a torch tensor on the context's device: skin_apply_device / morph_apply_device against trg_skin_apply / trg_morph_apply with the
    same values.  A HOST pointer is refused by the runtime's own records, nothing enqueued: scene, current and previous pose stay.  A tensor of the
    wrong dtype or count raises in Python."""
    import torch
    b, binding = rest[0]
    nv = b["positions"].shape[0]
    _, bones_of = rig_a
    t = MS.targets(b)
    rays = _rays(O, 271, RAY_LO, RAY_HI)
    P, Q = _ctx(capi, O, b, 1), _ctx(capi, O, b, 1)
    try:
        for c in (P, Q):
            _bind_skin(skin, c, b, binding)
            morph.bind(c, b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], bone_ids=binding[0], bone_weights=binding[1], n_bones=SS.N_BONES)
        for name in ("between", "past"):
            dev = torch.from_numpy(bones_of[name].copy()).to("cuda:0")
            torch.cuda.synchronize()
            rig.skin_apply_device(P, dev)
            skin.apply(Q, bones_of[name])
            (pos, nrm), (q_pos, q_nrm) = skin.read(P), skin.read(Q)
            assert np.array_equal(_bits(pos), _bits(q_pos)) and np.array_equal(_bits(nrm), _bits(q_nrm)) and _last(refit, P) == _last(refit, Q)
            assert _same_state(_strict_state(capi, P, rays), _strict_state(capi, Q, rays))
        dev = torch.from_numpy(bones_of["mixed"].copy()).to("cuda:0")
        torch.cuda.synchronize()
        rig.morph_apply_device(P, MS.weights("a"), dev)
        morph.apply(Q, MS.weights("a"), bones_of["mixed"])
        (pos, nrm), (q_pos, q_nrm) = morph.read(P), morph.read(Q)
        assert np.array_equal(_bits(pos), _bits(q_pos)) and np.array_equal(_bits(nrm), _bits(q_nrm)) and _last(refit, P) == _last(refit, Q)

        def state():
            p = skin.buffers(P)
            frame = _strict_state(capi, P, rays)
            P.sync()
            return frame, p, [_device_bytes(p[k], n) for k, n in (("pos", nv * 12), ("nrm", NT * 36), ("prev_pos", nv * 12), ("prev_nrm", NT * 36))], _last(refit, P)
        skin.apply(P, bones_of["between"])                                      # (the skin binding defines the scene again)
        before = state()
        host = np.ascontiguousarray(bones_of["past"])
        L = rig.load()
        for call in (lambda: L.trg_rig_skin_apply_device(P.h_ctx, host.ctypes.data), lambda: L.trg_rig_skin_apply_device(P.h_ctx, None),
                     lambda: L.trg_rig_morph_apply_device(P.h_ctx, MS.weights("a").ctypes.data, host.ctypes.data)):
            assert call() == -22
            print(L.trg_last_error(P.h_ctx).decode())
            assert b"trg_rig_" in L.trg_last_error(P.h_ctx)
            after = state()
            assert _same_state(after[0], before[0]) and after[1] == before[1] and all(np.array_equal(m, n) for m, n in zip(after[2], before[2])) and after[3] == before[3]
        with pytest.raises(TypeError):
            rig.skin_apply_device(P, dev.double())
        with pytest.raises(TypeError):
            rig.skin_apply_device(P, bones_of["past"])
        with pytest.raises(ValueError):
            rig.skin_apply_device(P, dev[:37])
        with pytest.raises(ValueError):
            rig.morph_apply_device(P, MS.weights("a"), dev.reshape(-1)[:-1].clone())
        with pytest.raises(ValueError):
            rig.skin_apply_device(P, dev.cpu())
    finally:
        for c in (P, Q):
            skin.release(c)
            morph.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 5. sequences
def test_applies_pose_the_rest_geometry_and_the_previous_pose_is_kept(capi, refit, skin, rig, O, rest, rig_a):
    """Clocks C1 then C2: the current pose is skin(rest, bones(C2)), not applied on top of the first; the previous buffers hold the first."""
    b, binding = rest[1]
    nv = b["positions"].shape[0]
    r, bones_of = rig_a
    ref = [skin.skin_reference(b["positions"], b["normals"], b["indices"], binding[0], binding[1], bones_of[n]) for n in ("on a key", "between", "past")]
    c = _ctx(capi, O, b)
    try:
        rig.bind(c, *GS.args(r))
        _bind_skin(skin, c, b, binding)
        rig.skin_apply(c, GS.CLOCKS_A["on a key"])
        rig.skin_apply(c, GS.CLOCKS_A["between"])
        p = skin.buffers(c)
        c.sync()
        pos, nrm = skin.read(c)
        assert np.array_equal(_bits(pos), _bits(ref[1][0])) and np.array_equal(_bits(nrm), _bits(ref[1][1]))
        assert np.array_equal(_device_bytes(p["prev_pos"], nv * 12), ref[0][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["prev_nrm"], NT * 36), ref[0][1].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(p["pos"], nv * 12), ref[1][0].view(np.uint8).reshape(-1))
        rig.skin_apply(c, GS.CLOCKS_A["past"])
        q = skin.buffers(c)
        c.sync()
        assert q["prev_pos"] == p["pos"] and q["pos"] not in (p["pos"], p["prev_pos"])
        assert np.array_equal(_device_bytes(q["prev_pos"], nv * 12), ref[1][0].view(np.uint8).reshape(-1))
        assert np.array_equal(_device_bytes(q["pos"], nv * 12), ref[2][0].view(np.uint8).reshape(-1))
    finally:
        rig.release(c)
        skin.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 6. 7. refusals
def test_bind_refusals_are_the_validator_cases_and_an_earlier_rig_stays(capi, rig):
    r = GS.rig_a()
    c = capi.Context(W, H)
    try:
        rig.bind(c, *GS.args(r))
        rig.evaluate(c, GS.CLOCKS_A["between"])
        want = rig.read(c)
        for name, (bad, what, joint, key, word) in GS.bad_rigs(r).items():
            with pytest.raises(capi.TrgError) as e:
                rig.bind(c, *GS.args(bad))
            print("%s: %s" % (name, e.value))
            assert e.value.code == -22 and word in str(e.value), (name, str(e.value))
            assert joint is None or "joint %d " % joint in str(e.value), (name, str(e.value))
            assert key is None or "key %d " % key in str(e.value), (name, str(e.value))
        with pytest.raises(capi.TrgError) as e:
            rig.bind(c, *GS.args(GS.deep_rig(65)))
        assert e.value.code == -34 and "joint 64 " in str(e.value)
        rig.evaluate(c, GS.CLOCKS_A["between"])                                 # the earlier rig is still bound, and evaluates to the same bits
        got = rig.read(c)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
        rig.bind(c, *GS.args(GS.deep_rig(64)))                                  # 64 levels: 64 launches
        rig.evaluate(c, [0.5])
        bones, world = rig.read(c)
        want = GS.reference(GS.deep_rig(64), [0.5])
        assert np.array_equal(_bits(bones), _bits(want[0])) and np.array_equal(_bits(world), _bits(want[1])) and world[63, 3] > 0.63
        rig.release(c)
        with pytest.raises(capi.TrgError):
            rig.buffers(c)
    finally:
        rig.release(c)
        c.close()


def test_refused_applies_leave_scene_and_poses_as_they_were(capi, refit, skin, rig, O, rest, rig_a):
    """On the host-built tree.  No rig; no skin; a rig of another joint count; a NaN clock; cube 9's corners split between two bones, which is no
    box under rig A (TRG_ERR_RANGE from the refit's flag words, before anything is written); a binding made stale by a reload.  Each leaves the
    strict frame, the trace, the current and the previous pose and trg_refit_last bit for bit what they were."""
    b = rest[0][0]
    binding = SS.scene_a_binding(b, split_cube=9)
    nv = b["positions"].shape[0]
    r, _ = rig_a
    rays = _rays(O, 281, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, 0)
    try:
        loaded = _strict_state(capi, c, rays), refit.refit_last(c)

        def scene_unchanged(name, was):
            assert _same_state(_strict_state(capi, c, rays), was[0]) and refit.refit_last(c) == was[1], name
        with pytest.raises(capi.TrgError) as e:                                  # no rig (and no skin)
            rig.skin_apply(c, GS.CLOCKS_A["between"])
        assert e.value.code == -22 and "trg_rig_bind" in str(e.value)
        scene_unchanged("no rig", loaded)
        rig.bind(c, *GS.args(r))
        with pytest.raises(capi.TrgError) as e:                                  # no skin
            rig.skin_apply(c, GS.CLOCKS_A["between"])
        assert e.value.code == -22 and "trg_skin_bind" in str(e.value)
        scene_unchanged("no skin", loaded)
        _bind_skin(skin, c, b, binding)
        skin.apply(c, SS.scene_a_bones(2, share=(10, 11)))
        skin.apply(c, SS.scene_a_bones(3, share=(10, 11)))
        good = refit.refit_last(c)
        assert good["path"] == refit.DEVICE and good["n_boxes"] == RS.N_CUBES + 1

        def state():
            frame = _strict_state(capi, c, rays)
            p = skin.buffers(c)
            c.sync()
            return frame, p, [_device_bytes(p[k], n) for k, n in (("pos", nv * 12), ("nrm", NT * 36), ("prev_pos", nv * 12), ("prev_nrm", NT * 36))], skin.read(c)

        def unchanged(name, before):
            after = state()
            assert _same_state(after[0], before[0]) and after[1] == before[1] and all(np.array_equal(m, n) for m, n in zip(after[2], before[2])), name
            assert all(np.array_equal(_bits(m), _bits(n)) for m, n in zip(after[3], before[3])), name
            assert refit.refit_last(c) == good, name                             # every field, the time of the last accepted refit included
        before = state()
        nan = np.array(GS.CLOCKS_A["between"], np.float32)
        nan[1] = np.nan
        for name, clocks, code, text in (("split cube", GS.CLOCKS_A["between"], -34, "triangle"), ("nan clock", nan, -22, "clock 1")):
            with pytest.raises(capi.TrgError) as e:
                rig.skin_apply(c, clocks)
            print("%s: %s" % (name, e.value))
            assert e.value.code == code and text in str(e.value), (name, str(e.value))
            unchanged(name, before)
        rig.bind(c, *GS.args(GS.deep_rig(5)))                                   # five joints, 38 bones
        with pytest.raises(capi.TrgError) as e:
            rig.skin_apply(c, [0.5])
        assert e.value.code == -22 and "5 joints" in str(e.value) and "38 bones" in str(e.value)
        unchanged("joint count", before)
        rig.bind(c, *GS.args(r))
        b2 = RS.scene_a(1)
        c.load_scene(b2["positions"], b2["normals"], b2["colors"], b2["indices"], b2["material_ids"])      # a load makes the skin binding stale -- not the rig
        loaded = _strict_state(capi, c, rays), refit.refit_last(c)
        with pytest.raises(capi.TrgError) as e:
            rig.skin_apply(c, GS.CLOCKS_A["between"])
        assert e.value.code == -22 and "bind again" in str(e.value)
        scene_unchanged("stale binding", loaded)
        rig.evaluate(c, GS.CLOCKS_A["between"])                                  # the rig survived the load
        assert np.array_equal(_bits(rig.read(c)[0]), _bits(rig_a[1]["between"]))
    finally:
        rig.release(c)
        skin.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 8. the LDS tier
def _cornell_ctx(capi, O, b, w, h):
    c = capi.Context(w, h)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
    c.set_pixel_offsets(O.pixel_offsets(w, h))
    return c


def test_cornell_box_bends_through_the_rebuild_and_hands_its_previous_pose_to_the_denoiser(capi, refit, skin, rig, dn, O):
    """The Cornell box, LDS-resident, its short box on the app's chain: the rebuild path, the oracle's strict frame of the read-back geometry,
    and the unit's PREVIOUS buffers handed to trg_temporal_set_previous_scene_device give the host form's motion planes."""
    w, h = 64, 48
    b = RS.cornell_moved(O, 0)
    r, ids, wts = GS.cornell_chain(b, 15.0)
    c = _cornell_ctx(capi, O, b, w, h)
    try:
        assert c.stats().scene_in_lds == 1
        rig.bind(c, *GS.args(r))
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, wts, 4)
        rig.skin_apply(c, [0.5])
        first = skin.read(c)
        rig.skin_apply(c, [1.0])
        assert refit.refit_last(c)["path"] == refit.REBUILD and c.stats().scene_in_lds == 1
        pos, nrm = skin.read(c)
        ref_pos, ref_nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, wts, GS.reference(r, [1.0])[0])
        assert np.array_equal(_bits(pos), _bits(ref_pos)) and np.array_equal(_bits(nrm), _bits(ref_nrm))
        assert (pos[36:] == b["positions"][36:]).all() and (pos[:36] != b["positions"][:36]).any(1).sum() >= 18
        moved = SS.posed_buffers(b, pos, nrm)
        c.set_option(capi.OPT_STRICT, 1)
        c.render(0, SPP, BOUNCES)
        got = c.read_accum()
        c.set_option(capi.OPT_STRICT, 0)
        O.set_trig_mode(O.TRIG_PORTABLE)
        want, _ = O.render(RS.oracle_scene(O, moved), w, h, SPP, BOUNCES, offsets=O.pixel_offsets(w, h))
        O.set_trig_mode(O.TRIG_LIBM)
        assert np.array_equal(_bits(got), _bits(want))
        assert c.stats().bvh_room == 5                                           # the shipped LDS kernels test the room ahead of the tree: the strict build does not know it
        _shipped_bars(capi, O, c, RS.oracle_scene(O, moved), moved, _rays(O, 291, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0)), "bent cornell", w=w, h=h)
        dn.temporal_set_previous_scene(c, first[0], first[1], b["indices"])
        want = dn.guides_motion(c, 0)
        dn.temporal_set_previous_scene(c, None, None, None)
        p = skin.buffers(c)
        dn.temporal_set_previous_scene_device(c, p["prev_pos"], p["prev_nrm"], p["idx"], n_verts=108, n_tris=36)
        got = dn.guides_motion(c, 0)
        for a, e in zip(got, want):
            assert np.array_equal(_bits(a), _bits(e))
        assert (got[2][0, ..., 3] == 1).any()
    finally:
        rig.release(c)
        skin.release(c)
        dn.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 9. group
def test_group_applies_match_the_single_context(capi, refit, skin, morph, rig, O, rest, rig_a, monkeypatch):
    """Two contexts on one device, each rendering its band of the animated scene, gathered: the single context's frame."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    b, binding = rest[0]
    r, _ = rig_a
    u = O.uniforms_bytes(O.make_uniforms(W, H))
    c = capi.Context(W, H)
    g = capi.Group([0, 0], W, H)
    try:
        for x in (c, g):
            x.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            x.set_uniforms(u)
            x.set_pixel_offsets_seed()
            _bind_skin(skin, x, b, binding)
            rig.bind(x, *GS.args(r))
            rig.skin_apply(x, GS.CLOCKS_A["between"])
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.DEVICE
        c.render(0, SPP, BOUNCES)
        g.render(0, SPP, BOUNCES)
        g.sync()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(c.read_accum()))
        with pytest.raises(capi.TrgError) as e:
            rig.skin_apply(g, [0.5, np.inf])
        assert e.value.code == -22 and "clock 1" in str(e.value)
        # trg_group_rig_morph_apply: tests/morph_scenes.py's binding with scene A's bones behind it, on the group and on the single context
        t = MS.targets(b)
        for x in (c, g):
            morph.bind(x, b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], bone_ids=binding[0], bone_weights=binding[1], n_bones=SS.N_BONES)
            rig.morph_apply(x, MS.weights("a"), GS.CLOCKS_A["mixed"])
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.DEVICE
        want = morph.read(c)
        L = morph.load()
        for rank in range(2):                                                    # every context of the group holds the single context's pose
            pos, nrm = np.empty_like(want[0]), np.empty_like(want[1])
            assert L.trg_morph_read(L.trg_group_ctx(g.g, rank), pos.ctypes.data, nrm.ctypes.data) == 0
            assert np.array_equal(_bits(pos), _bits(want[0])) and np.array_equal(_bits(nrm), _bits(want[1]))
        c.render(0, SPP, BOUNCES)
        g.render(0, SPP, BOUNCES)
        g.sync()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(c.read_accum()))
        assert (want[0] != skin.read(c)[0]).any()                                # (and it is another pose than the skin's above)
    finally:
        rig.release(g)
        morph.release(g)
        morph.release(c)
        skin.release(g)
        refit.release(g)
        g.close()
        rig.release(c)
        skin.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- 10. the app
def test_plugin_rig_option(capi, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png bend=5 rig: HipRenderer::bindSkin and bindRig once, animateSkin before every call but the first, plain
    and with denoise=5,temporal: exit 0, "3 rigs applied" as the last line, a picture that differs from the still one -- and in plain mode equals,
    byte for byte, the one from the same calls driven through the C ABI with tests/rig_scenes.py's Cornell chain.  bend=0: the still picture.
    Together with skin, pose, morph, refit or slide=D: refused."""
    from toyraygun_amd import host, rig, skin
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 64, 48, 4, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba(), r.stdout
    still = {False: run("still.png"), True: run("still_t.png", "denoise=5,temporal")}
    bent = {}
    for temporal in (False, True):
        extra = ("denoise=5,temporal",) if temporal else ()
        bent[temporal], out = run("rig%d.png" % temporal, *extra, "bend=5", "rig")
        assert out.strip().splitlines()[-1] == "%d rigs applied" % (frames - 1) and "refused" not in out
        assert not np.array_equal(bent[temporal], still[temporal][0])
        zero, out = run("zero%d.png" % temporal, *extra, "bend=0", "rig")         # no bend: bound, nothing applied
        assert out.strip().splitlines()[-1] == "0 rigs applied"
        assert np.array_equal(zero, still[temporal][0])
    assert "rigs" not in still[False][1]
    b = host.Scene.cornell_box().buffers()
    r, ids, wts = GS.cornell_chain(b, 5.0 * (frames - 1))
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, wts, 4)
        rig.bind(c, *GS.args(r))
        for k in range(frames):
            if k:
                rig.skin_apply(c, [k / (frames - 1)])
            c.render(k, 1, bounces)
        c.sync()
        assert np.array_equal(c.postprocess(flip_y=True), bent[False])
    finally:
        rig.release(c)
        skin.release(c)
        c.close()
    for other in ("skin", "pose", "morph", "refit", "slide=0.1"):                # (a slid box is a reloaded scene: the skin binding would be stale)
        assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "bend=5", "rig", other], capture_output=True, timeout=120).returncode != 0
