"""GPU tests (-m gpu) of the pose unit (include/trg_pose.h): a loaded scene posed on the device -- per-object transforms, and a refit from buffers that
are on the device already -- against pose_reference (bit for bit), against the CPU oracle's render of the read-back geometry (bit for bit in the
strict build, whatever tree the refit leaves; inside the shipped build's bar otherwise), against trg_refit_scene from the same arrays and against a
fresh trg_load_scene.  Images 32 x 24, 2 spp, 3 bounces; traces 4,096 random rays -- the sizes of tests/test_gpu_refit.py, whose bars these are.
The poses keep every box and quad leaf of scene A: tests/test_pose_host.py checks that on the CPU.  Nothing here provokes a fault: every refusal
is decided on the host or from flag words before anything is written."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import pose_scenes as PS
from tests import refit_scenes as RS
from tests.test_gpu_refit import BOUNCES, H, HBM_KERNELS, SPP, W, _bits, _close, _ctx, _rays, _shipped_bars, _strict_bars, _textures

pytestmark = pytest.mark.gpu
RAY_LO, RAY_HI = (-1.4, 0.02, -1.4), (1.4, 2.2, 3.0)       # the posed cubes wander up to 0.3 from where scene A has them


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
    """Scene A as loaded -- per corner and indexed -- shared and left unchanged."""
    return RS.scene_a(0), RS.scene_a_indexed(0)


def _device_bytes(address, nbytes):
    """A copy of device memory at `address` (what trg_pose_buffers hands out), through the HIP runtime the library itself is linked against."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, address, nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _read(pose, c, b, normals=True):
    return pose.read(c, b["positions"].shape[0], b["material_ids"].shape[0], normals)


def _posed(pose, c, b, x, first):
    """apply + read, checked against pose_reference bit for bit; returns the buffer dict of the read-back geometry."""
    pose.apply(c, x)
    pos, nrm = _read(pose, c, b)
    ref_pos, ref_nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], first, x)
    assert np.array_equal(_bits(pos), _bits(ref_pos)) and np.array_equal(_bits(nrm), _bits(ref_nrm))
    return PS.posed_buffers(b, pos, nrm)


def _fresh_trace_equal(capi, O, c, moved, rays, gpu_build, what):
    """Strict build: trg_trace of the posed context against a context that freshly loaded the read-back geometry, every ray, every byte."""
    fresh = _ctx(capi, O, moved, gpu_build)
    try:
        for x in (c, fresh):
            x.set_option(capi.OPT_STRICT, 1)
        assert np.array_equal(c.trace(rays).view(np.uint8), fresh.trace(rays).view(np.uint8)), what
    finally:
        c.set_option(capi.OPT_STRICT, 0)
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------- scene A posed
@pytest.mark.parametrize("gpu_build", [0, 1, 2, 3], ids=["host-built", "binned", "lbvh", "ploc"])
def test_scene_a_posed(capi, refit, pose, O, rest, gpu_build):
    """706 triangles in HBM; 2,118 vertices = 8 blocks of 256 + 70, 6,354 corner normals; objects of 2, 12 and 320 triangles.  Host-built (box
    leaves: every cube and the floor must survive the refit's checks) and the three device builders."""
    b = rest[0]
    first = PS.scene_a_first()
    rays = _rays(O, 51 + gpu_build, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, gpu_build)
    try:
        assert c.stats().scene_in_lds == 0
        pose.bind(c, b["positions"], b["normals"], b["indices"], first)
        pos, nrm = _read(pose, c, b)
        assert np.array_equal(_bits(pos), _bits(b["positions"])) and np.array_equal(_bits(nrm), _bits(b["normals"]))   # bound: the rest pose
        assert refit.refit_last(c)["path"] == refit.NONE                                                                 # bind does not refit
        moved = _posed(pose, c, b, PS.scene_a_xforms(1 + gpu_build), first)
        info = refit.refit_last(c)
        assert info["path"] == refit.DEVICE and info["n_records"] == 706
        if gpu_build == 0:
            assert info["n_boxes"] == RS.N_CUBES + 1 and info["n_quads"] == 1 + 6 * RS.N_CUBES
        assert np.array_equal(np.array(info["lo"], np.float32), moved["positions"].min(0)) and np.array_equal(np.array(info["hi"], np.float32), moved["positions"].max(0))
        scene = RS.oracle_scene(O, moved)
        what = "posed scene A, builder %d" % gpu_build
        _strict_bars(capi, O, c, scene, rays, what)
        _fresh_trace_equal(capi, O, c, moved, rays, gpu_build, what)
        _shipped_bars(capi, O, c, scene, moved, rays, what, gpu_build)
    finally:
        pose.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- device buffers
@pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
def test_refit_scene_device_is_refit_scene_without_the_upload(capi, refit, pose, O, rest, indexed):
    """Scene A moved to step 2 (the indexed one: a shuffled vertex buffer and a far-away vertex that no triangle names), handed over as torch tensors,
    against trg_refit_scene with the same arrays on a twin context: trg_refit_info field for field (ms aside), strict frames and trace records bit for
    bit.  Indices as int32, the dtype torch has everywhere."""
    import torch
    b0 = rest[1] if indexed else rest[0]
    b = RS.scene_a_indexed(2) if indexed else RS.scene_a(2)
    rays = _rays(O, 61)
    dev, twin = _ctx(capi, O, b0), _ctx(capi, O, b0)
    try:
        t_pos = torch.from_numpy(b["positions"]).cuda()
        t_nrm = torch.from_numpy(b["normals"]).cuda()
        t_idx = torch.from_numpy(b["indices"].view(np.int32)).cuda()
        torch.cuda.synchronize()
        pose.refit_scene_device(dev, t_pos, t_nrm, t_idx)
        refit.refit_scene(twin, b["positions"], b["normals"], b["indices"])
        a, t = refit.refit_last(dev), refit.refit_last(twin)
        assert a["path"] == refit.DEVICE and {k: v for k, v in a.items() if k != "ms"} == {k: v for k, v in t.items() if k != "ms"}
        for c in (dev, twin):
            c.set_option(capi.OPT_STRICT, 1)
            c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(dev.read_accum()), _bits(twin.read_accum()))
        assert np.array_equal(dev.trace(rays).view(np.uint8), twin.trace(rays).view(np.uint8))
        # without normals the loaded ones stay, on both
        pose.refit_scene_device(dev, t_pos, None, t_idx)
        refit.refit_scene(twin, b["positions"], None, b["indices"])
        for c in (dev, twin):
            c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(dev.read_accum()), _bits(twin.read_accum()))
        assert np.array_equal(t_pos.cpu().numpy().view(np.uint32), _bits(b["positions"]))      # the caller's tensor is read, not written
    finally:
        _close(dev, refit)
        _close(twin, refit)


def test_device_pointers_are_checked_before_anything_is_enqueued(capi, refit, pose, O, rest):
    import torch
    b0, b = rest[0], RS.scene_a(1)
    L = pose.load()
    c = _ctx(capi, O, b0)
    try:
        t_pos, t_nrm = torch.from_numpy(b["positions"]).cuda(), torch.from_numpy(b["normals"]).cuda()
        t_idx = torch.from_numpy(b["indices"].view(np.int32)).cuda()
        torch.cuda.synchronize()
        nv, nt = b["positions"].shape[0], 706
        c.render(0, SPP, BOUNCES)
        before = c.read_accum()

        def refused(call, text=None):
            rc = call()
            msg = (L.trg_last_error(c.h_ctx) or b"").decode()
            print(rc, msg)
            assert rc == -22 and (text is None or text in msg), (rc, msg)
            c.render(0, SPP, BOUNCES)
            assert np.array_equal(_bits(c.read_accum()), _bits(before))
        # host memory in each place
        refused(lambda: L.trg_refit_scene_device(c.h_ctx, b["positions"].ctypes.data, t_nrm.data_ptr(), t_idx.data_ptr(), nv, nt), "positions")
        refused(lambda: L.trg_refit_scene_device(c.h_ctx, t_pos.data_ptr(), b["normals"].ctypes.data, t_idx.data_ptr(), nv, nt), "normals")
        refused(lambda: L.trg_refit_scene_device(c.h_ctx, t_pos.data_ptr(), None, b["indices"].ctypes.data, nv, nt), "indices")
        # (sizes are the caller's responsibility at the C ABI -- include/trg_pose.h says why --; pose.refit_scene_device checks the element counts
        # of its tensors, and a positions tensor too short for the indices is refused by the refit's own index check: both below)
        refused(lambda: L.trg_refit_scene_device(c.h_ctx, t_pos.data_ptr(), None, t_idx.data_ptr(), nv, 705), "706")
        # a positions tensor with fewer vertices than the indices name: refused by the refit's own index check, naming the triangle
        with pytest.raises(capi.TrgError) as e:
            pose.refit_scene_device(c, t_pos[:2100].contiguous(), None, t_idx)
        assert e.value.code == -22 and "triangle 700" in str(e.value)
        for bad in (lambda: pose.refit_scene_device(c, t_pos, t_nrm[:-1], t_idx), lambda: pose.refit_scene_device(c, t_pos.double(), None, t_idx),
                    lambda: pose.refit_scene_device(c, t_pos.cpu(), None, t_idx), lambda: pose.refit_scene_device(c, t_pos.t(), None, t_idx),
                    lambda: pose.refit_scene_device(c, b["positions"], None, t_idx), lambda: pose.refit_scene_device(c, t_pos, None, t_idx.long())):
            with pytest.raises((TypeError, ValueError)):
                bad()
        c.render(0, SPP, BOUNCES)
        assert np.array_equal(_bits(c.read_accum()), _bits(before))
        pose.refit_scene_device(c, t_pos, t_nrm, t_idx)                      # and a good call still works
        assert refit.refit_last(c)["path"] == refit.DEVICE
    finally:
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- sequences
def test_poses_apply_to_the_rest_geometry_and_the_previous_pose_is_kept(capi, refit, pose, O, rest):
    """pose, then identity: the frame of a context that applied only the identity, bit for bit (a pose is a function of the rest geometry, not of
    the pose before).  Two applies: the `prev` buffers hold the first pose, the current ones the second; the indices are the bound ones."""
    b = rest[1]                                                               # the indexed scene: 422 vertices, two of them unnamed
    first = PS.scene_a_first()
    nv, nt = b["positions"].shape[0], 706
    ident = PS.identity(PS.N_OBJECTS_A)
    frames = []
    for path in ((PS.scene_a_xforms(1), ident), (ident,)):
        c = _ctx(capi, O, b)
        try:
            pose.bind(c, b["positions"], b["normals"], b["indices"], first)
            for x in path:
                pose.apply(c, x)
            c.render(0, SPP, BOUNCES)
            frames.append(c.read_accum())
            if len(path) == 2:
                p = pose.buffers(c)
                c.sync()
                first_pos, first_nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], first, path[0])
                assert np.array_equal(_device_bytes(p["prev_pos"], nv * 12), first_pos.view(np.uint8).reshape(-1))
                assert np.array_equal(_device_bytes(p["prev_nrm"], nt * 36), first_nrm.view(np.uint8).reshape(-1))
                assert np.array_equal(_device_bytes(p["idx"], nt * 12), b["indices"].view(np.uint8).reshape(-1))
                pos, nrm = _read(pose, c, b)
                assert np.array_equal(_device_bytes(p["pos"], nv * 12), pos.view(np.uint8).reshape(-1)) and (pos == b["positions"]).all()
                assert np.array_equal(_device_bytes(p["nrm"], nt * 36), nrm.view(np.uint8).reshape(-1))
                assert len({p["pos"], p["prev_pos"]}) == 2
        finally:
            pose.release(c)
            _close(c, refit)
    assert np.array_equal(_bits(frames[0]), _bits(frames[1]))


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_scene_and_poses_as_they_were(capi, refit, pose, O, rest):
    b, bi = rest
    first = PS.scene_a_first()
    nv, nt = b["positions"].shape[0], 706
    rays = _rays(O, 71, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b)
    try:
        with pytest.raises(capi.TrgError) as e:                                  # apply without bind
            pose.apply(c, PS.identity(PS.N_OBJECTS_A))
        assert e.value.code == -22 and "trg_pose_bind" in str(e.value)
        for name, (table, indexed) in PS.bad_tables().items():                   # each bad table (two of them need shared vertices: the indexed scene's
            x = bi if indexed else b                                              # arrays -- bind is refused on the host before it looks at the loaded scene's)
            with pytest.raises(capi.TrgError) as e:
                pose.bind(c, x["positions"], x["normals"], x["indices"], table)
            print("%s: %s" % (name, e.value))
            assert e.value.code == -22, name
            assert ("object" in str(e.value)) and (("vertex" in str(e.value)) == indexed), (name, str(e.value))
        bad = b["positions"].copy()
        bad[1234, 1] = np.inf
        with pytest.raises(capi.TrgError) as e:
            pose.bind(c, bad, b["normals"], b["indices"], first)
        assert e.value.code == -22 and "vertex 1234" in str(e.value)
        bad_idx = b["indices"].copy()
        bad_idx[3 * 400 + 1] = nv
        with pytest.raises(capi.TrgError) as e:
            pose.bind(c, b["positions"], b["normals"], bad_idx, first)
        assert e.value.code == -22 and "triangle 400" in str(e.value)
        with pytest.raises(capi.TrgError) as e:
            pose.bind(c, b["positions"], b["normals"], b["indices"], first, n_tris=705)
        assert e.value.code == -22 and "706" in str(e.value)
        with pytest.raises(capi.TrgError):                                       # still nothing bound
            pose.buffers(c)

        pose.bind(c, b["positions"], b["normals"], b["indices"], first)         # after every refusal the next valid call works
        x1 = PS.scene_a_xforms(1)
        pose.apply(c, PS.scene_a_xforms(2))
        pose.apply(c, x1)
        good = refit.refit_last(c)

        def state():
            c.set_option(capi.OPT_STRICT, 0)
            c.render(0, SPP, BOUNCES)
            img = c.read_accum()
            c.set_option(capi.OPT_STRICT, 1)
            tr = c.trace(rays)
            c.set_option(capi.OPT_STRICT, 0)
            p = pose.buffers(c)
            c.sync()
            mem = [_device_bytes(p[k], n) for k, n in (("pos", nv * 12), ("nrm", nt * 36), ("prev_pos", nv * 12), ("prev_nrm", nt * 36))]
            return img, tr, p, mem, _read(pose, c, b)
        before = state()
        collapsed = x1.copy()
        collapsed[1 + 9, :] = 0                                                  # cube 9 scaled to nothing: its faces are no quads, it is no box
        nan = x1.copy()
        nan[20, 7] = np.nan
        for name, x, code, text in (("zero scale", collapsed, -34, "triangle %d" % RS.cube_first_triangle(9)), ("nan", nan, -22, "object 20")):
            with pytest.raises(capi.TrgError) as e:
                pose.apply(c, x)
            print("%s: %s" % (name, e.value))
            assert e.value.code == code and text in str(e.value), (name, str(e.value))
            after = state()
            assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8)), name
            assert after[2] == before[2] and all(np.array_equal(m, n) for m, n in zip(after[3], before[3])), name
            assert all(np.array_equal(_bits(m), _bits(n)) for m, n in zip(after[4], before[4])), name
            assert refit.refit_last(c) == good
        moved = _posed(pose, c, b, PS.scene_a_xforms(3), first)                 # the next valid call works ...
        _strict_bars(capi, O, c, RS.oracle_scene(O, moved), rays, "after the refusals", kernels=HBM_KERNELS[:1])
        pose.release(c)                                                          # ... release unbinds, and only that
        with pytest.raises(capi.TrgError):
            pose.apply(c, x1)
        assert refit.refit_last(c)["path"] == refit.DEVICE
        pose.bind(c, b["positions"], b["normals"], b["indices"], first)
        b2 = RS.scene_a(1)
        c.load_scene(b2["positions"], b2["normals"], b2["colors"], b2["indices"], b2["material_ids"])      # a load makes the binding stale
        for call in (lambda: pose.apply(c, x1), lambda: _read(pose, c, b), lambda: pose.buffers(c)):
            with pytest.raises(capi.TrgError) as e:
                call()
            assert e.value.code == -22 and "bind again" in str(e.value)
        pose.bind(c, b["positions"], b["normals"], b["indices"], first)
        pose.apply(c, x1)
    finally:
        pose.release(c)
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- the LDS tier
def _box_turn(dx, angle, centre):
    """[2, 12]: the short box turned by `angle` about the vertical axis through `centre` and slid by dx along x; everything else stays."""
    A = RS._rot((0, 1, 0), angle)
    return np.stack([PS._about(A, centre, (dx, 0.0, 0.0)).reshape(12), np.eye(3, 4).reshape(12)]).astype(np.float32)


def test_small_scene_is_posed_through_the_rebuild_and_keeps_its_textures(capi, refit, pose, O):
    """The Cornell box, LDS-resident, its short box an object of its own, slid and turned: the buffers are downloaded and the host builder runs
    (REBUILD); strict frames are the oracle's of the read-back geometry bit for bit, in the LDS kernel and with TRG_OPT_FORCE_GLOBAL; textures on the
    short box and the floor survive."""
    rays = _rays(O, 81, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0))
    b = RS.cornell_moved(O, 0)
    first = np.array([0, 12, 36], np.uint32)
    centre = b["positions"][:36].astype(np.float64).mean(0)
    for tex in (None, _textures(36, 0, 14, 6)):
        c = _ctx(capi, O, b)
        try:
            assert c.stats().scene_in_lds == 1
            if tex:
                c.load_textures(*tex)
            pose.bind(c, b["positions"], b["normals"], b["indices"], first)
            for s in (1, 2):
                moved = _posed(pose, c, b, _box_turn(0.02 * s, 0.15 * s, centre), first)
                info = refit.refit_last(c)
                assert info["path"] == refit.REBUILD and c.stats().scene_in_lds == 1
                assert (moved["positions"][36:] == b["positions"][36:]).all() and (moved["positions"][:36] != b["positions"][:36]).any()
                scene = RS.oracle_scene(O, moved, tex)
                for force_global in (0, 1):
                    c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
                    _strict_bars(capi, O, c, scene, rays, "posed cornell step %d global %d" % (s, force_global), kernels=(("direct", 0, 1),))
                    if force_global == 0:                                    # the shipped LDS kernels test the room ahead of the tree: the strict build does not know it
                        assert c.stats().bvh_room == 5
                        _shipped_bars(capi, O, c, scene, moved, rays, "posed cornell step %d" % s)
                c.set_option(capi.OPT_FORCE_GLOBAL, 0)
        finally:
            pose.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- temporal
@pytest.mark.parametrize("force_global", [0, 1], ids=["lds", "hbm"])
def test_previous_scene_from_device_buffers_gives_the_host_forms_motion_planes(capi, dn, O, cornell, force_global):
    """trg_temporal_set_previous_scene_device on device copies of the arrays: M0 and M1 of trg_guides_render_motion bit for bit those after the host
    form, with and without previous normals; the refusals are the host form's."""
    import torch
    from tests.test_gpu_motion import moved_box
    from tests.util import make_ctx
    w, h = 64, 48
    b = cornell.buffers()
    prev = moved_box(b, 0.07, 0.35)
    t_pos, t_nrm = torch.from_numpy(prev["positions"]).cuda(), torch.from_numpy(prev["normals"]).cuda()
    t_idx = torch.from_numpy(np.ascontiguousarray(b["indices"], np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    c = make_ctx(O, cornell, w, h, offsets=O.pixel_offsets(w, h))
    try:
        c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
        for frame, normals in ((0, True), (3, False)):
            dn.temporal_set_previous_scene(c, prev["positions"], prev["normals"] if normals else None, b["indices"])
            want = dn.guides_motion(c, frame)
            dn.temporal_set_previous_scene(c, None, None, None)                  # forgotten: the next planes can only come from the device form
            dn.temporal_set_previous_scene_device(c, t_pos, t_nrm if normals else None, t_idx)
            got = dn.guides_motion(c, frame)
            for a, e in zip(got, want):
                assert np.array_equal(_bits(a), _bits(e)), (frame, normals)
            assert (got[2][0, ..., 3] == 1).any()
        with pytest.raises(capi.TrgError) as e:
            dn.temporal_set_previous_scene_device(c, t_pos, None, t_idx[:-3])    # another triangle count
        assert e.value.code == -22 and "36" in str(e.value)
        with pytest.raises(capi.TrgError):
            dn.temporal_set_previous_scene_device(c, None, None, t_idx, n_verts=108, n_tris=36)
        dn.temporal_set_previous_scene_device(c, None, None, None, n_verts=0, n_tris=0)   # forgets, like the host form
        with pytest.raises(capi.TrgError):
            dn.guides_motion(c, 0)
    finally:
        dn.release(c)
        c.close()


def _slide(k, d=0.02):
    x = PS.identity(2)
    x[0, 3] = np.float32(k * d)
    return x


def test_temporal_history_follows_the_poses_without_a_host_copy(capi, refit, pose, dn, O):
    """The short box sliding over five calls, as HipRenderer::poseObjects drives the C ABI: trg_pose_apply, the pose unit's PREVIOUS buffers to
    trg_temporal_set_previous_scene_device, trg_render_temporal -- against the same five calls with the read-back arrays through trg_refit_scene and
    the host form: every step's output bit for bit."""
    w, h, bounces = 64, 48, 3
    b = RS.cornell_moved(O, 0)
    first = np.array([0, 12, 36], np.uint32)

    def ctx():
        c = capi.Context(w, h)
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
        c.set_pixel_offsets(O.pixel_offsets(w, h))
        return c
    P, Q = ctx(), ctx()
    try:
        pose.bind(P, b["positions"], b["normals"], b["indices"], first)
        read = [(b["positions"], b["normals"])]
        for k in range(5):
            if k:
                pose.apply(P, _slide(k))
                p = pose.buffers(P)
                dn.temporal_set_previous_scene_device(P, p["prev_pos"], p["prev_nrm"], p["idx"], n_verts=108, n_tris=36)
                read.append(_read(pose, P, b))
                refit.refit_scene(Q, read[k][0], read[k][1], b["indices"])
                dn.temporal_set_previous_scene(Q, read[k - 1][0], read[k - 1][1], b["indices"])
            got, want = dn.render_temporal(P, k, 1, bounces, iterations=3), dn.render_temporal(Q, k, 1, bounces, iterations=3)
            assert np.array_equal(_bits(got), _bits(want)), k
        assert (read[4][0][:36, 0] != read[3][0][:36, 0]).all()
    finally:
        pose.release(P)
        for c in (P, Q):
            dn.release(c)
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- group, plugin
def test_group_poses_match_the_single_context(capi, refit, pose, O, rest, monkeypatch):
    """Two contexts on one device, each rendering its band of the posed scene, gathered: the single context's frame."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    b = rest[0]
    first = PS.scene_a_first()
    u = O.uniforms_bytes(O.make_uniforms(W, H))
    c = capi.Context(W, H)
    g = capi.Group([0, 0], W, H)
    try:
        for x in (c, g):
            x.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            x.set_uniforms(u)
            x.set_pixel_offsets_seed()
            pose.bind(x, b["positions"], b["normals"], b["indices"], first)
            pose.apply(x, PS.scene_a_xforms(2))
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.DEVICE
        c.render(0, SPP, BOUNCES)
        g.render(0, SPP, BOUNCES)
        g.sync()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(c.read_accum()))
        bad = PS.scene_a_xforms(2)
        bad[3, 0] = np.inf
        with pytest.raises(capi.TrgError) as e:
            pose.apply(g, bad)
        assert e.value.code == -22 and "object 3" in str(e.value)
    finally:
        pose.release(g)
        refit.release(g)
        g.close()
        pose.release(c)
        _close(c, refit)


def test_plugin_pose_option(capi, refit, pose, dn, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png slide=0.02 pose: HipRenderer::bindObjects once, poseObjects before every call but the first -- the picture
    of the same pose calls through the C ABI, plain and with denoise=5,temporal; the last line counts the poses; `refit` and plain slide= write what
    they wrote (each other's picture: tests/test_gpu_refit.py)."""
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 64, 48, 4, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba(), r.stdout
    pics = {False: run("pose.png", "slide=0.02", "pose"), True: run("pose_t.png", "denoise=5,temporal", "slide=0.02", "pose")}
    for pic, out in pics.values():
        assert out.strip().splitlines()[-1] == "%d poses applied" % (frames - 1) and "refused" not in out
    (re_pic, re_out), (plain, plain_out) = run("refit.png", "slide=0.02", "refit"), run("plain.png", "slide=0.02")
    assert np.array_equal(re_pic, plain) and "poses" not in re_out + plain_out and re_out.strip().splitlines()[-1].startswith("wrote")
    assert not np.array_equal(pics[False][0], run("still.png")[0])
    assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "slide=0.02", "pose", "refit"], capture_output=True, timeout=120).returncode != 0
    b = host.Scene.cornell_box().buffers()
    for temporal in (False, True):
        c = capi.Context(w, h)
        try:
            c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            c.set_uniforms(host.uniforms(w, h)[0])
            c.set_pixel_offsets_seed()
            pose.bind(c, b["positions"], b["normals"], b["indices"], np.array([0, 12, 36], np.uint32))
            den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            for k in range(frames):
                if k:
                    pose.apply(c, _slide(k))
                    assert refit.refit_last(c)["path"] == refit.REBUILD
                    if temporal:
                        p = pose.buffers(c)
                        dn.temporal_set_previous_scene_device(c, p["prev_pos"], p["prev_nrm"], p["idx"], n_verts=b["positions"].shape[0], n_tris=36)
                if temporal:
                    dn.render_temporal(c, k, 1, bounces, out=den, iterations=5)
                else:
                    c.render(k, 1, bounces)
            c.sync()
            if temporal:
                c.bind_accum(den.data_ptr())
            try:
                assert np.array_equal(c.postprocess(flip_y=True), pics[temporal][0]), temporal
            finally:
                c.bind_accum(None)
        finally:
            pose.release(c)
            dn.release(c)
            _close(c, refit)
