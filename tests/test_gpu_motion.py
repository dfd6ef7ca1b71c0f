"""GPU tests (-m gpu) of the temporal step for MOVING GEOMETRY (include/trg_denoise.h, "MOVING GEOMETRY"): the motion planes against
reference_motion, the motion form of the step against the plain one (identity planes: bit for bit) and against reference_temporal(motion=...) on
the moving stage of tests/test_motion_host.py, the armed trg_render_temporal end to end on a Cornell box whose short box slides, the refusals,
and the plugin's updateScene / slide=D.

The step is compared as tests/test_gpu_temporal_shapes.py compares it -- its _step / _ref / _compare / _finish are used as they are, the motion
planes travel in the parameter dict --: from the DEVICE's own previous history, E32 from the reference's float32 mode, bars max(1e-4, 4 E32) on
colour, N and the moments, max(1e-3, 4 E32) relative + 1e-9 on V_0, `near` pixels left out under the 1 % cap.  No call reaches N = 4."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _close
from tests.test_gpu_temporal import _filter_g0
from tests.test_gpu_temporal_shapes import _compare, _ctx, _finish, _ref, _step
from tests.test_motion_host import MOVING_CAMERAS, TIGHT, check_populations, identity_motion, motion_census, moving_frames
from tests.test_temporal_synthetic_host import SCHEDULE, schedule_frames
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
SHORT_BOX = 12                                   # the Cornell box's first twelve triangles (include/cornellBox.h)
SHORT_BOX_CENTRE = (0.3275, 0.0, 0.3725)


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


def moved_box(b, dx, angle=0.0):
    """The scene buffers `b` with the short box turned by `angle` about the vertical axis through its centre and moved by dx along x."""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    out = dict(b)
    pos, nrm = b["positions"].astype(np.float64), b["normals"].astype(np.float64)
    n = 3 * SHORT_BOX
    pos[:n] = (pos[:n] - SHORT_BOX_CENTRE) @ R.T + SHORT_BOX_CENTRE + (dx, 0.0, 0.0)
    nrm[:n] = nrm[:n] @ R.T
    out["positions"], out["normals"] = pos.astype(f32), nrm.astype(f32)
    return out


def _load(c, b):
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])


def _refused(capi, fn):
    with pytest.raises(capi.TrgError) as e:
        fn()
    assert e.value.code == capi.ERR_INVALID and len(str(e.value)) > len("trg error -22: "), str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------- 1. motion planes
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", [(64, 48), (17, 33)], ids=lambda s: "%dx%d" % s)
def test_motion_planes_are_the_previous_corners_at_the_hits_barycentrics(capi, dn, O, cornell, size, strict):
    """Cornell box, staged in LDS and traversed from HBM; the previous scene has the short box turned by 0.35 rad and moved by 0.07: M0, M1 bit for
    bit reference_motion of trg_raygen + trg_trace of the same frame index, zero on the misses, M0.w = 1 on the hits; G0, G1 and X are
    trg_guides_render_pos's; without previous normals M1.xyz is G0.xyz; the planes of the short box differ from X, the others do not."""
    import torch
    w, h = size
    b = cornell.buffers()
    prev = moved_box(b, 0.07, 0.35)
    c = make_ctx(O, cornell, w, h, offsets=O.pixel_offsets(w, h))
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for fg in (0, 1):
            c.set_option(capi.OPT_FORCE_GLOBAL, fg)
            for frame, normals in ((0, prev["normals"]), (3, None)):
                dn.temporal_set_previous_scene(c, prev["positions"], normals, b["indices"])
                g, X, m = dn.guides_motion(c, frame)
                g2, X2 = dn.guides_pos(c, frame)
                assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(X), _bits(X2))
                want = dn.reference_motion(c.trace(c.raygen(frame)), prev["positions"], normals, b["indices"], g[0])
                hit = g[0, ..., 3] >= 0
                assert np.array_equal(_bits(m), _bits(want)), (fg, frame, int((_bits(m) != _bits(want)).sum()))
                assert hit.any() and (m[:, ~hit] == 0).all() and (m[0][hit][:, 3] == 1).all() and (m[1, ..., 3] == 0).all()
                if normals is None:
                    assert np.array_equal(_bits(m[1, ..., :3][hit]), _bits(g[0, ..., :3][hit]))
                prim = np.ascontiguousarray(g[1, ..., 3]).view(np.int32)
                box = hit & (prim < SHORT_BOX)
                far = np.abs(m[0, ..., :3] - X[..., :3]).max(-1)
                assert box.sum() >= 4 and (far[box] > 0.02).all() and (far[hit & ~box] < 1e-5).all()
                if normals is not None:
                    assert (np.abs(m[1, ..., :3] - g[0, ..., :3]).max(-1)[box] > 0.05).mean() > 0.5
        gt, mt = (torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        xt = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        dn.guides_motion(c, 3, out=gt, pos=xt, motion=mt)
        c.sync()
        assert np.array_equal(_bits(mt.cpu().numpy()), _bits(m)) and np.array_equal(_bits(gt.cpu().numpy()), _bits(g)) and np.array_equal(_bits(xt.cpu().numpy()), _bits(X))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", [(1, 1), (9, 1), (16, 16), (17, 33)], ids=lambda s: "%dx%d" % s)
def test_identity_planes_give_the_plain_step_bit_for_bit(capi, dn, O, cornell, size, strict):
    """M0 = (X, 1), M1 = (G0.xyz, 0) in one context, trg_temporal_denoise in another, three calls of the synthetic schedule (no history, rest, the
    sub-pixel shift), two filter iterations: out, (I, V_0), V_N and the history are equal bit for bit after every call."""
    w, h = size
    (a, mats), (b, _) = (_ctx(O, cornell, w, h, capi, strict) for _ in range(2))
    try:
        for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, SCHEDULE[:3])):
            kw = dict(return_iv=True, return_variance=True, iterations=2)
            got = dn.temporal_denoise(a, colour, g, X, vp, motion=identity_motion(g, X), **kw) + (dn.temporal_history(a),)
            want = dn.temporal_denoise(b, colour, g, X, vp, **kw) + (dn.temporal_history(b),)
            for k, (x, y) in enumerate(zip(got, want)):
                assert np.array_equal(_bits(x), _bits(y)), (call, k, int((_bits(x) != _bits(y)).sum()))
            if call and w * h > 1:
                assert (got[3][0, ..., 3] > 1).any()                                                       # and history was found
    finally:
        _close(a, dn)
        _close(b, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. the step
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("name", ["default", "tight"])
@pytest.mark.parametrize("camera", MOVING_CAMERAS)
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (17, 33), (48, 32)], ids=lambda s: "%dx%d" % s)
def test_step_with_motion_matches_the_reference(capi, dn, O, cornell, size, camera, name, strict):
    """The moving stage through trg_temporal_denoise_motion_host (the third call plain), every call against reference_temporal(motion=...) evaluated
    from the device's own previous history.  On the images of at least 255 pixels the populations of the host test show on the DEVICE's N, on the
    pixels that are not `near`: history found with the motion planes and not by the plain step (a second context) on at least half of the moved
    plane, none where M0 lands on the floor alone, none in the block whose M0.w is cleared."""
    w, h = size
    params = dict({} if name == "default" else TIGHT, iterations=0)
    (c, mats), (plain, _) = (_ctx(O, cornell, w, h, capi, strict) for _ in range(2))
    try:
        frames = moving_frames(w, h, camera)
        prev = None
        for call, (colour, g, X, vp, m) in enumerate(frames):
            frame = (colour, g, X, vp, camera)
            p = params if m is None else dict(params, motion=m)
            out, iv, planes = _step(dn, c, mats, frame, p)
            R = _ref(dn, ("moving", size, camera, name), call, frame, prev, mats, p)
            _compare("temporal motion %s %dx%d camera %s strict %d" % (name, w, h, camera, strict), call, R, planes, iv)
            _finish(dn, frame, out, iv, mats, 1)
            if call < 2:
                dn.temporal_denoise(plain, colour, g, X, vp, **params)
            if call == 1 and w * h >= 255:
                cen = {k: v & ~R["near"] for k, v in motion_census(dn, frames, mats).items()}
                share = check_populations(cen, planes[0, ..., 3], dn.temporal_history(plain)[0, ..., 3], None)
                print("temporal motion %s %dx%d camera %s strict %d: history found with motion only on %.3f of the moved plane" % (name, w, h, camera, strict, share))
            prev = planes
    finally:
        _close(c, dn)
        _close(plain, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("strict", [1, 0])
def test_sliding_box_keeps_its_history_end_to_end(capi, dn, O, cornell, strict):
    """Cornell box 64 x 48, 2 spp, 4 calls, camera at rest, max_history = 3; before call k the short box has moved by 0.02 k:
    trg_load_scene + trg_temporal_set_previous_scene (no normals: a pure translation) + trg_render_temporal_read.
    After call k, against reference_temporal(motion=...) from the device's own previous history and this call's guides: N within the bar on every
    pixel that is not `near`; on the pixels that show the same non-emissive primitive as in the call before, N == min(k + 1, 3) (to 1e-3) exactly
    where the reference says so, their share of the hits the reference's; on the short box some pixel has a history.
    The same schedule with trg_temporal_reset instead: N == 1 on every hit after every call.
    And a further call without a new previous scene is the plain step from the same history, bit for bit: the arming was consumed."""
    import torch
    w, h, spp, bounces, calls = 64, 48, 2, 3, 4
    kw = dict(max_history=3)
    b = cornell.buffers()
    mats = b["material_ids"]
    off = O.pixel_offsets(w, h)
    scenes = [moved_box(b, 0.02 * k) for k in range(calls)]
    a, reset, twin = (make_ctx(O, cornell, w, h, offsets=off) for _ in range(3))
    try:
        for c in (a, reset, twin):
            c.set_option(capi.OPT_STRICT, strict)
        vp = dn.temporal_view_proj(O.make_uniforms(w, h))
        prev_planes = prev_prim = None
        for k in range(calls):
            for c in (a, reset, twin):
                if k:
                    _load(c, scenes[k])
            if k:
                for c in (a, twin):
                    dn.temporal_set_previous_scene(c, scenes[k - 1]["positions"], None, b["indices"])
                dn.temporal_reset(reset)
            for c in (a, reset, twin):
                dn.render_temporal(c, k * spp, spp, bounces, **kw)
            hist, Nr = dn.temporal_history(a), dn.temporal_history(reset)[0, ..., 3]
            N = hist[0, ..., 3]
            if k:
                g, X, m = dn.guides_motion(a, k * spp)                     # (the previous scene stays stored; the arming plays no part here)
            else:
                (g, X), m = dn.guides_pos(a, 0), None
            F = _filter_g0(dn, g, mats)
            hit = F[..., 3] >= 0
            assert (Nr[hit] == 1).all() and (Nr[~hit] == 0).all()
            prim = np.ascontiguousarray(g[1, ..., 3]).view(np.int32)
            if k:
                new, _, (near, near_n) = dn.reference_temporal(np.zeros((h, w, 4), f32), g[0], g[1], X, prev_planes, vp, motion=m, material_ids=mats, near_parts=True, **kw)
                Nref = new[0, ..., 3]
                assert near.mean() <= 0.01
                ok = hit & ~near
                assert (np.abs(N - Nref)[ok] <= 1e-4 * np.maximum(1.0, Nref[ok])).all(), float(np.abs(N - Nref)[ok].max())
                full = min(k + 1, kw["max_history"])
                same = ok & (prim == prev_prim)
                ref_full, dev_full = np.abs(Nref - full) <= 1e-3, np.abs(N - full) <= 1e-3
                clear = same & (np.abs(np.abs(Nref - full) - 1e-3) > 5e-4)                # (the reference itself is not at the edge of that band)
                assert np.array_equal(dev_full[clear], ref_full[clear])
                share_ref, share_dev = ref_full[same].sum() / hit.sum(), dev_full[same].sum() / hit.sum()
                box = same & (prim < SHORT_BOX)
                print("sliding box strict %d call %d: same primitive on %.3f of the hits; N == %d on %.3f of the hits (reference %.3f); short box: %d pixels, %.3f with a history" % (
                    strict, k, same.sum() / hit.sum(), full, share_dev, share_ref, box.sum(), float((N[box] > 1).mean()) if box.any() else 0.0))
                assert abs(share_dev - share_ref) <= (same & ~clear).sum() / hit.sum()
                assert box.any() and (N[box] > 1).any() and np.array_equal((N > 1)[box & clear], (Nref > 1)[box & clear])
            else:
                assert (N[hit] == 1).all()
            prev_planes, prev_prim = np.stack([hist[0], hist[1], F, X]), prim
        # one more call, nothing said about the geometry: the plain step
        first = calls * spp
        whole = dn.render_temporal(a, first, spp, bounces, **kw)
        img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        twin.bind_accum(img.data_ptr())
        try:
            twin.render(first, spp, bounces)
            twin.sync()
        finally:
            twin.bind_accum(None)
        mean = img.cpu().numpy()
        mean[..., :3] = mean[..., :3] * f32(np.float64(first + spp) / np.float64(spp))
        g, X = dn.guides_pos(twin, first)
        steps = dn.temporal_denoise(twin, mean, g, X, vp, **kw)
        assert np.array_equal(_bits(whole), _bits(steps)), int((_bits(whole) != _bits(steps)).sum())
        assert np.array_equal(_bits(dn.temporal_history(a)), _bits(dn.temporal_history(twin)))
    finally:
        for c in (a, reset, twin):
            _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 5. refusals
def test_motion_entry_points_refuse_bad_arguments(capi, dn, O, cornell):
    import torch
    w, h = 37, 29
    b = cornell.buffers()
    c = make_ctx(O, cornell, w, h, offsets=O.pixel_offsets(w, h))
    L = dn.load()
    refused = lambda fn: _refused(capi, fn)
    try:
        refused(lambda: dn.guides_motion(c, 0))                                                         # no previous scene yet
        pos, idx = b["positions"], b["indices"]
        refused(lambda: dn.temporal_set_previous_scene(c, pos, None, idx[:-3]))                         # another triangle count
        bad = idx.copy()
        bad[5] = pos.shape[0]
        refused(lambda: dn.temporal_set_previous_scene(c, pos, None, bad))                              # an index outside the vertices
        nt = idx.shape[0] // 3
        for args in ((None, None, idx.ctypes.data), (pos.ctypes.data, None, None)):
            refused(lambda: dn._chk(c, L.trg_temporal_set_previous_scene(c.h_ctx, *args, pos.shape[0], nt)))
        refused(lambda: dn.guides_motion(c, 0))                                                         # (a refused call stored nothing)
        dn.render_temporal(c, 0, 1, 3)
        before = dn.temporal_history(c)
        dn.temporal_set_previous_scene(c, pos, b["normals"], idx)                                       # armed
        g, X, m = dn.guides_motion(c, 0)
        other = O.OracleScene.cornell_box()
        mtx = np.diag([0.1, 0.1, 0.1, 1.0]).astype(f32)
        mtx[3, :3] = (0.0, 1.0, 0.5)
        other.add("cube", (0.5, 0.5, 0.5), mtx)
        _load(c, other.buffers())                                                                       # 12 triangles more
        refused(lambda: dn.render_temporal(c, 1, 1, 3))                                                 # armed for another triangle count
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(before))                             # ... and the history is untouched
        refused(lambda: dn.guides_motion(c, 0))
        dn.temporal_reset(c)                                                                            # disarms
        dn.render_temporal(c, 1, 1, 3)
        N = dn.temporal_history(c)[0, ..., 3]
        assert set(np.unique(N)) <= {0.0, 1.0}
        _load(c, b)
        dn.temporal_set_previous_scene(c, pos, None, idx)
        dn.temporal_set_previous_scene(c, None, None, None)                                             # forgotten: disarmed, and no planes
        refused(lambda: dn.guides_motion(c, 0))
        dn.render_temporal(c, 2, 1, 3)
        dn.temporal_set_previous_scene(c, pos, None, idx)
        colour = np.ones((h, w, 4), f32)
        vp = dn.temporal_view_proj(O.make_uniforms(w, h))
        ct, gt, xt, mt = (torch.from_numpy(x).cuda() for x in (colour, g, X, m))
        o = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        two = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
        before = dn.temporal_history(c)
        refused(lambda: dn.temporal_denoise(c, ct, gt, xt, vp, out=o, motion=gt))                       # motion overlaps the guides
        refused(lambda: dn.temporal_denoise(c, mt[0], gt, xt, vp, out=o, motion=mt))                    # ... the colour
        refused(lambda: dn.temporal_denoise(c, ct, gt, mt[1], vp, out=o, motion=mt))                    # ... the positions
        refused(lambda: dn.temporal_denoise(c, ct, gt, xt, vp, out=mt[1], motion=mt))                   # ... out
        refused(lambda: dn.guides_motion(c, 0, out=gt, pos=xt, motion=gt))
        refused(lambda: dn.guides_motion(c, 0, out=gt, pos=two[1], motion=two))
        ptr = lambda t: C.c_void_p(t.data_ptr())
        p = dn.make_temporal_params()
        vpp = vp.ctypes.data_as(C.POINTER(C.c_float))
        refused(lambda: dn._chk(c, L.trg_temporal_denoise_motion(c.h_ctx, ptr(ct), ptr(gt), ptr(xt), None, vpp, ptr(o), C.byref(p))))
        refused(lambda: dn._chk(c, L.trg_guides_render_motion(c.h_ctx, 0, ptr(gt), ptr(xt), None)))
        refused(lambda: dn.temporal_denoise(c, ct, gt, xt, vp, out=o, motion=mt, plane_tol=0.0))
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(before))
        dn.temporal_denoise(c, ct, gt, xt, vp, out=o, motion=mt)                                        # and a good call still works
        c.sync()
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 6. plugin
def _slid_cornell(host, dx):
    """include/cornellBox.h's placements through the host library's Scene, the short box moved by dx along x (toyraygun_cornell slide=D)."""
    white = (0.725, 0.71, 0.68)
    pi = float(f32(np.pi))
    table = [("cube", white, (0.6, 0.6, 0.6), (0.0, 0.3, 0.0), (float(f32(0.3275) + f32(dx)), 0.3, 0.3725)),
             ("cube", white, (0.6, 1.2, 0.6), (0.0, -0.3, 0.0), (-0.335, 0.6, -0.29)),
             ("plane", white, (2.0, 2.0, 2.0), (0.0, 0.0, pi), (0.0, 1.0, 0.0)),
             ("plane", white, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
             ("plane", (0.63, 0.065, 0.05), (2.0, 2.0, 2.0), (0.0, 0.0, float(f32(pi) / f32(2.0))), (0.0, 1.0, 0.0)),
             ("plane", (0.14, 0.491, 0.05), (2.0, 2.0, 2.0), (0.0, 0.0, float(-f32(pi) / f32(2.0))), (0.0, 1.0, 0.0)),
             ("plane", white, (2.0, 2.0, 2.0), (float(-f32(pi) / f32(2.0)), 0.0, 0.0), (0.0, 1.0, 0.0)),
             ("light", (1.0, 1.0, 1.0), (0.5, 1.98, 0.5), (0.0, 0.0, pi), (0.0, 1.0, 0.0))]
    s = host.Scene()
    for kind, color, scale, rot, pos in table:
        s.add(kind, color, host.mtx_srt(scale, rot, pos))
    return s.buffers()


def test_plugin_update_scene_and_slide(capi, dn, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png denoise=5,temporal slide=0.02: HipRenderer::updateScene before every call but the first; the picture
    differs from slide=0's and is trg_postprocess of what trg_load_scene + trg_temporal_set_previous_scene + trg_render_temporal give for the
    same calls.  Without a denoise mode updateScene is loadScene: the picture of the same calls with trg_load_scene + trg_render."""
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces, slide = 64, 48, 4, 3, 0.02

    def run(name, *extra):
        path = str(tmp_path / name)
        subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba()
    still, slid, plain = run("still.png", "denoise=5,temporal", "slide=0"), run("slid.png", "denoise=5,temporal", "slide=0.02"), run("plain.png", "slide=0.02")
    assert not np.array_equal(still, slid)
    assert np.array_equal(still, run("none.png", "denoise=5,temporal"))
    assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "denoise=5,temporal", "slide=x"], capture_output=True, timeout=120).returncode != 0
    assert np.array_equal(_slid_cornell(host, 0.0)["positions"], host.Scene.cornell_box().buffers()["positions"])
    scenes = [_slid_cornell(host, float(f32(k * slide))) for k in range(frames)]
    for temporal in (True, False):
        c = capi.Context(w, h)
        try:
            _load(c, scenes[0])
            c.set_uniforms(host.uniforms(w, h)[0])
            c.set_pixel_offsets_seed()
            den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            for k in range(frames):
                if k:
                    _load(c, scenes[k])
                    if temporal:
                        dn.temporal_set_previous_scene(c, scenes[k - 1]["positions"], scenes[k - 1]["normals"], scenes[k - 1]["indices"])
                if temporal:
                    dn.render_temporal(c, k, 1, bounces, out=den, iterations=5)
                else:
                    c.render(k, 1, bounces)
            c.sync()
            if temporal:
                c.bind_accum(den.data_ptr())
            try:
                assert np.array_equal(c.postprocess(flip_y=True), slid if temporal else plain), temporal
            finally:
                c.bind_accum(None)
        finally:
            _close(c, dn)
