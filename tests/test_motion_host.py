"""Host-side checks of the temporal step for MOVING GEOMETRY (include/trg_denoise.h, "MOVING GEOMETRY"; toyraygun_amd/denoise.py): the exported
surface, the float64 reference with its `motion` argument, and a synthetic stage whose raised plane moves between two calls
(tests/test_gpu_motion.py imports the generators from here).  No GPU.

THE MOVING STAGE.  The two-plane stage of tests/test_temporal_synthetic_host.py (seed 1) is the CURRENT frame.  In the PREVIOUS frame its raised
plane stood elsewhere: a point P of it was at
    A(P) = R (P - PIVOT) + PIVOT + T,    R = a rotation by 30 degrees about the y axis (cos 30 = 0.866: under normal_tol = 0.9 and 0.97),
    PIVOT = (0, 0, -1.5) on the plane,   T = 0.4 along the rotated normal, away from the camera (the plane tolerance 0.02 z is 0.05 at most)
                                             + the part of (0.8, 0.45, 0) that lies in the rotated plane (a slide by a fraction of a block).
The previous frame shows the raised plane in that pose at the SAME pixels (depth, normal and X replaced; the pushes off the plane, the zero
normals, the misses and the emitters stay), the floor unchanged.  M0 = (A(X(p)), 1) and M1 = (R G0(p).xyz, 0) on the raised plane, (X(p), 1) and
(G0(p).xyz, 0) on the floor, zero on the misses; a block of pixels (BLOCK) has M0.w = 0.
Three calls: the previous frame without history; the current frame with the motion planes, the previous camera at rest or on the `sub` shift;
the current frame again at rest, plain (no motion argument)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_temporal_host import NEAR_CAP, seeded_colour
from tests.test_temporal_synthetic_host import PARAM_SETS, PLANES, SCHEDULE, SHAPES_PARAMS, near_caps, previous_camera, schedule_frames, stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_denoise.h")
f32 = np.float32

MOTION_SYMBOLS = {"trg_temporal_set_previous_scene", "trg_guides_render_motion", "trg_temporal_denoise_motion", "trg_guides_motion_read",
                  "trg_temporal_denoise_motion_host"}
MOVING_SHAPES = [(48, 32), (17, 33)]
MOVING_CAMERAS = ["rest", "sub"]
THETA = np.deg2rad(30.0)
PIVOT = np.array([0.0, 0.0, -PLANES["raised"][0]])
LIFT, SLIDE = 0.4, np.array([0.8, 0.45, 0.0])
TIGHT = PARAM_SETS["tight"]                      # plane_tol 0.01, normal_tol 0.97, every other field off its default too


def block(w, h):
    """The pixels whose M0.w is cleared: (rows, columns)."""
    return slice(h // 4, h // 4 + 5), slice(w // 4, w // 4 + 4)


def rigid():
    """(R, T, the unit normal of the raised plane in its previous pose)."""
    c, s = np.cos(THETA), np.sin(THETA)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    n = np.array([PLANES["raised"][1], PLANES["raised"][2], 1.0])
    n_prev = R @ (n / np.sqrt((n * n).sum()))
    T = -LIFT * n_prev + (SLIDE - (SLIDE @ n_prev) * n_prev)
    return R, T, n_prev


def was_at(P):
    """A(P) of the docstring for points [..., 3], float64."""
    R, T, _ = rigid()
    return (np.asarray(P, np.float64) - PIVOT) @ R.T + PIVOT + T


def raised_mask(g):
    return (g[0, ..., 3] >= 0) & (g[0, ..., 3] < 2.7)


def moving_stage(w, h):
    """(previous guides, previous X, current guides, current X, motion [2, h, w, 4]) float32."""
    g, X = stage(w, h, 1)
    R, T, n_prev = rigid()
    raised = raised_mask(g)
    yy, xx = np.mgrid[0:h, 0:w]
    Xc, Yc = xx + 0.5, yy + 0.5
    P0 = PIVOT + T                                                    # a point of the plane in its previous pose
    Zp = P0[2] - (n_prev[0] * (Xc - P0[0]) + n_prev[1] * (Yc - P0[1])) / n_prev[2]
    push = -(X[..., 2].astype(np.float64) + g[0, ..., 3])            # what the stage pushed the pixel off its plane by
    gp, Xp = g.copy(), X.copy()
    has_normal = (np.abs(g[0, ..., :3]).max(-1) > 0)
    gp[0, ..., 3] = np.where(raised, -Zp, g[0, ..., 3]).astype(f32)
    gp[0, ..., :3] = np.where((raised & has_normal)[..., None], 0.9 * n_prev, g[0, ..., :3]).astype(f32)
    Xp[..., 2] = np.where(raised, Zp - push, X[..., 2]).astype(f32)
    assert (gp[0, ..., 3][raised] > 0.5).all()
    m = np.zeros((2, h, w, 4), f32)
    hit = g[0, ..., 3] >= 0
    m[0, ..., :3] = np.where(raised[..., None], was_at(X[..., :3]), X[..., :3]).astype(f32)
    m[0, ..., 3] = 1.0
    m[1, ..., :3] = np.where(raised[..., None], g[0, ..., :3].astype(np.float64) @ R.T, g[0, ..., :3]).astype(f32)
    m[:, ~hit] = 0.0
    rows, cols = block(w, h)
    m[0, rows, cols, 3] = 0.0
    return gp, Xp, g, X, m


def moving_frames(w, h, camera, colour_seed=700):
    """[(colour, guides, X, prev_vp or None, motion or None)] of the three calls."""
    gp, Xp, g, X, m = moving_stage(w, h)
    return [(seeded_colour(gp, colour_seed), gp, Xp, None, None),
            (seeded_colour(g, colour_seed + 1), g, X, previous_camera(w, h, camera), m),
            (seeded_colour(g, colour_seed + 2), g, X, previous_camera(w, h, "rest"), None)]


def identity_motion(g, X):
    """M0 = (X.xyz, 1), M1 = (G0.xyz, 0): the planes with which the motion form is the plain step."""
    m = np.zeros((2,) + X.shape, f32)
    m[0, ..., :3], m[0, ..., 3] = X[..., :3], 1.0
    m[1, ..., :3] = g[0, ..., :3]
    return m


def motion_census(dn, frames, mats):
    """Per-pixel bool planes of the moving call, float64, from the frames alone: `moved` (hits of the raised plane with a normal, outside BLOCK),
    `inside` (of those: the previous position's sample lies inside the image), `other` (of those: in the window, and every tap inside the image
    shows the floor or nothing in the previous frame), `blocked` (hits with a normal inside BLOCK), `floor` (hits of the floor outside BLOCK)."""
    (_, gp, _, _, _), (_, g, X, vp, m) = frames[0], frames[1]
    F, _, miss = dn._filter_inputs(g[0], g[1], mats, np.float64)
    h, w = miss.shape
    hit = ~miss & (np.abs(F[..., :3]).max(-1) > 0)
    in_block = np.zeros((h, w), bool)
    in_block[block(w, h)] = True
    raised = raised_mask(g)
    P, v = m[0, ..., :3].astype(np.float64), np.asarray(vp, np.float64)
    cw = v[12] * P[..., 0] + v[13] * P[..., 1] + v[14] * P[..., 2] + v[15]
    fx = ((v[0] * P[..., 0] + v[1] * P[..., 1] + v[2] * P[..., 2] + v[3]) / cw * 0.5 + 0.5) * w - 0.5
    fy = ((v[4] * P[..., 0] + v[5] * P[..., 1] + v[6] * P[..., 2] + v[7]) / cw * 0.5 + 0.5) * h - 0.5
    window = (fx >= -1) & (fx < w) & (fy >= -1) & (fy < h)
    x0, y0 = np.floor(np.where(window, fx, 0.0)).astype(np.int64), np.floor(np.where(window, fy, 0.0)).astype(np.int64)
    prev_raised = raised & ~dn.emitter_mask(gp[1], mats)                            # (the previous frame shows the plane at the same pixels)
    any_raised = np.zeros((h, w), bool)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            ins = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            any_raised |= ins & prev_raised[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
    moved = hit & raised & ~in_block
    return dict(moved=moved, inside=moved & (fx + 0.5 >= 0) & (fx + 0.5 < w) & (fy + 0.5 >= 0) & (fy + 0.5 < h), other=moved & window & ~any_raised,
                blocked=hit & in_block, floor=hit & ~raised & ~in_block)


def check_populations(cen, N_motion, N_plain, N_unblocked):
    """(a) - (c) of the moving call on a plane of history lengths N with motion, one without it, and one with motion whose BLOCK was not cleared
    (None: (c) is checked on N_motion alone).  Returns the share of (a)."""
    a = (N_motion == 2) & (N_plain == 1)
    share = float(a[cen["inside"]].mean())
    assert cen["inside"].sum() >= 20 and share >= 0.5, (int(cen["inside"].sum()), share)
    assert (N_plain[cen["moved"]] == 1).all()                                        # without motion the moved plane finds nothing
    assert cen["other"].sum() > 0 and (N_motion[cen["other"]] == 1).all()            # (b)
    assert cen["blocked"].sum() > 0 and (N_motion[cen["blocked"]] == 1).all()        # (c)
    if N_unblocked is not None:
        assert (N_unblocked[cen["blocked"]] == 2).any()                              # ... and some of them would have found history
    return share


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------------
def test_header_exports_and_python_agree_on_the_motion_entry_points(built):
    from toyraygun_amd import capi, denoise
    declared = set(denoise.header_symbols(HEADER))
    assert MOTION_SYMBOLS <= declared
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in MOTION_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert MOTION_SYMBOLS <= set(denoise.SYMBOL_NAMES) and sorted(denoise.SYMBOL_NAMES) == sorted(declared)
    trg_h = open(os.path.join(ROOT, "include", "trg.h")).read()
    for name in MOTION_SYMBOLS:
        assert name not in trg_h
    L = denoise.load()
    for name in MOTION_SYMBOLS:
        assert getattr(L, name).argtypes is not None


def test_set_previous_scene_refuses_without_a_context(built):
    """What is decided before the context is touched: a NULL context, with good and with NULL arrays."""
    from toyraygun_amd import capi, denoise
    L = denoise.load()
    pos, idx = np.zeros((3, 3), f32), np.arange(3, dtype=np.uint32)
    for args in ((pos.ctypes.data, None, idx.ctypes.data, 3, 1), (None, None, idx.ctypes.data, 3, 1), (pos.ctypes.data, None, None, 3, 1), (None, None, None, 0, 0)):
        assert L.trg_temporal_set_previous_scene(None, *args) == capi.ERR_INVALID
    assert L.trg_guides_render_motion(None, 0, None, None, None) == capi.ERR_INVALID
    assert L.trg_temporal_denoise_motion(None, None, None, None, None, None, None, None) == capi.ERR_INVALID


# ---- the reference: default and identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(17, 33), (48, 32)], ids=lambda s: "%dx%d" % s)
def test_motion_none_is_the_plain_reference_and_identity_planes_change_nothing(cornell, size):
    """Over the nine calls of the synthetic SCHEDULE, in float64 and in the float32 mode: motion=None gives what the keyword's absence gives, and
    motion = (X | 1, G0.xyz | 0) gives the same again, exactly -- history, (I, V_0) and both near planes."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = size
    for dtype in (np.float64, np.float32):
        hist = None
        for colour, g, X, vp, cam in schedule_frames(w, h, SCHEDULE):
            kw = dict(material_ids=mats, near_parts=True, dtype=dtype, **SHAPES_PARAMS)
            plain = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, **kw)
            for motion in (None, identity_motion(g, X)):
                got = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, motion=motion, **kw)
                assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
                assert np.array_equal(got[2][0], plain[2][0]) and np.array_equal(got[2][1], plain[2][1])
                assert got[0].dtype == dtype
            hist = plain[0]


def test_reference_motion_is_fp32_barycentric_interpolation():
    """Three hits and a miss by hand: M0 = ((c0 P0 + c1 P1) + c2 P2, 1) in fp32, M1 likewise from the normals or G0.xyz without them, zero on a miss."""
    from toyraygun_amd import capi, denoise as dn
    pos = np.array([[0.1, 0.2, 0.3], [1.7, -0.4, 0.9], [0.33, 2.1, -1.3], [5.0, 5.0, 5.0]], f32)
    idx = np.array([0, 1, 2, 3, 2, 1], np.uint32)
    nrm = np.arange(18, dtype=f32).reshape(6, 3) / f32(7.0)
    isect = np.zeros(4, capi.ISECT_DTYPE)
    isect["distance"] = (1.0, 2.0, -1.0, 0.5)
    isect["primitiveIndex"] = (0, 1, -1, 1)
    isect["coordinates"] = ((0.3, 0.6), (0.25, 0.125), (0.0, 0.0), (1.0 / 3.0, 1.0 / 3.0))
    g0 = np.zeros((2, 2, 4), f32)
    g0[..., :3] = (0.1, 0.7, -0.2)
    m = dn.reference_motion(isect, pos, nrm, idx, g0).reshape(2, 4, 4)
    for k, tri in ((0, 0), (1, 1), (3, 1)):
        c0, c1 = isect["coordinates"][k]
        c2 = f32(f32(1.0) - c0) - c1
        P = pos[idx[3 * tri:3 * tri + 3]]
        want = f32(f32(c0 * P[0] + c1 * P[1]) + c2 * P[2])
        assert np.array_equal(m[0, k, :3], want) and m[0, k, 3] == 1 and m[1, k, 3] == 0
        Nn = nrm[3 * tri:3 * tri + 3]
        assert np.array_equal(m[1, k, :3], f32(f32(c0 * Nn[0] + c1 * Nn[1]) + c2 * Nn[2]))
    assert (m[:, 2] == 0).all() and m.dtype == f32
    m2 = dn.reference_motion(isect, pos, None, idx, g0).reshape(2, 4, 4)
    assert np.array_equal(m2[0], m[0]) and np.array_equal(m2[1, 0, :3], g0[0, 0, :3]) and (m2[1, 2] == 0).all()


# ---- the moving stage -----------------------------------------------------------------------------------------------------------------------------------
def test_the_rigid_motion_is_beyond_both_tolerances():
    R, T, n_prev = rigid()
    n = np.array([PLANES["raised"][1], PLANES["raised"][2], 1.0])
    n /= np.sqrt((n * n).sum())
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert n @ n_prev < min(0.9, TIGHT["normal_tol"]) and abs(T @ n_prev) > 0.02 * 2.6 and abs(T @ n_prev) > 5 * 0.02 * 2.6 - 1e-9
    for w, h in MOVING_SHAPES:
        gp, Xp, g, X, m = moving_stage(w, h)
        raised = raised_mask(g)
        assert raised.mean() > 0.3 and (g[0, ..., 3][raised] * 0.02 < abs(T @ n_prev)).all()
        on = raised & (np.abs(X[..., 2] + g[0, ..., 3]) < 1e-3)                     # not pushed off the plane
        # M0 lies on the previous frame's plane: its distance from a point of that plane along the plane's normal is a rounding
        d = (m[0, ..., :3].astype(np.float64) - (PIVOT + T)) @ n_prev
        assert np.abs(d[on]).max() < 1e-4 and np.abs(((Xp[..., :3].astype(np.float64) - (PIVOT + T)) @ n_prev)[on]).max() < 1e-4
        assert np.array_equal(m[0, ..., :3][~raised], X[..., :3][~raised]) and np.array_equal(m[1, ..., :3][~raised], g[0, ..., :3][~raised])
        rows, cols = block(w, h)
        assert (m[0, rows, cols, 3] == 0).all() and (m[0, ..., 3] == 1).sum() > 0.8 * w * h


@pytest.mark.parametrize("name", ["default", "tight"])
@pytest.mark.parametrize("camera", MOVING_CAMERAS)
@pytest.mark.parametrize("size", MOVING_SHAPES, ids=lambda s: "%dx%d" % s)
def test_moving_stage_reaches_its_populations(cornell, size, camera, name):
    """The reference alone over the three calls: (a) at least half of the moved plane's pixels whose previous position lies inside the image find
    history (N == 2) with the motion planes and none (N == 1) without; (b) pixels whose M0 lands on the floor alone are rejected; (c) BLOCK takes
    no history, though some of its pixels would find it; (d) the floor's history is identical with and without motion; (e) `near` under the cap
    in every call; and the plain third call goes on from the motion call's history (N == 3 somewhere on the moved plane)."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = size
    params = {} if name == "default" else TIGHT
    frames = moving_frames(w, h, camera)
    kw = dict(material_ids=mats, near_parts=True, **params)
    colour, g, X, vp, _ = frames[0]
    h0, _, (near, near_n) = dn.reference_temporal(colour, g[0], g[1], X, None, None, **kw)
    near_caps(near, near_n, 0)
    colour, g, X, vp, m = frames[1]
    with_m, _, (near, near_n) = dn.reference_temporal(colour, g[0], g[1], X, h0, vp, motion=m, **kw)
    near_caps(near, near_n, 1)
    assert NEAR_CAP == 0.01
    # (the plain step is no call of the schedule: at rest its samples sit on pixel centres with every tap rejected, which `near` marks wholesale)
    plain, _, _ = dn.reference_temporal(colour, g[0], g[1], X, h0, vp, **kw)
    unblocked = m.copy()
    unblocked[0, ..., 3] = np.where(g[0, ..., 3] >= 0, 1.0, 0.0)
    free, _, _ = dn.reference_temporal(colour, g[0], g[1], X, h0, vp, motion=unblocked, **kw)
    cen = motion_census(dn, frames, mats)
    share = check_populations(cen, with_m[0, ..., 3], plain[0, ..., 3], free[0, ..., 3])
    fl = cen["floor"]
    assert fl.sum() > 0.2 * w * h and np.array_equal(with_m[0][fl], plain[0][fl]) and np.array_equal(with_m[1][fl], plain[1][fl])      # (d)
    assert (with_m[0, ..., 3][fl] == 2).mean() > 0.5 or camera != "rest"
    colour, g, X, vp, _ = frames[2]
    third, _, (near, near_n) = dn.reference_temporal(colour, g[0], g[1], X, with_m, vp, **kw)
    near_caps(near, near_n, 2)
    assert (np.abs(third[0, ..., 3][cen["moved"]] - 3) < 1e-6).sum() > 0.3 * cen["inside"].sum()
    print("moving stage %s %dx%d camera %s: moved %d, previous position inside %d, history found with motion only on %.3f of them; on the floor alone %d, blocked %d" % (
        name, w, h, camera, cen["moved"].sum(), cen["inside"].sum(), share, cen["other"].sum(), cen["blocked"].sum()))
