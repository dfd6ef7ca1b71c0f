"""A ROOM under moving geometry (tests/test_room_motion_host.py, tests/test_gpu_room_motion.py): the steps a loaded room scene is taken through
by trg_refit_scene, and the drivers that reach them through the pose, skin, morph and rig units.  Built on tests/room_scenes.py (frames, rays, the
float64 model) and on tests/refit_scenes.py cornell_moved's way of moving corners: a float64 map of the float32 corner, rounded ONCE per corner, so
that the copies of a corner stay the copies they were.

The Cornell box's buffers: triangles 0 .. 11 the short box, 12 .. 23 the tall box, 24 .. 33 the room's five walls, 34 and 35 the light's quad.
A step is a Step(name, buffers, room, wall_map): room = (C, H, faces) of the room the builder must find, or None where it must find none;
wall_map = (A, t), the affine map the walls went through -- the map that CARRIES the light block with them (uniforms(..., carried=True)).

  rest              nothing moves: 5 faces, the aligned frame
  rigid             every vertex and normal through one rotation (0.15 about x, then 0.4 about y) plus a translation; the default light
                    is then not inside the room, the light carried by the same map is
  sheared           walls and light quad through a shear plus a non-uniform scale about the floor's centre; the boxes stay, inside
  low_ceiling_in    the room scaled in y about the floor: the ceiling 3e-3 above the default light rectangle, which STANDS -- accepted by the rule
  low_ceiling_out   ... 1e-3 above it: inside the room, and refused
  broken            all copies, within ONE wall, of one of its corners moved by 1e-3: no room (tests/test_room_host.py test_no_room)
  mended            the bits of rest
  box_through_wall  the short box slid along -x until it straddles the left wall
and for room_scenes.gpu_scenes' "tube" (4 faces, a rotated frame, the room's triangles first): rest, rigid, broken, mended."""
import collections

import numpy as np

from tests import room_scenes as R
from tests.util import LIGHT_FIELDS, uniforms_case

Step = collections.namedtuple("Step", "name buffers room wall_map")
IDENTITY = (np.eye(3), np.zeros(3))
ROOM_FIRST_TRI, ROOM_TRIS = 24, 10                       # tests/test_room_host.py test_cornell_box_room
SHORT, TALL, WALLS = slice(0, 36), slice(36, 72), slice(72, 108)      # vertex rows; WALLS holds the light's quad too
OBJECT_FIRST = np.array([0, 12, 24, 36], np.uint32)     # the pose driver's objects: short box, tall box, walls plus light
BROKEN_WALL_TRI = 28                                     # the left wall's pair of triangles, 28 and 29
NUDGE = np.array([1e-3, 0.0, 0.0])                       # out of that wall's plane: not even a quad any more
LIGHT_Y = float(np.float32(1.98))                        # the default block's light_pos.y
CORNELL_STEPS = ("rest", "rigid", "sheared", "low_ceiling_in", "low_ceiling_out", "broken", "mended", "box_through_wall")
TUBE_STEPS = ("rest", "rigid", "broken", "mended")
TUBE_BROKEN_WALL_TRI = 2

# 0.15 about x, then 0.4 about y, then the shift: the default light rectangle, which stands, then STRADDLES the tilted ceiling -- not inside the room
RIGID = (R.rot(1, 0.4) @ R.rot(0, 0.15), np.array([0.2, 0.0, -0.3]))
_SH = np.eye(3)
_SH[0, 1], _SH[2, 0] = 0.15, -0.1
SHEAR = (_SH @ np.diag([1.15, 1.05, 1.1]), np.zeros(3))   # about the floor's centre, the origin: the floor stays in its plane, the boxes on it
BOX_SLIDE = np.array([-1.3, 0.0, 0.15])                  # (the z part keeps the short box clear of the tall one)


def ceiling_map(gap):
    """The room scaled in y about the floor so that its ceiling lies `gap` above the default light rectangle."""
    return np.diag([1.0, (LIGHT_Y + gap) / 2.0, 1.0]), np.zeros(3)


def moved(b, rows, A, t):
    """`b` with the vertices `rows` through x -> A x + t (float64, rounded once per corner) and their normals through A^-T, normalised."""
    out = dict(b, positions=b["positions"].copy(), normals=b["normals"].copy())
    out["positions"][rows] = (b["positions"][rows].astype(np.float64) @ A.T + t).astype(np.float32)
    n = b["normals"][rows].astype(np.float64) @ np.linalg.inv(A)
    out["normals"][rows] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return out


def corner_copies(b, wall_tri):
    """The vertex rows, within the wall whose first triangle is wall_tri, that hold the wall's first corner (two copies in pattern 1)."""
    rows = np.arange(3 * wall_tri, 3 * wall_tri + 6)
    return rows[(b["positions"][rows] == b["positions"][3 * wall_tri]).all(1)]


def nudged(b, wall_tri, offset=NUDGE):
    out = dict(b, positions=b["positions"].copy())
    rows = corner_copies(b, wall_tri)
    out["positions"][rows] = (b["positions"][rows].astype(np.float64) + offset).astype(np.float32)
    return out


def through(frame, A, t):
    C, H, faces = frame
    return A @ C + t, A @ H, faces


def cornell_steps(O):
    """name -> Step, in CORNELL_STEPS' order."""
    rest = O.OracleScene.cornell_box().buffers()
    C, H = R.frame("aligned")
    room = (C, H, R.OPEN_FRONT)
    every = slice(0, 108)
    out = collections.OrderedDict()
    out["rest"] = Step("rest", rest, room, IDENTITY)
    out["rigid"] = Step("rigid", moved(rest, every, *RIGID), through(room, *RIGID), RIGID)
    out["sheared"] = Step("sheared", moved(rest, WALLS, *SHEAR), through(room, *SHEAR), SHEAR)
    for name, gap in (("low_ceiling_in", 3e-3), ("low_ceiling_out", 1e-3)):
        m = ceiling_map(gap)
        out[name] = Step(name, moved(rest, WALLS, *m), through(room, *m), m)
    out["broken"] = Step("broken", nudged(rest, BROKEN_WALL_TRI), None, IDENTITY)
    out["mended"] = Step("mended", {k: v.copy() for k, v in rest.items()}, room, IDENTITY)
    out["box_through_wall"] = Step("box_through_wall", moved(rest, SHORT, np.eye(3), BOX_SLIDE), room, IDENTITY)
    assert tuple(out) == CORNELL_STEPS
    return out


def tube_steps(O):
    rest = R.gpu_scenes(O)["tube"][0].buffers()
    C, H = R.frame("rotated")
    room = (C, H, R.TUBE)
    out = collections.OrderedDict()
    out["rest"] = Step("rest", rest, room, IDENTITY)
    out["rigid"] = Step("rigid", moved(rest, slice(0, rest["positions"].shape[0]), *RIGID), through(room, *RIGID), RIGID)
    out["broken"] = Step("broken", nudged(rest, TUBE_BROKEN_WALL_TRI), None, IDENTITY)
    out["mended"] = Step("mended", {k: v.copy() for k, v in rest.items()}, room, IDENTITY)
    return out


SCENES = {"cornell": (cornell_steps, ROOM_FIRST_TRI, 5, BROKEN_WALL_TRI), "tube": (tube_steps, 0, 4, TUBE_BROKEN_WALL_TRI)}


def uniforms(O, w, h, step, cam="default", carried=False):
    """The oracle's block for tests/util.py CAMERAS[cam]; carried: the light block taken through the step's wall map -- position through the map,
    right and up through its matrix, forward through A^-T, normalised -- each component rounded to float32."""
    u = uniforms_case(O, w, h, cam, "default")
    if carried:
        A, t = step.wall_map
        f = np.array(u.light_forward[0:3], np.float64) @ np.linalg.inv(A)
        new = (A @ np.array(u.light_pos[0:3], np.float64) + t, f / np.linalg.norm(f), A @ np.array(u.light_right[0:3], np.float64),
               A @ np.array(u.light_up[0:3], np.float64))
        for name, v in zip(LIGHT_FIELDS, new):
            getattr(u, name)[0:3] = [float(np.float32(x)) for x in v]
    return u


def light_inside_f64(r, u):
    """include/trg.h trg_debug_room_light_inside, restated in float64 on the frame trg_debug_room reports (l = axis (P - center)): each of the four
    corners light_pos +- light_right +- light_up has |l_k| + 2.001e-3 |axis_k| <= 1 - 1e-4 on every axis k.  No room: no."""
    if r["n_faces"] == 0:
        return False
    pos, right, up = (np.array(getattr(u, k)[0:3], np.float64) for k in ("light_pos", "light_right", "light_up"))
    A, cen = r["axis"].astype(np.float64), r["center"].astype(np.float64)
    for sr in (-1.0, 1.0):
        for su in (-1.0, 1.0):
            l = A @ (pos + sr * right + su * up - cen)
            if not (np.abs(l) + 2.001e-3 * np.linalg.norm(A, axis=1) <= 1.0 - 1e-4).all():
                return False
    return True


# ------------------------------------------------------------------------------------------------------------------------------- the float64 model
def rays_of(O, step, rest, seed=300, n=20000):
    """About n room_rays in the step's frame (the rest frame where the step has no room) as trg_trace records, mask 3, and the SAME rays in
    float64 -- the float32 origin, the normalised float32 direction and maxDistance widened -- so that the model traces what the device traces.
    Returns (records, o, d, tmax, kind)."""
    C, H, faces = step.room if step.room is not None else rest.room
    o, d, tmax, kind = R.room_rays(C, H, faces, seed + len(step.name), n)
    rays = R.as_trace_rays(O, o, d, tmax, 3)
    return rays, rays["origin"].astype(np.float64), rays["direction"].astype(np.float64), rays["maxDistance"].astype(np.float64), kind


def tris_f64(T, o, d, tmax):
    """Two-sided float64 Moeller-Trumbore (the hit rule of room_scenes.coincident_f64) of the rays against the triangles T [n, 3, 3]: (index into T or
    -1, t) of the nearest hit in [0, tmax]."""
    best_k, best_t = np.full(len(o), -1), np.full(len(o), np.inf)
    for k in range(T.shape[0]):
        v0, e1, e2 = T[k, 0], T[k, 1] - T[k, 0], T[k, 2] - T[k, 0]
        p = np.cross(d, e2)
        det = p @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tv = o - v0
            u = (tv * p).sum(1) * inv
            q = np.cross(tv, e1)
            v = (d * q).sum(1) * inv
            t = (q @ e2) * inv
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= tmax) & (t < best_t)
        best_k[hit], best_t[hit] = k, t[hit]
    return best_k, best_t


def face_first_tri(b, frame, first_tri, n_faces):
    """face -> the first of the wall's two triangles in the buffers `b`: the pair whose centroid is the face's centre."""
    C, H, faces = frame
    P = b["positions"][b["indices"]].astype(np.float64).reshape(-1, 6, 3)[first_tri // 2:first_tri // 2 + n_faces]
    cen = np.stack([np.unique(q, axis=0).mean(0) for q in P])
    out = {}
    for f in faces:
        dist = np.linalg.norm(cen - R.face_quad(C, H, f).mean(0), axis=1)
        assert dist.min() < 1e-4 * np.linalg.norm(H, axis=0).max()
        out[f] = first_tri + 2 * int(dist.argmin())
    assert len(set(out.values())) == len(faces)
    return out


def scene_f64(step, rest, first_tri, n_faces, broken_tri, o, d, tmax, mask):
    """The step's scene in float64: the room by THE RULE (room_scenes.open_box_f64) in the step's frame -- for a step without a room its walls one
    by one (room_scenes.quads_f64 in the frame of the step `rest`), the nudged wall as the two triangles it now is -- and every other triangle by tris_f64;
    triangles whose material id has no bit in common with `mask` are not there (the walls' is 1).  Returns (quad = primitive // 2 of the
    nearest hit or -1, t, is it a wall, t of the nearest wall hit)."""
    b = step.buffers
    T = b["positions"][b["indices"]].astype(np.float64).reshape(-1, 3, 3)
    mats = b["material_ids"]
    n = len(o)
    wall_q, wall_t = np.full(n, -1), np.full(n, np.inf)
    if mask & int(mats[first_tri]):
        if step.room is not None:
            C, H, faces = step.room
            tri_of = face_first_tri(b, step.room, first_tri, n_faces)
            f, t = R.open_box_f64(C, H, faces, o, d, tmax)
        else:
            C, H, faces = rest.room
            tri_of = face_first_tri(rest.buffers, rest.room, first_tri, n_faces)
            whole = [x for x in faces if tri_of[x] != broken_tri]
            with np.errstate(invalid="ignore"):
                f, t = R.quads_f64(C, H, whole, o, d, tmax)
            k, tk = tris_f64(T[broken_tri:broken_tri + 2], o, d, tmax)
            nearer = (k >= 0) & (tk < t)
            (bf,) = [x for x in faces if tri_of[x] == broken_tri]
            f, t = np.where(nearer, bf, f), np.where(nearer, tk, t)
        lut = np.full(7, -1)
        for x, tri in tri_of.items():
            lut[x] = tri // 2
        wall_q, wall_t = lut[f], np.where(f >= 0, t, np.inf)
    others = np.array([k for k in range(T.shape[0]) if not first_tri <= k < first_tri + 2 * n_faces and (mask & int(mats[k]))], np.int64)
    k, tk = tris_f64(T[others], o, d, tmax) if len(others) else (np.full(n, -1), np.full(n, np.inf))
    other_q = np.where(k >= 0, others[np.maximum(k, 0)] // 2, -1) if len(others) else k
    wall = wall_t <= tk
    return np.where(wall, wall_q, other_q), np.where(wall, wall_t, tk), wall & (wall_q >= 0), wall_t


def excluded(step, rest, first_tri, n_faces, o, d, tmax):
    """The two classes of rays a float32 trace is not held to (tests/test_gpu_room.py): `edge`, the float64 wall hit within 1e-5 of the room's size
    of an edge of the room, and `tied`, something else IN a wall's plane at the hit (the boxes stand on the floor).  Each must stay under 1 %."""
    C, H, faces = step.room if step.room is not None else rest.room
    with np.errstate(invalid="ignore"):
        fm, tm = R.open_box_f64(C, H, faces, o, d, tmax) if step.room is not None else R.quads_f64(C, H, faces, o, d, tmax)
    size = float(np.linalg.norm(H, axis=0).max())
    edge = (fm >= 0) & (R.edge_distance(C, H, o, d, tm) * float(np.linalg.norm(H, axis=0).min()) < 1e-5 * size)
    b = step.buffers
    tied = R.coincident_f64(b["positions"][b["indices"]], np.arange(b["indices"].shape[0]), o, d, tmax, first_tri, 2 * n_faces, 1e-5 * size)
    return edge, tied


# ----------------------------------------------------------------------------------------------------------------------------------- the drivers
def xform(A, t):
    return np.concatenate([A, np.asarray(t, np.float64)[:, None]], axis=1).reshape(12).astype(np.float32)


EYE12 = xform(*IDENTITY)
POSES = {   # the pose driver: step -> [3, 12], one row per object of OBJECT_FIRST
    "rest": np.stack([EYE12, EYE12, EYE12]),
    "rigid": np.stack([xform(*RIGID)] * 3),
    "sheared": np.stack([EYE12, EYE12, xform(*SHEAR)]),
    "box_through_wall": np.stack([xform(np.eye(3), BOX_SLIDE), EYE12, EYE12]),
}


def skin_binding(b, blended=False):
    """(ids, weights, n_bones = 2): the boxes on bone 0, walls and light on bone 1; blended: the copies, within the left wall, of its first corner
    lean 0.5 / 0.5 on both bones -- under two equal bones the room it was, under bones that differ no wall of one."""
    nv = b["positions"].shape[0]
    ids = np.tile(np.array([0, 1, 0, 0], np.uint32), (nv, 1))
    w = np.zeros((nv, 4), np.float32)
    w[:72, 0] = 1.0
    w[72:, 1] = 1.0
    if blended:
        w[corner_copies(b, BROKEN_WALL_TRI)] = (0.5, 0.5, 0.0, 0.0)
    return ids, w, 2


BONES = {   # the skin driver: name -> [2, 12]
    "rest": np.stack([EYE12, EYE12]),
    "sheared": np.stack([EYE12, xform(*SHEAR)]),            # bones that differ
    "rigid": np.stack([xform(*RIGID)] * 2),                 # equal bones
}


def morph_target(b):
    """(target_first, entry_vertex, dpos): one target, the NUDGE on the copies, within the left wall, of its first corner."""
    rows = corner_copies(b, BROKEN_WALL_TRI)
    return np.array([0, rows.shape[0]], np.uint32), rows.astype(np.uint32), np.tile(NUDGE.astype(np.float32), (rows.shape[0], 1))


NO_PARENT = 0xFFFFFFFF


def _quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions: the rotation b, then a."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def wall_rig():
    """The rig driver over skin_binding's two bones: joint 0 (the boxes) rests; joint 1 (walls and light) has two keys, the rest pose at time 0 and
    RIGID at time 1.  No inverse bind: the joints sit at the origin."""
    half = lambda ax, ang: np.concatenate([np.eye(3)[ax] * np.sin(ang / 2), [np.cos(ang / 2)]])
    q = _quat_mul(half(1, 0.4), half(0, 0.15))
    still = [0.0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0]
    keys = np.array([still, still, np.concatenate([[1.0], RIGID[1], q, [1, 1, 1, 0]])], np.float64)
    return dict(parent=np.array([NO_PARENT, NO_PARENT], np.uint32), key_first=np.array([0, 1, 3], np.uint32),
                keys=np.ascontiguousarray(keys.astype(np.float32)), clock_of=np.zeros(2, np.uint32), n_clocks=1, inv_bind=None)


RIG_CLOCKS = {"on the first key": 0.0, "between": 0.5, "on the last key": 1.0}
