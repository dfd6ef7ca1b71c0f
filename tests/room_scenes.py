"""Scenes, rays and the float64 model for the ROOM (bvh_build.h RoomLeaf): 3 to 5 wall quads that are faces of one parallelepiped, which the shipped
build tests once per traversal call ahead of the tree (tests/test_room_host.py, tests/test_gpu_room.py).

A room is given by its frame -- centre C and the matrix H whose columns are the three half axes: the room is C + H l, |l_k| <= 1 -- and the list
of the faces that are there, f = 2 k + (1 if the face lies at l_k = +1 else 0).  The builder numbers and signs its own axes (by the world axis each
follows most), so a test that compares faces maps them through `match_frame`.
"""
import numpy as np

EYE4 = np.eye(4, dtype=np.float32)
ALL_FACES = (0, 1, 2, 3, 4, 5)
TUBE = (0, 1, 2, 3)            # both z faces absent
CORNER = (0, 2, 4)             # three faces that share the vertex (-1, -1, -1)
U_SHAPE = (0, 1, 2)            # an opposite pair and the floor
OPEN_FRONT = (0, 1, 2, 3, 4)   # the Cornell box's: the face at +z absent
FOUR = (0, 1, 2, 4)            # floor, two side walls... and the back: ceiling and front absent (two ADJACENT faces absent)


def rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    m = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def frame(kind):
    """(C, H) in float64.  aligned = the Cornell box's own room; rotated, sheared, mirrored as the box leaves' tests have them (mirrored: det H < 0,
    the vertex order of every quad flips)."""
    C = np.array([0.0, 1.0, 0.0])
    if kind == "aligned":
        return C, np.eye(3)
    if kind == "rotated":
        return C + [0.05, 0.1, -0.02], rot(1, 0.5) @ rot(0, 0.3) @ np.diag([1.2, 1.0, 1.3])
    if kind == "sheared":
        sh = np.eye(3); sh[0, 1] = 0.35; sh[2, 0] = -0.2
        return C + [-0.1, 0.0, 0.1], rot(1, -0.25) @ sh @ np.diag([1.3, 1.1, 1.2])
    if kind == "mirrored":
        return C, rot(2, 0.15) @ rot(1, 0.9) @ np.diag([-1.1, 1.2, 1.0])
    raise KeyError(kind)


def face_quad(C, H, f):
    """The four corners (a, a + e1, a + e1 + e2, a + e2) of face f, float64."""
    k, s = f // 2, 1.0 if f & 1 else -1.0
    i, j = [a for a in range(3) if a != k]
    a = C + s * H[:, k] - H[:, i] - H[:, j]
    e1, e2 = 2.0 * H[:, i], 2.0 * H[:, j]
    return np.stack([a, a + e1, a + e1 + e2, a + e2])


def add_room(scene, C, H, faces, color=(0.7, 0.7, 0.7), mat=1, pattern=1, mats=None, nudge=None):
    """The quads of `faces`, two consecutive triangles each, in the order given.  pattern 1 = (a b c)(a c d) as Scene::addCube's faces, 2 = (a c d)
    (a b c)... as addPlane's.  mats: one material id per face instead of `mat`; nudge = (face position in the list, corner, offset[3])."""
    for n, f in enumerate(faces):
        p4 = face_quad(C, H, f)
        if nudge is not None and nudge[0] == n:
            p4[nudge[1]] += np.asarray(nudge[2], np.float64)
        scene.add_geometry(p4.astype(np.float32), [0, 1, 2, 0, 2, 3] if pattern == 1 else [0, 2, 3, 0, 1, 2], EYE4, color, mat if mats is None else mats[n])


def unit_cube(O):
    s = O.OracleScene()
    s.add("cube", (1.0, 1.0, 1.0), EYE4)
    return s.buffers()["positions"].reshape(-1, 3).copy(), np.arange(36, dtype=np.uint32)


def cube_mtx(scale, rot_y, pos, shear=0.0):
    r = rot(1, rot_y)
    sh = np.eye(3); sh[0, 1] = shear
    m = np.eye(4)
    m[:3, :3] = r @ sh @ np.diag(scale)
    m[:3, 3] = pos
    return m.T.astype(np.float32)


def add_zoo_cubes(O, s):
    """tests/util.py box_zoo's parallelepipeds (rotated, sheared, mirrored, nested, emissive, material 3), clear of every wall."""
    verts, idx = unit_cube(O)
    s.add_geometry(verts, idx, cube_mtx((0.12, 0.12, 0.12), 0.7, (-0.5, 1.4, 0.4)), (0.3, 0.8, 0.4), 1)
    s.add_geometry(verts, idx, cube_mtx((0.15, 0.1, 0.08), -0.3, (0.45, 1.2, -0.3), shear=0.6), (0.8, 0.5, 0.2), 1)
    s.add_geometry(verts, idx, cube_mtx((-0.1, 0.14, 0.1), 1.1, (0.1, 1.5, 0.5)), (0.2, 0.4, 0.9), 1)
    s.add_geometry(verts, idx, cube_mtx((0.05, 0.05, 0.05), 0.2, (-0.5, 1.4, 0.4)), (0.9, 0.9, 0.1), 1)
    s.add_geometry(verts, idx, cube_mtx((0.08, 0.04, 0.08), 0.0, (-0.2, 1.6, 0.2)), (1.0, 1.0, 1.0), 2)
    s.add_geometry(verts, idx, cube_mtx((0.1, 0.1, 0.1), 0.5, (0.4, 0.5, 0.6)), (0.6, 0.6, 0.6), 3)
    return 6


def gpu_scenes(O):
    """name -> (scene, (C, H, faces) of its room, faces the builder must report, boxes).  All fit in LDS."""
    out = {}
    C, H = frame("aligned")
    out["cornell"] = (O.OracleScene.cornell_box(), (C, H, OPEN_FRONT), 5, 2)
    s = O.OracleScene()
    C, H = frame("sheared")
    n = add_zoo_cubes(O, s)                               # (the cubes first: the room's records are not the first)
    add_room(s, C, H, FOUR, (0.6, 0.7, 0.8), 1, pattern=2)
    out["zoo4"] = (s, (C, H, FOUR), 4, n)
    s = O.OracleScene()
    C, H = frame("rotated")
    add_room(s, C, H, TUBE, (0.8, 0.6, 0.5), 1)
    verts, idx = unit_cube(O)
    s.add_geometry(verts, idx, cube_mtx((0.2, 0.3, 0.2), 0.4, (0.1, 0.9, 0.0)), (0.4, 0.6, 0.9), 1)
    out["tube"] = (s, (C, H, TUBE), 4, 1)
    s = O.OracleScene()
    C, H = frame("mirrored")
    add_room(s, C, H, OPEN_FRONT, (0.5, 0.8, 0.6), 1)
    out["only_room"] = (s, (C, H, OPEN_FRONT), 5, 0)
    s = O.OracleScene()
    C, H = frame("aligned")
    add_room(s, C, H, CORNER, (0.7, 0.7, 0.5), 1, pattern=2)
    s.add_geometry(np.array([[-0.4, 0.5, 0.1], [0.5, 0.6, -0.2], [0.0, 1.3, 0.3]], np.float32), [0, 1, 2], EYE4, (0.9, 0.3, 0.3), 1)
    out["room_and_triangle"] = (s, (C, H, CORNER), 3, 0)
    return out


def match_frame(C, H, center, axis):
    """The builder's frame (center[3], axis[3, 3]: l' = axis (P - center)) against (C, H): perm[k'] = our axis its axis k' follows, sign[k'] = +-1, and the
    largest deviation of axis @ H from that signed permutation.  Face f' of the builder = 2 perm[k'] + (side' if sign > 0 else 1 - side')."""
    M = np.asarray(axis, np.float64) @ H                   # l' = M l (+ a shift that must vanish)
    perm = np.abs(M).argmax(1)
    sign = np.sign(M[np.arange(3), perm])
    P = np.zeros((3, 3)); P[np.arange(3), perm] = sign
    shift = np.asarray(axis, np.float64) @ (C - np.asarray(center, np.float64))
    return perm, sign, max(float(np.abs(M - P).max()), float(np.abs(shift).max()))


def builder_faces(present, perm, sign):
    """The builder's present-face mask translated to our face numbers."""
    out = []
    for f in range(6):
        if present >> f & 1:
            k, side = f // 2, f & 1
            out.append(2 * int(perm[k]) + (side if sign[k] > 0 else 1 - side))
    return tuple(sorted(out))


# --------------------------------------------------------------------------------------------------------------------------------- float64 geometry
def open_box_f64(C, H, faces, o, d, tmax):
    """THE RULE (trg_device.h trav_room_planes) in float64: the slab test in the room's frame; two candidates, the entry plane at tnear and the exit
    plane at tfar; a candidate counts when tnear <= tfar, its t is in [0, tmax] and its face is present; the nearer counting one is the hit.  A
    direction component that is exactly zero in the frame is parallel: outside that slab a miss, inside no constraint.  Returns (face or -1, t)."""
    A = np.linalg.inv(H)
    lo, ld = (o - C) @ A.T, d @ A.T
    present = np.zeros(6, bool); present[list(faces)] = True
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-1.0 - lo) / ld, (1.0 - lo) / ld
    par = ld == 0.0
    inside = np.abs(lo) <= 1.0
    near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    kn, kf = near.argmax(1), far.argmin(1)
    r = np.arange(len(o))
    tn, tf = near[r, kn], far[r, kf]
    fn = 2 * kn + (ld[r, kn] < 0)                            # towards +l_k: in by the face at -1
    ff = 2 * kf + (ld[r, kf] > 0)
    slab = tn <= tf
    cn = slab & (tn >= 0) & (tn <= tmax) & present[fn]
    cf = slab & (tf >= 0) & (tf <= tmax) & present[ff]
    face = np.where(cn, fn, np.where(cf, ff, -1))
    return face, np.where(cn, tn, np.where(cf, tf, np.inf))


def quads_f64(C, H, faces, o, d, tmax):
    """The room's quads one by one, two-sided parallelograms, float64: (face or -1, t) of the nearest hit in [0, tmax]."""
    best_f, best_t = np.full(len(o), -1), np.full(len(o), np.inf)
    for f in faces:
        p4 = face_quad(C, H, f)
        a, e1, e2 = p4[0], p4[1] - p4[0], p4[3] - p4[0]
        n = np.cross(e1, e2)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a - o) @ n) / (d @ n)
        P = o + t[:, None] * d - a
        # (s, t) in the quad's own basis
        G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
        st = np.linalg.solve(G, np.stack([P @ e1, P @ e2]))
        with np.errstate(invalid="ignore"):
            hit = np.isfinite(t) & (t >= 0) & (t <= tmax) & (st >= 0).all(0) & (st <= 1).all(0) & (t < best_t)
        best_f[hit], best_t[hit] = f, t[hit]
    return best_f, best_t


def edge_distance(C, H, o, d, t):
    """How far the hit point o + t d lies from the nearest edge of the room, in the room's own units (half axes = 1): 1 - the second largest |l_k|."""
    A = np.linalg.inv(H)
    with np.errstate(invalid="ignore"):
        l = np.abs((o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - C) @ A.T)
    return 1.0 - np.sort(l, 1)[:, 1]


# --------------------------------------------------------------------------------------------------------------------------------------------- rays
RAY_KINDS = ("inside", "through_open", "onto_outside", "open_to_open", "off_wall", "tmax_short", "tmax_beyond", "parallel")


def room_rays(C, H, faces, seed, n):
    """About n seeded rays of every kind that applies (float64 origin, direction, maxDistance; kind index):
      inside        from a point inside to a point inside;
      through_open  from outside in through an absent face;
      onto_outside  from outside onto the outer side of a present wall;
      open_to_open  in through one absent face and out through another (rooms with two absent faces);
      off_wall      starting 1e-3 off a present wall along its inward normal, directions cosine-weighted about that normal: the continuation rays
                    the renderer's shading event makes (its own offset; none of them skims the wall it starts from);
      tmax_short / tmax_beyond   towards a present wall with maxDistance 1e-3 short of / beyond it (the any-hit cases);
      parallel      along one half axis or a combination of two: one or two direction components exactly or nearly zero in the room's frame."""
    rng = np.random.default_rng(seed)
    faces = tuple(faces)
    absent = tuple(f for f in ALL_FACES if f not in faces)
    per = max(8, n // len(RAY_KINDS))
    O_, D_, T_, K_ = [], [], [], []

    def w(l):
        return C + l @ H.T

    def on_face(fs, m, reach=0.9):
        f = rng.choice(fs, m)
        l = rng.uniform(-reach, reach, (m, 3))
        l[np.arange(m), f // 2] = np.where(f & 1, 1.0, -1.0)
        return f, l

    def beyond(f, l, lo_, hi_):
        l = l.copy()
        l[np.arange(len(f)), f // 2] *= rng.uniform(lo_, hi_, len(f))
        return l + np.where(np.arange(3)[None, :] == (f // 2)[:, None], 0.0, rng.uniform(-0.5, 0.5, l.shape))

    def emit(o, d, k, tmax=None):
        O_.append(o); D_.append(d); K_.append(np.full(len(o), RAY_KINDS.index(k)))
        T_.append(np.full(len(o), np.inf) if tmax is None else tmax)

    a, b = rng.uniform(-0.95, 0.95, (per, 3)), rng.uniform(-0.95, 0.95, (per, 3))
    emit(w(a), w(b) - w(a), "inside")
    if absent:
        f, l = on_face(absent, per)
        o = w(beyond(f, l, 1.2, 2.5))
        emit(o, w(rng.uniform(-0.9, 0.9, (per, 3))) - o, "through_open")
    f, l = on_face(faces, per)
    o = w(beyond(f, l, 1.2, 2.5))
    emit(o, w(l) - o, "onto_outside")
    if len(absent) >= 2:
        fa, la = on_face(absent, per, 0.6)
        fb, lb = on_face(absent, per, 0.6)
        keep = fa != fb
        o, e = w(beyond(fa, la, 1.3, 2.0))[keep], w(beyond(fb, lb, 1.3, 2.0))[keep]
        emit(o, e - o, "open_to_open")
    f, l = on_face(faces, per)
    nrm = -np.where(f & 1, 1.0, -1.0)[:, None] * np.linalg.inv(H)[f // 2]           # the inward normal of face f: -+ row k of A
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = w(l) + 1e-3 * nrm
    u1, u2 = rng.random(per), rng.random(per)                                     # cosine-weighted hemisphere about nrm
    ct, st, phi = np.sqrt(u1), np.sqrt(1.0 - u1), 2.0 * np.pi * u2
    helper = np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    tx = np.cross(nrm, helper)
    tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(nrm, tx)
    emit(o, nrm * ct[:, None] + tx * (st * np.cos(phi))[:, None] + ty * (st * np.sin(phi))[:, None], "off_wall")
    for kind, delta in (("tmax_short", -1e-3), ("tmax_beyond", 1e-3)):
        f, l = on_face(faces, per)
        o = w(rng.uniform(-0.8, 0.8, (per, 3)))
        d = w(l) - o
        dist = np.linalg.norm(d, axis=1)
        emit(o, d / dist[:, None], kind, dist + delta)
    m = per // 2
    k = rng.integers(0, 3, m)
    d = H[:, k].T * rng.choice([-1.0, 1.0], (m, 1))
    l = rng.uniform(-1.4, 1.4, (m, 3))
    emit(w(l), d, "parallel")
    k2 = (k + 1 + rng.integers(0, 2, m)) % 3
    d = H[:, k].T * rng.uniform(0.3, 1.0, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1)) + H[:, k2].T * rng.uniform(0.3, 1.0, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1))
    emit(w(rng.uniform(-1.4, 1.4, (m, 3))), d, "parallel")
    return np.concatenate(O_), np.concatenate(D_), np.concatenate(T_), np.concatenate(K_)


def as_trace_rays(O, o, d, tmax, mask):
    """fp32 trg_trace records of float64 rays (directions normalised, maxDistance scaled to match)."""
    norm = np.linalg.norm(d, axis=1)
    rays = np.zeros(len(o), O.RAY_DTYPE)
    rays["origin"] = o.astype(np.float32)
    rays["direction"] = (d / norm[:, None]).astype(np.float32)
    rays["maxDistance"] = np.where(np.isfinite(tmax), tmax * norm, np.inf).astype(np.float32)
    rays["mask"] = mask
    return rays


def coincident_f64(positions, indices, o, d, tmax, first_tri, n_room_tris, tol):
    """Rays on which float64 Moeller-Trumbore over ALL triangles finds, within `tol` of the nearest hit's distance, a hit on the other side of the
    room / not-room divide: a face of something that lies IN a wall's plane (the Cornell box's cubes stand on the floor).  Which of the two a
    fp32 test names there is rounding, with the room or without (box leaves: "undecidable in fp32 either way")."""
    T = np.asarray(positions, np.float64).reshape(-1, 3)[np.asarray(indices).reshape(-1)].reshape(-1, 3, 3)
    best = np.full((2, len(o)), np.inf)                                           # nearest hit on a room triangle / on any other
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
            hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0) & (t <= tmax)
        side = 0 if first_tri <= k < first_tri + n_room_tris else 1
        best[side] = np.where(hit & (t < best[side]), t, best[side])
    with np.errstate(invalid="ignore"):
        return np.isfinite(best).all(0) & (np.abs(best[0] - best[1]) < tol)
