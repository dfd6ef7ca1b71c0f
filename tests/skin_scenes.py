"""Bones and weights of the skinning tests (tests/test_skin_host.py, tests/test_gpu_skin.py) over the scenes of tests/refit_scenes.py.

Scene A with N_BONES = 38 bones.  Bones 0 .. 32: the floor and each of the 32 cubes, one bone at weight 1 -- their matrices are
pose_scenes.scene_a_xforms(seed)'s, which keep every box and every quad (tests/test_pose_host.py), and a one-hot blend is that matrix.  Bones
33 .. 36: the sphere's, four maps about its centre; each of its 162 shared vertices is blended over them by its position (bilinear in x and y:
four non-zero weights), and the vertices of its upper part (z above 0.5 radii) over THREE -- the smallest weight is dropped, the others rescaled,
and the dropped slot names bone 37 at weight 0.  The weights are multiples of 2^-10 that sum to exactly 1: identity bones give the rest pose
back under ==.  Bone 37 = N_BONES - 1 is named by zero weights only; its matrix is large, so a weight that did
not multiply it away would show.  A vertex no triangle names (the indexed scene has two) follows the floor's bone: it moves.
The copies of a shared corner get equal ids and weights: both are functions of the corner's rest position and its object alone.

The Cornell box with two bones: bone 0 the identity, bone 1 a turn about the short box's vertical axis; the short box's corners lean on bone 1
by their height within the box, everything else has weight 1 on bone 0."""
import numpy as np

from tests import pose_scenes as PS
from tests import refit_scenes as RS

N_BONES = 38
SPHERE_BONES = (33, 34, 35, 36)
LAST_BONE = N_BONES - 1
SPHERE_OBJECT = PS.N_OBJECTS_A - 1


def _objects(b):
    """vertex -> object of scene A's buffers (floor 0, cubes 1 .. 32, sphere 33; -1: named by no triangle)."""
    first = PS.scene_a_first().astype(np.int64)
    idx = np.asarray(b["indices"], np.int64).reshape(-1)
    tri_obj = np.repeat(np.arange(first.shape[0] - 1), np.diff(first))
    vtx_obj = np.full(b["positions"].shape[0], -1, np.int64)
    vtx_obj[idx] = np.repeat(tri_obj, 3)
    return vtx_obj


def scene_a_binding(b, split_cube=None):
    """(bone_ids [n_verts, 4] uint32, weights [n_verts, 4] float32) of scene A's buffers `b` (per corner or indexed), as described above.
    split_cube=i: the corners of cube i that lie above its centre follow the bone of cube (i + 1) % 32 instead of their own -- eight corners
    split between two bones, which is no box under two different matrices."""
    pos = np.asarray(b["positions"], np.float32)
    obj = _objects(b)
    nv = pos.shape[0]
    ids = np.zeros((nv, 4), np.uint32)
    w = np.zeros((nv, 4), np.float64)
    w[:, 0] = 1.0
    rigid = obj != SPHERE_OBJECT
    ids[rigid, 0] = np.where(obj[rigid] < 0, 0, obj[rigid]).astype(np.uint32)
    sph = np.flatnonzero(~rigid)
    u = (pos[sph].astype(np.float64) - RS.SPHERE_CENTER) / 0.3
    a, c = np.clip((1 + u[:, 0]) / 2, 0.1, 0.9), np.clip((1 + u[:, 1]) / 2, 0.1, 0.9)
    ws = np.stack([(1 - a) * (1 - c), a * (1 - c), (1 - a) * c, a * c], axis=1)
    sid = np.tile(np.array(SPHERE_BONES, np.uint32), (sph.shape[0], 1))
    three = u[:, 2] > 0.5
    drop = ws.argmin(1)
    rows = np.flatnonzero(three)
    ws[rows, drop[rows]] = 0.0
    sid[rows, drop[rows]] = LAST_BONE
    ws /= ws.sum(1, keepdims=True)
    # multiples of 2^-10, the largest weight taking the remainder: the four sum to exactly 1 in fp32, in any order
    ws = np.round(ws * 1024.0) / 1024.0
    big = ws.argmax(1)
    every = np.arange(ws.shape[0])
    ws[every, big] = 0.0
    ws[every, big] = 1.0 - ws.sum(1)
    ids[sph], w[sph] = sid, ws
    if split_cube is not None:
        mine = np.flatnonzero(obj == 1 + split_cube)
        centre = pos[mine].astype(np.float64).mean(0)
        ids[mine[pos[mine, 1] > centre[1]], 0] = 1 + (split_cube + 1) % RS.N_CUBES
    return ids, np.ascontiguousarray(w.astype(np.float32))


def scene_a_bones(seed, share=None):
    """[38, 12] float32: the bones of scene A, a function of the seed.  share=(i, j): bone j is given bone i's matrix -- a cube whose corners are
    split between the two is then still the image of a cube under one matrix."""
    X = PS.scene_a_xforms(seed)
    rng = np.random.default_rng(9000 + seed)
    B = np.zeros((N_BONES, 3, 4))
    B[:33] = X[:33].reshape(33, 3, 4)
    for k in SPHERE_BONES:
        A = RS._rot(rng.normal(size=3), rng.uniform(-0.5, 0.5)) @ np.diag(rng.uniform(0.8, 1.25, 3))
        B[k] = PS._about(A, RS.SPHERE_CENTER, rng.uniform(-0.08, 0.08, 3))
    B[LAST_BONE] = rng.uniform(-1, 1, (3, 4)) * 1.0e6
    if share is not None:
        B[share[1]] = B[share[0]]
    return np.ascontiguousarray(B.reshape(N_BONES, 12).astype(np.float32))


def identity(n_bones=N_BONES):
    return PS.identity(n_bones)


def one_hot(b):
    """Scene A's buffers bound as scene A's 34 OBJECTS: every vertex weight 1 on its object's bone (the sphere rigid); for the comparison with
    trg_pose_apply.  A vertex no triangle names never moves under a pose: here it gets bone 34, which the caller sets to the identity.
    Returns (ids, weights, n_bones = 35)."""
    obj = _objects(b)
    ids = np.zeros((obj.shape[0], 4), np.uint32)
    ids[:, 0] = np.where(obj < 0, PS.N_OBJECTS_A, obj).astype(np.uint32)
    w = np.zeros((obj.shape[0], 4), np.float32)
    w[:, 0] = 1.0
    return ids, w, PS.N_OBJECTS_A + 1


def posed_buffers(b, pos, nrm):
    return PS.posed_buffers(b, pos, nrm)


def bad_bindings(b):
    """name -> (ids, weights, first offending vertex, word the error names) of bindings trg_skin_bind refuses, and one it accepts."""
    ids, w = scene_a_binding(b)
    out = {}
    i = ids.copy(); i[17, 2] = N_BONES
    out["a bad id"] = (i, w, 17, "bone")
    x = w.copy(); x[5] = (1.25, -0.25, 0, 0)
    out["a negative weight"] = (ids, x, 5, "negative")
    x = w.copy(); x[300, 1] = np.nan
    out["a NaN weight"] = (ids, x, 300, "not finite")
    x = w.copy(); x[41] = (0.5, 0.501, 0, 0)
    out["a sum off by 1e-3"] = (ids, x, 41, "sum")
    x = w.copy(); x[1200] = (0.5, np.float32(0.5) + np.float32(1e-6), 0, 0)     # (a vertex of the sphere: no quad or box leaf depends on it)
    out["a sum off by 1e-6"] = (ids, x, None, None)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the Cornell box
def cornell_binding(b):
    """(ids, weights, n_bones = 2, axis (x, z)) of the Cornell box's per-corner buffers: the short box is the first 36 vertices."""
    pos = np.asarray(b["positions"], np.float32)
    box = pos[:36]
    lo, hi = box[:, 1].min(), box[:, 1].max()
    ids = np.zeros((pos.shape[0], 4), np.uint32)
    ids[:, 1] = 1
    w = np.zeros((pos.shape[0], 4), np.float32)
    w[:36, 1] = (box[:, 1] - lo) / (hi - lo)
    w[:, 0] = np.float32(1) - w[:, 1]
    return ids, w, 2, (float(box[:, 0].astype(np.float64).mean()), float(box[:, 2].astype(np.float64).mean()))


def twist_bones(axis, degrees):
    """[2, 12]: the identity, and a turn by `degrees` about the vertical through axis = (x, z)."""
    t = np.deg2rad(degrees)
    R = RS._rot((0, 1, 0), t)
    c = np.array([axis[0], 0.0, axis[1]])
    return np.ascontiguousarray(np.stack([np.eye(3, 4), PS._about(R, c, (0, 0, 0))]).reshape(2, 12).astype(np.float32))
