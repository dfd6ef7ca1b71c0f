"""Targets of the blend-shape tests (tests/test_morph_host.py, tests/test_gpu_morph.py) over the scenes of tests/refit_scenes.py.

Scene A (706 triangles; 2,118 vertices per corner = 8 x 256 + 70, 424 indexed = 256 + 168; 6,354 corners = 24 x 256 + 210) with N_TARGETS = 7.
Whatever a target does to a vertex is a function of the vertex's rest position and its object alone, so the copies of a shared corner get equal
deltas and stay equal.
  T0  the floor and every cube shifted by a vector of its own: deltas equal within an object, which stays the box or quad it was.
  T1  every cube stretched about its own centre, d = 0.5 (p - centre) rounded once: a parallelepiped stays one.
  T2  the sphere's upper half bulged radially, WITH normal deltas.
  T3  empty.  (one_corner=True: all copies of ONE top corner of cube 9 moved by 0.02 -- no box any more: the refusal case.)
  T4  the sphere again, a second shape with normal deltas -- but for the vertices whose position hash is a multiple of 8, so that vertices
      with no entry at all exist: an upper sphere vertex holds two, three or four entries, a cube's two or three.
  T5  deltas of 1e6 on a scattering of vertices of every object.  ALWAYS given weight 0: a wrong weight index shows.
  T6  = N_TARGETS - 1, sparse: vertex 0, vertex n_verts - 1, the two vertices no triangle names (indexed scene) and a scattering of the sphere's.
      Where one of those belongs to the floor or a cube, the whole object is shifted with it (it has to stay a quad or a box).
The normal deltas of T5 are 1e6 too; T0, T1 and T6 carry zero normal deltas on the floor and the cubes -- an ACTIVE entry: the corner is
renormalised -- and T6 non-zero ones on the sphere.  The indexed scene has one -0.0 coordinate: the y of a floor vertex.

The Cornell box with one target: the copies of the short box's four top corners, each moved by its offset from the box's vertical axis."""
import numpy as np

from tests import refit_scenes as RS
from tests import skin_scenes as SS

N_TARGETS = 7
EMPTY, ALWAYS_ZERO, LAST = 3, 5, N_TARGETS - 1
REFUSED_CUBE = 9

# every weight vector the GPU tests apply (T5 always zero, of either sign; T3 is empty, or the refusal case: zero here).  The first five are
# (T0, T1, T2) vectors the box and quad rules were tried under; tests/test_morph_host.py checks every one, alone and under every bone seed
WEIGHTS = {
    "a": (0.7, -0.4, 1.0, 0.0, 0.5, 0.0, 1.0),
    "b": (1.0, 1.0, 0.5, 0.0, -0.8, -0.0, 0.25),
    "c": (-1.5, 0.9, -0.3, 0.0, 1.0, 0.0, -1.0),
    "d": (0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "e": (0.0, 0.61, 0.0, 0.0, 0.0, -0.0, 0.0),
    "last": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.75),
}
ZERO = (0.0, -0.0, 0.0, 0.0, -0.0, 0.0, 0.0)
BONE_SEEDS = (1, 2, 3)


def weights(name):
    return np.array(WEIGHTS[name] if isinstance(name, str) else name, np.float32)


def scene(indexed):
    """Scene A at rest, per corner or indexed; the indexed one with the y of one floor vertex set to -0.0 (it was +0.0: the same geometry)."""
    if not indexed:
        return RS.scene_a(0)
    b = RS.scene_a_indexed(0)
    pos = b["positions"].copy()
    v = int(np.flatnonzero(SS._objects(b) == 0)[0])
    assert pos[v, 1] == 0 and not np.signbit(pos[v, 1])
    pos[v, 1] = np.float32(-0.0)
    return dict(b, positions=pos)


def minus_zero_vertex(b):
    rows = np.flatnonzero(np.signbit(b["positions"][:, 1]) & (b["positions"][:, 1] == 0))
    assert rows.shape[0] == 1
    return int(rows[0])


def _hash(pos):
    """A number per vertex from the bits of its rest position (-0.0 counted as 0.0): equal for the copies of a corner, and in both forms of the scene."""
    w = (np.asarray(pos, np.float32) + np.float32(0)).view(np.uint32).astype(np.uint64)
    h = (w[:, 0] * np.uint64(2654435761) + w[:, 1] * np.uint64(40503) + w[:, 2] * np.uint64(2246822519)) >> np.uint64(7)
    return (h % np.uint64(1000003)).astype(np.int64)


def targets(b, one_corner=False):
    """(target_first [8] uint32, entry_vertex [n] uint32, dpos [n, 3] float32, dnrm [n, 3] float32) of scene A's buffers `b`."""
    pos = np.asarray(b["positions"], np.float32)
    p64 = pos.astype(np.float64)
    obj = SS._objects(b)
    nv = pos.shape[0]
    h = _hash(pos)
    rigid = (obj >= 0) & (obj != SS.SPHERE_OBJECT)
    sphere = obj == SS.SPHERE_OBJECT
    u = (p64 - RS.SPHERE_CENTER) / 0.3
    lists = []

    def shift_of(o, salt):
        return np.random.default_rng(7000 + 100 * salt + int(o)).uniform(-0.03, 0.03, 3)
    # T0
    v = np.flatnonzero(rigid)
    lists.append((v, np.stack([shift_of(o, 0) for o in obj[v]]), np.zeros((v.shape[0], 3))))
    # T1
    v = np.flatnonzero(rigid & (obj != 0))
    centre = np.zeros((nv, 3))
    for o in range(1, 1 + RS.N_CUBES):
        mine = np.flatnonzero(obj == o)
        centre[mine] = np.unique(pos[mine], axis=0).astype(np.float64).mean(0)
    lists.append((v, 0.5 * (p64[v] - centre[v]), np.zeros((v.shape[0], 3))))
    # T2
    v = np.flatnonzero(sphere & (u[:, 1] > 0))
    lists.append((v, 0.12 * u[v] * u[v, 1:2], 0.5 * u[v] + np.array([0.3, 0.0, -0.2])))
    # T3
    if one_corner:
        mine = np.flatnonzero(obj == 1 + REFUSED_CUBE)
        corners = np.unique(pos[mine], axis=0)
        top = corners[np.argmax(corners[:, 1])]
        v = mine[(pos[mine] == top).all(1)]
        lists.append((v, np.tile([0.0, 0.02, 0.0], (v.shape[0], 1)), np.zeros((v.shape[0], 3))))
    else:
        lists.append((np.zeros(0, np.int64), np.zeros((0, 3)), np.zeros((0, 3))))
    # T4
    v = np.flatnonzero(sphere & (h % 8 != 0))
    wave = np.sin(6.0 * u[v, 0:1]) * np.cos(5.0 * u[v, 2:3])
    lists.append((v, 0.04 * wave * u[v] + np.array([0.01, 0.0, 0.02]), 0.4 * wave * np.array([0.0, 1.0, 0.5]) - 0.1 * u[v]))
    # T5
    firsts = np.array([np.flatnonzero(obj == o)[0] for o in range(SS.SPHERE_OBJECT + 1)])
    pick = h % 5 == 1
    pick[firsts] = True
    v = np.flatnonzero(pick)
    lists.append((v, np.full((v.shape[0], 3), 1.0e6), np.full((v.shape[0], 3), -1.0e6)))
    # T6
    pick = (obj < 0) | (sphere & (h % 3 == 0))
    for end in (0, nv - 1):
        pick |= (obj == obj[end]) if rigid[end] else (np.arange(nv) == end)
    v = np.flatnonzero(pick)
    dp = np.where(rigid[v, None], np.stack([shift_of(max(o, 0), 6) for o in obj[v]]), 0.05 * np.cos(3.0 * p64[v] + 1.0))
    dn = np.where(sphere[v, None], 0.6 * np.sin(4.0 * p64[v]), 0.0)
    lists.append((v, dp, dn))
    assert len(lists) == N_TARGETS
    first = np.concatenate([[0], np.cumsum([l[0].shape[0] for l in lists])]).astype(np.uint32)
    return (first, np.concatenate([l[0] for l in lists]).astype(np.uint32), np.ascontiguousarray(np.concatenate([l[1] for l in lists]).astype(np.float32)),
            np.ascontiguousarray(np.concatenate([l[2] for l in lists]).astype(np.float32)))


def entries_per_vertex(t, n_verts):
    return np.bincount(t[1].astype(np.int64), minlength=n_verts)


def bad_targets(b):
    """name -> (target_first, entry_vertex, dpos, dnrm, n_entries or None, what check_targets says, words the C text has) of targets
    trg_morph_bind refuses."""
    first, ev, dp, dn = targets(b)
    nv = b["positions"].shape[0]
    out = {}
    f = first.copy(); f[0] = 1
    out["first[0] != 0"] = (f, ev, dp, dn, None, ("first", 0, None), ("target 0 ", "not at 0"))
    f = first.copy(); f[2] = f[1] - 1
    out["a descending table"] = (f, ev, dp, dn, None, ("order", 1, None), ("target 1 ", "descending"))
    out["a wrong end"] = (first, ev, dp, dn, ev.shape[0] - 1, ("end", N_TARGETS - 1, None), ("target %d " % (N_TARGETS - 1), "%d entries" % (ev.shape[0] - 1)))
    e = int(first[1]) + 5
    x = ev.copy(); x[e] = nv
    out["a vertex out of range"] = (first, x, dp, dn, None, ("vertex", 1, e), ("entry %d of target 1 " % e, "vertex %d" % nv))
    e = int(first[4]) + 3
    x = ev.copy(); x[e] = x[e - 1]
    out["a repeated vertex"] = (first, x, dp, dn, None, ("repeat", 4, e), ("entry %d of target 4 " % e, "ascending"))
    e = int(first[2]) + 1
    x = dp.copy(); x[e, 2] = np.nan
    out["a NaN delta"] = (first, ev, x, dn, None, ("delta", 2, e), ("entry %d of target 2 " % e, "position delta", "not finite"))
    e = int(first[6])
    x = dn.copy(); x[e, 0] = np.inf
    out["an infinite normal delta"] = (first, ev, dp, x, None, ("normal delta", 6, e), ("entry %d of target 6 " % e, "normal delta", "not finite"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the Cornell box
def cornell_axis(b):
    """The short box's vertical axis (x, z) as toyraygun_cornell forms it: the mean over the box's 36 corners, summed in double in their order."""
    x = z = 0.0
    for p in np.asarray(b["positions"], np.float32)[:36]:
        x += float(p[0]) / 36.0
        z += float(p[2]) / 36.0
    return x, z


def cornell_bulge(b):
    """(target_first, entry_vertex, dpos) of the Cornell box's per-corner buffers: one target, the copies of the short box's four top corners
    (the short box is the first 36 vertices), each delta the corner's offset from the box's vertical axis -- toyraygun_cornell's morph option."""
    pos = np.asarray(b["positions"], np.float32)
    box = pos[:36]
    top = np.flatnonzero(box[:, 1] == box[:, 1].max())
    axis = cornell_axis(b)
    d = np.zeros((top.shape[0], 3), np.float32)
    d[:, 0] = box[top, 0] - np.float32(axis[0])
    d[:, 2] = box[top, 2] - np.float32(axis[1])
    return np.array([0, top.shape[0]], np.uint32), top.astype(np.uint32), d


def cornell_app_bones(b, degrees):
    """[2, 12]: the identity and the turn by `degrees` about the box's axis, formed in double and rounded once as toyraygun_cornell does."""
    ax, az = cornell_axis(b)
    t = degrees * 3.14159265358979323846 / 180.0
    cs, sn = float(np.cos(t)), float(np.sin(t))
    B = np.tile(np.eye(3, 4), (2, 1, 1))
    B[1, 0, 0], B[1, 0, 2], B[1, 0, 3] = cs, sn, ax - cs * ax - sn * az
    B[1, 2, 0], B[1, 2, 2], B[1, 2, 3] = -sn, cs, az + sn * ax - cs * az
    return np.ascontiguousarray(B.reshape(2, 12).astype(np.float32))
