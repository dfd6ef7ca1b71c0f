"""Rigs of the rig tests (tests/test_rig_host.py, tests/test_gpu_rig.py): joint forests with keyframed tracks, as include/trg_rig.h takes them.

A rig is a dict: parent [n] uint32 (rig.NO_PARENT: a root), key_first [n + 1] uint32, keys [n_keys, 12] float32 {time, T | R | S, 0},
clock_of [n] uint32, n_clocks, inv_bind [n, 12] float32 or None.

Rig A drives the 38 bones of skin_scenes.scene_a_binding.  Joint 0 (the floor) is a root; the cubes 1 .. 32 hang below it -- 1 .. 8 directly,
9 .. 17 as ONE chain (joint 17 lies 9 levels down), 18 .. 32 in pairs --; 33 is a second root with 34 -> 35 and 36 below it (the sphere's four
bones); 37 a third root whose only key translates by 1e6 (the bone only zero weights name).  A joint sits at its object's centre, so its inverse
bind is a translation by minus that centre -- not the identity -- and a cube's bone is ONE affine matrix: every box and every quad leaf
survives.  Joints have 7, 2 or 1 keys (j % 3); key 3 of a seven-key track and key 1 of every other two-key track are stored NEGATED (the same
rotation, a negative dot with the key before); the sphere's root is mirrored (a negative scale), only there: the sphere has no quad or box leaves.
Joints below 20 run on clock 0, the others on clock 1.  CLOCKS_A puts a clock before every first key, exactly on an inner key time, between keys
(across the negated pair) and past every last key.

Rig B has no scene: 700 joints on 12 levels of 5, 257, 300, 40, 30, 20, 15, 12, 10, 6, 4 and 1 joints -- a level of one block plus one thread,
one of two blocks, one of a single joint --, five roots, numbered in a random order that only keeps parents before children, five clocks, random
tracks of 1, 2, 3 or 7 keys with negated rotations and negative scales, random inverse binds.

The Cornell chain is the app's (toyraygun_cornell ... bend=DEG rig): three joints up the short box's vertical axis."""
import numpy as np

from tests import refit_scenes as RS
from tests import skin_scenes as SS

NO_PARENT = 0xFFFFFFFF
TIMES7 = (0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0)
CHAIN = tuple(range(9, 18))
CLOCKS_A = {"before": (-0.5, -1.0), "on a key": (0.25, 0.75), "between": (0.6, 0.4), "past": (2.0, 3.0), "mixed": (0.7, 2.0)}
B_LEVELS = (5, 257, 300, 40, 30, 20, 15, 12, 10, 6, 4, 1)


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])


def _tracks(rest_T, n_keys_of, rng, angle, shift, scale, two_times=(0.0, 1.0)):
    """key_first and keys of joints that rest at the local translations rest_T: key 0 is the rest pose, the others random about it."""
    key_first, keys = [0], []
    for j, nk in enumerate(n_keys_of):
        times = {1: (0.0,), 2: two_times, 7: TIMES7}[nk]
        for i, t in enumerate(times):
            q = _quat(rng.normal(size=3), 0.0 if i == 0 and nk > 1 else rng.uniform(-angle, angle))
            if (nk == 7 and i == 3) or (nk == 2 and i == 1 and j % 2 == 1):
                q = -q
            T = rest_T[j] + (0.0 if i == 0 and nk > 1 else rng.uniform(-shift, shift, 3))
            S = np.ones(3) if i == 0 and nk > 1 else rng.uniform(1 - scale, 1 + scale, 3)
            keys.append(np.concatenate([[t], T, q, S, [0.0]]))
        key_first.append(len(keys))
    return np.array(key_first, np.uint32), np.array(keys, np.float64)


def rig_a():
    n = SS.N_BONES
    centre = np.zeros((n, 3))
    for i in range(RS.N_CUBES):
        centre[1 + i] = RS._cube_map(i, 0)[1]
    centre[33:37] = RS.SPHERE_CENTER
    parent = np.full(n, NO_PARENT, np.int64)
    parent[1:9] = 0
    parent[CHAIN[0]] = 0
    for j in CHAIN[1:]:
        parent[j] = j - 1
    for j in range(18, 33):
        parent[j] = 0 if j % 2 == 0 else j - 1
    parent[34], parent[35], parent[36] = 33, 34, 33
    rest_T = np.array([centre[j] - (centre[parent[j]] if parent[j] != NO_PARENT else 0.0) for j in range(n)])
    n_keys_of = [(7, 2, 1)[j % 3] for j in range(n)]
    n_keys_of[37] = 1
    rng = np.random.default_rng(4100)
    key_first, keys = _tracks(rest_T, n_keys_of, rng, 0.15, 0.03, 0.05)
    keys[key_first[33]:key_first[34], 8] *= -1.0                      # the sphere's root is mirrored, in every key
    keys[key_first[37], 1:4] = (1.0e6, -1.0e6, 1.0e6)
    inv_bind = np.tile(np.eye(3, 4).reshape(1, 12), (n, 1))
    inv_bind[:, [3, 7, 11]] = -centre
    clock_of = (np.arange(n) >= 20).astype(np.uint32)
    return dict(parent=parent.astype(np.uint32), key_first=key_first, keys=np.ascontiguousarray(keys.astype(np.float32)), clock_of=clock_of, n_clocks=2,
                inv_bind=np.ascontiguousarray(inv_bind.astype(np.float32)))


def rig_b():
    rng = np.random.default_rng(4200)
    level_of, par = [], []
    first = np.concatenate([[0], np.cumsum(B_LEVELS)])
    for l, count in enumerate(B_LEVELS):
        for _ in range(count):
            level_of.append(l)
            par.append(-1 if l == 0 else int(rng.integers(first[l - 1], first[l])))
    n = len(par)
    # renumber: a random order that keeps every parent before its children
    children = [[] for _ in range(n)]
    for j, p in enumerate(par):
        if p >= 0:
            children[p].append(j)
    ready, new_of, k = [j for j in range(n) if par[j] < 0], np.empty(n, np.int64), 0
    while ready:
        j = ready.pop(int(rng.integers(len(ready))))
        new_of[j] = k
        k += 1
        ready += children[j]
    parent = np.full(n, NO_PARENT, np.int64)
    for j, p in enumerate(par):
        if p >= 0:
            parent[new_of[j]] = new_of[p]
    key_first, keys = [0], []
    for j in range(n):
        nk = int(rng.choice([1, 2, 3, 7]))
        t = rng.uniform(-0.2, 0.2) + np.concatenate([[0.0], np.cumsum(rng.uniform(0.1, 0.5, nk - 1))])
        for i in range(nk):
            q = _quat(rng.normal(size=3), rng.uniform(-np.pi, np.pi)) * rng.choice([-1.0, 1.0])
            S = rng.uniform(0.7, 1.3, 3) * rng.choice([-1.0, 1.0], 3, p=[0.2, 0.8])
            keys.append(np.concatenate([[t[i]], rng.uniform(-1, 1, 3), q, S, [0.0]]))
        key_first.append(len(keys))
    inv_bind = np.zeros((n, 3, 4))
    for j in range(n):
        inv_bind[j, :, :3] = RS._rot(rng.normal(size=3), rng.uniform(-np.pi, np.pi)) @ np.diag(rng.uniform(0.8, 1.25, 3))
        inv_bind[j, :, 3] = rng.uniform(-1, 1, 3)
    return dict(parent=parent.astype(np.uint32), key_first=np.array(key_first, np.uint32), keys=np.ascontiguousarray(np.array(keys).astype(np.float32)),
                clock_of=rng.integers(0, 5, n).astype(np.uint32), n_clocks=5, inv_bind=np.ascontiguousarray(inv_bind.reshape(n, 12).astype(np.float32)))


def clocks_b(r):
    """name -> [5] float32: before every track, past every track, between keys, and clocks that sit exactly on inner key times."""
    kf, keys, co = r["key_first"].astype(np.int64), r["keys"], r["clock_of"]
    inner = {}
    for j in range(kf.shape[0] - 1):
        if kf[j + 1] - kf[j] >= 3 and int(co[j]) not in inner:
            inner[int(co[j])] = keys[kf[j] + 1, 0]
    assert len(inner) == 5
    rng = np.random.default_rng(4300)
    return {"before": np.full(5, -10.0, np.float32), "past": np.full(5, 100.0, np.float32), "between": rng.uniform(0.0, 1.5, 5).astype(np.float32),
            "on a key": np.array([inner[k] for k in range(5)], np.float32), "mixed": np.array([-10.0, 0.3, 100.0, 0.9, inner[4]], np.float32)}


def args(r):
    """The rig as rig.bind / rig.check_rig take it, after the context."""
    return r["parent"], r["key_first"], r["keys"], r["clock_of"], r["n_clocks"], r["inv_bind"]


def reference(r, clocks):
    from toyraygun_amd import rig
    return rig.rig_reference(r["parent"], r["key_first"], r["keys"], r["clock_of"], clocks, r["inv_bind"])


def bad_rigs(r):
    """name -> (rig, what check_rig says, joint, key, word the C text has), one per validator of trg_rig_bind, in its order."""
    def changed(**kw):
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
        for k, f in kw.items():
            out[k] = f(out[k]) if callable(f) else f
        return out

    def at(i, col, value):
        def f(a):
            a[i, col] = value
            return a
        return f

    def at1(i, value):
        def f(a):
            a[i] = value
            return a
        return f
    kf = r["key_first"].astype(np.int64)
    j7 = next(j for j in range(kf.shape[0] - 1) if kf[j + 1] - kf[j] == 7 and j > 3)
    out = {}
    out["no clocks"] = (changed(n_clocks=0), "counts", None, None, "zero")
    out["a parent after its child"] = (changed(parent=at1(5, 5)), "parent", 5, None, "parent")
    out["a table that begins at 1"] = (changed(key_first=at1(0, 1)), "table", 0, None, "begins")
    out["a joint without a key"] = (changed(key_first=at1(4, kf[5])), "table", 4, None, "ascending")
    out["a table that ends early"] = (changed(key_first=at1(kf.shape[0] - 1, kf[-1] + 1)), "table", kf.shape[0] - 2, None, "ends")
    out["a time that goes back"] = (changed(keys=at(kf[j7] + 2, 0, r["keys"][kf[j7] + 1, 0])), "time", j7, int(kf[j7] + 2), "time")
    out["a NaN scale"] = (changed(keys=at(kf[6], 9, np.nan)), "ts", 6, int(kf[6]), "translation or a scale")
    out["a rotation of length 1.1"] = (changed(keys=at(kf[7], slice(4, 8), r["keys"][kf[7], 4:8] * np.float32(1.1))), "rotation", 7, int(kf[7]), "rotation")
    out["a clock out of range"] = (changed(clock_of=at1(11, r["n_clocks"])), "clock", 11, None, "clock")
    out["an infinite inverse bind"] = (changed(inv_bind=at(13, 7, np.inf)), "inv_bind", 13, None, "inverse bind")
    return out


def deep_rig(depth=65):
    """One chain of `depth` joints: 65 is one level too many (TRG_ERR_RANGE), 64 is accepted."""
    parent = np.concatenate([[NO_PARENT], np.arange(depth - 1)]).astype(np.uint32)
    keys = np.tile(np.array([0, 0.01, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0], np.float32), (depth, 1))
    return dict(parent=parent, key_first=np.arange(depth + 1, dtype=np.uint32), keys=keys, clock_of=np.zeros(depth, np.uint32), n_clocks=1, inv_bind=None)


# ---------------------------------------------------------------------------------------------------------------------------- the Cornell box
def cornell_chain(b, degrees):
    """(rig, ids, weights) of the app's `bend=DEG rig` over the Cornell box's per-corner buffers, degrees = DEG x (calls - 1): the short box is the
    first 36 vertices; joints 0, 1, 2 stand on its vertical axis at its foot, half way up and at its top, each the child of the one below; key 0
    (time 0) is the rest pose, key 1 (time 1) has every joint turned by `degrees` about the x axis through its origin.  A corner leans on the
    joints by its height: weight max(0, 1 - |2 h - k|) on joint k, h its height within the box in 0 .. 1.  Everything else follows joint 0 -- which
    does not move: its origin is on the floor, and it turns; so the rest of the scene is bound to a FOURTH joint, a root with one key at rest."""
    pos = np.asarray(b["positions"], np.float32)
    box = pos[:36].astype(np.float64)
    lo, hi = box[:, 1].min(), box[:, 1].max()
    cx, cz = (box[:, 0].min() + box[:, 0].max()) / 2, (box[:, 2].min() + box[:, 2].max()) / 2
    origin = np.array([[cx, lo + (hi - lo) * k / 2, cz] for k in range(3)] + [[0.0, 0.0, 0.0]])
    a = degrees * 3.14159265358979323846 / 180.0
    turned = np.array([np.sin(a / 2), 0.0, 0.0, np.cos(a / 2)])
    keys = []
    for k in range(3):
        T = origin[k] - (origin[k - 1] if k else 0.0)
        keys.append(np.concatenate([[0.0], T, [0, 0, 0, 1], [1, 1, 1, 0]]))
        keys.append(np.concatenate([[1.0], T, turned, [1, 1, 1, 0]]))
    keys.append(np.array([0.0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0]))
    inv_bind = np.tile(np.eye(3, 4).reshape(1, 12), (4, 1))
    inv_bind[:, [3, 7, 11]] = -origin
    r = dict(parent=np.array([NO_PARENT, 0, 1, NO_PARENT], np.uint32), key_first=np.array([0, 2, 4, 6, 7], np.uint32),
             keys=np.ascontiguousarray(np.array(keys).astype(np.float32)), clock_of=np.zeros(4, np.uint32), n_clocks=1,
             inv_bind=np.ascontiguousarray(inv_bind.astype(np.float32)))
    ids = np.tile(np.array([0, 1, 2, 3], np.uint32), (pos.shape[0], 1))
    w = np.zeros((pos.shape[0], 4), np.float32)
    w[36:, 3] = 1.0
    h = (box[:, 1] - lo) / (hi - lo)
    for k in range(3):
        w[:36, k] = np.maximum(0.0, 1.0 - np.abs(2.0 * h - k)).astype(np.float32)
    return r, ids, w
