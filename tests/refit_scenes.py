"""Moving scenes of the refit tests (tests/test_refit_host.py, tests/test_gpu_refit.py, tests/test_gpu_refit_shapes.py): per-corner buffers as trg_load_scene takes them, a function
of the step, so that "moved" is the same geometry for the library, the oracle and a fresh load.

Scene A: a floor quad, a 4 x 4 x 2 lattice of rotated cubes (384 triangles: box leaves of the host builder) and a 320-triangle icosphere with smooth
normals -- 706 triangles, too many for the LDS tier.  Step s: every cube gets its own rigid-plus-shear map, the sphere a sinusoidal per-vertex
deformation with recomputed normals; step 0 is the scene as loaded.
Scene B: the Cornell box with its short box slid by 0.02 per step along x (and, for the small-scene path, turned about its own axis).
For tests/test_gpu_refit_shapes.py: scene A as an indexed mesh, with a collapsed edge, and far from the origin; the 263,460-triangle cube
lattice, every cube moved."""
import numpy as np

# a cube's corners and its faces in the (a, b, c) (a, c, d) pattern of the reference's addCube: six quads, each two triangles sharing their first vertex
_CORNERS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64)
_FACES = ((0, 1, 2, 3), (5, 4, 7, 6), (4, 0, 3, 7), (1, 5, 6, 2), (3, 2, 6, 7), (4, 5, 1, 0))
CUBE_CORNER_ORDER = np.array([[f[0], f[1], f[2], f[0], f[2], f[3]] for f in _FACES]).reshape(-1)      # 36 corner numbers
N_CUBES = 32
FLOOR_TRIS, CUBE_TRIS, SPHERE_TRIS = 2, 12 * N_CUBES, 320
SPHERE_CENTER = np.array([0.35, 1.45, 0.25])


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _icosphere():
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(2):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int64)


_SPHERE_V, _SPHERE_F = _icosphere()
assert _SPHERE_F.shape[0] == SPHERE_TRIS


def _cube_map(i, step):
    """3 x 3 matrix and translation of cube i at `step`: its place in the lattice, its own rotation, and -- from step 1 on -- its own rigid-plus-shear motion."""
    rng = np.random.default_rng(1000 + i)
    ix, iy, iz = i % 4, (i // 4) % 4, i // 16
    pos = np.array([-0.66 + 0.44 * ix, 0.22 + 0.3 * iy, -0.7 + 0.55 * iz])
    base = _rot(rng.normal(size=3), rng.uniform(0, np.pi)) @ np.diag(rng.uniform(0.05, 0.09, 3))
    ax, w, sh, drift = rng.normal(size=3), rng.uniform(-0.25, 0.25), rng.uniform(-0.2, 0.2), rng.uniform(-0.02, 0.02, 3)
    S = np.eye(3)
    S[0, 1] = sh * step
    return _rot(ax, w * step) @ S @ base, pos + drift * step


def _sphere_normals(v):
    """Area-weighted vertex normals of the sphere's mesh over the vertices `v` (float64); a triangle of no area adds nothing."""
    tri = v[_SPHERE_F]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, _SPHERE_F[:, k], fn)
    return vn / np.linalg.norm(vn, axis=1, keepdims=True)


def scene_a(step=0):
    """dict(positions [3n, 3], normals [3n, 3], colors [3n, 3], indices [3n], material_ids [n]) of scene A at `step`, float32 / uint32."""
    P, N, Cc, M = [], [], [], []
    fl = np.array([[-1.2, 0, -1.2], [1.2, 0, -1.2], [1.2, 0, 1.2], [-1.2, 0, 1.2]], np.float64)
    P.append(fl[[0, 1, 2, 0, 2, 3]]); N.append(np.tile([0.0, 1.0, 0.0], (6, 1))); Cc.append(np.tile([0.7, 0.7, 0.65], (6, 1))); M += [1, 1]
    for i in range(N_CUBES):
        A, t = _cube_map(i, step)
        corners = (_CORNERS @ A.T + t).astype(np.float32)                  # rounded ONCE per corner: the copies of a corner stay equal
        p = corners[CUBE_CORNER_ORDER].astype(np.float64)
        P.append(p)
        tri = p.reshape(12, 3, 3)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        N.append(np.repeat(n, 3, axis=0))
        rng = np.random.default_rng(2000 + i)
        Cc.append(np.tile(rng.uniform(0.2, 0.9, 3), (36, 1))); M += [3 if i % 11 == 5 else 1] * 12
    v = _SPHERE_V.copy()
    r = 0.3 * (1.0 + 0.12 * step * np.sin(5.0 * v[:, 0] + 1.3 * step) * np.cos(4.0 * v[:, 1] - 0.7 * step))
    v = (SPHERE_CENTER + np.array([0.03, -0.02, 0.025]) * step + v * r[:, None]).astype(np.float32).astype(np.float64)
    tri = v[_SPHERE_F]
    P.append(tri.reshape(-1, 3)); N.append(_sphere_normals(v)[_SPHERE_F].reshape(-1, 3))
    Cc.append(np.tile([0.85, 0.45, 0.3], (3 * SPHERE_TRIS, 1))); M += [1] * SPHERE_TRIS
    pos = np.concatenate(P).astype(np.float32)
    return dict(positions=pos, normals=np.concatenate(N).astype(np.float32), colors=np.concatenate(Cc).astype(np.float32),
                indices=np.arange(pos.shape[0], dtype=np.uint32), material_ids=np.array(M, np.uint32))


def cube_first_triangle(i):
    return FLOOR_TRIS + 12 * i


def oracle_scene(O, b, textures=None):
    """The oracle's scene of a buffer dict (its own tree, built from these triangles alone)."""
    s = O.OracleScene()
    s.add_raw(b["positions"], b["normals"], b["colors"], b["material_ids"])
    if textures is not None:
        s.set_textures(*textures)
    return s


def cornell_moved(O, step, slide=0.02, turn=0.0):
    """The Cornell box's buffers with the twelve triangles of its SHORT box slid by step * slide along x and turned by step * turn about the box's own
    vertical axis.  The short box is the first cube the scene adds (include/cornellBox.h): 0.6 high, standing on the floor."""
    b = O.OracleScene.cornell_box().buffers()
    box = b["positions"][:36]
    uniq, inv = np.unique(box, axis=0, return_inverse=True)
    assert uniq.shape[0] == 8 and abs(float(uniq[:, 1].max()) - 0.6) < 1e-3 and abs(float(uniq[:, 1].min())) < 1e-3
    c = uniq.astype(np.float64).mean(0)
    R = _rot((0, 1, 0), turn * step)
    moved = ((uniq.astype(np.float64) - c) @ R.T + c + np.array([slide * step, 0, 0])).astype(np.float32)   # rounded once per corner
    b["positions"][:36] = moved[np.asarray(inv).reshape(-1)]
    b["normals"][:36] = (b["normals"][:36].astype(np.float64) @ R.T).astype(np.float32)
    return b


# ---------------------------------------------------------------------------------------------------------------------------- indexed geometry
N_VERTS_INDEXED = 4 + 8 * N_CUBES + 162 + 2
UNUSED_FAR = (1e6, -1e6, 1e6)


def _scene_a_shared(step):
    """Scene A with every vertex stored once: (positions [420, 3] float32, indices [2118]) with positions[indices] bitwise scene_a(step)'s corners --
    the floor's 4 corners, 8 per cube, the sphere's 162 -- and the per-corner buffers of scene_a(step)."""
    b = scene_a(step)
    P = b["positions"]
    order = np.concatenate([[0, 1, 2, 0, 2, 3]] + [CUBE_CORNER_ORDER] * N_CUBES + [_SPHERE_F.reshape(-1)])
    base = np.concatenate([np.zeros(6, np.int64)] + [np.full(36, 4 + 8 * i) for i in range(N_CUBES)] + [np.full(3 * SPHERE_TRIS, 4 + 8 * N_CUBES)])
    idx = (order + base).astype(np.uint32)
    pos = np.zeros((int(idx.max()) + 1, 3), np.float32)
    pos[idx] = P                                                           # (the copies of a corner are equal: any of them)
    assert pos.shape[0] == N_VERTS_INDEXED - 2 and np.array_equal(pos[idx].view(np.uint32), P.view(np.uint32))
    return pos, idx, b


def _permuted(pos, idx, b, unused):
    """The vertex buffer with `unused` appended (vertices no triangle names) and everything shuffled by a seeded permutation."""
    pos = np.concatenate([pos, np.asarray(unused, np.float32).reshape(-1, 3)])
    perm = np.random.default_rng(4242).permutation(pos.shape[0])
    out = np.empty_like(pos)
    out[perm] = pos
    return dict(b, positions=out, indices=perm[idx].astype(np.uint32))


def scene_a_indexed(step=0, unused=(UNUSED_FAR, (0.1, 0.5, 0.1))):
    """Scene A at `step` as an INDEXED mesh: 420 shared vertices and two that no triangle names (one far outside the scene), the vertex buffer
    permuted.  positions[indices] is scene_a(step)["positions"] bit for bit; normals and colours stay per corner."""
    return _permuted(*_scene_a_shared(step), unused)


def scene_a_collapsed(step=1):
    """scene_a_indexed(step) with one vertex of the sphere moved ONTO a neighbour: the two triangles on that edge have no area.  The sphere's normals
    are recomputed from the collapsed mesh (finite: every vertex keeps triangles with an area).  Returns (buffers, the degenerate triangles)."""
    pos, idx, b = _scene_a_shared(step)
    first = 4 + 8 * N_CUBES
    a, n = int(_SPHERE_F[0, 0]), int(_SPHERE_F[0, 1])
    pos[first + a] = pos[first + n]
    v = pos[first:].astype(np.float64)
    nrm = b["normals"].copy()
    nrm[3 * (FLOOR_TRIS + CUBE_TRIS):] = _sphere_normals(v)[_SPHERE_F].reshape(-1, 3).astype(np.float32)
    assert np.isfinite(nrm).all()
    flat = np.flatnonzero(((_SPHERE_F == a) | (_SPHERE_F == n)).sum(1) == 2) + FLOOR_TRIS + CUBE_TRIS
    return _permuted(pos, idx, dict(b, normals=nrm), (UNUSED_FAR, (0.1, 0.5, 0.1))), flat


def unindexed(b):
    """The same triangles with a vertex per corner and the identity for indices: what the oracle's add_raw takes."""
    pos = np.ascontiguousarray(b["positions"][b["indices"]])
    return dict(b, positions=pos, indices=np.arange(pos.shape[0], dtype=np.uint32))


FAR_SHIFT = (5000.0, -3000.0, 800.0)      # tests/test_gpu_parity.py test_intersector_far_from_the_origin


def scene_a_far(step, shift=FAR_SHIFT, cubes=True):
    """Scene A at `step` translated by `shift`, rounded once per corner (the copies of a corner are equal before and after).  cubes=False: only
    the floor and the sphere go; the cubes stay where they are."""
    b = scene_a(step)
    pos = b["positions"].astype(np.float64)
    far = np.ones(pos.shape[0], bool)
    if not cubes:
        far[3 * FLOOR_TRIS:3 * (FLOOR_TRIS + CUBE_TRIS)] = False
    pos[far] += np.asarray(shift, np.float64)
    return dict(b, positions=pos.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------- beyond one grid stride
LATTICE_FIRST_CUBE_TRI = 36                # the Cornell box's 36 triangles come first, then twelve per lattice cube
LATTICE_FAR_PUSH = (2.0, -3.0, 0.0)


def cornell_lattice_moved(O, n, step, turns=True):
    """O.OracleScene.cornell_lattice(n) with every lattice cube moved: its own translation by whole multiples of 2^-12 per axis (at most 3 of them
    per step: exactly representable, so a cube that does not cross a power of two keeps its shape to the bit), a seeded tenth of the cubes also
    turned rigidly about their own centre by 0.2 per step (turns=True), and the LAST cube pushed by LATTICE_FAR_PUSH out of the room, where it alone
    sets hi.x and lo.y of the scene.  Corners are rounded once per corner.  step 0: the scene as built."""
    b = O.OracleScene.cornell_lattice(n).buffers()
    nc = n ** 3
    assert b["material_ids"].shape[0] == LATTICE_FIRST_CUBE_TRI + 12 * nc
    if step == 0:
        return b
    P = b["positions"][3 * LATTICE_FIRST_CUBE_TRI:].reshape(nc, 36, 3)
    uniq, inv = np.unique(P[0], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    first = np.array([int(np.flatnonzero(inv == c)[0]) for c in range(uniq.shape[0])])
    corners = P[:, first].astype(np.float64)                               # [cube, 8, 3]: every cube repeats its corners in cube 0's pattern
    assert uniq.shape[0] == 8 and np.array_equal(P[:, first][:, inv], P)
    rng = np.random.default_rng(2800 + n)
    shift = rng.integers(-3, 4, (nc, 3)) * (step * 2.0 ** -12)
    shift[nc - 1] += np.array(LATTICE_FAR_PUSH)
    if turns:
        turned = np.flatnonzero(rng.random(nc) < 0.1)
        axes = rng.normal(size=(nc, 3))[turned]
        c = corners[turned].mean(1, keepdims=True)
        R = np.stack([_rot(a, 0.2 * step) for a in axes])
        corners[turned] = np.einsum("kij,kcj->kci", R, corners[turned] - c) + c
    moved = (corners + shift[:, None, :]).astype(np.float32)             # rounded once per corner
    b["positions"][3 * LATTICE_FIRST_CUBE_TRI:] = moved[:, inv].reshape(-1, 3)
    if turns:                                                               # the faces' normals turn with them
        N = b["normals"][3 * LATTICE_FIRST_CUBE_TRI:].reshape(nc, 36, 3)
        N[turned] = np.einsum("kij,kcj->kci", R, N[turned].astype(np.float64)).astype(np.float32)
    return b
