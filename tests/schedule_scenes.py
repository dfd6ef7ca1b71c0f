"""Scenes of the schedule tests (tests/test_schedule_scenes_host.py, tests/test_gpu_schedule_scenes.py): triangles whose three corners carry
three different normals, colours and texture coordinates, small enough for every render schedule to run on them in a test.

Scene A, 102 triangles, LDS-resident: the Cornell box (36), the 8 x 5 UV sphere with per-vertex normals and per-vertex colours whose texture
coordinates wrap three times and go negative (64; texture 1, a 64 x 64 checker), and a floor quad with uv 0..2 (2; texture 2, a 37 x 37 checker).
Scene B: the same with the 40 x 24 sphere (1,840 triangles): HBM-resident by itself.
Variants: "base"; "flat" (every mesh triangle's corners get corner 0's normal and colour: what a kernel that ignores the weights would draw);
"rotated" (the mesh corners' normals, colours and uv moved on by one corner, the positions left alone: what a kernel that permutes the weights
would draw).

The edge family of the LDS tier: the Cornell box plus the first k of one seeded list of random triangles in the room, every corner with its own
normal and colour, every third triangle textured (5 x 3 texels).

Oracle references are rendered once per (scene, variant, textured, shape, trig mode) and handed out read-only."""
import functools

import numpy as np

N_BOX = 36                                             # the Cornell box's triangles come first
SHAPES = ((48, 40, 5, 5), (33, 17, 18, 5))            # (w, h, spp, bounces): partial 16 x 16 tiles; the second crosses the 16-frame tail chunk
SPHERES = {"A": (8, 5), "B": (40, 24)}
SPHERE_AT = (0.33, (0.25, 1.1, 0.15))
VARIANTS = ("base", "flat", "rotated")


def uv_sphere(nu, nv, radius, centre):
    """Indexed UV sphere: vertices, unit normals, per-vertex colours (a smooth function of the normal), triangles."""
    th = np.linspace(0.0, np.pi, nv + 1)
    ph = np.linspace(0.0, 2 * np.pi, nu, endpoint=False)
    n = np.array([[np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)] for t in th for p in ph])
    v = n * radius + np.asarray(centre)
    col = 0.15 + 0.7 * (0.5 + 0.5 * n[:, [0, 1, 2]]) * np.array([1.0, 0.8, 0.6])
    tris = []
    for a in range(nv):
        for b in range(nu):
            i0, i1 = a * nu + b, a * nu + (b + 1) % nu
            j0, j1 = i0 + nu, i1 + nu
            if a > 0:
                tris.append((i0, i1, j0))      # at the poles one of the two triangles is degenerate: skip it
            if a < nv - 1:
                tris.append((i1, j1, j0))
    return v.astype(np.float32), n.astype(np.float32), col.astype(np.float32), np.array(tris, np.uint32)


def checker_texture(n, cells, a, b, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    chk = ((xx * cells // n) + (yy * cells // n)) % 2
    img = np.where(chk[..., None] == 0, np.array(a, np.uint8), np.array(b, np.uint8)).astype(np.uint8)
    img = np.clip(img.astype(int) + rng.integers(-20, 21, img.shape), 0, 255).astype(np.uint8)   # every texel distinct-ish
    return np.concatenate([img, np.full((n, n, 1), 255, np.uint8)], -1)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False


def _rotate_corners(a):
    """[3 n, k] per-corner rows: corner j of every triangle gets what corner j + 1 had."""
    return a.reshape(-1, 3, a.shape[-1])[:, [1, 2, 0]].reshape(a.shape)


@functools.lru_cache(maxsize=None)
def scene(name, variant="base"):
    """(buffers dict as trg_load_scene takes them, uvs [3 n, 2], texture ids [n], images) of scene A or B; built by the product's host library
    (Scene::addMesh with texture coordinates), the sphere's colours then set per vertex."""
    from toyraygun_amd import host
    assert variant in VARIANTS
    nu, nv = SPHERES[name]
    v, n, col, tris = uv_sphere(nu, nv, *SPHERE_AT)
    th = np.linspace(0.0, 1.0, nv + 1)
    ph = np.linspace(0.0, 3.0, nu, endpoint=False)           # u runs 0..3: wraps
    uv = np.array([[p, 1.0 - t * 2.0] for t in th for p in ph], np.float32)   # v runs 1..-1: negative coordinates too
    t1 = host.Texture(rgba=checker_texture(64, 8, (230, 60, 40), (40, 90, 220), 1))
    t2 = host.Texture(rgba=checker_texture(37, 5, (250, 250, 250), (30, 30, 30), 2))   # non-power-of-two
    hs = host.Scene.cornell_box()
    hs.add_textured_mesh(v, n, uv, tris, np.eye(4, dtype=np.float32), (0.9, 0.9, 0.9), 1, t1)
    qv = np.array([[-0.9, 0.02, -0.2], [-0.2, 0.02, -0.2], [-0.2, 0.02, 0.9], [-0.9, 0.02, 0.9]], np.float32)
    qn = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
    quv = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.float32)
    hs.add_textured_mesh(qv, qn, quv, [0, 2, 1, 0, 3, 2], np.eye(4, dtype=np.float32), (0.8, 0.8, 0.8), 1, t2)
    b = hs.buffers()
    uvs, ids, imgs = hs.texture_buffers()
    nt, ns = b["material_ids"].shape[0], tris.shape[0]
    assert nt == N_BOX + ns + 2 and len(imgs) == 2
    assert (ids[:N_BOX] == 0).all() and (ids[N_BOX:N_BOX + ns] == 1).all() and (ids[-2:] == 2).all()
    b["colors"][3 * N_BOX:3 * (N_BOX + ns)] = col[tris.reshape(-1)]        # per-vertex colours UNDER the texture
    m = slice(3 * N_BOX, None)                                              # the mesh corners
    if variant == "flat":
        for k in ("normals", "colors"):
            b[k][m] = np.repeat(b[k][m].reshape(-1, 3, 3)[:, 0], 3, axis=0)
    elif variant == "rotated":
        for k in ("normals", "colors"):
            b[k][m] = _rotate_corners(b[k][m])
        uvs[m] = _rotate_corners(uvs[m])
    _frozen(uvs, ids, *imgs, *b.values())
    return b, uvs, ids, tuple(imgs)


def oracle_scene(O, buffers, textures=None):
    s = O.OracleScene()
    s.add_raw(buffers["positions"], buffers["normals"], buffers["colors"], buffers["material_ids"])
    if textures is not None:
        s.set_textures(*textures)
    return s


def _render(O, s, w, h, spp, bnc, trig):
    """(image, (primary, bounce, shadow rays, shaded hits), ray total), the image read-only."""
    O.set_trig_mode(getattr(O, trig))
    try:
        img, st = O.render(s, w, h, spp, bnc, offsets=O.pixel_offsets(w, h))
    finally:
        O.set_trig_mode(O.TRIG_LIBM)
    _frozen(img)
    return img, (int(st.primary_rays), int(st.bounce_rays), int(st.shadow_rays), int(st.shaded_hits)), int(st.rays)


@functools.lru_cache(maxsize=None)
def reference(name, variant, textured, shape, trig):
    """The oracle's render of scene `name` at SHAPES[shape]; trig = "TRIG_PORTABLE" (the strict build's bits) or "TRIG_LIBM" (the shipped
    build's yardstick)."""
    from oracle import pyoracle as O
    b, uvs, ids, imgs = scene(name, variant)
    return _render(O, oracle_scene(O, b, (uvs, ids, list(imgs)) if textured else None), *SHAPES[shape], trig)


def room_pixels(O, s, w, h):
    """[h, w] bool: the pixels whose frame-0 primary ray hits the Cornell box itself -- they see the meshes through bounces >= 1 only."""
    prim = O.intersect_nearest(s, O.raygen(w, h, 0, offsets=O.pixel_offsets(w, h)))["primitiveIndex"]
    return ((prim >= 0) & (prim < N_BOX)).reshape(h, w)


def differ(a, b, eps=1e-3):
    """[h, w] bool: pixels whose RGB differ by more than eps."""
    return np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)).max(-1) > eps


# ---------------------------------------------------------------------------------------------------------------------------- the LDS tier's edge
EDGE_N = range(120, 221)
EDGE_SHAPE = (32, 24, 2, 4)
EDGE_TEXTURE = np.random.default_rng(77).integers(0, 256, (3, 5, 4)).astype(np.uint8)        # 5 wide, 3 high


@functools.lru_cache(maxsize=None)
def _edge_pool():
    """max(EDGE_N) - 36 random triangles in the room: positions, per-corner normals and colours (all distinct), uv in [-1, 2)."""
    rng = np.random.default_rng(20261)
    k = max(EDGE_N) - N_BOX
    c = rng.uniform((-0.85, 0.15, -0.85), (0.85, 1.8, 0.85), (k, 1, 3))
    pos = (c + rng.uniform(-0.3, 0.3, (k, 3, 3))).astype(np.float32).reshape(-1, 3)
    nrm = rng.normal(size=(3 * k, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    col = rng.uniform(0.1, 0.95, (3 * k, 3)).astype(np.float32)
    uv = rng.uniform(-1.0, 2.0, (3 * k, 2)).astype(np.float32)
    return pos, nrm, col, uv


@functools.lru_cache(maxsize=None)
def edge_scene(n):
    """(buffers, uvs, ids, images) of the n-triangle member of the edge family."""
    from oracle import pyoracle as O
    b = O.OracleScene.cornell_box().buffers()
    k = n - N_BOX
    pos, nrm, col, uv = (a[:3 * k] for a in _edge_pool())
    out = dict(positions=np.concatenate([b["positions"][b["indices"]], pos]), normals=np.concatenate([b["normals"], nrm]),
               colors=np.concatenate([b["colors"], col]), indices=np.arange(3 * n, dtype=np.uint32),
               material_ids=np.concatenate([b["material_ids"], np.ones(k, np.uint32)]))
    uvs = np.concatenate([np.zeros((3 * N_BOX, 2), np.float32), uv])
    ids = np.zeros(n, np.uint32)
    ids[N_BOX::3] = 1
    _frozen(uvs, ids, *out.values())
    return out, uvs, ids, (EDGE_TEXTURE,)


@functools.lru_cache(maxsize=None)
def edge_reference(n, trig):
    from oracle import pyoracle as O
    b, uvs, ids, imgs = edge_scene(n)
    return _render(O, oracle_scene(O, b, (uvs, ids, list(imgs))), *EDGE_SHAPE, trig)


# ---------------------------------------------------------------------------------------------------------------------------- a deep tree
DEEP_FAN = (113, 0.7)                  # triangles of the fan, their shrink ratio
LDS_LIMIT, LDS_STACK_LEVEL_BYTES = 65536, 1024


def deep_scene(k=DEEP_FAN[0], ratio=DEEP_FAN[1], seed=5):
    """A floor, a back wall and a fan of k triangles, triangle i of size ratio^i at distance 1.6 ratio^i from the origin (so that fp32 keeps
    them apart): the host builder's binned SAH peels the large ones off a few at a time, and its tree gets about as deep as its depth cap
    lets it -- deep enough that the LDS traversal stacks no longer fit next to the staged scene.  Every corner has its own normal and colour.
    Buffers as trg_load_scene takes them; k + 4 triangles."""
    rng = np.random.default_rng(seed)
    s = ratio ** np.arange(k, dtype=np.float64)
    d = rng.normal(size=(k, 3))
    d = np.abs(d / np.linalg.norm(d, axis=1, keepdims=True))
    c = 1.6 * s[:, None] * d
    fan = c[:, None, :] + 0.35 * s[:, None, None] * rng.uniform(-1.0, 1.0, (k, 3, 3))
    fl = np.array([[-2.0, -0.3, -1.0], [2.0, -0.3, -1.0], [2.0, -0.3, 3.0], [-2.0, -0.3, 3.0]])
    wl = np.array([[-2.0, -0.3, -1.0], [2.0, -0.3, -1.0], [2.0, 2.5, -1.0], [-2.0, 2.5, -1.0]])
    pos = np.concatenate([fl[[0, 2, 1, 0, 3, 2]], wl[[0, 1, 2, 0, 2, 3]], fan.reshape(-1, 3)]).astype(np.float32)
    n = k + 4
    nrm = rng.normal(size=(3 * n, 3))
    nrm[:6], nrm[6:12] = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    col = rng.uniform(0.1, 0.95, (3 * n, 3)).astype(np.float32)
    return dict(positions=pos, normals=nrm, colors=col, indices=np.arange(3 * n, dtype=np.uint32), material_ids=np.ones(n, np.uint32))


def aimed_rays(O, buffers, tris, n, seed):
    """n rays from random points of the room towards random points of the triangles `tris` (each equally often, whatever its size), going on
    behind them: mask 3, no distance limit."""
    rng = np.random.default_rng(seed)
    T = buffers["positions"][buffers["indices"]].reshape(-1, 3, 3).astype(np.float64)[np.asarray(tris)]
    t = rng.integers(0, T.shape[0], n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    target = (T[t] * w[:, :, None]).sum(1)
    org = rng.uniform((-0.5, 0.0, -0.5), (1.6, 1.6, 2.5), (n, 3))
    d = target - org
    rays = np.zeros(n, O.RAY_DTYPE)
    rays["origin"], rays["direction"] = org.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["mask"], rays["maxDistance"] = 3, np.inf
    return rays


def random_textures(n_tris, first=0, seed=9):
    """(uvs, ids, images) that put EDGE_TEXTURE on every third triangle from `first` on, uv in [-1, 2)."""
    uvs = np.random.default_rng(seed).uniform(-1.0, 2.0, (3 * n_tris, 2)).astype(np.float32)
    ids = np.zeros(n_tris, np.uint32)
    ids[first::3] = 1
    return uvs, ids, (EDGE_TEXTURE,)


@functools.lru_cache(maxsize=None)
def deep_reference(trig):
    from oracle import pyoracle as O
    b = deep_scene()
    uvs, ids, imgs = random_textures(b["material_ids"].shape[0], 4)
    return _render(O, oracle_scene(O, b, (uvs, ids, list(imgs))), *EDGE_SHAPE, trig)


def staged_bytes(n_nodes, n_records, n_tris):
    """What a workgroup stages of an LDS-resident scene: 208-byte nodes, 48-byte records + a u16 each, 76 bytes of attributes per triangle,
    80 bytes of header and the Halton tables (trg_capi.cpp, small_bytes)."""
    return n_nodes * 208 + n_records * 50 + n_tris * 76 + 80 + 2192
