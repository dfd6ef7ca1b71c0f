"""Shared helpers for the test-suite (metrics, context construction)."""
import numpy as np


def image_metrics(img, ref):
    """Per-pixel L2 over RGB on the linear float4 buffer (SURVEY 8d 'Parity tolerance')."""
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    l2 = np.sqrt((d ** 2).sum(-1))
    refn = np.sqrt((ref[..., :3].astype(np.float64) ** 2).sum(-1))
    rmse = float(np.sqrt((d ** 2).mean()))
    frac_ok = float((l2 <= 1e-4 * np.maximum(1.0, refn)).mean())
    return rmse, frac_ok, float(l2.max())


# Tolerance for the FAST (FMA-contracted) build against the oracle, from north_star / SURVEY 8d:
# RMSE <= 1e-3 and >= 99.9 % of pixels with L2 <= 1e-4 * max(1, |ref|).
TOL_RMSE = 1e-3
TOL_FRAC = 0.999
# C4 exception ("C4 tolerance"): the replicated-mesh scene has 85,184 small cubes, i.e. ~1 M silhouette
# and crease edges where the Cornell box has ~50.  A ray that grazes an edge may resolve to the other face under FMA
# contraction (an "edge flip": a whole different path, not a rounding difference), and the share of such pixels scales
# with the edge length in the picture: measured 0.15 % at 1 spp, against 0.002 % on the Cornell box.  The RMSE bar is
# unchanged; the pixel share for C4 is 99.7 %.
TOL_FRAC_C4 = 0.997


# Edge flips per RAY (round 5; scripts/gpu_edge_flips.py, profiles/r05/edge_flips.txt).  An outlier pixel of the metric above is a path that resolved to the
# other face of an edge it passed within ~1e-7 of; how many there are is a matter of how many rays are traced and how much edge they meet, not of
# how many pixels the picture has.  Measured on the shipped build in the fuzz's regime (images up to 90 x 70, 1 - 40 spp, 1 - 6 bounces): 0.4 outlier
# pixels per MILLION rays on the bare Cornell box, 1 - 1.5 with 100 - 2,000 extra triangles, 2.7 - 3.1 with 4,000 - 9,000; worst single image 13.
# (The cube lattice of C4 -- a million silhouette edges a few pixels long -- is another regime: TOL_FRAC_C4.)  A random soup's picture may therefore
# hold 0.1 % of its pixels PLUS what a Poisson count with mean q x rays, q = 1e-5 (three times the largest measured rate), reaches
# with probability 1 - 1e-7: for a 60 x 50 image at 20 spp and 5 bounces (0.5 M rays) that is 3 + 20 pixels, for the 2-megapixel C2 frame it would be
# 0.1 % + 0.06 % -- the full-size tests do not use it, they keep the flat 99.9 %.
EDGE_FLIPS_PER_RAY = 1e-5


def edge_flip_allowance(pixels, rays, q=EDGE_FLIPS_PER_RAY):
    """Outlier pixels a random-soup picture of `pixels` pixels rendered with `rays` rays may hold (see above)."""
    from scipy.stats import poisson
    return int(0.001 * pixels) + int(poisson.ppf(1.0 - 1e-7, q * max(float(rays), 1.0)))


def make_ctx(O, scene, w, h, offsets=None, uniforms=None):
    from toyraygun_amd import capi
    c = capi.Context(w, h)
    b = scene.buffers()
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.set_uniforms(O.uniforms_bytes(uniforms if uniforms is not None else O.make_uniforms(w, h)))
    if offsets is None:
        c.set_pixel_offsets_seed()
    else:
        c.set_pixel_offsets(offsets)
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Cameras and lights other than the default block (tests/test_uniforms_host.py, tests/test_gpu_uniforms.py).  The default block is nearly blind
# to a permuted light colour (white), to light_right and light_up swapped (equal lengths, nine of twelve components zero) and to a wrong
# cam_pos.x (zero); these cases are not.  name -> (eye, at).
CAMERAS = {
    "default":      ((0.0, 1.0, 3.38), (0.0, 1.0, -1.0)),             # control
    "outside_back": ((0.0, 1.0, -6.0), (0.0, 1.0, 0.0)),              # outside the room: hits and misses in one wave
    "from_above":   ((0.0, 5.0, 0.3), (0.0, 0.0, 0.0)),               # through the back of the ceiling, the view almost along the look-at's up vector
    "inside_low":   ((0.7, 0.15, 1.5), (-0.5, 1.6, -0.5)),            # every component non-zero, grazing the floor
    "nearly_up":    ((0.0, 0.5, 0.5), (0.02, 2.0, 0.47)),             # one degree off the degenerate look-at
    "in_tall_box":  ((-0.335, 0.6, -0.29), (0.5, 0.3, 1.0)),          # origin inside a box leaf: every primary hit is a back face of that cube
    "away":         ((0.0, 1.0, 3.38), (0.0, 1.0, 8.0)),              # no ray hits anything: a black frame and not one secondary ray
}
# The exactly degenerate camera (`at` straight above `eye`) is NOT here and must not be added: its inverse view-projection is NaN and so is every
# ray; tests/test_uniforms_host.py asserts finite rays for every entry.

# name -> None (the block's own light) or (pos, forward, right, up, color)
LIGHTS = {
    "default":         None,
    "tilted_coloured": ((0.4, 1.6, 0.3), (-0.48, -0.8, -0.36), (0.3, 0.0, -0.4), (0.1, 0.05, 0.02), (5.0, 0.5, 2.0)),    # no two components alike
    "floor_up":        ((0.0, 0.0005, 0.5), (0.0, 1.0, 0.0), (0.6, 0.0, 0.0), (0.0, 0.0, 0.6), (0.2, 1.0, 0.4)),        # half a millimetre above the floor
    "sideways":        ((0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0), (1.0, 1.0, 1.0)),         # radiance ~67 near it; half the room dark
    "point_dim":       ((0.3, 1.2, 0.8), (0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.03, 1.5)),          # zero extent, one channel exactly zero
}
LIGHT_FIELDS = ("light_pos", "light_forward", "light_right", "light_up", "light_color")
UNIFORM_SHAPES = ((72, 40), (33, 17))      # 9 x 5 whole 8x8 tiles; partial tiles both ways
FAST_RUNS = {(72, 40): (8, 5), (33, 17): (3, 15)}      # shape -> (spp, bounces) of the shipped build's runs against the libm oracle


def uniforms_case(O, w, h, cam, light, frame=0):
    """The oracle's uniform block for CAMERAS[cam] with the first three floats of every light field overwritten by LIGHTS[light]."""
    eye, at = CAMERAS[cam]
    u = O.make_uniforms(w, h, frame, eye, at)
    if LIGHTS[light] is not None:
        for name, v in zip(LIGHT_FIELDS, LIGHTS[light]):
            getattr(u, name)[0:3] = [float(np.float32(x)) for x in v]
    return u


def fast_bar(img, ref, rays):
    """The shipped build's bar on a small image: (passes, rmse, outlier pixels, outlier pixels allowed) -- RMSE <= TOL_RMSE and no more pixels
    beyond 1e-4 * max(1, |ref|) than edge_flip_allowance gives `rays` rays."""
    pixels = ref.shape[0] * ref.shape[1]
    rmse, frac_ok, _ = image_metrics(img, ref)
    allowed = edge_flip_allowance(pixels, rays)
    return bool(rmse <= TOL_RMSE and frac_ok >= 1.0 - allowed / pixels), rmse, int(round((1.0 - frac_ok) * pixels)), allowed


def uniform_pairs():
    """All 7 x 5 (camera, light) names."""
    return [(c, l) for c in CAMERAS for l in LIGHTS]


# every camera and every light at least once (7 pairs)
REDUCED_PAIRS = (("default", "tilted_coloured"), ("outside_back", "floor_up"), ("from_above", "sideways"), ("inside_low", "point_dim"),
                 ("nearly_up", "default"), ("in_tall_box", "tilted_coloured"), ("away", "sideways"))


def box_zoo(O):
    """A scene that fits in LDS and exercises the BOX leaves (bvh_build.h kLeafBox): the Cornell box (two cubes standing on the floor) plus cubes that
    are rotated, sheared (a parallelepiped), mirrored (negative scale: the vertex order flips), nested in another, emissive (material 2: seen by
    primary rays only) and of material 3 -- seven parallelepipeds -- and one ALMOST-cube with a corner moved by 1e-3, which must stay six quads'
    worth of triangles.  Returns (scene, number of boxes the builder must find)."""
    unit = O.OracleScene()
    unit.add("cube", (1.0, 1.0, 1.0), np.eye(4, dtype=np.float32))
    verts = unit.buffers()["positions"].reshape(-1, 3).copy()          # addCube's 36 vertices in its own order (Scene.cpp:24-58)
    idx = np.arange(36, dtype=np.uint32)

    def mtx(scale, rot_y, pos, shear=0.0):
        c, s_ = np.cos(rot_y), np.sin(rot_y)
        r = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], np.float64)
        sh = np.eye(3); sh[0, 1] = shear                                  # x += shear * y
        m = np.eye(4)
        m[:3, :3] = r @ sh @ np.diag(scale)
        m[:3, 3] = pos
        return m.T.astype(np.float32)                                     # row-vector convention of bx (mtx[12..14] = translation)

    s = O.OracleScene.cornell_box()
    s.add_geometry(verts, idx, mtx((0.12, 0.12, 0.12), 0.7, (-0.6, 1.5, 0.5)), (0.3, 0.8, 0.4), 1)                 # rotated, floating
    s.add_geometry(verts, idx, mtx((0.15, 0.1, 0.08), -0.3, (0.55, 1.3, -0.4), shear=0.6), (0.8, 0.5, 0.2), 1)      # sheared
    s.add_geometry(verts, idx, mtx((-0.1, 0.14, 0.1), 1.1, (0.1, 1.6, 0.6)), (0.2, 0.4, 0.9), 1)                    # mirrored
    s.add_geometry(verts, idx, mtx((0.05, 0.05, 0.05), 0.2, (-0.6, 1.5, 0.5)), (0.9, 0.9, 0.1), 1)                  # inside the first
    s.add_geometry(verts, idx, mtx((0.08, 0.04, 0.08), 0.0, (-0.2, 1.85, 0.2)), (1.0, 1.0, 1.0), 2)                 # emissive
    s.add_geometry(verts, idx, mtx((0.1, 0.1, 0.1), 0.5, (0.6, 0.1, 0.9)), (0.6, 0.6, 0.6), 3)                      # material 3, on the floor
    almost = verts.copy()
    corner = almost[0].copy()
    almost[(almost == corner).all(1)] += np.float32(1e-2)                 # one corner of the unit cube off by 1e-2 (1e-3 once scaled)
    s.add_geometry(almost, idx, mtx((0.1, 0.1, 0.1), 0.9, (-0.1, 0.9, 1.2)), (0.5, 0.2, 0.7), 1)
    return s, 2 + 6


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Directed rays PARALLEL to faces (tests/test_gpu_parallel_rays.py).  The random ray sets of the suite draw directions from a normal distribution
# or aim at a point, so no component of a direction -- in the world's frame or in a box's own -- is ever exactly zero; these generators plant
# exact zeros, -0.0, +-1e-30, +-1e-38 and a denormal (+-1e-42) there, for every box leaf, lone quad and lone triangle of a scene.
RAY_KINDS = ("axis_outside", "axis_inside", "frame_axis", "frame_pair", "slab_edge", "tiny", "plane_in", "plane_off")
# what the zero of an axis-parallel direction is written as in the "tiny" rays
TINY_ZEROS = (-0.0, 1e-30, -1e-30, 1e-38, -1e-38, 1e-42, -1e-42)


def box_frames(boxes):
    """(centre[3], A[3,3], H[3,3]) per row of trg_debug_boxes, in float64: l = A (P - centre), inside <=> |l_k| <= 1; the columns of H = inv(A) are
    the box's half axes."""
    out = []
    for row in np.asarray(boxes):
        c, A = row[2:5].astype(np.float64), row[5:14].reshape(3, 3).astype(np.float64)
        out.append((c, A, np.linalg.inv(A)))
    return out


def box_triangles(positions, frames, tol=1e-4):
    """box[t] = the frame whose corners are the three vertices of triangle t (|l_k| = 1 on every axis), or -1: the triangle is not part of a box."""
    T = np.asarray(positions, np.float64).reshape(-1, 3, 3)
    box = np.full(T.shape[0], -1, np.int32)
    for i, (c, A, _) in enumerate(frames):
        l = np.abs((T - c) @ A.T)
        box[(np.abs(l - 1.0) < tol).all((1, 2)) & (box < 0)] = i
    return box


def _slabs(lo, ld):
    """The forward ray lo + t ld, t >= 0, against the solid |l_k| <= 1, float64, one row per ray.  A direction component that is exactly zero is
    PARALLEL: outside that slab a miss, inside no constraint."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-1.0 - lo) / ld, (1.0 - lo) / ld
    par = ld == 0.0
    near = np.where(par, np.where(np.abs(lo) <= 1.0, -np.inf, np.inf), np.minimum(t1, t2))
    far = np.where(par, np.inf, np.maximum(t1, t2))
    return np.maximum(near.max(1), 0.0) <= far.min(1)


def ray_box_f64(frames, which, rays):
    """Float64 geometry of ray r against box which[r] (-1: none), on the forward ray [0, inf): (passes the box's AABB, meets the box)."""
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)

    in_aabb, in_box = np.zeros(len(rays), bool), np.zeros(len(rays), bool)
    for i, (c, A, H) in enumerate(frames):
        m = which == i
        if not m.any():
            continue
        half = np.abs(H).sum(1)                                           # half extent of the AABB of c + H [-1, 1]^3
        in_aabb[m] = _slabs((o[m] - c) / half, d[m] / half)
        in_box[m] = _slabs((o[m] - c) @ A.T, d[m] @ A.T)
    return in_aabb, in_box


def _finish_rays(O, rng, org, dirn, kind, which):
    n = len(org)
    rays = np.zeros(n, O.RAY_DTYPE)
    rays["origin"], rays["direction"] = np.asarray(org, np.float32), np.asarray(dirn, np.float32)
    rays["mask"] = rng.choice([1, 2, 3], n, p=[0.2, 0.1, 0.7]).astype(np.uint32)
    rays["maxDistance"] = np.where(rng.random(n) < 0.25, rng.uniform(0.05, 2.0, n), np.inf).astype(np.float32)
    rays["maxDistance"][rng.random(n) < 0.01] = -1.0
    return rays, np.asarray(kind, np.int8), np.asarray(which, np.int32)


def parallel_box_rays(O, frames, seed, per_box=1.0, only=None):
    """Rays parallel to the faces of every box of `frames` (or of the boxes `only`).  Returns (rays, kind, which): kind indexes RAY_KINDS, which
    names the box a ray was built for.  About 1,300 x per_box rays per box:
      axis_outside / axis_inside   +-x, +-y, +-z, origins uniform over 1.3 x the footprint of the box's AABB, starting just outside the AABB along
                                   the ray / somewhere inside the AABB along the ray (inside the box or not);
      frame_axis / frame_pair      direction = one half axis of the box / a combination of two, rounded to fp32: two / one of the direction's
                                   components in the box's frame are zero or a few ulps from it; origins inside and outside each slab;
      slab_edge                    the same with |l_k| = 1 +- a few ulps on a parallel axis (mostly undecidable: kept few);
      tiny                         axis-parallel directions whose zeros are written as one of TINY_ZEROS."""
    rng = np.random.default_rng(seed)
    org, dirn, kind, which = [], [], [], []

    def emit(o, d, k, i):
        o, d = np.atleast_2d(o), np.atleast_2d(d)
        d = np.broadcast_to(d, o.shape)
        org.append(o); dirn.append(d); kind.append(np.full(len(o), RAY_KINDS.index(k))); which.append(np.full(len(o), i))

    n_ax, n_fr, n_tiny, n_edge = (max(lo, int(round(v * per_box))) for v, lo in ((40, 2), (30, 2), (12, 2), (2, 1)))
    ulps = np.array([-4, -1, 0, 1, 4]) * 2.0 ** -23
    for i, (c, A, H) in enumerate(frames):
        if only is not None and i not in only:
            continue
        half = np.abs(H).sum(1)
        for ax in range(3):
            for sgn in (1.0, -1.0):
                d = np.zeros(3); d[ax] = sgn
                def foot(n):
                    # half of the origins uniform over 1.3 x the footprint; the other half -- where the box leaves room for it -- uniform over the
                    # part of the AABB's footprint from which this direction passes the box by
                    o = c + rng.uniform(-1.3, 1.3, (n, 3)) * half
                    cand = c + rng.uniform(-1.0, 1.0, (8 * n, 3)) * half
                    cand[:, ax] = c[ax] - sgn * half[ax] * 1.5
                    cand = cand[~_slabs((cand - c) @ A.T, np.broadcast_to(A @ d, (8 * n, 3)))][: n // 2]
                    o[: len(cand)] = cand
                    return o
                o = foot(n_ax); o[:, ax] = c[ax] - sgn * half[ax] * rng.uniform(1.02, 1.5, n_ax)
                emit(o, d, "axis_outside", i)
                o = foot(n_ax); o[:, ax] = c[ax] + half[ax] * rng.uniform(-1.0, 1.0, n_ax)
                emit(o, d, "axis_inside", i)
                for z in TINY_ZEROS:
                    dz = np.full(3, z); dz[ax] = sgn
                    if rng.random() < 0.5:
                        dz[(ax + 1) % 3] = 0.0                             # (one tiny component beside an exact zero)
                    o = foot(n_tiny); o[:, ax] = c[ax] - sgn * half[ax] * (rng.uniform(1.02, 1.5, n_tiny) if z > 0 else rng.uniform(-1.0, 1.0, n_tiny))
                    emit(o, dz, "tiny", i)
        # in the box's own frame: l = the origin there, the direction a half axis (or two) of the box
        for axes, k, n in [((j,), "frame_axis", n_fr) for j in range(3)] + [((j, (j + 1) % 3), "frame_pair", n_fr) for j in range(3)]:
            par = [a for a in range(3) if a not in axes]
            for sgn in (1.0, -1.0):
                w = np.zeros(3); w[list(axes)] = sgn * (1.0 if len(axes) == 1 else rng.uniform(0.3, 1.0, 2) * rng.choice([-1.0, 1.0], 2))
                d = H @ w
                d = (d / np.linalg.norm(d)).astype(np.float32)
                l = rng.uniform(-1.45, 1.45, (n, 3))
                l[: n // 2, axes[0]] = -np.sign(w[axes[0]]) * rng.uniform(1.05, 1.6, n // 2)     # half of them start outside, on the side the ray comes from
                emit(c + l @ H.T, d, k, i)
                l = rng.uniform(-0.9, 0.9, (n_edge * len(par), 3))
                l[:, axes[0]] = -np.sign(w[axes[0]]) * 1.3
                for q, a in enumerate(par):
                    l[q * n_edge:(q + 1) * n_edge, a] = rng.choice([-1.0, 1.0], n_edge) * (1.0 + rng.choice(ulps, n_edge))
                emit(c + l @ H.T, d, "slab_edge", i)
    return _finish_rays(O, rng, np.concatenate(org), np.concatenate(dirn), np.concatenate(kind), np.concatenate(which))


def parallel_plane_rays(O, positions, tris, extent, seed, per_tri=1.0):
    """Rays parallel to the supporting plane of every triangle of `tris` (indices into the flat positions): along both edges from vertex 0 and
    along their sum -- of a parallelogram's first triangle that is the quad's diagonal --, starting inside and outside the footprint,
      plane_in    exactly IN the plane: only where fp32 can say so (the float64 normal, the direction and the origin's offset are exact, i.e. the
                  primitive is axis-aligned); of an oblique plane the fp32 ray nearest to "in the plane" is decided by its own rounding;
      plane_off   at 1e-6 ... 1e-2 of `extent` off the plane, either side: inside the child box an 8-bit quantised node gives a flat primitive.
    Returns (rays, kind, which) with which = the triangle."""
    rng = np.random.default_rng(seed)
    T = np.asarray(positions, np.float64).reshape(-1, 3, 3)
    org, dirn, kind, which = [], [], [], []
    n = max(2, int(round(6 * per_tri)))
    for t in tris:
        v0, e1, e2 = T[t, 0], T[t, 1] - T[t, 0], T[t, 2] - T[t, 0]
        nrm = np.cross(e1, e2)
        if not np.linalg.norm(nrm) > 0:
            continue
        nrm /= np.linalg.norm(nrm)
        for e in (e1, e2, e1 + e2, -e1, -e2):
            d = (e / np.linalg.norm(e)).astype(np.float32)
            exact = float(np.dot(nrm, d.astype(np.float64))) == 0.0 and np.count_nonzero(nrm) == 1
            for off in (0.0, 1e-6, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3, 1e-2, -1e-2):
                if off == 0.0 and not exact:
                    continue
                uv = rng.uniform(0.05, 0.95, (n, 2))
                start = rng.uniform(-0.6, 0.4, n)                           # along the ray, in units of |e|: before the footprint, or inside it
                o = v0 + uv[:, :1] * e1 + uv[:, 1:] * e2 + nrm * (off * extent)
                along = d.astype(np.float64) * np.linalg.norm(e)
                far = np.where(rng.random(n) < 0.5, 1.2, 0.0)               # half of them start clear of the footprint, the others wherever `start` says
                o = o + along * np.where(far > 0, -far, start)[:, None]
                o32 = o.astype(np.float32)
                if off == 0.0:                                               # keep the origin's plane coordinate exactly the vertices'
                    a = int(np.flatnonzero(nrm)[0])
                    o32[:, a] = np.float32(T[t, 0, a])
                org.append(o32); dirn.append(np.broadcast_to(d, o32.shape))
                kind.append(np.full(n, RAY_KINDS.index("plane_in" if off == 0.0 else "plane_off"))); which.append(np.full(n, t))
    return _finish_rays(O, rng, np.concatenate(org), np.concatenate(dirn), np.concatenate(kind), np.concatenate(which))
