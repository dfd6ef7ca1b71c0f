"""Rays PARALLEL to the faces of box leaves, lone quads and lone triangles (-m gpu), per ray, against float64 geometry.

Every other ray set of the suite draws its directions from a normal distribution or aims at a point, so no component of a direction -- in the
world's frame or in a box's own -- is ever exactly zero, and the twelve axis rays of test_gpu_parity._adversarial_rays start where the node test
culls both cubes.  trg_trace is public API, and axis-parallel rays are the first thing a caller sends (picking, orthographic probes, height
queries).  The battery (tests/util.py parallel_box_rays, parallel_plane_rays) plants exact zeros, -0.0, +-1e-30, +-1e-38 and a denormal in the
directions, in the world's frame and in each box's, with origins inside and outside every slab.

The bars are the ones of test_gpu_parity.test_box_leaves:
  * strict build: records byte-identical to the oracle's brute-force loop, any-hit answers identical;
  * shipped build: the primitive may differ from the oracle's only where O.nearest_f64 gives a margin below 1e-5; elsewhere the distance to 3e-6,
    the hit point to 1e-5, the weights to max(2e-5, 1e-5 / edge); any-hit: EVERY ray whose margin is >= 1e-5 agrees (a battery of a few thousand
    rays: the 2e-3 share the random sets allow would hide a whole class of them).
Nothing here reads anything outside the repository; the battery is generated from the scene and a seed.
"""
import functools
import time

import numpy as np
import pytest

from tests.util import RAY_KINDS, box_frames, box_triangles, box_zoo, parallel_box_rays, parallel_plane_rays, ray_box_f64

pytestmark = pytest.mark.gpu

MARGIN = 1e-5          # the SET bar of test_intersector / test_box_leaves: below it double precision says fp32 cannot decide
EXACT_ZERO_KINDS = tuple(RAY_KINDS.index(k) for k in ("axis_outside", "axis_inside", "plane_in"))   # rays whose zeros are written as +0.0


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def _soup(O):
    """Lone triangles and quads, axis-aligned (a ray along an edge has den == 0 exactly, an origin in the plane q == 0) and oblique, of three
    materials, far enough apart that none hides another entirely."""
    rng = np.random.default_rng(77)
    s = O.OracleScene()
    eye = np.eye(4, dtype=np.float32)

    def quad(a, e1, e2, pattern, mat=1):
        a, e1, e2 = (np.asarray(v, np.float32) for v in (a, e1, e2))
        p4 = np.stack([a, a + e1, a + e1 + e2, a + e2]).astype(np.float32)
        s.add_geometry(p4, [0, 1, 2, 0, 2, 3] if pattern == 1 else [0, 2, 3, 0, 1, 2], eye, rng.uniform(0.2, 0.9, 3), mat)

    def tri(a, e1, e2, mat=1):
        a, e1, e2 = (np.asarray(v, np.float32) for v in (a, e1, e2))
        s.add_geometry(np.stack([a, a + e1, a + e2]).astype(np.float32), [0, 1, 2], eye, rng.uniform(0.2, 0.9, 3), mat)

    quad((-0.75, 0.25, -0.5), (1.5, 0, 0), (0, 0, 1.0), 1)              # y = 0.25, a floor
    quad((-0.5, 0.5, 0.625), (0, 1.0, 0), (1.0, 0, 0), 2)               # z = 0.625, a back wall
    quad((0.875, 0.375, -0.5), (0, 0, 0.75), (0, 1.25, 0), 1, mat=3)    # x = 0.875
    quad((-1.0, 0.0, -1.0), (0, 2.0, 0), (0, 0, 2.0), 2)                # x = -1, a large wall
    quad((-1.0, 0.0, 1.0), (2.0, 0, 0), (0, 2.0, 0), 1)                 # z = 1, another
    tri((-0.25, 1.75, -0.25), (0.75, 0, 0), (0, 0, 0.5))                # y = 1.75
    tri((-0.875, 0.5, -0.25), (0, 0.75, 0), (0, 0, 0.75), mat=2)        # x = -0.875
    tri((0.0, 0.75, -0.625), (0.5, 0, 0), (0, 0.5, 0))                  # z = -0.625
    for k in range(3):
        quad(rng.uniform([-0.6, 0.5, -0.5], [0.1, 1.2, 0.2]), rng.normal(0, 0.35, 3), rng.normal(0, 0.35, 3), 1 + k % 2, mat=1 + k)
        tri(rng.uniform([-0.6, 0.5, -0.5], [0.4, 1.4, 0.4]), rng.normal(0, 0.4, 3), rng.normal(0, 0.4, 3))
    return s


def _parallelogram(ta, tb):
    """Two triangles [3, 3] with four distinct corners, two of them shared, whose diagonals halve each other."""
    pts = np.unique(np.concatenate([ta, tb]).astype(np.float64), axis=0)
    if len(pts) != 4:
        return False
    return any(np.abs(pts[0] + pts[j] - pts[[k for k in (1, 2, 3) if k != j]].sum(0)).max() < 1e-6 for j in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, buffers, rays, kind, built-for-box, float64 facts) of one scene; computed once per module run."""
    from oracle import pyoracle as O
    from toyraygun_amd import capi
    t0 = time.time()
    if name == "cornell":
        scene = O.OracleScene.cornell_box()
    elif name == "zoo":
        scene, _ = box_zoo(O)
    elif name == "lattice":
        scene = O.OracleScene.cornell_lattice(6)       # 2,628 triangles: too large for LDS by itself, the path the million-triangle configuration runs
    else:
        scene = _soup(O)
    b = scene.buffers()
    tri_pos = b["positions"].reshape(-1, 3)[b["indices"].reshape(-1)].reshape(-1, 3, 3)
    frames = box_frames(capi.debug_boxes(b["positions"], b["indices"], b["material_ids"]))
    in_box = box_triangles(tri_pos, frames)
    lone = np.flatnonzero(in_box < 0)
    if name != "soup":
        # the LONE QUADS of a scene with boxes: pairs of consecutive triangles whose four corners are a parallelogram (walls, the light, the flat
        # faces of the zoo's almost-cube).  Its warped faces -- triangle pairs 0.6 degrees apart -- are lone TRIANGLES: the soup's business
        lone = np.array([t for k in lone[:-1] if in_box[k + 1] < 0 and _parallelogram(tri_pos[k], tri_pos[k + 1]) for t in (k, k + 1)], np.int64)
        assert len(lone) >= 12
    extent = float((tri_pos.reshape(-1, 3).max(0) - tri_pos.reshape(-1, 3).min(0)).max())
    parts = []
    if name == "lattice":
        assert len(frames) >= 200
        only = set(np.random.default_rng(5).choice(len(frames), 24, replace=False).tolist()) | {len(frames) - 1}
        parts.append(parallel_box_rays(O, frames, 11, per_box=0.25, only=only))
        parts.append(parallel_plane_rays(O, tri_pos, lone, extent, 12, per_tri=0.5))
    elif name == "soup":
        assert not frames and len(lone) == scene.ntris
        parts.append(parallel_plane_rays(O, tri_pos, lone, extent, 13, per_tri=1.0))
    else:
        assert len(frames) == (2 if name == "cornell" else 8)
        parts.append(parallel_box_rays(O, frames, 14, per_box=1.0))
        parts.append(parallel_plane_rays(O, tri_pos, lone, extent, 15, per_tri=0.5 if name == "cornell" else 0.34))
    rays = np.concatenate([p[0] for p in parts])
    kind = np.concatenate([p[1] for p in parts])
    which = np.concatenate([p[2] if i == 0 and frames else np.full(len(p[2]), -1) for i, p in enumerate(parts)])
    ref = O.intersect_nearest(scene, rays, brute=True)
    ref_any = O.intersect_any(scene, rays, brute=True) >= 0
    prim64, t64, margin = O.nearest_f64(scene, rays)
    decidable = margin >= MARGIN
    active = rays["maxDistance"] >= 0
    # the oracle's fp32 answer is the float64 one wherever float64 can decide: the reference of the shipped build is sound on this battery
    assert np.array_equal(ref["primitiveIndex"][decidable], prim64[decidable])
    assert np.array_equal(ref_any[decidable], prim64[decidable] >= 0)
    print("battery %s: %d rays, undecidable share per kind %s" % (name, len(rays), {RAY_KINDS[k]: round(float((~decidable[kind == k]).mean()), 3) for k in np.unique(kind)}))
    # what keeps the battery from hiding a failure
    assert (~decidable).mean() <= 0.10, (name, (~decidable).mean())
    exact0 = np.isin(kind, EXACT_ZERO_KINDS)
    assert exact0.sum() >= (500 if frames else 200) and (decidable & exact0).sum() >= 0.85 * exact0.sum(), (name, exact0.sum())
    facts = {"n": len(rays), "undecidable": float((~decidable).mean()), "hit": float((prim64 >= 0).mean()), "seconds": 0.0}
    if frames:
        through_aabb, meets_box = ray_box_f64(frames, which, rays)
        beside = through_aabb & ~meets_box & active                    # by float64: through a box's AABB and past the box -- where a slab that a
        hits_box = (prim64 >= 0) & (in_box[np.maximum(prim64, 0)] >= 0)  # parallel ray sees as infinite gives a false hit
        boxrays = which >= 0
        facts.update(beside=float(beside[boxrays].mean()), hits_box=float(hits_box[boxrays].mean()), beside_exact0=float(beside[boxrays & exact0].mean()))
        assert facts["beside"] >= 0.20 and facts["hits_box"] >= 0.20, (name, facts)
        assert facts["beside_exact0"] >= 0.20 and (boxrays & exact0).sum() >= 900, (name, facts)
    else:
        assert 0.15 <= facts["hit"] <= 0.85, (name, facts)
    facts["seconds"] = time.time() - t0
    print("battery %s: %s" % (name, facts))
    return scene, b, rays, kind, ref, ref_any, decidable, t64


def _check(capi, c, name, tag):
    """One context as configured, both builds, nearest and any-hit, against the oracle."""
    scene, b, rays, kind, ref, ref_any, decidable, t64 = _case(name)
    exact0 = np.isin(kind, EXACT_ZERO_KINDS)
    try:
        c.set_option(capi.OPT_STRICT, 1)
        got = c.trace(rays)
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "%s strict: %d records differ from the oracle" % (tag, int((got != ref).sum()))
        assert np.array_equal(c.trace(rays, any_hit=True) >= 0, ref_any), "%s strict any-hit" % (tag,)
        c.set_option(capi.OPT_STRICT, 0)
        fast = c.trace(rays)
        fast_any = c.trace(rays, any_hit=True) >= 0
        diff = (fast["primitiveIndex"] != ref["primitiveIndex"]) & decidable
        diff_any = (fast_any != ref_any) & decidable
        by_kind = {RAY_KINDS[k]: (int(diff[kind == k].sum()), int(diff_any[kind == k].sum()), int((kind == k).sum())) for k in np.unique(kind)}
        print("%s shipped: %d of %d decidable rays name another primitive, %d any-hit answers differ; per kind (nearest, any, rays): %s"
              % (tag, int(diff.sum()), int(decidable.sum()), int(diff_any.sum()), by_kind))
        # the rays whose zeros are plain +0.0 first, on their own: nothing that follows can dilute them
        assert not (diff & exact0).any(), "%s: %d decidable exact-zero rays picked another primitive" % (tag, int((diff & exact0).sum()))
        assert not (diff_any & exact0).any(), "%s: %d decidable exact-zero rays, any-hit answer differs" % (tag, int((diff_any & exact0).sum()))
        assert not diff.any(), "%s: %d decidable rays picked another primitive %s" % (tag, int(diff.sum()), by_kind)
        assert not diff_any.any(), "%s: %d decidable rays, any-hit answer differs %s" % (tag, int(diff_any.sum()), by_kind)
        # distance, hit point and weights on the rays double precision can decide (on the others -- a ray a few ulps off a face's plane that skims
        # along it -- the distance is decided by rounding like the primitive is)
        same = decidable & (ref["primitiveIndex"] >= 0)
        err = np.abs(fast["distance"].astype(np.float64) - ref["distance"]) - 3e-6 * (1.0 + np.abs(ref["distance"]))
        for i in np.flatnonzero(same & (err > 0))[:20]:
            print("%s distance: ray %d (%s) shipped %.9g oracle %.9g float64 %.9g" % (tag, i, RAY_KINDS[kind[i]], fast["distance"][i], ref["distance"][i], t64[i]))
        np.testing.assert_allclose(fast["distance"][same], ref["distance"][same], rtol=3e-6, atol=3e-6)
        tri_pos = b["positions"].reshape(-1, 3)[b["indices"].reshape(-1)].reshape(-1, 3, 3)
        T = tri_pos[ref["primitiveIndex"][same]].astype(np.float64)
        uvf, uvr = fast["coordinates"][same].astype(np.float64), ref["coordinates"][same].astype(np.float64)
        point = lambda uv: T[:, 0] + uv[:, :1] * (T[:, 1] - T[:, 0]) + uv[:, 1:] * (T[:, 2] - T[:, 0])
        assert np.abs(point(uvf) - point(uvr)).max() < 1e-5, tag
        edge = np.minimum(np.linalg.norm(T[:, 1] - T[:, 0], axis=1), np.linalg.norm(T[:, 2] - T[:, 0], axis=1))
        assert (np.abs(uvf - uvr).max(1) <= np.maximum(2e-5, 1e-5 / edge)).all(), tag
        inactive = rays["maxDistance"] < 0
        assert inactive.any() and (fast["distance"][inactive] < 0).all() and (fast["primitiveIndex"][inactive] == -1).all() and not fast_any[inactive].any()
    finally:
        c.set_option(capi.OPT_STRICT, 0)


def _context(capi, b, gpu_build=0, force_global=0):
    c = capi.Context(16, 16)
    c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
    c.set_option(capi.OPT_GPU_BUILD, gpu_build)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    return c


@pytest.mark.parametrize("force_global", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "zoo"])
def test_parallel_rays_box_scenes(capi, O, name, force_global):
    """Scenes staged in LDS (box leaves of twelve plane records: trav_box_planes) and the same scenes traversed from HBM (box records, and every
    lone quad dressed as a box of no thickness: trav_box_rec)."""
    b = _case(name)[1]
    c = _context(capi, b, force_global=force_global)
    try:
        st = c.stats()
        assert st.scene_in_lds == (0 if force_global else 1) and st.bvh_boxes == (2 if name == "cornell" else 8)
        _check(capi, c, name, (name, "hbm" if force_global else "lds"))
    finally:
        c.close()


@pytest.mark.parametrize("force_global", [0, 1])
def test_parallel_rays_scene_too_large_for_lds(capi, O, force_global):
    """2,628 triangles, 218 cubes: traversed from HBM by itself, not forced."""
    b = _case("lattice")[1]
    c = _context(capi, b, force_global=force_global)
    try:
        assert c.stats().scene_in_lds == 0 and c.stats().bvh_boxes >= 200
        _check(capi, c, "lattice", ("lattice", force_global))
    finally:
        c.close()


@pytest.mark.parametrize("force_global", [0, 1])
@pytest.mark.parametrize("builder", [0, 1, 2, 3])
def test_parallel_rays_lone_triangles_and_quads(capi, O, builder, force_global):
    """A soup without boxes, all four tree builders: the plane-form triangle and quad tests meet den == 0 and origins in the plane."""
    b = _case("soup")[1]
    c = _context(capi, b, gpu_build=builder, force_global=force_global)
    try:
        assert c.stats().bvh_boxes == 0 and c.stats().gpu_built == (1 if builder else 0)
        _check(capi, c, "soup", ("soup", builder, force_global))
    finally:
        c.close()


@pytest.mark.parametrize("switch,force_global", [("TRG_BVH_BOXES", 0), ("TRG_BVH_BOXES", 1), ("TRG_BVH_BOXES_HBM", 1)])
def test_parallel_rays_without_box_leaves(capi, O, monkeypatch, switch, force_global):
    """The control: with the box leaves switched off the plane-form tests answer the same battery."""
    monkeypatch.setenv(switch, "0")
    b = _case("zoo")[1]
    c = _context(capi, b, force_global=force_global)
    try:
        if switch == "TRG_BVH_BOXES":
            assert c.stats().bvh_boxes == 0
        _check(capi, c, "zoo", ("zoo", switch + "=0", force_global))
    finally:
        c.close()
