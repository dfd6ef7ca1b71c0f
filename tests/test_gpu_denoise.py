"""GPU tests (-m gpu) of include/trg_denoise.h: the first-hit guide buffers against the CPU oracle, the a-trous filter against the float64
reference written from the header (toyraygun_amd/denoise.py reference_denoise), and that the denoiser leaves the render path alone."""
import numpy as np
import pytest

from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def dn(capi):
    from toyraygun_amd import denoise
    denoise.load()
    return denoise


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _close(ctx, dn):
    dn.release(ctx)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------- 1. guides
def _interp(attr, prim, c0, c1, c2):
    """c0 * A0 + c1 * A1 + c2 * A2 in fp32, one rounding per operation (interpolateVertexAttribute, weights not normalised)."""
    a = attr.reshape(-1, 3, attr.shape[-1])[prim].astype(f32)
    return (c0[:, None] * a[:, 0] + c1[:, None] * a[:, 1]).astype(f32) + c2[:, None] * a[:, 2]


def _reference_guides(O, scene, b, w, h, frame, uniforms=None, offsets=None, textures=None):
    rays = O.raygen(w, h, frame, offsets=offsets, uniforms=uniforms)
    assert (rays["mask"] == 3).all()
    isect = O.intersect_nearest(scene, rays)
    prim, dist = isect["primitiveIndex"], isect["distance"]
    hit = prim >= 0
    p = np.where(hit, prim, 0)
    c0, c1 = isect["coordinates"][:, 0].astype(f32), isect["coordinates"][:, 1].astype(f32)
    c2 = (f32(1.0) - c0).astype(f32) - c1
    nrm = _interp(b["normals"], p, c0, c1, c2)
    alb = _interp(b["colors"], p, c0, c1, c2)
    if textures is not None:
        uvs, ids, imgs = textures
        uv = _interp(np.asarray(uvs, f32).reshape(-1, 2), p, c0, c1, c2)
        for i in np.flatnonzero(hit & (np.asarray(ids)[p] > 0)):
            img = imgs[int(ids[p[i]]) - 1]
            th, tw = img.shape[:2]
            fu, fv = uv[i] - np.floor(uv[i])
            x, y = min(tw - 1, int(f32(fu) * f32(tw))), min(th - 1, int(f32(fv) * f32(th)))
            alb[i] = alb[i] * (img[y, x, :3].astype(f32) / f32(255.0))
    alb[b["material_ids"][p] == 2] = 1.0
    nrm[~hit] = 0.0
    alb[~hit] = 0.0
    return rays, prim.reshape(h, w), dist.reshape(h, w), nrm.reshape(h, w, 3), alb.reshape(h, w, 3)


GRAZING_COS = 0.02


def _grazing(b, ref):
    """[h, w]: first hits that meet their triangle at under GRAZING_COS of cosine (|n . d| < 0.02: within 1.15 degrees of its plane).
    Any fp32 ray / plane distance divides by n . d, which carries at least its own rounding, 1 u = 2^-24 for unit vectors: u / cos of t.
    test_intersector's distance rule is 3e-6 = 50 u, so under cos = 1 / 50 ONE rounding of the denominator is more than the whole bar, for
    the shipped plane form and for the oracle's fp32 Moeller-Trumbore alike (measured: NOTEBOOK.md, "grazing hits").  Such a pixel is one
    that fp32 cannot decide, like a margin below 1e-5: the guide tests count it among the undecidable ones, under the same cap."""
    rays, prim = ref[0], ref[1]
    hit = (prim >= 0).reshape(-1)
    pos = np.asarray(b["positions"], np.float64).reshape(-1, 3)
    T = pos[np.asarray(b["indices"]).reshape(-1)].reshape(-1, 3, 3)[np.where(hit, prim.reshape(-1), 0)]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    d = rays["direction"].astype(np.float64)
    cos = np.abs((n * d).sum(1)) / np.maximum(np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1), 1e-300)
    return (hit & (cos < GRAZING_COS)).reshape(prim.shape)


def _shipped_attr_bars(b, prim):
    """Per pixel and channel, what the SHIPPED build's interpolated normal and albedo may differ from the oracle's by where the primitive agrees:
    its barycentrics are allowed 2e-5 each by test_intersector, and value = A2 + c0 (A0 - A2) + c1 (A1 - A2), so
    1e-6 + 2e-5 (|A0 - A2| + |A1 - A2|) of that primitive's corner values; 1e-6 alone for the albedo of an emitter, which is (1, 1, 1)."""
    p = np.where(prim >= 0, prim, 0)

    def bar(attr):
        a = np.asarray(attr, np.float64).reshape(-1, 3, 3)[p]
        return 1e-6 + 2e-5 * (np.abs(a[..., 0, :] - a[..., 2, :]) + np.abs(a[..., 1, :] - a[..., 2, :]))
    nb, ab = bar(b["normals"]), bar(b["colors"])
    ab[np.asarray(b["material_ids"])[p] == 2] = 1e-6
    return nb, ab


def _check_guides(g, ref, strict, undecidable=None, attr_bars=None):
    """attr_bars: (normal, albedo) bars [h, w, 3] in place of the flat 1e-6 -- for the shipped setting on triangles whose corners differ."""
    _, prim, dist, nrm, alb = ref
    got_prim = np.ascontiguousarray(g[1, ..., 3]).view(np.int32)
    ok = np.ones(prim.shape, bool) if strict else ~undecidable.reshape(prim.shape)
    assert np.array_equal(got_prim[ok], prim[ok]), "primitive ids differ on %d decidable pixels" % int((got_prim != prim)[ok].sum())
    same = ok & (got_prim == prim)
    if strict:
        assert np.array_equal(_bits(g[0, ..., 3]), _bits(dist))
    else:
        # the shipped intersector's distance is its own arithmetic (plane form): the existing rule of test_intersector, rtol = atol = 3e-6
        np.testing.assert_allclose(g[0, ..., 3][same], dist[same], rtol=3e-6, atol=3e-6)
    miss = got_prim < 0
    assert np.array_equal(miss[ok], (prim < 0)[ok]) and (g[0, ..., 3][miss] < 0).all()
    if attr_bars is None:
        assert np.abs(g[0, ..., :3][same] - nrm[same]).max() <= 1e-6, "guide normals differ"
        assert np.abs(g[1, ..., :3][same] - alb[same]).max() <= 1e-6, "guide albedo differs"
    else:
        assert not strict
        assert (np.abs(g[0, ..., :3][same] - nrm[same]) <= attr_bars[0][same]).all(), "guide normals differ"
        assert (np.abs(g[1, ..., :3][same] - alb[same]) <= attr_bars[1][same]).all(), "guide albedo differs"
    return miss


@pytest.fixture(scope="module")
def cornell_guides_ref(O, cornell):
    w, h = 64, 48
    b = cornell.buffers()
    off = O.pixel_offsets(w, h)
    out = {}
    for frame in (0, 7):
        ref = _reference_guides(O, cornell, b, w, h, frame, offsets=off)
        _, _, margin = O.nearest_f64(cornell, ref[0])
        out[frame] = (ref, margin < 1e-5)
    return out


@pytest.mark.parametrize("force_global", [0, 1])
def test_guides_match_the_oracle(capi, dn, O, cornell, cornell_guides_ref, force_global):
    """Cornell box, 64 x 48, frames 0 and 7, scene staged in LDS and kept in HBM.  Strict: ids equal everywhere, distances bit-equal, normal and
    albedo within 1e-6 (inputs <= 1, three fp32 products summed).  Shipped: the same on every pixel whose primitive float64 geometry can decide
    (margin >= 1e-5: the set rule of test_intersector); its distances are the plane test's own arithmetic, compared at that test's 3e-6."""
    w, h = 64, 48
    c = make_ctx(O, cornell, w, h, offsets=O.pixel_offsets(w, h))
    try:
        c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
        for frame, (ref, undecidable) in cornell_guides_ref.items():
            assert undecidable.mean() < 0.05
            for strict in (1, 0):
                c.set_option(capi.OPT_STRICT, strict)
                g = dn.guides(c, frame)
                miss = _check_guides(g, ref, strict, undecidable)
                assert miss.mean() < 0.5                     # (at 4:3 the corners of the frame look past the box)
                if not strict:
                    print("guides frame %d force_global %d shipped: %d distances not bit-equal to the oracle, max rel %.2e" % (
                        frame, force_global, int((_bits(g[0, ..., 3]) != _bits(ref[2])).sum()),
                        float(np.abs(g[0, ..., 3] / ref[2] - 1).max())))
        assert c.stats().scene_in_lds == (0 if force_global else 1)
    finally:
        _close(c, dn)


def test_guides_of_a_textured_scene_and_of_a_frame_with_misses(capi, dn, O, cornell):
    """(a) Cornell box + a quad with a non-power-of-two texture, texture coordinates beyond [0, 1]: the albedo carries the texel.  Strict setting:
    the texel a hit reads depends on its barycentrics, which only the strict intersector shares with the oracle bit for bit.
    (b) the camera turned to the right so that part of the frame looks past the box: those pixels have distance < 0 and id -1."""
    from toyraygun_amd import host
    w, h = 64, 48
    rng = np.random.default_rng(5)
    tex = rng.integers(0, 256, (37, 23, 4)).astype(np.uint8)
    hs = host.Scene.cornell_box()
    qv = np.array([[-0.9, 0.02, -0.2], [-0.2, 0.02, -0.2], [-0.2, 0.02, 0.9], [-0.9, 0.02, 0.9]], f32)
    qn = np.tile(np.array([[0, 1, 0]], f32), (4, 1))
    quv = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], f32)
    hs.add_textured_mesh(qv, qn, quv, [0, 2, 1, 0, 3, 2], np.eye(4, dtype=f32), (0.8, 0.7, 0.6), 1, host.Texture(rgba=tex))
    b = hs.buffers()
    uvs, ids, imgs = hs.texture_buffers()
    scene = O.OracleScene()
    scene.add_raw(b["positions"], b["normals"], b["colors"], b["material_ids"])
    off = O.pixel_offsets(w, h)
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.load_textures(uvs, ids, imgs)
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
        c.set_pixel_offsets(off)
        c.set_option(capi.OPT_STRICT, 1)
        ref = _reference_guides(O, scene, b, w, h, 3, offsets=off, textures=(uvs, ids, imgs))
        plain = _reference_guides(O, scene, b, w, h, 3, offsets=off)
        assert (np.abs(ref[4] - plain[4]).max(-1) > 1e-2).mean() > 0.02      # the texture is in the picture
        for fg in (0, 1):
            c.set_option(capi.OPT_FORCE_GLOBAL, fg)
            _check_guides(dn.guides(c, 3), ref, True)
    finally:
        _close(c, dn)
    u = O.make_uniforms(w, h, 0, at=(2.2, 1.0, -1.0))
    b = cornell.buffers()
    c = make_ctx(O, cornell, w, h, offsets=off, uniforms=u)
    try:
        ref = _reference_guides(O, cornell, b, w, h, 2, uniforms=u, offsets=off)
        _, _, margin = O.nearest_f64(cornell, ref[0])
        for strict in (1, 0):
            c.set_option(capi.OPT_STRICT, strict)
            g = dn.guides(c, 2)
            miss = _check_guides(g, ref, strict, margin < 1e-5)
            assert 0.05 < miss.mean() < 0.95
            assert (np.ascontiguousarray(g[1, ..., 3]).view(np.int32)[miss] == -1).all() and (g[0, ..., 3][miss] < 0).all()
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 2. filter
def _synthetic(w, h, seed):
    """Seeded colour in [0, 4]; three planar regions with different unit normals, a depth ramp with a step between regions, a block of misses."""
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 4.0, (h, w, 4)).astype(f32)
    yy, xx = np.mgrid[0:h, 0:w]
    region = np.where(xx < w * 0.45, 0, np.where(yy < h * 0.55, 1, 2))
    normals = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]], f32)
    g0 = np.zeros((h, w, 4), f32)
    g1 = np.zeros((h, w, 4), f32)
    g0[..., :3] = normals[region]
    g0[..., 3] = (2.0 + 0.03 * xx + 0.02 * yy + 0.5 * region).astype(f32)
    g1[..., :3] = rng.uniform(0.2, 1.0, (h, w, 3)).astype(f32)
    ids = np.array([3, 100000, 17], np.int32)[region]      # primitives of the Cornell box the contexts of these tests hold, and one beyond it
    ids[(region == 2) & (xx >= w - 9) & (yy >= h - 6)] = 35                  # a block whose first hit is the box's light: kept out like the misses
    miss = (xx >= w // 3) & (xx < w // 3 + 7) & (yy >= h // 4) & (yy < h // 4 + 6)
    g0[miss] = (0.0, 0.0, 0.0, -1.0)
    g1[miss, :3] = 0.0
    ids[miss] = -1
    g1[..., 3] = ids.view(f32)
    return color, g0, g1


def _smooth(w, h, seed, blocks=True):
    """What _synthetic leaves out: a slowly turning normal field whose per-pixel length is in [0.97, 1] (interpolated normals are shorter than 1:
    n_p . n_q is near 1 and hardly ever equal to it; |n|^256 >= 4e-4 keeps the weight of the centre tap, and with it every weight sum, far from
    fp32 underflow); a curved depth with one step; a flat region facing the camera whose depth gradient is exactly 0; albedo uniform in [0, 1]
    with about 10 % of the pixels at exactly 0, so that the 1e-3 clamp of demodulation and remodulation acts; colour = noise in [0, 4] x the
    clamped albedo; a block of misses and a block of first-hit emitters like _synthetic's, shrunk with the image so that small images keep
    pixels to filter.  At 1 x 1 that one pixel is still a miss (in _synthetic too, which at 5 x 3 leaves only column 0 as hits);
    blocks=False leaves both blocks out: every pixel is a hit that the filter works on (_smooth_hits: the 1 x 1 image whose pixel is one)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = 0.25 + 0.011 * xx + 0.004 * yy                                      # polar angle: about 0.6 rad across 48 pixels
    b = 0.5 + 0.013 * yy - 0.006 * xx
    n = np.stack([np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)], -1)
    z = 2.0 + 0.02 * xx + 0.0015 * (yy - 0.5 * h) ** 2 + np.where(xx >= 0.6 * w, 0.4, 0.0)
    flat = (xx < 0.4 * w) & (yy >= 0.65 * h)
    n[flat] = (0.0, 0.0, 1.0)
    z[flat] = 3.0
    g0 = np.zeros((h, w, 4), f32)
    g1 = np.zeros((h, w, 4), f32)
    g0[..., :3] = (n * rng.uniform(0.97, 1.0, (h, w, 1))).astype(f32)
    g0[..., 3] = z.astype(f32)
    alb = rng.uniform(0.0, 1.0, (h, w, 3))
    alb[rng.uniform(0.0, 1.0, (h, w)) < 0.1] = 0.0
    g1[..., :3] = alb.astype(f32)
    color = np.empty((h, w, 4), f32)
    color[..., :3] = (rng.uniform(0.0, 4.0, (h, w, 3)).astype(f32) * np.maximum(g1[..., :3], f32(1e-3))).astype(f32)
    color[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(f32)
    ids = np.where(xx < 0.5 * w, 3, 100000).astype(np.int32)                  # a primitive of the Cornell box, and one beyond it
    ids[(xx >= w - min(9, w // 3)) & (yy >= h - min(6, h // 3))] = 35         # first hit = the box's light
    miss = (xx >= w // 3) & (xx < w // 3 + min(7, (w + 1) // 2)) & (yy >= h // 4) & (yy < h // 4 + min(6, (h + 1) // 2))
    if not blocks:
        ids = np.where(xx < 0.5 * w, 3, 100000).astype(np.int32)
        miss[:] = False
    g0[miss] = (0.0, 0.0, 0.0, -1.0)
    g1[miss, :3] = 0.0
    ids[miss] = -1
    g1[..., 3] = ids.view(f32)
    return color, g0, g1


def _smooth_hits(w, h, seed):
    """_smooth without its blocks of misses and emitters."""
    return _smooth(w, h, seed, blocks=False)


_filter_refs = {}


def _filter_ref(dn, size, it, demod, material_ids):
    key = (size, it, demod)
    if key not in _filter_refs:
        color, g0, g1 = _synthetic(size[0], size[1], 11)
        _filter_refs[key] = dn.reference_denoise(color, g0, g1, iterations=it, demodulate=demod, material_ids=material_ids)
    return _filter_refs[key]


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", [(37, 29), (80, 50)])
def test_filter_matches_the_reference(capi, dn, O, cornell, size, strict):
    """37 x 29: no multiple of the tile and smaller than the reach of the large spacings (taps skipped, weights renormalised); 80 x 50: the LDS
    halo of spacings 1 and 2 crosses tile borders in both axes.  Iterations 0, 1, 3, 5 x demodulate 0, 1.  Bar, every pixel:
    |out - ref|_2 <= 1e-4 * max(1, |ref|_2) over the four channels; iterations = 0 returns the input bits."""
    w, h = size
    color, g0, g1 = _synthetic(w, h, 11)
    guides = np.stack([g0, g1])
    c = make_ctx(O, cornell, w, h)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for it in (0, 1, 3, 5):
            for demod in (0, 1):
                out = dn.denoise(c, color, guides, iterations=it, demodulate=demod)
                if it == 0:
                    assert np.array_equal(_bits(out), _bits(color))
                    continue
                ref = _filter_ref(dn, size, it, demod, cornell.buffers()["material_ids"])
                err = np.sqrt(((out.astype(np.float64) - ref) ** 2).sum(-1))
                bar = 1e-4 * np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))
                print("filter %dx%d strict %d it %d demod %d: worst err / bar %.3f" % (w, h, strict, it, demod, float((err / bar).max())))
                assert (err <= bar).all(), (it, demod, int((err > bar).sum()), float((err / bar).max()))
                assert np.array_equal(_bits(out[..., 3]), _bits(color[..., 3]))          # alpha passes through
                kept = (g0[..., 3] < 0) | dn.emitter_mask(g1, cornell.buffers()["material_ids"])
                assert kept.sum() > 42 and np.array_equal(_bits(out[kept]), _bits(color[kept]))   # misses and emitters copy their input
                assert np.abs(out[..., :3] - color[..., :3]).max() > 0.1                 # and it did filter
    finally:
        _close(c, dn)


def test_filter_refuses_bad_arguments(capi, dn, O, cornell):
    import torch
    w, h = 37, 29
    color, g0, g1 = _synthetic(w, h, 11)
    c = make_ctx(O, cornell, w, h)
    try:
        with pytest.raises(capi.TrgError):
            dn.denoise(c, color, np.stack([g0, g1]), iterations=7)
        t = torch.from_numpy(color).cuda()
        g = torch.from_numpy(np.stack([g0, g1])).cuda()
        with pytest.raises(capi.TrgError):
            dn.denoise(c, t, g, out=t)                                                   # out may not alias the input
        out = dn.denoise(c, t, g, iterations=3)                                          # tensors are used in place, on the context's stream
        c.sync()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(dn.denoise(c, color, np.stack([g0, g1]), iterations=3)))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("strict", [1, 0])
def test_edges_hold(capi, dn, O, cornell, strict):
    """Two half images with orthogonal normals and colours 0 / 1: w_n = 0 across the edge, so after 5 iterations each side still is its input."""
    w, h = 40, 20
    g0 = np.zeros((h, w, 4), f32); g1 = np.ones((h, w, 4), f32)
    g0[..., :3] = (0.0, 0.0, 1.0); g0[..., 3] = 2.0
    g0[:, w // 2:, :3] = (1.0, 0.0, 0.0)
    g1[..., 3] = np.zeros((h, w), np.int32).view(f32)
    color = np.zeros((h, w, 4), f32)
    color[:, w // 2:, :3] = 1.0
    color[..., 3] = 1.0
    c = make_ctx(O, cornell, w, h)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        out = dn.denoise(c, color, np.stack([g0, g1]), iterations=5)
        assert np.array_equal(_bits(out), _bits(color))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. it denoises
def test_it_denoises(capi, dn, O, cornell):
    """Cornell box, 128 x 96, 3 bounces: the denoised 4-spp frame is closer to the oracle's 256-spp frame than the raw 4-spp frame is."""
    w, h = 128, 96
    off = O.pixel_offsets(w, h)
    ref, _ = O.render(cornell, w, h, 256, 3, offsets=off, want_stats=False)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        den = dn.render_denoised(c, 0, 4, 3)
        noisy = c.read_accum()
        rmse = lambda a: float(np.sqrt(((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2).mean()))
        print("rmse against 256 spp: noisy %.5f denoised %.5f" % (rmse(noisy), rmse(den)))
        assert rmse(den) < rmse(noisy)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 5. it disturbs nothing
def test_render_denoised_leaves_accumulation_and_counters_alone(capi, dn, O, cornell):
    w, h = 64, 48
    off = O.pixel_offsets(w, h)
    a = make_ctx(O, cornell, w, h, offsets=off)
    b = make_ctx(O, cornell, w, h, offsets=off)
    rays = lambda s: (s.primary_rays, s.bounce_rays, s.shadow_rays, s.shaded_hits)
    try:
        b.render(0, 4, 3)
        plain4, rays4 = b.read_accum(), rays(b.stats())
        den = dn.render_denoised(a, 0, 4, 3)
        assert np.array_equal(_bits(a.read_accum()), _bits(plain4))
        assert rays(a.stats()) == rays4                      # the guide rays go through the uncounted stage-level tracer
        dn.guides(a, 0)
        dn.denoise(a, plain4, dn.guides(a, 0))
        assert rays(a.stats()) == rays4
        assert not np.array_equal(_bits(den), _bits(plain4))
        a.render(4, 4, 3)
        b.reset_stats()
        b.render(0, 8, 3)
        assert np.array_equal(_bits(a.read_accum()), _bits(b.read_accum()))
        assert rays(a.stats()) == rays(b.stats())
    finally:
        _close(a, dn)
        _close(b, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 6. plugin
def test_plugin_denoise_switch(capi, dn, tmp_path):
    """The engine plugin through its demo app (a HipRenderer driven like the reference's main.cpp): denoise=0 writes the same picture as no
    argument at all; denoise=5 writes another one -- trg_postprocess of what the Python path denoises from the same accumulation."""
    import os
    import subprocess
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 96, 64, 4, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, timeout=120)
        return host.Texture(path=path).rgba()
    plain, off, on = run("plain.png"), run("off.png", "denoise=0"), run("on.png", "denoise=5")
    assert np.array_equal(plain, off)
    assert not np.array_equal(plain, on)
    b = host.Scene.cornell_box().buffers()
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        c.render(0, frames, bounces)
        assert np.array_equal(c.postprocess(flip_y=True), plain)
        acc = torch.from_numpy(c.read_accum()).cuda()
        g = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
        den = dn.denoise(c, acc, dn.guides(c, 0, out=g), iterations=5)
        c.sync()
        c.bind_accum(den.data_ptr())
        try:
            assert np.array_equal(c.postprocess(flip_y=True), on)
        finally:
            c.bind_accum(None)
    finally:
        _close(c, dn)
