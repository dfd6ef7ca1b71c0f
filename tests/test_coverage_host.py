"""Host-side checks of the centre guides and the coverage history (include/trg_denoise.h, "PIXEL FOOTPRINTS"; toyraygun_amd/denoise.py
reference_centre_rays, reference_agreement, reference_temporal(coverage=cov_min)): the exported surface, the centre rays, that the setting off
is the reference as it was, the reference against a per-pixel loop written once more from the header, the consequences the header states, the
populations of undecidable and of mixed pixels, and -- on the oracle's renders, in float64 -- that the step comes closer to a 512-spp render
with the setting on.  No GPU.

THE BOUNDS.  Unit length: 1 ulp of 1 (2^-23) on the direction's length as fp32 forms it -- the root of the left-to-right sum of squares, the
tracer's own view of the vector; an ulp is a quantity of that format.  The EXACT (float64) length of an fp32 vector normalised in fp32 by
trg_raygen's arithmetic cannot be promised to 2^-23, so it is held to what that arithmetic can promise, to first order in u = 2^-24: the sum of
squares carries three roundings (the products, weighted, count as one; two additions), 3 u, halved by the root: 1.5 u; the root, the reciprocal
and the three products (weighted by d_i^2: one) add u each: 4.5 u = 2.25 * 2^-23.  MEASURED: at most 1.38e-7 = 1.16 * 2^-23 over the four
cameras.  The projection: 1e-3 px, the issue's.  The reference as it was: the golden planes were written by reference_temporal before the
coverage argument existed; 1e-12 relative to max(1, |value|) lets another libm's exp and pow through, nothing else.  Per-pixel
loop: 1e-9 relative, two float64 evaluations that differ in summation order only, on the pixels whose discrete decisions are not `near`.
`near` under 1 % each, the cap of the other decisions (tests/test_temporal_host.py).  Mixed pixels at rest after eight calls at 64 x 48: more
than none, at most a quarter of the hits (the float64 prototype: 268 of 2,283).  The rmse ratios: at most 0.8 on all four sequences, the issue's
(the prototype's worst: 0.638)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.denoise_literal import CLAMP, _Guides, _lum
from tests.test_gpu_denoise import _interp
from tests.test_temporal_host import CAMERAS, NEAR_CAP, camera_uniforms, position_plane, seeded_colour
from tests.test_temporal_synthetic_host import SCHEDULE, SHAPES_PARAMS, near_caps, schedule_frames, spatial_form
from tests.test_vmean_host import _rmse, orbit_eye
from tests.util import CAMERAS as UNIFORM_CAMERAS

AWAY = UNIFORM_CAMERAS["outside_back"]            # the camera that faces partly away: centre misses beside hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_denoise.h")
f32 = np.float32

NEW_SYMBOLS = {"trg_guides_render_centre", "trg_guides_render_centre_motion", "trg_guides_centre_read", "trg_guides_centre_motion_read",
               "trg_temporal_set_coverage", "trg_temporal_coverage"}
COV_MIN = 0.9
# (name, calls, spp, degrees the eye turns per call): the two sequences of the issue, each with the variance of the mean off and on
SEQUENCES = [("at rest 8 x 1", 8, 1, 0.0), ("turning 8 x 2", 8, 2, 1.0)]
HELPS_BOUND = 0.8


def seeded_agreement(g, seed, zeros=0.2):
    """A 0 / 1 plane with about one fifth zeros."""
    h, w = g.shape[1:3]
    return (np.random.default_rng(seed).uniform(0.0, 1.0, (h, w)) >= zeros).astype(f32)


def with_agreement(X, A):
    X = np.array(X, f32)
    X[..., 3] = A
    return X


def test_header_exports_and_python_agree_on_the_coverage_entry_points(built):
    from toyraygun_amd import capi, denoise
    declared = set(denoise.header_symbols(HEADER))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(denoise.SYMBOL_NAMES)
    assert sorted(denoise.SYMBOL_NAMES) == sorted(declared)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    text = open(HEADER).read()
    assert float(re.search(r"#define TRG_TEMPORAL_COVERAGE_MIN_DEFAULT ([0-9.]+)f", text).group(1)) == denoise.COVERAGE_MIN_DEFAULT == COV_MIN
    assert "PIXEL FOOTPRINTS" in text and text.count("NOT COVERED") >= 3
    for name in ("guides_centre", "temporal_set_coverage", "temporal_coverage", "reference_centre_rays", "reference_agreement"):
        assert callable(getattr(denoise, name))
    assert [k for k, _ in denoise.TemporalParams._fields_] == list(denoise._TEMPORAL_DEFAULTS)      # trg_temporal_params keeps its layout


# ---- the centre rays -------------------------------------------------------------------------------------------------------------------------
def test_centre_rays(built, O):
    """Unit length to 1 ulp; at 1 x 1 the ray is the view axis; the point at distance 1, pushed through trg_temporal_view_proj of the same
    uniforms, lands within 1e-3 px of the pixel's centre -- for the four cameras, at a ragged size; the frame index plays no part."""
    from toyraygun_amd import capi, denoise as dn
    w, h = 37, 29
    for k in range(len(CAMERAS)):
        u = camera_uniforms(O, w, h, k)
        rays = dn.reference_centre_rays(u, w, h)
        assert rays.dtype == capi.RAY_DTYPE and rays.shape == (w * h,)
        assert (rays["mask"] == 3).all() and np.isposinf(rays["maxDistance"]).all() and (rays["color"] == np.array([1, 1, 1, 0], f32)).all()
        assert (rays["origin"] == np.array(CAMERAS[k], f32)).all()
        d32 = rays["direction"]
        assert d32.dtype == f32
        len32 = np.sqrt((d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]) + d32[:, 2] * d32[:, 2])
        assert len32.dtype == f32 and np.abs(len32.astype(np.float64) - 1.0).max() <= 2.0 ** -23
        d = d32.astype(np.float64)
        exact = np.abs(np.sqrt((d * d).sum(-1)) - 1.0).max()
        print("centre rays, camera %d: the float64 length of the fp32 directions is within %.3e = %.3f * 2^-23 of 1" % (k, exact, exact * 2.0 ** 23))
        assert exact <= 2.25 * 2.0 ** -23
        vp = dn.temporal_view_proj(u).astype(np.float64).reshape(4, 4)
        P = np.concatenate([rays["origin"].astype(np.float64) + d, np.ones((w * h, 1))], 1)
        clip = P @ vp.T
        sx, sy = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * w, (clip[:, 1] / clip[:, 3] * 0.5 + 0.5) * h
        yy, xx = np.mgrid[0:h, 0:w]
        err = max(np.abs(sx - (xx.reshape(-1) + 0.5)).max(), np.abs(sy - (yy.reshape(-1) + 0.5)).max())
        print("centre rays, camera %d: the point at distance 1 lands within %.2e px of the pixel centre" % (k, err))
        assert err <= 1e-3
        u.frameIndex = 77
        assert np.array_equal(dn.reference_centre_rays(O.uniforms_bytes(u), w, h), rays)
        one = dn.reference_centre_rays(camera_uniforms(O, 1, 1, k), 1, 1)
        axis = np.array((0.0, 1.0, -1.0)) - np.array(CAMERAS[k])
        assert np.abs(one["direction"][0] - axis / np.linalg.norm(axis)).max() <= 1e-6


# ---- frames from the oracle: centre guides, X with the agreement flag in .w ------------------------------------------------------------------------
def guides_of_isect(b, rays, isect, w, h):
    """(guides [2, h, w, 4], X [h, w, 4] with X.w = 0) of these rays and their hit records -- the oracle's or the device's own -- in the gather's
    arithmetic, as trg_guides_render_pos defines them.  b: the scene's buffers (no textures)."""
    prim = isect["primitiveIndex"]
    hit = prim >= 0
    p = np.where(hit, prim, 0)
    c0, c1 = isect["coordinates"][:, 0].astype(f32), isect["coordinates"][:, 1].astype(f32)
    c2 = (f32(1.0) - c0).astype(f32) - c1
    nrm, alb = _interp(b["normals"], p, c0, c1, c2), _interp(b["colors"], p, c0, c1, c2)
    alb[b["material_ids"][p] == 2] = 1.0
    nrm[~hit] = 0.0
    alb[~hit] = 0.0
    g = np.zeros((2, h, w, 4), f32)
    g[0, ..., :3] = nrm.reshape(h, w, 3)
    g[0, ..., 3] = np.where(hit, isect["distance"], f32(-1.0)).reshape(h, w)
    g[1, ..., :3] = alb.reshape(h, w, 3)
    g[1, ..., 3] = prim.astype(np.int32).view(f32).reshape(h, w)
    return g, position_plane(rays, g)


def guides_of_rays(O, scene, rays, w, h):
    isect = O.intersect_nearest(scene, rays)
    return guides_of_isect(scene.buffers(), rays, isect, w, h) + (isect,)


def centre_frame(O, dn, scene, w, h, frame, uniforms, offsets, plane_tol=0.02, normal_tol=0.9):
    """(guides, X with A in .w, near of the agreement) of trg_guides_render_centre from the oracle's intersector."""
    b = scene.buffers()
    g, X, isect_c = guides_of_rays(O, scene, dn.reference_centre_rays(uniforms, w, h), w, h)
    rays_j = O.raygen(w, h, frame, offsets=offsets, uniforms=uniforms)
    A, near = dn.reference_agreement(isect_c, g[0], X, O.intersect_nearest(scene, rays_j), rays_j, b["normals"], b["material_ids"], plane_tol, normal_tol)
    return g, with_agreement(X, A), near


# ---- off is what it was; on moves what the header says -------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "temporal_reference_9x7.npz")


@pytest.mark.parametrize("name,kw", [("plain", {}), ("track", dict(track=True)), ("lag", dict(lag=3.0))], ids=["plain", "track", "lag"])
def test_coverage_none_is_the_reference_as_it_was(cornell, name, kw):
    """The synthetic schedule at 9 x 7, chained: with coverage=None -- and without the argument -- the new history, (I, V_0) and `near` of every
    call are the planes tests/golden/temporal_reference_9x7.npz holds, which reference_temporal wrote before the argument existed (plain, with
    the variance of the mean, with the lag correction; float64)."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    gold = np.load(GOLDEN)
    w, h = 9, 7
    hist, longest = None, 0.0
    for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, SCHEDULE)):
        for args in (dict(coverage=None), {}):
            res = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, material_ids=mats, **args, **kw, **SHAPES_PARAMS)
            assert len(res) == 3
            for got, key in zip(res, ("new", "iv", "near")):
                want = gold["%s_%d_%s" % (name, call, key)]
                assert got.shape == want.shape and got.dtype == want.dtype, (call, key)
                if key == "near":
                    assert np.array_equal(got, want), call
                else:
                    assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (call, key)
        hist = res[0]
        longest = max(longest, float(hist[0, ..., 3].max()))
    assert longest >= 4 and sum(int(gold["%s_%d_near" % (name, c)].sum()) for c in range(9)) < 0.3 * 9 * w * h


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_off_is_off_and_coverage_touches_what_it_says(cornell, dtype):
    """The synthetic schedule at 17 x 33 with a seeded A.  coverage=None is the call without the argument, three results, Hm.w = 0 (that both are
    the reference as it was: the test above).  With a cov_min: Hc, the moments, F and X are the plain step's exactly (fed the covered chain's own history, whose Hm.w the plain step does not
    read); iv.rgb moves on the mixed pixels alone; V_0 stays where the history is four frames old and on pixels with no mixed pixel in their
    7 x 7 window; `near` only grows; the mask and the marked G0 are the two extra results."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = 17, 33
    hist, mixed_seen, moved = None, 0, 0
    for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, SCHEDULE)):
        X = with_agreement(X, seeded_agreement(g, 40 + call))
        args = (colour, g[0], g[1], X, hist, vp)
        plain = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, **SHAPES_PARAMS)
        off = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, coverage=None, **SHAPES_PARAMS)
        on = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, coverage=COV_MIN, **SHAPES_PARAMS)
        assert len(plain) == len(off) == 3 and len(on) == 5
        for a, b in zip(plain[:2] + plain[2], off[:2] + off[2]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert (off[0][1, ..., 2:] == 0).all()
        new, iv, (near, near_n), mixed, marked = on
        assert new.dtype == dtype and iv.dtype == dtype and mixed.dtype == bool and marked.dtype == dtype
        assert np.array_equal(new[0], plain[0][0]) and np.array_equal(new[2:], plain[0][2:])                 # Hc, F (unmarked), X
        assert np.array_equal(new[1, ..., :3], plain[0][1, ..., :3])                                         # m1, m2, and 0
        hit = new[2, ..., 3] >= 0
        cov = new[1, ..., 3]
        assert (cov[~hit] == 0).all() and (cov >= 0).all() and (cov <= 1).all()
        assert np.array_equal(mixed, hit & (cov < dtype(f32(COV_MIN))))
        assert np.array_equal(marked[..., :3], new[2, ..., :3]) and np.array_equal(marked[..., 3] < 0, ~hit | mixed)
        assert np.array_equal(marked[..., 3][~mixed], new[2, ..., 3][~mixed])
        assert np.array_equal(iv[..., :3][~mixed], plain[1][..., :3][~mixed])
        alb = np.maximum(g[1, ..., :3].astype(dtype), dtype(f32(1e-3)))
        assert np.array_equal(iv[..., :3][mixed], (new[0, ..., :3] * alb)[mixed])
        assert (near >= plain[2][0]).all() and np.array_equal(near_n, plain[2][1])
        from toyraygun_amd.denoise import _shift
        beside = np.zeros((h, w), bool)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                beside |= _shift(mixed, dx, dy, False)[0]
        N = new[0, ..., 3]
        same_v = hit & ~mixed & ((N >= 4) | ~beside)
        assert np.array_equal(iv[..., 3][same_v], plain[1][..., 3][same_v])
        assert np.array_equal(iv[..., 3][mixed], np.maximum(0.0, new[1, ..., 1] - new[1, ..., 0] * new[1, ..., 0])[mixed])
        mixed_seen += int(mixed.sum())
        moved += int((iv[..., 3] != plain[1][..., 3])[hit & ~mixed].sum())
        hist = new
    assert mixed_seen > 100 and moved > 0, (mixed_seen, moved)


# ---- the per-pixel loop ----------------------------------------------------------------------------------------------------------------------
def _literal_cov(colour, g0, g1, X, hist, vp, mats, q, cov_min):
    """cov, the mixed mask and a mixed pixel's (I, V_0) of the header for every pixel, one pixel and one tap at a time in Python floats, with
    what they need of the step: the reprojection's valid taps, N, am and a, the accumulated colour and moments.  hist: the previous call's four
    planes or None.  Returns (cov [h, w], mixed [h, w] bool, iv [h, w, 4] -- filled on the mixed pixels only)."""
    G_ = _Guides(g0, g1, mats)
    h, w = G_.h, G_.w
    col = np.asarray(colour, np.float32).tolist()
    Xl = np.asarray(X, np.float32).tolist()
    alpha, alpha_m, ptol, ntol = (float(f32(q[k])) for k in ("alpha", "alpha_moments", "plane_tol", "normal_tol"))
    maxh, cmin = float(int(q["max_history"])), float(f32(cov_min))
    m = None if vp is None else [float(v) for v in np.asarray(vp, np.float32).reshape(16)]
    H = None if hist is None else [np.asarray(p, np.float32).tolist() for p in hist]          # (a history is fp32 planes, as the device holds them)

    def unit(v):
        ln = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return (None if not ln > 0 else (v[0] / ln, v[1] / ln, v[2] / ln))
    cov, mixed, iv = np.zeros((h, w)), np.zeros((h, w), bool), np.zeros((h, w, 4))
    for y in range(h):
        for x in range(w):
            if G_.miss[y][x]:
                continue
            D = [col[y][x][k] / G_.a[y][x][k] if q["demodulate"] else col[y][x][k] for k in range(3)]
            l = _lum(D)
            A = Xl[y][x][3]
            W = nh = s1 = s2 = sc = 0.0
            sI = [0.0, 0.0, 0.0]
            n = unit(G_.n[y][x])
            if H is not None and n is not None:
                P = Xl[y][x]
                clip = [m[4 * j] * P[0] + m[4 * j + 1] * P[1] + m[4 * j + 2] * P[2] + m[4 * j + 3] for j in (0, 1, 3)]
                if clip[2] > 0:
                    fx, fy = (clip[0] / clip[2] * 0.5 + 0.5) * w - 0.5, (clip[1] / clip[2] * 0.5 + 0.5) * h - 0.5
                    if -1 <= fx < w and -1 <= fy < h:
                        x0, y0 = math.floor(fx), math.floor(fy)
                        tx, ty = fx - x0, fy - y0
                        for j in (0, 1):
                            for i in (0, 1):
                                qx, qy = x0 + i, y0 + j
                                if not G_.inside(qx, qy) or not H[2][qy][qx][3] >= 0:
                                    continue
                                xq = H[3][qy][qx]
                                if not abs(n[0] * (xq[0] - P[0]) + n[1] * (xq[1] - P[1]) + n[2] * (xq[2] - P[2])) <= ptol * G_.z[y][x]:
                                    continue
                                nq = unit(H[2][qy][qx])
                                if nq is None or not n[0] * nq[0] + n[1] * nq[1] + n[2] * nq[2] >= ntol:
                                    continue
                                b = (tx if i else 1 - tx) * (ty if j else 1 - ty)
                                W += b
                                nh += b * H[0][qy][qx][3]
                                s1 += b * H[1][qy][qx][0]
                                s2 += b * H[1][qy][qx][1]
                                sc += b * H[1][qy][qx][3]
                                for k in range(3):
                                    sI[k] += b * H[0][qy][qx][k]
            if W > 0:
                N = min(nh / W + 1, maxh)
                a, am = max(alpha, 1 / N), max(alpha_m, 1 / N)
                I = [sI[k] / W + a * (D[k] - sI[k] / W) for k in range(3)]
                m1, m2 = s1 / W + am * (l - s1 / W), s2 / W + am * (l * l - s2 / W)
                cov[y, x] = sc / W + am * (A - sc / W)
            else:
                I, m1, m2 = D, l, l * l
                cov[y, x] = A
            if cov[y, x] < cmin:
                mixed[y, x] = True
                iv[y, x, :3] = [I[k] * G_.a[y][x][k] if q["demodulate"] else I[k] for k in range(3)]
                iv[y, x, 3] = max(0.0, m2 - m1 * m1)
    return cov, mixed, iv


@pytest.mark.parametrize("demodulate", [1, 0])
def test_reference_coverage_is_the_per_pixel_loop(cornell, demodulate):
    """The synthetic schedule (moving cameras, rejected taps, N < 4 and N >= 4) at 17 x 33 with max_history = 6 and a seeded 0 / 1 plane A of about
    one fifth zeros: Hm.w, the mixed mask and a mixed pixel's (I, V_0) of reference_temporal(coverage=0.9) against the loop above, fed with the
    reference's own previous history, to 1e-9 of the value's scale on every pixel whose decisions are not `near`; and V_0 of the other pixels
    below four frames is the spatial form over the MARKED guide."""
    from toyraygun_amd import denoise as dn
    assert CLAMP == float(f32(1e-3))
    mats = cornell.buffers()["material_ids"]
    w, h = 17, 33
    params = dict(SHAPES_PARAMS, demodulate=demodulate)
    q = dict(dn._TEMPORAL_DEFAULTS, **params)
    hist, n_mixed, n_blend, n_short = None, 0, 0, 0
    for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, SCHEDULE)):
        X = with_agreement(X, seeded_agreement(g, 40 + call))
        new, iv, (near, near_n), mixed, marked = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, material_ids=mats, near_parts=True, coverage=COV_MIN, **params)
        near_caps(near, near_n, call)
        cov, lmixed, liv = _literal_cov(colour, g[0], g[1], X, hist, vp, mats, q, COV_MIN)
        ok = ~near
        assert np.abs(new[1, ..., 3] - cov)[ok].max() <= 1e-9, call
        assert np.array_equal(mixed[ok], lmixed[ok])
        sel = ok & mixed
        err = np.abs(iv - liv) / np.maximum(1.0, np.abs(liv))
        assert err[sel].max() <= 1e-9 if sel.any() else True, (call, float(err[sel].max()))
        # the pixels beside them: V_0 below four frames is the spatial estimate over the marked guide, from this call's moments
        marked_planes = new.copy()
        marked_planes[2] = marked
        short = ok & ~near_n & (marked[..., 3] >= 0) & (new[0, ..., 3] < 4)
        want = spatial_form(dn, marked_planes, params)
        assert np.abs(iv[..., 3] - want)[short].max() <= 1e-9 * max(1.0, float(want.max())) if short.any() else True
        n_mixed += int(sel.sum())
        n_blend += int((ok & (new[0, ..., 3] > 1) & (new[1, ..., 3] > 0) & (new[1, ..., 3] < 1)).sum())
        n_short += int(short.sum())
        hist = new
    assert n_mixed > 100 and n_blend > 100 and n_short > 100, (n_mixed, n_blend, n_short)


# ---- the consequences of the header ------------------------------------------------------------------------------------------------------------
def test_consequences_on_the_cornell_guides(O, cornell):
    """37 x 29, the oracle's centre guides, the four cameras of tests/test_temporal_host.py in turn.  A = 1 on every hit: cov is exactly 1 in
    float64 and in the float32 mode, nobody is mixed, and everything but Hm.w is the setting-off step exactly.  A = 0 everywhere: every hit is
    mixed from the first call on, and the step's output -- through five iterations -- is the accumulated colour remodulated once.  cov within
    1e-4 of cov_min is marked `near`."""
    from toyraygun_amd import denoise as dn
    w, h = 37, 29
    mats = cornell.buffers()["material_ids"]
    off = O.pixel_offsets(w, h)
    for dtype in (np.float64, np.float32):
        h1, h0, hp, prev_vp = None, None, None, None
        for call, k in enumerate((0, 1, 2, 3, 3)):
            u = camera_uniforms(O, w, h, k)
            g, X, _ = centre_frame(O, dn, cornell, w, h, call, u, off)
            colour = seeded_colour(g, 700 + call)
            hit = ~((g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats))
            kw = dict(material_ids=mats, dtype=dtype)
            plain = dn.reference_temporal(colour, g[0], g[1], X, hp, prev_vp, **kw)
            ones = dn.reference_temporal(colour, g[0], g[1], with_agreement(X, hit.astype(f32)), h1, prev_vp, coverage=COV_MIN, **kw)
            assert (ones[0][1, ..., 3][hit] == 1).all() and (ones[0][1, ..., 3][~hit] == 0).all() and not ones[3].any()
            assert np.array_equal(ones[0][[0, 2, 3]][..., :3], plain[0][[0, 2, 3]][..., :3]) and np.array_equal(ones[0][1, ..., :3], plain[0][1, ..., :3])
            assert np.array_equal(ones[0][0], plain[0][0]) and np.array_equal(ones[1], plain[1]) and np.array_equal(ones[2], plain[2])
            assert np.array_equal(ones[4], plain[0][2])
            zeros = dn.reference_temporal(colour, g[0], g[1], with_agreement(X, 0.0), h0, prev_vp, coverage=COV_MIN, **kw)
            assert np.array_equal(zeros[3], hit) and (zeros[0][1, ..., 3] == 0).all() and (zeros[4][..., 3] < 0).all()
            assert np.array_equal(zeros[0][0], plain[0][0])                                                # the accumulation itself is untouched
            alb = np.maximum(g[1, ..., :3].astype(dtype), dtype(f32(1e-3)))
            want = np.where(hit[..., None], zeros[0][0, ..., :3] * alb, colour[..., :3].astype(dtype))
            assert np.array_equal(zeros[1][..., :3], want)
            if dtype is np.float64:
                rgb, _ = dn.reference_atrous_variance(zeros[1][..., :3], zeros[1][..., 3], zeros[4], g[1], material_ids=None)
                assert np.array_equal(rgb, want)
            h1, h0, hp, prev_vp = ones[0], zeros[0], plain[0], dn.temporal_view_proj(u)
    # the new decision is marked: a plane A that puts cov within 1e-4 of cov_min on one pixel, on another just outside
    u = camera_uniforms(O, w, h, 0)
    g, X, _ = centre_frame(O, dn, cornell, w, h, 0, u, off)
    hit = ~((g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats))
    ys, xs = np.nonzero(hit)
    A = np.ones((h, w), f32)
    A[ys[0], xs[0]], A[ys[1], xs[1]], A[ys[2], xs[2]] = f32(COV_MIN + 5e-5), f32(COV_MIN - 5e-4), f32(COV_MIN - 5e-5)
    res = dn.reference_temporal(seeded_colour(g, 1), g[0], g[1], with_agreement(X, A), None, None, material_ids=mats, coverage=COV_MIN)
    assert res[2][ys[0], xs[0]] and not res[2][ys[1], xs[1]] and res[2][ys[2], xs[2]] and res[2].sum() == 2
    assert not res[3][ys[0], xs[0]] and res[3][ys[1], xs[1]] and res[3][ys[2], xs[2]]


# ---- the populations -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (37, 29), (17, 33), (5, 3)], ids=lambda s: "%dx%d" % s)
def test_undecidable_pixels_stay_under_the_cap(O, cornell, size):
    """The cameras the GPU tests use, on the oracle's hit records, at their sizes: `near` of the agreement under 1 % for every camera and the frame
    indices 0 .. 3 (at most one pixel on an image under 256 pixels), and some pixels agree and some do not.  The camera that faces partly away
    ("outside_back" of tests/util.py: outside the room) has centre misses beside hits."""
    from toyraygun_amd import denoise as dn
    w, h = size
    off = O.pixel_offsets(w, h)
    cap = NEAR_CAP * w * h if w * h >= 256 else 1
    for k, (eye, at) in enumerate([(eye, (0.0, 1.0, -1.0)) for eye in CAMERAS] + [AWAY]):
        u = O.make_uniforms(w, h, 0, eye=eye, at=at)
        for frame in range(4):
            g, X, near = centre_frame(O, dn, cornell, w, h, frame, u, off)
            hit = g[0, ..., 3] >= 0
            A = X[..., 3]
            assert near.sum() <= cap, (k, at, frame, int(near.sum()))
            assert set(np.unique(A)) <= {0.0, 1.0} and (A[~hit] == 0).all()
            if w * h >= 256:                                      # (seen from outside the room is one flat wall: all of its pixels may agree)
                assert 0.5 < A[hit].mean() and ((eye, at) == AWAY or A[hit].mean() < 1.0), (k, frame, float(A[hit].mean()))
        if (eye, at) == AWAY and w * h >= 256:
            assert 0.05 < (~hit).mean() < 0.95


def run_sequence(O, dn, scene, w, h, bounces, calls, spp, degrees, track, coverage, frames, **params):
    """tests/test_vmean_host.py's run_sequence with the setting: the last output of `calls` temporal steps of `spp` samples each on the oracle's
    renders, float64.  coverage None: the jittered guides of frame b = k * spp, as trg_render_temporal takes them today; else the centre guides
    with the agreement flag of frame b.  Returns (rgb of the last call, its uniforms, the last step's results, the `near` counts per call)."""
    from tests.test_temporal_host import oracle_frame
    mats = scene.buffers()["material_ids"]
    off = O.pixel_offsets(w, h)
    hist, prev_vp, nears = None, None, []
    for k in range(calls):
        eye = orbit_eye(k * degrees)
        b = k * spp
        key = (tuple(np.round(eye, 9)), b, spp)
        if key not in frames:
            u = O.make_uniforms(w, h, 0, eye=eye)
            acc, _ = O.render(scene, w, h, spp, bounces, frame_begin=b, offsets=off, uniforms=u, want_stats=False)
            acc[..., :3] = acc[..., :3] * f32((b + spp) / spp)
            frames[key] = dict(colour=acc, u=u, jitter=oracle_frame(O, scene, w, h, b, u, off), centre=centre_frame(O, dn, scene, w, h, b, u, off))
        fr = frames[key]
        if coverage is None:
            g, X = fr["jitter"]
            res = dn.reference_temporal(fr["colour"], g[0], g[1], X, hist, prev_vp, material_ids=mats, track=track, **params)
            F = None
        else:
            g, X, near_a = fr["centre"]
            res = dn.reference_temporal(fr["colour"], g[0], g[1], X, hist, prev_vp, material_ids=mats, track=track, coverage=coverage, near_parts=True, **params)
            nears.append((int(near_a.sum()), int((res[2][0] & ~_plain_near(dn, fr, hist, prev_vp, mats, track, params)).sum())))
            F = res[4]
        hist, iv = res[0], res[1]
        prev_vp = dn.temporal_view_proj(fr["u"])
    if F is None:
        rgb, _ = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], g[0], g[1], params=params, material_ids=mats)
    else:
        rgb, _ = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], F, g[1], params=params, material_ids=None)
    return rgb, fr["u"], res, g, nears


def _plain_near(dn, fr, hist, prev_vp, mats, track, params):
    """`near` of the same step without the coverage decision: what is left is cov against cov_min alone."""
    g, X, _ = fr["centre"]
    return dn.reference_temporal(fr["colour"], g[0], g[1], X, hist, prev_vp, material_ids=mats, track=track, near_parts=True, **params)[2][0]


def pixel_classes(dn, g, mats):
    """The issue's four classes on a frame's guides: misses and emitters; hits within 1 px of them; other pixels with a neighbour of another
    primitive; interiors."""
    from toyraygun_amd.denoise import _shift
    kept = (g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats)
    prim = np.ascontiguousarray(g[1, ..., 3]).view(np.int32)
    beside_kept, other = np.zeros_like(kept), np.zeros_like(kept)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            beside_kept |= _shift(kept, dx, dy, False)[0]
            q, ins = _shift(prim, dx, dy, 0)
            other |= ins & (q != prim)
    a = kept
    b = ~kept & beside_kept
    c = ~kept & ~beside_kept & other
    return [("misses and emitters", a), ("hits within 1 px of them", b), ("other pixels with a neighbour of another primitive", c), ("interiors", ~(a | b | c))]


def test_it_helps(O, cornell):
    """Cornell box 64 x 48, 3 bounces, default parameters, cov_min 0.9, rmse over the whole image against 512 spp at the last camera: the setting
    on at most 0.8 x the setting off on the sequences at rest 8 x 1 and turning 8 x 2, each with the variance of the mean off and on.  At rest
    after eight calls the mixed pixels number more than none and at most a quarter of the hits; `near` of the agreement and of cov against cov_min
    stay under 1 % in every call.  The squared error by pixel class is printed for both settings.
    MEASURED (this test, float64): see DESIGN.md, "Denoiser", *Pixel footprints*."""
    from toyraygun_amd import denoise as dn
    w, h, bounces = 64, 48, 3
    off = O.pixel_offsets(w, h)
    mats = cornell.buffers()["material_ids"]
    targets, ratios, frames = {}, {}, {}
    for name, calls, spp, degrees in SEQUENCES:
        for track in (False, True):
            rgb_off, u, _, _, _ = run_sequence(O, dn, cornell, w, h, bounces, calls, spp, degrees, track, None, frames)
            rgb_on, _, res, g, nears = run_sequence(O, dn, cornell, w, h, bounces, calls, spp, degrees, track, COV_MIN, frames)
            last = (calls - 1) * degrees
            if last not in targets:
                targets[last], _ = O.render(cornell, w, h, 512, bounces, offsets=off, uniforms=u, want_stats=False)
            e_off, e_on = _rmse(rgb_off, targets[last]), _rmse(rgb_on, targets[last])
            label = "%s, variance of the mean %s" % (name, "on" if track else "off")
            ratios[label] = e_on / e_off
            hits = int((res[4][..., 3] >= 0).sum() + res[3].sum())
            print("coverage it helps, %s: rmse against 512 spp off %.5f, on %.5f, ratio %.3f; mixed %d of %d hits; near (agreement, cov) per call %s" % (
                label, e_off, e_on, e_on / e_off, int(res[3].sum()), hits, nears))
            for na, nc in nears:
                assert na <= NEAR_CAP * w * h and nc <= NEAR_CAP * w * h, nears
            if degrees == 0.0:
                assert 0 < res[3].sum() <= 0.25 * hits, (int(res[3].sum()), hits)
            sq = lambda rgb: ((np.asarray(rgb, np.float64) - targets[last][..., :3].astype(np.float64)) ** 2).sum(-1)
            for setting, err in (("off", sq(rgb_off)), ("on", sq(rgb_on))):
                print("    squared error by pixel class, setting %s: %s" % (setting, "; ".join(
                    "%s %d px %.3f" % (cname, int(mask.sum()), err[mask].sum() / err.sum()) for cname, mask in pixel_classes(dn, g, mats))))
            # the same split by the JITTERED guides of the last call, which is how the setting-off step itself classifies (the issue's table)
            gj = frames[(tuple(np.round(orbit_eye(last), 9)), (calls - 1) * spp, spp)]["jitter"][0]
            print("    squared error by pixel class, setting off, classes from the last call's jittered guides: %s" % "; ".join(
                "%s %d px %.3f" % (cname, int(mask.sum()), sq(rgb_off)[mask].sum() / sq(rgb_off).sum()) for cname, mask in pixel_classes(dn, gj, mats)))
    for label, r in ratios.items():
        assert r <= HELPS_BOUND, (label, r)
