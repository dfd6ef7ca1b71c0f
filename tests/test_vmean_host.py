"""Host-side checks of the variance of the mean (include/trg_denoise.h, "A LONG HISTORY"; toyraygun_amd/denoise.py reference_temporal(track=True)):
the exported surface, off-is-off, that tracking touches the variance alone, the reference against a per-pixel loop written once more from the
header, the three consequences the header states on the Cornell guides, and -- on the oracle's renders, in float64 -- that the filter steered by
the tracked variance comes closer to a 512-spp render than the plain step on the four sequences of the issue.  No GPU.

THE BOUNDS.  Per-pixel loop: 1e-9 relative, two float64 evaluations that differ in summation order only, on the pixels whose discrete decisions
are not `near`.  Vc <= max(Vh, S): (1 - a)^2 + a^2 <= 1 for a in (0, 1]; 1e-12 relative for the rounding of two products and a sum.  The median
of Vc / S after 16 calls at rest with alpha = 0.01 (a = 1 / N throughout): the arithmetic-mean recursion gives 1 / 16 = 0.0625 where S is
constant; S is itself an estimate from N samples that moves from call to call, hence 0.15.  The rmse ratios: tracked below plain on all four,
at most 0.95 on the turning 8 x 2 sequence (the float64 prototype: 0.909)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.denoise_literal import CLAMP, _Guides, _lum
from tests.test_temporal_host import CAMERAS, camera_uniforms, oracle_frame, seeded_colour
from tests.test_temporal_synthetic_host import SCHEDULE, SHAPES_PARAMS, near_caps, schedule_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_denoise.h")
f32 = np.float32

NEW_SYMBOLS = {"trg_temporal_set_variance_of_mean", "trg_temporal_variance_of_mean"}
# (name, calls, spp, degrees the eye turns per call): the sequences of the issue's table at alpha = 0.2
SEQUENCES = [("turning 8 x 2", 8, 2, 1.0), ("at rest 8 x 1", 8, 1, 0.0), ("at rest 24 x 1", 24, 1, 0.0), ("turning 16 x 1", 16, 1, 1.0)]
TURNING_8x2_BOUND = 0.95


def orbit_eye(deg, eye=CAMERAS[0], at=(0.0, 1.0, -1.0)):
    """The eye turned by `deg` degrees about the vertical axis through the look-at point (the plugin's orbit=DEG)."""
    t = np.deg2rad(deg)
    dx, dz = eye[0] - at[0], eye[2] - at[2]
    return (at[0] + dx * np.cos(t) + dz * np.sin(t), eye[1], at[2] - dx * np.sin(t) + dz * np.cos(t))


def test_header_exports_and_python_agree_on_the_variance_of_mean_entry_points(built):
    from toyraygun_amd import capi, denoise
    declared = set(denoise.header_symbols(HEADER))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(denoise.SYMBOL_NAMES)
    assert sorted(denoise.SYMBOL_NAMES) == sorted(declared)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert [k for k, _ in denoise.TemporalParams._fields_] == list(denoise._TEMPORAL_DEFAULTS)      # trg_temporal_params keeps its layout
    assert [k for k, _ in denoise.TemporalParams._fields_] == ["iterations", "sigma_lum", "sigma_normal", "sigma_depth", "demodulate", "alpha", "alpha_moments",
                                                               "plane_tol", "normal_tol", "max_history"]
    text = open(HEADER).read()
    assert "NOT COVERED" in text and "feedback" in text and "0.02277" in text and "0.03414" in text    # the mixed figures of the prototype


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_off_is_off_and_track_only_touches_the_variance(cornell, dtype):
    """The synthetic schedule at 17 x 33.  track=False is the call without the argument, exactly, and its Hm.z is 0.  With track=True Hc, m1, m2,
    F, X and `near` are the plain step's exactly -- fed with the tracked chain's own history, whose Hm.z the plain step does not read -- and only
    Hm.z and iv.w differ; they are equal to each other, and they do differ from the plain V_0 once a history is four frames old."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = 17, 33
    hist, differed = None, 0
    for colour, g, X, vp, cam in schedule_frames(w, h, SCHEDULE):
        args = (colour, g[0], g[1], X, hist, vp)
        plain = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, **SHAPES_PARAMS)
        off = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, track=False, **SHAPES_PARAMS)
        on = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, track=True, **SHAPES_PARAMS)
        for a, b in zip(plain[:2] + plain[2], off[:2] + off[2]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert (off[0][1, ..., 2:] == 0).all()
        assert on[0].dtype == dtype and on[1].dtype == dtype
        assert np.array_equal(on[0][0], plain[0][0]) and np.array_equal(on[0][2:], plain[0][2:])          # Hc, F, X
        assert np.array_equal(on[0][1, ..., :2], plain[0][1, ..., :2]) and (on[0][1, ..., 3] == 0).all()   # m1, m2
        assert np.array_equal(on[1][..., :3], plain[1][..., :3])
        assert np.array_equal(on[2][0], plain[2][0]) and np.array_equal(on[2][1], plain[2][1])            # near, near_n
        assert np.array_equal(on[0][1, ..., 2], on[1][..., 3])                                             # Hm.z = V_0 = Vc
        N = on[0][0, ..., 3]
        short = N < 4
        assert np.array_equal(on[1][..., 3][short], plain[1][..., 3][short])                              # below four frames: S
        differed += int((on[1][..., 3] != plain[1][..., 3]).sum())
        hist = on[0]
    assert differed > 0


def _literal_vc(colour, g0, g1, X, hist, vp, mats, q):
    """Vc of the header for every pixel, one pixel and one tap at a time in Python floats, with what it needs of the step: the reprojection's
    valid taps, Nh, m1h, m2h and Vh, N, a, the moments, S in both forms.  hist: the previous call's four planes or None.
    Returns (Vc [h, w], N [h, w])."""
    G_ = _Guides(g0, g1, mats)
    h, w = G_.h, G_.w
    col = np.asarray(colour, np.float32).tolist()
    Xl = np.asarray(X, np.float32).tolist()
    alpha, alpha_m, ptol, ntol = (float(f32(q[k])) for k in ("alpha", "alpha_moments", "plane_tol", "normal_tol"))
    sn, sd, maxh = float(f32(q["sigma_normal"])), float(f32(q["sigma_depth"])), float(int(q["max_history"]))
    m = None if vp is None else [float(v) for v in np.asarray(vp, np.float32).reshape(16)]
    H = None if hist is None else [np.asarray(p, np.float32).tolist() for p in hist]          # (a history is fp32 planes, as the device holds them)

    def unit(v):
        ln = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return (None if not ln > 0 else (v[0] / ln, v[1] / ln, v[2] / ln))
    N = [[0.0] * w for _ in range(h)]
    a_ = [[1.0] * w for _ in range(h)]
    m1 = [[0.0] * w for _ in range(h)]
    m2 = [[0.0] * w for _ in range(h)]
    Vh = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            if G_.miss[y][x]:
                continue
            D = [col[y][x][k] / G_.a[y][x][k] if q["demodulate"] else col[y][x][k] for k in range(3)]
            l = _lum(D)
            W = nh = s1 = s2 = sv = 0.0
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
                                sv += b * H[1][qy][qx][2]
            if W > 0:
                N[y][x] = min(nh / W + 1, maxh)
                a_[y][x] = max(alpha, 1 / N[y][x])
                am = max(alpha_m, 1 / N[y][x])
                m1[y][x] = s1 / W + am * (l - s1 / W)
                m2[y][x] = s2 / W + am * (l * l - s2 / W)
                Vh[y][x] = sv / W
            else:
                N[y][x], m1[y][x], m2[y][x] = 1.0, l, l * l
    Vc = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            if G_.miss[y][x]:
                continue
            if N[y][x] >= 4:
                S = max(0.0, m2[y][x] - m1[y][x] * m1[y][x])
            else:
                gs = M1 = M2 = 0.0
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        if G_.inside(x + dx, y + dy):
                            gq = G_.geometry(x, y, x + dx, y + dy, 1, dx, dy, sn, sd)
                            gs += gq; M1 += gq * m1[y + dy][x + dx]; M2 += gq * m2[y + dy][x + dx]
                S = max(0.0, M2 / gs - (M1 / gs) ** 2) * 4 / N[y][x] if gs > 0 else 0.0
            a = a_[y][x]
            Vc[y, x] = S if Vh[y][x] is None or N[y][x] < 4 else (1 - a) * (1 - a) * Vh[y][x] + a * a * S
    return Vc, np.array(N)


def test_reference_track_is_the_per_pixel_loop(cornell):
    """The synthetic schedule (moving cameras, rejected taps, N < 4 and N >= 4) at 17 x 33 with max_history = 6: Hm.z and iv.w of
    reference_temporal(track=True) against the loop above, fed with the reference's own previous history, to 1e-9 of the value's scale on every
    pixel whose decisions are not `near`; both forms of Vc are met."""
    from toyraygun_amd import denoise as dn
    assert CLAMP == float(f32(1e-3))
    mats = cornell.buffers()["material_ids"]
    w, h = 17, 33
    q = dict(dn._TEMPORAL_DEFAULTS, **SHAPES_PARAMS)
    hist, recursed, short = None, 0, 0
    for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, SCHEDULE)):
        new, iv, (near, near_n) = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, material_ids=mats, near_parts=True, track=True, **SHAPES_PARAMS)
        near_caps(near, near_n, call)
        want, N = _literal_vc(colour, g[0], g[1], X, hist, vp, mats, q)
        ok = ~near & ~near_n
        hit = new[2, ..., 3] >= 0
        assert np.abs(N - new[0, ..., 3])[ok].max() <= 1e-9
        err = np.abs(new[1, ..., 2] - want) / np.maximum(1.0, np.abs(want))
        assert err[ok].max() <= 1e-9, (call, float(err[ok].max()))
        assert np.array_equal(new[1, ..., 2], iv[..., 3]) and (want[~hit] == 0).all()
        recursed += int((ok & hit & (N >= 4)).sum())
        short += int((ok & hit & (N < 4)).sum())
        hist = new
    assert recursed > 100 and short > 100, (recursed, short)


def test_consequences_on_the_cornell_guides(O, cornell):
    """37 x 29, the oracle's guides, camera at rest.  A first call has Vc = S.  Every interior hit pixel with history has Vc <= max(Vh, S).  With
    alpha = 0.01, max_history = 64 and colours of constant per-pixel variance the median of Vc / S over the hit pixels falls from call to call
    from call 4 on and lies below 0.15 after 16 calls (S / N would be 0.0625)."""
    from toyraygun_amd import denoise as dn
    w, h = 37, 29
    mats = cornell.buffers()["material_ids"]
    u = camera_uniforms(O, w, h, 0)
    g, X = oracle_frame(O, cornell, w, h, 0, u, O.pixel_offsets(w, h))
    vp = dn.temporal_view_proj(u)
    kw = dict(material_ids=mats, alpha=0.01, alpha_moments=0.01, max_history=64)
    hist, medians = None, []
    interior = np.zeros((h, w), bool)
    interior[1:-1, 1:-1] = True
    for call in range(16):
        colour = seeded_colour(g, 900 + call)
        plain = dn.reference_temporal(colour, g[0], g[1], X, hist, None if hist is None else vp, **kw)
        new, iv, near = dn.reference_temporal(colour, g[0], g[1], X, hist, None if hist is None else vp, track=True, **kw)
        hit = new[2, ..., 3] >= 0
        S, Vc, N = plain[1][..., 3], new[1, ..., 2], new[0, ..., 3]
        if hist is None:
            assert np.array_equal(Vc, S) and (N[hit] == 1).all()
        else:
            # the camera is at rest: an interior hit reprojects onto itself, Vh is the previous Vc of the same pixel up to a rounding of fx
            with_hist = hit & interior & (N > 1.5)
            assert with_hist.sum() > 0.5 * hit.sum()
            # Vh by another road: the colour goes through the same taps, and with a zero sample I = (1 - a) Ih -- so a history whose red is
            # Vc' gives Vh = I.r / (1 - a), a = max(alpha, 1 / N) from N alone
            carrier = hist.copy()
            carrier[0, ..., 0] = hist[1, ..., 2]
            red = dn.reference_temporal(np.zeros_like(colour), g[0], g[1], X, carrier, vp, demodulate=0, **kw)[0][0, ..., 0]
            a = np.maximum(float(f32(0.01)), 1.0 / np.where(with_hist, N, 2.0))
            Vh = red / (1.0 - a)
            assert (Vc <= np.maximum(Vh, S) * (1 + 1e-12))[with_hist].all()
            tracked_form = with_hist & (N >= 4)
            assert not tracked_form.any() or np.abs(Vc - ((1 - a) * (1 - a) * Vh + a * a * S))[tracked_form].max() <= 1e-12 * max(1.0, float(Vc.max()))
        if call >= 3:
            sel = hit & (N >= 4) & (S > 0)
            medians.append(float(np.median((Vc / np.where(S > 0, S, 1.0))[sel])))
        hist = new
    print("vmean consequences: median Vc / S over the hit pixels, calls 4 .. 16: %s" % " ".join("%.4f" % v for v in medians))
    assert all(b < a for a, b in zip(medians, medians[1:])), medians
    assert medians[-1] < 0.15, medians[-1]


# ---- it helps: the oracle's renders, float64 ---------------------------------------------------------------------------------------------------
def _rmse(a, ref):
    return float(np.sqrt(((np.asarray(a, np.float64)[..., :3] - np.asarray(ref, np.float64)[..., :3]) ** 2).mean()))


def run_sequence(O, dn, scene, w, h, bounces, calls, spp, degrees, track, frames, **params):
    """The last output of `calls` temporal steps of `spp` samples each on the oracle's renders, float64: frame_begin = k * spp, the colour scaled
    by (b + n) / n to the mean of its samples, the eye turned by k * degrees, default offsets; only the last call is filtered (the history holds
    unfiltered values).  frames: a cache {(eye, frame_begin, spp): (colour, guides, X, uniforms)} shared between the two settings."""
    mats = scene.buffers()["material_ids"]
    off = O.pixel_offsets(w, h)
    hist, prev_vp = None, None
    for k in range(calls):
        eye = orbit_eye(k * degrees)
        key = (tuple(np.round(eye, 9)), k * spp, spp)
        if key not in frames:
            u = O.make_uniforms(w, h, 0, eye=eye)
            b = k * spp
            acc, _ = O.render(scene, w, h, spp, bounces, frame_begin=b, offsets=off, uniforms=u, want_stats=False)
            acc[..., :3] = acc[..., :3] * f32((b + spp) / spp)
            frames[key] = (acc,) + oracle_frame(O, scene, w, h, b, u, off) + (u,)
        colour, g, X, u = frames[key]
        hist, iv, _ = dn.reference_temporal(colour, g[0], g[1], X, hist, prev_vp, material_ids=mats, track=track, **params)
        prev_vp = dn.temporal_view_proj(u)
    rgb, _ = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], g[0], g[1], params=params, material_ids=mats)
    return rgb, u


def test_it_helps(O, cornell):
    """Cornell box 64 x 48, 3 bounces, default parameters (alpha = 0.2, five iterations), rmse over the whole image against 512 spp at the last
    camera: tracked below plain on the four sequences, at most 0.95 x plain on the eye turning 1 degree per call over 8 calls of 2 spp.
    MEASURED (this test, float64): see DESIGN.md, "Denoiser", *Variance of the mean*."""
    from toyraygun_amd import denoise as dn
    w, h, bounces = 64, 48, 3
    off = O.pixel_offsets(w, h)
    targets, ratios = {}, {}
    frames = {}                                                 # (the sequences at rest share their first eight frames)
    for name, calls, spp, degrees in SEQUENCES:
        out = {}
        for track in (False, True):
            out[track], u = run_sequence(O, dn, cornell, w, h, bounces, calls, spp, degrees, track, frames)
        last = (calls - 1) * degrees
        if last not in targets:
            targets[last], _ = O.render(cornell, w, h, 512, bounces, offsets=off, uniforms=u, want_stats=False)
        plain, tracked = _rmse(out[False], targets[last]), _rmse(out[True], targets[last])
        ratios[name] = tracked / plain
        print("vmean it helps, %s: rmse against 512 spp plain %.5f, tracked %.5f, ratio %.3f" % (name, plain, tracked, tracked / plain))
    for name, r in ratios.items():
        assert r < 1.0, (name, r)
    assert ratios["turning 8 x 2"] <= TURNING_8x2_BOUND, ratios["turning 8 x 2"]
