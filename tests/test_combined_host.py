"""Host-side checks of the temporal step's four settings TOGETHER (include/trg_denoise.h: MOVING GEOMETRY, CHANGING LIGHT, A LONG HISTORY, PIXEL
FOOTPRINTS; toyraygun_amd/denoise.py reference_temporal(motion=, lag=, track=, coverage=)): the COMBINED SCHEDULE that tests/test_gpu_combined.py
runs on the device, on the float64 reference alone -- under every one of the 16 subsets of {motion, lag, track, cover} it stays under the caps on
undecidable pixels and reaches the populations that only exist in combination --, and a second reading of the combination: one step with all
four settings written once more from the header, one pixel and one tap at a time, against the reference, with the rules that hold between the
settings asserted from the reference's own outputs.  No GPU.

THE COMBINED SCHEDULE (combined_frames; eight calls on the moving stage of tests/test_motion_host.py, (gp, Xp) its previous pose, (g, X, m) its
current pose and motion planes):
    call  guides, X   previous camera   motion            colour
    0     gp, Xp      none              -                 seed 900
    1     gp, Xp      rest              -                 901
    2     gp, Xp      sub               -                 902
    3     gp, Xp      rest              -                 903            (the history turns four frames old: TURNS_FOUR)
    4     gp, Xp      rest              -                 904
    5     g, X        sub               m (rigid motion)  905            (the raised plane finds its history through m alone)
    6     g, X        rest              -                 906 x 0.25     (the light changed: rgb x 0.25 in fp32 from here on)
    7     g, X        border            identity planes   907 x 0.25
X.w of call k is seeded_agreement(guides, AGREEMENT_SEED + k, zeros=0.08); the parameters are SHAPES_PARAMS (max_history 6), the gate 3.0, cov_min 0.7.  It
stops at call 7 on purpose: the pixels that lose their history at call 5 reach N = 4 at call 8, a second call in which N against 4 is undecidable.
cov_min 0.5 would put the pixels of N = 2 exactly on the threshold, and the parameter set "low" brings 66 undecidable pixels at 48 x 32: neither is
used.  AGREEMENT_SEED is 64 and not the 60 the schedule was first drawn with: under 60 the last call leaves 6 mixed pixels of 256 at 16 x 16 with
the motion planes on, under the 3 % this file asks for; the seed moved, the bound did not.

THE BOUNDS.  `near`, `near_n`: near_caps of tests/test_temporal_synthetic_host.py as it stands.  Unresolved V_0 (tests/test_gpu_coverage.py's rule):
at most 2 % of the pixels of a schedule.  Mixed pixels: 3 % .. 50 % of the pixels of every call with the coverage history on (a plane A of 8 %
zeros blended at the moments' rate under cov_min 0.7 leaves between a twentieth and a seventh of the pixels below it).  The per-pixel loop:
the tolerances of the three loops it extends -- 1e-9 absolute on cov, 1e-9 of max(1, |value|) on N, Vc and a mixed pixel's (I, V_0), 1e-11 of the
plane's scale on the corrected colour -- two float64 evaluations that differ in summation order only."""
import itertools
import math

import numpy as np
import pytest

from tests.denoise_literal import CLAMP, _Guides, _lum
from tests.test_coverage_host import seeded_agreement, with_agreement
from tests.test_gpu_coverage import _unresolved
from tests.test_motion_host import check_populations, identity_motion, motion_census, moving_stage
from tests.test_temporal_host import seeded_colour
from tests.test_temporal_synthetic_host import SHAPES_PARAMS, near_caps, previous_camera

f32 = np.float32

GATE, COMBINED_COV_MIN = 3.0, 0.7
CHANGE_CALL, CHANGE_FACTOR = 6, 0.25
MOVING_CALL = 5
ZEROS = 0.08
AGREEMENT_SEED = 64
SETTINGS = ("motion", "lag", "track", "cover")
SUBSETS = [dict(zip(SETTINGS, bits)) for bits in itertools.product((False, True), repeat=4)]
HOST_SHAPES = [(5, 3), (16, 16), (17, 33), (48, 32)]
LITERAL_SHAPES = [(9, 7), (15, 17)]
LITERAL_CALLS = (0, 4, 5, 7)
UNRESOLVED_CAP = 0.02
MIXED_SHARE = (0.03, 0.50)
#              guides, previous camera, motion
_CALLS = [("prev", None, None), ("prev", "rest", None), ("prev", "sub", None), ("prev", "rest", None), ("prev", "rest", None),
          ("now", "sub", "rigid"), ("now", "rest", None), ("now", "border", "identity")]


def subset_id(s):
    return "+".join(k for k in SETTINGS if s[k]) or "plain"


def combined_frames(w, h):
    """[(colour, guides, X with A in .w, prev_vp or None, the camera's name, motion planes or None)] of the eight calls."""
    gp, Xp, g, X, m = moving_stage(w, h)
    frames = []
    for k, (pose, cam, motion) in enumerate(_CALLS):
        gg, XX = (gp, Xp) if pose == "prev" else (g, X)
        colour = seeded_colour(gg, 900 + k)
        if k >= CHANGE_CALL:
            colour = colour.copy()
            colour[..., :3] = colour[..., :3] * f32(CHANGE_FACTOR)
        XA = with_agreement(XX, seeded_agreement(gg, AGREEMENT_SEED + k, zeros=ZEROS))
        planes = None if motion is None else (m if motion == "rigid" else identity_motion(gg, XX))
        frames.append((colour, gg, XA, previous_camera(w, h, cam), cam, planes))
    return frames


def reference_kwargs(subset, frame):
    """reference_temporal's keywords for this subset in this call (the motion planes only where the schedule has them)."""
    return dict(motion=frame[5] if subset["motion"] else None, lag=GATE if subset["lag"] else None, track=subset["track"],
                coverage=COMBINED_COV_MIN if subset["cover"] else None)


def combined_reference(dn, frame, prev, mats, params, subset, dtype=np.float64, **override):
    """One step of the reference under a subset, from the previous history planes `prev` (None: no history): a dict of new, iv, near, near_n, mixed and
    marked (the filter's G0: emitters and mixed pixels marked) -- the last two also with the coverage history off (nobody mixed)."""
    colour, g, X, vp = frame[:4]
    kw = dict(reference_kwargs(subset, frame), **override)
    res = dn.reference_temporal(colour, g[0], g[1], X, prev, None if prev is None else vp, material_ids=mats, near_parts=True, dtype=dtype, **kw, **params)
    new, iv, (near, near_n) = res[:3]
    mixed, marked = (res[3], res[4]) if len(res) == 5 else (np.zeros(near.shape, bool), new[2])
    return dict(new=new, iv=iv, near=near, near_n=near_n, mixed=mixed, marked=marked)


def _window(mask):
    """The pixels with a pixel of `mask` inside their 7 x 7 window."""
    from toyraygun_amd.denoise import _shift
    out = np.zeros_like(mask)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            out |= _shift(mask, dx, dy, False)[0]
    return out


# ---- the schedule --------------------------------------------------------------------------------------------------------------------------------
def test_the_schedule_is_what_the_table_says():
    w, h = 17, 33
    gp, Xp, g, X, m = moving_stage(w, h)
    frames = combined_frames(w, h)
    assert len(frames) == 8 and [f[4] for f in frames] == [None, "rest", "sub", "rest", "rest", "sub", "rest", "border"]
    for k, (colour, gg, XA, vp, cam, planes) in enumerate(frames):
        want_g, want_X = (gp, Xp) if k < MOVING_CALL else (g, X)
        assert np.array_equal(gg.view(np.uint32), want_g.view(np.uint32)) and np.array_equal(XA[..., :3], want_X[..., :3])    # (G1.w holds integer bits)
        assert np.array_equal(XA[..., 3], seeded_agreement(gg, AGREEMENT_SEED + k, zeros=ZEROS)) and 0.02 < (XA[..., 3] == 0).mean() < 0.16
        want_c = seeded_colour(gg, 900 + k)
        if k >= CHANGE_CALL:
            want_c[..., :3] = want_c[..., :3] * f32(0.25)
        assert np.array_equal(colour, want_c) and colour.dtype == f32
        assert (vp is None) == (k == 0)
    assert [f[5] is not None for f in frames] == [False] * 5 + [True, False, True]
    assert np.array_equal(frames[5][5], m) and np.array_equal(frames[7][5], identity_motion(g, X))
    assert len(SUBSETS) == 16 and sum(sum(s.values()) >= 2 for s in SUBSETS) == 11


@pytest.mark.parametrize("size", HOST_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("subset", SUBSETS, ids=subset_id)
def test_combined_schedule_stays_under_the_caps_and_reaches_its_populations(cornell, subset, size):
    """The float64 reference chained through the combined schedule under one subset of the settings: `near` and `near_n` under near_caps in every
    call; on images of at least 255 pixels the unresolved V_0 pixels under 2 % of the schedule's pixels, N < 4 and N >= 4 both met from call 3 on,
    and the populations of the settings that are on -- mixed pixels on 3 % .. 50 % of the pixels of every call and one of them inside the window of
    a hit that is not mixed; history found through the motion planes and not without them at call 5; both forms of Vc at call 5 (among the moved
    pixels when the motion planes are on); the lag correction changing a colour in every call from 2 on, at 48 x 32 from call 1 on."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = size
    big = w * h >= 255
    params = dict(SHAPES_PARAMS)
    frames = combined_frames(w, h)
    prev, unresolved, report = None, 0, []
    for call, frame in enumerate(frames):
        R = combined_reference(dn, frame, prev, mats, params, subset)
        near_caps(R["near"], R["near_n"], call)
        new, iv, mixed, marked = R["new"], R["iv"], R["mixed"], R["marked"]
        flat = _unresolved(dn, new, marked, mixed, params)
        unresolved += int(flat.sum())
        N, hit = new[0, ..., 3], new[2, ..., 3] >= 0
        moved_colours = 0
        if subset["lag"]:
            off = combined_reference(dn, frame, prev, mats, params, subset, lag=None)
            moved_colours = int((off["new"][0, ..., :3] != new[0, ..., :3]).any(-1).sum())
            # no history: D = I.  Call 1 has two samples and a = 1 / 2: d is half the difference of two window means and has to pass three standard
            # errors of one of them, which a window of a dozen taps does on a few pixels in a thousand -- asked of the image that has a thousand
            assert moved_colours == 0 if call == 0 else (moved_colours > 0 or not big or (call == 1 and w * h < 1024)), (call, moved_colours)
        report.append((int(R["near"].sum()), int(R["near_n"].sum()), int(flat.sum()), int(mixed.sum()), int((hit & (N >= 4)).sum()), int((hit & (N < 4)).sum()), moved_colours))
        if big:
            if call >= 3:
                assert (hit & (N >= 4)).any() and (hit & (N < 4)).any(), call
            if subset["cover"]:
                assert MIXED_SHARE[0] * w * h <= mixed.sum() <= MIXED_SHARE[1] * w * h, (call, int(mixed.sum()))
                assert (_window(mixed) & hit & ~mixed).any(), call
            if call == MOVING_CALL:
                have = N > 1
                recursed, short = hit & have & (N >= 4), hit & (N < 4)
                if subset["motion"]:
                    plain = combined_reference(dn, frame, prev, mats, params, subset, motion=None)
                    cen = motion_census(dn, [frames[call - 1][:5], frame[:4] + (frame[5],)], mats)
                    found = lambda n: np.where(n > 1, 2.0, 1.0)                       # check_populations reads "history found" as N == 2
                    check_populations(cen, found(N), found(plain["new"][0, ..., 3]), None)
                    recursed, short = recursed & cen["moved"], short & cen["moved"]
                if subset["track"]:
                    assert recursed.any() and short.any()
        prev = new
    print("combined %s %dx%d: per call (near, near_n, unresolved V_0, mixed, N >= 4, N < 4, colours the lag correction moved): %s" % (subset_id(subset), w, h, report))
    if big:
        assert unresolved <= UNRESOLVED_CAP * w * h * len(frames), unresolved


# ---- a second reading of the combination ------------------------------------------------------------------------------------------------------------
def _literal_all(colour, g0, g1, X, hist, vp, mats, q, motion, gate, cov_min):
    """One step with the four settings on, written from include/trg_denoise.h alone: one pixel and one tap at a time in Python floats.  hist: the
    previous call's four planes or None; motion: (M0, M1) or None (then X and the pixel's own normal, the step without the planes).
    Returns a dict of [h, w] planes: N, m1, m2, cov, Vc, Vh (None without history), have, mixed; and I, Ic, iv_rgb [h, w, 3]."""
    G_ = _Guides(g0, g1, mats)
    h, w = G_.h, G_.w
    col = np.asarray(colour, np.float32).tolist()
    Xl = np.asarray(X, np.float32).tolist()
    M = None if motion is None else np.asarray(motion, np.float32).tolist()
    alpha, alpha_m, ptol, ntol = (float(f32(q[k])) for k in ("alpha", "alpha_moments", "plane_tol", "normal_tol"))
    sn, sd, maxh = float(f32(q["sigma_normal"])), float(f32(q["sigma_depth"])), float(int(q["max_history"]))
    gate, cmin, demod = float(f32(gate)), float(f32(cov_min)), bool(q["demodulate"])
    m = None if vp is None else [float(v) for v in np.asarray(vp, np.float32).reshape(16)]
    H = None if hist is None else [np.asarray(p, np.float32).tolist() for p in hist]          # (a history is fp32 planes, as the device holds them)

    def unit(v):
        ln = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return (None if not ln > 0 else (v[0] / ln, v[1] / ln, v[2] / ln))
    grid = lambda fill: [[fill] * w for _ in range(h)]
    N, a_, m1, m2, cov, Vh, have, mixed = grid(0.0), grid(1.0), grid(0.0), grid(0.0), grid(0.0), grid(None), grid(False), grid(False)
    D, I = grid(None), grid(None)
    # Reproject and Accumulate (MOVING GEOMETRY's three substitutions; Vh and covh through the taps of m1h)
    for y in range(h):
        for x in range(w):
            c = col[y][x][:3]
            if G_.miss[y][x]:
                D[y][x] = I[y][x] = list(c)
                continue
            D[y][x] = [c[k] / G_.a[y][x][k] if demod else c[k] for k in range(3)]
            l = _lum(D[y][x])
            A = Xl[y][x][3]
            W = nh = s1 = s2 = sv = sc = 0.0
            sI = [0.0, 0.0, 0.0]
            P, n, known = (Xl[y][x], unit(G_.n[y][x]), True) if M is None else (M[0][y][x], unit(M[1][y][x]), M[0][y][x][3] > 0)
            if H is not None and known and n is not None:
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
                                sc += b * H[1][qy][qx][3]
                                for k in range(3):
                                    sI[k] += b * H[0][qy][qx][k]
            if W > 0:
                have[y][x] = True
                N[y][x] = min(nh / W + 1, maxh)
                a, am = max(alpha, 1 / N[y][x]), max(alpha_m, 1 / N[y][x])
                a_[y][x] = a
                I[y][x] = [sI[k] / W + a * (D[y][x][k] - sI[k] / W) for k in range(3)]
                m1[y][x], m2[y][x] = s1 / W + am * (l - s1 / W), s2 / W + am * (l * l - s2 / W)
                Vh[y][x] = sv / W
                cov[y][x] = sc / W + am * (A - sc / W)
            else:
                N[y][x], I[y][x], m1[y][x], m2[y][x], cov[y][x] = 1.0, list(D[y][x]), l, l * l, A
            mixed[y][x] = cov[y][x] < cmin
    # behind the reprojection a mixed pixel is a miss: the guide the lag correction and the spatial estimate see
    marked = np.array(g0, np.float32)
    marked[np.array(mixed), 3] = -1.0
    K_ = _Guides(marked, g1, mats)
    Ic, Vc, iv_rgb = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            Ic[y, x] = I[y][x]
            iv_rgb[y, x] = I[y][x]
            if G_.miss[y][x]:
                continue
            if mixed[y][x]:
                # its I is not corrected; (I, V_0).rgb is I remodulated; V_0 is the temporal form whatever N -- what the recursion gives with it
                iv_rgb[y, x] = [I[y][x][k] * G_.a[y][x][k] if demod else I[y][x][k] for k in range(3)]
                S = max(0.0, m2[y][x] - m1[y][x] * m1[y][x])
            else:
                taps = [(x + dx, y + dy, K_.geometry(x, y, x + dx, y + dy, 1, dx, dy, sn, sd)) for dy in range(-3, 4) for dx in range(-3, 4) if K_.inside(x + dx, y + dy)]
                G, G2 = sum(t[2] for t in taps), sum(t[2] * t[2] for t in taps)
                # CHANGING LIGHT, between Accumulate and Variance
                if G > 0:
                    for k in range(3):
                        d = sum(gq * (D[qy][qx][k] - I[qy][qx][k]) for qx, qy, gq in taps) / G
                        A1 = sum(gq * (D[qy][qx][k] - D[y][x][k]) for qx, qy, gq in taps)
                        A2 = sum(gq * (D[qy][qx][k] - D[y][x][k]) ** 2 for qx, qy, gq in taps)
                        se = math.sqrt(max(0.0, A2 / G - (A1 / G) ** 2) * G2) / G
                        mm = abs(d) - gate * se
                        if mm > 0:
                            Ic[y, x, k] = max(I[y][x][k] + math.copysign(mm, d), min(I[y][x][k], 0.0))
                    iv_rgb[y, x] = Ic[y, x]
                # Variance: S
                if N[y][x] >= 4:
                    S = max(0.0, m2[y][x] - m1[y][x] * m1[y][x])
                elif G > 0:
                    M1, M2 = sum(gq * m1[qy][qx] for qx, qy, gq in taps) / G, sum(gq * m2[qy][qx] for qx, qy, gq in taps) / G
                    S = max(0.0, M2 - M1 * M1) * 4 / N[y][x]
                else:
                    S = 0.0
            a = a_[y][x]
            Vc[y, x] = S if Vh[y][x] is None or N[y][x] < 4 else (1 - a) * (1 - a) * Vh[y][x] + a * a * S
    return dict(N=np.array(N), m1=np.array(m1), m2=np.array(m2), cov=np.array(cov), Vc=Vc, Vh=Vh, have=np.array(have), mixed=np.array(mixed),
                I=np.array(I, np.float64), Ic=Ic, iv_rgb=iv_rgb)


ALL_ON = dict(motion=True, lag=True, track=True, cover=True)


@pytest.mark.parametrize("demodulate", [1, 0])
@pytest.mark.parametrize("size", LITERAL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_with_everything_on_is_the_per_pixel_loop(cornell, size, demodulate):
    """Calls 0, 4, 5 and 7 of the combined schedule with all four settings on, each from the reference's own chained history:
    reference_temporal(motion=, lag=, track=True, coverage=) against the loop above on every pixel whose decisions are not `near` (Vc also not
    `near_n`), and the rules between the settings from the reference's outputs alone: a mixed pixel's Hc.rgb is the UNCORRECTED I, its iv.rgb that
    remodulated, it is nobody's tap in the lag sums (another sample under it moves no neighbour's colour or V_0), its Hm.z is the recursion's
    value from four frames on with history and the temporal form otherwise; and the lag correction leaves N, the moments, Vc and cov exactly as
    the same step without it has them."""
    from toyraygun_amd import denoise as dn
    assert CLAMP == float(f32(1e-3))
    mats = cornell.buffers()["material_ids"]
    w, h = size
    params = dict(SHAPES_PARAMS, demodulate=demodulate)
    q = dict(dn._TEMPORAL_DEFAULTS, **params)
    prev, seen = None, dict(mixed=0, corrected=0, recursed=0, short=0, mixed_recursed=0, mixed_short=0)
    for call, frame in enumerate(combined_frames(w, h)):
        R = combined_reference(dn, frame, prev, mats, params, ALL_ON)
        new, iv, mixed = R["new"], R["iv"], R["mixed"]
        if call in LITERAL_CALLS:
            colour, g, X, vp, cam, motion = frame
            L = _literal_all(colour, g[0], g[1], X, prev, vp, mats, q, motion, GATE, COMBINED_COV_MIN)
            ok = ~R["near"]
            okv = ok & ~R["near_n"]
            hit = new[2, ..., 3] >= 0
            assert okv.mean() > 0.9                                                                            # (the caps are the other test's, at its shapes)
            rel = lambda a, want: np.abs(a - want) / np.maximum(1.0, np.abs(want))
            assert np.abs(new[0, ..., 3] - L["N"])[ok].max() <= 1e-9, call
            assert rel(new[1, ..., 0], L["m1"])[ok].max() <= 1e-9 and rel(new[1, ..., 1], L["m2"])[ok].max() <= 1e-9, call
            assert np.abs(new[1, ..., 3] - L["cov"])[ok].max() <= 1e-9, call
            assert np.array_equal(mixed[ok], L["mixed"][ok]) and np.array_equal(R["marked"][..., 3] < 0, ~hit | mixed), call
            assert rel(new[1, ..., 2], L["Vc"])[okv].max() <= 1e-9, (call, float(rel(new[1, ..., 2], L["Vc"])[okv].max()))
            assert np.array_equal(new[1, ..., 2], iv[..., 3])
            scale = max(1.0, float(np.abs(L["Ic"]).max()))
            assert np.abs(new[0, ..., :3] - L["Ic"])[ok].max() <= 1e-11 * scale, (call, float(np.abs(new[0, ..., :3] - L["Ic"])[ok].max()))
            sel = ok & mixed
            assert not sel.any() or rel(iv[..., :3], L["iv_rgb"])[sel].max() <= 1e-9, call
            assert np.abs(iv[..., :3] - L["iv_rgb"])[ok & ~mixed].max() <= 1e-11 * scale, call
            # ---- the cross rules, from the reference's outputs
            off = combined_reference(dn, frame, prev, mats, params, ALL_ON, lag=None)
            alb = np.maximum(g[1, ..., :3].astype(np.float64), float(f32(1e-3)))
            assert np.array_equal(new[0, ..., :3][mixed], off["new"][0, ..., :3][mixed])                       # a mixed pixel is not corrected
            assert np.array_equal(iv[..., :3][mixed], (new[0, ..., :3] * alb if demodulate else new[0, ..., :3])[mixed])
            for k in (0, 1):                                                                                   # N, the moments, Vc, cov; V_0; the mask
                assert np.array_equal(new[k] if k else new[0, ..., 3], off["new"][k] if k else off["new"][0, ..., 3]), (call, k)
            assert np.array_equal(iv[..., 3], off["iv"][..., 3]) and np.array_equal(mixed, off["mixed"]) and np.array_equal(new[2:], off["new"][2:])
            # nobody's tap: another sample under every mixed pixel leaves every other pixel's colour and V_0 where they were
            other = colour.copy()
            other[..., :3][mixed] = other[..., :3][mixed] * f32(3.0) + f32(1.0)
            flipped = combined_reference(dn, (other,) + frame[1:], prev, mats, params, ALL_ON)
            assert np.array_equal(flipped["mixed"], mixed)
            assert np.array_equal(flipped["new"][0][~mixed], new[0][~mixed]) and np.array_equal(flipped["iv"][~mixed], iv[~mixed])
            assert not mixed.any() or not np.array_equal(flipped["new"][0][mixed], new[0][mixed])
            # a mixed pixel's Hm.z
            m1, m2, N = new[1, ..., 0], new[1, ..., 1], new[0, ..., 3]
            S = np.maximum(0.0, m2 - m1 * m1)
            rec = mixed & L["have"] & (N >= 4)
            assert np.array_equal(new[1, ..., 2][mixed & ~rec], S[mixed & ~rec])
            if (rec & okv).any():
                a = np.maximum(float(f32(q["alpha"])), 1.0 / np.where(rec, N, 1.0))
                Vh = np.array([[v if v is not None else 0.0 for v in row] for row in L["Vh"]])
                want = (1 - a) * (1 - a) * Vh + a * a * S
                assert rel(new[1, ..., 2], want)[rec & okv].max() <= 1e-9, call
            seen["mixed"] += int(sel.sum())
            seen["corrected"] += int((ok & (new[0, ..., :3] != off["new"][0, ..., :3]).any(-1)).sum())
            seen["recursed"] += int((okv & hit & L["have"] & (N >= 4)).sum())
            seen["short"] += int((okv & hit & (N < 4)).sum())
            seen["mixed_recursed"] += int((rec & okv).sum())
            seen["mixed_short"] += int((okv & mixed & ~rec).sum())
        prev = new
    print("combined literal %dx%d demodulate %d: compared %s" % (w, h, demodulate, seen))
    assert all(v > 0 for v in seen.values()), seen
