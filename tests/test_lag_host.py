"""Host-side checks of the gated lag correction (include/trg_denoise.h, "CHANGING LIGHT"; toyraygun_amd/denoise.py reference_lag and
reference_temporal(lag=...)): the exported surface, the three consequences the header states, the reference against a per-pixel loop written
once more from the header, and the CHANGED SCHEDULE that tests/test_gpu_lag.py runs on the device -- the synthetic schedule of
tests/test_temporal_synthetic_host.py with the colours of every call from its middle on multiplied by 0.25 -- on the float64 reference alone:
it reaches what it is meant to reach.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests.denoise_literal import CLAMP, _Guides
from tests.test_temporal_host import camera_uniforms, oracle_frame, seeded_colour
from tests.test_temporal_synthetic_host import SCHEDULE, SHAPES, SHAPES_PARAMS, near_caps, schedule_frames, stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_denoise.h")
f32 = np.float32

NEW_SYMBOLS = {"trg_temporal_set_lag_correction", "trg_temporal_lag_correction", "trg_temporal_lag_correct_host"}
GATES = (0.0, 3.0, 30.0)
CHANGE_CALL = len(SCHEDULE) // 2              # call 4: camera at rest, the history four frames old
CHANGE_FACTOR = 0.25
# The share of the hit pixels the correction at gate 3 changes in a call of the UNCHANGED schedule (colours: independent uniform noise in [0, 4]
# times the albedo per call), float64 reference, images of at least 255 pixels.  Measured in this very test: at most 0.140 (15 x 17, call 4;
# 0.119 at 16 x 16, 0.116 at 17 x 33, 0.061 at 32 x 16, 0.058 at 48 x 32).  The stage interleaves its two planes in blocks of 3 x 2 pixels, so
# a window holds a dozen taps and its standard error is itself an estimate from a dozen samples: three of them are passed far more often than
# by a normal variable.  The cap is the worst figure with a margin of a quarter on top.
AT_REST_CAP = 0.175


def changed_frames(w, h, factor=CHANGE_FACTOR):
    """schedule_frames(SCHEDULE) with colour.rgb of the calls CHANGE_CALL .. multiplied by `factor` (one fp32 multiply): the light changed."""
    frames = []
    for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, SCHEDULE)):
        if call >= CHANGE_CALL and factor != 1.0:
            colour = colour.copy()
            colour[..., :3] = colour[..., :3] * f32(factor)
        frames.append((colour, g, X, vp, cam))
    return frames


def test_header_exports_and_python_agree_on_the_lag_entry_points(built):
    from toyraygun_amd import capi, denoise
    declared = set(denoise.header_symbols(HEADER))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(denoise.SYMBOL_NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    text = open(HEADER).read()
    assert re.search(r"#define\s+TRG_TEMPORAL_LAG_GATE_DEFAULT\s+3\.0f", text) and denoise.LAG_GATE_DEFAULT == 3.0
    assert "only `alpha` forgets it" not in text
    assert [k for k, _ in denoise.TemporalParams._fields_] == list(denoise._TEMPORAL_DEFAULTS)      # trg_temporal_params keeps its layout


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_lag_none_is_the_plain_step_and_the_rest_is_never_corrected(cornell, dtype):
    """reference_temporal(lag=None) is reference_temporal without the argument, exactly, over the changed schedule at 17 x 33; with a gate the
    moments, N, F, X, V_0 and `near` are still the plain step's exactly, and only colour moves."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = 17, 33
    hist, moved = None, 0
    for colour, g, X, vp, cam in changed_frames(w, h):
        args = (colour, g[0], g[1], X, hist, vp)
        plain = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, **SHAPES_PARAMS)
        none = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, lag=None, **SHAPES_PARAMS)
        on = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, near_parts=True, lag=3.0, **SHAPES_PARAMS)
        for a, b in zip(plain[:2] + plain[2], none[:2] + none[2]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert on[0].dtype == dtype and on[1].dtype == dtype
        assert np.array_equal(on[0][1:], plain[0][1:]) and np.array_equal(on[0][0, ..., 3], plain[0][0, ..., 3]) and np.array_equal(on[1][..., 3], plain[1][..., 3])
        assert np.array_equal(on[2][0], plain[2][0]) and np.array_equal(on[2][1], plain[2][1])
        assert np.array_equal(on[1][..., :3], on[0][0, ..., :3])                                         # (I, V_0) carries the history's colour
        moved += int((on[0][0, ..., :3] != plain[0][0, ..., :3]).any(-1).sum())
        hist = plain[0]
    assert moved > 0


def test_consequences_on_the_cornell_guides(O, cornell):
    """37 x 29, the oracle's guides, camera at rest.  1: a first call (noise, demodulated) and a second call of the same constant colour are
    bit for bit the uncorrected step's, at every gate.  2: constant c0 then c1: wherever every tap of the window found history (one history
    length, so one I), Ic = c1 within 1e-5 at every gate; and without the correction those pixels sit at c0 + 0.5 (c1 - c0)."""
    from toyraygun_amd import denoise as dn
    w, h = 37, 29
    mats = cornell.buffers()["material_ids"]
    u = camera_uniforms(O, w, h, 0)
    g, X = oracle_frame(O, cornell, w, h, 0, u, O.pixel_offsets(w, h))
    vp = dn.temporal_view_proj(u)
    noise = seeded_colour(g, 7)
    c0, c1 = np.full((h, w, 4), 0.25, f32), np.full((h, w, 4), 1.0, f32)
    for dtype in (np.float64, np.float32):
        first = dn.reference_temporal(noise, g[0], g[1], X, None, None, material_ids=mats, dtype=dtype)
        h0 = dn.reference_temporal(c0, g[0], g[1], X, None, None, material_ids=mats, demodulate=0, dtype=dtype)[0]
        same = dn.reference_temporal(c0, g[0], g[1], X, h0, vp, material_ids=mats, demodulate=0, dtype=dtype)
        plain = dn.reference_temporal(c1, g[0], g[1], X, h0, vp, material_ids=mats, demodulate=0, dtype=dtype)[0]
        F = plain[2]
        hit = F[..., 3] >= 0
        N = plain[0, ..., 3]
        support = dn.geometry_weights(F.astype(np.float64), 1, 128.0, 1.0, kernel=(1.0,) * 7) > 0
        fresh = np.zeros((h, w))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                fresh += support[dy + 3, dx + 3] & dn._shift(N < 1.5, dx, dy, False)[0]
        whole = hit & (N > 1.5) & (fresh == 0) & support[3, 3]
        assert whole.sum() > 0.5 * hit.sum()
        assert np.abs(plain[0][whole][:, :3] - 0.625).max() < 1e-5
        for gate in GATES:
            for args, want in (((noise, g[0], g[1], X, None, None), first), ((c0, g[0], g[1], X, h0, vp), same)):
                kw = {} if want is first else dict(demodulate=0)
                got = dn.reference_temporal(*args, material_ids=mats, dtype=dtype, lag=gate, **kw)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                assert not dn.reference_lag(args[0], g[0], g[1], want[0][0], gate, material_ids=mats, dtype=dtype, **kw)[1].any()
            new = dn.reference_temporal(c1, g[0], g[1], X, h0, vp, material_ids=mats, demodulate=0, dtype=dtype, lag=gate)[0]
            err = float(np.abs(new[0][whole][:, :3] - 1.0).max())
            print("lag consequences %s gate %g: %d of %d hits with a whole window, worst |Ic - c1| %.2e" % (dtype.__name__, gate, whole.sum(), hit.sum(), err))
            assert err <= 1e-5
            assert np.array_equal(new[0, ..., 3], N) and np.array_equal(new[1:], plain[1:])


def _literal_lag(color, g0, g1, hc, gate, sigma_normal, sigma_depth, demodulate, material_ids):
    """The header's definition one pixel and one tap at a time in Python floats; the guides' reading is tests/denoise_literal.py's."""
    G_ = _Guides(g0, g1, material_ids)
    col, I = np.asarray(color, np.float32).tolist(), np.asarray(hc, np.float32).tolist()
    sn, sd, gate = float(f32(sigma_normal)), float(f32(sigma_depth)), float(f32(gate))
    h, w = G_.h, G_.w

    def D(x, y, k):
        return col[y][x][k] / G_.a[y][x][k] if demodulate and not G_.miss[y][x] else col[y][x][k]
    out = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            out[y, x] = I[y][x][:3]
            if G_.miss[y][x]:
                continue
            taps = [(x + dx, y + dy, G_.geometry(x, y, x + dx, y + dy, 1, dx, dy, sn, sd)) for dy in range(-3, 4) for dx in range(-3, 4) if G_.inside(x + dx, y + dy)]
            G, G2 = sum(t[2] for t in taps), sum(t[2] * t[2] for t in taps)
            if not G > 0:
                continue
            for k in range(3):
                d = sum(gq * (D(qx, qy, k) - I[qy][qx][k]) for qx, qy, gq in taps) / G
                A1 = sum(gq * (D(qx, qy, k) - D(x, y, k)) for qx, qy, gq in taps)
                A2 = sum(gq * (D(qx, qy, k) - D(x, y, k)) ** 2 for qx, qy, gq in taps)
                se = math.sqrt(max(0.0, A2 / G - (A1 / G) ** 2) * G2) / G
                m = abs(d) - gate * se
                if m > 0:
                    out[y, x, k] = max(I[y][x][k] + math.copysign(m, d), min(I[y][x][k], 0.0))
    return out


@pytest.mark.parametrize("demodulate", [1, 0])
@pytest.mark.parametrize("gate", GATES)
def test_reference_lag_is_the_per_pixel_loop(cornell, gate, demodulate):
    """5 x 3 and 9 x 7, the synthetic stage (misses, an emitter, zero normals, albedo under the clamp, two planes), I = D of another noise
    blended with this one: reference_lag against the loop above to 1e-11 of the value's scale, and the mask is where it differs from I."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    assert CLAMP == float(f32(1e-3))
    changed = 0
    for w, h in ((5, 3), (9, 7)):
        g, X = stage(w, h, 1)
        colour, other = seeded_colour(g, 31), seeded_colour(g, 32)
        hc = np.zeros((h, w, 4), f32)
        hc[..., :3] = (0.3 * colour[..., :3] + 0.7 * 1.8 * other[..., :3]) / (np.maximum(g[1, ..., :3], f32(1e-3)) if demodulate else 1.0)
        hc[..., 3] = 3.0
        kw = dict(sigma_normal=128.0, sigma_depth=1.0, demodulate=demodulate)
        Ic, mask = dn.reference_lag(colour, g[0], g[1], hc, gate, material_ids=mats, **kw)
        want = _literal_lag(colour, g[0], g[1], hc, gate, 128.0, 1.0, demodulate, mats)
        assert np.abs(Ic - want).max() <= 1e-11 * max(1.0, float(np.abs(want).max()))
        assert np.array_equal(mask, (Ic != hc[..., :3].astype(np.float64)).any(-1))
        miss = (g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats)
        assert not mask[miss].any()
        changed += int(mask.sum())
    assert changed > 0 or gate >= 30.0                                          # (thirty standard errors: this noise never gets there)


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_changed_schedule_reaches_its_populations(cornell, size):
    """The float64 reference chained through the changed schedule (x 0.25 from call 4 on) and the unchanged one, max_history = 6, gate 3, at the
    nine shapes: `near` and `near_n` under the existing caps in every call with the correction on; on images of at least 255 pixels the
    correction changes at least half of the hit pixels in the call of the change, brings the mean colour of the changed pixels nearer to this
    call's samples' than the uncorrected step does, and on the unchanged schedule changes at most AT_REST_CAP of the hits in any call."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = size
    shares = {}
    for name, factor in (("changed", CHANGE_FACTOR), ("at rest", 1.0)):
        hist, shares[name] = None, []
        for call, (colour, g, X, vp, cam) in enumerate(changed_frames(w, h, factor)):
            args = (colour, g[0], g[1], X, hist, vp)
            new, iv, (near, near_n) = dn.reference_temporal(*args, material_ids=mats, near_parts=True, lag=3.0, **SHAPES_PARAMS)
            plain = dn.reference_temporal(*args, material_ids=mats, **SHAPES_PARAMS)[0]
            near_caps(near, near_n, call)
            hit = new[2, ..., 3] >= 0
            Ic, mask = dn.reference_lag(colour, g[0], g[1], plain[0], 3.0, material_ids=mats, **SHAPES_PARAMS)
            assert np.array_equal(Ic, new[0, ..., :3])
            shares[name].append(float(mask[hit].mean()) if hit.any() else 0.0)
            if name == "changed" and call == CHANGE_CALL and w * h >= 255:
                D = colour[..., :3].astype(np.float64) / np.maximum(g[1, ..., :3].astype(np.float64), float(f32(1e-3)))
                m = mask & hit
                off = abs(float((plain[0, ..., :3][m] - D[m]).mean()))
                on = abs(float((new[0, ..., :3][m] - D[m]).mean()))
                print("lag %dx%d: mean colour against the samples' in the call of the change: off %.4f, on %.4f" % (w, h, off, on))
                assert on < 0.25 * off
            hist = new
    print("lag %dx%d: share of the hits changed per call: changed schedule %s; at rest %s" % (
        w, h, " ".join("%.3f" % s for s in shares["changed"]), " ".join("%.3f" % s for s in shares["at rest"])))
    assert shares["changed"][0] == 0 and shares["at rest"][0] == 0                                              # no history: D = I
    if w * h >= 255:
        assert shares["changed"][CHANGE_CALL] >= 0.5
        assert max(shares["at rest"]) <= AT_REST_CAP
