"""GPU tests (-m gpu) of the temporal step's four settings TOGETHER -- the previous-position planes, the gated lag correction, the variance of the
mean and the coverage history (include/trg_denoise.h; dn_temporal_reproject_kernel's eight forms [MOTION][TRACK][COVER], the lag launch behind it,
dn_temporal_spatial_kernel's TRACK form behind that): every subset of two and more settings on the combined schedule of
tests/test_combined_host.py against reference_temporal from the DEVICE's own previous history, the filter iterations behind the step with
everything on, trg_render_temporal armed with a previous scene against its own steps, the plugin's option string with all tokens and slide=, and
the three setters as independent state.

BARS.  Exactly those of tests/test_gpu_coverage.py (_cov_reference) with the coverage history on and of tests/test_gpu_temporal_shapes.py
(step_reference) with it off: E32 = the reference's float32 mode against its float64 mode on the same inputs under the same settings;
max(1e-4, 4 E32) on Hc.rgb, N, Hm (the moments, Vc, cov) and I, relative to max(1, |ref|_2); max(1e-3, 4 E32) relative + 1e-9 on V_0; only where
`near` is false, V_0 also outside `near_n` and -- with the coverage history on -- outside the unresolved pixels of tests/test_gpu_coverage.py's
docstring.  Nothing in a bar comes from the device.  (In call 3, where N turns four, the two precisions of the reference take different forms of Vc
on most pixels: with the variance of the mean on, E32 of Hm -- which holds Vc -- is of order 1 there and Hm's bar with it, as V_0's compared set
is nearly empty in that call; Hm.z is still iv.w bit for bit, and m1, m2 and cov, which do not know that setting, are in every call ALSO held to
the Hm bar of the same subset without it.)  The filter: the bars of tests/test_gpu_temporal.py::test_filter_chain_matches_the_reference.
Everything else is bit for bit.

MEASURED on an MI355X: see DESIGN.md, "Denoiser", *Settings together*."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests.test_combined_host import (ALL_ON, COMBINED_COV_MIN, GATE, SUBSETS, combined_frames, combined_reference, reference_kwargs, subset_id)
from tests.test_gpu_coverage import _cov_reference
from tests.test_gpu_denoise import _bits, _close
from tests.test_gpu_motion import _load, _slid_cornell, moved_box
from tests.test_gpu_temporal import _filter_g0
from tests.test_gpu_temporal_shapes import _ctx
from tests.test_temporal_synthetic_host import SHAPES_PARAMS, _max, _rel, near_caps, step_ratios, step_reference
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = ("Hc.rgb", "N", "Hm", "I", "V_0")
UNSEEN = [s for s in SUBSETS if sum(s.values()) >= 2]          # the eleven subsets no other file compares with the reference
SIZES = [(5, 3), (17, 33), (48, 32)]                           # a pixel row under a tile; ragged over several tiles; full tiles with a ragged edge


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


def _configure(dn, c, subset, lag=None):
    """The three setters for a subset (the motion planes travel with the calls); lag: another gate than the subset's (False: off)."""
    gate = (GATE if subset["lag"] else None) if lag is None else (None if lag is False else lag)
    if gate is not None:
        dn.temporal_set_lag_correction(c, gate)
    if subset["track"]:
        dn.temporal_set_variance_of_mean(c, True)
    if subset["cover"]:
        dn.temporal_set_coverage(c, COMBINED_COV_MIN)


def _step(dn, c, mats, frame, subset, params):
    """One call on the device: (out, iv, the new history planes as the next call's reference reads them)."""
    colour, g, X, vp, cam, motion = frame
    out, iv = dn.temporal_denoise(c, colour, g, X, vp, return_iv=True, motion=motion if subset["motion"] else None, **params)[:2]
    hist = dn.temporal_history(c)
    return out, iv, np.stack([hist[0], hist[1], _filter_g0(dn, g, mats), X])


_refs = {}


def _ref(dn, subset, size, call, frame, prev, mats, params):
    """The reference of one call of one subset, its compared pixels and its bars, computed once for both build settings -- as long as both hand it
    the same previous history, bit for bit.  _cov_reference with the coverage history on, step_reference with it off, each as it stands: the
    other settings travel to reference_temporal in the parameter dict."""
    key = (subset_id(subset), size, call, params.get("demodulate", 1), hashlib.sha1(b"" if prev is None else np.ascontiguousarray(prev).tobytes()).hexdigest())
    if key not in _refs:
        kw = reference_kwargs(subset, frame)
        cov_min = kw.pop("coverage")
        q = dict(params, **kw)
        if cov_min is None:
            R = step_reference(dn, frame[:5], prev, mats, q)
            R.update(mixed=np.zeros(R["near"].shape, bool), marked=R["new"][2], flat=np.zeros(R["near"].shape, bool))
        else:
            R = _cov_reference(dn, frame[:5], prev, mats, q, cov_min)
        _refs[key] = R
    return _refs[key]


def _ratios(R, subset, planes, iv):
    """error / bar per plane on the compared pixels: Hc.rgb, N, Hm, I, V_0."""
    if not subset["cover"]:
        return step_ratios(R, planes[0], planes[1], iv)
    ok, okv, (bc, bn, bm, bi, bv) = R["ok"], R["okv"], R["bars"]
    new, v64 = R["new"], R["iv"][..., 3]
    return (_rel(planes[0][..., :3], new[0][..., :3])[ok] / bc, _rel(planes[0][..., 3:], new[0][..., 3:])[ok] / bn, _rel(planes[1], new[1])[ok] / bm,
            _rel(iv[..., :3], R["iv"][..., :3])[ok] / bi, (np.abs(np.asarray(iv[..., 3], np.float64) - v64) / (bv * np.abs(v64) + 1e-9))[okv])


def _identities(tag, call, subset, frame, planes, out, iv, demod):
    """What holds bit for bit on EVERY pixel, whatever the subset.  Returns the device's mixed mask."""
    colour, g = frame[0], frame[1]
    hit = planes[2, ..., 3] >= 0
    cov = planes[1][..., 3]
    mixed = hit & (cov < f32(COMBINED_COV_MIN)) if subset["cover"] else np.zeros(hit.shape, bool)
    alb = np.maximum(g[1, ..., :3], f32(1e-3))
    remod = lambda a: (a * alb).astype(f32) if demod else a
    # a mixed pixel: (I, V_0).rgb is its history colour remodulated, and the output copies that; any other pixel: (I, V_0).rgb is its history colour
    assert np.array_equal(_bits(iv[..., :3][mixed]), _bits(remod(planes[0][..., :3])[mixed])), (tag, call)
    assert np.array_equal(_bits(iv[..., :3][~mixed]), _bits(planes[0][..., :3][~mixed])), (tag, call)
    assert np.array_equal(_bits(out[..., :3][mixed]), _bits(iv[..., :3][mixed])), (tag, call)
    # the other hits: out = (I, V_0) remodulated; misses copy; alpha is the input's
    others = hit & ~mixed
    assert np.array_equal(_bits(out[..., :3][others]), _bits(remod(iv[..., :3])[others])), (tag, call)
    assert np.array_equal(_bits(out[~hit]), _bits(colour[~hit])) and np.array_equal(_bits(out[..., 3]), _bits(colour[..., 3])), (tag, call)
    assert (iv[..., 3][~hit] == 0).all() and (planes[0][..., 3][~hit] == 0).all() and (planes[1][~hit] == 0).all(), (tag, call)
    # Hm.z is Vc and what (I, V_0) carries -- or 0; Hm.w is cov in [0, 1] -- or 0
    if subset["track"]:
        assert np.array_equal(_bits(iv[..., 3]), _bits(planes[1][..., 2])), (tag, call)
    else:
        assert (planes[1][..., 2] == 0).all(), (tag, call)
    assert ((cov >= 0).all() and (cov <= 1).all()) if subset["cover"] else (cov == 0).all(), (tag, call)
    return mixed


def _run_subset(dn, capi, O, cornell, subset, size, strict, params):
    """The combined schedule under one subset on the device, every call from the device's own previous history.  Returns the worst err / bar per plane."""
    w, h = size
    demod = params.get("demodulate", 1)
    tag = "combined %s %dx%d strict %d%s" % (subset_id(subset), w, h, strict, "" if demod else " demodulate 0")
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    twin = _ctx(O, cornell, w, h, capi, strict)[0] if subset["lag"] else None            # the same subset without the lag correction
    try:
        _configure(dn, c, subset)
        if twin is not None:
            _configure(dn, twin, subset, lag=False)
        prev, worst = None, [0.0] * len(NAMES)
        n_mixed = n_flat = n_lt4 = n_ge4 = n_corrected = 0
        frames = combined_frames(w, h)
        for call, frame in enumerate(frames):
            out, iv, planes = _step(dn, c, mats, frame, subset, params)
            R = _ref(dn, subset, size, call, frame, prev, mats, params)
            near_caps(R["near"], R["near_n"], call)
            ratios = _ratios(R, subset, planes, iv)
            now = [_max(r) for r in ratios]
            worst = [max(a, b) for a, b in zip(worst, now)]
            print("%s call %d: near %d, near_n %d, unresolved V_0 %d, mixed %d of %d pixels; bars %s; worst err / bar: %s" % (
                tag, call, R["near"].sum(), R["near_n"].sum(), R["flat"].sum(), R["mixed"].sum(), R["near"].size, " ".join("%.1e" % b for b in R["bars"]),
                " ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, now))))
            for name, r in zip(NAMES, ratios):
                assert (r <= 1.0).all(), (tag, call, name, int((r > 1).sum()), float(r.max()))
            if subset["track"]:
                # the moments and cov do not know the variance of the mean: they are also held to the bar of the same subset without it, whose Hm has
                # no Vc in it (this is what compares them in call 3)
                S = _ref(dn, dict(subset, track=False), size, call, frame, prev, mats, params)
                r = _rel(planes[1][..., [0, 1, 3]], S["new"][1][..., [0, 1, 3]])[S["ok"]] / S["bars"][2]
                assert (r <= 1.0).all(), (tag, call, "m1, m2, cov", float(r.max()))
            mixed = _identities(tag, call, subset, frame, planes, out, iv, demod)
            assert np.array_equal(mixed[R["ok"]], R["mixed"][R["ok"]]), (tag, call)
            if twin is not None:
                _, iv2, planes2 = _step(dn, twin, mats, frame, subset, params)
                assert np.array_equal(_bits(planes[0][..., 3]), _bits(planes2[0][..., 3])) and np.array_equal(_bits(planes[1]), _bits(planes2[1])), (tag, call)
                assert np.array_equal(_bits(iv[..., 3]), _bits(iv2[..., 3])), (tag, call)
                # (the colours are each context's own chain: a mixed pixel is not corrected, but its history taps may have been)
                changed = (_bits(planes[0][..., :3]) != _bits(planes2[0][..., :3])).any(-1)
                assert not changed[planes[2, ..., 3] < 0].any(), (tag, call)                                  # a miss copies its sample either way
                n_corrected += int(changed.sum())
            N, hit = planes[0, ..., 3], planes[2, ..., 3] >= 0
            n_mixed += int((mixed & R["ok"]).sum())
            n_flat += int(R["flat"].sum())
            if call >= 3:
                n_lt4 += int((hit & (N < 4)).sum())
                n_ge4 += int((hit & (N >= 4)).sum())
            prev = planes
        print("%s: worst err / bar over the schedule: %s; compared mixed pixels %d, corrected colours %d" % (
            tag, " ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, worst)), n_mixed, n_corrected))
        if w * h >= 255:
            assert n_lt4 > 0 and n_ge4 > 0
            assert n_flat <= 0.02 * w * h * len(frames), n_flat
            assert n_mixed > 0.03 * w * h * len(frames) or not subset["cover"]
            assert n_corrected > 0 or not subset["lag"]
        return worst
    finally:
        _close(c, dn)
        if twin is not None:
            _close(twin, dn)


# ---------------------------------------------------------------------------------------------------------------------------- a. every unseen subset
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("subset", UNSEEN, ids=subset_id)
def test_every_unseen_subset_matches_the_reference(capi, dn, O, cornell, subset, size, strict):
    """The eleven subsets of {motion, lag, track, cover} with two and more settings on, the combined schedule (eight calls; the rigid motion at
    call 5, the light x 0.25 from call 6, identity planes at call 7; A of 8 % zeros, gate 3, cov_min 0.7, max_history 6, iterations 0): every call
    against reference_temporal under the same settings from the device's own previous history, under the module's bars; the mixed mask equal
    to the reference's outside `near`; and bit for bit on every pixel: the mixed pixels' identities, out = (I, V_0) remodulated on the other hits,
    misses copy, iv.w = Hm.z with the variance of the mean on, and -- with the lag correction on -- N, Hm and iv.w of a second context that runs
    the same subset without it (that a mixed pixel is not corrected and is nobody's tap shows in Hc.rgb against the reference)."""
    _run_subset(dn, capi, O, cornell, subset, size, strict, dict(SHAPES_PARAMS, iterations=0))


@pytest.mark.parametrize("strict", [1, 0])
def test_everything_on_without_demodulation(capi, dn, O, cornell, strict):
    """The schedule's one variant of the parameters, demodulate = 0 (no discrete decision moves), with all four settings on at 17 x 33."""
    _run_subset(dn, capi, O, cornell, ALL_ON, (17, 33), strict, dict(SHAPES_PARAMS, iterations=0, demodulate=0))


# ---------------------------------------------------------------------------------------------------------------------------- b. the filter behind it
@pytest.mark.parametrize("strict", [1, 0])
def test_filter_behind_the_step_with_everything_on(capi, dn, O, cornell, strict):
    """17 x 33, all four settings on, the combined schedule with two iterations in calls 4, 5 and 7: out and V_N against reference_atrous_variance fed
    with the device's own (I, V_0) -- the corrected colour and Vc -- and the reference's marked G0 (a `near` pixel takes the device's own decision),
    under the bars of test_filter_chain_matches_the_reference: |out - ref|_2 <= 1e-4 max(1, |ref|_2) over the four channels, |V - V_ref| <=
    1e-3 |V_ref| + 1e-9.  The mixed pixels copy bit for bit, the other hits are filtered."""
    w, h = 17, 33
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    try:
        _configure(dn, c, ALL_ON)
        prev = None
        for call, frame in enumerate(combined_frames(w, h)):
            colour, g, X, vp, cam, motion = frame
            it = 2 if call in (4, 5, 7) else 0
            out, iv, var = dn.temporal_denoise(c, colour, g, X, vp, motion=motion, return_iv=True, return_variance=True, **dict(SHAPES_PARAMS, iterations=it))
            hist = dn.temporal_history(c)
            planes = np.stack([hist[0], hist[1], _filter_g0(dn, g, mats), X])
            if it:
                R = combined_reference(dn, frame, prev, mats, dict(SHAPES_PARAMS), ALL_ON)
                hit = planes[2, ..., 3] >= 0
                mixed = hit & (planes[1][..., 3] < f32(COMBINED_COV_MIN))
                assert np.array_equal(mixed[~R["near"]], R["mixed"][~R["near"]]) and mixed.sum() > 0.03 * w * h, call
                marked = R["marked"].copy()
                marked[..., 3] = np.where(R["near"], np.where(mixed, -1.0, planes[2, ..., 3]), marked[..., 3])
                rgb, vref = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], marked, g[1], iterations=it, material_ids=None, **SHAPES_PARAMS)
                ref = np.concatenate([rgb, colour[..., 3:].astype(np.float64)], -1)
                err = np.sqrt(((out.astype(np.float64) - ref) ** 2).sum(-1))
                bar = 1e-4 * np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))
                verr, vbar = np.abs(var.astype(np.float64) - vref), 1e-3 * np.abs(vref) + 1e-9
                print("combined filter 17x33 strict %d call %d: worst err / bar %.3f, variance %.3f; mixed %d" % (
                    strict, call, float((err / bar).max()), float((verr / vbar).max()), mixed.sum()))
                # (the floor's normals are 1.2 long: w_n = 1.44^128 = 2e20, whose square fp32 does not hold -- the iterations scale their weights)
                assert np.isfinite(var).all() and np.isfinite(out).all(), (call, int((~np.isfinite(var)).sum()))
                assert (err <= bar).all(), (call, int((err > bar).sum()), float((err / bar).max()))
                assert (verr <= vbar).all(), (call, int((verr > vbar).sum()), float((verr / vbar).max()))
                assert np.array_equal(_bits(out[..., :3][mixed]), _bits(iv[..., :3][mixed])) and np.array_equal(_bits(var[mixed]), _bits(iv[..., 3][mixed]))
                assert np.array_equal(_bits(out[~hit]), _bits(colour[~hit]))
                alb = np.maximum(g[1, ..., :3], f32(1e-3))
                others = hit & ~mixed
                assert (_bits(out[..., :3][others]) != _bits((iv[..., :3] * alb).astype(f32))[others]).any(-1).mean() > 0.5      # and it did filter
            prev = planes
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- c. end to end
@pytest.mark.parametrize("strict", [1, 0])
def test_render_temporal_is_its_steps_with_everything_on(capi, dn, O, cornell, strict):
    """Cornell box 64 x 48, 2 spp, 3 bounces, four calls, the short box moved by 0.02 k before call k and trg_temporal_set_previous_scene before
    calls 1 .. 3; gate 3, the variance of the mean on, cov_min 0.9.  trg_render_temporal in one context; in a second one its steps by hand:
    trg_render into a zeroed image, the scaling to the mean, trg_guides_render_centre(_motion) under the step's two tolerances, and
    trg_temporal_denoise(_motion) against the previous camera.  The output and the history (Hc, Hm with Vc and cov) are equal bit for bit after
    every call.  A fifth call without a previous scene is the steps without motion planes: the arming was consumed."""
    import torch
    w, h, spp, bounces, calls = 64, 48, 2, 3, 4
    b = cornell.buffers()
    off = O.pixel_offsets(w, h)
    scenes = [moved_box(b, 0.02 * k) for k in range(calls)]
    whole, steps = (make_ctx(O, cornell, w, h, offsets=off) for _ in range(2))
    try:
        for c in (whole, steps):
            c.set_option(capi.OPT_STRICT, strict)
            dn.temporal_set_lag_correction(c, 3.0)
            dn.temporal_set_variance_of_mean(c, True)
            dn.temporal_set_coverage(c, 0.9)
        vp = dn.temporal_view_proj(O.make_uniforms(w, h))
        q = dn._TEMPORAL_DEFAULTS
        seen_motion = seen_mixed = 0
        for k in range(calls + 1):
            armed = 0 < k < calls
            if armed:
                for c in (whole, steps):
                    _load(c, scenes[k])
                    dn.temporal_set_previous_scene(c, scenes[k - 1]["positions"], None, b["indices"])
            first = k * spp
            got = dn.render_temporal(whole, first, spp, bounces)
            img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                                                                       # (the zeros are torch's stream's, the render the context's)
            steps.bind_accum(img.data_ptr())
            try:
                steps.render(first, spp, bounces)
                steps.sync()
            finally:
                steps.bind_accum(None)
            mean = img.cpu().numpy()
            mean[..., :3] = mean[..., :3] * f32(np.float64(first + spp) / np.float64(spp))
            if armed:
                g, X, m = dn.guides_centre(steps, first, q["plane_tol"], q["normal_tol"], with_motion=True)
                seen_motion += int((np.abs(m[0, ..., :3] - X[..., :3]).max(-1) > 0.01).sum())
            else:
                (g, X), m = dn.guides_centre(steps, first, q["plane_tol"], q["normal_tol"]), None
            want = dn.temporal_denoise(steps, mean, g, X, vp if k else None, motion=m)
            assert np.array_equal(_bits(got), _bits(want)), (k, int((_bits(got) != _bits(want)).sum()))
            ha, hb = dn.temporal_history(whole), dn.temporal_history(steps)
            assert np.array_equal(_bits(ha), _bits(hb)), (k, int((_bits(ha) != _bits(hb)).sum()))
            seen_mixed += int(((ha[0, ..., 3] > 0) & (ha[1, ..., 3] < f32(0.9))).sum())
            assert (ha[1, ..., 2] > 0).any() and (ha[1, ..., 3] > 0).any()
        assert seen_motion > 0 and seen_mixed > 0
        assert (ha[0, ..., 3] > 4).any()                                                                   # and the history went on growing
    finally:
        for c in (whole, steps):
            _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- d. plugin
def test_plugin_with_every_token_and_slide(capi, dn, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png denoise=5,temporal,lag,vmean,cover slide=0.02: the picture is trg_postprocess of what trg_load_scene +
    trg_temporal_set_previous_scene + trg_render_temporal give for the same calls with the three settings made (the default gate and cov_min);
    the order of the three tokens does not change it; and it is another picture than `,cover` alone gives under the same slide."""
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces, slide = 64, 48, 4, 3, 0.02

    def run(name, *extra):
        path = str(tmp_path / name)
        subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba()
    pic = run("all.png", "denoise=5,temporal,lag,vmean,cover", "slide=0.02")
    assert np.array_equal(run("order1.png", "denoise=5,temporal,cover,lag,vmean", "slide=0.02"), pic)
    assert np.array_equal(run("order2.png", "denoise=5,temporal,vmean,cover,lag", "slide=0.02"), pic)
    assert not np.array_equal(run("cover.png", "denoise=5,temporal,cover", "slide=0.02"), pic)
    scenes = [_slid_cornell(host, float(f32(k * slide))) for k in range(frames)]
    c = capi.Context(w, h)
    try:
        _load(c, scenes[0])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        dn.temporal_set_lag_correction(c, dn.LAG_GATE_DEFAULT)
        dn.temporal_set_variance_of_mean(c, True)
        dn.temporal_set_coverage(c, dn.COVERAGE_MIN_DEFAULT)
        den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        for k in range(frames):
            if k:
                _load(c, scenes[k])
                dn.temporal_set_previous_scene(c, scenes[k - 1]["positions"], scenes[k - 1]["normals"], scenes[k - 1]["indices"])
            dn.render_temporal(c, k, 1, bounces, out=den, iterations=5)
        c.sync()
        c.bind_accum(den.data_ptr())
        try:
            assert np.array_equal(c.postprocess(flip_y=True), pic)
        finally:
            c.bind_accum(None)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- e. independent state
@pytest.mark.parametrize("strict", [1, 0])
def test_the_settings_are_independent_state(capi, dn, O, cornell, strict):
    """17 x 33, two calls of the combined schedule with everything on, then per setter: repeating the current value keeps the history bit for bit;
    a change of the variance of the mean or of cov_min forgets it (trg_temporal_history_read refuses) and the calls that follow are those of a
    fresh context with the same final settings, bit for bit; every query still reports the other two settings.  The lag gate: the header gives
    its setter no reset -- a change KEEPS the history bit for bit, and the next call runs under the new gate from that history: N, Hm and iv.w of
    a context that kept the old gate, another colour."""
    w, h = 17, 33
    frames = combined_frames(w, h)
    params = dict(SHAPES_PARAMS, iterations=2)
    cov = float(f32(COMBINED_COV_MIN))

    def run(c, frame):
        colour, g, X, vp, cam, motion = frame
        return dn.temporal_denoise(c, colour, g, X, vp, motion=motion, return_iv=True, return_variance=True, **params) + (dn.temporal_history(c),)

    def same(a, b, what):
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(_bits(x), _bits(y)), (what, k)

    def started():
        c = _ctx(O, cornell, w, h, capi, strict)[0]
        _configure(dn, c, ALL_ON)
        for frame in frames[:2]:
            last = run(c, frame)
        return c, last

    def refuses(c):
        with pytest.raises(capi.TrgError) as e:
            dn.temporal_history(c)
        assert e.value.code == capi.ERR_INVALID

    def fresh(lag, track, cover):
        c = _ctx(O, cornell, w, h, capi, strict)[0]
        if lag is not None:
            dn.temporal_set_lag_correction(c, lag)
        dn.temporal_set_variance_of_mean(c, track)
        dn.temporal_set_coverage(c, cover)
        return c
    settings = lambda c: (dn.temporal_lag_correction(c), dn.temporal_variance_of_mean(c), dn.temporal_coverage(c))
    open_ctx = []
    try:
        # repeating each value keeps the history
        c, last = started()
        open_ctx.append(c)
        assert settings(c) == (GATE, True, cov)
        dn.temporal_set_lag_correction(c, GATE)
        dn.temporal_set_variance_of_mean(c, True)
        dn.temporal_set_coverage(c, COMBINED_COV_MIN)
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(last[3])) and settings(c) == (GATE, True, cov)
        # the lag gate: a change keeps the history, and the next call runs under the new gate
        keeper = started()[0]
        open_ctx.append(keeper)
        dn.temporal_set_lag_correction(c, 0.5)
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(last[3])) and settings(c) == (0.5, True, cov)
        a, b = run(c, frames[2]), run(keeper, frames[2])
        assert np.array_equal(_bits(a[3][0, ..., 3]), _bits(b[3][0, ..., 3])) and np.array_equal(_bits(a[3][1]), _bits(b[3][1])) and np.array_equal(_bits(a[1][..., 3]), _bits(b[1][..., 3]))
        assert not np.array_equal(_bits(a[3][0, ..., :3]), _bits(b[3][0, ..., :3]))
        dn.temporal_set_lag_correction(c, None)                                                           # off: still no reset
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(a[3])) and settings(c)[1:] == (True, cov) and settings(c)[0] < 0
        # the variance of the mean and cov_min: a change forgets the history; what follows is a fresh context with the final settings
        for change, final in ((lambda x: dn.temporal_set_variance_of_mean(x, False), (GATE, False, COMBINED_COV_MIN)),
                              (lambda x: dn.temporal_set_coverage(x, 0.5), (GATE, True, 0.5)),
                              (lambda x: dn.temporal_set_coverage(x, None), (GATE, True, None))):
            x = started()[0]
            open_ctx.append(x)
            change(x)
            refuses(x)
            want = (GATE, final[1], float(f32(final[2])) if final[2] is not None else None)
            got = settings(x)
            assert got[:2] == want[:2] and (got[2] == want[2] if want[2] is not None else got[2] < 0)
            y = fresh(*final)
            open_ctx.append(y)
            for frame in frames[2:5]:
                same(run(x, frame), run(y, frame), final)
            for z in (x, y):
                _close(z, dn)
                open_ctx.remove(z)
    finally:
        for c in open_ctx:
            _close(c, dn)
