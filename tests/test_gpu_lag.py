"""GPU tests (-m gpu) of the gated lag correction of the temporal step (include/trg_denoise.h, "CHANGING LIGHT"; dn_temporal_lag_kernel): the
stage kernel against reference_lag at every shape, the whole step on the changed schedule of tests/test_lag_host.py against
reference_temporal(lag=gate) from the DEVICE's own previous history, off-means-off, the refusals, a change of the light's colour end to end on
the Cornell box, and the plugin's `,lag`.

BARS.  The stage kernel: the convention of tests/test_gpu_denoise_shapes.py -- E32 = the reference's float32 mode against its float64 mode on the
same inputs, |a - ref|_2 <= max(1e-4, 4 E32) x max(1, |ref|_2) per pixel.  The whole step: the bars of tests/test_gpu_temporal_shapes.py, its
_compare / _finish used as they are.  The end-to-end ratios are the issue's: the correction at gate 3 against off, rmse against a 512-spp render
under the light of the call -- dimmed x 0.25, first call after: on <= 0.5 off (the float64 prototype on the oracle's renders: 0.24);
brightened x 4: on <= 0.9 off (0.75); at rest on within 1 % of off (under 0.3 %).  The margins are there because the noise realisation, not
the device's arithmetic, sets these ratios.

MEASURED on an MI355X: see DESIGN.md, "Denoiser", *Changing light*."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _close
from tests.test_gpu_motion import _load, _slid_cornell
from tests.test_gpu_temporal import _filter_g0
from tests.test_gpu_temporal_shapes import _compare, _ctx, _finish, _ref
from tests.test_lag_host import CHANGE_CALL, GATES, changed_frames
from tests.test_motion_host import identity_motion
from tests.test_temporal_host import seeded_colour
from tests.test_temporal_synthetic_host import SHAPES_PARAMS, _max, _rel, stage
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
STAGE_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (15, 17), (16, 16), (17, 33), (48, 32)]     # w x h: narrower than the halo .. several tiles


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


def _refused(capi, fn):
    with pytest.raises(capi.TrgError) as e:
        fn()
    assert e.value.code == capi.ERR_INVALID and len(str(e.value)) > len("trg error -22: "), str(e.value)


def _lagged_history(g, colour, demodulate, seed):
    """A plane (I.rgb, N): 0.3 x this call's colour + 2 x another noise, demodulated -- a history that lags behind a dimmed light --,
    N = 3; misses hold their colour and N = 0, as the Accumulate step leaves them."""
    other = seeded_colour(g, seed)
    hc = np.zeros(colour.shape, f32)
    alb = np.maximum(g[1, ..., :3], f32(1e-3)) if demodulate else f32(1.0)
    hc[..., :3] = ((f32(0.3) * colour[..., :3] + f32(2.0) * other[..., :3]) / alb).astype(f32)
    hc[..., 3] = 3.0
    miss = g[0, ..., 3] < 0
    hc[miss] = np.concatenate([colour[miss][:, :3], np.zeros((int(miss.sum()), 1), f32)], -1)
    return hc


# ---------------------------------------------------------------------------------------------------------------------------- 1. the stage kernel
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", STAGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_stage_kernel_matches_reference_lag(capi, dn, O, cornell, size, strict):
    """trg_temporal_lag_correct_host on the synthetic stage (misses, emitters, zero normals, albedo under the clamp, normals longer than 1) at the
    eight shapes, gates 0, 3 and 30, demodulate 0 and 1: Ic within the bar of reference_lag on every pixel; N, and every miss and emitter,
    bit for bit the input's; the zero normals unchanged; and on the images of at least 255 pixels the correction did something at gate 3."""
    w, h = size
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    try:
        g, X = stage(w, h, 1)
        colour = seeded_colour(g, 41)
        F = _filter_g0(dn, g, mats)
        kept = F[..., 3] < 0
        zero = ~kept & ((F[..., :3] ** 2).sum(-1) == 0)
        for demod in (1, 0):
            hc = _lagged_history(g, colour, demod, 42)
            for gate in GATES:
                got = dn.lag_correct(c, colour, g, hc, gate, demodulate=demod)
                ref, mask = dn.reference_lag(colour, g[0], g[1], hc, gate, material_ids=mats, demodulate=demod)
                r32, _ = dn.reference_lag(colour, g[0], g[1], hc, gate, material_ids=mats, demodulate=demod, dtype=np.float32)
                assert r32.dtype == np.float32
                e32 = _max(_rel(r32, ref))
                bar = max(1e-4, 4.0 * e32)
                err = _max(_rel(got[..., :3], ref))
                print("lag stage %dx%d strict %d demodulate %d gate %g: E32 %.2e, err / bar %.3f, changed %d of %d hits" % (
                    w, h, strict, demod, gate, e32, err / bar, int(mask.sum()), int((~kept).sum())))
                assert err <= bar, (demod, gate, err, bar)
                assert np.array_equal(_bits(got[..., 3]), _bits(hc[..., 3]))
                assert np.array_equal(_bits(got[kept | zero]), _bits(hc[kept | zero])) and not mask[kept | zero].any()
                if w * h >= 255 and gate == 3.0:
                    assert mask.mean() > 0.25 and (_bits(got[..., :3]) != _bits(hc[..., :3])).any(-1)[mask].mean() > 0.9
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 2. the whole step
def _step(dn, c, mats, frame, params, motion=False):
    """One call on the device with the context's correction as it is set: (out, iv, the new history planes as the next call's reference reads them)."""
    colour, g, X, vp, cam = frame
    kw = {k: v for k, v in params.items() if k != "lag"}
    out, iv = dn.temporal_denoise(c, colour, g, X, vp, return_iv=True, motion=identity_motion(g, X) if motion else None, **kw)
    hist = dn.temporal_history(c)
    return out, iv, np.stack([hist[0], hist[1], _filter_g0(dn, g, mats), X])


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("size", [(5, 3), (17, 33), (48, 32)], ids=lambda s: "%dx%d" % s)
def test_whole_step_on_the_changed_schedule(capi, dn, O, cornell, size, gate, strict):
    """The changed schedule (x 0.25 from call 4 on) through trg_temporal_denoise_host with the correction on, max_history = 6, iterations = 0:
    Hc, Hm and (I, V_0) of every call against reference_temporal(lag=gate) from the device's own previous history, out = (I, V_0) remodulated
    bit for bit.  A second context runs the same calls through trg_temporal_denoise_motion_host with identity planes: bit for bit the first's.
    On the larger images the device's own correction moved at least half of the hits in the call of the change (gates 0 and 3)."""
    w, h = size
    params = dict(SHAPES_PARAMS, iterations=0, lag=gate)
    (c, mats), (m, _) = (_ctx(O, cornell, w, h, capi, strict) for _ in range(2))
    try:
        for x in (c, m):
            dn.temporal_set_lag_correction(x, gate)
        prev = None
        for call, frame in enumerate(changed_frames(w, h)):
            out, iv, planes = _step(dn, c, mats, frame, params)
            R = _ref(dn, ("lag", size, gate), call, frame, prev, mats, params)
            _compare("temporal lag %dx%d gate %g strict %d" % (w, h, gate, strict), call, R, planes, iv)
            _finish(dn, frame, out, iv, mats, 1)
            for a, b in zip((out, iv, planes), _step(dn, m, mats, frame, params, motion=True)):
                assert np.array_equal(_bits(a), _bits(b)), call
            if call == CHANGE_CALL and w * h >= 255 and gate <= 3.0:
                plain = dn.reference_temporal(frame[0], frame[1][0], frame[1][1], frame[2], prev, frame[3], material_ids=mats, **SHAPES_PARAMS)[0]
                hit = planes[2, ..., 3] >= 0
                moved = (_rel(planes[0, ..., :3], plain[0, ..., :3]) > 1e-3) & hit
                assert moved.sum() >= 0.5 * hit.sum(), (int(moved.sum()), int(hit.sum()))
            prev = planes
    finally:
        _close(c, dn)
        _close(m, dn)


@pytest.mark.parametrize("strict", [1, 0])
def test_filter_runs_from_the_corrected_colour(capi, dn, O, cornell, strict):
    """17 x 33, the call of the change with two iterations behind the correction: out against reference_atrous_variance fed with the device's own
    (I, V_0), under the E32 rule (the float32 mode of that loop against its float64 mode on the same input)."""
    w, h = 17, 33
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    try:
        dn.temporal_set_lag_correction(c, 3.0)
        for call, (colour, g, X, vp, cam) in enumerate(changed_frames(w, h)[:CHANGE_CALL + 1]):
            out, iv = dn.temporal_denoise(c, colour, g, X, vp, return_iv=True, iterations=2, **SHAPES_PARAMS)
        ref, _ = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], g[0], g[1], iterations=2, material_ids=mats)
        r32, _ = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], g[0], g[1], iterations=2, material_ids=mats, dtype=np.float32)
        bar = max(1e-4, 4.0 * _max(_rel(r32, ref)))
        err = _max(_rel(out[..., :3], ref))
        print("lag filter strict %d: err / bar %.3f" % (strict, err / bar))
        assert err <= bar and np.array_equal(_bits(out[..., 3]), _bits(colour[..., 3]))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. off means off
@pytest.mark.parametrize("strict", [1, 0])
def test_off_means_off(capi, dn, O, cornell, strict):
    """37 x 29, the changed schedule with two iterations.  A context that switched the correction on and off again before its first call, and one
    that ran its first call with it on (no history: nothing to correct) and switched it off then, give the sequence of a context that never
    switched it on, bit for bit: out, (I, V_0), V_N and the history of every call.  And with the correction on, the first call after
    trg_temporal_reset is the plain one bit for bit, while the calls with history were not."""
    w, h = 37, 29
    (never, mats), (early, _), (late, _), (on, _) = (_ctx(O, cornell, w, h, capi, strict) for _ in range(4))
    try:
        dn.temporal_set_lag_correction(early, 3.0)
        dn.temporal_set_lag_correction(early, -1.0)
        dn.temporal_set_lag_correction(late, 0.0)
        dn.temporal_set_lag_correction(on, 3.0)
        kw = dict(return_iv=True, return_variance=True, iterations=2)
        frames = changed_frames(w, h)[:CHANGE_CALL + 2]
        differed = 0
        for call, (colour, g, X, vp, cam) in enumerate(frames):
            got = {name: dn.temporal_denoise(x, colour, g, X, vp, **kw) + (dn.temporal_history(x),) for name, x in (("never", never), ("early", early), ("late", late), ("on", on))}
            for name in ("early", "late"):
                for k, (a, b) in enumerate(zip(got[name], got["never"])):
                    assert np.array_equal(_bits(a), _bits(b)), (name, call, k)
            same = all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got["on"], got["never"]))
            assert same or call > 0
            differed += not same
            if call == 0:
                dn.temporal_set_lag_correction(late, -1.0)
        assert differed >= 2
        assert dn.temporal_lag_correction(on) == 3.0 and dn.temporal_lag_correction(late) < 0
        for x in (on, never):
            dn.temporal_reset(x)
        colour, g, X, vp, cam = frames[-1]
        a, b = (dn.temporal_denoise(x, colour, g, X, vp, **kw) + (dn.temporal_history(x),) for x in (on, never))
        assert dn.temporal_lag_correction(on) == 3.0                                                          # the setting survives the reset
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(_bits(x), _bits(y)), k
    finally:
        for x in (never, early, late, on):
            _close(x, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. refusals
def test_lag_entry_points_refuse_and_report(capi, dn, O, cornell):
    w, h = 17, 9
    c = make_ctx(O, cornell, w, h)
    try:
        assert dn.temporal_lag_correction(c) < 0                                                              # a fresh context: off
        _refused(capi, lambda: dn.temporal_set_lag_correction(c, float("nan")))
        assert dn.temporal_lag_correction(c) < 0
        dn.temporal_set_lag_correction(c, 2.5)                                                                # (a context that never denoised)
        assert dn.temporal_lag_correction(c) == 2.5
        _refused(capi, lambda: dn.temporal_set_lag_correction(c, float("nan")))
        assert dn.temporal_lag_correction(c) == 2.5                                                           # nothing changed
        dn.temporal_reset(c)
        assert dn.temporal_lag_correction(c) == 2.5
        dn.temporal_set_lag_correction(c)
        assert dn.temporal_lag_correction(c) == dn.LAG_GATE_DEFAULT
        dn.temporal_set_lag_correction(c, None)
        assert dn.temporal_lag_correction(c) < 0
        g, X = stage(w, h, 1)
        colour = seeded_colour(g, 3)
        hc = _lagged_history(g, colour, 1, 4)
        for bad in (dict(gate=-1.0), dict(gate=float("nan")), dict(sigma_depth=0.0), dict(sigma_normal=-1.0)):
            args = dict(dict(gate=3.0), **bad)
            _refused(capi, lambda: dn.lag_correct(c, colour, g, hc, **args))
        L = dn.load()
        _refused(capi, lambda: dn._chk(c, L.trg_temporal_lag_correct_host(c.h_ctx, colour.ctypes.data, g.ctypes.data, None, 3.0, 128.0, 1.0, 1, hc.ctypes.data)))
        dn.temporal_set_lag_correction(c, 3.0)
        assert dn.lag_correct(c, colour, g, hc, 3.0).shape == (h, w, 4)                                       # and a good call still works
        dn.release(c)
        assert dn.temporal_lag_correction(c) < 0                                                              # the setting ends with the state
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 5. end to end
AT_REST, AFTER = 8, 6


def _rmse(a, ref):
    return float(np.sqrt(((a[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2).mean()))


def _light_case(O, w, h, case):
    u = O.make_uniforms(w, h)
    if case == "dimmed":
        u.light_color[0:3] = [float(f32(v) * f32(0.25)) for v in u.light_color[0:3]]
    elif case == "brightened":
        u.light_color[0:3] = [float(f32(v) * f32(4.0)) for v in u.light_color[0:3]]
    elif case == "moved":
        u.light_pos[0] = float(f32(u.light_pos[0]) + f32(0.4))
    return u


@pytest.fixture(scope="module")
def light_truth(capi, dn, O, cornell):
    """512-spp trg_render of the Cornell box at 64 x 48, 3 bounces, strict build, under the four lights; computed once."""
    w, h = 64, 48
    c = make_ctx(O, cornell, w, h, offsets=O.pixel_offsets(w, h))
    try:
        c.set_option(capi.OPT_STRICT, 1)
        truth = {}
        for case in ("rest", "dimmed", "brightened", "moved"):
            c.set_uniforms(O.uniforms_bytes(_light_case(O, w, h, case)))
            c.render(0, 512, 3)
            truth[case] = c.read_accum().copy()
        return truth
    finally:
        _close(c, dn)


@pytest.mark.parametrize("case", ["dimmed", "brightened", "moved"])
def test_changed_light_end_to_end(capi, dn, O, cornell, light_truth, case):
    """Cornell box 64 x 48, trg_render_temporal_read of 1 spp and 3 bounces, default parameters, strict build: eight calls at rest, then the
    light changes (its colour x 0.25, x 4, or light_pos.x + 0.4) and six more calls; one context with the correction at gate 3, one without.
    rmse over rgb against the 512-spp render under the light of the call.  At rest every call: on within 1 % of off.  First call after the
    change: dimmed on <= 0.5 off, brightened on <= 0.9 off; the moved light's ratio is printed only."""
    w, h, bounces = 64, 48, 3
    off = O.pixel_offsets(w, h)
    on_ctx, off_ctx = (make_ctx(O, cornell, w, h, offsets=off) for _ in range(2))
    try:
        for c in (on_ctx, off_ctx):
            c.set_option(capi.OPT_STRICT, 1)
        dn.temporal_set_lag_correction(on_ctx, dn.LAG_GATE_DEFAULT)
        ratios = []
        for call in range(AT_REST + AFTER):
            name = "rest" if call < AT_REST else case
            u = O.uniforms_bytes(_light_case(O, w, h, name))
            e = []
            for c in (on_ctx, off_ctx):
                c.set_uniforms(u)
                e.append(_rmse(dn.render_temporal(c, call, 1, bounces), light_truth[name]))
            ratios.append((e[0], e[1], e[0] / e[1]))
        print("lag end to end %s: rmse on / off = ratio per call: %s" % (case, "  ".join("%d: %.4f / %.4f = %.3f" % ((k,) + r) for k, r in enumerate(ratios))))
        assert ratios[0][0] == ratios[0][1]                                                                   # no history: nothing to correct
        for k in range(AT_REST):
            assert abs(ratios[k][2] - 1.0) <= 0.01, (k, ratios[k])
        first = ratios[AT_REST][2]
        if case == "dimmed":
            assert first <= 0.5, first
        elif case == "brightened":
            assert first <= 0.9, first
    finally:
        _close(on_ctx, dn)
        _close(off_ctx, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 6. plugin
def test_plugin_lag_option(capi, dn, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png denoise=5,temporal,lag slide=0.02: the picture of the same calls through the C ABI with
    trg_temporal_set_lag_correction(ctx, 3.0f); without `,lag` today's picture, which differs; a bad gate is refused before anything starts."""
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces, slide = 64, 48, 4, 3, 0.02

    def run(name, *extra):
        path = str(tmp_path / name)
        subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba()
    lag, plain = run("lag.png", "denoise=5,temporal,lag", "slide=0.02"), run("plain.png", "denoise=5,temporal", "slide=0.02")
    assert not np.array_equal(lag, plain)
    for bad in ("denoise=5,temporal,lag=x", "denoise=5,temporal,lag=-1", "denoise=5,var,lag"):
        assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), bad], capture_output=True, timeout=120).returncode != 0
    scenes = [_slid_cornell(host, float(f32(k * slide))) for k in range(frames)]
    for gate, want in ((3.0, lag), (None, plain)):
        c = capi.Context(w, h)
        try:
            _load(c, scenes[0])
            c.set_uniforms(host.uniforms(w, h)[0])
            c.set_pixel_offsets_seed()
            if gate is not None:
                dn.temporal_set_lag_correction(c, gate)
            den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            for k in range(frames):
                if k:
                    _load(c, scenes[k])
                    dn.temporal_set_previous_scene(c, scenes[k - 1]["positions"], scenes[k - 1]["normals"], scenes[k - 1]["indices"])
                dn.render_temporal(c, k, 1, bounces, out=den, iterations=5)
            c.sync()
            c.bind_accum(den.data_ptr())
            try:
                assert np.array_equal(c.postprocess(flip_y=True), want), gate
            finally:
                c.bind_accum(None)
        finally:
            _close(c, dn)
