"""GPU tests (-m gpu) of the variance of the mean (include/trg_denoise.h, "A LONG HISTORY"; the TRACK forms of dn_temporal_reproject_kernel and
dn_temporal_spatial_kernel): the step with the setting on against reference_temporal(track=True) from the DEVICE's own previous history on the
synthetic stage of tests/test_temporal_synthetic_host.py, the motion form and the lag correction beside it bit for bit, off-means-off, the
refusals, the turning eye end to end on the Cornell box, and the plugin's `,vmean`.

BARS.  Those of tests/test_gpu_temporal_shapes.py, from the reference alone: E32 = the reference's float32 mode against its float64 mode on the
same inputs (both with track=True); max(1e-4, 4 E32) on Hc.rgb, on N, on the moments (m1, m2) and on I, relative to max(1, |ref|_2);
max(1e-3, 4 E32) relative + 1e-9 on V_0 = (I, V_0).w AND on Hm.z, which hold Vc; only where `near` is false, for the two variances also
`near_n`.  Hm.w is 0 bit for bit.  Nothing in a bar comes from the device.

MEASURED on an MI355X: see DESIGN.md, "Denoiser", *Variance of the mean*."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _close
from tests.test_gpu_temporal import _filter_g0
from tests.test_gpu_temporal_shapes import _ctx, _finish, _ref
from tests.test_motion_host import identity_motion
from tests.test_temporal_synthetic_host import (COLOUR_BAR, SCHEDULE, SHAPES_PARAMS, _max, _rel, near_caps, schedule_frames)
from tests.test_vmean_host import orbit_eye
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
STEP_SHAPES = [(1, 1), (9, 1), (15, 17), (16, 16), (17, 33), (48, 32)]      # w x h: the issue's
NAMES = ("Hc.rgb", "N", "m1 m2", "I", "V_0", "Hm.z")


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


def _step(dn, c, mats, frame, params, motion=False, **kw):
    """One call on the device with the context's settings as they are: (out, iv, the new history planes as the next call's reference reads them)."""
    colour, g, X, vp, cam = frame
    res = dn.temporal_denoise(c, colour, g, X, vp, return_iv=True, motion=identity_motion(g, X) if motion else None, **dict(params, **kw))
    hist = dn.temporal_history(c)
    return res + (np.stack([hist[0], hist[1], _filter_g0(dn, g, mats), X]),)


def _compare(tag, call, R, planes, iv):
    """near and near_n under their caps, then every plane within its bar on the compared pixels: the rule of tests/test_gpu_temporal_shapes.py with
    the moments' bar from (m1, m2) alone and Hm.z under V_0's."""
    near_caps(R["near"], R["near_n"], call)
    ok, okv, (bc, bn, _, bv) = R["ok"], R["okv"], R["bars"]
    new, n32, v64 = R["new"], R["n32"], R["iv"][..., 3]
    bm = max(COLOUR_BAR, 4.0 * _max(_rel(n32[1][..., :2], new[1][..., :2])[ok]))
    assert np.array_equal(new[1, ..., 2], v64) and (new[1, ..., 3] == 0).all()                            # the reference: Hm.z = V_0 = Vc
    variance = lambda v: (np.abs(np.asarray(v, np.float64) - v64) / (bv * np.abs(v64) + 1e-9))[okv]
    ratios = (_rel(planes[0][..., :3], new[0][..., :3])[ok] / bc, _rel(planes[0][..., 3:], new[0][..., 3:])[ok] / bn,
              _rel(planes[1][..., :2], new[1][..., :2])[ok] / bm, _rel(iv[..., :3], R["iv"][..., :3])[ok] / bc, variance(iv[..., 3]), variance(planes[1][..., 2]))
    worst = [_max(r) for r in ratios]
    print("%s call %d: near %d, near_n %d of %d pixels; E32 V %.2e; worst err / bar: %s" % (
        tag, call, R["near"].sum(), R["near_n"].sum(), R["near"].size, R["e32"][3], " ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, worst))))
    for name, r in zip(NAMES, ratios):
        assert (r <= 1.0).all(), (tag, call, name, int((r > 1).sum()), float(r.max()))
    assert np.array_equal(_bits(iv[..., :3]), _bits(planes[0][..., :3]))                                  # (I, V_0) carries the history's colour
    assert np.array_equal(_bits(iv[..., 3]), _bits(planes[1][..., 2]))                                    # ... and the history's Vc
    assert np.array_equal(_bits(planes[1][..., 3]), _bits(np.zeros_like(planes[1][..., 3])))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------- 1. the step
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", STEP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_step_with_the_setting_on(capi, dn, O, cornell, size, strict):
    """SCHEDULE (nine calls, two stages, the five matrices) with max_history = 6 and iterations = 0, the setting on: every call against
    reference_temporal(track=True) from the device's own previous history; out = (I, V_0) remodulated bit for bit.  A second context runs the same
    calls through trg_temporal_denoise_motion_host with identity planes: bit for bit the first's.  A third has the lag correction on as well:
    N, Hm (the moments and Vc) and V_0 are the first's bit for bit, while its colour moved.  On the larger images both forms of Vc are met, and
    Vc differs from the plain step's V_0."""
    w, h = size
    params = dict(SHAPES_PARAMS, iterations=0)
    (c, mats), (m, _), (l, _) = (_ctx(O, cornell, w, h, capi, strict) for _ in range(3))
    try:
        for x in (c, m, l):
            dn.temporal_set_variance_of_mean(x, True)
            assert dn.temporal_variance_of_mean(x)
        dn.temporal_set_lag_correction(l, 3.0)
        prev, worst, recursed, short, lag_moved, differs = None, [0.0] * len(NAMES), 0, 0, 0, 0
        tag = "vmean %dx%d strict %d" % (w, h, strict)
        for call, frame in enumerate(schedule_frames(w, h, SCHEDULE)):
            out, iv, planes = _step(dn, c, mats, frame, params)
            R = _ref(dn, ("vmean", size), call, frame, prev, mats, dict(params, track=True))
            worst = [max(a, b) for a, b in zip(worst, _compare(tag, call, R, planes, iv))]
            _finish(dn, frame, out, iv, mats, 1)
            for a, b in zip((out, iv, planes), _step(dn, m, mats, frame, params, motion=True)):
                assert np.array_equal(_bits(a), _bits(b)), call
            lout, liv, lplanes = _step(dn, l, mats, frame, params)
            assert np.array_equal(_bits(lplanes[1]), _bits(planes[1])) and np.array_equal(_bits(liv[..., 3]), _bits(iv[..., 3])), call
            assert np.array_equal(_bits(lplanes[0][..., 3]), _bits(planes[0][..., 3])), call
            lag_moved += int((_bits(lplanes[0][..., :3]) != _bits(planes[0][..., :3])).any(-1).sum())
            N, hit = planes[0, ..., 3], planes[2, ..., 3] >= 0
            recursed += int((hit & (N >= 4) & R["okv"]).sum())
            short += int((hit & (N < 4) & R["okv"]).sum())
            plain = dn.reference_temporal(frame[0], frame[1][0], frame[1][1], frame[2], prev, None if prev is None else frame[3], material_ids=mats, **params)[1]
            differs += int((hit & R["okv"] & (np.abs(iv[..., 3] - plain[..., 3]) > 2.0 * R["bars"][3] * np.abs(plain[..., 3]) + 2e-9)).sum())
            prev = planes
        print("%s: worst err / bar over the schedule: %s; compared pixels with the recursion %d, with S %d; Vc off the plain V_0 on %d; the lag correction moved %d colours" % (
            tag, " ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, worst)), recursed, short, differs, lag_moved))
        if w * h >= 255:
            assert recursed > 0.2 * w * h and short > 0.2 * w * h and differs > 0.1 * w * h and lag_moved > 0
    finally:
        for x in (c, m, l):
            _close(x, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 2. off means off
@pytest.mark.parametrize("strict", [1, 0])
def test_off_means_off(capi, dn, O, cornell, strict):
    """37 x 29, SCHEDULE with two iterations.  A context that switched the setting on and off again before its first call gives the sequence of a
    context that never knew it, bit for bit: out, (I, V_0), V_N and the history of every call, and Hm.z stays 0; a context with the setting on
    gives another V_0 once a history is four frames old.  Repeating the current value keeps the history; a CHANGE leaves none
    (trg_temporal_history_read refuses), in either direction, and what follows is the sequence after trg_temporal_reset."""
    w, h = 37, 29
    (never, mats), (toggled, _), (on, _), (late, _) = (_ctx(O, cornell, w, h, capi, strict) for _ in range(4))
    try:
        dn.temporal_set_variance_of_mean(toggled, True)
        dn.temporal_set_variance_of_mean(toggled, False)
        dn.temporal_set_variance_of_mean(on, True)
        dn.temporal_set_variance_of_mean(late, True)
        kw = dict(return_iv=True, return_variance=True, iterations=2)
        frames = schedule_frames(w, h, SCHEDULE)[:6]
        run = lambda x, frame: dn.temporal_denoise(x, frame[0], frame[1], frame[2], frame[3], **kw) + (dn.temporal_history(x),)
        differed = 0
        for call, frame in enumerate(frames):
            got = {name: run(x, frame) for name, x in (("never", never), ("toggled", toggled), ("on", on))}
            for k, (a, b) in enumerate(zip(got["toggled"], got["never"])):
                assert np.array_equal(_bits(a), _bits(b)), (call, k)
            assert (got["never"][3][1, ..., 2:] == 0).all()
            assert np.array_equal(_bits(got["on"][3][0]), _bits(got["never"][3][0]))                      # Hc: tracking touches the variance alone
            assert np.array_equal(_bits(got["on"][3][1][..., :2]), _bits(got["never"][3][1][..., :2]))
            differed += not np.array_equal(_bits(got["on"][1][..., 3]), _bits(got["never"][1][..., 3]))
            assert call >= 3 or np.array_equal(_bits(got["on"][0]), _bits(got["never"][0]))                # below four frames Vc = S
        assert differed >= 2
        # repeating the value changes nothing; a change forgets the history
        for frame in frames[:2]:
            run(late, frame)
        dn.temporal_set_variance_of_mean(late, True)
        assert dn.temporal_history(late).shape == (2, h, w, 4)
        dn.temporal_set_variance_of_mean(late, False)
        assert not dn.temporal_variance_of_mean(late)
        with pytest.raises(capi.TrgError) as e:
            dn.temporal_history(late)
        assert e.value.code == capi.ERR_INVALID
        dn.temporal_reset(never)
        for frame in frames[2:5]:
            for k, (a, b) in enumerate(zip(run(late, frame), run(never, frame))):
                assert np.array_equal(_bits(a), _bits(b)), k
        dn.temporal_set_variance_of_mean(late, True)
        with pytest.raises(capi.TrgError):
            dn.temporal_history(late)
        dn.temporal_reset(on)
        assert dn.temporal_variance_of_mean(on)                                                            # the setting survives the reset
        for frame in frames[2:4]:
            for k, (a, b) in enumerate(zip(run(late, frame), run(on, frame))):
                assert np.array_equal(_bits(a), _bits(b)), k
    finally:
        for x in (never, toggled, on, late):
            _close(x, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. refusals and queries
def test_variance_of_mean_entry_points_refuse_and_report(capi, dn, O, cornell):
    w, h = 17, 9
    c = make_ctx(O, cornell, w, h)
    try:
        L = dn.load()
        on = C.c_int(7)
        assert L.trg_temporal_set_variance_of_mean(None, 1) == capi.ERR_INVALID
        assert L.trg_temporal_variance_of_mean(None, C.byref(on)) == capi.ERR_INVALID and on.value == 7
        assert not dn.temporal_variance_of_mean(c)                                                         # a fresh context: off
        with pytest.raises(capi.TrgError) as e:
            dn._chk(c, L.trg_temporal_variance_of_mean(c.h_ctx, None))
        assert e.value.code == capi.ERR_INVALID and len(str(e.value)) > len("trg error -22: "), str(e.value)
        dn.temporal_set_variance_of_mean(c, True)                                                          # (a context that never denoised)
        assert dn.temporal_variance_of_mean(c)
        dn.temporal_reset(c)
        assert dn.temporal_variance_of_mean(c)
        assert L.trg_temporal_set_variance_of_mean(c.h_ctx, 5) == capi.OK and dn.temporal_variance_of_mean(c)   # any non-zero value: on
        assert dn.temporal_lag_correction(c) < 0                                                           # the two settings are apart
        dn.temporal_set_variance_of_mean(c, False)
        assert not dn.temporal_variance_of_mean(c)
        dn.temporal_set_variance_of_mean(c, True)
        dn.release(c)
        assert not dn.temporal_variance_of_mean(c)                                                         # the setting ends with the state
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. end to end
def test_it_helps_end_to_end(capi, dn, O, cornell):
    """Cornell box, 64 x 48, 3 bounces, eight calls of 2 spp through trg_render_temporal while the eye turns 1 degree per call, default
    parameters, with the setting on and off: the last output with it on is closer to a 512-spp render at the last camera.  The ratio is
    printed (DESIGN.md records it; the float64 reference on the oracle's renders gives 0.909)."""
    w, h, bounces, calls, spp = 64, 48, 3, 8, 2
    off = O.pixel_offsets(w, h)
    tracked, plain = (make_ctx(O, cornell, w, h, offsets=off) for _ in range(2))
    try:
        dn.temporal_set_variance_of_mean(tracked, True)
        for k in range(calls):
            u = O.uniforms_bytes(O.make_uniforms(w, h, 0, eye=orbit_eye(float(k))))
            outs = []
            for c in (tracked, plain):
                c.set_uniforms(u)
                outs.append(dn.render_temporal(c, k * spp, spp, bounces))
        vc = dn.temporal_history(tracked)[1, ..., 2]
        assert (dn.temporal_history(plain)[1, ..., 2] == 0).all() and (vc > 0).mean() > 0.5
        plain.render(0, 512, bounces)                                                                     # the target: 512 spp at the last camera
        target = plain.read_accum()
        rmse = lambda a: float(np.sqrt(((a[..., :3].astype(np.float64) - target[..., :3]) ** 2).mean()))
        print("vmean end to end, eye turning, 8 x 2 spp, rmse against 512 spp: plain %.5f, tracked %.5f, ratio %.3f" % (rmse(outs[1]), rmse(outs[0]), rmse(outs[0]) / rmse(outs[1])))
        assert rmse(outs[0]) < rmse(outs[1])
    finally:
        _close(tracked, dn)
        _close(plain, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 5. plugin
def test_plugin_vmean_option(capi, dn, tmp_path):
    """toyraygun_cornell 64 48 8 3 out.png denoise=5,temporal,vmean: another picture than without `,vmean`; with `,lag` in front of it another one
    again, the picture of the same calls through the C ABI with both settings on; a malformed token is refused before anything starts."""
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 64, 48, 8, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba()
    vmean, plain, both = run("vmean.png", "denoise=5,temporal,vmean"), run("plain.png", "denoise=5,temporal"), run("both.png", "denoise=5,temporal,lag,vmean")
    assert not np.array_equal(vmean, plain) and not np.array_equal(both, vmean)
    for bad in ("denoise=5,temporal,vmean=1", "denoise=5,temporal,vmean,vmean", "denoise=5,var,vmean", "denoise=5,vmean", "denoise=5,temporal,vmean,",
                "denoise=5,temporal,lag,vmean,lag"):
        assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), bad], capture_output=True, timeout=120).returncode != 0
    b = host.Scene.cornell_box().buffers()
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        dn.temporal_set_variance_of_mean(c, True)
        dn.temporal_set_lag_correction(c, dn.LAG_GATE_DEFAULT)
        den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        for k in range(frames):
            dn.render_temporal(c, k, 1, bounces, out=den, iterations=5)
        c.sync()
        c.bind_accum(den.data_ptr())
        try:
            assert np.array_equal(c.postprocess(flip_y=True), both)
        finally:
            c.bind_accum(None)
    finally:
        _close(c, dn)
