"""Device time of trg_guides_render, trg_denoise, the variance-guided path (trg_render_halves, trg_denoise_variance) and the temporal step
(trg_guides_render_pos, trg_temporal_denoise) on the Cornell box, HIP events on the context's stream:
python scripts/denoise_time.py [width height reps spp]   (default 1920 1080 20 16; one warm-up each).  Prints one JSON line with the medians in
ms, next to the filter's compulsory traffic (per iteration 48 B read + 16 B written per pixel) at the measured time.  The launches of the
variance-guided filter are taken as differences of runs that differ by one launch (prefilter on / off, N and N - 1 iterations).  The temporal
leg runs at rest (every tile of the spatial estimate leaves early once the history is four frames old) and with the eye turning 1 degree per
call; `temporal_front_ms` = the emitter marking, the reprojection and the spatial-estimate launch (a step of 0 iterations minus its final
copy is not separable here, so it is a step of 1 iteration minus one variance iteration of spacing 1).  The moving-geometry leg
(trg_temporal_set_previous_scene, trg_guides_render_motion, trg_temporal_denoise_motion) comes last: the motion-plane launch, and the step with
the motion planes beside the plain step at rest.  The changing-light leg (trg_temporal_set_lag_correction) is the plain step at rest with the
lag correction on and, right beside it, off again: the two differ by the one launch of dn_temporal_lag_kernel.  The long-history leg
(trg_temporal_set_variance_of_mean) is the 5-iteration step with the variance of the mean on and, right beside it, off, at rest and with the eye
turning: the same launches, two kernels in their TRACK forms.  The pixel-footprint leg (trg_guides_render_centre, trg_temporal_set_coverage)
comes last: the centre guide pass beside trg_guides_render_pos (two raygen and two trace launches instead of one of each), and the 5-iteration
step with the coverage history on and, right beside it, off, at rest and with the eye turning, on the centre guides' planes (X.w = A) in both."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toyraygun_amd import capi, denoise, host   # noqa: E402

w, h, reps, spp = (int(a) for a in (sys.argv[1:5] + ["1920", "1080", "20", "16"][len(sys.argv[1:5]):]))
b = host.Scene.cornell_box().buffers()
c = capi.Context(w, h)
c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
c.set_uniforms(host.uniforms(w, h)[0])
c.set_pixel_offsets_seed()
c.set_option(capi.OPT_TIMING, 0)
stream = torch.cuda.Stream()
c.set_stream(stream.cuda_stream)
acc = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
g = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
out = torch.empty_like(acc)
c.bind_accum(acc.data_ptr())
c.render(0, 4, 3)


def timed(fn):
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


res = {"width": w, "height": h, "reps": reps}
res["guides_ms"] = timed(lambda: denoise.guides(c, 0, out=g))
for it in (1, 5):
    res["denoise_%d_ms" % it] = timed(lambda: denoise.denoise(c, acc, g, out=out, iterations=it))
res["render_4spp_ms"] = timed(lambda: c.render(0, 4, 3))
# the variance-guided path: the price of the estimate (two half launches + the scaling against one launch of the same samples) ...
hv = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
res["spp"] = spp
res["render_%dspp_ms" % spp] = timed(lambda: c.render(0, spp, 3))
res["render_halves_%dspp_ms" % spp] = timed(lambda: denoise.render_halves(c, 0, spp, 3, out=hv))
res["render_half_%dspp_ms" % (spp // 2)] = timed(lambda: c.render(0, spp // 2, 3))
# ... and the filter: whole runs, then single launches as differences
var = lambda **kw: timed(lambda: denoise.denoise_variance(c, hv, g, out=out, **kw))
t = {(it, pre): var(iterations=it, prefilter=pre) for it in range(0, 6) for pre in (0, 1) if pre == 0 or it in (1, 5)}
res["denoise_variance_5_ms"] = t[(5, 1)]
res["denoise_variance_1_ms"] = t[(1, 1)]
res["variance_prefilter_ms"] = t[(5, 1)] - t[(5, 0)]
res["variance_combine_ms"] = t[(0, 0)]
res["variance_iteration_ms"] = [t[(1, 0)] - t[(0, 0)]] + [t[(it, 0)] - t[(it - 1, 0)] for it in range(2, 6)]
old = {it: timed(lambda: denoise.denoise(c, acc, g, out=out, iterations=it)) for it in range(1, 6)}
res["denoise_iteration_ms"] = [old[1]] + [old[it] - old[it - 1] for it in range(2, 6)]
res["compulsory_GB_5"] = 5 * 64 * w * h / 1e9
res["compulsory_GBps_at_denoise_5"] = res["compulsory_GB_5"] / (res["denoise_5_ms"] * 1e-3)
# the temporal step: guides with the position plane, then whole steps at rest and with a turning eye
from oracle import pyoracle as O   # noqa: E402  (the uniforms of another eye; host.uniforms has the default camera only)
x = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
res["guides_pos_ms"] = timed(lambda: denoise.guides_pos(c, 0, out=g, pos=x))
u_rest = O.make_uniforms(w, h)
vp_rest = denoise.temporal_view_proj(u_rest)
c.set_uniforms(O.uniforms_bytes(u_rest))
denoise.guides_pos(c, 0, out=g, pos=x)
denoise.temporal_reset(c)
step = lambda vp, **kw: denoise.temporal_denoise(c, acc, g, x, vp, out=out, **kw)
for _ in range(6):
    step(vp_rest)
res["temporal_5_rest_ms"] = timed(lambda: step(vp_rest))
res["temporal_1_rest_ms"] = timed(lambda: step(vp_rest, iterations=1))
res["temporal_front_rest_ms"] = res["temporal_1_rest_ms"] - res["variance_iteration_ms"][0]
# moving: the history planes of the eye one degree back (one untimed step there), then steps at this eye against that camera
t = np.deg2rad(1.0)
u_back = O.make_uniforms(w, h, eye=(4.38 * np.sin(-t), 1.0, -1.0 + 4.38 * np.cos(-t)))
vp_back = denoise.temporal_view_proj(u_back)


def moving(centre=False, **kw):
    c.set_uniforms(O.uniforms_bytes(u_back))
    g2, x2 = torch.empty_like(g), torch.empty_like(x)
    (denoise.guides_centre if centre else denoise.guides_pos)(c, 0, out=g2, pos=x2)   # (centre: the pixel-footprint leg, X.w = A)
    denoise.temporal_reset(c)
    denoise.temporal_denoise(c, acc, g2, x2, None, out=out, **kw)     # N = 1 everywhere at the other eye
    c.set_uniforms(O.uniforms_bytes(u_rest))
    ms = []
    for _ in range(reps):
        # every timed step needs that history again: re-seed it untimed
        if ms:
            denoise.temporal_reset(c)
            denoise.temporal_denoise(c, acc, g2, x2, None, out=out, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); step(vp_back, **kw); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


res["temporal_5_moving_ms"] = moving()
res["temporal_1_moving_ms"] = moving(iterations=1)
res["temporal_front_moving_ms"] = res["temporal_1_moving_ms"] - res["variance_iteration_ms"][0]
res["l2_iteration_ms"] = res["variance_iteration_ms"][2]
# moving geometry.  The motion-plane launch as guides_motion minus guides_pos.  Then steps with the motion planes, the camera at rest, after six
# calls: first with a previous scene that IS the loaded scene (nothing moved: every pixel finds its history as in the plain leg at rest, every
# tile of the spatial estimate leaves early, so the difference to the plain 1-iteration step is the reprojection kernel's MOTION form alone),
# then with the short box 0.02 further left at the previous call (the pixels the box uncovers keep N < 4, so the spatial estimate runs on
# their tiles in every call)
mo = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
moved = b["positions"].copy()
moved[:36, 0] -= np.float32(0.02)
for name, prev in (("still", b["positions"]), ("moved", moved)):
    denoise.temporal_set_previous_scene(c, prev, b["normals"], b["indices"])
    if name == "still":
        res["guides_motion_ms"] = timed(lambda: denoise.guides_motion(c, 0, out=g, pos=x, motion=mo))
        res["motion_planes_ms"] = res["guides_motion_ms"] - res["guides_pos_ms"]
    denoise.guides_motion(c, 0, out=g, pos=x, motion=mo)
    denoise.temporal_reset(c)
    for _ in range(6):
        step(vp_rest, motion=mo)
    res["temporal_5_motion_%s_ms" % name] = timed(lambda: step(vp_rest, motion=mo))
    res["temporal_1_motion_%s_ms" % name] = timed(lambda: step(vp_rest, motion=mo, iterations=1))
res["reproject_motion_extra_ms"] = res["temporal_1_motion_still_ms"] - res["temporal_1_rest_ms"]
# changing light: the step at rest with the lag correction on, then off, measured side by side after six calls each -- the same launches but one
denoise.temporal_reset(c)
for name, gate in (("lag", denoise.LAG_GATE_DEFAULT), ("lag_off", -1.0)):
    denoise.temporal_set_lag_correction(c, gate)
    for _ in range(6):
        step(vp_rest)
    res["temporal_5_%s_ms" % name] = timed(lambda: step(vp_rest))
    res["temporal_1_%s_ms" % name] = timed(lambda: step(vp_rest, iterations=1))
res["lag_launch_ms"] = [res["temporal_%d_lag_ms" % it] - res["temporal_%d_lag_off_ms" % it] for it in (1, 5)]
# a long history: the 5-iteration step with the variance of the mean on and, right beside it, off -- at rest after six calls (a change of the
# setting forgets the history), and with the eye turning as in the moving leg above.  The same launches; the TRACK forms of two kernels
for name, on in (("vmean", True), ("vmean_off", False)):
    denoise.temporal_set_variance_of_mean(c, on)
    for _ in range(6):
        step(vp_rest)
    res["temporal_5_rest_%s_ms" % name] = timed(lambda: step(vp_rest))
    res["temporal_5_moving_%s_ms" % name] = moving()
res["vmean_extra_ms"] = {leg: res["temporal_5_%s_vmean_ms" % leg] - res["temporal_5_%s_vmean_off_ms" % leg] for leg in ("rest", "moving")}
# pixel footprints: the guide pass from the pixel centres with the agreement flag, then the step on ITS planes with the coverage history on and,
# right beside it, off (a change of the setting forgets the history: six calls at rest first).  The same launches; the COVER form of one kernel
denoise.temporal_set_variance_of_mean(c, False)
res["guides_centre_ms"] = timed(lambda: denoise.guides_centre(c, 0, out=g, pos=x))
res["guides_pos_again_ms"] = timed(lambda: denoise.guides_pos(c, 0, out=g, pos=x))
res["guides_centre_extra_ms"] = res["guides_centre_ms"] - res["guides_pos_again_ms"]
denoise.guides_centre(c, 0, out=g, pos=x)
for name, cov in (("cover", denoise.COVERAGE_MIN_DEFAULT), ("cover_off", None)):
    denoise.temporal_set_coverage(c, cov)
    for _ in range(6):
        step(vp_rest)
    res["temporal_5_rest_%s_ms" % name] = timed(lambda: step(vp_rest))
    res["temporal_5_moving_%s_ms" % name] = moving(centre=True)
res["cover_extra_ms"] = {leg: res["temporal_5_%s_cover_ms" % leg] - res["temporal_5_%s_cover_off_ms" % leg] for leg in ("rest", "moving")}
print(json.dumps(res))
c.bind_accum(None)
c.set_stream(None)
denoise.release(c)
c.close()
