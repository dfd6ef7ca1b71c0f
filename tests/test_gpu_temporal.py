"""GPU tests (-m gpu) of temporal reprojection and accumulation (include/trg_denoise.h): the world-position plane against the primary rays,
one temporal step against the float64 reference written from the header (toyraygun_amd/denoise.py reference_temporal), the filter chain behind
it against reference_atrous_variance, the behaviour of the history, the composed entry points, the refusals and the plugin's switch.

BARS of the single-step comparison: the rule of tests/test_gpu_denoise_shapes.py.  The float32 mode of the reference says how far fp32
arithmetic alone moves a result (E32); the bar coefficient is max(1e-4, 4 E32) on colour, on N and on the moments, each on its own
(|a - ref|_2 over the channels against max(1, |ref|_2)), and max(1e-3, 4 E32) relative + 1e-9 on V_0.  Only pixels where the reference's
`near` plane is false are compared -- there no discrete decision of the definition is within 1e-4 of flipping -- and `near` may cover 1 % of
the picture at most.  One decision is kept apart: N against 4 only chooses the form of V_0, so a pixel near it is left out of the V_0
comparison alone, and its share is capped in every call but the one in which a history turns four frames old.  Every step is compared from
the DEVICE's own previous history, so a flipped decision cannot travel.  The cameras and the three call schedules: tests/test_temporal_host.py."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _close
from tests.test_temporal_host import CAMERAS, NEAR_CAP, SCHEDULES, camera_uniforms, position_plane, schedule_calls, seeded_colour
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [(37, 29), (80, 50)]          # no tile multiples; the reprojected taps of the border pixels fall outside the image
COLOUR_BAR, VARIANCE_BAR = 1e-4, 1e-3


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


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((a - ref) ** 2).sum(-1)) / np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))


def _set_camera(c, O, k):
    u = camera_uniforms(O, c.w, c.h, k)
    c.set_uniforms(O.uniforms_bytes(u))
    return u


def _filter_g0(dn, g, mats):
    """The filter's G0: the emitters marked as misses."""
    f = g[0].copy()
    f[dn.emitter_mask(g[1], mats), 3] = -1.0
    return f


# ---------------------------------------------------------------------------------------------------------------------------- 1. X plane
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_position_plane_is_the_ray_at_the_hit_distance(capi, dn, O, cornell, size, strict):
    """Scene in LDS and in HBM, two frame indices, a camera that sees the whole box and one that looks past it: X = fl(o + fl(z d)) bit for
    bit from trg_raygen's rays of the same setting and the G0.w returned, zero on the misses; G0 and G1 are trg_guides_render's."""
    import torch
    w, h = size
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for fg in (0, 1):
            c.set_option(capi.OPT_FORCE_GLOBAL, fg)
            for frame, u in ((0, camera_uniforms(O, w, h, 1)), (5, O.make_uniforms(w, h, 0, at=(2.2, 1.0, -1.0)))):
                c.set_uniforms(O.uniforms_bytes(u))
                g, X = dn.guides_pos(c, frame)
                assert np.array_equal(_bits(g), _bits(dn.guides(c, frame)))
                want = position_plane(c.raygen(frame), g)
                miss = g[0, ..., 3] < 0
                assert np.array_equal(_bits(X), _bits(want)), (fg, frame, int((_bits(X) != _bits(want)).sum()))
                assert (X[miss] == 0).all() and (X[..., 3] == 0).all() and (np.abs(X[~miss][:, :3]).max(-1) > 0).all()
                assert miss.any() and (frame == 0 or miss.mean() > 0.05)
        assert c.stats().scene_in_lds == 0
        gt = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
        xt = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        dn.guides_pos(c, 5, out=gt, pos=xt)
        c.sync()
        assert np.array_equal(_bits(gt.cpu().numpy()), _bits(g)) and np.array_equal(_bits(xt.cpu().numpy()), _bits(X))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 2. one step
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_one_step_matches_the_reference(capi, dn, O, cornell, size, strict):
    """The schedules of tests/test_temporal_host.py: start, a small move, the same again, a jump that uncovers surfaces -- after a reset at the
    default parameters, after a reset with max_history = 3 (the spatial variance everywhere) and after five calls at rest (the temporal
    variance; short histories where a move uncovered something).  Colour = seeded noise x albedo; guides and X from the device; after every compared call the history read back and
    (I, V_0) against reference_temporal evaluated from the device's own previous history."""
    w, h = size
    off = O.pixel_offsets(w, h)
    mats = cornell.buffers()["material_ids"]
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for name, sched in SCHEDULES.items():
            dn.temporal_reset(c)
            prev = None                                   # (the device's four history planes, the view-projection of their frame)
            seen_short = seen_long = False
            for call, (k, compared) in enumerate(schedule_calls(name)):
                u = _set_camera(c, O, k)
                g, X = dn.guides_pos(c, call)
                colour = seeded_colour(g, 200 + call)
                kw = dict(max_history=sched["max_history"], iterations=1)
                _, iv = dn.temporal_denoise(c, colour, g, X, None if prev is None else prev[1], return_iv=True, **kw)
                hist = dn.temporal_history(c)
                planes = np.stack([hist[0], hist[1], _filter_g0(dn, g, mats), X])
                if compared:
                    ref = dn.reference_temporal(colour, g[0], g[1], X, None if prev is None else prev[0], None if prev is None else prev[1], material_ids=mats,
                                                near_parts=True, **kw)
                    r32 = dn.reference_temporal(colour, g[0], g[1], X, None if prev is None else prev[0], None if prev is None else prev[1], material_ids=mats,
                                                dtype=np.float32, **kw)
                    near, near_n = ref[2]
                    ok = ~near                            # colour, N, moments
                    okv = ok & ~near_n                    # V_0: also decided which of its two forms applies
                    N = hist[0, ..., 3]
                    hit = planes[2, ..., 3] >= 0
                    assert near.mean() <= NEAR_CAP, (name, call, float(near.mean()))
                    assert near_n.mean() <= NEAR_CAP or (name == "default" and call == 3), (name, call, float(near_n.mean()))
                    assert (okv & hit).mean() > 0.02
                    e_c = float(_rel(r32[0][0][..., :3], ref[0][0][..., :3])[ok].max())
                    e_n = float(_rel(r32[0][0][..., 3:], ref[0][0][..., 3:])[ok].max())
                    e_m = float(_rel(r32[0][1], ref[0][1])[ok].max())
                    v64, v32 = ref[1][..., 3], r32[1][..., 3].astype(np.float64)
                    e_v = float((np.abs(v32 - v64) / (np.abs(v64) + 1e-9))[okv].max())
                    bc, bn, bm, bv = max(COLOUR_BAR, 4.0 * e_c), max(COLOUR_BAR, 4.0 * e_n), max(COLOUR_BAR, 4.0 * e_m), max(VARIANCE_BAR, 4.0 * e_v)
                    rc, rm, ri = _rel(hist[0][..., :3], ref[0][0][..., :3])[ok] / bc, _rel(hist[1], ref[0][1])[ok] / bm, _rel(iv[..., :3], ref[1][..., :3])[ok] / bc
                    rn = _rel(hist[0][..., 3:], ref[0][0][..., 3:])[ok] / bn
                    rv = (np.abs(iv[..., 3].astype(np.float64) - v64) / (bv * np.abs(v64) + 1e-9))[okv]
                    print("temporal step %s %dx%d strict %d call %d camera %d: near %.4f (N against 4: %.4f), E32 colour %.2e N %.2e moments %.2e V %.2e, worst err / bar: Hc.rgb %.3f N %.3f Hm %.3f I %.3f V %.3f; "
                          "N < 4 on %.3f of the hits, history found on %.3f" % (name, w, h, strict, call, k, near.mean(), near_n.mean(), e_c, e_n, e_m, e_v, rc.max(), rn.max(), rm.max(), ri.max(), rv.max(),
                                                                                 float((N[hit] < 4).mean()), float((N[hit] > 1).mean())))
                    assert (rc <= 1.0).all(), (name, call, int((rc > 1).sum()), float(rc.max()))
                    assert (rm <= 1.0).all(), (name, call, int((rm > 1).sum()), float(rm.max()))
                    assert (rn <= 1.0).all(), (name, call, int((rn > 1).sum()), float(rn.max()))
                    assert (ri <= 1.0).all(), (name, call, int((ri > 1).sum()), float(ri.max()))
                    assert (rv <= 1.0).all(), (name, call, int((rv > 1).sum()), float(rv.max()))
                    assert np.array_equal(_bits(iv[..., :3]), _bits(hist[0, ..., :3]))                 # (I, V_0) carries the history's colour
                    if prev is not None:
                        assert (N[hit] > 1).mean() > 0.5                                               # and history was found
                    seen_short |= bool((N[hit] < 4).any() and prev is not None)
                    seen_long |= bool((N[hit] >= 4).any())
                prev = (planes, dn.temporal_view_proj(u))
            assert seen_short and seen_long == (name != "fresh")
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. filter chain
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_filter_chain_matches_the_reference(capi, dn, O, cornell, size, strict):
    """out and V_N against reference_atrous_variance fed with the device's own (I, V_0): iterations 1, 2 (the LDS forms), 3, 5 (the L2 form) x
    demodulate, on a history that grows from call to call.  Bars of test_variance_filter_matches_the_reference: every pixel
    |out - ref|_2 <= 1e-4 max(1, |ref|_2) over the four channels, |V - V_ref| <= 1e-3 |V_ref| + 1e-9.  iterations = 0: out is (I, V_0)
    remodulated bit for bit, with the input's alpha."""
    w, h = size
    off = O.pixel_offsets(w, h)
    mats = cornell.buffers()["material_ids"]
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        vp_prev, call = None, 0
        for demod in (1, 0):
            for it in (1, 2, 3, 5, 0):
                u = _set_camera(c, O, (0, 1, 2, 1)[call % 4])
                g, X = dn.guides_pos(c, call)
                colour = seeded_colour(g, 300 + call)
                out, iv, var = dn.temporal_denoise(c, colour, g, X, vp_prev, return_iv=True, return_variance=True, iterations=it, demodulate=demod)
                vp_prev, call = dn.temporal_view_proj(u), call + 1
                kept = (g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats)
                assert np.array_equal(_bits(out[..., 3]), _bits(colour[..., 3]))                       # alpha is the input's
                assert kept.sum() > 20 and np.array_equal(_bits(out[kept]), _bits(colour[kept]))       # misses and emitters copy, bit for bit
                assert (var[kept] == 0).all() and (iv[kept][:, 3] == 0).all()
                if it == 0:
                    alb = np.maximum(g[1, ..., :3], f32(1e-3))
                    want = np.where(kept[..., None], iv[..., :3], iv[..., :3] * alb) if demod else iv[..., :3]
                    assert np.array_equal(_bits(out[..., :3]), _bits(want.astype(f32))) and np.array_equal(_bits(var), _bits(iv[..., 3]))
                    continue
                rgb, vref = dn.reference_atrous_variance(iv[..., :3], iv[..., 3], g[0], g[1], iterations=it, demodulate=demod, material_ids=mats)
                ref = np.concatenate([rgb, colour[..., 3:].astype(np.float64)], -1)
                err = np.sqrt(((out.astype(np.float64) - ref) ** 2).sum(-1))
                bar = 1e-4 * np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))
                verr = np.abs(var.astype(np.float64) - vref)
                vbar = 1e-3 * np.abs(vref) + 1e-9
                print("temporal filter chain %dx%d strict %d it %d demod %d: worst err / bar %.3f, variance %.3f" % (
                    w, h, strict, it, demod, float((err / bar).max()), float((verr / vbar).max())))
                assert (err <= bar).all(), (it, demod, int((err > bar).sum()), float((err / bar).max()))
                assert (verr <= vbar).all(), (it, demod, int((verr > vbar).sum()), float((verr / vbar).max()))
                hist_rgb = dn.temporal_history(c)[0, ..., :3]
                remod = np.where(kept[..., None], hist_rgb, hist_rgb * np.maximum(g[1, ..., :3], f32(1e-3))) if demod else hist_rgb
                assert np.abs(out[..., :3] - remod).max() > 0.05                                       # and it did filter
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. behaviour
@pytest.mark.parametrize("strict", [1, 0])
def test_history_length_and_copies(capi, dn, O, cornell, strict):
    """After a reset every hit pixel has N = 1; with the camera at rest, six calls and max_history = 4, N never exceeds 4 and never shrinks from
    call to call; misses and emitters are bit-exact copies with N = 0 and V = 0 throughout; a reset in between starts over."""
    w, h = 37, 29
    off = O.pixel_offsets(w, h)
    mats = cornell.buffers()["material_ids"]
    c = make_ctx(O, cornell, w, h, offsets=off, uniforms=O.make_uniforms(w, h, 0, at=(0.6, 1.0, -1.0)))
    try:
        c.set_option(capi.OPT_STRICT, strict)
        u = O.make_uniforms(w, h, 0, at=(0.6, 1.0, -1.0))
        vp = dn.temporal_view_proj(u)
        g, X = dn.guides_pos(c, 0)
        kept = (g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats)
        hit = ~kept
        assert (g[0, ..., 3] < 0).sum() > 20 and dn.emitter_mask(g[1], mats).sum() > 2
        for round_ in (0, 1):
            dn.temporal_reset(c)
            with pytest.raises(capi.TrgError):
                dn.temporal_history(c)                                                              # nothing to read after a reset
            last = None
            for call in range(6):
                colour = seeded_colour(g, 400 + call)
                out, iv = dn.temporal_denoise(c, colour, g, X, vp, return_iv=True, max_history=4, iterations=2)
                hist = dn.temporal_history(c)
                N = hist[0, ..., 3]
                if call == 0:
                    assert (N[hit] == 1).all()
                    D = colour[..., :3] / np.maximum(g[1, ..., :3], f32(1e-3))
                    assert np.array_equal(_bits(hist[0][hit][:, :3]), _bits(D[hit].astype(f32)))    # I = D exactly
                else:
                    assert (N[hit] >= last[hit]).all() and (N[hit] > 1).mean() > 0.9
                assert N.max() <= 4.0 and (N[hit] >= 1).all()
                assert (N[kept] == 0).all() and (hist[1][kept] == 0).all() and (iv[kept][:, 3] == 0).all()
                assert np.array_equal(_bits(out[kept]), _bits(colour[kept])) and np.array_equal(_bits(hist[0][kept][:, :3]), _bits(colour[kept][:, :3]))
                last = N
            assert (last[hit] == 4).mean() > 0.9
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 5. composed calls
@pytest.mark.parametrize("strict", [1, 0])
def test_render_temporal_is_its_steps(capi, dn, O, cornell, strict):
    """trg_render_temporal = a render from a zeroed image scaled to the mean of its samples + trg_guides_render_pos + trg_temporal_denoise
    against the previous call's view-projection, bit for bit, over three calls with a moving camera, through host buffers and on tensors;
    primary_rays == spp w h and `renders` goes up by one per call."""
    import torch
    w, h, bounces = 64, 48, 3
    off = O.pixel_offsets(w, h)
    a = make_ctx(O, cornell, w, h, offsets=off)
    b = make_ctx(O, cornell, w, h, offsets=off)
    t_ctx = make_ctx(O, cornell, w, h, offsets=off)
    try:
        for ctx in (a, b, t_ctx):
            ctx.set_option(capi.OPT_STRICT, strict)
        vp_prev = None
        for call, (k, first, spp, kw) in enumerate(((0, 0, 2, {}), (1, 2, 1, {}), (3, 3, 3, dict(iterations=3, alpha=0.5)))):
            u = None
            for ctx in (a, b, t_ctx):
                u = _set_camera(ctx, O, k)
            a.reset_stats()
            whole = dn.render_temporal(a, first, spp, bounces, **kw)
            st = a.stats()
            assert st.primary_rays == spp * w * h and st.renders == 1
            img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            b.bind_accum(img.data_ptr())
            try:
                b.render(first, spp, bounces)
                b.sync()
            finally:
                b.bind_accum(None)
            mean = img.cpu().numpy()
            mean[..., :3] = mean[..., :3] * f32(np.float64(first + spp) / np.float64(spp))
            g, X = dn.guides_pos(b, first)
            steps = dn.temporal_denoise(b, mean, g, X, vp_prev, **kw)
            assert np.array_equal(_bits(whole), _bits(steps)), (call, int((_bits(whole) != _bits(steps)).sum()))
            assert np.array_equal(_bits(dn.temporal_history(a)), _bits(dn.temporal_history(b)))
            out_t = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            dn.render_temporal(t_ctx, first, spp, bounces, out=out_t, **kw)
            t_ctx.sync()
            assert np.array_equal(_bits(out_t.cpu().numpy()), _bits(whole))
            vp_prev = dn.temporal_view_proj(u)
        assert not np.array_equal(_bits(whole), _bits(mean))
        # the tensor form of the step itself
        dn.temporal_reset(b)
        dn.temporal_reset(a)
        gt, xt, ct = (torch.from_numpy(x).cuda() for x in (g, X, mean))
        o_t = dn.temporal_denoise(b, ct, gt, xt, None, iterations=2)
        b.sync()
        assert np.array_equal(_bits(o_t.cpu().numpy()), _bits(dn.temporal_denoise(a, mean, g, X, None, iterations=2)))
    finally:
        for ctx in (a, b, t_ctx):
            _close(ctx, dn)


def test_render_temporal_leaves_the_callers_accumulation_and_binding_alone(capi, dn, O, cornell):
    """As test_halves_leave_the_callers_accumulation_and_binding_alone: the context's own buffer and a bound tensor keep their bits and their
    binding, and progressive accumulation goes on as if nothing had happened."""
    import torch
    w, h = 40, 30
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.render(0, 3, 3)
        own_ptr, own = c.accum_device_ptr(), c.read_accum()
        dn.render_temporal(c, 0, 2, 3)
        assert c.accum_device_ptr() == own_ptr and np.array_equal(_bits(c.read_accum()), _bits(own))
        mine = torch.full((h, w, 4), 0.25, dtype=torch.float32, device="cuda")
        c.bind_accum(mine.data_ptr())
        try:
            out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            dn.render_temporal(c, 2, 2, 3, out=out)
            c.sync()
            assert c.accum_device_ptr() == mine.data_ptr() and bool((mine == 0.25).all())
            dn.render_temporal(c, 4, 1, 3)
            assert c.accum_device_ptr() == mine.data_ptr() and bool((mine == 0.25).all())
        finally:
            c.bind_accum(None)
        assert c.accum_device_ptr() == own_ptr and np.array_equal(_bits(c.read_accum()), _bits(own))
        c.render(3, 2, 3)                                   # progressive accumulation goes on as if nothing had happened
        d = make_ctx(O, cornell, w, h, offsets=off)
        try:
            d.render(0, 5, 3)
            assert np.array_equal(_bits(c.read_accum()), _bits(d.read_accum()))
        finally:
            _close(d, dn)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 6. it helps
def orbit_eye(deg, eye=CAMERAS[0], at=(0.0, 1.0, -1.0)):
    """The eye turned by `deg` degrees about the vertical axis through the look-at point (the plugin's orbit=DEG)."""
    t = np.deg2rad(deg)
    dx, dz = eye[0] - at[0], eye[2] - at[2]
    return (at[0] + dx * np.cos(t) + dz * np.sin(t), eye[1], at[2] - dx * np.sin(t) + dz * np.cos(t))


def test_it_helps_a_moving_camera(capi, dn, O, cornell):
    """Cornell box, 64 x 48, 3 bounces, eight calls of 2 spp while the eye turns 1 degree per call: the last output is closer to a 512-spp
    render at the last camera than render_denoised_variance's 2 spp there.  The ratio is printed (DESIGN.md records it)."""
    w, h, bounces, calls, spp = 64, 48, 3, 8, 2
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        for k in range(calls):
            c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h, 0, eye=orbit_eye(float(k)))))
            out = dn.render_temporal(c, k * spp, spp, bounces)
        N = dn.temporal_history(c)[0, ..., 3]
        spatial = dn.render_denoised_variance(c, (calls - 1) * spp, spp, bounces)
        # the target: 512 spp at the last camera, from a zeroed buffer
        import torch
        acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        c.bind_accum(acc.data_ptr())
        try:
            c.render(0, 512, bounces)
            c.sync()
        finally:
            c.bind_accum(None)
        target = acc.cpu().numpy()
        rmse = lambda a: float(np.sqrt(((a[..., :3].astype(np.float64) - target[..., :3]) ** 2).mean()))
        print("moving camera, rmse against 512 spp: temporal (8 x 2 spp) %.5f, render_denoised_variance (2 spp) %.5f, ratio %.3f; mean N %.2f" % (
            rmse(out), rmse(spatial), rmse(out) / rmse(spatial), float(N[N > 0].mean())))
        assert N.max() > 6
        assert rmse(out) < rmse(spatial)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 7. refusals
def test_temporal_path_refuses_bad_arguments(capi, dn, O, cornell):
    import torch
    w, h = 37, 29
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    L = dn.load()

    def refused(fn):
        with pytest.raises(capi.TrgError) as e:
            fn()
        assert e.value.code == capi.ERR_INVALID and len(str(e.value)) > len("trg error -22: "), str(e.value)
    try:
        g, X = dn.guides_pos(c, 0)
        colour = seeded_colour(g, 7)
        vp = dn.temporal_view_proj(camera_uniforms(O, w, h, 0))
        dn.temporal_denoise(c, colour, g, X, None)
        before = dn.temporal_history(c)
        for kw in (dict(alpha=0.0), dict(alpha=1.5), dict(alpha=-0.1), dict(alpha_moments=0.0), dict(alpha_moments=1.01), dict(plane_tol=0.0), dict(plane_tol=-1.0),
                   dict(normal_tol=1.5), dict(normal_tol=-1.5), dict(max_history=0), dict(max_history=-3), dict(iterations=7), dict(iterations=-1)):
            refused(lambda: dn.temporal_denoise(c, colour, g, X, vp, **kw))
            refused(lambda: dn.render_temporal(c, 0, 1, 3, **kw))
        refused(lambda: dn.render_temporal(c, 0, 0, 3))                                              # no samples
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(before))                          # a refused call leaves the history alone
        ct, gt, xt = (torch.from_numpy(x).cuda() for x in (colour, g, X))
        o = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        refused(lambda: dn.temporal_denoise(c, ct, gt, xt, vp, out=ct))                              # out overlaps the colour
        refused(lambda: dn.temporal_denoise(c, ct, gt, xt, vp, out=gt[1]))                           # ... the guides
        refused(lambda: dn.temporal_denoise(c, ct, gt, xt, vp, out=xt))                              # ... the positions
        refused(lambda: dn.temporal_denoise(c, ct, gt, gt[0], vp, out=o))                            # the positions overlap the guides
        refused(lambda: dn.guides_pos(c, 0, out=gt, pos=gt[1]))
        p = dn.make_temporal_params()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        vpp = vp.ctypes.data_as(C.POINTER(C.c_float))
        for args in ((None, ptr(gt), ptr(xt), vpp, ptr(o)), (ptr(ct), None, ptr(xt), vpp, ptr(o)), (ptr(ct), ptr(gt), None, vpp, ptr(o)),
                     (ptr(ct), ptr(gt), ptr(xt), None, ptr(o)), (ptr(ct), ptr(gt), ptr(xt), vpp, None)):
            refused(lambda: dn._chk(c, L.trg_temporal_denoise(c.h_ctx, *args, C.byref(p))))         # NULLs
        c.bind_accum(o.data_ptr())
        try:
            refused(lambda: dn.render_temporal(c, 0, 1, 3, out=o))                                   # out is the bound accumulation buffer
        finally:
            c.bind_accum(None)
        refused(lambda: dn._chk(c, L.trg_guides_render_pos(c.h_ctx, 0, ptr(gt), None)))
        refused(lambda: dn._chk(c, L.trg_render_temporal(c.h_ctx, 0, 1, 3, None, C.byref(p))))
        refused(lambda: dn._chk(c, L.trg_temporal_history_read(c.h_ctx, None)))
        assert np.array_equal(_bits(dn.temporal_history(c)), _bits(before))
        out = dn.temporal_denoise(c, ct, gt, xt, vp, out=o, iterations=2)                            # and a good call still works
        c.sync()
        a = make_ctx(O, cornell, w, h, offsets=off)
        try:
            dn.temporal_denoise(a, colour, g, X, None)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(dn.temporal_denoise(a, colour, g, X, vp, iterations=2)))
        finally:
            _close(a, dn)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 8. plugin
def test_plugin_temporal_switch(capi, dn, tmp_path):
    """toyraygun_cornell ... denoise=5,temporal renders its frames as calls of 1 spp through trg_render_temporal_own and writes another picture
    than denoise=5,var: trg_postprocess of what render_temporal gives for the same calls; orbit=2 turns the eye between the calls and
    writes another picture again; an unknown token still fails."""
    import os
    import subprocess
    import torch
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 96, 64, 4, 3

    def run(name, *extra):
        path = str(tmp_path / name)
        subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba()
    var, tmp, orbit = run("var.png", "denoise=5,var"), run("tmp.png", "denoise=5,temporal"), run("orbit.png", "denoise=5,temporal", "orbit=2")
    assert not np.array_equal(var, tmp) and not np.array_equal(tmp, orbit) and not np.array_equal(var, orbit)
    for bad in (["denoise=5,nope"], ["denoise=5,temporal", "orbit=x"], ["denoise=5,temporal", "spin=2"]):
        assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png")] + bad, capture_output=True, timeout=120).returncode != 0
    b = host.Scene.cornell_box().buffers()
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        for k in range(frames):
            dn.render_temporal(c, k, 1, bounces, out=den, iterations=5)
        c.sync()
        c.bind_accum(den.data_ptr())
        try:
            assert np.array_equal(c.postprocess(flip_y=True), tmp)
        finally:
            c.bind_accum(None)
    finally:
        _close(c, dn)
