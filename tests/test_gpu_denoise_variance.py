"""GPU tests (-m gpu) of the variance-guided path of include/trg_denoise.h: the two half-sample buffers against the CPU oracle, the filter against
the float64 reference written from the header (toyraygun_amd/denoise.py reference_denoise_variance), the composed entry point, the refusals and
the plugin's switch."""
import numpy as np
import pytest

from tests.test_denoise_variance_host import oracle_halves
from tests.test_gpu_denoise import _synthetic
from tests.util import TOL_FRAC, TOL_RMSE, image_metrics, make_ctx

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


# ---------------------------------------------------------------------------------------------------------------------------- 1. halves
HALF_W, HALF_H, HALF_BOUNCES = 40, 30, 3
HALF_CASES = [(0, 2), (0, 6), (4, 4)]


@pytest.fixture(scope="module")
def halves_ref(O, cornell):
    """The oracle's renders of the two frame ranges from zeroed buffers with the same fp32 scaling: with the portable trigonometry the strict
    build shares bit for bit, and with libm's for the shipped build's image tolerance."""
    off = O.pixel_offsets(HALF_W, HALF_H)
    out = {}
    for mode, key in ((O.TRIG_PORTABLE, 1), (O.TRIG_LIBM, 0)):
        O.set_trig_mode(mode)
        try:
            for b, n in HALF_CASES:
                out[(key, b, n)] = oracle_halves(O, cornell, HALF_W, HALF_H, b, n, HALF_BOUNCES, off)
        finally:
            O.set_trig_mode(O.TRIG_LIBM)
    return out


@pytest.mark.parametrize("force_global", [0, 1])
def test_halves_match_the_oracle(capi, dn, O, cornell, halves_ref, force_global):
    """40 x 30, (b, n) = (0, 2), (0, 6), (4, 4), scene staged in LDS and kept in HBM.  Strict: both planes bit for bit.  Shipped: the project's
    image tolerance per plane.  The rays of both renders count: exactly n frames' primary rays, and all four counters those of ONE trg_render
    of the same frames."""
    w, h = HALF_W, HALF_H
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    plain = make_ctx(O, cornell, w, h, offsets=off)
    rays = lambda s: (s.primary_rays, s.bounce_rays, s.shadow_rays, s.shaded_hits)
    try:
        c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
        plain.set_option(capi.OPT_FORCE_GLOBAL, force_global)
        for b, n in HALF_CASES:
            for strict in (1, 0):
                c.set_option(capi.OPT_STRICT, strict)
                c.reset_stats()
                hv = dn.render_halves(c, b, n, HALF_BOUNCES)
                st = c.stats()
                ref = halves_ref[(strict, b, n)]
                if strict:
                    assert np.array_equal(_bits(hv), _bits(ref)), (b, n, int((_bits(hv) != _bits(ref)).sum()))
                else:
                    for k in (0, 1):
                        rmse, frac, worst = image_metrics(hv[k], ref[k])
                        print("halves b %d n %d force_global %d plane %d shipped: rmse %.2e, %.4f of the pixels inside, worst %.2e" % (b, n, force_global, k, rmse, frac, worst))
                        assert rmse <= TOL_RMSE and frac >= TOL_FRAC
                        assert np.array_equal(_bits(hv[k][..., 3]), _bits(ref[k][..., 3]))
                assert st.primary_rays == n * w * h and st.renders == 2
                plain.set_option(capi.OPT_STRICT, strict)
                plain.reset_stats()
                plain.render(b, n, HALF_BOUNCES)     # (from whatever the buffer holds: only the counters matter)
                assert rays(st) == rays(plain.stats())
        assert c.stats().scene_in_lds == (0 if force_global else 1)
    finally:
        _close(c, dn)
        _close(plain, dn)


def test_halves_leave_the_callers_accumulation_and_binding_alone(capi, dn, O, cornell):
    import torch
    w, h = HALF_W, HALF_H
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.render(0, 3, 3)
        own_ptr, own = c.accum_device_ptr(), c.read_accum()
        dn.render_halves(c, 0, 4, 3)
        assert c.accum_device_ptr() == own_ptr and np.array_equal(_bits(c.read_accum()), _bits(own))
        mine = torch.full((h, w, 4), 0.25, dtype=torch.float32, device="cuda")
        c.bind_accum(mine.data_ptr())
        try:
            hv = torch.empty((2, h, w, 4), dtype=torch.float32, device="cuda")
            dn.render_halves(c, 2, 2, 3, out=hv)
            c.sync()
            assert c.accum_device_ptr() == mine.data_ptr() and bool((mine == 0.25).all())
            assert np.array_equal(_bits(hv.cpu().numpy()), _bits(dn.render_halves(c, 2, 2, 3)))   # device and host variants agree
            assert bool((mine == 0.25).all())
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


# ---------------------------------------------------------------------------------------------------------------------------- 2. filter
def _synthetic_halves(w, h, seed=11, gen=_synthetic):
    """_synthetic's (or another generator's) colour, guides, misses and emitter block; the halves are that colour with independent relative
    noise of up to 30 %, their own alphas, and one pixel column where H1 == H2 (images narrower than six pixels: their last column; one
    pixel wide: their last row instead; 1 x 1: none, its pixel keeps two different halves)."""
    color, g0, g1 = gen(w, h, seed)
    rng = np.random.default_rng(seed + 1)
    h1 = (color * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, (h, w, 4)))).astype(f32)
    h2 = (color * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, (h, w, 4)))).astype(f32)
    if w > 1:
        h2[:, min(5, w - 1)] = h1[:, min(5, w - 1)]
    elif h > 1:
        h2[h - 1] = h1[h - 1]
    return np.stack([h1, h2]), g0, g1


_var_refs = {}


def _var_ref(dn, size, it, pre, demod, material_ids):
    key = (size, it, pre, demod)
    if key not in _var_refs:
        hv, g0, g1 = _synthetic_halves(*size)
        _var_refs[key] = dn.reference_denoise_variance(hv[0], hv[1], g0, g1, iterations=it, prefilter=pre, demodulate=demod, material_ids=material_ids,
                                                       return_variance=True)
    return _var_refs[key]


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", [(37, 29), (80, 50)])
def test_variance_filter_matches_the_reference(capi, dn, O, cornell, size, strict):
    """37 x 29 and 80 x 50: no multiples of the tile, spacing 16 has taps inside and outside the image.  Iterations 1, 2 (the two LDS forms), 3, 5
    (the L2 form) x prefilter x demodulate, with misses, an emitter block and a column with H1 == H2.  Bars: every pixel
    |out - ref|_2 <= 1e-4 * max(1, |ref|_2) over the four channels; the variance after the last iteration |V - V_ref| <= 1e-3 |V_ref| + 1e-9."""
    w, h = size
    hv, g0, g1 = _synthetic_halves(w, h)
    guides = np.stack([g0, g1])
    mats = cornell.buffers()["material_ids"]
    kept = (g0[..., 3] < 0) | dn.emitter_mask(g1, mats)
    assert kept.sum() > 42 and np.array_equal(hv[0][:, 5], hv[1][:, 5])
    c = make_ctx(O, cornell, w, h)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for it in (1, 2, 3, 5):
            for pre in (0, 1):
                for demod in (0, 1):
                    out, var = dn.denoise_variance(c, hv, guides, iterations=it, prefilter=pre, demodulate=demod, return_variance=True)
                    ref, vref = _var_ref(dn, size, it, pre, demod, mats)
                    err = np.sqrt(((out.astype(np.float64) - ref) ** 2).sum(-1))
                    bar = 1e-4 * np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))
                    verr = np.abs(var.astype(np.float64) - vref)
                    vbar = 1e-3 * np.abs(vref) + 1e-9
                    print("variance filter %dx%d strict %d it %d prefilter %d demod %d: worst err / bar %.3f, variance %.3f" % (
                        w, h, strict, it, pre, demod, float((err / bar).max()), float((verr / vbar).max())))
                    assert (err <= bar).all(), (it, pre, demod, int((err > bar).sum()), float((err / bar).max()))
                    assert (verr <= vbar).all(), (it, pre, demod, int((verr > vbar).sum()), float((verr / vbar).max()))
                    assert np.array_equal(_bits(out[..., 3]), _bits(hv[0][..., 3]))      # alpha is H1's
                    mean = (f32(0.5) * (hv[0] + hv[1]))[..., :3]
                    assert np.array_equal(_bits(out[kept][..., :3]), _bits(mean[kept]))  # misses and emitters carry the plain mean
                    assert (var[kept] == 0).all()
                    assert np.abs(out[..., :3] - mean).max() > 0.1                       # and it did filter
        # iterations = 0: the mean of the halves in fp32, alpha of H1
        out = dn.denoise_variance(c, hv, guides, iterations=0)
        assert np.array_equal(_bits(out[..., :3]), _bits((f32(0.5) * (hv[0] + hv[1]))[..., :3])) and np.array_equal(_bits(out[..., 3]), _bits(hv[0][..., 3]))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("strict", [1, 0])
def test_render_denoised_variance_is_its_three_steps(capi, dn, O, cornell, strict):
    """trg_render_denoised_variance = trg_render_halves + trg_guides_render + trg_denoise_variance, bit for bit, through host buffers and on
    tensors."""
    import torch
    w, h = 64, 48
    off = O.pixel_offsets(w, h)
    c = make_ctx(O, cornell, w, h, offsets=off)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for b, n, kw in ((0, 4, {}), (2, 2, dict(iterations=3, prefilter=0))):
            whole = dn.render_denoised_variance(c, b, n, 3, **kw)
            hv = dn.render_halves(c, b, n, 3)
            steps = dn.denoise_variance(c, hv, dn.guides(c, b), **kw)
            assert np.array_equal(_bits(whole), _bits(steps))
        t = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        dn.render_denoised_variance(c, 2, 2, 3, out=t, **kw)
        c.sync()
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(whole))
        hv_t = torch.from_numpy(hv).cuda()
        g_t = torch.from_numpy(dn.guides(c, 2)).cuda()
        o_t = dn.denoise_variance(c, hv_t, g_t, **kw)
        c.sync()
        assert np.array_equal(_bits(o_t.cpu().numpy()), _bits(whole))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 4. refusals
def test_variance_path_refuses_bad_arguments(capi, dn, O, cornell):
    import ctypes as C
    import torch
    w, h = 37, 29
    hv, g0, g1 = _synthetic_halves(w, h)
    guides = np.stack([g0, g1])
    c = make_ctx(O, cornell, w, h)
    L = dn.load()

    def refused(fn):
        with pytest.raises(capi.TrgError) as e:
            fn()
        assert e.value.code == capi.ERR_INVALID and len(str(e.value)) > len("trg error -22: "), str(e.value)
    try:
        for n in (3, 1, 0):
            refused(lambda: dn.render_halves(c, 0, n, 3))                                # odd n, n < 2
            refused(lambda: dn.render_denoised_variance(c, 0, n, 3))
        refused(lambda: dn.denoise_variance(c, hv, guides, iterations=7))
        refused(lambda: dn.render_denoised_variance(c, 0, 2, 3, iterations=7))
        t = torch.from_numpy(hv).cuda()
        g = torch.from_numpy(guides).cuda()
        refused(lambda: dn.denoise_variance(c, t, g, out=t[1]))                          # out overlaps the halves
        o = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        p = dn.make_var_params()
        refused(lambda: dn._chk(c, L.trg_denoise_variance(c.h_ctx, None, C.c_void_p(g.data_ptr()), C.c_void_p(o.data_ptr()), C.byref(p))))   # NULL halves
        refused(lambda: dn._chk(c, L.trg_render_halves(c.h_ctx, 0, 2, 3, None)))
        acc = torch.zeros((2, h, w, 4), dtype=torch.float32, device="cuda")
        c.bind_accum(acc[1].data_ptr())
        try:
            refused(lambda: dn.render_halves(c, 0, 2, 3, out=acc))                        # the halves overlap the bound accumulation buffer
        finally:
            c.bind_accum(None)
        out = dn.denoise_variance(c, t, g, out=o, iterations=2)                           # and a good call still works
        c.sync()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(dn.denoise_variance(c, hv, guides, iterations=2)))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- 5. plugin
def test_plugin_variance_guided_switch(capi, dn, tmp_path):
    """toyraygun_cornell ... denoise=5,var writes another picture than denoise=5: trg_postprocess of what render_denoised_variance gives for the
    same frames; with an odd frame count it renders one more sample, says so, and writes the picture of the even count."""
    import os
    import subprocess
    from toyraygun_amd import host
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces = 96, 64, 4, 3

    def run(name, n, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, str(w), str(h), str(n), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba(), r.stdout
    (old, _), (var, said), (odd, said_odd) = run("old.png", frames, "denoise=5"), run("var.png", frames, "denoise=5,var"), run("odd.png", frames - 1, "denoise=5,var")
    assert not np.array_equal(old, var)
    assert "rendering 4 samples, not 3" in said_odd and "samples, not" not in said
    assert np.array_equal(odd, var)
    assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "denoise=5,nope"], capture_output=True, timeout=120).returncode != 0
    b = host.Scene.cornell_box().buffers()
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        import torch
        den = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        dn.render_denoised_variance(c, 0, frames, bounces, out=den, iterations=5)
        c.sync()
        c.bind_accum(den.data_ptr())
        try:
            assert np.array_equal(c.postprocess(flip_y=True), var)
        finally:
            c.bind_accum(None)
    finally:
        _close(c, dn)
