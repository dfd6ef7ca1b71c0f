"""GPU tests (-m gpu) of the two filters of include/trg_denoise.h at the shapes and parameters tests/test_gpu_denoise.py and
tests/test_gpu_denoise_variance.py leave out: images smaller than a 16 x 16 tile, one pixel wide or high, 1 x 1, exact tile multiples; every
iteration count (spacing 2 as the last launch, spacing 32); normals that are not unit and dot products near 1; albedo under the 1e-3 clamp;
other sigmas, sigma_normal == 0 among them -- and of the state-owned entry points trg_denoise_accum / trg_render_denoised_variance_own.

BARS.  The kernels compute in fp32, the reference in float64.  For every case the float32 mode of the reference (every intermediate fp32, pow and
exp through exp2 / log2 as the shipped build has them) says how far fp32 arithmetic alone moves the result: E32 = the worst
|ref32 - ref64|_2 / max(1, |ref64|_2) over the pixels, and |V32 - V64| / (|V64| + 1e-9) for the carried variance.  The bar coefficient is
max(the existing bar, 4 E32) -- existing: 1e-4 for colour, 1e-3 for V; the factor 4 covers the hardware's 1-ulp exp2 / log2 against numpy's
correctly rounded ones and a tap order that differs from numpy's.  Nothing here is taken from what the kernels return."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _close, _smooth, _smooth_hits, _synthetic
from tests.test_gpu_denoise_variance import _synthetic_halves
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (15, 17), (16, 16), (32, 16), (17, 33), (48, 32)]     # w x h
GENERATORS = {"synthetic": _synthetic, "smooth": _smooth, "hits": _smooth_hits}


def _generators(size):
    """_synthetic's and _smooth's inputs; at 1 x 1, where the one pixel of both is a miss (the copy path), also the 1 x 1 image whose pixel is
    a hit: the centre tap alone, the 3 x 3 variance and GV over one pixel, all 48 taps of the prefilter outside, demodulation and
    remodulation.  (No bit-equality is asked of it: the pixel's result is (w c) / w in fp32, which need not be c.)"""
    return ("smooth", "synthetic") + (("hits",) if size == (1, 1) else ())
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
    """|a - ref|_2 / max(1, |ref|_2) per pixel over the four channels."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((a - ref) ** 2).sum(-1)) / np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))


_refs = {}


def _plain_ref(dn, gen, size, mats, **kw):
    """(float64 reference, colour bar coefficient, E32) of one case, computed once for both settings."""
    key = ("plain", gen, size, tuple(sorted(kw.items())))
    if key not in _refs:
        color, g0, g1 = GENERATORS[gen](size[0], size[1], 11)
        r64 = dn.reference_denoise(color, g0, g1, material_ids=mats, **kw)
        r32 = dn.reference_denoise(color, g0, g1, material_ids=mats, dtype=np.float32, **kw)
        e32 = float(_rel(r32, r64).max())
        _refs[key] = (r64, max(COLOUR_BAR, 4.0 * e32), e32)
    return _refs[key]


def _var_ref(dn, gen, size, mats, **kw):
    """(float64 image, float64 V_N, colour bar coefficient, V bar coefficient, E32, E32 of V)."""
    key = ("var", gen, size, tuple(sorted(kw.items())))
    if key not in _refs:
        hv, g0, g1 = _synthetic_halves(size[0], size[1], gen=GENERATORS[gen])
        r64, v64 = dn.reference_denoise_variance(hv[0], hv[1], g0, g1, material_ids=mats, return_variance=True, **kw)
        r32, v32 = dn.reference_denoise_variance(hv[0], hv[1], g0, g1, material_ids=mats, return_variance=True, dtype=np.float32, **kw)
        e32 = float(_rel(r32, r64).max())
        ev32 = float((np.abs(v32.astype(np.float64) - v64) / (np.abs(v64) + 1e-9)).max())
        _refs[key] = (r64, v64, max(COLOUR_BAR, 4.0 * e32), max(VARIANCE_BAR, 4.0 * ev32), e32, ev32)
    return _refs[key]


def _check_plain(dn, c, gen, size, strict, mats, **kw):
    w, h = size
    color, g0, g1 = GENERATORS[gen](w, h, 11)
    out = dn.denoise(c, color, np.stack([g0, g1]), **kw)
    ref, coef, e32 = _plain_ref(dn, gen, size, mats, **kw)
    ratio = _rel(out, ref) / coef
    print("plain %s %dx%d strict %d %s: E32 %.2e, bar %.2e, worst err / bar %.3f" % (
        gen, w, h, strict, " ".join("%s %g" % kv for kv in sorted(kw.items())), e32, coef, float(ratio.max())))
    assert (ratio <= 1.0).all(), (gen, size, strict, kw, int((ratio > 1.0).sum()), float(ratio.max()))
    assert np.array_equal(_bits(out[..., 3]), _bits(color[..., 3]))                           # alpha passes through
    kept = (g0[..., 3] < 0) | dn.emitter_mask(g1, mats)
    assert kept.any() == (gen != "hits") and np.array_equal(_bits(out[kept]), _bits(color[kept]))   # misses and emitters copy their input
    if w * h == 1 and gen != "hits":
        assert np.array_equal(_bits(out), _bits(color))
    return out


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_plain_filter_at_every_shape_and_iteration_count(capi, dn, O, cornell, size, strict):
    """Iterations 1 .. 6 x demodulate 0, 1 on _synthetic's and _smooth's inputs (1 x 1: and on a pixel that is a hit, _generators).  Even counts end on an odd launch (2: the spacing-2 LDS form
    remodulates and stores the result), 6 reaches spacing 32, the largest the header allows; at 1 x 9 and 9 x 1 most taps fall outside, at
    16 x 16, 32 x 16 and 48 x 32 a tile's halo is wholly inside or wholly outside the image."""
    mats = cornell.buffers()["material_ids"]
    c = make_ctx(O, cornell, size[0], size[1])
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for gen in _generators(size):
            filtered = False
            for it in range(1, 7):
                for demod in (0, 1):
                    out = _check_plain(dn, c, gen, size, strict, mats, iterations=it, demodulate=demod)
                    filtered |= bool(np.abs(out[..., :3] - GENERATORS[gen](size[0], size[1], 11)[0][..., :3]).max() > 0.05)
            assert filtered or size[0] * size[1] < 10                                         # and it did filter
    finally:
        _close(c, dn)


@pytest.mark.parametrize("strict", [1, 0])
def test_plain_filter_with_other_sigmas(capi, dn, O, cornell, strict):
    """48 x 32: sigma_normal 0 (w_n = x^0 = 1 for every x > 0: the shipped build's exp2(0 * log2 x)) with sigma_depth 0.25 and sigma_color 0.5;
    and sigma_normal 1 (w_n = n_p . n_q itself)."""
    mats = cornell.buffers()["material_ids"]
    size = (48, 32)
    c = make_ctx(O, cornell, size[0], size[1])
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for gen in _generators(size):
            _check_plain(dn, c, gen, size, strict, mats, iterations=5, sigma_normal=0.0, sigma_depth=0.25, sigma_color=0.5)
            _check_plain(dn, c, gen, size, strict, mats, iterations=5, sigma_normal=1.0)
            _check_plain(dn, c, gen, size, strict, mats, iterations=2, sigma_normal=0.0, demodulate=0)
    finally:
        _close(c, dn)


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_variance_filter_at_every_shape(capi, dn, O, cornell, size, strict):
    """Iterations 1, 2, 3, 6 x prefilter 0, 1 x demodulate 0, 1, the image and the carried variance V_N; the halves as _synthetic_halves makes
    them from _synthetic's and _smooth's inputs."""
    w, h = size
    mats = cornell.buffers()["material_ids"]
    c = make_ctx(O, cornell, w, h)
    try:
        c.set_option(capi.OPT_STRICT, strict)
        for gen in _generators(size):
            hv, g0, g1 = _synthetic_halves(w, h, gen=GENERATORS[gen])
            guides = np.stack([g0, g1])
            kept = (g0[..., 3] < 0) | dn.emitter_mask(g1, mats)
            mean = (f32(0.5) * (hv[0] + hv[1]))[..., :3]
            assert kept.any() == (gen != "hits")
            for it in (1, 2, 3, 6):
                for pre in (0, 1):
                    for demod in (0, 1):
                        kw = dict(iterations=it, prefilter=pre, demodulate=demod)
                        out, var = dn.denoise_variance(c, hv, guides, return_variance=True, **kw)
                        ref, vref, coef, vcoef, e32, ev32 = _var_ref(dn, gen, size, mats, **kw)
                        ratio = _rel(out, ref) / coef
                        vratio = np.abs(var.astype(np.float64) - vref) / (vcoef * np.abs(vref) + 1e-9)
                        print("variance %s %dx%d strict %d it %d prefilter %d demod %d: E32 %.2e (V %.2e), bars %.2e (V %.2e), worst err / bar %.3f (V %.3f)" % (
                            gen, w, h, strict, it, pre, demod, e32, ev32, coef, vcoef, float(ratio.max()), float(vratio.max())))
                        assert (ratio <= 1.0).all(), (gen, kw, int((ratio > 1.0).sum()), float(ratio.max()))
                        assert (vratio <= 1.0).all(), (gen, kw, int((vratio > 1.0).sum()), float(vratio.max()))
                        assert np.array_equal(_bits(out[..., 3]), _bits(hv[0][..., 3]))              # alpha is H1's
                        assert np.array_equal(_bits(out[kept][..., :3]), _bits(mean[kept]))          # misses and emitters carry the plain mean
                        assert (var[kept] == 0).all()
                        if w * h == 1 and gen != "hits":
                            assert np.array_equal(_bits(out[..., :3]), _bits(mean))
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- state-owned entry points
def _read_device_image(c, ptr):
    """The width*height float4 image at a device pointer, through the context's own reader: bound as the accumulation buffer for the copy."""
    c.sync()
    c.bind_accum(ptr)
    try:
        return c.read_accum()
    finally:
        c.bind_accum(None)


def test_state_owned_entry_points_share_one_state(capi, dn, O, cornell):
    """trg_denoise_accum and trg_render_denoised_variance_own (what the engine plugin calls) on one 64 x 48 Cornell context: each equals the
    caller-buffer path bit for bit; plain, variance, plain gives the first result again (neither path clobbers what the other keeps in the
    state: ping, pong, the filter's guide copy, the result image, the guide and half planes); with the state's image bound as the accumulation
    buffer both refuse; and the accumulation buffer and the ray counters are those of a context that never denoised."""
    w, h, spp, bounces = 64, 48, 4, 3
    off = O.pixel_offsets(w, h)
    L = dn.load()
    a = make_ctx(O, cornell, w, h, offsets=off)
    b = make_ctx(O, cornell, w, h, offsets=off)
    rays = lambda s: (s.primary_rays, s.bounce_rays, s.shadow_rays, s.shaded_hits)

    def plain_own(frame=0, **kw):
        p, out = dn.make_params(**kw), C.c_void_p()
        dn._chk(a, L.trg_denoise_accum(a.h_ctx, frame, C.byref(p), C.byref(out)))
        return out.value

    def variance_own(**kw):
        p, out = dn.make_var_params(**kw), C.c_void_p()
        dn._chk(a, L.trg_render_denoised_variance_own(a.h_ctx, 0, spp, bounces, C.byref(p), C.byref(out)))
        return out.value
    try:
        a.render(0, spp, bounces)
        b.render(0, spp, bounces)
        noisy, rays4 = b.read_accum(), rays(b.stats())
        want_plain = dn.denoise(a, a.read_accum(), dn.guides(a, 0))
        want_var = dn.render_denoised_variance(a, 0, spp, bounces)
        variance_calls = 1
        ptr = plain_own()
        first = _read_device_image(a, ptr)
        assert np.array_equal(_bits(first), _bits(want_plain)) and not np.array_equal(_bits(first), _bits(noisy))
        ptr_v = variance_own()
        variance_calls += 1
        assert ptr_v == ptr                                                                   # one image of the state serves both
        var = _read_device_image(a, ptr_v)
        assert np.array_equal(_bits(var), _bits(want_var)) and not np.array_equal(_bits(var), _bits(first))
        assert np.array_equal(_bits(_read_device_image(a, plain_own())), _bits(first))        # plain, variance, plain
        variance_own()
        variance_calls += 1
        assert np.array_equal(_bits(_read_device_image(a, ptr)), _bits(var))
        # other parameters through the same state, then the first again
        assert np.array_equal(_bits(_read_device_image(a, plain_own(iterations=2, demodulate=0))),
                              _bits(dn.denoise(a, noisy, dn.guides(a, 0), iterations=2, demodulate=0)))
        assert np.array_equal(_bits(_read_device_image(a, plain_own())), _bits(first))
        # the state's image bound as the accumulation buffer: refused, and nothing is rendered into it
        a.sync()
        a.bind_accum(ptr)
        try:
            for call in (plain_own, variance_own):
                with pytest.raises(capi.TrgError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID and "bound" in str(e.value)
        finally:
            a.bind_accum(None)
        # the accumulation buffer was only read and the guide rays are not counted.  "The ray counters match a context that never denoised"
        # holds for the plain path as it stands; a variance call renders its two halves, spp frames in all, and those rays are counted like
        # any render's (test_gpu_denoise_variance.py, test_halves_...): so one more multiple of the never-denoised context's per variance call
        assert np.array_equal(_bits(a.read_accum()), _bits(noisy))
        assert rays(a.stats()) == tuple((1 + variance_calls) * v for v in rays4)
        a.render(spp, spp, bounces)
        b.render(spp, spp, bounces)
        assert np.array_equal(_bits(a.read_accum()), _bits(b.read_accum()))
    finally:
        _close(a, dn)
        _close(b, dn)
