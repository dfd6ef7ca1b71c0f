"""The two float64 readings of include/trg_denoise.h against each other (no GPU): toyraygun_amd/denoise.py's vectorised reference, which the GPU
tests compare the kernels with, and tests/denoise_literal.py, written once more from the header's text one pixel and one tap at a time.  Both are
float64 and differ in summation order only, so they agree to 1e-12; a disagreement means one of them misread the header."""
import numpy as np
import pytest

from tests import denoise_literal as lit
from tests.test_gpu_denoise import _smooth, _smooth_hits, _synthetic
from tests.test_gpu_denoise_variance import _synthetic_halves
from toyraygun_amd import denoise as dn

SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (15, 17), (16, 16), (17, 33)]     # w x h
ITERATIONS = (1, 2, 3, 6)
GENERATORS = {"synthetic": _synthetic, "smooth": _smooth}


def _inputs(gen, size):
    """The generator's input; at 1 x 1, where its one pixel is a miss, also the 1 x 1 image whose pixel is a hit (_smooth_hits)."""
    return [GENERATORS[gen]] + ([_smooth_hits] if size == (1, 1) and gen == "smooth" else [])


def _agree(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = ~(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b)))
    assert not bad.any(), "%s: %d values differ, worst %.3e" % (what, int(bad.sum()), float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()))


@pytest.mark.parametrize("gen", sorted(GENERATORS))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_plain_filter_literal_and_vectorised_agree(cornell, size, gen):
    """Iterations 1, 2, 3, 6 x demodulate x with / without the scene's material ids (with them the block whose first hit is the light is kept
    out like the misses), on _synthetic's and _smooth's inputs: |a - b| <= 1e-12 max(1, |b|) on every value."""
    w, h = size
    for make in _inputs(gen, size):
        color, g0, g1 = make(w, h, 11)
        for mats in (None, cornell.buffers()["material_ids"]):
            for demod in (0, 1):
                runs = lit.literal_denoise(color, g0, g1, iterations=6, demodulate=demod, material_ids=mats, every=True)
                for it in ITERATIONS:
                    ref = dn.reference_denoise(color, g0, g1, iterations=it, demodulate=demod, material_ids=mats)
                    _agree(runs[it], ref, "%s %dx%d it %d demod %d mats %s" % (make.__name__, w, h, it, demod, mats is not None))
                    if w * h == 1 and make is _smooth_hits and demod == 0:
                        # one hit pixel, the centre tap alone: its result is its colour (to the rounding of (w c) / w)
                        assert np.allclose(ref[..., :3], color[..., :3].astype(np.float64), rtol=1e-15, atol=0)
        assert np.array_equal(lit.literal_denoise(color, g0, g1, iterations=0), color.astype(np.float64))


@pytest.mark.parametrize("gen", sorted(GENERATORS))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_variance_filter_literal_and_vectorised_agree(cornell, size, gen):
    """The same for trg_denoise_variance, x prefilter 0 / 1, the image and the carried variance V_N; iterations 0 (the plain mean, V_0) as well."""
    w, h = size
    for make in _inputs(gen, size):
        hv, g0, g1 = _synthetic_halves(w, h, gen=make)
        for mats in (None, cornell.buffers()["material_ids"]):
            for demod in (0, 1):
                for pre in (0, 1):
                    runs = lit.literal_denoise_variance(hv[0], hv[1], g0, g1, iterations=6, demodulate=demod, prefilter=pre, material_ids=mats, every=True)
                    for it in (0,) + ITERATIONS:
                        ref, vref = dn.reference_denoise_variance(hv[0], hv[1], g0, g1, iterations=it, demodulate=demod, prefilter=pre,
                                                                  material_ids=mats, return_variance=True)
                        what = "%s %dx%d it %d demod %d prefilter %d mats %s" % (make.__name__, w, h, it, demod, pre, mats is not None)
                        _agree(runs[it][0], ref, what)
                        _agree(runs[it][1], vref, what + " (variance)")


def test_the_inputs_reach_what_they_are_for(cornell):
    """_smooth: normal lengths in [0.97, 1] and dot products near but not equal to 1; albedo clamped on about a tenth of the pixels; a region of
    depth gradient exactly 0; misses and emitters present; and every weight sum of the reference stays far from fp32 underflow (the centre tap
    alone weighs 9/64 |n|^256 >= 5.8e-5), so `sum of weights > 0` is no knife edge in these tests."""
    mats = cornell.buffers()["material_ids"]
    color, g0, g1 = _smooth(48, 32, 11)
    hit = g0[..., 3] >= 0
    ln = np.sqrt((g0[..., :3].astype(np.float64) ** 2).sum(-1))[hit]
    assert 0.97 - 1e-6 <= ln.min() and ln.max() <= 1.0 + 1e-6 and ln.std() > 0.005
    d = (g0[:, 1:, :3].astype(np.float64) * g0[:, :-1, :3]).sum(-1)[hit[:, 1:] & hit[:, :-1]]
    assert ((d > 0.9) & (d < 1.0)).mean() > 0.8 and len(np.unique(d)) > 0.5 * d.size
    zero = (g1[..., :3] == 0).all(-1) & hit
    assert 0.05 < zero.mean() < 0.2
    assert (dn._depth_gradient(g0[..., 3].astype(np.float64))[hit] == 0).sum() > 20
    assert dn.emitter_mask(g1, mats).sum() > 20 and (~hit).sum() == 42
    for w, h in SHAPES + [(32, 16), (48, 32)]:
        color, g0, g1 = _smooth(w, h, 11)
        g = g0.astype(np.float64)
        g[dn.emitter_mask(g1, mats), 3] = -1.0
        keep = g[..., 3] >= 0
        I = color[..., :3].astype(np.float64)
        for i in range(6):
            ws = dn.atrous_weights(I, g, 1 << i, 4.0, 128.0, 1.0).sum((0, 1))
            assert not keep.any() or ws[keep].min() >= 5.8e-5, (w, h, i, float(ws[keep].min()))


def test_float32_mode_of_the_vectorised_reference():
    """dtype=np.float32: fp32 results close to the float64 ones (they are the yardstick of the GPU tests' bars), the default stays float64."""
    color, g0, g1 = _smooth(17, 33, 11)
    hv, _, _ = _synthetic_halves(17, 33, gen=_smooth)
    a, b = dn.reference_denoise(color, g0, g1, iterations=3), dn.reference_denoise(color, g0, g1, iterations=3, dtype=np.float32)
    assert a.dtype == np.float64 and b.dtype == np.float32
    assert 0 < np.abs(a - b).max() < 1e-4
    a, av = dn.reference_denoise_variance(hv[0], hv[1], g0, g1, iterations=3, return_variance=True)
    b, bv = dn.reference_denoise_variance(hv[0], hv[1], g0, g1, iterations=3, return_variance=True, dtype=np.float32)
    assert a.dtype == av.dtype == np.float64 and b.dtype == bv.dtype == np.float32
    assert 0 < np.abs(a - b).max() < 1e-4 and (np.abs(av - bv) <= 1e-3 * np.abs(av) + 1e-9).all()
    # sigma_normal == 0: x ** 0 = exp2(0 * log2 x) = 1 in both modes
    for t in (np.float64, np.float32):
        W = dn.geometry_weights(g0.astype(t), 1, 0.0, 1e30, dtype=t)
        assert set(np.unique(W[2, 2])) <= {0.0, t(9.0 / 64.0)}
    with pytest.raises(ValueError):
        dn.reference_denoise(color, g0, g1, dtype=np.float16)
