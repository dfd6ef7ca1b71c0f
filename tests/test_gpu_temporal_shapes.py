"""GPU tests (-m gpu) of the temporal step (trg_temporal_denoise: dn_temporal_reproject_kernel, dn_temporal_spatial_kernel, dn_temporal_finish_kernel) where
tests/test_gpu_temporal.py does not go: synthetic frames and matrices (tests/test_temporal_synthetic_host.py has the generators and says what they
hold), every shape of tests/test_gpu_denoise_shapes.py, every field of trg_temporal_params away from its default, a history length of exactly 4, and
the temporal path sharing one state with the other filters.

Every step goes through trg_temporal_denoise_host and trg_temporal_history_read and is compared with reference_temporal evaluated from the DEVICE's own
previous history (Hc, Hm read back; F = the filter's G0 with the emitters marked; X as supplied), under the bar rule of tests/test_gpu_temporal.py,
unchanged (step_reference in the host module): E32 from the reference's float32 mode, max(1e-4, 4 E32) on colour, on N and on the moments,
max(1e-3, 4 E32) relative + 1e-9 on V_0, only where `near` is false, for V_0 also `near_n`.  Nothing in a bar comes from the device.

MEASURED on an MI355X (error / bar, worst over the calls and both settings): see DESIGN.md, "Denoiser"."""
import hashlib

import numpy as np
import pytest

from tests.test_gpu_denoise import _bits, _close, _synthetic
from tests.test_gpu_denoise_variance import _synthetic_halves
from tests.test_gpu_temporal import _filter_g0
from tests.test_temporal_synthetic_host import (IDENTITY_SCHEDULE, IDENTITY_SHAPES, INVISIBLE, ONE_STATE_SCHEDULE, ONE_STATE_SHAPE, PARAM_SETS, SCHEDULE,
                                                SHAPES, SHAPES_PARAMS, TURNS_FOUR, _max, census, near_caps, schedule_frames, spatial_form, step_ratios,
                                                step_reference, varied_fields, visible_fields)
from tests.util import make_ctx

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = ("Hc.rgb", "N", "Hm", "I", "V")


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


_refs = {}


def _ref(dn, case, call, frame, prev, mats, params, **kw):
    """step_reference of one call of one case, computed once for both settings -- as long as both hand it the same previous history, bit for bit."""
    key = (case, call, hashlib.sha1(b"" if prev is None else np.ascontiguousarray(prev).tobytes()).hexdigest())
    if key not in _refs:
        _refs[key] = step_reference(dn, frame, prev, mats, params, **kw)
    return _refs[key]


def _step(dn, c, mats, frame, params):
    """One call on the device: (out, iv, the new history planes as the next call's reference reads them)."""
    colour, g, X, vp, cam = frame
    out, iv = dn.temporal_denoise(c, colour, g, X, vp, return_iv=True, **params)
    hist = dn.temporal_history(c)
    return out, iv, np.stack([hist[0], hist[1], _filter_g0(dn, g, mats), X])


def _compare(tag, call, R, planes, iv, turns_four=TURNS_FOUR):
    """The caps on near and near_n, then every plane of the step within its bar on the compared pixels."""
    near_caps(R["near"], R["near_n"], call, turns_four)
    ratios = step_ratios(R, planes[0], planes[1], iv)
    worst = [_max(r) for r in ratios]
    print("%s call %d: near %d, near_n %d of %d pixels; E32 colour %.2e N %.2e moments %.2e V %.2e; worst err / bar: %s" % (
        tag, call, R["near"].sum(), R["near_n"].sum(), R["near"].size, R["e32"][0], R["e32"][1], R["e32"][2], R["e32"][3],
        " ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, worst))))
    for name, r in zip(NAMES, ratios):
        assert (r <= 1.0).all(), (tag, call, name, int((r > 1).sum()), float(r.max()))
    assert np.array_equal(_bits(iv[..., :3]), _bits(planes[0][..., :3]))                                  # (I, V_0) carries the history's colour
    return worst


def _finish(dn, frame, out, iv, mats, demod):
    """iterations = 0: out is (I, V_0) remodulated, bit for bit, with the input's alpha; misses and emitters copy their input."""
    colour, g = frame[0], frame[1]
    kept = (g[0, ..., 3] < 0) | dn.emitter_mask(g[1], mats)
    alb = np.maximum(g[1, ..., :3], f32(1e-3))
    want = np.where(kept[..., None], iv[..., :3], iv[..., :3] * alb) if demod else iv[..., :3]
    assert np.array_equal(_bits(out[..., :3]), _bits(want.astype(f32)))
    assert np.array_equal(_bits(out[..., 3]), _bits(colour[..., 3]))
    assert np.array_equal(_bits(out[kept]), _bits(colour[kept])) and (iv[kept][:, 3] == 0).all()


def _ctx(O, cornell, w, h, capi, strict, offsets=None):
    c = make_ctx(O, cornell, w, h, offsets=offsets)
    c.set_option(capi.OPT_STRICT, strict)
    return c, cornell.buffers()["material_ids"]


def _run_schedule(dn, c, mats, tag, case, w, h, params, visible=None):
    """SCHEDULE on the device, every call compared from the device's own previous history; returns the worst err / bar per plane."""
    prev, worst = None, [0.0] * 5
    populations = dict(found=0, lost=0, lt4=0, ge4=0)
    for call, frame in enumerate(schedule_frames(w, h, SCHEDULE)):
        out, iv, planes = _step(dn, c, mats, frame, params)
        R = _ref(dn, case, call, frame, prev, mats, params)
        worst = [max(a, b) for a, b in zip(worst, _compare(tag, call, R, planes, iv))]
        _finish(dn, frame, out, iv, mats, params.get("demodulate", 1))
        if visible is not None:
            visible |= visible_fields(dn, R, frame, prev, mats, params)
        N, hit = planes[0, ..., 3], planes[2, ..., 3] >= 0
        cen = census(dn, frame[1], frame[2], prev, frame[3], mats, **params)
        assert (N[~hit] == 0).all() and (N[cen["zero"]] == 1).all()
        if frame[4] in (None, "out"):
            assert (N[hit] == 1).all()                                                                       # no history anywhere
        populations["found"] += int((cen["found"] & R["ok"]).sum())
        populations["lost"] += int((cen["front"] & ~cen["found"] & R["ok"]).sum())
        populations["lt4"] += int((hit & (N < 4)).sum())
        populations["ge4"] += int((hit & (N >= 4)).sum())
        prev = planes
    print("%s: worst err / bar over the schedule: %s; compared pixels with history %d, looking for it in vain %d; N < 4 on %d, N >= 4 on %d" % (
        tag, " ".join("%s %.3f" % (n, v) for n, v in zip(NAMES, worst)), populations["found"], populations["lost"], populations["lt4"], populations["ge4"]))
    return worst, populations


# ---------------------------------------------------------------------------------------------------------------------------- a. every shape
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_step_at_every_shape(capi, dn, O, cornell, size, strict):
    """SCHEDULE (nine calls, two stages, the five matrices) with max_history = 6 and iterations = 0 at the nine shapes: 1 x 1, one pixel wide or
    high, smaller than a tile, exact tile multiples, one pixel more than a tile.  Every call against the reference; out against (I, V_0)
    remodulated bit for bit (the finish kernel)."""
    w, h = size
    params = dict(SHAPES_PARAMS, iterations=0)
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    try:
        worst, pop = _run_schedule(dn, c, mats, "temporal shapes %dx%d strict %d" % (w, h, strict), ("shapes", size), w, h, params)
        if w * h >= 255:
            assert pop["found"] > 0.2 * w * h and pop["lost"] > 0 and pop["lt4"] > 0 and pop["ge4"] > 0
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- b. every parameter
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_step_with_every_parameter_off_its_default(capi, dn, O, cornell, name, strict):
    """17 x 33, SCHEDULE under the four parameter sets of the host module: every field but `iterations` differs from the default and between the
    sets.  Per set, and from the reference alone: putting any one varied field back to its default moves some compared pixel of some call by
    more than that call's bar -- the test can see the field -- except where the definition itself hides it (INVISIBLE in the host module says
    which and why: sigma_lum at iterations = 0; alpha, alpha_moments and the two tap tolerances once alpha = alpha_moments = max_history = 1)."""
    w, h = 17, 33
    params = dict(PARAM_SETS[name], iterations=0)
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    try:
        visible = set()
        _run_schedule(dn, c, mats, "temporal parameters %s strict %d" % (name, strict), ("parameters", name), w, h, params, visible=visible)
        varied = set(varied_fields(dn, params))
        print("temporal parameters %s: varied %s; hidden by the definition %s" % (name, sorted(varied), sorted(INVISIBLE[name])))
        assert varied >= set(PARAM_SETS[name]) - {"demodulate"}
        assert visible >= varied - INVISIBLE[name], sorted(varied - INVISIBLE[name] - visible)
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- c. N exactly 4
@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", IDENTITY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_history_of_exactly_four_frames(capi, dn, O, cornell, size, strict):
    """ortho_vp(w, h, 0, 0) at powers of two, one stage, six calls: every sample lands on a pixel centre (fx = x exactly, in fp32 and float64), the
    one contributing tap has weight 1, and N is 1, 2, 3, 4, 5, 6 BIT FOR BIT on every hit with a normal, 1 on the zero normals, 0 on misses and
    emitters.  In the fourth call both precisions of the reference have N == 4 exactly, so which form V_0 takes is decided: it is compared on
    every pixel that is not `near`, near_n ignored -- after the reference alone has shown the two forms more than the bar apart on half of them."""
    w, h = size
    params = dict(iterations=0)
    c, mats = _ctx(O, cornell, w, h, capi, strict)
    try:
        prev = None
        for call, frame in enumerate(schedule_frames(w, h, IDENTITY_SCHEDULE)):
            out, iv, planes = _step(dn, c, mats, frame, params)
            R = _ref(dn, ("identity", size), call, frame, prev, mats, params, ignore_near_n=(call == 3))
            cen = census(dn, frame[1], frame[2], prev, frame[3], mats)
            N, normal = planes[0, ..., 3], cen["hit"] & ~cen["zero"]
            assert normal.any() and np.array_equal(_bits(N[normal]), _bits(np.full(int(normal.sum()), call + 1, f32)))
            assert np.array_equal(_bits(N[cen["zero"]]), _bits(np.ones(int(cen["zero"].sum()), f32)))
            assert np.array_equal(_bits(N[~cen["hit"]]), _bits(np.zeros(int((~cen["hit"]).sum()), f32)))
            assert (R["new"][0, ..., 3][normal] == call + 1).all() and (R["n32"][0, ..., 3][normal] == call + 1).all() and R["n32"].dtype == np.float32
            if call == 3:
                assert np.array_equal(R["okv"], R["ok"]) and R["near_n"][normal].all()
                temporal, spatial = R["iv"][..., 3], spatial_form(dn, R["new"], params)
                far = (np.abs(spatial - temporal) > R["bars"][3] * np.abs(temporal) + 1e-9)[R["ok"] & normal]
                print("temporal identity %dx%d: the two forms of V_0 are more than the bar apart on %.3f of the %d compared hits with N = 4" % (w, h, far.mean(), far.size))
                assert far.mean() >= 0.5
            _compare("temporal identity %dx%d strict %d" % (w, h, strict), call, R, planes, iv)
            _finish(dn, frame, out, iv, mats, 1)
            prev = planes
    finally:
        _close(c, dn)


# ---------------------------------------------------------------------------------------------------------------------------- d. one state
@pytest.mark.parametrize("strict", [1, 0])
def test_temporal_path_shares_its_state_with_the_other_filters(capi, dn, O, cornell, strict):
    """37 x 29, four temporal calls (three iterations: ping, pong and the filter's guide copy are all in use) in two contexts.  Context A runs
    trg_denoise, trg_denoise_variance (synthetic halves) and trg_render_denoised between them, context B none of them: outputs, (I, V_0) and
    histories are equal bit for bit after every call; and what A's other calls returned is what a third context returns that runs them alone."""
    w, h = ONE_STATE_SHAPE
    off = O.pixel_offsets(w, h)
    (a, mats), (b, _), (alone, _) = (_ctx(O, cornell, w, h, capi, strict, offsets=off) for _ in range(3))
    colour, g0, g1 = _synthetic(w, h, 11)
    halves, hg0, hg1 = _synthetic_halves(w, h)

    def others(c, call):
        return [dn.denoise(c, colour, np.stack([g0, g1]), iterations=2 + call % 3),
                dn.denoise_variance(c, halves, np.stack([hg0, hg1]), iterations=1 + call, return_variance=True)[0],
                dn.render_denoised(c, 0, 2, 3, iterations=5 - call)]
    try:
        prev = None
        for call, frame in enumerate(schedule_frames(w, h, ONE_STATE_SCHEDULE)):
            params = dict(iterations=3)
            got = [_step(dn, c, mats, frame, params) for c in (a, b)]
            for x, y in zip(*got):
                assert np.array_equal(_bits(x), _bits(y)), call
            assert not np.array_equal(_bits(got[0][0]), _bits(frame[0]))                                    # and it did filter
            R = _ref(dn, ("one state",), call, frame, prev, mats, params)
            _compare("temporal one state strict %d" % strict, call, R, got[0][2], got[0][1], turns_four=3)
            prev = got[0][2]
            mine, theirs = others(a, call), others(alone, call)
            for k, (x, y) in enumerate(zip(mine, theirs)):
                assert np.array_equal(_bits(x), _bits(y)), (call, k)
            assert not np.array_equal(_bits(mine[0]), _bits(colour)) and not np.array_equal(_bits(mine[0]), _bits(mine[1]))
    finally:
        for c in (a, b, alone):
            _close(c, dn)
