"""GPU tests (-m gpu) of who owns the denoiser's and the refit unit's per-context state: the context (trg_ctx::denoise, trg_ctx::refit in
csrc/trg_ctx.h).  trg_destroy frees it, so nothing of a destroyed context -- temporal history, the lag / variance-of-mean / coverage settings, the
last refit -- can reach a later context, whatever address the allocator hands that one; trg_denoise_release / trg_refit_release still free early.

Every "destroy" here is WITHOUT a release: Context.close() and Group.close() call trg_destroy / trg_group_destroy and nothing else.

The Cornell box at 48 x 32 and at 33 x 17 (partial 16 x 16 tiles), 1 sample per pixel, 2 bounces.  A first temporal frame has no history, so two
contexts with the same parameters give the same bits in the strict and in the shipped setting: the comparisons are exact.

The two leak tests are REGRESSION GUARDS for the state on the context, not a demonstration of the earlier fault: the table keyed by the context's
address, which this replaced, handed a dead context's state on only when the allocator returned the same address to a context of the same device
and size, which no allocator promises."""
import numpy as np
import pytest

from tests.util import make_ctx

pytestmark = pytest.mark.gpu

SIZES = [(48, 32), (33, 17)]
SPP, BOUNCES = 1, 2
LAG, COVERAGE = 3.0, 0.25             # non-default: a new context has -1 (off), variance-of-mean off, -1 (off)


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


@pytest.fixture(scope="module")
def refit(capi):
    from toyraygun_amd import refit as r
    r.load()
    return r


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(capi, O, cornell, size, strict):
    c = make_ctx(O, cornell, size[0], size[1])
    c.set_option(capi.OPT_STRICT, strict)
    return c


def _settings(dn, c):
    return dn.temporal_lag_correction(c), dn.temporal_variance_of_mean(c), dn.temporal_coverage(c)


def _moved(cornell):
    b = cornell.buffers()
    pos = np.array(b["positions"], np.float32).reshape(-1, 3)
    pos[:, 0] += np.float32(0.01)
    return pos, b["normals"], b["indices"]


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_temporal_history_and_settings_end_with_the_context(capi, dn, O, cornell, size, strict):
    """C, created and closed before A exists, gives the first temporal frame of a fresh context.  A gets the three settings and two temporal
    frames and is destroyed.  B, same device and size, reports the defaults and its first temporal frame is C's, bit for bit."""
    c = _ctx(capi, O, cornell, size, strict)
    try:
        first = dn.render_temporal(c, 0, SPP, BOUNCES)
    finally:
        c.close()
    a = _ctx(capi, O, cornell, size, strict)
    try:
        dn.temporal_set_lag_correction(a, LAG)
        dn.temporal_set_variance_of_mean(a, True)
        dn.temporal_set_coverage(a, COVERAGE)
        assert _settings(dn, a) == (LAG, True, COVERAGE)
        dn.render_temporal(a, 0, SPP, BOUNCES)
        dn.render_temporal(a, SPP, SPP, BOUNCES)
    finally:
        a.close()
    b = _ctx(capi, O, cornell, size, strict)
    try:
        assert _settings(dn, b) == (-1.0, False, -1.0)
        assert np.array_equal(_bits(dn.render_temporal(b, 0, SPP, BOUNCES)), _bits(first))
        assert _settings(dn, b) == (-1.0, False, -1.0)
    finally:
        b.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_last_refit_ends_with_the_context(capi, refit, O, cornell, size):
    pos, nrm, idx = _moved(cornell)
    a = _ctx(capi, O, cornell, size, 0)
    try:
        refit.refit_scene(a, pos, nrm, idx)
        assert refit.refit_last(a)["path"] != refit.NONE
    finally:
        a.close()
    b = _ctx(capi, O, cornell, size, 0)
    try:
        info = refit.refit_last(b)
        assert info["path"] == refit.NONE and info["n_records"] == 0 and info["ms"] == 0.0 and info["area_ratio"] == 0.0
    finally:
        b.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_release_frees_early_and_the_context_goes_on(capi, dn, refit, O, cornell, size):
    """Release on a context that never denoised or refitted is OK; denoise, release, denoise again gives the first result's bits (the state is
    made again on first use); a refit after a release works and a release forgets the last one; destroy after release is clean."""
    L = dn.load()
    c = _ctx(capi, O, cornell, size, 0)
    try:
        assert L.trg_denoise_release(c.h_ctx) == capi.OK and L.trg_refit_release(c.h_ctx) == capi.OK
        one = dn.render_denoised(c, 0, SPP, BOUNCES)
        assert L.trg_denoise_release(c.h_ctx) == capi.OK
        two = dn.render_denoised(c, 0, SPP, BOUNCES)
        assert np.array_equal(_bits(one), _bits(two))
        pos, nrm, idx = _moved(cornell)
        refit.refit_scene(c, pos, nrm, idx)
        assert refit.refit_last(c)["path"] != refit.NONE
        assert L.trg_refit_release(c.h_ctx) == capi.OK
        assert refit.refit_last(c)["path"] == refit.NONE
        refit.refit_scene(c, pos, nrm, idx)
        assert L.trg_denoise_release(c.h_ctx) == capi.OK and L.trg_refit_release(c.h_ctx) == capi.OK
        assert L.trg_denoise_release(c.h_ctx) == capi.OK and L.trg_refit_release(c.h_ctx) == capi.OK      # (nothing left: still OK)
    finally:
        c.close()


def test_group_contexts_own_their_refit_state(capi, refit, O, cornell, monkeypatch):
    """A refit through a two-context group on the one device; the group is destroyed and made again: no context of the new group has refitted."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    w, h = SIZES[0]
    b = cornell.buffers()
    pos, nrm, idx = _moved(cornell)

    def group():
        g = capi.Group([0, 0], w, h)
        g.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        return g
    g = group()
    try:
        refit.refit_scene(g, pos, nrm, idx)
        assert refit.refit_last(g, 0)["path"] != refit.NONE and refit.refit_last(g, 1)["path"] != refit.NONE
    finally:
        g.close()
    g = group()
    try:
        for rank in (0, 1):
            info = refit.refit_last(g, rank)
            assert info["path"] == refit.NONE and info["n_records"] == 0 and info["ms"] == 0.0
    finally:
        g.close()
