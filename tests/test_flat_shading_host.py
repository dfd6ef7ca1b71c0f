"""Flat-attribute records (include/trg.h trg_debug_flat_attributes; no GPU): which scenes the shipped build's LDS kernels shade from one
(unit normal | r) (right | g) (forward | b) record per triangle, and what the records hold -- the frame of align_hemisphere (common.h:95-110)
recomputed here in float64."""
import numpy as np
import pytest

HELPER = np.array([0.0072, 1.0, 0.0034], np.float64)


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def box(O, cornell):
    b = cornell.buffers()
    return np.array(b["normals"], np.float32).reshape(-1, 9), np.array(b["colors"], np.float32).reshape(-1, 9)


def _check_records(rec, nrm, col):
    """Every record against the float64 frame of its triangle's normal, to 1e-6; the colour exactly."""
    n = nrm[:, :3].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    right = np.cross(n, HELPER)
    right /= np.linalg.norm(right, axis=1, keepdims=True)
    forward = np.cross(right, n)
    N, R, F = rec[:, 0:3].astype(np.float64), rec[:, 4:7].astype(np.float64), rec[:, 8:11].astype(np.float64)
    assert np.abs(N - n).max() <= 1e-6 and np.abs(R - right).max() <= 1e-6 and np.abs(F - forward).max() <= 1e-6
    assert np.abs(np.linalg.norm(N, axis=1) - 1.0).max() <= 1e-6 and np.abs(np.linalg.norm(R, axis=1) - 1.0).max() <= 1e-6
    assert np.abs((N * R).sum(1)).max() <= 1e-6
    assert np.abs(F - np.cross(R, N)).max() <= 1e-6
    assert np.array_equal(rec[:, [3, 7, 11]].view(np.uint32), col[:, :3].view(np.uint32))


def test_cornell_box_is_flat_and_its_records_are_the_reference_frame(capi, box):
    nrm, col = box
    flat, rec = capi.debug_flat_attributes(nrm, col)
    assert flat and rec.shape == (nrm.shape[0], 12) and nrm.shape[0] == 36
    _check_records(rec, nrm, col)


def test_normal_length_does_not_matter(capi, box):
    nrm, col = box
    flat1, rec1 = capi.debug_flat_attributes(nrm, col)
    flat3, rec3 = capi.debug_flat_attributes(nrm * np.float32(3.0), col)
    assert flat1 and flat3
    assert np.abs(rec3[:, 0:3].astype(np.float64) - rec1[:, 0:3].astype(np.float64)).max() <= 1e-6
    _check_records(rec3, nrm * np.float32(3.0), col)


def test_oblique_normals_and_a_colour_per_triangle(capi):
    rng = np.random.default_rng(5)
    n = rng.normal(size=(200, 3)).astype(np.float32) * rng.uniform(0.1, 4.0, (200, 1)).astype(np.float32)
    c = rng.uniform(0.0, 1.0, (200, 3)).astype(np.float32)
    nrm, col = np.tile(n, (1, 3)), np.tile(c, (1, 3))
    flat, rec = capi.debug_flat_attributes(nrm, col)
    assert flat
    _check_records(rec, nrm, col)


@pytest.mark.parametrize("case", ["normal_one_ulp", "colour", "zero_normal", "nan_normal", "inf_normal", "helper_axis", "minus_helper_axis"])
def test_one_doubtful_triangle_makes_the_scene_generic(capi, box, case):
    nrm, col = box[0].copy(), box[1].copy()
    t = 17
    if case == "normal_one_ulp":       # vertex 2's normal differs from the others in the last bit of one component
        k = int(np.argmax(np.abs(nrm[t, 6:9])))
        nrm[t, 6 + k] = np.nextafter(nrm[t, 6 + k], np.float32(2.0) * nrm[t, 6 + k])
        assert nrm[t, 6 + k] != nrm[t, k]
    elif case == "colour":
        col[t, 4] = np.nextafter(col[t, 4], np.float32(2.0))
    elif case == "zero_normal":
        nrm[t] = 0.0
    elif case == "nan_normal":
        nrm[t, 0::3] = np.nan              # the same NaN at all three vertices: bitwise equal, still not a normal
    elif case == "inf_normal":
        nrm[t, 1::3] = np.inf
    elif case == "helper_axis":          # cross(N, helper) = 0: the reference's frame is undefined there
        nrm[t] = np.tile(HELPER.astype(np.float32), 3)
    else:
        nrm[t] = np.tile(-HELPER.astype(np.float32), 3)
    flat, rec = capi.debug_flat_attributes(nrm, col)
    assert not flat and rec is None
    assert capi.debug_flat_attributes(box[0], box[1])[0]       # (the untouched scene still is)


def test_near_the_helper_axis_the_threshold_is_the_stated_one(capi):
    """|cross(N, helper)| = sin(angle to the helper axis): flat at 2e-3, generic at 5e-4 (the bar is 1e-3)."""
    h = HELPER / np.linalg.norm(HELPER)
    side = np.cross(h, [1.0, 0.0, 0.0]); side /= np.linalg.norm(side)
    col = np.full((1, 9), 0.5, np.float32)
    for s, want in ((2e-3, True), (5e-4, False)):
        n = (h * np.sqrt(1.0 - s * s) + side * s).astype(np.float32)
        assert capi.debug_flat_attributes(np.tile(n, 3)[None], col)[0] == want, s


def test_switch_and_empty_scene(capi, box, monkeypatch):
    assert not capi.debug_flat_attributes(np.zeros((0, 9), np.float32), np.zeros((0, 9), np.float32))[0]
    monkeypatch.setenv("TRG_FLAT_SHADING", "0")
    assert not capi.debug_flat_attributes(box[0], box[1])[0]
    monkeypatch.setenv("TRG_FLAT_SHADING", "1")
    assert capi.debug_flat_attributes(box[0], box[1])[0]
