"""The scenes of tests/schedule_scenes.py can tell a wrong kernel from a right one (no GPU: the oracle and the host-only entry points).

tests/test_gpu_schedule_scenes.py compares every render schedule with the oracle on these scenes; the conditions here keep those comparisons
from passing vacuously: the pixels that reach the meshes only through bounces >= 1 (which the tail and regeneration kernels shade) are many,
and they change when the textures go, when the weights are ignored (the flattened control) and when the corners are permuted.  The bounds are
conditions the scenes must meet, set well under what the oracle gives on them (in brackets, 48 x 40 and 33 x 17)."""
import ctypes as C

import numpy as np
import pytest

from tests import schedule_scenes as S


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def rooms(built, O):
    b = S.scene("A")[0]
    s = S.oracle_scene(O, b)
    return [S.room_pixels(O, s, w, h) for (w, h, _, _) in S.SHAPES]


def _img(variant, textured, shape):
    return S.reference("A", variant, textured, shape, "TRIG_LIBM")[0]


def test_scene_a_is_what_it_says(built):
    b, uvs, ids, imgs = S.scene("A")
    assert b["material_ids"].shape[0] == 102 and uvs.shape == (306, 2) and [im.shape for im in imgs] == [(64, 64, 4), (37, 37, 4)]
    mesh = slice(3 * S.N_BOX, 3 * 100)
    n, c, t = (a[mesh].reshape(-1, 3, a.shape[-1]) for a in (b["normals"], b["colors"], uvs))
    for a in (n, c, t):                                  # three different normals, colours and uv on every triangle of the sphere
        assert (np.abs(a[:, 0] - a[:, 1]).max(-1) > 1e-3).all() and (np.abs(a[:, 1] - a[:, 2]).max(-1) > 1e-3).all() and (np.abs(a[:, 0] - a[:, 2]).max(-1) > 1e-3).all()
    assert uvs[mesh, 0].max() > 2.0 and uvs[mesh, 1].min() < -0.5          # wraps, goes negative
    assert S.scene("B")[0]["material_ids"].shape[0] == 36 + 1840 + 2
    # the variants move attributes only
    for v in ("flat", "rotated"):
        assert np.array_equal(S.scene("A", v)[0]["positions"], b["positions"])
    bf = S.scene("A", "flat")[0]
    assert np.array_equal(bf["normals"][:108], b["normals"][:108]) and np.array_equal(bf["normals"][108::3], b["normals"][108::3])
    assert np.array_equal(bf["normals"][109::3], b["normals"][108::3]) and np.array_equal(bf["colors"][110::3], b["colors"][108::3])
    br, uvr = S.scene("A", "rotated")[:2]
    assert np.array_equal(br["normals"][108::3], b["normals"][109::3]) and np.array_equal(br["colors"][110::3], b["colors"][108::3])
    assert np.array_equal(uvr[109::3], uvs[110::3]) and np.array_equal(uvr[:108], uvs[:108])


@pytest.mark.parametrize("shape", range(len(S.SHAPES)))
def test_room_pixels_are_many_and_see_the_meshes(rooms, shape):
    room = rooms[shape]
    share = room.mean()
    tex, plain, flat, rot = _img("base", True, shape), _img("base", False, shape), _img("flat", True, shape), _img("rotated", True, shape)
    by_texture, by_weights, by_corners = S.differ(tex, plain)[room].mean(), S.differ(tex, flat)[room].mean(), S.differ(tex, rot).mean()
    print("%dx%d: room pixels %.2f; of them changed by the textures %.2f, by flattening %.2f; all pixels changed by the corner rotation %.2f"
          % (S.SHAPES[shape][0], S.SHAPES[shape][1], share, by_texture, by_weights, by_corners))
    assert share >= 0.40                       # (0.78, 0.49)
    assert by_texture >= 0.10                  # (0.38, 0.66)
    assert by_weights >= 0.10                  # (0.22, 0.35)
    assert by_corners >= 0.01                  # (0.34, 0.30)
    # the untextured scene too depends on the weights and on the corner order (bar C of the GPU tests runs on it)
    assert S.differ(plain, _img("flat", False, shape))[room].mean() >= 0.10
    assert S.differ(plain, _img("rotated", False, shape)).mean() >= 0.01


def test_references_are_computed_once_and_read_only(built):
    a = S.reference("A", "base", True, 0, "TRIG_PORTABLE")
    assert S.reference("A", "base", True, 0, "TRIG_PORTABLE")[0] is a[0] and not a[0].flags.writeable
    assert a[2] == sum(a[1][:3]) and a[2] == 58001
    assert S.reference("A", "base", True, 1, "TRIG_PORTABLE")[2] == 41710
    # portable and libm trig: the same paths, other bits
    b = S.reference("A", "base", True, 0, "TRIG_LIBM")
    assert not np.array_equal(a[0], b[0]) and np.abs(a[0] - b[0]).max() < 1e-2


def test_what_the_flat_attribute_records_make_of_the_scenes(capi):
    """Scene A is generic (not flat), with or without textures: the function sees normals and colours only.  The flattened control IS flat to it --
    one normal and one colour per triangle is all it asks --, so the shipped build would shade the control's untextured form from the flat records:
    the control is used for the oracle comparison above only, never loaded into the library by the GPU tests."""
    for name in ("A", "B"):
        for v in ("base", "rotated"):
            b = S.scene(name, v)[0]
            assert capi.debug_flat_attributes(b["normals"], b["colors"]) == (False, None)
    b = S.scene("A", "flat")[0]
    flat, rec = capi.debug_flat_attributes(b["normals"], b["colors"])
    assert flat and rec.shape == (102, 12)
    for n in (120, 170, 220):
        b = S.edge_scene(n)[0]
        assert not capi.debug_flat_attributes(b["normals"], b["colors"])[0]


def _leaf_records(capi, b):
    L = capi.load()
    pos, nrm, col = (np.ascontiguousarray(b[k], np.float32) for k in ("positions", "normals", "colors"))
    idx, mat = np.ascontiguousarray(b["indices"], np.uint32), np.ascontiguousarray(b["material_ids"], np.uint32)
    n = C.c_uint32()
    args = (pos.ctypes.data, nrm.ctypes.data, col.ctypes.data, idx.ctypes.data, mat.ctypes.data, pos.shape[0], mat.shape[0])
    assert L.trg_debug_leaf_records(*args, None, 0, C.byref(n)) == capi.OK and n.value == mat.shape[0]
    rec = np.zeros((n.value, 32), np.float32)
    assert L.trg_debug_leaf_records(*args, rec.ctypes.data, n.value, C.byref(n)) == capi.OK
    return rec


@pytest.mark.parametrize("variant", ["base", "rotated"])
def test_leaf_records_carry_three_distinct_normals_per_mesh_triangle(capi, variant):
    b = S.scene("A", variant)[0]
    rec = _leaf_records(capi, b)
    prim = rec[:, 3].view(np.uint32)
    assert sorted(prim.tolist()) == list(range(102))
    assert np.array_equal(rec[:, 12:21], b["normals"].reshape(-1, 9)[prim]) and np.array_equal(rec[:, 21:30], b["colors"].reshape(-1, 9)[prim])
    sphere = (prim >= S.N_BOX) & (prim < 100)
    n = rec[sphere, 12:21].reshape(-1, 3, 3)
    assert sphere.sum() == 64
    assert (np.abs(n[:, 0] - n[:, 1]).max(-1) > 1e-3).all() and (np.abs(n[:, 1] - n[:, 2]).max(-1) > 1e-3).all() and (np.abs(n[:, 0] - n[:, 2]).max(-1) > 1e-3).all()
    assert (rec[prim < S.N_BOX, 12:15] == rec[prim < S.N_BOX, 15:18]).all()      # (the box's are the flat ones)


def test_edge_family_grows_by_one_triangle_and_differs_in_every_corner(built):
    a, b = S.edge_scene(150), S.edge_scene(151)
    assert a[0]["material_ids"].shape[0] == 150 and b[0]["material_ids"].shape[0] == 151
    for k in ("positions", "normals", "colors"):
        assert np.array_equal(b[0][k][:450], a[0][k])
    n = b[0]["normals"][108:].reshape(-1, 3, 3)
    c = b[0]["colors"][108:].reshape(-1, 3, 3)
    assert (np.abs(n[:, 0] - n[:, 1]).max(-1) > 1e-3).all() and (np.abs(c[:, 1] - c[:, 2]).max(-1) > 1e-4).all()
    assert (b[2][36::3] == 1).all() and b[2].sum() == len(b[2][36::3]) and b[3][0].shape == (3, 5, 4)
    # its staged size crosses the LDS tier's 40 KiB somewhere inside the family
    sizes = []
    from toyraygun_amd import capi
    for n_t in (min(S.EDGE_N), max(S.EDGE_N)):
        s = S.edge_scene(n_t)[0]
        nodes, recs, _ = capi.debug_build_bvh(s["positions"], s["indices"], s["material_ids"])
        sizes.append(S.staged_bytes(nodes.shape[0], recs.shape[0], n_t))
    assert sizes[0] < 40 * 1024 < sizes[1], sizes


def test_deep_scene_is_small_enough_to_stage_and_too_deep_for_lds_stacks(capi):
    """The host builder's tree of tests/schedule_scenes.py deep_scene: the staged bytes fit the LDS tier (<= 40 KiB), the frame-serial LDS plan
    -- staged bytes, (depth + 2) stack levels of 1 KiB, 128 bytes of reduction scratch -- does not fit 64 KiB."""
    b = S.deep_scene()
    nt = b["material_ids"].shape[0]
    assert nt <= 170
    nodes, recs, depth = capi.debug_build_bvh(b["positions"], b["indices"], b["material_ids"])
    staged = S.staged_bytes(nodes.shape[0], recs.shape[0], nt)
    print("deep scene: %d triangles, %d nodes, depth %d, %d bytes staged" % (nt, nodes.shape[0], depth, staged))
    assert staged <= 40 * 1024
    assert staged + (depth + 2) * S.LDS_STACK_LEVEL_BYTES + 128 > S.LDS_LIMIT + 1024      # by more than one level
    assert not capi.debug_flat_attributes(b["normals"], b["colors"])[0]
    tri = b["positions"].reshape(-1, 3, 3).astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area > 1e-37).all()              # no triangle's area falls out of fp32's normal range
