"""The ROOM on the host (no GPU): what the builder finds (bvh_build.cpp room_group through trg_debug_room), what it refuses, that scenes outside the
LDS tier keep the blob they had, and the open-box rule as a float64 model against the room's quads tested one by one."""
import json
import os

import numpy as np
import pytest

from tests import room_scenes as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "room_parent_blobs.json")


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def _room(capi, scene):
    b = scene.buffers() if hasattr(scene, "buffers") else scene
    return capi.debug_room(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])


def _corners_local(b, r):
    first = r["first_tri"]
    P = b["positions"].reshape(-1, 3)[b["indices"].reshape(-1)].reshape(-1, 3, 3)[first:first + 2 * r["n_faces"]].reshape(-1, 3).astype(np.float64)
    return (P - r["center"].astype(np.float64)) @ r["axis"].astype(np.float64).T


def test_cornell_box_room(capi, O, cornell):
    b = cornell.buffers()
    r = _room(capi, cornell)
    assert r["n_faces"] == 5 and r["first_tri"] == 24 and r["mask"] == 1 and r["lds_candidate"] == 1
    assert r["present"] == 0b011111                                   # the face at local +z is absent: the camera looks in through it
    assert r["rest_prims"] == 3 and r["rest_kind"] == 1                # two boxes and the light under a node of their own
    l = _corners_local(b, r)
    assert l.shape == (30, 3) and np.abs(np.abs(l) - 1.0).max() <= 1e-5
    assert np.abs(r["axis"] - np.eye(3)).max() < 1e-6                  # axis-aligned walls: local x, y, z = world x, y, z
    # every present face names a different quad of the five
    offs = sorted(int(r["face_rec"][f]) for f in range(6) if r["present"] >> f & 1)
    assert offs == [0, 2, 4, 6, 8]
    # the records: the room's ten behind everything else
    _, tris, _ = capi.debug_build_bvh(b["positions"], b["indices"], b["material_ids"])
    assert r["first_rec"] == tris.shape[0] - 10


@pytest.mark.parametrize("kind", ["rotated", "sheared", "mirrored"])
@pytest.mark.parametrize("faces", [R.CORNER, R.U_SHAPE, R.TUBE, R.FOUR, R.OPEN_FRONT], ids=["corner3", "u3", "tube4", "four4", "open5"])
@pytest.mark.parametrize("pattern", [1, 2])
def test_rooms_found(capi, O, kind, faces, pattern):
    C, H = R.frame(kind)
    s = O.OracleScene()
    order = list(faces)
    np.random.default_rng(len(faces) * 7 + pattern).shuffle(order)     # (the faces in any order in the index buffer)
    R.add_room(s, C, H, order, mat=1 + (len(faces) + pattern) % 3, pattern=pattern)
    R.add_zoo_cubes(O, s)
    r = _room(capi, s)
    assert r["n_faces"] == len(faces) and r["first_tri"] == 0 and r["mask"] == 1 + (len(faces) + pattern) % 3
    perm, sign, dev = R.match_frame(C, H, r["center"], r["axis"])
    assert dev < 1e-5 and sorted(perm.tolist()) == [0, 1, 2]
    assert R.builder_faces(r["present"], perm, sign) == tuple(sorted(faces))
    assert np.abs(np.abs(_corners_local(s.buffers(), r)) - 1.0).max() <= 1e-5
    assert r["rest_prims"] == 6 and r["rest_kind"] == 1


def _aligned_room(O, faces=R.OPEN_FRONT, **kw):
    s = O.OracleScene()
    C, H = R.frame("rotated")
    R.add_room(s, C, H, faces, **kw)
    return s


def test_no_room(capi, O, monkeypatch):
    assert _room(capi, _aligned_room(O))["n_faces"] == 5               # control
    # one corner moved by 1e-3 (the quad stays a parallelogram only if two corners move: move the shared edge of the pair's diagonal corner)
    C, H = R.frame("rotated")
    for corner in range(4):
        s = O.OracleScene()
        R.add_room(s, C, H, R.CORNER, nudge=(1, corner, (1e-3, 0.0, 0.0)))
        assert _room(capi, s)["n_faces"] == 0, corner
    # a whole face moved by 1e-3 along its normal: still three parallelograms, no longer faces of one parallelepiped with the others' corners
    s = O.OracleScene()
    R.add_room(s, C, H, (0, 2))
    p4 = R.face_quad(C, H, 4) + 1e-3 * H[:, 0] / np.linalg.norm(H[:, 0])
    s.add_geometry(p4.astype(np.float32), [0, 1, 2, 0, 2, 3], R.EYE4, (0.5, 0.5, 0.5), 1)
    assert _room(capi, s)["n_faces"] == 0
    # one wall of another material: the largest run of one material that is left counts (here two quads either side: none)
    assert _room(capi, _aligned_room(O, mats=[1, 1, 3, 1, 1]))["n_faces"] == 0
    # the quads not consecutive: a triangle in between
    s = O.OracleScene()
    R.add_room(s, C, H, (0, 2))
    s.add_geometry(np.array([[0, 0.5, 0], [0.2, 0.5, 0], [0, 0.7, 0]], np.float32), [0, 1, 2], R.EYE4, (0.5, 0.5, 0.5), 1)
    R.add_room(s, C, H, (4, 1))
    assert _room(capi, s)["n_faces"] == 0
    # a face twice
    assert _room(capi, _aligned_room(O, faces=(0, 2, 2)))["n_faces"] == 0
    assert _room(capi, _aligned_room(O, faces=(0, 2, 4, 2)))["n_faces"] == 3   # (the first three are a corner; the repeat stays a quad)
    # two parallel walls and nothing else: the corners present do not fix the third axis... three parallel quads are no room either
    s = O.OracleScene()
    for shift in (0.0, 0.5, 1.0):
        s.add_geometry((R.face_quad(C, H, 0) + shift * H[:, 0]).astype(np.float32), [0, 1, 2, 0, 2, 3], R.EYE4, (0.5, 0.5, 0.5), 1)
    assert _room(capi, s)["n_faces"] == 0
    for var in ("TRG_BVH_ROOM", "TRG_BVH_BOXES", "TRG_BVH_QUADS"):
        monkeypatch.setenv(var, "0")
        assert _room(capi, _aligned_room(O))["n_faces"] == 0, var
        monkeypatch.delenv(var)
    assert _room(capi, _aligned_room(O))["n_faces"] == 5


def test_two_rooms_only_the_first(capi, O):
    s = O.OracleScene()
    C, H = R.frame("sheared")
    R.add_room(s, C, H, R.CORNER)
    C2, H2 = R.frame("rotated")
    R.add_room(s, C2 + [3.0, 0.0, 0.0], H2, R.OPEN_FRONT)
    r = _room(capi, s)
    assert r["n_faces"] == 3 and r["first_tri"] == 0
    assert r["rest_prims"] == 5                                        # the second room's walls stay five quads of the tree
    perm, sign, dev = R.match_frame(C, H, r["center"], r["axis"])
    assert dev < 1e-5


def test_closed_box_of_planes_is_a_box_leaf(capi, O):
    s = O.OracleScene()
    C, H = R.frame("rotated")
    R.add_room(s, C, H, R.ALL_FACES, pattern=2)
    b = s.buffers()
    assert _room(capi, s)["n_faces"] == 0
    assert capi.debug_boxes(b["positions"], b["indices"], b["material_ids"]).shape[0] == 1


def test_scenes_outside_the_lds_tier_keep_their_blob(capi, O):
    """The digests were taken from the commit before the room existed, with the same FNV-1a over the same host blob (tests/golden/room_parent_blobs.json)."""
    with open(GOLDEN) as f:
        want = json.load(f)
    cases = {"cornell_lattice_44": O.OracleScene.cornell_lattice(44), "cornell_lattice_6": O.OracleScene.cornell_lattice(6)}
    for name, scene in cases.items():
        r = _room(capi, scene)
        assert r["lds_candidate"] == 0 and r["n_faces"] == 0
        assert [r["blob_bytes"], "%016x" % r["blob_hash"]] == want[name], name
    # ... and a scene of the LDS tier with the room switched off is the parent's too
    os.environ["TRG_BVH_ROOM"] = "0"
    try:
        r = _room(capi, O.OracleScene.cornell_box())
    finally:
        del os.environ["TRG_BVH_ROOM"]
    assert [r["blob_bytes"], "%016x" % r["blob_hash"]] != want["cornell_box"]     # (word 6 of a box leaf's face table now says "all present")
    assert r["blob_bytes"] == want["cornell_box"][0]


# ------------------------------------------------------------------------------------------------------------------------------- the open-box rule
MODEL_ROOMS = (("aligned", R.OPEN_FRONT), ("rotated", R.TUBE), ("sheared", R.FOUR), ("mirrored", R.CORNER), ("sheared", R.U_SHAPE))


@pytest.mark.parametrize("kind,faces", MODEL_ROOMS, ids=["%s-%d" % (k, len(f)) for k, f in MODEL_ROOMS])
def test_open_box_rule_is_the_quads_one_by_one(kind, faces):
    """100,000 seeded rays of every kind: the model names the face the nearest quad has and agrees on the distance to 1e-12 -- but for rays whose hit
    lies within 1e-9 of an edge of the room, fewer than 0.1 % of the set."""
    C, H = R.frame(kind)
    o, d, tmax, k = R.room_rays(C, H, faces, 1234 + len(faces), 100000)
    assert len(o) >= 70000 and len(np.unique(k)) >= (7 if len(faces) == 5 else 8) - (0 if len(faces) < 5 else 0)
    fm, tm = R.open_box_f64(C, H, faces, o, d, tmax)
    fq, tq = R.quads_f64(C, H, faces, o, d, tmax)
    t_any = np.where(np.isfinite(tm), tm, tq)
    edge = (R.edge_distance(C, H, o, d, t_any) < 1e-9) & np.isfinite(t_any)
    # rays whose maxDistance ends within 1e-9 of the wall are the same kind of undecidable
    with np.errstate(invalid="ignore"):
        edge |= np.isfinite(t_any) & (np.abs(t_any - tmax) < 1e-9)
    assert edge.mean() < 1e-3, edge.mean()
    ok = ~edge
    assert np.array_equal(fm[ok], fq[ok]), (int((fm[ok] != fq[ok]).sum()), np.unique(k[ok][fm[ok] != fq[ok]]))
    hit = ok & (fm >= 0)
    assert np.abs(tm[hit] - tq[hit]).max() <= 1e-12 * np.maximum(1.0, np.abs(tq[hit])).max()
    # every kind does what it is there for
    frac = lambda name, cond: float(cond[k == R.RAY_KINDS.index(name)].mean())
    assert frac("inside", fm >= 0) > (0.3 if len(faces) == 3 else 0.6)
    assert frac("onto_outside", fm >= 0) > 0.95
    assert frac("tmax_short", fm >= 0) < 0.05 and frac("tmax_beyond", fm >= 0) > 0.95
    if len(faces) < 5:
        assert frac("open_to_open", fm < 0) > 0.3
    assert frac("through_open", fm >= 0) > 0.3
