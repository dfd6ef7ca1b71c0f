"""Host-side checks of the pose unit (include/trg_pose.h, toyraygun_amd/pose.py, toyraygun_amd/csrc/trg_pose_math.h): the exported surface, the files
it must leave alone, the header's arithmetic and maps -- run by a stand-alone program under the host sanitizers -- against pose_reference, and the
condition the GPU tests rely on: the test poses keep every box and every quad leaf of scene A.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pose_scenes as PS
from tests import refit_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_pose.h")
CSRC = os.path.join(ROOT, "toyraygun_amd", "csrc")
HELPER = os.path.join(ROOT, "tests", "helpers", "pose_check.cpp")
DECLARED = ["trg_group_pose_apply", "trg_group_pose_bind", "trg_pose_apply", "trg_pose_bind", "trg_pose_buffers", "trg_pose_read", "trg_pose_release",
            "trg_refit_scene_device"]


def test_library_exports_and_python_binds_every_declared_symbol(built):
    from toyraygun_amd import capi, denoise, pose
    declared = sorted(set(denoise.header_symbols(HEADER)))
    assert declared == DECLARED
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(pose.SYMBOL_NAMES) == declared
    L = pose.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None


def test_render_abi_and_hashed_kernel_sources_are_untouched(built):
    from toyraygun_amd import capi, pose, refit
    from toyraygun_amd.srchash import kernel_source_files, kernel_source_hash
    trg_h = open(os.path.join(ROOT, "include", "trg.h")).read()
    refit_h = open(os.path.join(ROOT, "include", "trg_refit.h")).read()
    for name in pose.SYMBOL_NAMES:
        assert name not in trg_h and name not in capi.SYMBOL_NAMES
        assert name not in refit_h and name not in refit.SYMBOL_NAMES
    assert not any("pose" in os.path.basename(p) for p in kernel_source_files())
    with open(os.path.join(ROOT, "profiles", "r05", "c2_counters.json")) as f:
        assert json.load(f)["kernel_source_hash"] == kernel_source_hash()


# ---------------------------------------------------------------------------------------------------------------------------- the sanitizer program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/helpers/pose_check.cpp with -fsanitize=address,undefined: a program of its own, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("pose") / "pose_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-fno-omit-frame-pointer", "-I" + CSRC, HELPER, "-o", exe])
    return exe


def _run(program, tmp_path, name, b, first, xforms, normals=True):
    pos = np.ascontiguousarray(b["positions"], np.float32)
    idx = np.ascontiguousarray(b["indices"], np.uint32)
    first = np.ascontiguousarray(first, np.uint32)
    path = str(tmp_path / (name + ".bin"))
    with open(path, "wb") as f:
        f.write(np.array([pos.shape[0], idx.shape[0] // 3, first.shape[0] - 1, 1 if normals else 0], np.uint32).tobytes())
        f.write(pos.tobytes())
        if normals:
            f.write(np.ascontiguousarray(b["normals"], np.float32).tobytes())
        f.write(idx.tobytes() + first.tobytes() + np.ascontiguousarray(xforms, np.float32).tobytes())
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    return r.stdout.splitlines()


def _words(lines, tag):
    return np.array([[int(w, 16) for w in l.split()[1:]] for l in lines if l.startswith(tag + " ")], np.uint32)


@pytest.mark.parametrize("make, n_verts", [(RS.scene_a, 3 * 706), (RS.scene_a_indexed, RS.N_VERTS_INDEXED)], ids=["per-corner", "indexed"])
def test_header_poses_scene_a_to_the_bits_of_pose_reference(program, tmp_path, make, n_verts):
    """Scene A as 34 objects (floor, 32 cubes, sphere) -- per corner, and indexed with its two vertices that no triangle names -- posed by the
    header's functions in the sanitized program: the maps are pose.object_maps', the posed positions and normals pose_reference's, bit for bit; the
    unnamed vertices keep their rest bits."""
    from toyraygun_amd import pose
    b = make(0)
    first = PS.scene_a_first()
    assert first.shape[0] == PS.N_OBJECTS_A + 1 == 35 and b["positions"].shape[0] == n_verts
    for seed in (1, 2):
        x = PS.scene_a_xforms(seed)
        lines = _run(program, tmp_path, "a%d" % seed, b, first, x)
        assert lines[0] == "table ok" and lines[1] == "vertices ok"
        tri_obj, vtx_obj = pose.object_maps(b["indices"], first, n_verts)
        assert np.array_equal(_words(lines, "T")[0], tri_obj.astype(np.uint32))
        assert np.array_equal(_words(lines, "V")[0], vtx_obj.astype(np.uint32))        # (-1 is ffffffff)
        ref_pos, ref_nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], first, x)
        got_pos, got_nrm = _words(lines, "P"), _words(lines, "N")
        assert got_pos.shape == (n_verts, 3) and got_nrm.shape == (3 * 706, 3)
        assert np.array_equal(got_pos, ref_pos.view(np.uint32)) and np.array_equal(got_nrm, ref_nrm.view(np.uint32))
        unnamed = vtx_obj < 0
        assert int(unnamed.sum()) == (2 if make is RS.scene_a_indexed else 0)
        assert np.array_equal(ref_pos[unnamed].view(np.uint32), b["positions"][unnamed].view(np.uint32))
        assert (ref_pos[~unnamed] != b["positions"][~unnamed]).any(1).mean() > 0.99      # everything named moves
        np.testing.assert_allclose(np.linalg.norm(ref_nrm.astype(np.float64), axis=1), 1.0, atol=3e-7)


def test_bad_tables_are_refused_by_the_header(program, tmp_path):
    """The four bad tables of tests/pose_scenes.py.  `an object of one triangle` is a legal table in itself (strictly ascending): what refuses it is
    the shared-vertex rule, in the indexed scene, where the floor's two triangles share two vertices; per corner it passes."""
    from toyraygun_amd import pose
    want = {"not ascending": "table refused order object 5", "not ending at n_tris": "table refused end object 33",
            "a vertex shared by two objects": "vertices refused shared triangle 4", "an object of one triangle": "vertices refused shared triangle 1 "}
    for name, (table, indexed) in PS.bad_tables().items():
        b = RS.scene_a_indexed(0) if indexed else RS.scene_a(0)
        lines = _run(program, tmp_path, "bad", b, table, PS.identity(table.shape[0] - 1))
        said = lines[0] if lines[0] != "table ok" else lines[1]
        print("%s: %s" % (name, said))
        assert said.startswith(want[name]), (name, said)
        if name == "a vertex shared by two objects":                             # the first triangle of the sphere's second part that names a vertex of the first
            assert 486 <= int(said.split()[4]) < 500
        assert not any(l.startswith("P ") for l in lines)
        with pytest.raises(ValueError):
            pose.object_maps(b["indices"], table, b["positions"].shape[0])
    table = PS.bad_tables()["an object of one triangle"][0]
    lines = _run(program, tmp_path, "one", RS.scene_a(0), table, PS.identity(table.shape[0] - 1))
    assert lines[:2] == ["table ok", "vertices ok"]


# ---------------------------------------------------------------------------------------------------------------------------- the builders' rules
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_the_test_poses_keep_every_box_and_every_quad(tmp_path):
    """The condition the GPU tests rely on, with zero exceptions: scene A posed by scene_a_xforms (the seeds the GPU tests use) and by the poses of
    the sequence tests -- all 32 cubes still pass the builder's box rule (box_group_pos, through the refit_check shim) and all 193 quad leaves the
    quad rule (quad_still).  And the refusal the GPU test provokes is one: a cube scaled to nothing is no box and none of its faces a quad."""
    from tests.test_refit_host import build_shim
    from toyraygun_amd import pose
    shim = build_shim(str(tmp_path / "librefit_check.so"))
    first = PS.scene_a_first()
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)

    def rules(b, x):
        pos, _ = pose.pose_reference(b["positions"], b["normals"], b["indices"], first, x)
        idx, nv, nt = b["indices"], pos.shape[0], 706
        boxes = [shim.rf_host_box(_p(pos), _p(idx), nv, nt, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) for i in range(RS.N_CUBES)]
        quads = [shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 2 * q, 2 * q + 1) for q in range(1 + 6 * RS.N_CUBES)]
        return boxes, quads
    for make in (RS.scene_a, RS.scene_a_indexed):
        b = make(0)
        for x in [PS.scene_a_xforms(s) for s in (1, 2, 3, 4, 5)] + [PS.identity(PS.N_OBJECTS_A)]:
            boxes, quads = rules(b, x)
            assert all(v == 1 for v in boxes) and all(v == 1 for v in quads), (boxes.count(0), quads.count(0))
    x = PS.scene_a_xforms(1)
    x[1 + 9] = 0
    boxes, quads = rules(RS.scene_a(0), x)
    assert boxes.count(0) == 1 and boxes[9] == 0 and quads.count(0) == 6


# ---------------------------------------------------------------------------------------------------------------------------- pose_reference
def _one_triangle(normal=(0.0, 0.6, 0.8)):
    pos = np.array([[0.25, -0.0, 1.5], [1.0, 2.0, -0.0], [-3.0, 0.5, 0.125]], np.float32)
    return pos, np.tile(np.array(normal, np.float32), (3, 1)), np.arange(3, dtype=np.uint32), np.array([0, 1], np.uint32)


def test_identity_returns_the_rest_pose_under_equality():
    from toyraygun_amd import pose
    b = RS.scene_a(0)
    pos, nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], PS.scene_a_first(), PS.identity(PS.N_OBJECTS_A))
    assert (pos == b["positions"]).all()
    # a unit normal renormalised: the components are rounded (|n|^2 off by 2^-23 at most), three roundings in the sum, one in the root, one in the
    # division -- n / len is n to within 3.3 x 2^-24 < 2^-22 -- and exactly n for the exactly unit ones
    assert np.abs(nrm.astype(np.float64) - b["normals"]).max() <= 2.0 ** -22
    assert (nrm[:6] == b["normals"][:6]).all()                                   # the floor's (0, 1, 0)
    p, n, idx, first = _one_triangle()
    pos, _ = pose.pose_reference(p, n, idx, first, PS.identity(1))
    assert (pos == p).all() and not np.array_equal(pos.view(np.uint32), p.view(np.uint32))   # equal values; the -0 became +0


def test_a_mirror_flips_the_sign_and_rank_one_keeps_the_rest_normal():
    from toyraygun_amd import pose
    p, n, idx, first = _one_triangle()
    mirror = np.eye(3, 4, dtype=np.float32)
    mirror[0, 0] = -1
    _, out = pose.pose_reference(p, n, idx, first, mirror.reshape(1, 12))
    # cofactors of diag(-1, 1, 1): diag(1, -1, -1); det < 0, s = -1: n' = (-nx, ny, nz) -- the reflected normal, not its negative
    np.testing.assert_allclose(out, np.tile([0.0, 0.6, 0.8], (3, 1)), atol=1e-7)
    n2 = np.tile(np.array([0.6, 0.0, 0.8], np.float32), (3, 1))
    _, out = pose.pose_reference(p, n2, idx, first, mirror.reshape(1, 12))
    np.testing.assert_allclose(out, np.tile([-0.6, 0.0, 0.8], (3, 1)), atol=1e-7)
    scale = np.eye(3, 4, dtype=np.float32) * np.float32(2.0)
    _, out = pose.pose_reference(p, n2, idx, first, scale.reshape(1, 12))
    np.testing.assert_allclose(out, n2, atol=1e-7)                               # the same matrix without the mirror: s = +1
    rank1 = np.zeros((3, 4), np.float32)
    rank1[:, :3] = np.outer([1.0, 2.0, -1.0], [0.5, 0.25, 2.0])
    _, out = pose.pose_reference(p, n, idx, first, rank1.reshape(1, 12))
    assert np.array_equal(out.view(np.uint32), n.view(np.uint32))                # every cofactor is 0: len == 0, the rest normal is copied
    _, out = pose.pose_reference(p, n, idx, first, np.zeros((1, 12), np.float32))
    assert np.array_equal(out.view(np.uint32), n.view(np.uint32))
