"""Host-side checks of the skin unit (include/trg_skin.h, toyraygun_amd/skin.py, toyraygun_amd/csrc/trg_skin_math.h): the exported surface, the
files it must leave alone, the header's arithmetic and validators -- run by a stand-alone program under the host sanitizers -- against
skin_reference, skin_reference against a float64 evaluation, and the condition the GPU tests rely on: the test bones keep every box and every quad
leaf of scene A.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pose_scenes as PS
from tests import refit_scenes as RS
from tests import skin_scenes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_skin.h")
CSRC = os.path.join(ROOT, "toyraygun_amd", "csrc")
HELPER = os.path.join(ROOT, "tests", "helpers", "skin_check.cpp")
DECLARED = ["trg_group_skin_apply", "trg_group_skin_bind", "trg_skin_apply", "trg_skin_bind", "trg_skin_buffers", "trg_skin_read", "trg_skin_release"]
SEEDS = (1, 2, 3)          # every seed tests/test_gpu_skin.py uses


def test_library_exports_and_python_binds_every_declared_symbol(built):
    from toyraygun_amd import capi, denoise, skin
    declared = sorted(set(denoise.header_symbols(HEADER)))
    assert declared == DECLARED
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(skin.SYMBOL_NAMES) == declared
    L = skin.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None


def test_other_headers_and_hashed_kernel_sources_are_untouched(built):
    from toyraygun_amd import capi, denoise, pose, refit, skin
    from toyraygun_amd.srchash import kernel_source_files, kernel_source_hash
    others = [open(os.path.join(ROOT, "include", h)).read() for h in ("trg.h", "trg_refit.h", "trg_pose.h", "trg_denoise.h")]
    lists = [capi.SYMBOL_NAMES, refit.SYMBOL_NAMES, pose.SYMBOL_NAMES, denoise.SYMBOL_NAMES]
    for name in skin.SYMBOL_NAMES:
        assert not any(name in text for text in others)
        assert not any(name in names for names in lists)
    assert not any("skin" in os.path.basename(p) for p in kernel_source_files())
    for p in kernel_source_files():
        with open(p, errors="replace") as f:
            assert "skin" not in f.read().lower(), p
    with open(os.path.join(ROOT, "profiles", "r05", "c2_counters.json")) as f:
        assert json.load(f)["kernel_source_hash"] == kernel_source_hash()


# ---------------------------------------------------------------------------------------------------------------------------- the sanitizer program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/helpers/skin_check.cpp with -fsanitize=address,undefined: a program of its own, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("skin") / "skin_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-fno-omit-frame-pointer", "-I" + CSRC, HELPER, "-o", exe])
    return exe


def _run(program, tmp_path, name, b, ids, weights, bones, normals=True):
    pos = np.ascontiguousarray(b["positions"], np.float32)
    idx = np.ascontiguousarray(b["indices"], np.uint32)
    bones = np.ascontiguousarray(bones, np.float32).reshape(-1, 12)
    path = str(tmp_path / (name + ".bin"))
    with open(path, "wb") as f:
        f.write(np.array([pos.shape[0], idx.shape[0] // 3, bones.shape[0], 1 if normals else 0], np.uint32).tobytes())
        f.write(pos.tobytes())
        if normals:
            f.write(np.ascontiguousarray(b["normals"], np.float32).tobytes())
        f.write(idx.tobytes() + np.ascontiguousarray(ids, np.uint32).tobytes() + np.ascontiguousarray(weights, np.float32).tobytes() + bones.tobytes())
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    return r.stdout.splitlines()


def _words(lines, tag):
    return np.array([[int(w, 16) for w in l.split()[1:]] for l in lines if l.startswith(tag + " ")], np.uint32)


@pytest.mark.parametrize("make, n_verts", [(RS.scene_a, 3 * 706), (RS.scene_a_indexed, RS.N_VERTS_INDEXED)], ids=["per-corner", "indexed"])
def test_header_skins_scene_a_to_the_bits_of_skin_reference(program, tmp_path, make, n_verts):
    """Scene A under its 38 bones -- per corner (2,118 vertices), and indexed (424, two that no triangle names) -- skinned by the header's functions
    in the sanitized program: positions and normals are skin_reference's, bit for bit.  The binding has what the kernel can get wrong: a vertex
    with four non-zero weights, one with a zero weight whose id is the last bone, unnamed vertices that move."""
    from toyraygun_amd import skin
    b = make(0)
    ids, w = SS.scene_a_binding(b)
    assert b["positions"].shape[0] == n_verts == ids.shape[0] == w.shape[0] and skin.check_binding(ids, w, SS.N_BONES) is None
    assert ((w > 0).sum(1) == 4).any() and ((w > 0).sum(1) == 3).any()
    assert ((ids == SS.LAST_BONE) & (w == 0)).any() and not ((ids == SS.LAST_BONE) & (w != 0)).any() and SS.LAST_BONE == SS.N_BONES - 1
    obj = SS._objects(b)
    assert int((obj < 0).sum()) == (2 if make is RS.scene_a_indexed else 0)
    for seed in SEEDS[:2]:
        bones = SS.scene_a_bones(seed)
        lines = _run(program, tmp_path, "a%d" % seed, b, ids, w, bones)
        assert lines[0] == "ids ok" and lines[1] == "weights ok"
        ref_pos, ref_nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, bones)
        got_pos, got_nrm = _words(lines, "P"), _words(lines, "N")
        assert got_pos.shape == (n_verts, 3) and got_nrm.shape == (3 * 706, 3)
        assert np.array_equal(got_pos, ref_pos.view(np.uint32)) and np.array_equal(got_nrm, ref_nrm.view(np.uint32))
        assert (ref_pos != b["positions"]).any(1).all()                          # everything moves, the unnamed vertices too
        assert np.abs(ref_pos[obj >= 0]).max() < 10                              # (and bone 37's 1e6 reached nothing)
        np.testing.assert_allclose(np.linalg.norm(ref_nrm.astype(np.float64), axis=1), 1.0, atol=3e-7)
        # the copies of a shared corner: equal inputs, equal bits
        key = np.concatenate([b["positions"][b["indices"]].view(np.uint32), b["normals"].view(np.uint32)], axis=1)
        _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        assert first.shape[0] < key.shape[0]
        assert np.array_equal(ref_nrm.view(np.uint32), ref_nrm.view(np.uint32)[first][inv])
        assert np.array_equal(ref_pos[b["indices"]].view(np.uint32), ref_pos[b["indices"]].view(np.uint32)[first][inv])
    lines = _run(program, tmp_path, "nonrm", b, ids, w, SS.scene_a_bones(1), normals=False)
    assert _words(lines, "P").shape == (n_verts, 3) and _words(lines, "N").size == 0


def test_the_validators_name_the_first_offending_vertex(program, tmp_path):
    """A bad id, a negative weight, a NaN weight and a sum off by 1e-3 are each refused by the header, the first vertex named; a sum off by 1e-6
    passes.  skin.check_binding, the same rules in numpy, agrees."""
    from toyraygun_amd import skin
    b = RS.scene_a(0)
    want = {"a bad id": "ids refused vertex 17 slot 2", "a negative weight": "weights refused weight vertex 5", "a NaN weight": "weights refused weight vertex 300",
            "a sum off by 1e-3": "weights refused sum vertex 41"}
    for name, (ids, w, vert, _) in SS.bad_bindings(b).items():
        lines = _run(program, tmp_path, "bad", b, ids, w, SS.identity())
        if vert is None:
            assert lines[:2] == ["ids ok", "weights ok"] and skin.check_binding(ids, w, SS.N_BONES) is None
            assert abs(float(w[1200].astype(np.float64).sum()) - 1.0) > 5e-7 and SS._objects(b)[1200] == SS.SPHERE_OBJECT
            continue
        said = lines[0] if lines[0] != "ids ok" else lines[1]
        assert said == want[name], (name, said)
        assert not any(l.startswith("P ") for l in lines)
        assert skin.check_binding(ids, w, SS.N_BONES)[0] == vert
    # two faults: the first vertex is named, whichever rule it breaks
    ids, w = SS.scene_a_binding(b)
    w[9] = (0.25, 0.25, 0.25, 0.2)
    w[30, 0] = -1.0
    assert _run(program, tmp_path, "two", b, ids, w, SS.identity())[1] == "weights refused sum vertex 9"
    assert skin.check_binding(ids, w, SS.N_BONES) == (9, "sum")


# ---------------------------------------------------------------------------------------------------------------------------- the builders' rules
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_the_test_bones_keep_every_box_and_every_quad(tmp_path):
    """The condition the GPU tests rely on, with zero exceptions: scene A skinned by scene_a_bones under every seed the GPU tests use, per corner and
    indexed -- all 32 cubes still pass the builder's box rule (through the refit_check shim) and all 193 quad leaves the quad rule.  And the refusal
    the GPU test provokes is one: a cube whose eight corners are split between two bones is no box."""
    from tests.test_refit_host import build_shim
    from toyraygun_amd import skin
    shim = build_shim(str(tmp_path / "librefit_check.so"))
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)

    def rules(b, ids, w, bones):
        pos, _ = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, bones)
        idx, nv, nt = b["indices"], pos.shape[0], 706
        boxes = [shim.rf_host_box(_p(pos), _p(idx), nv, nt, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) for i in range(RS.N_CUBES)]
        quads = [shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 2 * q, 2 * q + 1) for q in range(1 + 6 * RS.N_CUBES)]
        return boxes, quads
    for make in (RS.scene_a, RS.scene_a_indexed):
        b = make(0)
        ids, w = SS.scene_a_binding(b)
        for bones in [SS.scene_a_bones(s) for s in SEEDS] + [SS.identity()]:
            boxes, quads = rules(b, ids, w, bones)
            assert all(v == 1 for v in boxes) and all(v == 1 for v in quads), (boxes.count(0), quads.count(0))
        ids1, w1, nb = SS.one_hot(b)
        for s in SEEDS:
            boxes, quads = rules(b, ids1, w1, np.concatenate([PS.scene_a_xforms(s), PS.identity(1)]))
            assert all(v == 1 for v in boxes) and all(v == 1 for v in quads)
    b = RS.scene_a(0)
    ids, w = SS.scene_a_binding(b, split_cube=9)
    own = ids[3 * RS.cube_first_triangle(9):3 * RS.cube_first_triangle(10), 0]
    corners = np.unique(b["positions"][3 * RS.cube_first_triangle(9):3 * RS.cube_first_triangle(10)], axis=0)
    assert sorted(set(own.tolist())) == [10, 11] and corners.shape[0] == 8
    boxes, quads = rules(b, ids, w, SS.identity())
    assert all(v == 1 for v in boxes) and all(v == 1 for v in quads)              # at rest the split cube is the cube it was
    for s in (2, 3):                                                            # and while its two bones are equal
        boxes, quads = rules(b, ids, w, SS.scene_a_bones(s, share=(10, 11)))
        assert all(v == 1 for v in boxes) and all(v == 1 for v in quads)
    boxes, quads = rules(b, ids, w, SS.scene_a_bones(1))
    assert boxes.count(0) == 1 and boxes[9] == 0


# ---------------------------------------------------------------------------------------------------------------------------- skin_reference
def _float64_blend(b, ids, w, bones):
    """Linear-blend skinning evaluated in float64 from the float32 inputs: x' = sum_j w_j (A_j x + t_j); n' = the unit vector along
    sign(det) cof(sum_j w_j A_j) n."""
    pos = b["positions"].astype(np.float64)
    B = np.asarray(bones, np.float64).reshape(-1, 3, 4)
    M = np.einsum("vj,vjrc->vrc", w.astype(np.float64), B[ids.astype(np.int64)])
    out = np.einsum("vrc,vc->vr", M[:, :, :3], pos) + M[:, :, 3]
    A = M[b["indices"].astype(np.int64)][:, :, :3]
    det = np.linalg.det(A)
    cof = np.linalg.inv(A).transpose(0, 2, 1) * det[:, None, None]
    n = np.sign(det)[:, None] * np.einsum("krc,kc->kr", cof, b["normals"].astype(np.float64))
    return out, n / np.linalg.norm(n, axis=1, keepdims=True)


@pytest.mark.parametrize("make", [RS.scene_a, RS.scene_a_indexed], ids=["per-corner", "indexed"])
def test_skin_reference_against_a_float64_linear_blend(make):
    """fp32 against float64.  A position is 12 blended entries (3 roundings each beyond the products: relative 4 x 2^-24 per entry, generously) times
    coordinates within the scene's extent E, three products and three sums: within 16 ulp of E.  (The vertices no triangle names are compared
    relative to their own size: one is 1e6 away.)  A normal goes through differences of products of entries -- cancellation is bounded by the
    bones' condition, all mild here -- and ends as a unit vector: 1e-5 absolute, and unit length to 3e-7."""
    from toyraygun_amd import skin
    b = make(0)
    ids, w = SS.scene_a_binding(b)
    named = SS._objects(b) >= 0
    for seed in SEEDS:
        bones = SS.scene_a_bones(seed)
        pos, nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, bones)
        ref_pos, ref_nrm = _float64_blend(b, ids, w, bones)
        extent = max(np.abs(ref_pos[named]).max(), np.abs(b["positions"][named]).max())
        ulp = 2.0 ** -23 * extent
        assert np.abs(pos[named] - ref_pos[named]).max() <= 16 * ulp
        assert (np.abs(pos[~named] - ref_pos[~named]) <= 16 * 2.0 ** -23 * np.abs(ref_pos[~named]).max(axis=1, keepdims=True)).all()
        assert np.abs(nrm - ref_nrm).max() <= 1e-5
        np.testing.assert_allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=3e-7)


def test_one_hot_weights_equal_the_pose_reference():
    """Weights (1, 0, 0, 0): the blended matrix is the bone (1 x = x, 0 x = 0, x + 0 = x), so positions and normals equal pose_reference's with
    that bone as the object's matrix, under == (only the sign of a zero may differ).  The other three ids name arbitrary finite bones."""
    from toyraygun_amd import pose, skin
    for make in (RS.scene_a, RS.scene_a_indexed):
        b = make(0)
        ids, w, nb = SS.one_hot(b)
        ids[:, 1:] = np.random.default_rng(5).integers(0, nb, (ids.shape[0], 3))
        for seed in SEEDS[:2]:
            x = PS.scene_a_xforms(seed)
            pos, nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, np.concatenate([x, PS.identity(1)]))
            ref_pos, ref_nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], PS.scene_a_first(), x)
            assert (pos == ref_pos).all() and (nrm == ref_nrm).all()


def test_one_rigid_matrix_on_every_bone_is_that_matrix_on_one_object():
    """All bones equal to one rigid matrix R: a blend with weights summing to 1 is R up to the rounding of the weights -- each entry within
    4 x 2^-24 of |R|'s, so positions agree with the single-object pose within a few ulp of the extent, normals to 2e-6."""
    from toyraygun_amd import pose, skin
    b = RS.scene_a(0)
    ids, w = SS.scene_a_binding(b)
    R = PS._about(RS._rot((1.0, 2.0, -0.5), 0.7), (0.1, 0.5, -0.2), (0.3, -0.1, 0.2)).reshape(1, 12).astype(np.float32)
    pos, nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, np.tile(R, (SS.N_BONES, 1)))
    ref_pos, ref_nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], np.array([0, 706], np.uint32), R)
    assert np.abs(pos - ref_pos).max() <= 16 * 2.0 ** -23 * np.abs(ref_pos).max()
    assert np.abs(nrm - ref_nrm).max() <= 2e-6
    one = w[:, 0] == 1
    assert one.any() and (pos[one] == ref_pos[one]).all()


def test_identity_bones_return_the_rest_pose_under_equality():
    """Identity bones: every entry of the blend is a sum of weights or of zeros.  The test weights are multiples of 2^-10 that sum to exactly 1, so
    M is the identity and the rest pose comes back under == (a -0 becomes +0); a unit normal renormalised is itself to within 2^-22."""
    from toyraygun_amd import skin
    for make in (RS.scene_a, RS.scene_a_indexed):
        b = make(0)
        ids, w = SS.scene_a_binding(b)
        assert (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3] == np.float32(1)).all() and (w * 1024 == np.round(w * 1024)).all()
        pos, nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, SS.identity())
        assert (pos == b["positions"]).all()
        assert np.abs(nrm.astype(np.float64) - b["normals"]).max() <= 2.0 ** -22
        assert (nrm[:6] == b["normals"][:6]).all()                               # the floor's (0, 1, 0)
