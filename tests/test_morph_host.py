"""Host-side checks of the morph unit (include/trg_morph.h, toyraygun_amd/morph.py, toyraygun_amd/csrc/trg_morph_math.h): the exported surface, the
files it must leave alone, the header's arithmetic, validators and transposition -- run by a stand-alone program under the host sanitizers -- against
morph_reference, the identities that arithmetic promises, morph_reference against a float64 evaluation, and the condition the GPU tests rely on:
the test targets, weights and bones keep every box and every quad leaf of scene A.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import morph_scenes as MS
from tests import pose_scenes as PS
from tests import refit_scenes as RS
from tests import skin_scenes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_morph.h")
CSRC = os.path.join(ROOT, "toyraygun_amd", "csrc")
HELPER = os.path.join(ROOT, "tests", "helpers", "morph_check.cpp")
DECLARED = ["trg_group_morph_apply", "trg_group_morph_bind", "trg_morph_apply", "trg_morph_bind", "trg_morph_buffers", "trg_morph_read", "trg_morph_release"]
SCENES = pytest.mark.parametrize("indexed", [False, True], ids=["per-corner", "indexed"])
# fp32 morph_reference against float64, measured on these scenes under every weight vector and bone seed of tests/morph_scenes.py (NOTEBOOK,
# "Blend shapes"): positions 0.539 ulp of the scene's extent without bones and 1.736 with, normals 1.023e-7 and 1.652e-7 absolute, the same in
# both forms of the scene.  The bars are twice that
POS_ULP_BAR = {False: 1.078, True: 3.472}
NRM_BAR = {False: 2.046e-7, True: 3.304e-7}


def test_library_exports_and_python_binds_every_declared_symbol(built):
    from toyraygun_amd import capi, denoise, morph
    declared = sorted(set(denoise.header_symbols(HEADER)))
    assert declared == DECLARED
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(morph.SYMBOL_NAMES) == declared
    L = morph.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None


def test_other_headers_and_hashed_kernel_sources_are_untouched(built):
    from toyraygun_amd import capi, denoise, morph, pose, refit, skin
    from toyraygun_amd.srchash import kernel_source_files, kernel_source_hash
    others = [open(os.path.join(ROOT, "include", h)).read() for h in ("trg.h", "trg_refit.h", "trg_pose.h", "trg_skin.h", "trg_denoise.h")]
    lists = [capi.SYMBOL_NAMES, refit.SYMBOL_NAMES, pose.SYMBOL_NAMES, skin.SYMBOL_NAMES, denoise.SYMBOL_NAMES]
    for name in morph.SYMBOL_NAMES:
        assert not any(name in text for text in others)
        assert not any(name in names for names in lists)
    assert not any("morph" in os.path.basename(p) for p in kernel_source_files())
    for p in kernel_source_files():
        with open(p, errors="replace") as f:
            assert "morph" not in f.read().lower(), p
    with open(os.path.join(ROOT, "profiles", "r05", "c2_counters.json")) as f:
        assert json.load(f)["kernel_source_hash"] == kernel_source_hash()


def test_the_targets_mix_every_entry_count_within_64_vertices():
    """What the gather can get wrong shows where lanes of one wave walk ranges of different lengths: vertices with 0, 1, 2, 3 and >= 4 entries occur
    inside one run of 64 vertices, in both forms of the scene.  And the table has what its description says: an empty target, a last target that
    holds vertex 0, the last vertex and the unnamed ones, T5 on every object."""
    for indexed in (False, True):
        b = MS.scene(indexed)
        t = MS.targets(b)
        nv = b["positions"].shape[0]
        assert nv == (424 if indexed else 2118) and t[0].shape[0] == MS.N_TARGETS + 1
        counts = np.minimum(MS.entries_per_vertex(t, nv), 4)
        runs = [set(counts[s:s + 64].tolist()) for s in range(0, nv - 63)]
        assert any(r == {0, 1, 2, 3, 4} for r in runs), sorted(set(counts.tolist()))
        assert t[0][MS.EMPTY] == t[0][MS.EMPTY + 1]
        last = t[1][t[0][MS.LAST]:t[0][MS.LAST + 1]]
        obj = SS._objects(b)
        assert 0 in last and nv - 1 in last and set(np.flatnonzero(obj < 0).tolist()) <= set(last.tolist())
        assert int((obj < 0).sum()) == (2 if indexed else 0)
        zero = t[1][t[0][MS.ALWAYS_ZERO]:t[0][MS.ALWAYS_ZERO + 1]]
        assert set(obj[zero].tolist()) >= set(range(SS.SPHERE_OBJECT + 1))
        assert all(MS.WEIGHTS[k][MS.ALWAYS_ZERO] == 0 and MS.WEIGHTS[k][MS.EMPTY] == 0 for k in MS.WEIGHTS)
        if indexed:
            v = MS.minus_zero_vertex(b)
            assert np.signbit(b["positions"][v, 1]) and counts[v] >= 1


# ---------------------------------------------------------------------------------------------------------------------------- the sanitizer program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/helpers/morph_check.cpp with -fsanitize=address,undefined: a program of its own, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("morph") / "morph_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-fno-omit-frame-pointer", "-I" + CSRC, HELPER, "-o", exe])
    return exe


def _run(program, tmp_path, name, b, t, tw, binding=None, bones=None, normals=True, deltas=True, records=False, n_entries=None):
    pos = np.ascontiguousarray(b["positions"], np.float32)
    idx = np.ascontiguousarray(b["indices"], np.uint32)
    first, ev, dp, dn = t
    ne = ev.shape[0] if n_entries is None else n_entries
    n_bones = 0 if bones is None else np.asarray(bones).reshape(-1, 12).shape[0]
    path = str(tmp_path / (name + ".bin"))
    with open(path, "wb") as f:
        f.write(np.array([pos.shape[0], idx.shape[0] // 3, first.shape[0] - 1, ne, n_bones, 1 if normals else 0, 1 if deltas else 0, 1 if records else 0], np.uint32).tobytes())
        f.write(pos.tobytes())
        if normals:
            f.write(np.ascontiguousarray(b["normals"], np.float32).tobytes())
        f.write(idx.tobytes() + np.ascontiguousarray(first, np.uint32).tobytes() + np.ascontiguousarray(ev[:ne], np.uint32).tobytes())
        f.write(np.ascontiguousarray(dp[:ne], np.float32).tobytes())
        if deltas:
            f.write(np.ascontiguousarray(dn[:ne], np.float32).tobytes())
        f.write(np.ascontiguousarray(tw, np.float32).tobytes())
        if n_bones:
            f.write(np.ascontiguousarray(binding[0], np.uint32).tobytes() + np.ascontiguousarray(binding[1], np.float32).tobytes())
            f.write(np.ascontiguousarray(bones, np.float32).tobytes())
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    return r.stdout.splitlines()


def _words(lines, tag, base=16):
    return np.array([[int(w, base) for w in l.split()[1:]] for l in lines if l.startswith(tag + " ")], np.uint32)


@SCENES
def test_header_morphs_scene_a_to_the_bits_of_morph_reference(program, tmp_path, indexed):
    """Scene A under its seven targets, morphed by the header's functions in the sanitized program -- with and without bones, with and without normal
    deltas, and bound without normals: positions and normals are morph_reference's, bit for bit.  The copies of a shared corner stay equal."""
    from toyraygun_amd import morph
    b = MS.scene(indexed)
    t = MS.targets(b)
    binding = SS.scene_a_binding(b)
    nv = b["positions"].shape[0]
    assert morph.check_targets(*t, nv) is None
    for name, seed, deltas in (("a", None, True), ("b", 1, True), ("c", 2, False), ("c", None, False), ("last", 3, True)):
        tw = MS.weights(name)
        bones = None if seed is None else SS.scene_a_bones(seed)
        lines = _run(program, tmp_path, "m", b, t, tw, binding, bones, deltas=deltas)
        assert lines[:2] == ["targets ok", "entries ok"]
        skin_args = {} if seed is None else dict(bone_ids=binding[0], bone_weights=binding[1], bones=bones)
        ref_pos, ref_nrm = morph.morph_reference(b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3] if deltas else None, tw, **skin_args)
        got_pos, got_nrm = _words(lines, "P"), _words(lines, "N")
        assert got_pos.shape == (nv, 3) and got_nrm.shape == (3 * 706, 3)
        assert np.array_equal(got_pos, ref_pos.view(np.uint32)) and np.array_equal(got_nrm, ref_nrm.view(np.uint32)), (name, seed, deltas)
        named = SS._objects(b) >= 0
        assert np.abs(ref_pos[named]).max() < 10                                 # T5's 1e6 reached nothing
        if seed is None and not deltas:
            assert np.array_equal(ref_nrm.view(np.uint32), b["normals"].view(np.uint32))      # no deltas, no bones: the loaded normals' bits
        np.testing.assert_allclose(np.linalg.norm(ref_nrm.astype(np.float64), axis=1), 1.0, atol=3e-7)
        key = np.concatenate([b["positions"][b["indices"]].view(np.uint32), b["normals"].view(np.uint32)], axis=1)
        _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        assert first.shape[0] < key.shape[0]
        assert np.array_equal(ref_nrm.view(np.uint32), ref_nrm.view(np.uint32)[first][inv])
        assert np.array_equal(ref_pos[b["indices"]].view(np.uint32), ref_pos[b["indices"]].view(np.uint32)[first][inv])
    lines = _run(program, tmp_path, "nonrm", b, t, MS.weights("a"), normals=False, deltas=False)
    ref_pos, ref_nrm = morph.morph_reference(b["positions"], None, b["indices"], t[0], t[1], t[2], None, MS.weights("a"))
    assert ref_nrm is None and np.array_equal(_words(lines, "P"), ref_pos.view(np.uint32)) and _words(lines, "N").size == 0


@SCENES
def test_the_transposed_records_are_each_vertexs_entries_in_target_order(program, tmp_path, indexed):
    """The transposition, looked at directly: vfirst begins at 0, ends at n_entries and steps by each vertex's entry count; a vertex's records
    are its entries in ascending target order, the deltas bit for bit; the empty target contributes nothing; the last vertex has a record (its
    range ends where the arrays end)."""
    b = MS.scene(indexed)
    first, ev, dp, dn = t = MS.targets(b)
    nv, ne = b["positions"].shape[0], ev.shape[0]
    lines = _run(program, tmp_path, "rec", b, t, MS.weights("a"), records=True)
    vfirst = _words(lines, "F", 10).reshape(-1).astype(np.int64)
    R, Q = _words(lines, "R"), _words(lines, "Q")
    tgt_r = np.array([int(l.split()[1]) for l in lines if l.startswith("R ")])
    tgt_q = np.array([int(l.split()[1]) for l in lines if l.startswith("Q ")])
    assert vfirst.shape[0] == nv + 1 and vfirst[0] == 0 and vfirst[-1] == ne and R.shape == (ne, 4) and Q.shape == (ne, 4)
    assert np.array_equal(np.diff(vfirst), MS.entries_per_vertex(t, nv))
    owner = np.repeat(np.arange(MS.N_TARGETS), np.diff(first.astype(np.int64)))
    order = np.lexsort((owner, ev))                                              # by vertex, then by target: what the records must be
    assert np.array_equal(tgt_r, owner[order]) and np.array_equal(tgt_q, owner[order])
    assert np.array_equal(R[:, 1:], dp[order].view(np.uint32)) and np.array_equal(Q[:, 1:], dn[order].view(np.uint32))
    for v in range(nv):
        assert (np.diff(tgt_r[vfirst[v]:vfirst[v + 1]]) > 0).all()
    assert MS.EMPTY not in tgt_r and vfirst[nv] - vfirst[nv - 1] >= 1


def test_the_validators_name_the_planted_offender(program, tmp_path):
    """Each refused table or entry list: the header's validators, in the sanitized program, name the target (and the entry) planted; morph.check_targets,
    the same rules in numpy, agrees.  Normal deltas without normals and half-given bones are trg_morph_bind's own checks: check_targets words them."""
    from toyraygun_amd import morph
    b = MS.scene(False)
    nv = b["positions"].shape[0]
    said = {"first": "targets refused first target %d", "order": "targets refused order target %d", "end": "targets refused end target %d",
            "vertex": "entries refused vertex target %d entry %d", "repeat": "entries refused order target %d entry %d",
            "delta": "entries refused delta target %d entry %d", "normal delta": "entries refused normal-delta target %d entry %d"}
    cases = MS.bad_targets(b)
    assert len(cases) == 7
    for name, (first, ev, dp, dn, ne, want, _) in cases.items():
        lines = _run(program, tmp_path, "bad", b, (first, ev, dp, dn), MS.weights("a"), n_entries=ne)
        line = lines[0] if lines[0] != "targets ok" else lines[1]
        assert line == said[want[0]] % tuple(x for x in want[1:] if x is not None), (name, line)
        assert not any(l.startswith("P ") for l in lines)
        assert morph.check_targets(first, ev, dp, dn, nv, n_entries=ne) == want, name
    t = MS.targets(b)
    ids, w = SS.scene_a_binding(b)
    assert morph.check_targets(*t, nv, has_normals=False) == ("normals", None, None)
    assert morph.check_targets(t[0], t[1], t[2], None, nv, has_normals=False) is None
    for given in ((ids, None, SS.N_BONES), (None, w, SS.N_BONES), (ids, w, 0), (None, None, SS.N_BONES)):
        assert morph.check_targets(*t, nv, bone_ids=given[0], bone_weights=given[1], n_bones=given[2]) == ("bones", None, None)
    assert morph.check_targets(*t, nv, bone_ids=ids, bone_weights=w, n_bones=SS.N_BONES) is None
    bad_ids, bad_w, vert, _ = SS.bad_bindings(b)["a NaN weight"]
    assert morph.check_targets(*t, nv, bone_ids=bad_ids, bone_weights=bad_w, n_bones=SS.N_BONES) == ("skin", vert, "weight")
    # two faults: the table's comes first, then the entry with the smaller number
    first, ev, dp, dn = (x.copy() for x in t)
    dp[3, 0] = np.nan
    ev[int(first[1]) + 2] = nv + 7
    assert morph.check_targets(first, ev, dp, dn, nv) == ("vertex", 1, int(first[1]) + 2)      # every vertex is looked at before any delta
    assert _run(program, tmp_path, "two", b, (first, ev, dp, dn), MS.weights("a"))[1] == "entries refused vertex target 1 entry %d" % (int(first[1]) + 2)


# ---------------------------------------------------------------------------------------------------------------------------- the identities
@SCENES
def test_zero_weights_return_the_rest_bits_and_with_bones_the_skin(indexed):
    """All-zero weights (zeros of either sign): every target is skipped -- the rest pose comes back BIT FOR BIT, the -0.0 coordinate included (p + 0
    would have made it +0.0), and T5's 1e6 with it; with bones the result is skin_reference's, bit for bit."""
    from toyraygun_amd import morph, skin
    b = MS.scene(indexed)
    t = MS.targets(b)
    ids, w = SS.scene_a_binding(b)
    pos, nrm = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t, MS.weights(MS.ZERO))
    assert np.array_equal(pos.view(np.uint32), b["positions"].view(np.uint32)) and np.array_equal(nrm.view(np.uint32), b["normals"].view(np.uint32))
    if indexed:
        assert np.signbit(pos[MS.minus_zero_vertex(b), 1])
    for seed in MS.BONE_SEEDS:
        bones = SS.scene_a_bones(seed)
        pos, nrm = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t, MS.weights(MS.ZERO), ids, w, bones)
        ref = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, bones)
        assert np.array_equal(pos.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(nrm.view(np.uint32), ref[1].view(np.uint32))


@SCENES
def test_the_fused_form_is_the_skin_of_the_bone_free_morph(program, tmp_path, indexed):
    """skin_reference applied to the bone-free morph_reference output equals what the HEADER computes in one go under bones, bit for bit (the
    header's corner function normalises a touched corner and then transforms it: the composition, by construction)."""
    from toyraygun_amd import morph, skin
    b = MS.scene(indexed)
    t = MS.targets(b)
    ids, w = SS.scene_a_binding(b)
    for name, seed in (("a", 1), ("c", 3)):
        bones = SS.scene_a_bones(seed)
        free = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t, MS.weights(name))
        ref = skin.skin_reference(free[0], free[1], b["indices"], ids, w, bones)
        lines = _run(program, tmp_path, "fused", b, t, MS.weights(name), (ids, w), bones)
        assert np.array_equal(_words(lines, "P"), ref[0].view(np.uint32)) and np.array_equal(_words(lines, "N"), ref[1].view(np.uint32))
        fused = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t, MS.weights(name), ids, w, bones)
        assert np.array_equal(fused[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(fused[1].view(np.uint32), ref[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------- the builders' rules
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_the_test_targets_keep_every_box_and_every_quad(tmp_path):
    """The condition the GPU tests rely on, with zero exceptions: scene A morphed under every weight vector of tests/morph_scenes.py, alone and
    followed by scene_a_bones of every seed, per corner and indexed -- all 32 cubes still pass the builder's box rule (through the refit_check
    shim) and all 193 quad leaves the quad rule.  And the refusal the GPU test provokes is one: all copies of one top corner of cube 9 moved by
    0.02 fail exactly one box and three quads."""
    from tests.test_refit_host import build_shim
    from toyraygun_amd import morph
    shim = build_shim(str(tmp_path / "librefit_check.so"))
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)

    def rules(b, pos):
        idx, nv, nt = b["indices"], pos.shape[0], 706
        boxes = [shim.rf_host_box(_p(pos), _p(idx), nv, nt, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) for i in range(RS.N_CUBES)]
        quads = [shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 2 * q, 2 * q + 1) for q in range(1 + 6 * RS.N_CUBES)]
        return boxes, quads
    for indexed in (False, True):
        b = MS.scene(indexed)
        t = MS.targets(b)
        ids, w = SS.scene_a_binding(b)
        for name in list(MS.WEIGHTS) + [MS.ZERO]:
            for seed in (None,) + MS.BONE_SEEDS:
                skin_args = () if seed is None else (ids, w, SS.scene_a_bones(seed))
                pos, _ = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t, MS.weights(name), *skin_args)
                boxes, quads = rules(b, pos)
                assert all(v == 1 for v in boxes) and all(v == 1 for v in quads), (indexed, name, seed, boxes.count(0), quads.count(0))
        t1 = MS.targets(b, one_corner=True)
        n_moved = int(t1[0][MS.EMPTY + 1] - t1[0][MS.EMPTY])
        assert n_moved == 1 if indexed else n_moved >= 3                         # (per corner: every copy of that corner)
        tw = MS.weights("a").copy()
        pos, _ = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t1, tw)      # its weight is zero: the cube it was
        boxes, quads = rules(b, pos)
        assert all(v == 1 for v in boxes) and all(v == 1 for v in quads)
        tw[MS.EMPTY] = 1.0
        pos, _ = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t1, tw)
        boxes, quads = rules(b, pos)
        assert boxes.count(0) == 1 and boxes[MS.REFUSED_CUBE] == 0 and quads.count(0) == 3, (boxes.count(0), quads.count(0))


# ---------------------------------------------------------------------------------------------------------------------------- morph_reference
def _float64_morph(b, t, tw, binding=None, bones=None):
    """The same morph evaluated in float64 from the float32 inputs: p = rest + sum_k w_k d_k, n = the unit vector along rest + sum_k w_k dn_k for a
    corner with an active entry; then, with bones, the float64 linear blend of tests/test_skin_host.py."""
    from tests.test_skin_host import _float64_blend
    first, ev, dp, dn = t
    pos, nrm, idx = b["positions"].astype(np.float64), b["normals"].astype(np.float64), b["indices"].astype(np.int64)
    acc = np.zeros((pos.shape[0], 3))
    touched = np.zeros(pos.shape[0], bool)
    for k in range(first.shape[0] - 1):
        if tw[k] != 0:
            e = slice(int(first[k]), int(first[k + 1]))
            pos[ev[e]] += float(tw[k]) * dp[e].astype(np.float64)
            acc[ev[e]] += float(tw[k]) * dn[e].astype(np.float64)
            touched[ev[e]] = True
    n = nrm + acc[idx]
    nrm = np.where(touched[idx][:, None], n / np.linalg.norm(n, axis=1, keepdims=True), nrm)
    if bones is None:
        return pos, nrm
    return _float64_blend(dict(positions=pos, normals=nrm, indices=b["indices"]), binding[0], binding[1], bones)


@SCENES
def test_morph_reference_against_a_float64_evaluation(indexed):
    """fp32 against float64, under every weight vector and every bone seed the GPU tests use.  The largest position error is counted in ulps of the
    scene's extent (the vertices no triangle names relative to their own size: one is 1e6 away), the largest normal error absolutely; both are
    printed, and asserted at twice what this reference showed on these scenes when the unit was written -- not at the skin unit's 16 ulp."""
    from toyraygun_amd import morph
    b = MS.scene(indexed)
    t = MS.targets(b)
    binding = SS.scene_a_binding(b)
    named = SS._objects(b) >= 0
    for with_bones in (False, True):
        worst_pos = worst_nrm = 0.0
        for name in MS.WEIGHTS:
            for seed in (MS.BONE_SEEDS if with_bones else (None,)):
                tw = MS.weights(name)
                bones = None if seed is None else SS.scene_a_bones(seed)
                skin_args = () if seed is None else (binding[0], binding[1], bones)
                pos, nrm = morph.morph_reference(b["positions"], b["normals"], b["indices"], *t, tw, *skin_args)
                ref_pos, ref_nrm = _float64_morph(b, t, tw, binding, bones)
                extent = max(np.abs(ref_pos[named]).max(), np.abs(b["positions"][named]).max())
                err = np.abs(pos[named] - ref_pos[named]).max() / (2.0 ** -23 * extent)
                if (~named).any():
                    err = max(err, (np.abs(pos[~named] - ref_pos[~named]) / (2.0 ** -23 * np.abs(ref_pos[~named]).max(axis=1, keepdims=True))).max())
                worst_pos, worst_nrm = max(worst_pos, err), max(worst_nrm, np.abs(nrm - ref_nrm).max())
        print("morph_reference vs float64, %s, bones %d: positions %.3f ulp of the extent, normals %.3e" % ("indexed" if indexed else "per corner", with_bones, worst_pos, worst_nrm))
        assert worst_pos <= POS_ULP_BAR[with_bones] and worst_nrm <= NRM_BAR[with_bones]


@SCENES
def test_pose_and_one_hot_skin_share_one_normal_transform_bit_for_bit(indexed):
    """pose_reference and skin_reference call ONE normal transform (toyraygun_amd/_binding.py): handed random affine matrices per object, and the
    same matrices blended with one-hot weights (1 B + 0 B' = B exactly while no entry of B is zero), it gives the same bits -- what
    test_one_hot_weights_are_trg_pose_apply asserts of the device.  A vertex no triangle names keeps its place under a pose and follows the
    identity bone here."""
    from toyraygun_amd import pose, skin
    b = MS.scene(indexed)
    ids, w, nb = SS.one_hot(b)
    named = SS._objects(b) >= 0
    for seed in (1, 2, 3):
        X = np.random.default_rng(4100 + seed).normal(size=(PS.N_OBJECTS_A, 12)).astype(np.float32)
        X[seed] *= np.float32(-1.0)                                         # one object mirrored against the others, whatever its sign was
        assert (X != 0).all()
        p_pos, p_nrm = pose.pose_reference(b["positions"], b["normals"], b["indices"], PS.scene_a_first(), X)
        s_pos, s_nrm = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, np.concatenate([X, SS.identity(1)]))
        assert (p_nrm != b["normals"]).any()
        assert np.array_equal(p_nrm.view(np.uint32), s_nrm.view(np.uint32))
        assert np.array_equal(p_pos[named].view(np.uint32), s_pos[named].view(np.uint32))
