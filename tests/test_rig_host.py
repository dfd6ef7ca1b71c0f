"""Host-side checks of the rig unit (include/trg_rig.h, toyraygun_amd/rig.py, toyraygun_amd/csrc/trg_rig_math.h): the exported surface, the files it
must leave alone, the header's arithmetic, validators and level table -- run by a stand-alone program under the host sanitizers -- against
rig_reference, rig_reference against a float64 evaluation, check_rig on every malformed table, and the condition the GPU tests rely on: rig A's
bones keep every box and every quad leaf of scene A.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import refit_scenes as RS
from tests import rig_scenes as GS
from tests import skin_scenes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_rig.h")
CSRC = os.path.join(ROOT, "toyraygun_amd", "csrc")
HELPER = os.path.join(ROOT, "tests", "helpers", "rig_check.cpp")
DECLARED = ["trg_group_rig_bind", "trg_group_rig_morph_apply", "trg_group_rig_skin_apply", "trg_rig_bind", "trg_rig_buffers", "trg_rig_evaluate", "trg_rig_morph_apply",
            "trg_rig_morph_apply_device", "trg_rig_read", "trg_rig_release", "trg_rig_skin_apply", "trg_rig_skin_apply_device"]
CODES = {"counts": (1,), "parent": (2,), "table": (3, 4, 5), "time": (6,), "ts": (7,), "rotation": (8,), "clock": (9,), "inv_bind": (10,)}   # trg::rig's enum


def test_library_exports_and_python_binds_every_declared_symbol(built):
    from toyraygun_amd import capi, denoise, rig
    declared = sorted(set(denoise.header_symbols(HEADER)))
    assert declared == DECLARED
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(rig.SYMBOL_NAMES) == declared
    L = rig.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None


def test_other_headers_and_hashed_kernel_sources_are_untouched(built):
    from toyraygun_amd import capi, denoise, morph, pose, refit, rig, skin
    from toyraygun_amd.srchash import kernel_source_files, kernel_source_hash
    others = [open(os.path.join(ROOT, "include", h)).read() for h in ("trg.h", "trg_refit.h", "trg_pose.h", "trg_skin.h", "trg_morph.h", "trg_denoise.h")]
    lists = [capi.SYMBOL_NAMES, refit.SYMBOL_NAMES, pose.SYMBOL_NAMES, skin.SYMBOL_NAMES, morph.SYMBOL_NAMES, denoise.SYMBOL_NAMES]
    for name in rig.SYMBOL_NAMES:
        assert not any(name in text for text in others)
        assert not any(name in names for names in lists)
    assert not any("rig" in os.path.basename(p) for p in kernel_source_files())
    for p in kernel_source_files():
        with open(p, errors="replace") as f:
            assert "trg_rig" not in f.read(), p
    with open(os.path.join(ROOT, "profiles", "r05", "c2_counters.json")) as f:
        assert json.load(f)["kernel_source_hash"] == kernel_source_hash()


# ---------------------------------------------------------------------------------------------------------------------------- the sanitizer program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/helpers/rig_check.cpp with -fsanitize=address,undefined: a program of its own, nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("rig") / "rig_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-fno-omit-frame-pointer", "-I" + CSRC, HELPER, "-o", exe])
    return exe


def _run(program, tmp_path, name, r, clock_vectors):
    clocks = np.ascontiguousarray(clock_vectors, np.float32).reshape(-1, max(r["n_clocks"], 1))
    path = str(tmp_path / (name + ".bin"))
    with open(path, "wb") as f:
        f.write(np.array([r["parent"].shape[0], r["keys"].shape[0], r["n_clocks"], 0 if r["inv_bind"] is None else 1, clocks.shape[0]], np.uint32).tobytes())
        f.write(r["parent"].astype(np.uint32).tobytes() + r["key_first"].astype(np.uint32).tobytes() + r["keys"].astype(np.float32).tobytes() +
                r["clock_of"].astype(np.uint32).tobytes())
        if r["inv_bind"] is not None:
            f.write(r["inv_bind"].astype(np.float32).tobytes())
        f.write(clocks.tobytes() if r["n_clocks"] else b"")
    p = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-500:], p.stderr[-2000:])
    return p.stdout.splitlines()


def _matrices(lines, n_joints, n_vectors):
    def words(tag):
        return np.array([[int(w, 16) for w in l.split()[1:]] for l in lines if l.startswith(tag + " ")], np.uint32).reshape(n_vectors, n_joints, 12)
    return words("B"), words("W")


@pytest.mark.parametrize("which", ["A", "B"])
def test_header_evaluates_the_rigs_to_the_bits_of_rig_reference(program, tmp_path, which):
    """Rigs A and B under every clock vector of tests/rig_scenes.py, evaluated by the header's functions in the sanitized program on arrays of
    exactly the stated sizes: validators pass, the level table is rig.level_table's, bones and world are rig_reference's, bit for bit."""
    from toyraygun_amd import rig
    r = GS.rig_a() if which == "A" else GS.rig_b()
    vectors = GS.CLOCKS_A if which == "A" else GS.clocks_b(r)
    assert rig.check_rig(*GS.args(r)) is None
    n = r["parent"].shape[0]
    lines = _run(program, tmp_path, which, r, list(vectors.values()))
    # the fallback: a pair of zero length, one whose length overflows -- the first rotation's bits
    assert [l for l in lines if l.startswith("F ")] == ["F 00000000 80000000 00000000 00000000", "F %08x %08x %08x 3f800000" % ((np.float32(3e38).view(np.uint32),) * 2 + (np.float32(-3e38).view(np.uint32),))]
    assert "check ok" in lines
    order, level_first = rig.level_table(r["parent"])
    assert "levels %d" % (level_first.shape[0] - 1) in lines
    assert [l for l in lines if l.startswith("O ")] == ["O " + " ".join(str(j) for j in order)]
    assert [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("L ")] == [(l, int(level_first[l]), int(level_first[l + 1] - level_first[l])) for l in range(level_first.shape[0] - 1)]
    got_b, got_w = _matrices(lines, n, len(vectors))
    for v, (name, clocks) in enumerate(vectors.items()):
        bones, world = GS.reference(r, clocks)
        assert np.array_equal(got_b[v], bones.view(np.uint32)), name
        assert np.array_equal(got_w[v], world.view(np.uint32)), name
        assert np.isfinite(bones).all()


def test_the_rigs_have_what_the_kernel_can_get_wrong():
    """The properties tests/rig_scenes.py promises: forests, depths, key counts, negative dots and scales, level sizes around a block, clocks before,
    on, between and past the keys."""
    from toyraygun_amd import rig
    a, b = GS.rig_a(), GS.rig_b()
    for r, roots in ((a, 3), (b, 5)):
        assert int((r["parent"] == GS.NO_PARENT).sum()) == roots
    d = rig.depths(a["parent"])
    assert a["parent"].shape[0] == SS.N_BONES and d.max() >= 8 and d[17] == 9 and list(d[33:38]) == [0, 1, 2, 1, 0]
    nk = np.diff(a["key_first"].astype(np.int64))
    assert set(nk.tolist()) == {1, 2, 7} and nk[37] == 1 and (a["keys"][a["key_first"][37], 1:4] == (1e6, -1e6, 1e6)).all()
    kf = a["key_first"].astype(np.int64)
    dots = [float(np.dot(a["keys"][i, 4:8], a["keys"][i + 1, 4:8])) for j in range(38) for i in range(kf[j], kf[j + 1] - 1)]
    assert min(dots) < -0.9 and max(dots) > 0.9 and (a["keys"][:, 8:11] < 0).any() and set(a["clock_of"].tolist()) == {0, 1}
    assert not np.array_equal(a["inv_bind"], np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (38, 1)))
    for j, lo, hi in ((0, 0.0, 2.0), (21, 0.0, 2.0)):                               # seven-key joints on clock 0 and on clock 1
        c = int(a["clock_of"][j])
        assert nk[j] == 7 and a["keys"][kf[j], 0] == lo and a["keys"][kf[j + 1] - 1, 0] == hi
        t = {name: v[c] for name, v in GS.CLOCKS_A.items()}
        assert t["before"] < lo and t["past"] >= hi and t["on a key"] in a["keys"][kf[j] + 1:kf[j + 1] - 1, 0] and lo < t["between"] < hi
    assert GS.CLOCKS_A["between"][0] > 0.5 and GS.CLOCKS_A["between"][0] < 0.75      # across the negated pair (keys 2, 3) of clock 0's seven-key tracks
    order, level_first = rig.level_table(b["parent"])
    assert b["parent"].shape[0] == 700 and tuple(np.diff(level_first.astype(np.int64))) == GS.B_LEVELS and {1, 257, 300} <= set(GS.B_LEVELS)
    assert not np.array_equal(order, np.arange(700)) and (b["keys"][:, 8:11] < 0).any()


# ---------------------------------------------------------------------------------------------------------------------------- the validators
def test_check_rig_and_the_header_refuse_each_malformed_table(program, tmp_path):
    """One case per validator of trg_rig_bind, in its order: check_rig and the header's check name the same first offender.  Two faults: the
    earlier rule wins.  A chain of 65 joints is one level too deep; 64 pass."""
    from toyraygun_amd import rig
    r = GS.rig_a()
    for name, (bad, what, joint, key, _) in GS.bad_rigs(r).items():
        said = rig.check_rig(bad["parent"], bad["key_first"], bad["keys"], bad["clock_of"], bad["n_clocks"], bad["inv_bind"])
        assert said == (what, joint, key), (name, said)
        line = [l for l in _run(program, tmp_path, "bad", bad, np.zeros(max(bad["n_clocks"], 1), np.float32)) if l.startswith("check")][0]
        code, j, k = (int(x) for x in re.match(r"check refused (\d+) joint (\d+) key (\d+)", line).groups())
        assert code in CODES[what] and j == (joint or 0) and k == (key or 0), (name, line)
    bad = GS.bad_rigs(r)["an infinite inverse bind"][0]
    bad["clock_of"][30] = 7
    bad["keys"][3, 5] = np.nan                                                  # a rotation: after times, translations and scales; before clocks
    assert rig.check_rig(*GS.args(bad))[:2] == ("rotation", 0)
    deep = GS.deep_rig(65)
    assert rig.check_rig(*GS.args(deep)) == ("depth", 64, None)
    lines = _run(program, tmp_path, "deep", deep, np.zeros(1, np.float32))
    assert "check ok" in lines and "depth refused joint 64" in lines
    ok = GS.deep_rig(64)
    assert rig.check_rig(*GS.args(ok)) is None and "levels 64" in _run(program, tmp_path, "ok", ok, np.zeros(1, np.float32))


# ---------------------------------------------------------------------------------------------------------------------------- rig_reference
def _float64_rig(r, clocks):
    """The same rig evaluated in float64 from the float32 inputs, with numpy's own matrix products."""
    kf, keys = r["key_first"].astype(np.int64), r["keys"].astype(np.float64)
    n = kf.shape[0] - 1
    world, bones = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    for j in range(n):
        t = float(np.float32(clocks[int(r["clock_of"][j])]))
        tr = keys[kf[j]:kf[j + 1]]
        if t <= tr[0, 0]:
            T, q, S = tr[0, 1:4], tr[0, 4:8], tr[0, 8:11]
        elif t >= tr[-1, 0]:
            T, q, S = tr[-1, 1:4], tr[-1, 4:8], tr[-1, 8:11]
        else:
            i = int(np.searchsorted(tr[:, 0], t, side="right")) - 1
            u = (t - tr[i, 0]) / (tr[i + 1, 0] - tr[i, 0])
            T, S = tr[i, 1:4] + u * (tr[i + 1, 1:4] - tr[i, 1:4]), tr[i, 8:11] + u * (tr[i + 1, 8:11] - tr[i, 8:11])
            qb = tr[i + 1, 4:8] if np.dot(tr[i, 4:8], tr[i + 1, 4:8]) >= 0 else -tr[i + 1, 4:8]
            q = tr[i, 4:8] + u * (qb - tr[i, 4:8])
            q = q / np.linalg.norm(q)
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = R * S[None, :], T
        p = int(r["parent"][j])
        world[j] = L if p == GS.NO_PARENT else world[p] @ L
        I = np.eye(4)
        I[:3] = r["inv_bind"][j].astype(np.float64).reshape(3, 4)
        bones[j] = world[j] @ I
    return bones[:, :3].reshape(n, 12), world[:, :3].reshape(n, 12)


# measured on these rigs (NOTEBOOK.md, "Rigs"): the largest error of rig_reference against the float64 evaluation over every clock vector --
# rig A: linear part 3.14e-7 (relative to the largest entry of the joint's matrix, at least 1), translations 3.4 ulp of the extent; rig B (12
# levels, scales to 1.3 per level): linear part 6.77e-7, translations 2.6 ulp of the extent.  The bars are twice that.
BARS = {"A": (6.3e-7, 6.8), "B": (1.36e-6, 5.2)}


@pytest.mark.parametrize("which", ["A", "B"])
def test_rig_reference_against_a_float64_evaluation(which):
    """fp32 against float64 over every clock vector: the linear parts of bones and world absolutely, relative to the largest entry of the joint's
    matrix (at least 1); the translations in ulp of the extent -- the largest translation of the evaluation (rig A leaves out joint 37, a
    million away, which is compared relative to its own size).  Each figure is printed before it is checked."""
    r = GS.rig_a() if which == "A" else GS.rig_b()
    vectors = GS.CLOCKS_A if which == "A" else GS.clocks_b(r)
    lin_bar, ulp_bar = BARS[which]
    lin_worst = ulp_worst = 0.0
    near = np.ones(r["parent"].shape[0], bool)
    if which == "A":
        near[37] = False
    for name, clocks in vectors.items():
        got = GS.reference(r, clocks)
        ref = _float64_rig(r, clocks)
        for g, f in zip(got, ref):
            g3, f3 = g.astype(np.float64).reshape(-1, 3, 4), f.reshape(-1, 3, 4)
            size = np.maximum(np.abs(f3[:, :, :3]).max(axis=(1, 2)), 1.0)
            lin_worst = max(lin_worst, float((np.abs(g3[:, :, :3] - f3[:, :, :3]).max(axis=(1, 2)) / size).max()))
            extent = np.abs(f3[near][:, :, 3]).max()
            ulp_worst = max(ulp_worst, float(np.abs(g3[near][:, :, 3] - f3[near][:, :, 3]).max() / (2.0 ** -23 * extent)))
            far = ~near
            if far.any():
                assert (np.abs(g3[far][:, :, 3] - f3[far][:, :, 3]) <= 16 * 2.0 ** -23 * np.abs(f3[far][:, :, 3]).max()).all()
    print("rig %s: linear part %.3g, translations %.3g ulp of the extent" % (which, lin_worst, ulp_worst))
    assert lin_worst <= lin_bar and ulp_worst <= ulp_bar


# ---------------------------------------------------------------------------------------------------------------------------- the builders' rules
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_rig_a_keeps_every_box_and_every_quad_of_scene_a(tmp_path):
    """The condition the GPU tests rely on: scene A skinned with rig A's bones under every clock vector, per corner and indexed -- every named
    vertex stays below 10 in magnitude (joint 37's million reached nothing), all 32 cubes pass the builder's box rule (through the refit_check
    shim) and all 193 quad leaves the quad rule; everything moves.  And the split cube of the GPU refusal test is no box under rig A."""
    from tests.test_refit_host import build_shim
    from toyraygun_amd import skin
    shim = build_shim(str(tmp_path / "librefit_check.so"))
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)
    r = GS.rig_a()

    def rules(b, ids, w, bones):
        pos, _ = skin.skin_reference(b["positions"], b["normals"], b["indices"], ids, w, bones)
        idx, nv, nt = b["indices"], pos.shape[0], 706
        boxes = [shim.rf_host_box(_p(pos), _p(idx), nv, nt, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) for i in range(RS.N_CUBES)]
        quads = [shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 2 * q, 2 * q + 1) for q in range(1 + 6 * RS.N_CUBES)]
        return pos, boxes, quads
    for make in (RS.scene_a, RS.scene_a_indexed):
        b = make(0)
        ids, w = SS.scene_a_binding(b)
        named = SS._objects(b) >= 0
        for name, clocks in GS.CLOCKS_A.items():
            bones, _ = GS.reference(r, clocks)
            pos, boxes, quads = rules(b, ids, w, bones)
            assert all(v == 1 for v in boxes) and all(v == 1 for v in quads), (name, boxes.count(0), quads.count(0))
            assert np.abs(pos[named]).max() < 10, name
            if name != "before":
                assert (pos[named] != b["positions"][named]).any(1).mean() > 0.9
    b = RS.scene_a(0)
    ids, w = SS.scene_a_binding(b, split_cube=9)
    _, boxes, quads = rules(b, ids, w, GS.reference(r, GS.CLOCKS_A["between"])[0])
    assert boxes.count(0) == 1 and boxes[9] == 0


def test_morph_targets_under_rig_a_keep_every_box_and_every_quad(tmp_path):
    """What the group test of tests/test_gpu_rig.py relies on, on the host-built tree: tests/morph_scenes.py's targets at weights "a" with rig A's
    bones behind them still form all 32 boxes and all 193 quad leaves."""
    from tests import morph_scenes as MS
    from tests.test_refit_host import build_shim
    from toyraygun_amd import morph
    shim = build_shim(str(tmp_path / "librefit_check.so"))
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)
    b = RS.scene_a(0)
    ids, w = SS.scene_a_binding(b)
    t = MS.targets(b)
    bones = GS.reference(GS.rig_a(), GS.CLOCKS_A["mixed"])[0]
    pos, _ = morph.morph_reference(b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], MS.weights("a"), bone_ids=ids, bone_weights=w, bones=bones)
    idx, nv = b["indices"], pos.shape[0]
    assert all(shim.rf_host_box(_p(pos), _p(idx), nv, 706, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) == 1 for i in range(RS.N_CUBES))
    assert all(shim.rf_host_quad_still(_p(pos), _p(idx), nv, 706, 2 * q, 2 * q + 1) == 1 for q in range(1 + 6 * RS.N_CUBES))
