"""Host-side checks of the refit unit (include/trg_refit.h, toyraygun_amd/refit.py, toyraygun_amd/csrc/trg_refit_math.h): the exported surface, the
files it must leave alone, and the arithmetic the kernels apply -- evaluated on the CPU from the same header -- against the builders.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import refit_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trg_refit.h")
CSRC = os.path.join(ROOT, "toyraygun_amd", "csrc")
HELPER = os.path.join(ROOT, "tests", "helpers", "refit_check.cpp")


def build_shim(so):
    """tests/helpers/refit_check.cpp as the shared object `so`: the header's functions behind a C interface."""
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-DREFIT_SHARED", "-I" + CSRC, HELPER, "-o", so])
    L = C.CDLL(so)
    L.rf_host_area.restype = L.rf_host_area_blocks.restype = C.c_double
    return L


def test_library_exports_and_python_binds_every_declared_symbol(built):
    from toyraygun_amd import capi, denoise, refit
    declared = sorted(set(denoise.header_symbols(HEADER)))
    assert declared == ["trg_group_refit_scene", "trg_refit_last", "trg_refit_release", "trg_refit_scene"]
    out = subprocess.run(["nm", "-D", "--defined-only", capi.HIP_SO], capture_output=True, text=True).stdout
    for name in declared:
        assert re.search(r"\bT %s\b" % name, out), "libtoyraygun_hip.so does not export %s" % name
    assert sorted(refit.SYMBOL_NAMES) == declared
    L = refit.load()
    for name in declared:
        assert getattr(L, name).argtypes is not None
    # the info block as the header lays it out: 8 dwords, 8 floats, 3 doubles
    assert C.sizeof(refit.Info) == 88 and refit.Info.ms.offset == 64 and refit.Info.lo.offset == 32


def test_render_abi_and_hashed_kernel_sources_are_untouched(built):
    from toyraygun_amd import capi, refit
    from toyraygun_amd.srchash import kernel_source_files, kernel_source_hash
    trg_h = open(os.path.join(ROOT, "include", "trg.h")).read()
    for name in refit.SYMBOL_NAMES + ["trg_refit_info"]:
        assert name not in trg_h and name not in capi.SYMBOL_NAMES
    assert not any("refit" in os.path.basename(p) for p in kernel_source_files())
    with open(os.path.join(ROOT, "profiles", "r05", "c2_counters.json")) as f:
        assert json.load(f)["kernel_source_hash"] == kernel_source_hash()


def test_refit_arithmetic_against_fresh_builds_under_sanitizers(tmp_path):
    """tests/helpers/refit_check.cpp as a program, with -fsanitize=address,undefined: scenes of a floor, 1 ... 700 cubes, lone triangles and lone quads
    -- a 60-cube one a second time as an INDEXED mesh: shared corners, a shuffled vertex buffer, two vertices that no triangle names -- are built
    with box leaves, moved (identity, small, large: per-cube rigid-plus-shear maps) and refitted by the header's functions in the order the
    kernels apply them.  Asserted: the bounds are those of the vertices the triangles name; the passes settle in max(depth4, depth4_box); the quad marks read off the leaf codes are the builder's; the strict
    rows are bitwise those of a fresh build of the moved geometry; every box -- parallelepiped or lone quad -- still passes the builder's test and its
    frame is the fresh build's (measured difference: 0, the two evaluate the same double expressions); every triangle lies inside the decoded box of
    every ancestor in BOTH node flavours; and the identity motion reproduces both loaded node arrays word for word."""
    exe = str(tmp_path / "refit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-pthread",
                           "-fno-omit-frame-pointer", "-I" + CSRC, HELPER, os.path.join(CSRC, "bvh_build.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, TRG_BVH_THREADS="4"))
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "refit check: every scene passed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    ident = re.findall(r"identity n (\d+): plain nodes differ in (\d+) of (\d+) words, box flavour in (\d+) of (\d+)", r.stdout)
    assert len(ident) == 6 and all(int(a) == 0 and int(c) == 0 and int(b) > 0 and int(d) > 0 for _, a, b, c, d in ident)
    assert "box frames against the fresh build: worst difference 0\n" in r.stdout
    assert r.stdout.count("leaves walked") == 18                          # six scenes, one of them indexed, three motions each
    shared = re.search(r"indexed n 60: (\d+) corners are (\d+) vertices", r.stdout)
    assert shared and int(shared.group(2)) < int(shared.group(1)) // 3


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """The same helper as a shared object: the header's functions behind a C interface."""
    return build_shim(str(tmp_path_factory.mktemp("refit") / "librefit_check.so"))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _leaf_records(capi, b):
    L = capi.load()
    args = (_p(b["positions"]), _p(b["normals"]), _p(b["colors"]), _p(b["indices"]), _p(b["material_ids"]), b["positions"].shape[0], b["material_ids"].shape[0])
    n = C.c_uint32()
    assert L.trg_debug_leaf_records(*args, None, 0, C.byref(n)) == capi.OK
    rec = np.zeros((n.value, 32), np.float32)
    assert L.trg_debug_leaf_records(*args, _p(rec), n.value, C.byref(n)) == capi.OK
    return rec


def _header_over_the_debug_arrays(shim, make):
    """The checks of test_header_over_the_debug_arrays_of_scene_a on the buffers make(step) gives for steps 0 .. 3.  Returns, per step, what the header
    re-derived: the strict rows and plane rows by primitive index, the cubes' box frames, the refitted node array."""
    from toyraygun_amd import capi
    b0 = make(0)
    nv, nt = b0["positions"].shape[0], b0["material_ids"].shape[0]
    assert nt == RS.FLOOR_TRIS + RS.CUBE_TRIS + RS.SPHERE_TRIS == 706
    nodes0 = capi.debug_build_bvh4q(b0["positions"], b0["indices"], b0["material_ids"])
    _, depth4 = capi.debug_build_bvh4(b0["positions"], b0["indices"], b0["material_ids"])
    rec0 = _leaf_records(capi, b0)
    prim = np.ascontiguousarray(rec0[:, 3].view(np.uint32))
    assert sorted(prim.tolist()) == list(range(nt))
    boxes0 = capi.debug_boxes(b0["positions"], b0["indices"], b0["material_ids"])
    assert boxes0.shape[0] == RS.N_CUBES                                   # every rotated cube is a box leaf
    worst_plane = worst_frame = 0.0
    derived = []
    for step in (0, 1, 2, 3):
        b = make(step)
        pos, idx = b["positions"], b["indices"]
        lo, hi, ctr, pad = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_float()
        shim.rf_host_bounds(_p(pos), _p(idx), nv, nt, _p(lo), _p(hi), _p(ctr), C.byref(pad))
        assert np.array_equal(lo, pos[idx].min(0)) and np.array_equal(hi, pos[idx].max(0))   # of the vertices the triangles name, no others
        planes_f, _, ctr_f = capi.debug_plane_records(pos, idx, b["material_ids"])
        assert np.array_equal(ctr, ctr_f)
        out = np.zeros_like(nodes0)
        quadx = np.zeros(rec0.shape[0], np.uint8)
        assert shim.rf_host_nodes(_p(pos), _p(idx), nv, nt, _p(nodes0), nodes0.shape[0], _p(prim), prim.shape[0], depth4, pad, _p(out), _p(quadx)) == 1
        assert int(quadx.sum()) == 1 + 6 * RS.N_CUBES                      # the floor and six faces per cube
        assert shim.rf_host_contained(_p(pos), _p(idx), nv, nt, _p(out), out.shape[0], _p(prim), prim.shape[0]) == 1
        assert np.array_equal(out[:, 12:], nodes0[:, 12:])                 # child codes and unused slots do not change
        if step == 0:
            assert np.array_equal(out, nodes0)                             # identity motion: the loaded node array, word for word
        else:
            assert shim.rf_host_contained(_p(pos), _p(idx), nv, nt, _p(nodes0), nodes0.shape[0], _p(prim), prim.shape[0]) == 0   # (the check can fail: the stale tree does)
        rec = rec0.copy()
        planes = np.zeros((rec.shape[0], 12), np.float32)
        shim.rf_host_records(_p(pos), _p(idx), nv, nt, _p(rec), rec.shape[0], _p(quadx), _p(ctr), _p(planes))
        rec_f = _leaf_records(capi, b)
        prim_f = rec_f[:, 3].view(np.uint32)
        at = np.empty(nt, np.int64)
        at[prim_f] = np.arange(nt)
        rows = [0, 1, 2, 4, 5, 6, 8, 9, 10]
        assert np.array_equal(rec[:, rows].view(np.uint32), rec_f[at[prim]][:, rows].view(np.uint32))
        # a fresh build may pair or order a quad's records differently only if the geometry said so; here it does not: same X records, same planes
        worst_plane = max(worst_plane, float(np.abs(planes.astype(np.float64) - planes_f[at[prim]].astype(np.float64)).max()))
        assert np.array_equal(planes.view(np.uint32), planes_f[at[prim]].view(np.uint32))
        boxes_f = capi.debug_boxes(pos, idx, b["material_ids"])
        assert boxes_f.shape[0] == RS.N_CUBES
        frames = np.zeros((RS.N_CUBES, 24), np.float32)
        for i in range(RS.N_CUBES):
            frame, rows12 = frames[i, :12], frames[i, 12:]
            assert shim.rf_host_box(_p(pos), _p(idx), nv, nt, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) == 1
            j = int(np.argmin(np.abs(boxes_f[:, 2:5] - frame[:3]).sum(1)))
            worst_frame = max(worst_frame, float(np.abs(boxes_f[j, 2:14].astype(np.float64) - frame).max()))
            assert np.array_equal(boxes_f[j, 2:14].view(np.uint32), frame.view(np.uint32))
            assert np.array_equal(rows12.reshape(3, 4)[:, :3].reshape(-1), frame[3:])
        by_prim = np.argsort(prim)
        derived.append(dict(rows=rec[by_prim][:, rows].copy(), planes=planes[by_prim].copy(), frames=frames, nodes=out, pad=pad.value, center=ctr))
    print("plane rows: worst difference %g; box frames: %g" % (worst_plane, worst_frame))
    return derived


def test_header_over_the_debug_arrays_of_scene_a(built, shim):
    """The header driven over what trg_debug_build_bvh4q, trg_debug_leaf_records, trg_debug_plane_records and trg_debug_boxes return for scene A,
    then the vertices move (three steps).  Matched by primitive index, the re-derived records against a fresh debug build of the moved geometry:
    strict rows bitwise; plane rows bitwise too -- MEASURED HERE: 0 ulp on every step, because trg_capi.cpp fill_plane_record and the header's
    plane_rows are the same double expressions, neither contracted (x86-64 without FMA on the host, `fp contract(off)` in the header) --; box frames
    (centre and rows of trg_debug_boxes) bitwise for the same reason.  Every triangle inside every ancestor's decoded box; identity reproduces the
    loaded node array."""
    assert len(_header_over_the_debug_arrays(shim, RS.scene_a)) == 4


def test_refusal_rules_on_the_host(built, shim):
    """What the device path refuses, by the same functions: a cube corner moved by 1e-3 of its edge breaks the quads that meet there and the box; a
    bent quad is no parallelogram; the unmoved scene passes."""
    b = RS.scene_a(1)
    pos, idx = b["positions"].copy(), b["indices"]
    nv, nt = pos.shape[0], b["material_ids"].shape[0]
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)
    k0 = RS.cube_first_triangle(9)
    assert shim.rf_host_box(_p(pos), _p(idx), nv, nt, k0, _p(ctr), _p(frame), _p(rows12)) == 1
    assert all(shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, k0 + 2 * q, k0 + 2 * q + 1) == 1 for q in range(6))
    corner = pos[3 * k0].copy()
    edge = float(np.linalg.norm(pos[3 * k0 + 1] - pos[3 * k0]))
    pos[(pos == corner).all(1)] += np.float32(1e-3 * edge)
    assert shim.rf_host_box(_p(pos), _p(idx), nv, nt, k0, _p(ctr), _p(frame), _p(rows12)) == 0
    assert sum(shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, k0 + 2 * q, k0 + 2 * q + 1) for q in range(6)) == 3
    pos = b["positions"].copy()
    assert shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 0, 1) == 1
    pos[5, 1] += np.float32(0.01)                                          # the floor's fourth corner leaves its plane
    assert shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 0, 1) == 0
    assert shim.rf_host_quad_still(_p(b["positions"]), _p(idx), nv, nt, 1, 0) == 0    # (the pair the other way round is not what the builder made)


def test_header_over_the_debug_arrays_of_indexed_scene_a(built, shim):
    """The same checks on scene A as an INDEXED mesh (162 shared sphere vertices, 8 corners per cube, the vertex buffer permuted, two vertices that
    no triangle names, one of them at (1e6, -1e6, 1e6)): they are the same triangles, so everything the header re-derives -- strict rows, plane rows,
    box frames, node arrays, padding and centre -- is bitwise what it re-derives from the unindexed scene A at the same step; and the bounds are
    those of the indexed vertices only (asserted inside, against positions[indices])."""
    plain = _header_over_the_debug_arrays(shim, RS.scene_a)
    indexed = _header_over_the_debug_arrays(shim, RS.scene_a_indexed)
    for step, (a, b) in enumerate(zip(plain, indexed)):
        assert a["pad"] == b["pad"] and np.array_equal(a["center"], b["center"]), step
        for what in ("rows", "planes", "frames", "nodes"):
            assert np.array_equal(a[what].view(np.uint32), b[what].view(np.uint32)), (step, what)
    b = RS.scene_a_indexed(1)
    used = np.zeros(b["positions"].shape[0], bool)
    used[b["indices"]] = True
    assert b["positions"].shape[0] == RS.N_VERTS_INDEXED and int((~used).sum()) == 2
    assert np.abs(b["positions"][~used]).max() == 1e6 and np.abs(b["positions"][used]).max() < 3.0
    assert not np.array_equal(b["indices"], np.sort(b["indices"]))


def test_moved_lattice_keeps_every_box_and_every_quad(built, shim, O):
    """The condition the large GPU tests rely on: in cornell_lattice_moved(28, 1) -- 21,952 cubes translated by exactly representable steps, a tenth
    of them also turned -- every cube still passes the builder's 1e-5 corner rule (rf_host_box) and every face is still the parallelogram it was
    (rf_host_quad_still, in the order the unmoved scene pairs it); one cube whose triangles all lie beyond the first grid stride of 262,144 sets hi.x
    and lo.y alone; and the host builder finds a box in every cube, before and after."""
    from toyraygun_amd import capi
    n = 28
    b0, b = RS.cornell_lattice_moved(O, n, 0), RS.cornell_lattice_moved(O, n, 1)
    nv, nt = b["positions"].shape[0], b["material_ids"].shape[0]
    assert nt == 263460 and np.array_equal(b["indices"], b0["indices"])
    moved = (b["positions"] != b0["positions"]).any(1).reshape(-1, 36).any(1)
    assert not moved[:3].any() and moved[3:].mean() > 0.9                  # the Cornell box stays; the cubes move
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)
    for pos in (b0["positions"], b["positions"]):
        refused = [k for k in range(n ** 3) if shim.rf_host_box(_p(pos), _p(b["indices"]), nv, nt, RS.LATTICE_FIRST_CUBE_TRI + 12 * k, _p(ctr), _p(frame), _p(rows12)) != 1]
        assert not refused, (len(refused), refused[:8])

    def pairing(pos):
        return np.array([shim.rf_host_quad_still(_p(pos), _p(b["indices"]), nv, nt, 2 * q, 2 * q + 1) + 2 * shim.rf_host_quad_still(_p(pos), _p(b["indices"]), nv, nt, 2 * q + 1, 2 * q)
                         for q in range(nt // 2)])
    was, now = pairing(b0["positions"]), pairing(b["positions"])
    assert (was > 0).all() and np.array_equal(was, now)
    far = b["positions"][-36:]
    first_tri = RS.LATTICE_FIRST_CUBE_TRI + 12 * (n ** 3 - 1)
    assert first_tri >= 262144 and first_tri + 12 == nt
    rest = b["positions"][:-36]
    assert far[:, 0].max() > rest[:, 0].max() + 1.0 and far[:, 1].min() < rest[:, 1].min() - 1.0
    assert rest[:, 2].max() >= far[:, 2].max() and rest[:, 2].min() <= far[:, 2].min()
    for x in (b0, b):
        assert capi.debug_boxes(x["positions"], x["indices"], x["material_ids"]).shape[0] >= n ** 3


def test_box_leaves_far_from_the_origin_on_the_host(shim):
    """Scene A translated by (5000, -3000, 800) and rounded to float32 once per corner: a cube of half edge 0.05 .. 0.09 there has corners half an
    ulp (2.4e-4) off, far beyond the builder's 1e-5 corner rule -- the refit must refuse such a box, by its stated contract, and the GPU test of the
    far scene therefore moves the floor and the sphere only.  MEASURED: 1 of the 32 cubes still passes at that distance; all 192 faces stay quads."""
    ctr, frame, rows12 = np.zeros(3, np.float32), np.zeros(12, np.float32), np.zeros(12, np.float32)
    for cubes, every_box in ((True, False), (False, True)):
        b = RS.scene_a_far(1, cubes=cubes)
        pos, idx = b["positions"], b["indices"]
        nv, nt = pos.shape[0], b["material_ids"].shape[0]
        ok = sum(shim.rf_host_box(_p(pos), _p(idx), nv, nt, RS.cube_first_triangle(i), _p(ctr), _p(frame), _p(rows12)) for i in range(RS.N_CUBES))
        print("cubes moved far: %s -- %d of %d cubes pass the corner rule" % (cubes, ok, RS.N_CUBES))
        assert (ok == RS.N_CUBES) == every_box
        assert all(shim.rf_host_quad_still(_p(pos), _p(idx), nv, nt, 2 * q, 2 * q + 1) == 1 for q in range(1 + 6 * RS.N_CUBES))


def test_area_sum_in_the_kernels_order(shim):
    """rf_host_area_blocks (the order rf_area_kernel adds in) against the plain sum over the same nodes: the same number to rounding, not a new one."""
    from toyraygun_amd import capi
    b = RS.scene_a(0)
    nodes = capi.debug_build_bvh4q(b["positions"], b["indices"], b["material_ids"])
    a, blocks = shim.rf_host_area(_p(nodes), nodes.shape[0]), shim.rf_host_area_blocks(_p(nodes), nodes.shape[0])
    assert a > 0 and abs(a - blocks) <= 1e-12 * a
