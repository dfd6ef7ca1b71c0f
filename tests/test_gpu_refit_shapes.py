"""GPU tests (-m gpu) of the refit unit on the inputs tests/test_gpu_refit.py does not reach: indexed geometry (shared, permuted and unused
vertices), a scene beyond one grid stride of the reductions (263,460 triangles), device-built trees of more than a handful of nodes, the temporal
denoiser on a refitted scene, the shipped build's LDS kernels after a rebuild, geometry far from the origin and a collapsed triangle.  The
references are the ones that file uses -- the oracle's render and intersector of the moved geometry, a fresh trg_load_scene of the same buffers,
denoise.reference_motion -- and so are the bars (_strict_bars, _shipped_bars).  Images 32 x 24, 2 spp, 3 bounces; traces 4,096 rays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import refit_scenes as RS
from tests.test_gpu_refit import BOUNCES, H, HBM_KERNELS, SPP, STEPS, W, _bits, _close, _ctx, _move, _rays, _shipped_bars, _strict_bars
from tests.test_refit_host import _leaf_records, _p, build_shim
from tests.util import fast_bar

pytestmark = pytest.mark.gpu
LOCK_STEP = HBM_KERNELS[:1]
LATTICE_N = 28                                     # 21,952 cubes, 263,460 triangles: 1,316 beyond the 262,144 of one grid stride
STRIDE = 1024 * 256
LATTICE_RAYS = dict(lo=(-1.0, -1.3, -1.0), hi=(3.0, 1.95, 3.0))      # the room and the cube pushed out of it


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def refit(built):
    from toyraygun_amd import refit as r
    r.load()
    return r


@pytest.fixture(scope="module")
def dn(capi):
    from toyraygun_amd import denoise
    denoise.load()
    return denoise


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("refit_shapes") / "librefit_check.so"))


@pytest.fixture(scope="module")
def scene_a_steps(O):
    bufs = [RS.scene_a(s) for s in range(4)]
    return bufs, [RS.oracle_scene(O, b) for b in bufs]


@pytest.fixture(scope="module")
def indexed_steps(O):
    """Scene A as an indexed mesh at steps 0..3 and the oracle's scenes of positions[indices]: the triangles of scene A, so the expected images too."""
    bufs = [RS.scene_a_indexed(s) for s in range(4)]
    return bufs, [RS.oracle_scene(O, RS.unindexed(b)) for b in bufs]


def _pad32(lo, hi):
    """trg_refit_math.h scene_pad, in float32 as there."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    diag, maxabs = (hi - lo).max(), np.maximum(np.abs(lo), np.abs(hi)).max()
    return float(max(np.float32(2e-5) * max(diag, np.float32(1e-3)), np.float32(4e-6) * maxabs))


def _assert_bounds(info, b):
    """lo, hi and pad of the refit are those of the vertices the triangles name."""
    named = b["positions"][b["indices"]]
    assert np.array_equal(np.array(info["lo"], np.float32), named.min(0)) and np.array_equal(np.array(info["hi"], np.float32), named.max(0)), (info["lo"], info["hi"])
    assert info["pad"] == _pad32(named.min(0), named.max(0))


def _outcome(capi, fn):
    try:
        fn()
    except capi.TrgError as e:
        return e.code
    return capi.OK


# ---------------------------------------------------------------------------------------------------------------------------- A. indexed geometry
@pytest.mark.parametrize("gpu_build", [0, 2])
def test_indexed_scene_a(capi, refit, O, indexed_steps, gpu_build):
    """Shared vertices, a permuted vertex buffer, two vertices no triangle names (one at 1e6): the bounds are those of the named vertices, and the
    scene is scene A's under both bars -- with the host builder's tree (box leaves) and with the LBVH's."""
    bufs, scenes = indexed_steps
    rays = _rays(O, 41)
    c = _ctx(capi, O, bufs[0], gpu_build)
    try:
        assert c.stats().scene_in_lds == 0
        for s in STEPS:
            info = _move(refit, c, bufs[s])
            assert info["path"] == refit.DEVICE and info["n_records"] == 706 and info["n_quads"] > 0
            if gpu_build == 0:
                assert info["n_quads"] == 1 + 6 * RS.N_CUBES and info["n_boxes"] == RS.N_CUBES + 1
            _assert_bounds(info, bufs[s])
            what = "indexed scene A builder %d step %d" % (gpu_build, s)
            _strict_bars(capi, O, c, scenes[s], rays, what)
            _shipped_bars(capi, O, c, scenes[s], bufs[s], rays, what, gpu_build)
    finally:
        _close(c, refit)


def test_not_finite_in_a_vertex_no_triangle_names(capi, refit, O, indexed_steps):
    """What trg_load_scene does with a NaN and an infinity in a vertex that no triangle names -- MEASURED: it accepts the scene (it reads positions
    through the indices only) -- trg_refit_scene does on both of its paths, and the accepted scene is the one without that vertex, bit for bit."""
    bufs, _ = indexed_steps
    clean = bufs[1]
    dirty = RS.scene_a_indexed(1, unused=(RS.UNUSED_FAR, (np.nan, 0.5, np.inf)))
    assert not np.isfinite(dirty["positions"]).all() and np.isfinite(dirty["positions"][dirty["indices"]]).all()
    small_clean = RS.cornell_moved(O, 1, turn=0.15)
    small_dirty = dict(small_clean, positions=np.concatenate([small_clean["positions"], np.array([[np.nan, -np.inf, 0.0]], np.float32)]))
    for first, a, b, path in ((bufs[0], clean, dirty, refit.DEVICE), (RS.cornell_moved(O, 0), small_clean, small_dirty, refit.REBUILD)):
        probe = capi.Context(W, H)
        try:
            loads = _outcome(capi, lambda: probe.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"]))
        finally:
            probe.close()
        c = _ctx(capi, O, first)
        try:
            frames = []
            for x in (a, b):
                refits = _outcome(capi, lambda: refit.refit_scene(c, x["positions"], x["normals"], x["indices"]))
                assert refits == (capi.OK if x is a else loads), (path, refits, loads)
                if refits == capi.OK:
                    assert refit.refit_last(c)["path"] == path
                    _assert_bounds(refit.refit_last(c), x)
                    c.render(0, SPP, BOUNCES)
                    frames.append(c.read_accum())
            print("a vertex that is not finite and that no triangle names: trg_load_scene returns %d, trg_refit_scene (%s) the same" % (loads, refit.PATH_NAMES[path]))
            assert len(frames) < 2 or np.array_equal(_bits(frames[0]), _bits(frames[1]))
        finally:
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- B. beyond one grid stride
@pytest.fixture(scope="module")
def lattice(O):
    """cornell_lattice(28) as loaded and moved (tests/test_refit_host.py checks on the CPU that every box and quad survives the motion), and the
    oracle's scene of the moved one."""
    b0, b1 = RS.cornell_lattice_moved(O, LATTICE_N, 0), RS.cornell_lattice_moved(O, LATTICE_N, 1)
    assert np.array_equal(b1["indices"], np.arange(b1["indices"].shape[0]))
    return b0, b1, RS.oracle_scene(O, b1)


def _far_cube_sets_the_bounds(info, b1):
    far = b1["positions"][-36:]
    assert info["hi"][0] == far[:, 0].max() and info["lo"][1] == far[:, 1].min()
    _assert_bounds(info, b1)


def test_lattice_host_built_tree(capi, refit, O, lattice, shim, monkeypatch):
    """One refit of 263,460 triangles in a host-built tree with 21,954 box leaves: the bounds pass strides, the node kernels run over hundreds of
    blocks for bvh_depth4 passes.  The identity refit's area ratios are exactly 1; the moved one's is the ratio the header gives on the host, the
    doubles added in the kernels' order (rf_host_area_blocks): bitwise."""
    b0, b1, scene = lattice
    rays = _rays(O, 42, **LATTICE_RAYS)
    c = _ctx(capi, O, b0)
    try:
        assert c.stats().scene_in_lds == 0
        info = _move(refit, c, b0)
        assert info["path"] == refit.DEVICE and info["area_ratio"] == 1.0 and info["area_ratio_box"] == 1.0
        info = _move(refit, c, b1)
        assert info["path"] == refit.DEVICE and info["n_records"] == b1["material_ids"].shape[0] > STRIDE
        assert info["n_boxes"] >= LATTICE_N ** 3 and info["n_nodes_box"] > 0 and info["passes"] == c.stats().bvh_depth4 > 1
        _far_cube_sets_the_bounds(info, b1)
        monkeypatch.setenv("TRG_DEBUG_BVH_BOXES", "1")                         # the debug builds with box leaves, as trg_load_scene builds
        nodes0 = capi.debug_build_bvh4q(b0["positions"], b0["indices"], b0["material_ids"])
        prim = np.ascontiguousarray(_leaf_records(capi, b0)[:, 3].view(np.uint32))
        assert info["n_nodes"] == nodes0.shape[0] > 4 * 256
        nodes1, quadx = np.zeros_like(nodes0), np.zeros(prim.shape[0], np.uint8)
        nv, nt = b1["positions"].shape[0], prim.shape[0]
        assert shim.rf_host_nodes(_p(b1["positions"]), _p(b1["indices"]), nv, nt, _p(nodes0), nodes0.shape[0], _p(prim), nt, info["passes"], C.c_float(info["pad"]), _p(nodes1), _p(quadx)) == 1
        want = shim.rf_host_area_blocks(_p(nodes1), nodes1.shape[0]) / shim.rf_host_area_blocks(_p(nodes0), nodes0.shape[0])
        print("lattice: %.3f ms, %d passes, %d nodes, area ratio %.17g (host %.17g)" % (info["ms"], info["passes"], info["n_nodes"], info["area_ratio"], want))
        assert info["area_ratio"] == want and info["n_quads"] == int(quadx.sum())
        _strict_bars(capi, O, c, scene, rays, "lattice", kernels=LOCK_STEP)
        _shipped_bars(capi, O, c, scene, b1, rays, "lattice")
    finally:
        _close(c, refit)


def test_lattice_refusals_beyond_the_first_stride(capi, refit, O, lattice):
    """Two refusals whose offenders lie beyond triangle 262,144, each leaving the frame and the trace records as they were: of two NaNs the error
    names the smaller triangle; a corner of the far cube moved by 1e-3 of its edge is -34 and names one of that cube's triangles."""
    b0, b1, _ = lattice
    rays = _rays(O, 43, **LATTICE_RAYS)
    c = _ctx(capi, O, b0)
    try:
        _move(refit, c, b1)
        good = refit.refit_last(c)

        def state():
            c.set_option(capi.OPT_STRICT, 0)
            c.render(0, SPP, BOUNCES)
            img = c.read_accum()
            c.set_option(capi.OPT_STRICT, 1)
            tr = c.trace(rays)
            c.set_option(capi.OPT_STRICT, 0)
            return img, tr
        before = state()
        nt = b1["material_ids"].shape[0]
        t_nan = STRIDE + 5
        pos = b1["positions"].copy()
        pos[3 * t_nan + 1, 2] = np.nan
        pos[3 * (t_nan + 700), 0] = np.nan                                    # (another block's, and a higher number)
        cases = [("two NaNs", pos, -22, {t_nan})]
        k0 = nt - 12
        assert k0 >= STRIDE
        pos = b1["positions"].copy()
        cube = pos[3 * k0:]
        cube[(cube == cube[0]).all(1)] += np.float32(1e-3 * np.linalg.norm(cube[1] - cube[0]))
        assert 0 < (pos != b1["positions"]).any(1).sum() <= 9
        cases.append(("corner of the far cube", pos, -34, set(range(k0, nt))))
        for name, pos, code, offenders in cases:
            with pytest.raises(capi.TrgError) as e:
                refit.refit_scene(c, pos, b1["normals"], b1["indices"])
            msg = str(e.value)
            print("%s: %s" % (name, msg))
            assert e.value.code == code, (name, msg)
            assert int(re.search(r"triangle (\d+)", msg).group(1)) in offenders, (name, msg)
            after = state()
            assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8)), name
            assert refit.refit_last(c) == good
    finally:
        _close(c, refit)


def test_lattice_device_built_tree(capi, refit, O, lattice):
    """The same refit in the binned-SAH builder's tree: node order (every child index above its parent's), depth4 as the pass count and the quad
    marks of a large device-built tree; strict frame and traces are the oracle's."""
    b0, b1, scene = lattice
    c = _ctx(capi, O, b0, 1)
    try:
        assert c.stats().gpu_built == 1 and c.stats().scene_in_lds == 0
        info = _move(refit, c, b1)
        assert info["path"] == refit.DEVICE and info["n_boxes"] == 0 and info["n_quads"] > 6 * LATTICE_N ** 3 // 2
        assert info["passes"] == c.stats().bvh_depth4 > 1
        _far_cube_sets_the_bounds(info, b1)
        print("lattice, builder 1: %.3f ms, %d passes, %d nodes, %d quads, area ratio %.4f" % (info["ms"], info["passes"], info["n_nodes"], info["n_quads"], info["area_ratio"]))
        _strict_bars(capi, O, c, scene, _rays(O, 44, **LATTICE_RAYS), "lattice builder 1", kernels=LOCK_STEP)
    finally:
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- C. device builders on scene A
@pytest.mark.parametrize("gpu_build", [1, 2, 3])
def test_scene_a_device_built_trees(capi, refit, O, scene_a_steps, gpu_build):
    bufs, scenes = scene_a_steps
    rays = _rays(O, 45 + gpu_build)
    c = _ctx(capi, O, bufs[0], gpu_build)
    try:
        assert c.stats().gpu_built == 1 and c.stats().scene_in_lds == 0
        for s in STEPS:
            info = _move(refit, c, bufs[s])
            assert info["path"] == refit.DEVICE and info["n_records"] == 706 and info["n_boxes"] == 0 and info["n_quads"] > 0
            assert info["passes"] == c.stats().bvh_depth4
            _assert_bounds(info, bufs[s])
            what = "scene A builder %d step %d" % (gpu_build, s)
            print("%s: %.3f ms, %d passes, %d quads, area ratio %.4f" % (what, info["ms"], info["passes"], info["n_quads"], info["area_ratio"]))
            _strict_bars(capi, O, c, scenes[s], rays, what)
            _shipped_bars(capi, O, c, scenes[s], bufs[s], rays, what, gpu_build)
    finally:
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- D. the denoiser
def _close_dn(c, refit, dn):
    dn.release(c)
    _close(c, refit)


def test_denoiser_strict_build_refit_against_load(capi, refit, dn, O, scene_a_steps):
    """Two contexts on scene A (HBM, host-built, box leaves), the same uniforms, offsets and previous scene before every step; L is updated by
    trg_load_scene, R by trg_refit_scene.  Strict results do not depend on the tree: guides, positions, motion planes, centre guides, the output of
    render_temporal and the history it leaves are bitwise equal after every call."""
    bufs, _ = scene_a_steps
    kw = dict(max_history=3)
    L, R = _ctx(capi, O, bufs[0]), _ctx(capi, O, bufs[0])
    try:
        for c in (L, R):
            c.set_option(capi.OPT_STRICT, 1)
            assert c.stats().scene_in_lds == 0
        first = [dn.render_temporal(c, 0, SPP, BOUNCES, **kw) for c in (L, R)]
        assert np.array_equal(_bits(first[0]), _bits(first[1]))
        for s in STEPS:
            b, prev = bufs[s], bufs[s - 1]
            L.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            assert _move(refit, R, b)["path"] == refit.DEVICE
            for c in (L, R):
                dn.temporal_set_previous_scene(c, prev["positions"], prev["normals"], prev["indices"])
            (gl, xl, ml), (gr, xr, mr) = (dn.guides_motion(c, s * SPP) for c in (L, R))
            hit = gr[0, ..., 3] >= 0
            assert hit.any() and (np.abs(mr[0, ..., :3] - xr[..., :3]).max(-1)[hit] > 1e-3).any()      # (something in the picture did move)
            for name, x, y in (("G", gl, gr), ("X", xl, xr), ("M", ml, mr)):
                assert np.array_equal(_bits(x), _bits(y)), (s, name, int((_bits(x) != _bits(y)).sum()))
            for x, y in zip(dn.guides_centre(L, s * SPP), dn.guides_centre(R, s * SPP)):
                assert np.array_equal(_bits(x), _bits(y)), (s, "centre guides")
            out = [dn.render_temporal(c, s * SPP, SPP, BOUNCES, **kw) for c in (L, R)]
            assert np.array_equal(_bits(out[0]), _bits(out[1])), (s, "render_temporal")
            hist = [dn.temporal_history(c) for c in (L, R)]
            assert np.array_equal(_bits(hist[0]), _bits(hist[1])) and (hist[1][0, ..., 3] > 1).any(), (s, "history")
    finally:
        for c in (L, R):
            _close_dn(c, refit, dn)


def test_denoiser_shipped_build_on_a_refitted_scene(capi, refit, dn, O, scene_a_steps):
    """The shipped build's guide kernels read what the refit wrote (plane-form records, box frames, normals, sc.center): M0 and M1 are
    reference_motion of the context's own trg_raygen + trg_trace, bit for bit, as for a loaded scene; the shading normal G0.xyz is the strict
    build's where both show the same primitive -- to 1e-4: the two builds' weights differ by at most 2e-5 and the normal is a
    normalised blend of three unit normals at most 0.5 apart on this sphere, so it moves by less than 2 * 2e-5 * 0.5 * 2 --; and the trace records
    meet _shipped_bars."""
    bufs, scenes = scene_a_steps
    rays = _rays(O, 49)
    R = _ctx(capi, O, bufs[0])
    try:
        for s in STEPS:
            b, prev = bufs[s], bufs[s - 1]
            assert _move(refit, R, b)["path"] == refit.DEVICE
            dn.temporal_set_previous_scene(R, prev["positions"], prev["normals"], prev["indices"])
            R.set_option(capi.OPT_STRICT, 1)
            gs, _, _ = dn.guides_motion(R, s * SPP)
            R.set_option(capi.OPT_STRICT, 0)
            g, X, m = dn.guides_motion(R, s * SPP)
            want = dn.reference_motion(R.trace(R.raygen(s * SPP)), prev["positions"], prev["normals"], prev["indices"], g[0])
            assert np.array_equal(_bits(m), _bits(want)), (s, int((_bits(m) != _bits(want)).sum()))
            hit = g[0, ..., 3] >= 0
            same = hit & (gs[0, ..., 3] >= 0) & (_bits(g[1, ..., 3]) == _bits(gs[1, ..., 3]))
            worst = float(np.abs(g[0, ..., :3] - gs[0, ..., :3]).max(-1)[same].max())
            print("refitted scene A step %d: %d of %d hits show the strict build's primitive; normals differ by at most %.3g" % (s, int(same.sum()), int(hit.sum()), worst))
            assert same.sum() > 0.9 * hit.sum() and worst <= 1e-4
            _shipped_bars(capi, O, R, scenes[s], b, rays, "denoiser scene A step %d" % s)
    finally:
        _close_dn(R, refit, dn)


def test_plugin_temporal_denoise_with_refit(capi, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png denoise=5,temporal slide=0.02 refit: the PNG of the same line without `refit`, byte for byte (the Cornell
    box is rebuilt by the host builder either way), and three updates served by a refit."""
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")

    def run(name, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, "64", "48", "4", "3", path, "denoise=5,temporal", "slide=0.02"] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        with open(path, "rb") as f:
            return f.read(), r.stdout
    (pic, out), (plain, out_plain) = run("refit.png", "refit"), run("plain.png")
    assert "3 scene updates served by a refit" in out and "refit refused" not in out and "served by a refit" not in out_plain
    assert len(pic) > 100 and pic == plain


# ---------------------------------------------------------------------------------------------------------------------------- E. small-scene path
def _smooth_short_box(b):
    """The buffers with the short box's normals averaged per corner (smooth shading: its triangles are no longer flat)."""
    pos, nrm = b["positions"][:36], b["normals"][:36].astype(np.float64)
    out = nrm.copy()
    for i in range(36):
        n = nrm[(pos == pos[i]).all(1)].sum(0)
        out[i] = n / np.linalg.norm(n)
    normals = b["normals"].copy()
    normals[:36] = out.astype(np.float32)
    return dict(b, normals=normals)


@pytest.mark.parametrize("variant", ["flat", "flat_off", "smooth_and_back", "force_global"])
def test_small_scene_shipped_build_is_the_fresh_loads(capi, refit, O, monkeypatch, variant):
    """The Cornell box staged in LDS, its short box slid and turned, new normals given: after each refit (the rebuild path) the shipped frame and
    4,096 shipped trace records are bitwise those of a fresh context that loaded the same buffers -- the same builder, blob and flat records -- and
    the frame is inside fast_bar against the oracle.  flat_off: TRG_FLAT_SHADING=0 for both.  smooth_and_back: the scene stops being flat (step 2)
    and is flat again (step 3).  force_global: TRG_OPT_FORCE_GLOBAL set before the load; still a rebuild, the strict frame the oracle's."""
    monkeypatch.delenv("TRG_FLAT_SHADING", raising=False)
    if variant == "flat_off":
        monkeypatch.setenv("TRG_FLAT_SHADING", "0")
    rays = _rays(O, 50, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0))
    force_global = int(variant == "force_global")

    def ctx(b):
        c = capi.Context(W, H)
        c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(W, H)))
        c.set_pixel_offsets(O.pixel_offsets(W, H))
        return c

    def shipped(c):
        c.set_option(capi.OPT_STRICT, 0)
        c.reset_stats()
        c.render(0, SPP, BOUNCES)
        return c.read_accum(), c.trace(rays), c.stats()
    c = ctx(RS.cornell_moved(O, 0, turn=0.15))
    try:
        assert c.stats().scene_in_lds == 1 - force_global
        for s in STEPS:
            b = RS.cornell_moved(O, s, turn=0.15)
            if variant == "smooth_and_back" and s == 2:
                b = _smooth_short_box(b)
            flat = capi.debug_flat_attributes(b["normals"], b["colors"])[0]
            assert flat == (variant != "flat_off" and not (variant == "smooth_and_back" and s == 2))     # which kernel flavour runs, as the library decides it
            info = _move(refit, c, b)
            assert info["path"] == refit.REBUILD and c.stats().scene_in_lds == 1 - force_global
            img, tr, st = shipped(c)
            fresh = ctx(b)
            try:
                img_f, tr_f, _ = shipped(fresh)
            finally:
                fresh.close()
            what = "cornell %s step %d" % (variant, s)
            assert np.array_equal(_bits(img), _bits(img_f)), (what, int((_bits(img) != _bits(img_f)).any(-1).sum()))
            assert np.array_equal(tr.view(np.uint8), tr_f.view(np.uint8)), what
            scene = RS.oracle_scene(O, b)
            ok, rmse, outliers, allowed = fast_bar(img, O.render(scene, W, H, SPP, BOUNCES)[0], st.rays)
            print("%s: flat %d, shipped rmse %.3g, %d outlier pixels (%d allowed)" % (what, flat, rmse, outliers, allowed))
            assert ok, (what, rmse, outliers, allowed)
            if force_global:
                _strict_bars(capi, O, c, scene, rays, what, kernels=(("direct", 0, 1),))
    finally:
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- F. the edges
@pytest.mark.parametrize("gpu_build, cubes", [(0, False), (2, True)], ids=["host_tree_floor_and_sphere_far", "lbvh_whole_scene_far"])
def test_far_from_the_origin_and_back(capi, refit, O, scene_a_steps, gpu_build, cubes):
    """Scene A step 1 at (5000, -3000, 800), refitted from step 0 at the origin: sc.center jumps, and for the whole scene the padding is
    4e-6 * max|coord|.  The host builder's box leaves cannot follow there -- a cube's rounded corners miss the 1e-5 rule, the library's stated
    contract (tests/test_refit_host.py test_box_leaves_far_from_the_origin_on_the_host) -- so in its tree only the floor and the sphere go; the
    LBVH's tree has no box leaves and takes the whole scene.  Camera and rays go with the geometry.  Then back to step 0: the frame and the records
    of a single identity refit."""
    bufs, _ = scene_a_steps
    shift = np.array(RS.FAR_SHIFT, np.float32)
    far = RS.scene_a_far(1, cubes=cubes)
    scene = RS.oracle_scene(O, far)
    u = O.make_uniforms(W, H, eye=np.asarray(O.EYE, np.float32) + shift, at=np.asarray(O.AT, np.float32) + shift)
    rays = _rays(O, 51)
    rays["origin"][::1 if cubes else 2] += shift                               # (every ray, or every other one: the cubes that stayed are traced too)
    c, once = _ctx(capi, O, bufs[0], gpu_build), _ctx(capi, O, bufs[0], gpu_build)
    try:
        info = _move(refit, c, far)
        assert info["path"] == refit.DEVICE
        _assert_bounds(info, far)
        maxabs = np.abs(far["positions"]).max()
        print("far scene, builder %d: pad %.6g, 4e-6 * max|coord| = %.6g" % (gpu_build, info["pad"], float(np.float32(4e-6) * maxabs)))
        if cubes:
            assert info["pad"] == float(np.float32(4e-6) * maxabs)
        c.set_uniforms(O.uniforms_bytes(u))
        what = "far scene builder %d" % gpu_build
        _strict_bars(capi, O, c, scene, rays, what, kernels=LOCK_STEP, uniforms=u)
        _shipped_bars(capi, O, c, scene, far, rays, what, gpu_build, uniforms=u)
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(W, H)))
        home = _rays(O, 52)
        out = []
        for x in (c, once):
            _move(refit, x, bufs[0])
            x.render(0, SPP, BOUNCES)
            out.append((x.read_accum(), x.trace(home)))
        assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(out[0][1].view(np.uint8), out[1][1].view(np.uint8))
    finally:
        _close(c, refit)
        _close(once, refit)


def test_collapsed_triangles(capi, refit, O, indexed_steps):
    """Indexed scene A with one sphere vertex moved onto a neighbour: two triangles lose their area, plane_rows writes the planes no ray passes.
    The refit succeeds, the scene meets both bars, and no ray of either build names a degenerate triangle."""
    bufs, _ = indexed_steps
    b, flat = RS.scene_a_collapsed(1)
    T = b["positions"][b["indices"]].reshape(-1, 3, 3).astype(np.float64)
    area = np.linalg.norm(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]), axis=1)
    assert flat.shape[0] == 2 and (area[flat] == 0).all() and (np.delete(area, flat) > 0).all()
    scene = RS.oracle_scene(O, RS.unindexed(b))
    rays = _rays(O, 53)
    aimed = rays.copy()                                                        # a few hundred rays straight at the collapsed edge's neighbourhood
    target = T[flat].reshape(-1, 3).mean(0)
    d = target - aimed["origin"][:512].astype(np.float64) + np.random.default_rng(54).normal(scale=0.02, size=(512, 3))
    aimed["direction"][:512] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    c = _ctx(capi, O, bufs[0])
    try:
        info = _move(refit, c, b)
        assert info["path"] == refit.DEVICE
        _assert_bounds(info, b)
        _strict_bars(capi, O, c, scene, aimed, "collapsed", kernels=LOCK_STEP)
        _shipped_bars(capi, O, c, scene, b, aimed, "collapsed")
        for strict in (1, 0):
            c.set_option(capi.OPT_STRICT, strict)
            got = c.trace(aimed)["primitiveIndex"]
            assert (got >= 0).sum() > 500 and not np.isin(got, flat).any()
        c.set_option(capi.OPT_STRICT, 0)
    finally:
        _close(c, refit)
