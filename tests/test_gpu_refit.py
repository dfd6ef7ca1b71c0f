"""GPU tests (-m gpu) of the refit unit (include/trg_refit.h): a loaded scene refitted from moved vertices against the CPU oracle's render of the
moved scene -- bit for bit in the strict build, whatever tree the refit leaves (strict results are tree-independent), inside the shipped build's bar
otherwise -- and against a fresh trg_load_scene of the same geometry.  Images 32 x 24, 2 spp, 3 bounces; traces 4,096 random rays."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import refit_scenes as RS
from tests.util import fast_bar

pytestmark = pytest.mark.gpu
W, H, SPP, BOUNCES, N_RAYS = 32, 24, 2, 3, 4096
STEPS = (1, 2, 3)


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rays(O, seed, lo=(-1.1, 0.02, -1.1), hi=(1.1, 1.9, 3.0)):
    rng = np.random.default_rng(seed)
    rays = np.zeros(N_RAYS, O.RAY_DTYPE)
    rays["origin"] = rng.uniform(lo, hi, (N_RAYS, 3)).astype(np.float32)
    d = rng.normal(size=(N_RAYS, 3))
    rays["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays["mask"] = rng.choice([1, 2, 3], N_RAYS).astype(np.uint32)
    rays["maxDistance"] = np.where(rng.random(N_RAYS) < 0.25, rng.uniform(0.05, 3.0, N_RAYS), np.inf).astype(np.float32)
    rays["maxDistance"][rng.random(N_RAYS) < 0.02] = -1.0
    return rays


def _ctx(capi, O, b, gpu_build=0):
    c = capi.Context(W, H)
    c.set_option(capi.OPT_GPU_BUILD, gpu_build)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(W, H)))
    c.set_pixel_offsets(O.pixel_offsets(W, H))
    return c


def _close(c, refit):
    refit.release(c)
    c.close()


def _move(refit, c, b, normals=True):
    refit.refit_scene(c, b["positions"], b["normals"] if normals else None, b["indices"])
    return refit.refit_last(c)


# the kernels an HBM-resident scene can be rendered by: lock step, path regeneration, frame split
HBM_KERNELS = (("lock-step", 0, 1), ("regen", 1, 1), ("frame-split", 0, 2))


def _strict_bars(capi, O, c, scene, rays, what, kernels=HBM_KERNELS, uniforms=None):
    """Strict build: every kernel's frame and both kinds of trace records are the oracle's, bit for bit.  uniforms: the block the context was given
    (default: the one _ctx sets)."""
    O.set_trig_mode(O.TRIG_PORTABLE)
    try:
        ref, rst = O.render(scene, W, H, SPP, BOUNCES, uniforms=uniforms)
    finally:
        O.set_trig_mode(O.TRIG_LIBM)
    c.set_option(capi.OPT_STRICT, 1)
    try:
        for name, regen, fsplit in kernels:
            c.set_option(capi.OPT_REGEN, regen)
            c.set_option(capi.OPT_FRAME_SPLIT, fsplit)
            c.reset_stats()
            c.render(0, SPP, BOUNCES)
            assert np.array_equal(_bits(c.read_accum()), _bits(ref)), (what, name)
            assert c.stats().rays == rst.rays, (what, name)
        got = c.trace(rays)
        assert np.array_equal(got.view(np.uint8), O.intersect_nearest(scene, rays).view(np.uint8)), what
        assert np.array_equal(c.trace(rays, any_hit=True) >= 0, O.intersect_any(scene, rays) >= 0), what
    finally:
        c.set_option(capi.OPT_REGEN, -1)
        c.set_option(capi.OPT_FRAME_SPLIT, 0)
        c.set_option(capi.OPT_STRICT, 0)


def _shipped_bars(capi, O, c, scene, b, rays, what, gpu_build=0, uniforms=None, w=W, h=H):
    """Shipped build: the frame inside fast_bar against the oracle; trace records against a fresh trg_load_scene of the moved geometry within
    DESIGN section 2's figures (distance 3e-6, weights 2e-5) wherever the two name the same primitive -- and they may name another one only where
    double precision cannot decide (margin below 1e-5, the rule of tests/test_gpu_parity.py test_intersector).  w, h: the context's size."""
    ref, _ = O.render(scene, w, h, SPP, BOUNCES, uniforms=uniforms)
    c.set_option(capi.OPT_STRICT, 0)
    c.reset_stats()
    c.render(0, SPP, BOUNCES)
    ok, rmse, outliers, allowed = fast_bar(c.read_accum(), ref, c.stats().rays)
    print("%s: shipped rmse %.3g, %d outlier pixels (%d allowed)" % (what, rmse, outliers, allowed))
    assert ok, (what, rmse, outliers, allowed)
    got = c.trace(rays)
    fresh = _ctx(capi, O, b, gpu_build)
    try:
        want = fresh.trace(rays)
    finally:
        fresh.close()
    diff = got["primitiveIndex"] != want["primitiveIndex"]
    if diff.any():
        _, _, margin = O.nearest_f64(scene, rays)
        assert not (diff & ~(margin < 1e-5)).any(), (what, int(diff.sum()))
    same = ~diff & (want["primitiveIndex"] >= 0)
    dd = float(np.abs(got["distance"][same] - want["distance"][same]).max()) if same.any() else 0.0
    dw = float(np.abs(got["coordinates"][same] - want["coordinates"][same]).max()) if same.any() else 0.0
    print("%s: %d of %d rays name another primitive; distances differ by at most %.3g, weights by %.3g" % (what, int(diff.sum()), N_RAYS, dd, dw))
    np.testing.assert_allclose(got["distance"][same], want["distance"][same], rtol=3e-6, atol=3e-6)
    np.testing.assert_allclose(got["coordinates"][same], want["coordinates"][same], rtol=0, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------------- device path
@pytest.fixture(scope="module")
def scene_a_steps(O):
    """Scene A's buffers and the oracle's scene at steps 0..3, shared and left unchanged."""
    bufs = [RS.scene_a(s) for s in range(4)]
    return bufs, [RS.oracle_scene(O, b) for b in bufs]


def test_scene_a_device_path_strict_and_shipped(capi, refit, O, scene_a_steps):
    bufs, scenes = scene_a_steps
    rays = _rays(O, 31)
    c = _ctx(capi, O, bufs[0])
    try:
        assert c.stats().scene_in_lds == 0
        for s in STEPS:
            info = _move(refit, c, bufs[s])
            assert info["path"] == refit.DEVICE and info["n_records"] == 706 and info["n_quads"] == 1 + 6 * RS.N_CUBES
            assert info["n_boxes"] == RS.N_CUBES + 1 and info["n_nodes_box"] > 0      # 32 parallelepipeds and the floor, a lone quad dressed as a box
            assert np.array_equal(np.array(info["lo"], np.float32), bufs[s]["positions"].min(0)) and np.array_equal(np.array(info["hi"], np.float32), bufs[s]["positions"].max(0))
            print("scene A step %d: %.3f ms, %d passes, area ratio %.4f (box flavour %.4f), pad %.3g" % (s, info["ms"], info["passes"], info["area_ratio"], info["area_ratio_box"], info["pad"]))
            assert info["area_ratio"] > 0.5 and info["area_ratio_box"] > 0.5
            _strict_bars(capi, O, c, scenes[s], rays, "scene A step %d" % s)
            _shipped_bars(capi, O, c, scenes[s], bufs[s], rays, "scene A step %d" % s)
    finally:
        _close(c, refit)


@pytest.mark.parametrize("gpu_build", [1, 2, 3])
def test_scene_b_device_built_trees(capi, refit, O, gpu_build):
    """The Cornell box built on the device (binned SAH, LBVH, PLOC: never LDS-staged), its short box sliding 0.02 per step."""
    rays = _rays(O, 32 + gpu_build, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0))
    c = _ctx(capi, O, RS.cornell_moved(O, 0), gpu_build)
    try:
        assert c.stats().scene_in_lds == 0
        for s in STEPS:
            b = RS.cornell_moved(O, s)
            scene = RS.oracle_scene(O, b)
            info = _move(refit, c, b)
            assert info["path"] == refit.DEVICE and info["n_records"] == 36 and info["n_boxes"] == 0 and info["n_nodes_box"] == 0
            print("scene B builder %d step %d: %.3f ms, %d quads, area ratio %.4f" % (gpu_build, s, info["ms"], info["n_quads"], info["area_ratio"]))
            _strict_bars(capi, O, c, scene, rays, "scene B builder %d step %d" % (gpu_build, s))
            _shipped_bars(capi, O, c, scene, b, rays, "scene B builder %d step %d" % (gpu_build, s), gpu_build)
    finally:
        _close(c, refit)


def test_there_and_back_is_a_function_of_the_positions(capi, refit, O, scene_a_steps):
    """Refit to P1, then back to P0: the shipped frame and the trace records are those of a single refit to P0 -- no drift."""
    bufs, _ = scene_a_steps
    rays = _rays(O, 33)
    out = []
    for path in ((1, 0), (0,), (3, 2, 1, 0)):
        c = _ctx(capi, O, bufs[0])
        try:
            for s in path:
                _move(refit, c, bufs[s])
            c.render(0, SPP, BOUNCES)
            out.append((c.read_accum(), c.trace(rays)))
        finally:
            _close(c, refit)
    for img, tr in out[1:]:
        assert np.array_equal(_bits(img), _bits(out[0][0])) and np.array_equal(tr.view(np.uint8), out[0][1].view(np.uint8))
    # reported, not asserted: whether the identity refit also gives the never-refitted scene's frame
    c = _ctx(capi, O, bufs[0])
    try:
        c.render(0, SPP, BOUNCES)
        print("identity refit against the scene as loaded: frames %s" % ("equal" if np.array_equal(_bits(c.read_accum()), _bits(out[1][0])) else "differ"))
    finally:
        c.close()


def test_refusals_leave_the_scene_as_it_was(capi, refit, O, scene_a_steps):
    bufs, _ = scene_a_steps
    rays = _rays(O, 34)
    b = bufs[1]
    c = _ctx(capi, O, bufs[0])
    try:
        _move(refit, c, b)
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
        cases = []
        k0 = RS.cube_first_triangle(9)
        pos = b["positions"].copy()                                          # one cube corner moved by 1e-3 of its edge
        corner = pos[3 * k0].copy()
        pos[(pos == corner).all(1)] += np.float32(1e-3 * np.linalg.norm(pos[3 * k0 + 1] - pos[3 * k0]))
        touched = {int(i) // 3 for i in np.flatnonzero((b["positions"] != pos).any(1))}
        cases.append(("corner", pos, None, -34,{t - t % 2 + d for t in touched for d in (0, 1)}))
        pos = b["positions"].copy()                                          # the floor quad bent: its fourth corner leaves the plane
        pos[5, 1] += np.float32(0.01)
        cases.append(("bent quad", pos, None, -34, {0}))
        pos = b["positions"].copy()                                          # a NaN vertex, in the sphere
        t_nan = RS.FLOOR_TRIS + RS.CUBE_TRIS + 77
        pos[3 * t_nan + 1, 2] = np.nan
        cases.append(("nan", pos, None, -22, {t_nan}))
        cases.append(("n_tris", b["positions"], 705, -22, None))
        for name, pos, n_tris, code, offenders in cases:
            with pytest.raises(capi.TrgError) as e:
                refit.refit_scene(c, pos, b["normals"], b["indices"], n_tris=n_tris)
            msg = str(e.value)
            print("%s: %s" % (name, msg))
            assert e.value.code == code, (name, msg)
            if offenders is not None:
                named = int(re.search(r"triangle (\d+)", msg).group(1))
                assert named in offenders, (name, named, sorted(offenders))
            else:
                assert "705" in msg and "706" in msg
            after = state()
            assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8)), name
            assert refit.refit_last(c) == good                                   # the last SUCCESSFUL refit
        # an index out of range is refused like the rest, and a good call still works afterwards
        idx = b["indices"].copy()
        idx[3 * 400] = idx.shape[0]
        with pytest.raises(capi.TrgError) as e:
            refit.refit_scene(c, b["positions"], None, idx)
        assert e.value.code == -22 and "triangle 400" in str(e.value)
        _move(refit, c, bufs[2], normals=False)
    finally:
        _close(c, refit)


def _textures(n_tris, first, count, seed):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 1, (3 * n_tris, 2)).astype(np.float32)
    ids = np.zeros(n_tris, np.uint32)
    ids[first:first + count] = 1 + (np.arange(count) % 2)
    images = [rng.integers(0, 256, (8, 8, 4), dtype=np.uint8), rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)]
    return uv, ids, images


def test_textures_survive_a_device_refit(capi, refit, O, scene_a_steps):
    bufs, _ = scene_a_steps
    tex = _textures(706, RS.FLOOR_TRIS + RS.CUBE_TRIS, RS.SPHERE_TRIS, 5)
    c = _ctx(capi, O, bufs[0])
    try:
        c.load_textures(*tex)
        info = _move(refit, c, bufs[2])
        assert info["path"] == refit.DEVICE
        _strict_bars(capi, O, c, RS.oracle_scene(O, bufs[2], tex), _rays(O, 35), "textured scene A", kernels=HBM_KERNELS[:1])
    finally:
        _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- small-scene path
def test_small_scene_is_rebuilt_and_keeps_its_textures(capi, refit, O):
    """The Cornell box, host-built and LDS-resident, its short box sliding and turning: the rebuild path, strict bit-exact in the LDS kernel and with
    TRG_OPT_FORCE_GLOBAL; then the same with textures on the short box and the floor."""
    rays = _rays(O, 36, lo=(-0.95, 0.05, -0.95), hi=(0.95, 1.9, 3.0))
    for tex in (None, _textures(36, 0, 14, 6)):
        c = _ctx(capi, O, RS.cornell_moved(O, 0, turn=0.15))
        try:
            assert c.stats().scene_in_lds == 1
            if tex:
                c.load_textures(*tex)
            for s in (1, 2):
                b = RS.cornell_moved(O, s, turn=0.15)
                info = _move(refit, c, b, normals=(s == 1))                  # (step 2 keeps the loaded normals: the turn is small, the oracle gets the same)
                assert info["path"] == refit.REBUILD and info["path_name"] == "rebuild"
                if s == 2:
                    b = dict(b, normals=RS.cornell_moved(O, 1, turn=0.15)["normals"])
                scene = RS.oracle_scene(O, b, tex)
                for force_global in (0, 1):
                    c.set_option(capi.OPT_FORCE_GLOBAL, force_global)
                    assert c.stats().scene_in_lds == 1 - force_global
                    _strict_bars(capi, O, c, scene, rays, "cornell step %d global %d" % (s, force_global), kernels=(("direct", 0, 1),))
                    if force_global == 0:                                    # the shipped LDS kernels test the room ahead of the tree: the strict build does not know it
                        assert c.stats().bvh_room == 5
                        _shipped_bars(capi, O, c, scene, b, rays, "cornell step %d" % s)
                c.set_option(capi.OPT_FORCE_GLOBAL, 0)
            with pytest.raises(capi.TrgError) as e:                          # the small path refuses what it cannot build from, by name
                bad = RS.cornell_moved(O, 3)
                bad["positions"][3 * 20 + 2, 0] = np.inf
                refit.refit_scene(c, bad["positions"], None, bad["indices"])
            assert e.value.code == -22 and "triangle 20" in str(e.value)
        finally:
            _close(c, refit)


# ---------------------------------------------------------------------------------------------------------------------------- group, plugin
def test_group_refit_matches_the_single_context(capi, refit, O, scene_a_steps, monkeypatch):
    """Two contexts on one device, each rendering its band of the refitted scene, gathered: the single context's frame."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    bufs, _ = scene_a_steps
    b0, b1 = bufs[0], bufs[2]
    u = O.uniforms_bytes(O.make_uniforms(W, H))
    c = capi.Context(W, H)
    g = capi.Group([0, 0], W, H)
    try:
        for x in (c, g):
            x.load_scene(b0["positions"], b0["normals"], b0["colors"], b0["indices"], b0["material_ids"])
            x.set_uniforms(u)
            x.set_pixel_offsets_seed()
            refit.refit_scene(x, b1["positions"], b1["normals"], b1["indices"])
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.DEVICE
        c.render(0, SPP, BOUNCES)
        g.render(0, SPP, BOUNCES)
        g.sync()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(c.read_accum()))
        with pytest.raises(capi.TrgError) as e:
            refit.refit_scene(g, b1["positions"], b1["normals"], b1["indices"], n_tris=12)
        assert e.value.code == -22 and "706" in str(e.value)
    finally:
        refit.release(g)
        g.close()
        _close(c, refit)


def test_plugin_refit_option(capi, refit, tmp_path):
    """toyraygun_cornell 64 48 4 3 out.png slide=0.02 refit: HipRenderer::setRefit(true), every updateScene served by trg_refit_scene -- the picture of
    the same calls through the C ABI.  The Cornell box is rebuilt by the host builder (the small-scene path), so it is also, bit for bit, the picture
    without `refit`."""
    from toyraygun_amd import host
    from tests.test_gpu_motion import _load, _slid_cornell
    app = os.path.join(capi.LIB_DIR, "toyraygun_cornell")
    w, h, frames, bounces, slide = 64, 48, 4, 3, 0.02

    def run(name, *extra):
        path = str(tmp_path / name)
        r = subprocess.run([app, str(w), str(h), str(frames), str(bounces), path] + list(extra), check=True, capture_output=True, text=True, timeout=120)
        return host.Texture(path=path).rgba(), r.stdout
    (pic, out), (plain, out_plain) = run("refit.png", "slide=0.02", "refit"), run("plain.png", "slide=0.02")
    assert "%d scene updates served by a refit" % (frames - 1) in out and "refit refused" not in out and "served by a refit" not in out_plain
    assert np.array_equal(pic, plain)
    assert subprocess.run([app, str(w), str(h), "2", "3", str(tmp_path / "bad.png"), "slide=0.02", "refit=1"], capture_output=True, timeout=120).returncode != 0
    scenes = [_slid_cornell(host, float(np.float32(k * slide))) for k in range(frames)]
    c = capi.Context(w, h)
    try:
        _load(c, scenes[0])
        c.set_uniforms(host.uniforms(w, h)[0])
        c.set_pixel_offsets_seed()
        for k in range(frames):
            if k:
                refit.refit_scene(c, scenes[k]["positions"], scenes[k]["normals"], scenes[k]["indices"])
                assert refit.refit_last(c)["path"] == refit.REBUILD
            c.render(k, 1, bounces)
        c.sync()
        assert np.array_equal(c.postprocess(flip_y=True), pic)
    finally:
        _close(c, refit)


def test_plugin_update_scene_refits_or_falls_back(capi, refit, capfd):
    """HipRenderer::updateScene with setRefit(true) on a scene traversed from HBM (the Cornell box and 40 cubes added as meshes): a moved scene is
    refitted (one update served, the frame inside the shipped build's bar of a loadScene of the moved scene); a scene in which one cube lost a corner
    is REFUSED by the library, loaded instead -- the frame of loadScene, bit for bit -- and the renderer says so; with setRefit(false) nothing is refitted."""
    from toyraygun_amd import host
    unit = host.Scene()
    unit.add("cube", (1.0, 1.0, 1.0), np.eye(4, dtype=np.float32))
    ub = unit.buffers()
    verts, normals, idx = ub["positions"].reshape(-1, 3), ub["normals"].reshape(-1, 3), np.arange(36, dtype=np.uint32)

    def scene(step, bend=False):
        s = host.Scene.cornell_box()
        rng = np.random.default_rng(77)
        for i in range(40):
            v = verts.copy()
            if bend and i == 7:
                v[(v == v[0]).all(1)] += np.float32(1e-2)
            scale, rot, pos = rng.uniform(0.05, 0.09, 3), rng.uniform(0, 3, 3), np.array([-0.8 + 0.2 * (i % 8), 1.0 + 0.15 * (i // 8), -0.6 + 0.1 * (i % 5)])
            s.add_mesh(v, normals, idx, host.mtx_srt(scale, rot + step * rng.uniform(-0.3, 0.3, 3), pos + step * rng.uniform(-0.03, 0.03, 3)), rng.uniform(0.2, 0.9, 3), 1)
        return s
    w, h, frames = 48, 32, 2
    a, ok, bad = scene(0), scene(1), scene(1, bend=True)
    assert a.buffers()["material_ids"].shape[0] == 36 + 480
    ref_ok, ref_bad = host.render_scene(ok, w, h, frames)[0], host.render_scene(bad, w, h, frames)[0]
    capfd.readouterr()
    img, n = host.update_scene(a, ok, w, h, frames, refit=True)
    passes, rmse, outliers, allowed = fast_bar(img, ref_ok, w * h * frames * 7)
    print("plugin refit against loadScene of the moved scene: rmse %.3g, %d outlier pixels (%d allowed)" % (rmse, outliers, allowed))
    assert n == 1 and passes and "refit refused" not in capfd.readouterr().out
    img, n = host.update_scene(a, bad, w, h, frames, refit=True)
    said = capfd.readouterr().out
    assert n == 0 and np.array_equal(_bits(img), _bits(ref_bad))
    assert "refit refused" in said and "loading the scene" in said and "no longer a parallelogram" in said
    img, n = host.update_scene(a, ok, w, h, frames, refit=False)
    assert n == 0 and np.array_equal(_bits(img), _bits(ref_ok))
