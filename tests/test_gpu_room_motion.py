"""A ROOM under moving geometry on the GPU (-m gpu): what a rebuild (trg_refit.hip refit_rebuild) must carry over into the shipped LDS kernels --
SceneDesc::room_first1 and the face words, bvh_room, bvh_walk_depth, the room's frame that decides per launch whether shadow rays skip the room --
when the WALLS move, through trg_refit_scene and through the pose, skin, morph and rig units.  Steps, drivers and the float64 model:
tests/room_motion_scenes.py; the rooms and ray caps of the steps on the CPU: tests/test_room_motion_host.py.

Every moved state has two references: a FRESH context that loaded the moved geometry (the rebuild feeds the same builder the same buffers: bit
for bit), and the CPU oracle / the float64 room model.  Images 64 x 48 and 33 x 17, 3 spp, 5 bounces; traces of about 20,000 seeded rays per
step.  The bars are the project's own: bit identity, tests/util.py fast_bar, ray totals within 1e-4, trace distances within 3e-6 + 3e-6 |t|,
two exclusion classes under 1 % each.  Nothing here provokes a fault: every refusal is decided on the host.

Measured on an MI355X (profiles/r05/room_motion_test.txt): see the figures there."""
import numpy as np
import pytest

from tests import refit_scenes as RS
from tests import rig_scenes as GS
from tests import room_motion_scenes as M
from tests import room_scenes as R
from tests.test_gpu_room import PAIRS
from tests.test_gpu_room_inside import SCHEDULES, SWITCH
from tests.util import fast_bar, uniforms_case

pytestmark = pytest.mark.gpu
SHAPES = ((64, 48), (33, 17))
SPP, BNC = 3, 5
ONE_SCHEDULE = {"megakernel": SCHEDULES["megakernel"]}


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
def steps(O):
    """The steps of both scenes, shared and left unchanged."""
    return {scene: M.SCENES[scene][0](O) for scene in M.SCENES}


@pytest.fixture(scope="module")
def step_rays(O, steps):
    """(scene, step) -> rays_of: made once."""
    return {(scene, name): M.rays_of(O, st, steps[scene]["rest"]) for scene in steps for name, st in steps[scene].items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counts(st):
    return (int(st.primary_rays), int(st.bounce_rays), int(st.shadow_rays), int(st.shaded_hits))


def _switch(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, value)


def _ctx(capi, O, b, w, h, seed_offsets=False):
    c = capi.Context(w, h)
    try:
        c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
        if seed_offsets:
            c.set_pixel_offsets_seed()
        else:
            c.set_pixel_offsets(O.pixel_offsets(w, h))
        c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
        c.set_option(capi.OPT_COUNTERS, 1)
    except Exception:
        c.close()
        raise
    return c


def _close(c, refit):
    refit.release(c)
    c.close()


def _mixed_masks(rays):
    out = rays.copy()
    out["mask"] = 1 + np.arange(len(out)) % 3
    return out


def _schedule(capi, c, opts):
    for k, v in opts.items():
        c.set_option(getattr(capi, "OPT_" + k), v)


def _observe(capi, c, rays, schedules=SCHEDULES, force_global=(0, 1)):
    """Everything two contexts that hold the same scene must agree on, as a dict of comparable values: bvh_room and scene_in_lds, and with
    TRG_OPT_FORCE_GLOBAL 0 and 1 the accumulation buffer's bytes, the ray counters, node_fetches and tri_tests under every schedule, and the
    records of trg_trace, nearest and any-hit."""
    out = {"bvh_room": int(c.stats().bvh_room)}
    try:
        for fg in force_global:
            c.set_option(capi.OPT_FORCE_GLOBAL, fg)
            out[("scene_in_lds", fg)] = int(c.stats().scene_in_lds)
            for name, opts in schedules.items():
                _schedule(capi, c, opts)
                c.reset_stats()
                c.render(0, SPP, BNC)
                st = c.stats()
                out[("frame", fg, name)] = c.read_accum().tobytes()
                out[("counters", fg, name)] = _counts(st) + (int(st.node_fetches), int(st.tri_tests))
            out[("trace", fg)] = c.trace(rays).tobytes()
            out[("any", fg)] = c.trace(rays, any_hit=True).tobytes()
    finally:
        c.set_option(capi.OPT_FORCE_GLOBAL, 0)
        _schedule(capi, c, SCHEDULES["megakernel"])
    return out


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, (what, differ, [(got[k], want[k]) for k in differ if not isinstance(want[k], bytes)])


def _as_loaded(capi, O, c, b, w, h, rays, what, n_faces, **kw):
    """The context `c` against a fresh one that loaded `b`; returns what was observed."""
    got = _observe(capi, c, rays, **kw)
    fresh = _ctx(capi, O, b, w, h)
    try:
        want = _observe(capi, fresh, rays, **kw)
    finally:
        fresh.close()
    assert want["bvh_room"] == n_faces and want[("scene_in_lds", 0)] == 1, (what, want["bvh_room"])
    if 1 in kw.get("force_global", (0, 1)):
        assert want[("scene_in_lds", 1)] == 0
    _assert_same(got, want, what)
    return got


def _move(refit, c, b, normals=True):
    refit.refit_scene(c, b["positions"], b["normals"] if normals else None, b["indices"])
    info = refit.refit_last(c)
    assert info["path"] == refit.REBUILD, info["path_name"]


def _faces(scene, step):
    return 0 if step.room is None else M.SCENES[scene][2]


# ------------------------------------------------------------------------------------------------------------------- 1. moved equals loaded
@pytest.mark.parametrize("shape", SHAPES, ids=["64x48", "33x17"])
@pytest.mark.parametrize("scene", list(M.SCENES))
def test_moved_equals_loaded(capi, refit, O, steps, step_rays, scene, shape):
    """Every step in order on ONE context through trg_refit_scene, first without a normals table (the normals the blob holds stay: the fresh
    context loads the step's corners with the previous step's normals), then with the moved normals: the shipped build, three schedules, the LDS
    kernels and TRG_OPT_FORCE_GLOBAL (there the tree walked is the one built without the room from the moved geometry), counters and traces."""
    w, h = shape
    seq = steps[scene]
    c = _ctx(capi, O, seq["rest"].buffers, w, h)
    try:
        held = seq["rest"].buffers["normals"]
        for name, step in seq.items():
            rays = _mixed_masks(step_rays[(scene, name)][0])
            for normals in (False, True):
                _move(refit, c, step.buffers, normals)
                b = step.buffers if normals else dict(step.buffers, normals=held)
                got = _as_loaded(capi, O, c, b, w, h, rays, (scene, name, "normals given" if normals else "normals kept"), _faces(scene, step))
            held = step.buffers["normals"]
            n = got[("counters", 0, "megakernel")]
            print("room motion refit %-7s %-16s %dx%d: bvh_room %d, rays %d, node steps %d (LDS) / %d (global), primitive tests %d / %d"
                  % (scene, name, w, h, got["bvh_room"], sum(n[:3]), n[4], got[("counters", 1, "megakernel")][4], n[5], got[("counters", 1, "megakernel")][5]))
    finally:
        _close(c, refit)


# ----------------------------------------------------------------------------------------------------------------- 2. moved against the oracle
@pytest.mark.parametrize("shape", SHAPES, ids=["64x48", "33x17"])
def test_moved_against_the_oracle(capi, refit, O, steps, shape):
    """After each step the shipped frame meets fast_bar against the libm oracle's render of the step's buffers with ray totals within 1e-4, and
    the strict frame is the portable oracle's bit for bit, under the cameras and lights of tests/test_gpu_room.py PAIRS."""
    w, h = shape
    off = O.pixel_offsets(w, h)
    failed = []
    c = _ctx(capi, O, steps["cornell"]["rest"].buffers, w, h)
    try:
        c.set_option(capi.OPT_COUNTERS, 0)
        for name, step in steps["cornell"].items():
            _move(refit, c, step.buffers)
            assert c.stats().bvh_room == _faces("cornell", step) and c.stats().scene_in_lds == 1
            scene = RS.oracle_scene(O, step.buffers)
            for cam, light in PAIRS:
                u = uniforms_case(O, w, h, cam, light)
                c.set_uniforms(O.uniforms_bytes(u))
                ref, rst = O.render(scene, w, h, SPP, BNC, offsets=off, uniforms=u)
                c.reset_stats()
                c.render(0, SPP, BNC)
                img, st = c.read_accum(), c.stats()
                ok, rmse, outliers, allowed = fast_bar(img, ref, rst.rays)
                rays_ok = abs(st.rays - rst.rays) <= 1e-4 * max(rst.rays, 1)
                print("room motion oracle %-16s %dx%d %-12s x %-15s rmse %.3e  outliers %d (allowed %d)  rays %d / %d%s"
                      % (name, w, h, cam, light, rmse, outliers, allowed, st.rays, rst.rays, "" if ok and rays_ok else "   <-- FAILS"))
                assert np.isfinite(img).all()
                if not (ok and rays_ok):
                    failed.append((name, cam, light, rmse, outliers, allowed, st.rays, rst.rays))
                O.set_trig_mode(O.TRIG_PORTABLE)
                try:
                    ref, rst = O.render(scene, w, h, SPP, BNC, offsets=off, uniforms=u)
                finally:
                    O.set_trig_mode(O.TRIG_LIBM)
                c.set_option(capi.OPT_STRICT, 1)
                try:
                    c.reset_stats()
                    c.render(0, SPP, BNC)
                    assert np.array_equal(_bits(c.read_accum()), _bits(ref)) and _counts(c.stats()) == _counts(rst), (name, cam, light, "strict")
                finally:
                    c.set_option(capi.OPT_STRICT, 0)
    finally:
        _close(c, refit)
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------ 3. trace against float64, moved frame
@pytest.mark.parametrize("scene", list(M.SCENES))
def test_trace_against_float64_in_the_moved_frame(capi, refit, O, steps, step_rays, monkeypatch, scene):
    """trg_trace of the refitted context, nearest and any-hit, masks 1 / 2 / 3, against room_motion_scenes.scene_f64 (the room by the open-box
    rule in the step's frame; where the step has no room its walls one by one).  Where the model names a wall the device must name that wall
    (the pair of triangles) at the model's distance to 3e-6 + 3e-6 |t|; where it names something else or nothing the device must name no wall;
    any-hit is the model's.  Left out: the two classes of room_motion_scenes.excluded, each under 1 % (tests/test_room_motion_host.py shows
    that on the model alone).

    The float64 model is a model of the WALLS: what a ray meets before a wall (a box's face, the light's quad) is in it only so that it knows
    when a wall is not the nearest thing.  Those hits are held to the build with the room switched off (TRG_BVH_ROOM=0, a fresh load of the
    step's buffers: the tree without the room), as tests/test_gpu_room.py holds every hit: the same primitive, the distance to 3e-6 + 3e-6 |t|."""
    _, first_tri, n_faces, broken_tri = M.SCENES[scene]
    seq = steps[scene]
    rest = seq["rest"]
    bad = []
    c = _ctx(capi, O, rest.buffers, 64, 48)
    try:
        for name, step in seq.items():
            _move(refit, c, step.buffers)
            assert c.stats().bvh_room == _faces(scene, step)
            rays, o, d, tmax, kind = step_rays[(scene, name)]
            rays = rays.copy()
            edge, tied = M.excluded(step, rest, first_tri, n_faces, o, d, tmax)
            assert edge.mean() < 0.01 and tied.mean() < 0.01, (name, edge.mean(), tied.mean())
            keep = ~(edge | tied)
            monkeypatch.setenv("TRG_BVH_ROOM", "0")
            try:
                off = _ctx(capi, O, step.buffers, 64, 48)
            finally:
                monkeypatch.delenv("TRG_BVH_ROOM")
            try:
                assert off.stats().bvh_room == 0 and off.stats().scene_in_lds == 1
                for mask in (1, 2, 3):
                    quad, t, is_wall, _ = M.scene_f64(step, rest, first_tri, n_faces, broken_tri, o, d, tmax, mask)
                    rays["mask"] = mask
                    got, got_any, ref = c.trace(rays), c.trace(rays, any_hit=True) >= 0, off.trace(rays)
                    prim = got["primitiveIndex"].astype(np.int64)
                    got_wall = (prim >= first_tri) & (prim < first_tri + 2 * n_faces)
                    hit = quad >= 0
                    ahead = hit & ~is_wall                                                                # something else is met before any wall
                    wrong = keep & ((hit != (prim >= 0)) | (is_wall != got_wall) | (is_wall & (prim // 2 != quad)) | (ahead & (prim != ref["primitiveIndex"])))
                    want = np.where(is_wall, t, ref["distance"].astype(np.float64))
                    with np.errstate(invalid="ignore"):
                        err = np.abs(got["distance"].astype(np.float64) - want) - 3e-6 * np.abs(want)
                    held = keep & hit & (prim >= 0) & ~wrong
                    far = held & (err > 3e-6)
                    any_wrong = keep & (got_any != hit)
                    print("room motion trace %-7s %-16s mask %d: %d rays, left out %.4f at edges and %.4f tied, hit share %.3f (walls %.3f); primitive wrong on %d (kinds %s), "
                          "distance beyond the bar on %d (worst: walls %.3e, ahead of a wall %.3e), any-hit wrong on %d"
                          % (scene, name, mask, len(o), edge.mean(), tied.mean(), hit.mean(), is_wall.mean(), int(wrong.sum()), [R.RAY_KINDS[k] for k in np.unique(kind[wrong])],
                             int(far.sum()), float(err[held & is_wall].max()) if (held & is_wall).any() else 0.0, float(err[held & ahead].max()) if (held & ahead).any() else 0.0,
                             int(any_wrong.sum())))
                    for i in np.flatnonzero(wrong | far | any_wrong)[:8]:                                 # the rays themselves, for whoever reads a failure
                        print("room motion trace     ray %d (%s): origin %s direction %s maxDistance %g; device primitive %d at %.9g (any-hit %d), room off primitive %d at %.9g, "
                              "float64 quad %d at %.9g (a wall: %d)" % (i, R.RAY_KINDS[kind[i]], o[i].tolist(), d[i].tolist(), tmax[i], prim[i], got["distance"][i], got_any[i],
                                                                       ref["primitiveIndex"][i], ref["distance"][i], quad[i], t[i], is_wall[i]))
                    if mask != 2:
                        assert is_wall.mean() > 0.3
                    if wrong.any() or far.any() or any_wrong.any():
                        bad.append((name, mask, int(wrong.sum()), int(far.sum()), int(any_wrong.sum())))
            finally:
                off.close()
    finally:
        _close(c, refit)
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------- 4. the inside rule follows the room
def _on_and_off(c, monkeypatch):
    """(frame bytes, ray counters, node steps) with TRG_ROOM_INSIDE unset and with 0."""
    out = []
    for value in (None, "0"):
        _switch(monkeypatch, value)
        c.reset_stats()
        c.render(0, SPP, BNC)
        st = c.stats()
        out.append((c.read_accum().tobytes(), _counts(st), int(st.node_fetches)))
    _switch(monkeypatch, None)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["64x48", "33x17"])
def test_the_inside_rule_follows_the_room(capi, refit, O, steps, monkeypatch, shape):
    """For every step and both light placements (the default block's light, which stands, and the light carried by the walls' map) the expected
    flag comes from trg_debug_room of the step's buffers and trg_debug_room_light_inside, both on the CPU.  Where it is 0 the node steps with the
    switch unset and with 0 are equal; where it is 1 the switch costs node steps, at most one per shadow ray; bits and ray counters are equal
    either way.  rigid / default light: 0 (a frame left over from the load would say 1).  mended: what rest gave."""
    w, h = shape
    seen = {}
    c = _ctx(capi, O, steps["cornell"]["rest"].buffers, w, h)
    try:
        for name, step in steps["cornell"].items():
            _move(refit, c, step.buffers)
            b = step.buffers
            r = capi.debug_room(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
            for carried in (False, True):
                u = M.uniforms(O, w, h, step, carried=carried)
                want = bool(r["n_faces"]) and capi.debug_room_light_inside(r["center"], r["axis"], O.uniforms_bytes(u))
                assert want == M.light_inside_f64(r, u)
                c.set_uniforms(O.uniforms_bytes(u))
                (on, on_counts, on_nodes), (off, off_counts, off_nodes) = seen[(name, carried)] = _on_and_off(c, monkeypatch)
                print("room motion inside %-16s %dx%d light %-7s: flag %d, node steps %d off / %d on, shadow rays %d"
                      % (name, w, h, "carried" if carried else "default", want, off_nodes, on_nodes, on_counts[2]))
                assert on == off and on_counts == off_counts and on_counts[2] > 0, (name, carried)
                if want:
                    assert 0 < off_nodes - on_nodes <= on_counts[2], (name, carried, off_nodes, on_nodes)
                else:
                    assert off_nodes == on_nodes, (name, carried, off_nodes, on_nodes)
        flags = {k: v[1][2] > v[0][2] for k, v in seen.items()}
        assert not flags[("rigid", False)] and flags[("rigid", True)]
        assert flags[("low_ceiling_in", False)] and not flags[("low_ceiling_out", False)]
        assert not flags[("broken", False)] and not flags[("broken", True)]
        assert seen[("mended", False)] == seen[("rest", False)] and seen[("mended", True)] == seen[("rest", True)]
    finally:
        _close(c, refit)


# ------------------------------------------------------------------------------------------------------------------- 5. a room that is born
@pytest.mark.parametrize("shape", SHAPES, ids=["64x48", "33x17"])
@pytest.mark.parametrize("scene", list(M.SCENES))
def test_a_room_that_is_born(capi, refit, O, steps, step_rays, monkeypatch, scene, shape):
    """A scene LOADED without a room (the step `broken`) and refitted to `rigid`: the room, its frame and the depth the launch plans with come
    from the rebuild alone.  Everything of test 1 against a fresh load of `rigid`, and the inside rule's flag with the carried light."""
    w, h = shape
    seq = steps[scene]
    rays = _mixed_masks(step_rays[(scene, "rigid")][0])
    c = _ctx(capi, O, seq["broken"].buffers, w, h)
    try:
        assert c.stats().bvh_room == 0 and c.stats().scene_in_lds == 1
        _move(refit, c, seq["rigid"].buffers)
        _as_loaded(capi, O, c, seq["rigid"].buffers, w, h, rays, (scene, "born"), M.SCENES[scene][2])
        c.set_uniforms(O.uniforms_bytes(M.uniforms(O, w, h, seq["rigid"], carried=True)))
        (on, on_counts, on_nodes), (off, off_counts, off_nodes) = _on_and_off(c, monkeypatch)
        assert on == off and on_counts == off_counts and 0 < off_nodes - on_nodes <= on_counts[2]
    finally:
        _close(c, refit)


# ------------------------------------------------------------------------------------------------------- 6. every unit reaches the same state
def _unit_applies(O, unit, units, c, b, steps):
    """The applies of one unit's driver: yields (what, read-back buffers, faces expected or None = whatever a fresh load says)."""
    pose, skin, morph, rig = units
    if unit == "pose":
        pose.bind(c, b["positions"], b["normals"], b["indices"], M.OBJECT_FIRST)
        for name in ("rigid", "sheared", "box_through_wall", "rest"):
            pose.apply(c, M.POSES[name])
            yield name, pose.read(c), 5
    elif unit in ("skin", "skin_blended"):
        ids, w, nb = M.skin_binding(b, unit == "skin_blended")
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, w, nb)
        for name in ("sheared", "rigid", "rest"):                                # bones that differ, then equal bones: the next apply mends the room
            skin.apply(c, M.BONES[name])
            yield name, skin.read(c), 0 if (unit == "skin_blended" and name == "sheared") else 5
    elif unit == "morph":
        morph.bind(c, b["positions"], b["normals"], b["indices"], *M.morph_target(b), None)
        for wt, faces in ((0.0, 5), (1.0, 0), (0.5, None), (0.0, 5)):
            morph.apply(c, np.array([wt], np.float32))
            yield "weight %g" % wt, morph.read(c), faces
    elif unit == "rig":
        ids, w, nb = M.skin_binding(b)
        rig.bind(c, *GS.args(M.wall_rig()))
        skin.bind(c, b["positions"], b["normals"], b["indices"], ids, w, nb)
        for name, clock in M.RIG_CLOCKS.items():
            rig.skin_apply(c, [clock])
            yield name, skin.read(c), 5
    else:
        import torch
        for name in ("rigid", "broken", "rest"):
            m = steps[name].buffers
            t = [torch.from_numpy(m["positions"]).cuda(), torch.from_numpy(m["normals"]).cuda(), torch.from_numpy(m["indices"].view(np.int32)).cuda()]
            torch.cuda.synchronize()
            pose.refit_scene_device(c, *t)
            yield name, (m["positions"], m["normals"]), 0 if name == "broken" else 5


@pytest.mark.parametrize("shape", SHAPES, ids=["64x48", "33x17"])
@pytest.mark.parametrize("unit", ["pose", "skin", "skin_blended", "morph", "rig", "device_tensors"])
def test_every_unit_reaches_the_same_state(capi, refit, O, steps, step_rays, unit, shape):
    """The drivers of tests/room_motion_scenes.py and trg_refit_scene_device from torch tensors: after every apply the geometry is read back and
    the context compared with a fresh load of it (one schedule, one trace), bvh_room is what the driver is meant to give -- 0 after the blended
    corner under bones that differ and after the morph at weight 1, 5 again after the next apply -- and the refit took the REBUILD path."""
    from toyraygun_amd import morph, pose, rig, skin
    units = (pose, skin, morph, rig)
    for x in units:
        x.load()
    w, h = shape
    b = steps["cornell"]["rest"].buffers
    rays = _mixed_masks(step_rays[("cornell", "rest")][0])
    c = _ctx(capi, O, b, w, h)
    try:
        for what, (pos, nrm), faces in _unit_applies(O, unit, units, c, b, steps["cornell"]):
            assert refit.refit_last(c)["path"] == refit.REBUILD, (unit, what)
            moved = dict(b, positions=pos, normals=nrm)
            if faces is None:
                faces = capi.debug_room(pos, nrm, b["colors"], b["indices"], b["material_ids"])["n_faces"]
            got = _as_loaded(capi, O, c, moved, w, h, rays, (unit, what), faces, schedules=ONE_SCHEDULE)
            print("room motion unit %-14s %-18s %dx%d: bvh_room %d" % (unit, what, w, h, got["bvh_room"]))
    finally:
        for x in units:
            x.release(c)
        _close(c, refit)


# ------------------------------------------------------------------------------------------------------------------ 7. refusals keep the room
def test_refusals_keep_the_room(capi, refit, O, steps, step_rays, monkeypatch):
    """A context at `rigid` with the carried light: a refit with one infinite wall coordinate, a rig apply with a NaN clock and a skin apply through
    a binding made stale by a reload of the same buffers are refused with the codes they always had, and frame, counters, bvh_room, traces and
    the on / off pair of node steps are what they were."""
    from toyraygun_amd import rig, skin
    rig.load()
    skin.load()
    w, h = 64, 48
    rest, rigid = steps["cornell"]["rest"], steps["cornell"]["rigid"]
    rays = _mixed_masks(step_rays[("cornell", "rigid")][0])
    c = _ctx(capi, O, rest.buffers, w, h)
    try:
        _move(refit, c, rigid.buffers)
        c.set_uniforms(O.uniforms_bytes(M.uniforms(O, w, h, rigid, carried=True)))

        def state():
            return _observe(capi, c, rays, schedules=ONE_SCHEDULE), _on_and_off(c, monkeypatch)
        before = state()
        assert before[0]["bvh_room"] == 5 and before[1][1][2] > before[1][0][2]
        good = refit.refit_last(c)
        bad = rigid.buffers["positions"].copy()
        bad[3 * M.ROOM_FIRST_TRI + 4, 1] = np.inf
        with pytest.raises(capi.TrgError) as e:
            refit.refit_scene(c, bad, rigid.buffers["normals"], rigid.buffers["indices"])
        assert e.value.code == -22 and "triangle %d" % (M.ROOM_FIRST_TRI + 1) in str(e.value)
        assert state() == before and refit.refit_last(c) == good
        ids, wts, nb = M.skin_binding(rest.buffers)
        rig.bind(c, *GS.args(M.wall_rig()))
        skin.bind(c, rest.buffers["positions"], rest.buffers["normals"], rest.buffers["indices"], ids, wts, nb)
        with pytest.raises(capi.TrgError) as e:
            rig.skin_apply(c, [np.nan])
        assert e.value.code == -22 and "clock 0" in str(e.value)
        assert state() == before and refit.refit_last(c) == good
        m = rigid.buffers
        c.load_scene(m["positions"], m["normals"], m["colors"], m["indices"], m["material_ids"])      # the same buffers: only the binding goes stale
        with pytest.raises(capi.TrgError) as e:
            skin.apply(c, M.BONES["sheared"])
        assert e.value.code == -22 and "bind again" in str(e.value)
        assert state() == before
    finally:
        rig.release(c)
        skin.release(c)
        _close(c, refit)


# ------------------------------------------------------------------------------------------------------------------------------------ 8. group
@pytest.mark.parametrize("shape", SHAPES, ids=["64x48", "33x17"])
def test_group_refit_keeps_the_room(capi, refit, O, steps, monkeypatch, shape):
    """Two contexts on one device refitted to `rigid`, each rendering its band with the carried light: the gathered frame is the single context's."""
    monkeypatch.setenv("TRG_GROUP_EXCHANGE", "copy")          # (an RCCL communicator needs distinct devices; the copy exchange does not)
    w, h = shape
    rest, rigid = steps["cornell"]["rest"].buffers, steps["cornell"]["rigid"]
    u = O.uniforms_bytes(M.uniforms(O, w, h, rigid, carried=True))
    c = capi.Context(w, h)
    g = capi.Group([0, 0], w, h)
    try:
        for x in (c, g):
            x.load_scene(rest["positions"], rest["normals"], rest["colors"], rest["indices"], rest["material_ids"])
            x.set_uniforms(u)
            x.set_pixel_offsets_seed()
            refit.refit_scene(x, rigid.buffers["positions"], rigid.buffers["normals"], rigid.buffers["indices"])
        assert refit.refit_last(g, 0)["path"] == refit.refit_last(g, 1)["path"] == refit.REBUILD
        assert c.stats().bvh_room == 5 and g.rank_stats(0).bvh_room == 5 and g.rank_stats(1).bvh_room == 5
        c.render(0, SPP, BNC)
        g.render(0, SPP, BNC)
        g.sync()
        img = c.read_accum()
        assert np.isfinite(img).all() and (img[..., :3] > 0).any()
        assert np.array_equal(_bits(g.read_accum(0)), _bits(img))
    finally:
        refit.release(g)
        g.close()
        _close(c, refit)
