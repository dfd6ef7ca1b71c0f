"""Shadow rays between two points inside the room, on the GPU (-m gpu): the shipped build leaves the room test out for the any-hit rays of a
wavefront whose origins all lie inside the room when the launch's light lies inside it too (trg_device.h trav_room_planes, trg_capi.cpp
room_light_inside).  TRG_ROOM_INSIDE=0 in the environment, read per launch, switches the rule off.  The rule on the host:
tests/test_room_inside_host.py.

  * bit identity: the switch unset against 0 (and against 1, which is "on" said aloud) in one process -- accumulation buffers bit for bit, ray
    counters equal -- on the Cornell box and on scene A of tests/schedule_scenes.py (varying attributes and textures: the generic shading
    event), under the frame-serial megakernel, the frame lanes and head / tail, from the default camera and from two that put origins outside
    the room (wavefronts that mix lanes inside and outside); the strict build's bits do not know the switch;
  * the rule is in use: on the default Cornell frame the node steps counted with the switch off exceed those with it on by at least 95 % of
    the shadow rays and by no more than all of them (a skipped test is not counted as a node step);
  * the flag goes off when it must: under every light of tests/util.py LIGHTS the expected flag comes from trg_debug_room's frame on the CPU;
    where it is 0 the node steps are equal on and off; in every case the image meets fast_bar against the libm oracle; a planted rectangle that
    pokes through a present wall gives equal counters and equal bits; so do a light 2.2e-3 under the ceiling, the nearest the rule accepts, and
    one 1e-4 under it, inside the room and refused: a shadow ray is aimed from the hit point and traced from 1e-3 off it, so it ends up to 2e-3
    from its light sample, and from the floor that is in the ceiling;
  * trg_trace, nearest and any-hit, returns identical records on and off.
"""
import numpy as np
import pytest

from tests import room_scenes as R
from tests import schedule_scenes as S
from tests.util import LIGHT_FIELDS, LIGHTS, fast_bar, uniforms_case

pytestmark = pytest.mark.gpu
SHAPES = ((64, 48), (33, 17))
SPP, BNC = 6, 4
SCHEDULES = {"megakernel": dict(FRAME_SPLIT=1, TAIL_BOUNCE=0), "frame_lanes": dict(FRAME_SPLIT=2, TAIL_BOUNCE=0), "head_tail": dict(FRAME_SPLIT=1, TAIL_BOUNCE=1)}
EXPECT = {"megakernel": dict(last_frame_split=1, last_tail_bounce=0), "frame_lanes": dict(last_frame_split=2), "head_tail": dict(last_tail_bounce=1)}
CAMERAS = ("default", "outside_back", "from_above")
SWITCH = "TRG_ROOM_INSIDE"


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counts(st):
    return (int(st.primary_rays), int(st.bounce_rays), int(st.shadow_rays), int(st.shaded_hits))


def _switch(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, value)


def _cornell_ctx(capi, O, cornell, w, h):
    b = cornell.buffers()
    c = capi.Context(w, h)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.set_pixel_offsets(O.pixel_offsets(w, h))
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
    return c


def _scene_a_ctx(capi, O, w, h):
    b, uvs, ids, imgs = S.scene("A")
    c = capi.Context(w, h)
    c.load_scene(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    c.load_textures(uvs, ids, list(imgs))
    c.set_pixel_offsets(O.pixel_offsets(w, h))
    c.set_uniforms(O.uniforms_bytes(O.make_uniforms(w, h)))
    return c


def _draw(c, monkeypatch, value, counters=False):
    _switch(monkeypatch, value)
    c.reset_stats()
    c.render(0, SPP, BNC)
    st = c.stats()
    return c.read_accum(), _counts(st), (int(st.node_fetches), int(st.tri_tests)) if counters else None, st


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("scene", ["cornell", "A"])
def test_bits_do_not_know_the_switch(capi, O, cornell, monkeypatch, scene, schedule):
    for (w, h) in SHAPES:
        c = _cornell_ctx(capi, O, cornell, w, h) if scene == "cornell" else _scene_a_ctx(capi, O, w, h)
        try:
            st = c.stats()
            assert st.bvh_room == 5 and st.scene_in_lds == 1
            for k, v in SCHEDULES[schedule].items():
                c.set_option(getattr(capi, "OPT_" + k), v)
            for strict in (0, 1):
                c.set_option(capi.OPT_STRICT, strict)
                for cam in CAMERAS:
                    c.set_uniforms(O.uniforms_bytes(uniforms_case(O, w, h, cam, "default")))
                    on, on_counts, _, st = _draw(c, monkeypatch, None)
                    for k, v in EXPECT[schedule].items():
                        assert getattr(st, k) == v, (k, getattr(st, k))
                    assert np.isfinite(on).all() and st.shadow_rays > 0
                    for value in ("0", "1"):
                        off, off_counts, _, _ = _draw(c, monkeypatch, value)
                        n = int((_bits(on) != _bits(off)).any(-1).sum())
                        assert n == 0 and on_counts == off_counts, (scene, schedule, w, h, strict, cam, value, n, on_counts, off_counts)
        finally:
            c.close()


def test_the_rule_is_in_use(capi, O, cornell, monkeypatch):
    for (w, h) in SHAPES:
        c = _cornell_ctx(capi, O, cornell, w, h)
        try:
            c.set_option(capi.OPT_COUNTERS, 1)
            for schedule in SCHEDULES:
                for k, v in SCHEDULES[schedule].items():
                    c.set_option(getattr(capi, "OPT_" + k), v)
                on, on_counts, (on_nodes, on_tris), st = _draw(c, monkeypatch, None, True)
                off, off_counts, (off_nodes, off_tris), _ = _draw(c, monkeypatch, "0", True)
                part1, _, (p1_nodes, _), _ = _draw(c, monkeypatch, "1", True)
                shadow = on_counts[2]
                saved = off_nodes - on_nodes
                print("room inside %-11s %dx%d: node steps %d off, %d on: %d fewer = %.4f of %d shadow rays; primitive tests %d / %d"
                      % (schedule, w, h, off_nodes, on_nodes, saved, saved / shadow, shadow, off_tris, on_tris))
                assert np.array_equal(_bits(on), _bits(off)) and np.array_equal(_bits(on), _bits(part1)) and on_counts == off_counts
                assert 0 < saved <= shadow and on_tris == off_tris
                assert saved >= 0.95 * shadow, (schedule, w, h, saved, shadow)    # every shading point of this camera lies inside the room
                assert p1_nodes == on_nodes                                       # (any value but 0 is "on")
        finally:
            c.close()


def _flag_f64(r, u):
    """trg_capi.cpp room_light_inside restated on the frame trg_debug_room reports: the four corners of the block's light, grown by the 2.001e-3
    world units a shadow ray may end from its light sample (it is aimed from the hit point and traced from 1e-3 off it), within 1 - 1e-4."""
    pos, right, up = (np.array(getattr(u, k)[0:3], np.float64) for k in ("light_pos", "light_right", "light_up"))
    A, cen = r["axis"].astype(np.float64), r["center"].astype(np.float64)
    grow = 2.001e-3 * np.linalg.norm(A, axis=1)
    return all(bool((np.abs(A @ (pos + sr * right + su * up - cen)) + grow <= 1.0 - 1e-4).all()) for sr in (-1.0, 1.0) for su in (-1.0, 1.0))


# name -> ((pos, forward, right, up, colour), expected flag)
PLANTED = {
    "planted": (((0.9, 1.0, 0.0), (0.0, -1.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0), (1.0, 0.9, 0.8)), False),      # pokes through the present wall at x = +1
    # 2.2e-3 under the ceiling (a present wall), the nearest the rule accepts: a ray from the floor ends up to 2e-3 above its sample, still inside
    "near_ceiling": (((0.0, 1.9978, 0.0), (0.0, -1.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25), (1.0, 0.9, 0.8)), True),
    # 1.01e-4 under the ceiling: within 1 - 1e-4 of the frame, and the oblique rays from the floor end IN the ceiling.  The whole test calls them
    # occluded, so the rule must refuse this light.  (No oracle bar here: rays that end within rounding of the ceiling's plane are a set fp32
    # cannot decide; what is asked is that the switch changes nothing.)
    "too_near_ceiling": (((0.0, 1.999899, 0.0), (0.0, -1.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25), (1.0, 0.9, 0.8)), False),
}


@pytest.mark.parametrize("light", list(LIGHTS) + list(PLANTED))
def test_the_flag_goes_off_when_it_must(capi, O, cornell, monkeypatch, light):
    b = cornell.buffers()
    r = capi.debug_room(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    for (w, h) in SHAPES:
        if light in PLANTED:
            u = O.make_uniforms(w, h)
            for name, v in zip(LIGHT_FIELDS, PLANTED[light][0]):
                getattr(u, name)[0:3] = [float(np.float32(x)) for x in v]
        else:
            u = uniforms_case(O, w, h, "default", light)
        want = _flag_f64(r, u)
        assert want == capi.debug_room_light_inside(r["center"], r["axis"], O.uniforms_bytes(u))
        expected = {"default": True, "tilted_coloured": True, "floor_up": False, "sideways": True, "point_dim": True}
        assert want == (PLANTED[light][1] if light in PLANTED else expected[light])
        ref, rst = O.render(cornell, w, h, SPP, BNC, offsets=O.pixel_offsets(w, h), uniforms=u)
        c = _cornell_ctx(capi, O, cornell, w, h)
        try:
            c.set_option(capi.OPT_COUNTERS, 1)
            c.set_uniforms(O.uniforms_bytes(u))
            on, on_counts, (on_nodes, _), st = _draw(c, monkeypatch, None, True)
            off, off_counts, (off_nodes, _), _ = _draw(c, monkeypatch, "0", True)
            ok, rmse, outliers, allowed = fast_bar(on, ref, rst.rays)
            print("room inside light %-15s %dx%d: flag %d, node steps %d off / %d on, shadow rays %d; rmse %.3e outliers %d (allowed %d)"
                  % (light, w, h, want, off_nodes, on_nodes, on_counts[2], rmse, outliers, allowed))
            assert np.array_equal(_bits(on), _bits(off)) and on_counts == off_counts, (light, w, h)
            if want:
                assert 0 < off_nodes - on_nodes <= on_counts[2], (light, w, h)
            else:
                assert off_nodes == on_nodes, (light, w, h, off_nodes, on_nodes)
            if light != "too_near_ceiling":
                assert ok and abs(st.rays - rst.rays) <= 1e-4 * max(rst.rays, 1), (light, w, h, rmse, outliers, allowed, st.rays, rst.rays)
            if light in ("near_ceiling", "too_near_ceiling"):                    # ... and from the cameras that mix lanes inside and outside, every schedule
                for schedule in SCHEDULES:
                    for k, v in SCHEDULES[schedule].items():
                        c.set_option(getattr(capi, "OPT_" + k), v)
                    for cam in CAMERAS:
                        uc = uniforms_case(O, w, h, cam, "default")
                        for name, v in zip(LIGHT_FIELDS, PLANTED[light][0]):
                            getattr(uc, name)[0:3] = [float(np.float32(x)) for x in v]
                        c.set_uniforms(O.uniforms_bytes(uc))
                        a, a_counts, _, _ = _draw(c, monkeypatch, None, True)
                        z, z_counts, _, _ = _draw(c, monkeypatch, "0", True)
                        assert np.array_equal(_bits(a), _bits(z)) and a_counts == z_counts, (light, w, h, schedule, cam)
        finally:
            c.close()


def test_tracing_is_untouched(capi, O, cornell, monkeypatch):
    C, H = R.frame("aligned")
    o, d, tmax, _ = R.room_rays(C, H, R.OPEN_FRONT, 91, 20000)
    c = _cornell_ctx(capi, O, cornell, 64, 48)
    try:
        got = {}
        for value in (None, "0"):
            _switch(monkeypatch, value)
            for mask in (1, 3):
                rays = R.as_trace_rays(O, o, d, tmax, mask)
                got[(value, mask)] = (c.trace(rays), c.trace(rays, any_hit=True))
        for mask in (1, 3):
            (a, a_any), (z, z_any) = got[(None, mask)], got[("0", mask)]
            assert (a["primitiveIndex"] >= 0).mean() > 0.3
            assert a.tobytes() == z.tobytes() and a_any.tobytes() == z_any.tobytes(), mask
    finally:
        c.close()
