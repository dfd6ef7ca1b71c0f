"""The camera / light table of tests/util.py does what it claims -- on the CPU oracle, without a GPU -- so that a green run of
tests/test_gpu_uniforms.py means something.

  * every camera gives finite rays (the exactly degenerate look-at, whose rays are NaN, is thereby kept out of the table);
  * the populations the cases are there for exist: `away` shades nothing, `outside_back` mixes hits and misses, `in_tall_box` sees only the
    inside of the tall cube, every light changes the picture;
  * BLINDNESS: a uniform block read with a permuted light colour, with light_right and light_up exchanged, with a rotated light_forward or
    with the wrong sign of cam_pos.x gives another picture for cases of the table, while the default block cannot tell a permuted colour
    (white), an x <-> z exchange of light_forward ((0, -1, 0)) or the sign of cam_pos.x (0) at all;
  * HipRenderer's host-side uniforms equal the oracle's byte for byte for every camera;
  * the oracle compiled with contraction, and the oracle with the device's sin/cos, stay inside the shipped build's bar against the
    checker for every case: the inputs are chosen so that the REFERENCE passes the bar the GPU is held to.  If a later change of the oracle
    breaks that, change the case, not the bar.
"""
import numpy as np
import pytest

from tests.util import (CAMERAS, FAST_RUNS, LIGHTS, TOL_RMSE, UNIFORM_SHAPES, box_frames, box_triangles, fast_bar, image_metrics,
                        uniform_pairs, uniforms_case)

SPP, BOUNCES = 3, 5


@pytest.fixture(scope="module")
def refs(O, cornell):
    """(w, h, cam, light) -> (image, stats) of the checker (libm trig) at SPP x BOUNCES, rendered once."""
    out = {}
    for (w, h) in UNIFORM_SHAPES:
        off = O.pixel_offsets(w, h)
        for cam, light in uniform_pairs():
            out[(w, h, cam, light)] = O.render(cornell, w, h, SPP, BOUNCES, offsets=off, uniforms=uniforms_case(O, w, h, cam, light))
    return out


def test_every_camera_gives_finite_rays(O):
    for (w, h) in UNIFORM_SHAPES:
        for cam in CAMERAS:
            for frame in (0, 2 ** 32 - 1):
                u = uniforms_case(O, w, h, cam, "default", frame)
                assert np.isfinite(np.array(u.inv_view_proj)).all() and np.isfinite(np.array(u.cam_pos)).all(), cam
                rays = O.raygen(w, h, frame, uniforms=u)
                assert np.isfinite(rays["direction"]).all() and np.isfinite(rays["origin"]).all(), cam
                np.testing.assert_allclose(np.linalg.norm(rays["direction"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the light fields really are overwritten, and only their first three floats
    u, d = uniforms_case(O, 72, 40, "inside_low", "tilted_coloured"), uniforms_case(O, 72, 40, "inside_low", "default")
    assert [round(v, 6) for v in u.light_color] == [5.0, 0.5, 2.0, round(d.light_color[3], 6)]
    assert list(u.cam_pos) == list(d.cam_pos) and list(u.inv_view_proj) == list(d.inv_view_proj) and u.light_up[3] == d.light_up[3]
    assert list(d.light_pos[0:3]) == [0.0, np.float32(1.98), 0.0] and list(d.light_color[0:3]) == [1.0, 1.0, 1.0]


def test_the_populations_the_cases_are_there_for(built, O, cornell, refs):
    from toyraygun_amd import capi
    b = cornell.buffers()
    frames = box_frames(capi.debug_boxes(b["positions"], b["indices"], b["material_ids"]))
    tall = [i for i, (c, _, _) in enumerate(frames) if np.allclose(c, (-0.335, 0.6, -0.29), atol=1e-5)]
    assert len(tall) == 1
    in_tall = box_triangles(b["positions"][b["indices"]], frames) == tall[0]
    assert in_tall.sum() == 12
    for (w, h) in UNIFORM_SHAPES:
        for light in LIGHTS:
            img, st = refs[(w, h, "away", light)]
            assert (st.shaded_hits, st.bounce_rays, st.shadow_rays, st.primary_rays) == (0, 0, 0, w * h * SPP)
            assert (img[..., :3] == 0).all() and (img[..., 3] == 1).all()
            img, st = refs[(w, h, "outside_back", light)]
            lit = (img[..., :3] > 0).any(-1).mean()
            assert 0.05 < lit < 0.40, (light, lit)
            assert np.isfinite(refs[(w, h, "nearly_up", light)][0]).all()
        for frame in (0, 1, 2):
            rays = O.raygen(w, h, frame, uniforms=uniforms_case(O, w, h, "in_tall_box", "default", frame))
            hit = O.intersect_nearest(cornell, rays)
            assert (hit["primitiveIndex"] >= 0).all() and in_tall[hit["primitiveIndex"]].all()
        # every light changes the default camera's picture by more than the shipped build may differ from the oracle
        base, st = refs[(w, h, "default", "default")]
        for light in LIGHTS:
            if light != "default":
                ok, rmse, outliers, allowed = fast_bar(refs[(w, h, "default", light)][0], base, st.rays)
                assert not ok and rmse > TOL_RMSE, (light, rmse, outliers, allowed)
    assert all(np.isfinite(img).all() for img, _ in refs.values())


def _rot(v):
    return [v[1], v[2], v[0]]


def _mut_color(u):
    u.light_color[0:3] = _rot(list(u.light_color[0:3]))


def _mut_right_up(u):
    r, p = list(u.light_right[0:3]), list(u.light_up[0:3])
    u.light_right[0:3], u.light_up[0:3] = p, r


def _mut_forward_rotated(u):
    u.light_forward[0:3] = _rot(list(u.light_forward[0:3]))


def _mut_forward_xz(u):
    f = list(u.light_forward[0:3])
    u.light_forward[0:3] = [f[2], f[1], f[0]]


def _mut_cam_x(u):
    u.cam_pos[0] = -u.cam_pos[0]


# mutation -> does the DEFAULT block see it?  The colour is white, light_forward is (0, -1, 0) and cam_pos.x is 0: a permuted colour, forward's
# x and z exchanged and the other sign of cam_pos.x leave the default frame as it is, to the bit.  Two mutations the default block DOES see:
#   * a ROTATION of light_forward's components moves its one non-zero component (measured: RMSE 0.49 at 72 x 40, 2.3 at 33 x 17);
#   * light_right <-> light_up: the two span the same parallelogram whichever way round, for ANY light, so the converged picture is the same
#     and what the exchange changes is which sample of the Halton pair goes where -- sampling noise, RMSE 1.7e-2 at 3 spp on the default block,
#     seventeen times the bar and far above a bit-exact comparison.  The table adds lights whose right and up differ (0.5 against 0.11 long,
#     no zero components), where the same exchange moves single samples by up to RMSE 17.
MUTATIONS = [("light_color permuted", _mut_color, False), ("light_right <-> light_up", _mut_right_up, True),
             ("light_forward rotated", _mut_forward_rotated, True), ("light_forward x <-> z", _mut_forward_xz, False),
             ("cam_pos.x sign", _mut_cam_x, False)]


@pytest.mark.parametrize("name,mutate,default_sees_it", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_blindness_of_the_default_block_and_sight_of_the_table(O, cornell, refs, name, mutate, default_sees_it):
    for (w, h) in UNIFORM_SHAPES:
        off = O.pixel_offsets(w, h)
        rmse = {}
        for cam, light in uniform_pairs():
            u = uniforms_case(O, w, h, cam, light)
            mutate(u)
            img, _ = O.render(cornell, w, h, SPP, BOUNCES, offsets=off, uniforms=u)
            rmse[(cam, light)] = image_metrics(img, refs[(w, h, cam, light)][0])[0]
            if (cam, light) == ("default", "default") and not default_sees_it:
                assert np.array_equal(img.view(np.uint32), refs[(w, h, cam, light)][0].view(np.uint32)), name
        seen = [k for k, v in rmse.items() if v > TOL_RMSE]
        print("%s at %dx%d: default block RMSE %.3g; %d of %d cases beyond %.0e, worst %s %.3g"
              % (name, w, h, rmse[("default", "default")], len(seen), len(rmse), TOL_RMSE, max(rmse, key=rmse.get), max(rmse.values())))
        assert (rmse[("default", "default")] > TOL_RMSE) == default_sees_it, (name, rmse[("default", "default")])
        assert [k for k in seen if k != ("default", "default")], name
        if name == "cam_pos.x sign":      # (cameras with x = 0 cannot see it under any light)
            assert all(CAMERAS[c][0][0] != 0.0 for c, _ in seen)
        if name == "light_right <-> light_up":    # the table sees it far better than the default block does
            assert max(rmse.values()) > 20 * rmse[("default", "default")]


def test_host_uniforms_equal_the_oracle_for_every_camera(built, O):
    from toyraygun_amd import host
    for (w, h) in UNIFORM_SHAPES:
        for cam, (eye, at) in CAMERAS.items():
            for f in (0, 5, 2 ** 32 - 1):
                assert bytes(host.uniforms(w, h, f, eye=eye, at=at)[0]) == O.uniforms_bytes(O.make_uniforms(w, h, f, eye, at)), (cam, w, h, f)
                assert bytes(host.uniforms(w, h, f, eye=eye, at=at)[0]) == O.uniforms_bytes(uniforms_case(O, w, h, cam, "default", f))


def test_reference_builds_stay_inside_the_shipped_builds_bar(O, cornell):
    """CPU proxy for the bar of test_gpu_uniforms.test_fast_build_every_pair, on its runs (FAST_RUNS): the contracted -O3 oracle and the
    portable-trig oracle against the checker.  Measured worst case: from_above x tilted_coloured at 72 x 40, one outlier pixel of 2,880."""
    worst = {}
    for (w, h), (spp, bnc) in FAST_RUNS.items():
        off = O.pixel_offsets(w, h)
        for cam, light in uniform_pairs():
            u = uniforms_case(O, w, h, cam, light)
            ref, st = O.render(cornell, w, h, spp, bnc, offsets=off, uniforms=u)
            O.set_trig_mode(O.TRIG_PORTABLE)
            try:
                portable, pst = O.render(cornell, w, h, spp, bnc, offsets=off, uniforms=u)
            finally:
                O.set_trig_mode(O.TRIG_LIBM)
            tuned, tst = O.render(cornell, w, h, spp, bnc, offsets=off, uniforms=u, tuned=True)
            for build, img, s in (("portable", portable, pst), ("tuned", tuned, tst)):
                ok, rmse, outliers, allowed = fast_bar(img, ref, st.rays)
                assert ok, (build, cam, light, w, h, rmse, outliers, allowed)
                assert abs(s.rays - st.rays) <= 1e-4 * st.rays
                if rmse >= worst.get(build, (0.0,))[0]:
                    worst[build] = (rmse, outliers, cam, light, w, h)
    print("worst:", worst)
