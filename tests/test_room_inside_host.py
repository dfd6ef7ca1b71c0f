"""Rays that start INSIDE the room, on the host (no GPU): the rule by which the shipped build leaves the room test out for shadow rays
(trg_device.h trav_room_planes, trg_capi.cpp room_light_inside), against an fp32 numpy restatement of the whole test.

  * the shadow ray the shading event makes -- direction and distance measured from the hit point P, traced from o = P + nrm * 1e-3 to
    dist - 1e-3, so that it ends at the light sample + 1e-3 (nrm - dir) -- is never a hit of the whole test when |lo_k| <= 1 - 2^-20 in the
    room's frame and the light's corners pass the host rule, |l_k| + 2.001e-3 |a_k| <= 1 - 1e-4: with the faces the room has, and with all
    six; P on the walls with the wall's normal, on and off the walls with arbitrary unit normals, origins planted at the ballot's margin;
    without the offset term the same rays do hit (test_the_ray_end_offset_is_needed);
  * on every such origin, whatever the direction, the test without the entry plane gives the whole test's (hit, t, face) bit for bit (a
    nearest-hit form of the rule that was measured and not kept -- NOTEBOOK.md -- rests on this; so does half of the argument above);
  * the host rule for the flag (trg_debug_room_light_inside) on rectangles inside, touching the margin, poking through a present wall, poking
    through the absent face and wholly outside, and against its restatement in float64 on seeded rectangles.

The restatement rounds every fused multiply-add once (the product and the sum are formed in float64: the product of two fp32 numbers is exact
there), takes the planes -lo * i -+ |i| as one fma each and as a rounded product and a sum, and the reciprocal correctly rounded or one ulp to either side of it (v_rcp_f32 is
good to one ulp)."""
import numpy as np
import pytest

from tests import room_scenes as R

F = np.float32
INSIDE = F(1.0) - F(2.0 ** -20)           # trg_device.h kRoomInside
LIGHT_MARGIN = 1.0 - 1e-4                 # trg_capi.cpp room_light_inside (float64)
RAY_END_OFFSET = 2.001e-3                 # ... kRayEndOffset: how far a shadow ray's end may lie from its light sample, world units
HELD = F(1e30)                            # trg_device.h kRcpParallel
N = 100000
ROOMS = (("aligned", R.OPEN_FRONT), ("sheared", R.FOUR), ("rotated", R.TUBE))


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def builder_frame(C, H, scene_centre):
    """What the library keeps of the room (C, H): centre and rows in fp32 (trg_debug_room), and the rows (a_k, d_k) of the staged record, relative
    to the scene's centre (trg_capi.cpp box_frame_rows): l_k = a_k . (P - scene centre) + d_k."""
    c32, A32 = C.astype(F), np.linalg.inv(H).astype(F)
    dk = -(A32.astype(np.float64) @ (c32.astype(np.float64) - scene_centre.astype(np.float64)))
    return c32, A32, np.concatenate([A32, dk.astype(F)[:, None]], 1)


def origin_local(rows, o):
    """lo of the device: o relative to the scene's centre, three nested fma per axis."""
    return np.stack([fma(rows[k, 0], o[:, 0], fma(rows[k, 1], o[:, 1], fma(rows[k, 2], o[:, 2], rows[k, 3]))) for k in range(3)], 1)


def inside(lo):
    with np.errstate(invalid="ignore"):
        return np.abs(lo).max(1) <= INSIDE


def room_test(rows, present, o, d, tmax, ulp=0, exit_only=False, fused=True):
    """trav_room_planes in fp32: (hit, t, face, tnear).  exit_only: the test without tnear, fnear, anear and cn.  fused: the planes m -+ |i|,
    m = -lo * i, as one fma each or as a rounded product and a sum (the compiler contracts them or does not: both must hold)."""
    lo = origin_local(rows, o)
    ld = np.stack([fma(rows[k, 0], d[:, 0], fma(rows[k, 1], d[:, 1], (rows[k, 2].astype(np.float64) * d[:, 2]).astype(F))) for k in range(3)], 1)
    with np.errstate(divide="ignore"):
        inv = (F(1.0) / ld).astype(F)
    for _ in range(abs(ulp)):
        inv = np.nextafter(inv, F(np.inf if ulp > 0 else -np.inf)).astype(F)
    inv = np.clip(inv, -HELD, HELD)                                              # v_med3 with +-1e30 (an infinity is held there too)
    a = np.abs(inv)
    plane = (lambda c: fma(-lo, inv, c)) if fused else (lambda c: ((-lo * inv).astype(F) + c).astype(F))
    far = plane(a)
    tfar = far.min(1)
    s = np.signbit(inv).astype(np.int64)
    fisx, fisy = far[:, 0] <= tfar, far[:, 1] <= tfar
    ffar = np.where(fisx, s[:, 0] ^ 1, np.where(fisy, 2 + (s[:, 1] ^ 1), 4 + (s[:, 2] ^ 1)))
    afar = np.where(fisx, a[:, 0], np.where(fisy, a[:, 1], a[:, 2]))
    cf = (tfar >= 0) & (tfar <= tmax) & ((present >> ffar) & 1).astype(bool) & (afar < HELD)
    if exit_only:
        tnear, cn, fnear = np.full(len(o), F(-1.0)), np.zeros(len(o), bool), np.zeros(len(o), np.int64)
    else:
        near = plane(-a)
        tnear = near.max(1)
        nisx, nisy = near[:, 0] >= tnear, near[:, 1] >= tnear
        fnear = np.where(nisx, s[:, 0], np.where(nisy, 2 + s[:, 1], 4 + s[:, 2]))
        anear = np.where(nisx, a[:, 0], np.where(nisy, a[:, 1], a[:, 2]))
        cn = (tnear >= 0) & (tnear <= tmax) & ((present >> fnear) & 1).astype(bool) & (anear < HELD)
    hit = (tnear <= tfar) & (cn | cf)
    return hit, np.where(cn, tnear, tfar), np.where(cn, fnear, ffar), tnear


def mask_of(A32, C, H, faces):
    """The present-face mask in the numbering of the frame A32 (here the frame is (C, H) itself: no permutation, no sign)."""
    assert np.abs(A32.astype(np.float64) @ H - np.eye(3)).max() < 1e-6
    return sum(1 << f for f in faces)


def inside_origins(rng, C, H, rows, scene_centre, n):
    """fp32 origins relative to the scene's centre whose device-side lo passes the margin: uniform inside, a fifth within a few ulps of the
    margin on one or more axes (those past it are dropped: the device runs the whole test on them)."""
    l = rng.uniform(-1.0, 1.0, (2 * n, 3))
    edge = rng.random(2 * n) < 0.2
    ax = rng.random((2 * n, 3)) < 0.5
    near = (float(INSIDE) + rng.integers(-6, 3, (2 * n, 3)) * 2.0 ** -24) * rng.choice([-1.0, 1.0], (2 * n, 3))
    l = np.where(edge[:, None] & ax, near, l)
    o = ((C + l @ H.T) - scene_centre).astype(F)
    lo = origin_local(rows, o)
    keep = inside(lo)
    return o[keep][:n], np.abs(lo[keep][:n]).max(1)


def corner_reach(c32, A32, pos, right, up, offset=RAY_END_OFFSET):
    """[n, 3]: per axis of the frame the largest |l_k| of the four corners plus the ray-end offset in that axis' units, offset * |a_k| (float64)."""
    A = A32.astype(np.float64)
    reach = np.zeros((len(pos), 3))
    for sr in (-1.0, 1.0):
        for su in (-1.0, 1.0):
            P = pos.astype(np.float64) + sr * right.astype(np.float64) + su * up.astype(np.float64) - c32.astype(np.float64)
            with np.errstate(invalid="ignore"):
                l = np.abs(P @ A.T)
                reach = np.where(np.isnan(l) | np.isnan(reach), np.nan, np.maximum(reach, l))
    return reach + offset * np.linalg.norm(A, axis=1)


def host_rule_f64(c32, A32, pos, right, up, offset=RAY_END_OFFSET):
    """trg_capi.cpp room_light_inside restated (offset = 0: the rule WITHOUT the ray-end offset, which is not enough)."""
    with np.errstate(invalid="ignore"):
        return (corner_reach(c32, A32, pos, right, up, offset) <= LIGHT_MARGIN).all(1)


def light_rectangles(rng, C, H, n, c32, A32, offset=RAY_END_OFFSET):
    """n rectangles (pos, right, up in fp32, world) that pass the host rule with this offset; every other one scaled until it touches the rule's
    bound on one axis, and a quarter lie flat under one wall with all four corners at the bound (the lights whose rays from the opposite wall
    end nearest that wall).  Returns them and how close each comes to the bound."""
    lc = rng.uniform(-0.7, 0.7, (4 * n, 3))
    lr, lu = rng.normal(size=(4 * n, 3)) * 0.25, rng.normal(size=(4 * n, 3)) * 0.25
    lr[rng.random(4 * n) < 0.05] = 0.0                                           # (a light of no extent, a line)
    reach = np.max([np.abs(lc + sr * lr + su * lu) for sr in (-1, 1) for su in (-1, 1)], 0)                 # per axis
    room = LIGHT_MARGIN - offset * np.linalg.norm(np.linalg.inv(H), axis=1)     # what the rule leaves |l_k| on each axis
    fit = (room / reach).min(1)
    grow = rng.random(4 * n) < 0.5
    k = np.where(grow, fit, np.minimum(1.0, fit))
    lc, lr, lu = lc * k[:, None], lr * k[:, None], lu * k[:, None]
    flat = np.flatnonzero(rng.random(4 * n) < 0.25)                              # a quarter lie flat under a wall, all four corners at the bound
    ax = rng.integers(0, 3, len(flat))
    lr[flat, ax], lu[flat, ax] = 0.0, 0.0
    lc[flat, ax] = rng.choice([-1.0, 1.0], len(flat)) * room[ax] * (1.0 - 2e-7)  # (fp32 positions: a few land beyond the bound and are dropped)
    pos, right, up = (C + lc @ H.T).astype(F), (lr @ H.T).astype(F), (lu @ H.T).astype(F)
    ok = host_rule_f64(c32, A32, pos, right, up, offset)
    assert ok.mean() > 0.4
    slack = (LIGHT_MARGIN - corner_reach(c32, A32, pos, right, up, offset)).min(1)
    return pos[ok][:n], right[ok][:n], up[ok][:n], slack[ok][:n]


def shading_points(rng, C, H, rows, scene_centre, n):
    """Hit points and normals as the shading event meets them, and the origins it makes of them (trg_kernels.hip shade_event: o = P + nrm * 1e-3,
    the origin of the shadow ray AND of the continuation ray), fp32, relative to the scene's centre.  Half of the points lie ON a wall (any of the
    six faces, |l_k| = 1) with the wall's inward normal, a fifth on a wall or inside with an arbitrary unit normal (interpolated normals, the
    objects in the room), the rest are built backwards from origins within a few ulps of the ballot's margin.  Only origins the ballot calls
    inside are kept: the device runs the whole test on the others.  Returns (P, o, largest |lo_k|)."""
    A = np.linalg.inv(H)
    m = 3 * n
    l = rng.uniform(-1.0, 1.0, (m, 3))
    nrm = rng.normal(size=(m, 3))
    kind = rng.random(m)
    wall = kind < 0.7
    k, side = rng.integers(0, 3, m), rng.choice([-1.0, 1.0], m)
    l[wall, k[wall]] = side[wall]
    inward = -side[:, None] * A[k]                                               # the gradient of l_k, towards the inside
    nrm = np.where((kind < 0.5)[:, None], inward, nrm)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    P = ((C + l @ H.T) - scene_centre).astype(F)
    edge = kind >= 0.8                                                           # origins at the margin: P = such an origin - nrm * 1e-3
    near = (float(INSIDE) + rng.integers(-6, 3, (m, 3)) * 2.0 ** -24) * rng.choice([-1.0, 1.0], (m, 3))
    le = np.where(rng.random((m, 3)) < 0.5, near, l)
    oe = ((C + le @ H.T) - scene_centre).astype(F)
    P = np.where(edge[:, None], (oe - nrm * F(1e-3)).astype(F), P)
    o = fma(nrm, F(1e-3), P)                                                     # (contracted or not, the ballot decides on what comes out)
    lo = origin_local(rows, o)
    keep = inside(lo)
    return P[keep][:n], o[keep][:n], np.abs(lo[keep][:n]).max(1)


def shadow_rays(scene_centre, P, pos, right, up, r0, r1):
    """The shading event's shadow ray in fp32 (trg_device.h sample_area_light, trg_kernels.hip shade_event): direction and distance are measured
    FROM THE HIT POINT P, smax = dist - 1e-3 -- and the ray is traced from o = P + nrm * 1e-3, so it ends at sample + 1e-3 (nrm - dir)."""
    ux, uy = (r0 * F(2.0) - F(1.0)).astype(F), (r1 * F(2.0) - F(1.0)).astype(F)
    sp = (pos + right * ux[:, None] + up * uy[:, None]).astype(F)
    d = (sp - (P + scene_centre.astype(F))).astype(F)
    dist = np.sqrt((d * d).sum(1, dtype=F)).astype(F)
    inv = (F(1.0) / np.maximum(dist, F(1e-3))).astype(F)
    return (d * inv[:, None]).astype(F), (dist - F(1e-3)).astype(F)


@pytest.mark.parametrize("kind,faces", ROOMS, ids=[k for k, _ in ROOMS])
def test_a_segment_with_both_ends_inside_is_never_a_hit(kind, faces):
    C, H = R.frame(kind)
    scene_centre = (C + np.array([0.03, -0.21, 0.11])).astype(F).astype(np.float64)
    c32, A32, rows = builder_frame(C, H, scene_centre)
    rng = np.random.default_rng(31 + len(faces))
    P, o, reach = shading_points(rng, C, H, rows, scene_centre, N)
    assert len(o) == N and (reach == INSIDE).sum() > (1000 if kind == "aligned" else 50), int((reach == INSIDE).sum())
    pos, right, up, slack = light_rectangles(rng, C, H, N, c32, A32)
    assert len(pos) == N and (slack < 1e-6).mean() > 0.2
    r0, r1 = rng.random(N).astype(F), rng.random(N).astype(F)
    corner = rng.random(N) < 0.2                                                 # samples at the rectangle's corners and edges
    r0[corner], r1[corner] = rng.choice([F(0.0), np.nextafter(F(1.0), F(0.0))], corner.sum()), rng.choice([F(0.0), np.nextafter(F(1.0), F(0.0)), F(0.5)], corner.sum())
    d, smax = shadow_rays(scene_centre, P, pos, right, up, r0, r1)
    traced = smax >= 0                                                           # (want_shadow: shorter ones are not traced)
    assert traced.mean() > 0.99
    for present in (mask_of(A32, C, H, faces), 63):
        for ulp, fused in ((-1, True), (0, True), (1, True), (-1, False), (0, False), (1, False)):
            hit, t, _, tnear = room_test(rows, present, o[traced], d[traced], smax[traced], ulp, fused=fused)
            assert not hit.any(), (kind, present, ulp, fused, int(hit.sum()), float((t[hit] - smax[traced][hit]).max()))
            assert (tnear < 0).all()                                             # the entry plane lies behind every such origin


def test_the_ray_end_offset_is_needed():
    """The same rays under a light that passes the rule WITHOUT the offset and no more -- the Cornell box's rectangle raised to l_y = 1 - 1e-4 -
    1e-6 under the ceiling: the whole test then does report hits on the ceiling for origins the ballot calls inside.  A ray from a point of the
    floor starts 1e-3 above it and is as long as the distance from the floor itself, so it ends 1e-3 (1 - cos) above its sample, in the
    ceiling for every oblique ray.  The rule the library uses refuses this light (test_host_rule_for_the_flag plants it too)."""
    C, H = R.frame("aligned")
    scene_centre = (C + np.array([0.03, -0.21, 0.11])).astype(F).astype(np.float64)
    c32, A32, rows = builder_frame(C, H, scene_centre)
    rng = np.random.default_rng(9)
    P, o, _ = shading_points(rng, C, H, rows, scene_centre, N)
    pos = np.tile((C + [0.0, 1.0 - 1e-4 - 1e-6, 0.0]).astype(F), (N, 1))
    right, up = np.tile(np.array([0.25, 0.0, 0.0], F), (N, 1)), np.tile(np.array([0.0, 0.0, 0.25], F), (N, 1))
    assert host_rule_f64(c32, A32, pos, right, up, offset=0.0).all() and not host_rule_f64(c32, A32, pos, right, up).any()
    d, smax = shadow_rays(scene_centre, P, pos, right, up, rng.random(N).astype(F), rng.random(N).astype(F))
    hit, _, face, _ = room_test(rows, 63, o, d, smax)
    print("without the offset: %d of %d rays hit a wall, faces %s" % (hit.sum(), N, np.unique(face[hit])))
    assert hit.sum() > 1000 and (face[hit] == 3).all()                           # the face at l_y = +1


@pytest.mark.parametrize("kind,faces", ROOMS, ids=[k for k, _ in ROOMS])
def test_exit_only_is_the_whole_test_from_inside(kind, faces):
    C, H = R.frame(kind)
    scene_centre = (C + np.array([-0.07, 0.13, 0.02])).astype(F).astype(np.float64)
    c32, A32, rows = builder_frame(C, H, scene_centre)
    rng = np.random.default_rng(57 + len(faces))
    o, reach = inside_origins(rng, C, H, rows, scene_centre, N)
    assert len(o) == N and (reach == INSIDE).any()
    d = rng.normal(size=(N, 3))
    k = rng.integers(0, 3, N)
    par = rng.random(N) < 0.15                                                   # along one half axis of the room, or in the plane of two: zeros in the room's frame
    d[par] = (H[:, k[par]].T * rng.choice([-1.0, 1.0], (par.sum(), 1)) + (rng.random((par.sum(), 1)) < 0.5) * H[:, (k[par] + 1) % 3].T * rng.uniform(-1, 1, (par.sum(), 1)))
    world = rng.random(N) < 0.1                                                  # and along the world's axes, with exact zeros and -0.0
    e = np.zeros((world.sum(), 3)); e[np.arange(world.sum()), rng.integers(0, 3, world.sum())] = rng.choice([-1.0, 1.0], world.sum())
    e[rng.random(e.shape) < 0.3] *= -1.0
    d[world] = e
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    tmax = np.where(rng.random(N) < 0.3, rng.uniform(0.0, 3.0, N), np.inf).astype(F)
    hits = 0
    for present in (mask_of(A32, C, H, faces), 63):
        for ulp, fused in ((-1, True), (0, True), (1, True), (0, False)):
            hw, tw, fw, tnear = room_test(rows, present, o, d, tmax, ulp, fused=fused)
            he, te, fe, _ = room_test(rows, present, o, d, tmax, ulp, exit_only=True, fused=fused)
            assert (tnear < 0).all()
            assert np.array_equal(hw, he), (kind, present, ulp, int((hw != he).sum()))
            assert np.array_equal(tw[hw].view(np.uint32), te[hw].view(np.uint32)) and np.array_equal(fw[hw], fe[hw]), (kind, present, ulp)
            hits += int(hw.sum())
    assert hits > N                                                              # (the walls are there: most of these rays meet one)


def _block(O, pos, right, up):
    u = O.make_uniforms(64, 48)
    for name, v in (("light_pos", pos), ("light_right", right), ("light_up", up)):
        getattr(u, name)[0:3] = [float(F(x)) for x in v]
    return O.uniforms_bytes(u)


def test_host_rule_for_the_flag(capi, O, cornell):
    b = cornell.buffers()
    r = capi.debug_room(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    assert r["n_faces"] == 5 and r["present"] == 0b011111                         # x in [-1, 1], y in [0, 2], z in [-1, 1]; the face at +z is absent
    flag = lambda pos, right, up: capi.debug_room_light_inside(r["center"], r["axis"], _block(O, pos, right, up))
    assert flag((0.0, 1.98, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))           # the Cornell box's own light: l_y = 0.98
    assert capi.debug_room_light_inside(r["center"], r["axis"], O.uniforms_bytes(O.make_uniforms(64, 48)))
    assert flag((0.3, 1.2, 0.8), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))              # a point
    assert flag((0.0, 1.9978, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))         # 2.2e-3 under the ceiling: the last the rule lets through
    assert not flag((0.0, 1.9980, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))     # inside 1 - 1e-4, but a ray from the floor would end in the ceiling
    # touching the margin: nine neighbouring fp32 values around the rule's bound, 1 - 1e-4 - 2.001e-3 |a_k|, on every axis, either side, as a point light and as the corner of a
    # rectangle.  Which of them still pass is the float64 rule on the frame the builder reports (its centre and rows are fp32 and need not be
    # exactly the scene's); both answers occur on every axis and side, and the answer changes once
    half = F(0.25)
    for axis in range(3):
        for side in (-1.0, 1.0):
            v0 = F(side * (LIGHT_MARGIN - RAY_END_OFFSET * float(np.linalg.norm(r["axis"][axis].astype(np.float64)))) + float(r["center"][axis]))
            vs = [v0]
            for _ in range(4):
                vs = [np.nextafter(vs[0], F(-10.0))] + vs + [np.nextafter(vs[-1], F(10.0))]
            got = []
            for v in vs:
                p = np.array([0.1, 1.0, -0.2], F); p[axis] = v
                want = bool(host_rule_f64(r["center"], r["axis"], p[None], np.zeros((1, 3), F), np.zeros((1, 3), F))[0])
                assert flag(p, (0, 0, 0), (0, 0, 0)) == want, (axis, side, v)
                q, e = p.copy(), np.zeros(3, F)
                q[axis], e[axis] = F(v - F(side) * half), half                   # (exact where v is a multiple of 2^-24)
                want_corner = bool(host_rule_f64(r["center"], r["axis"], q[None], e[None], np.zeros((1, 3), F))[0])
                assert want_corner == want or float(q[axis]) + side * float(half) != float(v)
                assert flag(q, e, (0.0, 0.0, 0.0)) == want_corner, (axis, side, v, "corner")
                got.append(want)
            assert True in got and False in got and sum(a != b for a, b in zip(got, got[1:])) == 1, (axis, side, got)
    assert not flag((0.9, 1.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0))        # pokes through the present wall at x = +1
    assert not flag((0.0, 0.1, 0.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0))        # ... through the floor
    assert not flag((0.0, 1.0, 0.9), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))        # ... through the absent face at z = +1
    assert not flag((0.0, 1.0, 3.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0))        # wholly outside, in front of the room
    assert not flag((0.0, 5.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))        # wholly outside, above it
    assert not flag((np.nan, 1.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))
    assert not flag((0.0, 1.0, 0.0), (np.inf, 0.0, 0.0), (0.0, 0.0, 0.25))
    # tests/util.py LIGHTS: floor_up reaches z = 1.1 through the absent face; the others lie inside
    from tests.util import LIGHTS
    want = {"default": True, "tilted_coloured": True, "floor_up": False, "sideways": True, "point_dim": True}
    for name, L in LIGHTS.items():
        got = flag(*((L[0], L[2], L[3]) if L is not None else ((0.0, 1.98, 0.0), (0.25, 0.0, 0.0), (0.0, 0.0, 0.25))))
        assert got == want[name], name


@pytest.mark.parametrize("kind", ["rotated", "sheared"])
def test_host_rule_is_its_restatement(capi, O, kind):
    """2,000 seeded rectangles around the margin of a rotated and a sheared room (frames as the builder reports them, checked against the
    scene's own): the library's answer is the float64 restatement's, but for rectangles whose farthest corner lies within 1e-12 of the margin."""
    C, H = R.frame(kind)
    s = O.OracleScene()
    R.add_room(s, C, H, R.OPEN_FRONT)
    b = s.buffers()
    r = capi.debug_room(b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"])
    assert r["n_faces"] == 5 and R.match_frame(C, H, r["center"], r["axis"])[2] < 1e-5
    rng = np.random.default_rng(5)
    n = 2000
    lc, lr, lu = rng.uniform(-0.8, 0.8, (n, 3)), rng.normal(size=(n, 3)) * 0.2, rng.normal(size=(n, 3)) * 0.2
    reach = np.max([np.abs(lc + sr * lr + su * lu).max(1) for sr in (-1, 1) for su in (-1, 1)], 0)
    k = (LIGHT_MARGIN - 2.2e-3 + rng.choice([-1e-3, -1e-6, -1e-7, 0.0, 1e-7, 1e-6, 1e-3, 2.15e-3, 0.3], n)) / reach
    pos, right, up = (C + (lc * k[:, None]) @ H.T).astype(F), ((lr * k[:, None]) @ H.T).astype(F), ((lu * k[:, None]) @ H.T).astype(F)
    c32, A32 = r["center"], r["axis"]
    want = host_rule_f64(c32, A32, pos, right, up)
    decidable = np.abs(corner_reach(c32, A32, pos, right, up) - LIGHT_MARGIN).min(1) > 1e-12
    got = np.array([capi.debug_room_light_inside(c32, A32, _block(O, pos[i], right[i], up[i])) for i in range(n)])
    assert decidable.mean() > 0.99 and 0.2 < want.mean() < 0.8
    assert np.array_equal(got[decidable], want[decidable]), int((got != want)[decidable].sum())
