"""Synthetic frames and matrices for the temporal step (include/trg_denoise.h; tests/test_gpu_temporal_shapes.py imports them from here), and host-side
checks, on the float64 reference alone, that these inputs reach what they are meant to reach.  No GPU.

trg_temporal_denoise_host takes colour, guides, positions and the previous view-projection from the caller, so a test needs no render:

THE STAGE.  World space is the pixel grid: X(p) = (x + 0.5, y + 0.5, -z_p).  Two planes z = z0 + a X + b Y, interleaved in small blocks: a deep
"floor" (z about 3) and a "raised" pattern (z in 1 .. 2.5), each with its geometric normal (a, b, 1) scaled to a length that is not 1
(1.2 and 0.9), so a tap on the same plane is at plane distance 0 wherever the camera moved it, and a tap on the other plane is far outside
every tolerance.  About 5 % misses, about 4 % hits with a ZERO normal, 2 % first-hit emitters (primitive 35, the Cornell box's light, which
the contexts of these tests hold), albedo in [0.0005, 1] (some channels under the 1e-3 clamp).  Every pixel with (x + 2 y) % 5 == 0 is pushed
off its plane in X.z by 0.3 .. 6 times the default plane tolerance 0.02 z: the plane test rejects real taps, and which ones depends on
plane_tol.  The zero normals keep out of the 16 x 16 tiles whose tile coordinates add up to an odd number, so that the spatial-estimate kernel
meets tiles it leaves early as well as tiles with N < 4 and N >= 4 side by side.
A second stage (seed 2: other blocks, depths 0.012 deeper) gives its blocks SHADING normals that do not follow the planes -- every other one
untilted, the others in turn tilted by 0.5, by 0.3 and by -2: cosines 1, 0.894, 0.953 and 0.447 against the first stage's --: as the previous frame of a call it makes F' and X'
differ from the current frame's and feeds the normal test cosines on either side of 0.9, 0.97 and 0.5.
The normals' lengths keep (n_p . n_q)^128 <= 1.44^128 = 2e20: the header's w_n takes the normals as they come, and fp32 is to hold it.

THE MATRICES.  ortho_vp(w, h, sx, sy): clip.w = 1, world (X, Y) lands on the sample position (X + sx, Y + sy), i.e. fx = x + sx.
perspective_vp(w, h): clip.w = 2.75 + Z, scaled by 0.6 about the image centre and shifted by (0.31, -0.17): the floor is BEHIND the previous camera (clip.w <= 0; without
the test of clip.w its pixels would land mirrored inside the image, on other floor pixels whose plane and normal tests they pass), the raised
pattern in front, most of it landing inside the image on its own plane.

THE SCHEDULE (SCHEDULE below; nine calls): no history, rest, a sub-pixel shift, rest (the call in which the history turns four frames old), rest,
the shift (-0.75, 0.6) that puts border pixels at fx in [-1, 0) with the second stage, the perspective matrix against that second stage,
the shift (2.3, 1.6) with the second stage again, and a shift that throws every pixel out of the window (no history anywhere, N = 1)."""
import numpy as np
import pytest

from tests.test_temporal_host import NEAR_CAP, seeded_colour

f32 = np.float32
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (15, 17), (16, 16), (32, 16), (17, 33), (48, 32)]     # w x h, those of tests/test_gpu_denoise_shapes.py
IDENTITY_SHAPES = [(16, 16), (32, 16), (4, 2)]                                                  # powers of two: fx = x exactly
ONE_STATE_SHAPE = (37, 29)
LIGHT = 35                                    # an emissive triangle of the Cornell box
SHIFTS = dict(sub=(0.37, -0.21), border=(-0.75, 0.6), large=(2.3, 1.6))
PLANES = dict(floor=(3.0, 0.004, 0.003), raised=(1.5, 0.02, -0.015))                            # z0, a, b
PERSPECTIVE = (2.75, 1.0, 0.6, (0.31, -0.17))    # clip.w = c0 + c1 Z; the scale about the image centre; a sub-pixel shift on top

# (stage seed, the previous camera): the calls of the shape and the parameter tests
SCHEDULE = [(1, None), (1, "rest"), (1, "sub"), (1, "rest"), (1, "rest"), (2, "border"), (1, "perspective"), (2, "large"), (1, "out")]
TURNS_FOUR = 3                                # N = 1, 2, 3, 4 up to a rounding over calls 0 .. 3: there N against 4 is undecidable for most pixels
IDENTITY_SCHEDULE = [(1, None)] + [(1, "rest")] * 5
ONE_STATE_SCHEDULE = [(1, None), (1, "sub"), (2, "border"), (1, "large")]

# the parameter tests: every field but `iterations` differs from the defaults and between the sets (demodulate has two values only).  "degenerate" is the set with
# alpha = alpha_moments = 1 and max_history = 1: every found history gives N = 1 and a = am = 1, and V_0 is always the spatial form.
PARAM_SETS = {
    "low":        dict(sigma_lum=2.0, sigma_normal=8.0, sigma_depth=2.0, demodulate=0, alpha=0.1, alpha_moments=0.3, plane_tol=0.05, normal_tol=0.5, max_history=6),
    "anynormal":  dict(sigma_lum=8.0, sigma_normal=0.0, sigma_depth=0.25, demodulate=0, alpha=0.5, alpha_moments=0.45, plane_tol=0.1, normal_tol=-1.0, max_history=5),
    "tight":      dict(sigma_lum=1.0, sigma_normal=32.0, sigma_depth=0.5, demodulate=1, alpha=0.35, alpha_moments=0.6, plane_tol=0.01, normal_tol=0.97, max_history=7),
    "degenerate": dict(sigma_lum=3.0, sigma_normal=64.0, sigma_depth=4.0, demodulate=1, alpha=1.0, alpha_moments=1.0, plane_tol=0.03, normal_tol=0.7, max_history=1),
}
SHAPES_PARAMS = dict(max_history=6)           # the shape tests; the GPU tests add iterations = 0
# Fields whose default cannot be told from the set's value, by the definition itself: sigma_lum is read by the filter iterations only and the
# step is compared with iterations = 0; in "degenerate" N = 1 wherever history is found, so a = max(alpha, 1/N) = 1 = am whatever alpha and
# alpha_moments are, and with a = am = 1 the history's values cancel (I = Ih + 1 (D - Ih)): which taps the plane and the normal test let
# through no longer shows beyond a rounding.
INVISIBLE = {"low": {"sigma_lum"}, "anynormal": {"sigma_lum"}, "tight": {"sigma_lum"},
             "degenerate": {"sigma_lum", "alpha", "alpha_moments", "plane_tol", "normal_tol"}}


# ---- generators -------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def stage(w, h, seed):
    """(guides [2, h, w, 4], X [h, w, 4]) float32 of the stage with this seed (1: normals along the planes; any other: tilted shading normals)."""
    rng = np.random.default_rng(1000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    Xc, Yc = xx + 0.5, yy + 0.5
    bw, bh = (3, 2) if seed == 1 else (2, 3)
    bx, by = (xx + seed) // bw, (yy + 2 * seed) // bh
    block = bx + by
    raised = block % 2 == 1
    deeper = 0.0 if seed == 1 else 0.012
    z = np.where(raised, PLANES["raised"][0] + PLANES["raised"][1] * Xc + PLANES["raised"][2] * Yc,
                 PLANES["floor"][0] + PLANES["floor"][1] * Xc + PLANES["floor"][2] * Yc) + deeper
    n = np.where(raised[..., None], 0.9 * _unit((PLANES["raised"][1], PLANES["raised"][2], 1.0)), 1.2 * _unit((PLANES["floor"][1], PLANES["floor"][2], 1.0)))
    if seed != 1:
        tilts = np.array([1.1 * _unit((0.004, 0.003, 1.0)), 1.05 * _unit((0.5, 0.0, 1.0)), 0.95 * _unit((0.3, 0.1, 1.0)), 1.15 * _unit((-2.0, 0.0, 1.0))])
        n = tilts[np.array([0, 1, 0, 2, 0, 3])[(bx + 2 * by) % 6]]                  # (per block: at sigma_normal = 128 a pixel alone with its normal has V_0 near 0)
    u = rng.uniform(0.0, 1.0, (h, w))
    u[0, 0] = 0.5                                                          # (the 1 x 1 image is a hit with a normal)
    miss = u < 0.05
    zero = (u >= 0.05) & (u < 0.12) & ((xx // 16 + yy // 16) % 2 == 0)
    light = (u >= 0.95) & (u < 0.97)
    g = np.zeros((2, h, w, 4), f32)
    g[0, ..., :3] = np.where(zero[..., None], 0.0, n).astype(f32)
    g[0, ..., 3] = z.astype(f32)
    g[1, ..., :3] = rng.uniform(0.0005, 1.0, (h, w, 3)).astype(f32)
    ids = np.where(rng.uniform(0.0, 1.0, (h, w)) < 0.5, 3, 100000).astype(np.int32)    # a primitive of the Cornell box, and one beyond it
    ids[light] = LIGHT
    pushed = (xx + 2 * yy) % 5 == 0
    push = np.where(pushed, rng.choice([-1.0, 1.0], (h, w)) * rng.uniform(0.3, 6.0, (h, w)) * 0.02 * z, 0.0)
    X = np.zeros((h, w, 4), f32)
    X[..., 0], X[..., 1], X[..., 2] = Xc, Yc, (-z - push).astype(f32)
    g[0][miss] = (0.0, 0.0, 0.0, -1.0)
    g[1][miss] = 0.0
    ids[miss] = -1
    X[miss] = 0.0
    g[1, ..., 3] = ids.view(f32)
    return g, X


def ortho_vp(w, h, sx, sy):
    """World -> clip with clip.w = 1: world (X, Y) lands on the sample position (X + sx, Y + sy)."""
    m = np.zeros(16, np.float64)
    m[0], m[3] = 2.0 / w, 2.0 * sx / w - 1.0
    m[5], m[7] = 2.0 / h, 2.0 * sy / h - 1.0
    m[10] = m[15] = 1.0
    return m.astype(f32)


def perspective_vp(w, h, c0=PERSPECTIVE[0], c1=PERSPECTIVE[1], scale=PERSPECTIVE[2], shift=PERSPECTIVE[3]):
    """World -> clip with clip.w = c0 + c1 Z and clip.xy = scale * (the ndc of ortho_vp(w, h, 0, 0)) + (the ndc of `shift`) * clip.w: a sample lands at
    centre + scale (X - centre) / clip.w + shift.  (The sub-pixel shift keeps the centre column of an odd width off the pixel grid, where W > 0
    could not be decided.)"""
    m = np.zeros(16, np.float64)
    ox, oy = 2.0 * shift[0] / w, 2.0 * shift[1] / h
    m[0], m[2], m[3] = scale * 2.0 / w, ox * c1, ox * c0 - scale
    m[5], m[6], m[7] = scale * 2.0 / h, oy * c1, oy * c0 - scale
    m[10] = 1.0
    m[14], m[15] = c1, c0
    return m.astype(f32)


def previous_camera(w, h, name):
    if name is None:
        return None
    if name == "rest":
        return ortho_vp(w, h, 0.0, 0.0)
    if name == "perspective":
        return perspective_vp(w, h)
    if name == "out":
        return ortho_vp(w, h, -w - 3.0, 0.0)
    return ortho_vp(w, h, *SHIFTS[name])


def schedule_frames(w, h, schedule, colour_seed=500):
    """[(colour, guides, X, prev_vp or None, the camera's name)] of a schedule's calls."""
    stages = {seed: stage(w, h, seed) for seed in {s for s, _ in schedule}}
    return [(seeded_colour(stages[seed][0], colour_seed + call),) + stages[seed] + (previous_camera(w, h, cam), cam) for call, (seed, cam) in enumerate(schedule)]


# ---- what a call's inputs reach: a census of the definition's decisions, float64 -----------------------------------------------------------------
def census(dn, g, X, prev, vp, mats, plane_tol=0.02, normal_tol=0.9, **_):
    """Per-pixel bool planes of one call whose previous history planes are `prev` [4, h, w, 4] (None: all False): `hit` (not a miss, not an emitter),
    `zero` (a hit whose normal has no length), `behind` (a hit with clip.w <= 0), `front` (a hit with a normal and clip.w > 0), `partial` (in the
    window with one to three of the four taps outside the image), `plane` (some live tap fails the plane test), `normal` (some live tap passes the
    plane test and fails the normal test), `found` (W > 0)."""
    F, _, miss = dn._filter_inputs(g[0], g[1], mats, np.float64)
    h, w = miss.shape
    hit = ~miss
    ln = np.sqrt((F[..., :3] ** 2).sum(-1))
    out = dict(hit=hit, zero=hit & ~(ln > 0))
    for k in ("behind", "front", "partial", "plane", "normal", "found"):
        out[k] = np.zeros((h, w), bool)
    if prev is None:
        return out
    P = np.asarray(X, np.float64)[..., :3]
    m = np.asarray(vp, np.float64)
    clip = [m[4 * j] * P[..., 0] + m[4 * j + 1] * P[..., 1] + m[4 * j + 2] * P[..., 2] + m[4 * j + 3] for j in (0, 1, 3)]
    out["behind"] = hit & ~(clip[2] > 0)
    front = hit & (ln > 0) & (clip[2] > 0)
    out["front"] = front
    cw = np.where(front, clip[2], 1.0)
    fx, fy = (clip[0] / cw * 0.5 + 0.5) * w - 0.5, (clip[1] / cw * 0.5 + 0.5) * h - 0.5
    window = front & (fx >= -1) & (fx < w) & (fy >= -1) & (fy < h)
    fx, fy = np.where(window, fx, 0.0), np.where(window, fy, 0.0)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    tx, ty = fx - x0, fy - y0
    W = np.zeros((h, w))
    n = F[..., :3] / np.where(ln > 0, ln, 1.0)[..., None]
    Hf, Hx = np.asarray(prev[2], np.float64), np.asarray(prev[3], np.float64)[..., :3]
    outside = np.zeros((h, w), np.int64)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            outside += window & ~inside
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            fq = Hf[cy, cx]
            live = window & inside & (fq[..., 3] >= 0)
            dist = np.abs((n * (Hx[cy, cx] - P)).sum(-1))
            on_plane = dist <= plane_tol * F[..., 3]
            lq = np.sqrt((fq[..., :3] ** 2).sum(-1))
            cosn = (n * fq[..., :3]).sum(-1) / np.where(lq > 0, lq, 1.0)
            out["plane"] |= live & ~on_plane
            facing = (lq > 0) & (cosn >= normal_tol)
            out["normal"] |= live & on_plane & ~facing
            W += np.where(live & on_plane & facing, (tx if i else 1 - tx) * (ty if j else 1 - ty), 0.0)
    out["found"] = W > 0
    out["partial"] = window & (outside >= 1) & (outside <= 3)
    return out


def tiles(mask_lt4, hit, w, h):
    """(tiles with a hit of N < 4 and a hit of N >= 4, tiles with hits and none of N < 4) over the 16 x 16 tiles of the image."""
    mixed = quiet = 0
    for ty in range(0, h, 16):
        for tx in range(0, w, 16):
            a, b = mask_lt4[ty:ty + 16, tx:tx + 16], hit[ty:ty + 16, tx:tx + 16]
            lt, ge = bool((a & b).any()), bool((~a & b).any())
            mixed += lt and ge
            quiet += ge and not lt
    return mixed, quiet


def near_caps(near, near_n, call, turns_four=TURNS_FOUR):
    """The cap of tests/test_gpu_temporal.py, and at most one pixel on images under 256 pixels."""
    n = near.size
    cap = NEAR_CAP * n if n >= 256 else 1
    assert near.sum() <= cap, (call, int(near.sum()), n)
    assert near_n.sum() <= cap or call == turns_four, (call, int(near_n.sum()), n)


def run_reference(dn, w, h, schedule, mats, params, on_call=None):
    """The float64 reference chained through a schedule.  Returns per call (frame, (new history, iv, (near, near_n)), census, previous history)."""
    hist, calls = None, []
    for call, frame in enumerate(schedule_frames(w, h, schedule)):
        colour, g, X, vp, cam = frame
        ref = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, material_ids=mats, near_parts=True, **params)
        calls.append((frame, ref, census(dn, g, X, hist, vp, mats, **params), hist))
        hist = ref[0]
    return calls


def spatial_form(dn, new, params):
    """V_0's spatial form from a step's new history planes (Hc, Hm, F, X), float64: the definition's N < 4 branch for every pixel."""
    q = dict(dn._TEMPORAL_DEFAULTS)
    q.update(params)
    F, m1, m2, N = new[2], new[1, ..., 0], new[1, ..., 1], new[0, ..., 3]
    miss = F[..., 3] < 0
    G = dn.geometry_weights(F, 1, float(f32(q["sigma_normal"])), float(f32(q["sigma_depth"])), kernel=(1.0,) * 7)
    gs = G.sum((0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        M1, M2 = dn._gather(G, m1, 1) / gs, dn._gather(G, m2, 1) / gs
        v = np.where(gs > 0, np.maximum(0.0, M2 - M1 * M1) * 4.0 / np.where(miss, 1.0, N), 0.0)
    return np.where(miss, 0.0, v)


# ---- the comparison of one step: the bar rule of tests/test_gpu_temporal.py, unchanged ----------------------------------------------------------
COLOUR_BAR, VARIANCE_BAR = 1e-4, 1e-3


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.sqrt(((a - ref) ** 2).sum(-1)) / np.maximum(1.0, np.sqrt((ref ** 2).sum(-1)))


def _max(a):
    return float(a.max()) if a.size else 0.0


def step_reference(dn, frame, prev, mats, params, ignore_near_n=False):
    """One step of the reference from the previous history planes `prev` (None: no history), in float64 and in the float32 mode, and what follows
    from the two alone: the compared pixels (`ok`: not near; `okv`, for V_0: nor near_n, unless ignore_near_n), E32 and the bar coefficients
    max(1e-4, 4 E32) on colour, on N and on the moments, max(1e-3, 4 E32) on V_0."""
    colour, g, X, vp, cam = frame
    args = (colour, g[0], g[1], X, prev, None if prev is None else vp)
    new, iv, (near, near_n) = dn.reference_temporal(*args, material_ids=mats, near_parts=True, **params)
    n32, iv32, _ = dn.reference_temporal(*args, material_ids=mats, dtype=np.float32, **params)
    ok = ~near
    okv = ok if ignore_near_n else ok & ~near_n
    v64, v32 = iv[..., 3], iv32[..., 3].astype(np.float64)
    e = (_max(_rel(n32[0][..., :3], new[0][..., :3])[ok]), _max(_rel(n32[0][..., 3:], new[0][..., 3:])[ok]), _max(_rel(n32[1], new[1])[ok]),
         _max((np.abs(v32 - v64) / (np.abs(v64) + 1e-9))[okv]))
    bars = (max(COLOUR_BAR, 4.0 * e[0]), max(COLOUR_BAR, 4.0 * e[1]), max(COLOUR_BAR, 4.0 * e[2]), max(VARIANCE_BAR, 4.0 * e[3]))
    return dict(new=new, iv=iv, n32=n32, near=near, near_n=near_n, ok=ok, okv=okv, e32=e, bars=bars)


def step_ratios(R, hc, hm, iv):
    """error / bar of (Hc, Hm, (I, V_0)) -- the device's, or another evaluation of the reference -- on the compared pixels of step_reference's R:
    Hc.rgb, N, Hm, I.rgb, V_0."""
    ok, okv, (bc, bn, bm, bv) = R["ok"], R["okv"], R["bars"]
    new, v64 = R["new"], R["iv"][..., 3]
    return (_rel(hc[..., :3], new[0][..., :3])[ok] / bc, _rel(hc[..., 3:], new[0][..., 3:])[ok] / bn, _rel(hm, new[1])[ok] / bm,
            _rel(iv[..., :3], R["iv"][..., :3])[ok] / bc, (np.abs(np.asarray(iv[..., 3], np.float64) - v64) / (bv * np.abs(v64) + 1e-9))[okv])


def varied_fields(dn, params):
    return [k for k, v in dn._TEMPORAL_DEFAULTS.items() if k != "iterations" and k in params and float(f32(params[k])) != float(f32(v))]


def visible_fields(dn, R, frame, prev, mats, params):
    """The varied fields of `params` whose DEFAULT value moves the reference of this step by more than the bar on some compared pixel."""
    colour, g, X, vp, cam = frame
    seen = set()
    for k in varied_fields(dn, params):
        alt = dict(params)
        alt[k] = dn._TEMPORAL_DEFAULTS[k]
        new, iv, _ = dn.reference_temporal(colour, g[0], g[1], X, prev, None if prev is None else vp, material_ids=mats, **alt)
        if any(_max(r) > 1.0 for r in step_ratios(R, new[0], new[1], iv)):
            seen.add(k)
    return seen


# ---- host tests ---------------------------------------------------------------------------------------------------------------------------------
def test_the_matrices_land_where_they_say():
    """ortho_vp: fx = x + sx, fy = y + sy to a rounding, and exactly x, y at powers of two with no shift, in fp32 as the kernel forms them;
    perspective_vp: clip.w = 2.75 + Z, the floor behind, the raised pattern in front and inside the image."""
    for w, h in SHAPES + IDENTITY_SHAPES:
        g, X = stage(w, h, 1)
        for sx, sy in [(0.0, 0.0)] + list(SHIFTS.values()) + [(-w - 3.0, 0.0)]:
            m = ortho_vp(w, h, sx, sy)
            cx = (m[0] * X[..., 0] + m[1] * X[..., 1]) + m[2] * X[..., 2] + m[3]
            cy = (m[4] * X[..., 0] + m[5] * X[..., 1]) + m[6] * X[..., 2] + m[7]
            cw = (m[12] * X[..., 0] + m[13] * X[..., 1]) + m[14] * X[..., 2] + m[15]
            fx, fy = (cx / cw * f32(0.5) + f32(0.5)) * f32(w) - f32(0.5), (cy / cw * f32(0.5) + f32(0.5)) * f32(h) - f32(0.5)
            hit = g[0, ..., 3] >= 0
            yy, xx = np.mgrid[0:h, 0:w]
            assert fx.dtype == f32 and (cw[hit] == 1).all()
            assert np.abs(fx - (xx + sx))[hit].max() <= 1e-5 * max(w, 4) and np.abs(fy - (yy + sy))[hit].max() <= 1e-5 * max(h, 4)
            if (w, h) in IDENTITY_SHAPES and sx == 0.0 and sy == 0.0:
                assert np.array_equal(fx[hit], xx[hit].astype(f32)) and np.array_equal(fy[hit], yy[hit].astype(f32))
            if sx < -w:
                assert (fx < -1).all()
        m = perspective_vp(w, h).astype(np.float64)
        P = X[..., :3].astype(np.float64)
        cw = m[12] * P[..., 0] + m[13] * P[..., 1] + m[14] * P[..., 2] + m[15]
        assert np.allclose(cw[hit], PERSPECTIVE[0] + P[..., 2][hit])
        raised = hit & (g[0, ..., 3] < 2.7)
        on_plane = np.abs(X[..., 2] + g[0, ..., 3]) < 1e-3                              # (a pushed pixel may come out on the other side)
        assert (cw[raised & on_plane] > 0.2).all() and (cw[hit & ~raised & on_plane] < -0.2).all()
        fx = ((m[0] * P[..., 0] + m[2] * P[..., 2] + m[3]) / cw * 0.5 + 0.5) * w - 0.5
        fy = ((m[5] * P[..., 1] + m[6] * P[..., 2] + m[7]) / cw * 0.5 + 0.5) * h - 0.5
        with np.errstate(invalid="ignore", divide="ignore"):
            clear = hit & (np.abs(cw) > 0.1)                                            # (the matrix is rounded to fp32)
            assert np.allclose(fx[clear], (w / 2 + PERSPECTIVE[2] * (P[..., 0] - w / 2) / cw + PERSPECTIVE[3][0] - 0.5)[clear], rtol=1e-4, atol=1e-4)
        assert w * h < 255 or ((fx >= -1) & (fx < w) & (fy >= -1) & (fy < h))[raised & on_plane].mean() >= 0.5


def test_the_stage_holds_what_it_promises(cornell):
    """At 48 x 32: the shares of misses, zero normals, emitters and pushed pixels, non-unit normals on two planes, albedo under the clamp, X on the
    pixel grid; the second stage differs in F and X on most pixels."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = 48, 32
    (g, X), (g2, X2) = stage(w, h, 1), stage(w, h, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    for gg, XX in ((g, X), (g2, X2)):
        miss = gg[0, ..., 3] < 0
        light = dn.emitter_mask(gg[1], mats)
        hit = ~miss & ~light
        ln = np.sqrt((gg[0, ..., :3].astype(np.float64) ** 2).sum(-1))
        zero = hit & (ln == 0)
        assert 0.03 < miss.mean() < 0.08 and 0.02 < zero.sum() / hit.sum() < 0.07 and 2 <= light.sum() < 0.05 * w * h
        assert (gg[0][miss] == (0, 0, 0, -1)).all() and (gg[1][miss][:, :3] == 0).all() and (XX[miss] == 0).all()
        assert (gg[1, ..., 3][miss].view(np.int32) == -1).all()
        assert (np.abs(ln[hit & ~zero] - 1) > 0.04).all() and ln.max() <= 1.2 + 1e-6
        assert (gg[1, ..., :3][hit] < 1e-3).any() and (gg[1, ..., :3][hit] >= 0.0005).all()
        assert np.array_equal(XX[..., 0][~miss], (xx + 0.5).astype(f32)[~miss]) and np.array_equal(XX[..., 1][~miss], (yy + 0.5).astype(f32)[~miss])
        off = np.abs(XX[..., 2] + gg[0, ..., 3]) > 1e-3
        assert np.array_equal(off & ~miss, ((xx + 2 * yy) % 5 == 0) & ~miss)
        assert not zero[:16, 16:32].any() and zero[:16, :16].any()
        z = gg[0, ..., 3]
        assert (z[~miss] < 2.6).any() and (z[~miss] > 2.9).any() and not ((z > 2.6) & (z < 2.9)).any()
    both = (g[0, ..., 3] >= 0) & (g2[0, ..., 3] >= 0)
    assert (np.abs(g[0] - g2[0]).max(-1)[both] > 1e-3).mean() > 0.9 and (np.abs(X - X2).max(-1)[both] > 1e-3).mean() > 0.9


def _populations(calls, w, h):
    """The populations a schedule is meant to reach, summed over its calls."""
    tot = dict(hits=0, zero_lonely=0, partial=0, plane=0, normal=0, nonint=0, mixed=0, quiet=0, behind=0.0, front_found=0.0)
    for call, (frame, (new, iv, (near, near_n)), cen, hist) in enumerate(calls):
        N = new[0, ..., 3]
        hit = cen["hit"]
        found = cen["found"]
        if hist is not None and frame[4] != "out":
            tot["hits"] += int(hit.sum())
            around = np.zeros_like(hit)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    around |= _shifted(found, dx, dy)
            tot["zero_lonely"] += int((cen["zero"] & ~found & (N == 1) & around).sum())
            for k in ("partial", "plane", "normal"):
                tot[k] += int(cen[k].sum())
            tot["nonint"] += int((hit & (np.abs(N - np.round(N)) > 1e-3)).sum())
        mixed, quiet = tiles(N < 4, hit, w, h)
        tot["mixed"] += mixed
        tot["quiet"] += quiet
        if frame[4] == "perspective":
            tot["behind"] = float(cen["behind"].sum()) / max(1, int(hit.sum()))
            tot["front_found"] = float((cen["front"] & found).sum()) / max(1, int(cen["front"].sum()))
    return tot


def _shifted(mask, dx, dy):
    from toyraygun_amd.denoise import _shift
    return _shift(mask, dx, dy, False)[0]


@pytest.mark.parametrize("name", ["shapes"] + list(PARAM_SETS))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_schedule_reaches_its_populations(cornell, size, name):
    """The reference alone over SCHEDULE, with the parameters of the shape tests and of every parameter set, at every shape: `near` and `near_n`
    under their caps in every call, and every population non-empty.  On images of at least 255 pixels, over the calls that look for history: zero-normal hits
    without history beside pixels that find it; in the perspective call at least 10 % of the hits behind the camera and at least 10 % of those in
    front finding history; pixels with one to three taps outside the image; at least 3 % of the hits with a live tap the plane test rejects, and 3 %
    with one the normal test rejects; non-integer N; tiles with N < 4 beside N >= 4, and tiles without any N < 4 (not at 16 x 16: one tile cannot
    hold zero normals and be left early).  On smaller images: taps outside the image wherever a pixel looks for history."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = size
    params = SHAPES_PARAMS if name == "shapes" else PARAM_SETS[name]
    calls = run_reference(dn, w, h, SCHEDULE, mats, params)
    nears = []
    for call, (frame, (new, iv, (near, near_n)), cen, hist) in enumerate(calls):
        near_caps(near, near_n, call)
        nears.append((int(near.sum()), int(near_n.sum())))
        N = new[0, ..., 3]
        if frame[4] in (None, "out"):
            assert (N[cen["hit"]] == 1).all()                                        # no history anywhere
    t = _populations(calls, w, h)
    hits = max(1, t["hits"])
    print("synthetic %s %dx%d: near / near_n per call %s; over %d hits: zero-normal hits alone without history %d, taps outside %.3f, plane-rejected %.3f, "
          "normal-rejected %.3f, non-integer N %.3f; tiles mixed %d, left early %d; perspective: behind %.3f, in front and found %.3f" % (
              name, w, h, nears, t["hits"], t["zero_lonely"], t["partial"] / hits, t["plane"] / hits, t["normal"] / hits, t["nonint"] / hits, t["mixed"],
              t["quiet"], t["behind"], t["front_found"]))
    ntol = params.get("normal_tol", 0.9)
    if w * h >= 255:
        assert t["zero_lonely"] > 0 and t["partial"] > 0
        assert t["behind"] >= 0.10 and t["front_found"] >= 0.10
        assert t["plane"] >= 0.03 * hits
        assert t["normal"] >= 0.03 * hits or ntol <= -1.0                            # (normal_tol = -1 rejects no normal with a length)
        if params["max_history"] > 1:
            assert t["nonint"] > 0
        if params["max_history"] >= 4:
            assert t["mixed"] > 0
            assert t["quiet"] > 0 or (w <= 16 and h <= 16)                           # (one tile cannot hold zero normals and be left early)
    elif t["hits"]:
        assert t["partial"] > 0


@pytest.mark.parametrize("size", IDENTITY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_identity_schedule_counts_exactly(cornell, size):
    """The N-exactly-4 schedule on the reference: ortho_vp(w, h, 0, 0) at powers of two, one stage, six calls: N is exactly 1 .. 6 on every hit with a normal in
    float64 and in the float32 mode, 1 on the zero normals, 0 on misses and emitters; nothing is `near`; and in the call with N = 4 the two
    forms of V_0 are far apart on at least half of the compared pixels."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = size
    for dtype in (np.float64, np.float32):
        hist = None
        for call, (colour, g, X, vp, cam) in enumerate(schedule_frames(w, h, IDENTITY_SCHEDULE)):
            new, iv, (near, near_n) = dn.reference_temporal(colour, g[0], g[1], X, hist, vp, material_ids=mats, near_parts=True, dtype=dtype)
            cen = census(dn, g, X, hist, vp, mats)
            N = new[0, ..., 3]
            normal = cen["hit"] & ~cen["zero"]
            assert normal.any() and (N[normal] == call + 1).all() and (N[cen["zero"]] == 1).all() and (N[~cen["hit"]] == 0).all()
            assert not near.any() and near_n.sum() == (normal.sum() if call == 3 else 0)
            if call == 3 and dtype is np.float64:
                temporal, spatial = iv[..., 3], spatial_form(dn, new, {})
                far = np.abs(temporal - spatial) > 1e-3 * np.abs(temporal) + 1e-9
                print("identity %dx%d: the two forms of V_0 differ on %.3f of the %d hits with N = 4" % (w, h, far[normal].mean(), normal.sum()))
                assert far[normal].mean() >= 0.5
            hist = new


def test_one_state_schedule_stays_under_the_caps(cornell):
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = ONE_STATE_SHAPE
    for call, (frame, (new, iv, (near, near_n)), cen, hist) in enumerate(run_reference(dn, w, h, ONE_STATE_SCHEDULE, mats, {})):
        near_caps(near, near_n, call)
        assert hist is None or cen["found"].mean() > 0.1


def test_parameter_sets_differ_in_every_field():
    from toyraygun_amd import denoise as dn
    fields = [k for k in dn._TEMPORAL_DEFAULTS if k != "iterations"]
    sets = list(PARAM_SETS.values())
    assert len(sets) >= 3
    for k in fields:
        vals = [s[k] for s in sets]
        if k == "demodulate":
            assert set(vals) == {0, 1}
            continue
        assert len(set(vals)) == len(vals) and dn._TEMPORAL_DEFAULTS[k] not in vals, k
    assert any(s["alpha"] == s["alpha_moments"] == 1.0 and s["max_history"] == 1 for s in sets)
    assert any(s["normal_tol"] == -1.0 and s["sigma_normal"] == 0.0 for s in sets)


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_every_varied_parameter_shows(cornell, name):
    """The parameter sets on the reference chain at 17 x 33: setting any one varied field back to its default moves some compared pixel of some call by
    more than that call's bar -- but for the fields of INVISIBLE, which the definition itself hides in that set (and those stay hidden)."""
    from toyraygun_amd import denoise as dn
    mats = cornell.buffers()["material_ids"]
    w, h = 17, 33
    params = PARAM_SETS[name]
    prev, seen = None, set()
    for frame in schedule_frames(w, h, SCHEDULE):
        R = step_reference(dn, frame, prev, mats, params)
        seen |= visible_fields(dn, R, frame, prev, mats, params)
        prev = R["new"]
    varied = set(varied_fields(dn, params))
    print("synthetic %s: varied %s, seen %s" % (name, sorted(varied), sorted(seen)))
    assert varied >= set(params) - {"demodulate"} and seen == varied - INVISIBLE[name]
