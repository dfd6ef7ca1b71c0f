"""A second reading of include/trg_denoise.h: trg_denoise and trg_denoise_variance written once more straight from the header's text, one pixel
at a time and one tap at a time in plain Python floats (float64).  It shares nothing with toyraygun_amd/denoise.py -- no helper, no numpy
arithmetic (numpy only carries the images in and out) -- so a formula that module misread is not misread here in the same way.
tests/test_denoise_literal_host.py compares the two.

Constants: the sigmas and the two 1e-3 (the albedo clamp, the floor of w_l's denominator) are taken as the fp32 values the device holds, the 1e-4
of w_c and the 1e-6 of w_z as written -- the conventions of the vectorised reference, so that the two differ in summation order only."""
import math
import struct

import numpy as np

MAX_ITERATIONS = 6
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)      # h of the header, offsets -2 .. 2
B3x3 = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)                             # b of GV, offsets -1 .. 1
EMISSIVE = 2                                                         # TRG_MATERIAL_EMISSIVE


def _f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


CLAMP = _f32(1e-3)


def _lum(c):
    return 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2]


class _Guides:
    """n_p, z_p (negative for a miss AND for a first-hit emitter), max(a_p, 1e-3) per pixel as nested lists [y][x]."""

    def __init__(self, g0, g1, material_ids):
        g0 = np.asarray(g0, np.float32)
        g1 = np.asarray(g1, np.float32)
        self.h, self.w = g0.shape[:2]
        prim = np.ascontiguousarray(g1[..., 3]).view(np.int32).tolist()
        mats = None if material_ids is None else [int(m) for m in np.asarray(material_ids).reshape(-1)]
        g0l, g1l = g0.tolist(), g1.tolist()
        self.n = [[tuple(g0l[y][x][:3]) for x in range(self.w)] for y in range(self.h)]
        self.z = [[g0l[y][x][3] for x in range(self.w)] for y in range(self.h)]
        self.a = [[tuple(max(v, CLAMP) for v in g1l[y][x][:3]) for x in range(self.w)] for y in range(self.h)]
        if mats is not None:
            for y in range(self.h):
                for x in range(self.w):
                    k = prim[y][x]
                    if 0 <= k < len(mats) and mats[k] == EMISSIVE:
                        self.z[y][x] = -1.0
        self.miss = [[self.z[y][x] < 0 for x in range(self.w)] for y in range(self.h)]
        self.g = [[self._gradient(x, y) for x in range(self.w)] for y in range(self.h)]

    def inside(self, x, y):
        return 0 <= x < self.w and 0 <= y < self.h

    def _gradient(self, x, y):
        """g_p: forward difference where the forward neighbour is inside and not a miss, else backward likewise, else 0; per axis."""
        z = self.z
        d = []
        for ax, ay in ((1, 0), (0, 1)):
            if self.inside(x + ax, y + ay) and not z[y + ay][x + ax] < 0:
                d.append(z[y + ay][x + ax] - z[y][x])
            elif self.inside(x - ax, y - ay) and not z[y - ay][x - ax] < 0:
                d.append(z[y][x] - z[y - ay][x - ax])
            else:
                d.append(0.0)
        return math.sqrt(d[0] * d[0] + d[1] * d[1])

    def geometry(self, x, y, qx, qy, s, dx, dy, sigma_normal, sigma_depth):
        """w_n * w_z * w_id of the tap q = p + s (dx, dy), which lies inside the image."""
        if self.miss[qy][qx]:
            return 0.0
        n, m = self.n[y][x], self.n[qy][qx]
        dot = n[0] * m[0] + n[1] * m[1] + n[2] * m[2]
        if dot <= 0:
            return 0.0
        w_n = dot ** sigma_normal
        w_z = math.exp(-abs(self.z[y][x] - self.z[qy][qx]) / (sigma_depth * (self.g[y][x] * s * math.sqrt(dx * dx + dy * dy) + 1e-6)))
        return w_n * w_z


def _params(defaults, params, kw):
    q = dict(defaults)
    q.update(params or {})
    q.update(kw)
    it = int(q["iterations"])
    if not 0 <= it <= MAX_ITERATIONS:
        raise ValueError("iterations must be 0..%d" % MAX_ITERATIONS)
    return q, it


def literal_denoise(color, g0, g1, params=None, material_ids=None, every=False, **kw):
    """trg_denoise.  Returns [h, w, 4] float64; with every=True a dict {N: result of N iterations} for N = 1 .. iterations (the iterations of a
    longer run are those of a shorter one; only step 3 of the header differs)."""
    q, it = _params(dict(iterations=5, sigma_color=4.0, sigma_normal=128.0, sigma_depth=1.0, demodulate=1), params, kw)
    color = np.asarray(color)
    if it == 0:
        return {} if every else color.astype(np.float64)
    sc, sn, sd = _f32(q["sigma_color"]), _f32(q["sigma_normal"]), _f32(q["sigma_depth"])
    demod = bool(q["demodulate"])
    G = _Guides(g0, g1, material_ids)
    w, h = G.w, G.h
    C = color.astype(np.float64).tolist()
    # 1. demodulation
    I = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            c = C[y][x][:3]
            if demod and not G.miss[y][x]:
                c = [c[k] / G.a[y][x][k] for k in range(3)]
            I[y][x] = tuple(c)
    results = {}
    for i in range(it):
        s = 2 ** i
        L = [[_lum(I[y][x]) for x in range(w)] for y in range(h)]
        J = [[None] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                if G.miss[y][x]:
                    J[y][x] = I[y][x]
                    continue
                # var_p over the 3 x 3 window at spacing 1, pixels inside the image, misses included
                window = [L[y + ey][x + ex] for ey in (-1, 0, 1) for ex in (-1, 0, 1) if G.inside(x + ex, y + ey)]
                mean = sum(window) / len(window)
                var = sum((l - mean) ** 2 for l in window) / len(window)
                p = I[y][x]
                acc, wsum = [0.0, 0.0, 0.0], 0.0
                for dy in (-2, -1, 0, 1, 2):
                    for dx in (-2, -1, 0, 1, 2):
                        qx, qy = x + s * dx, y + s * dy
                        if not G.inside(qx, qy):
                            continue
                        wg = G.geometry(x, y, qx, qy, s, dx, dy, sn, sd)
                        if wg == 0.0:
                            continue
                        t = I[qy][qx]
                        d2 = (p[0] - t[0]) ** 2 + (p[1] - t[1]) ** 2 + (p[2] - t[2]) ** 2
                        w_c = math.exp(-d2 / (sc * sc * (var + 1e-4)))
                        wt = H5[dx + 2] * H5[dy + 2] * wg * w_c
                        acc[0] += wt * t[0]; acc[1] += wt * t[1]; acc[2] += wt * t[2]
                        wsum += wt
                J[y][x] = (acc[0] / wsum, acc[1] / wsum, acc[2] / wsum) if wsum > 0 else p
        I = J
        if every or i + 1 == it:
            # 3. remodulation; alpha is the input's
            out = color.astype(np.float64)
            for y in range(h):
                for x in range(w):
                    c = I[y][x]
                    if demod and not G.miss[y][x]:
                        c = [c[k] * G.a[y][x][k] for k in range(3)]
                    out[y, x, :3] = c
            results[i + 1] = out
    return results if every else results[it]


def literal_denoise_variance(h1, h2, g0, g1, params=None, material_ids=None, every=False, **kw):
    """trg_denoise_variance.  Returns ([h, w, 4], V_N [h, w]) float64; with every=True a dict {N: (out, V_N)} for N = 0 .. iterations."""
    q, it = _params(dict(iterations=5, sigma_lum=4.0, sigma_normal=128.0, sigma_depth=1.0, demodulate=1, prefilter=1), params, kw)
    sl, sn, sd = _f32(q["sigma_lum"]), _f32(q["sigma_normal"]), _f32(q["sigma_depth"])
    demod = bool(q["demodulate"])
    G = _Guides(g0, g1, material_ids)
    w, h = G.w, G.h
    h1, h2 = np.asarray(h1), np.asarray(h2)
    A, B = h1.astype(np.float64).tolist(), h2.astype(np.float64).tolist()
    # Start
    I = [[None] * w for _ in range(h)]
    V = [[0.0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            a, b = A[y][x][:3], B[y][x][:3]
            if demod and not G.miss[y][x]:
                a = [a[k] / G.a[y][x][k] for k in range(3)]
                b = [b[k] / G.a[y][x][k] for k in range(3)]
            I[y][x] = tuple(0.5 * (a[k] + b[k]) for k in range(3))
            V[y][x] = 0.0 if G.miss[y][x] else 0.25 * (_lum(a) - _lum(b)) ** 2
    # Prefilter: 7 x 7 at spacing 1, g = w_n w_z w_id, the V_0 on the right all un-prefiltered
    if q["prefilter"]:
        P = [row[:] for row in V]
        for y in range(h):
            for x in range(w):
                if G.miss[y][x]:
                    continue
                vs, gs = 0.0, 0.0
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        qx, qy = x + dx, y + dy
                        if not G.inside(qx, qy):
                            continue
                        g = G.geometry(x, y, qx, qy, 1, dx, dy, sn, sd)
                        vs += g * V[qy][qx]
                        gs += g
                if gs > 0:
                    P[y][x] = vs / gs
        V = P

    def finish(I, V, n):
        out = np.empty(h1.shape, np.float64)
        out[..., 3] = h1[..., 3]
        if n == 0:   # iterations == 0: the plain mean of the halves
            out[..., :3] = 0.5 * (h1[..., :3].astype(np.float64) + h2[..., :3].astype(np.float64))
        else:
            for y in range(h):
                for x in range(w):
                    c = I[y][x]
                    if demod and not G.miss[y][x]:
                        c = [c[k] * G.a[y][x][k] for k in range(3)]
                    out[y, x, :3] = c
        return out, np.array(V, np.float64).reshape(h, w)

    results = {0: finish(I, V, 0)}
    for i in range(it):
        s = 2 ** i
        L = [[_lum(I[y][x]) for x in range(w)] for y in range(h)]
        J = [[None] * w for _ in range(h)]
        U = [[0.0] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                if G.miss[y][x]:
                    J[y][x], U[y][x] = I[y][x], V[y][x]
                    continue
                # GV_i(p): 3 x 3 binomial over the pixels inside the image that are not misses
                vs, bs = 0.0, 0.0
                for ey in (-1, 0, 1):
                    for ex in (-1, 0, 1):
                        if G.inside(x + ex, y + ey) and not G.miss[y + ey][x + ex]:
                            b = B3x3[ex + 1] * B3x3[ey + 1]
                            vs += b * V[y + ey][x + ex]
                            bs += b
                gv = vs / bs
                den = sl * math.sqrt(max(0.0, gv)) + CLAMP
                si, sv, wsum = [0.0, 0.0, 0.0], 0.0, 0.0
                for dy in (-2, -1, 0, 1, 2):
                    for dx in (-2, -1, 0, 1, 2):
                        qx, qy = x + s * dx, y + s * dy
                        if not G.inside(qx, qy):
                            continue
                        wg = G.geometry(x, y, qx, qy, s, dx, dy, sn, sd)
                        if wg == 0.0:
                            continue
                        w_l = math.exp(-abs(L[y][x] - L[qy][qx]) / den)
                        wt = H5[dx + 2] * H5[dy + 2] * wg * w_l
                        t = I[qy][qx]
                        si[0] += wt * t[0]; si[1] += wt * t[1]; si[2] += wt * t[2]
                        sv += wt * wt * V[qy][qx]
                        wsum += wt
                if wsum > 0:
                    J[y][x], U[y][x] = (si[0] / wsum, si[1] / wsum, si[2] / wsum), sv / (wsum * wsum)
                else:
                    J[y][x], U[y][x] = I[y][x], V[y][x]
        I, V = J, U
        if every or i + 1 == it:
            results[i + 1] = finish(I, V, i + 1)
    return results if every else results[it]
