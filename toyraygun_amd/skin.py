"""Linear-blend skinning of a loaded scene on the device (include/trg_skin.h).

    ctx.load_scene(positions, normals, colors, indices, material_ids)
    bind(ctx, positions, normals, indices, bone_ids, weights, n_bones)   # the REST geometry; per vertex four bone ids and four weights
    apply(ctx, bones)                                    # [n_bones, 12] float32, row-major [A | t]: 48 bytes per bone go to the device
    pos, nrm = read(ctx)                                 # the current pose, from the device (the counts are remembered from bind)

`ctx` is a capi.Context; bind and apply also take a capi.Group (every context of a group keeps its own copy).  A refused call raises capi.TrgError
and leaves the scene, the current and the previous pose as they were.  skin_reference is the arithmetic of toyraygun_amd/csrc/trg_skin_math.h in
numpy float32, written from that header's text: trg_skin_read must equal it bit for bit.  Weights are used as given; nothing normalises them.
"""
import ctypes as C

import numpy as np

from . import capi
from .pose import _group_chk

_P = C.c_void_p
_U = C.c_uint32
_PP = C.POINTER(C.c_void_p)
_SYMBOLS = [
    ("trg_skin_bind", C.c_int, [_P, _P, _P, _P, _U, _U, _P, _P, _U]),
    ("trg_skin_apply", C.c_int, [_P, _P]),
    ("trg_skin_read", C.c_int, [_P, _P, _P]),
    ("trg_skin_buffers", C.c_int, [_P, _PP, _PP, _PP, _PP, _PP]),
    ("trg_skin_release", C.c_int, [_P]),
    ("trg_group_skin_bind", C.c_int, [_P, _P, _P, _P, _U, _U, _P, _P, _U]),
    ("trg_group_skin_apply", C.c_int, [_P, _P]),
]
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]

_bound = None


def load():
    """The library handle of capi.load() with the symbols of include/trg_skin.h bound.  No fallback: a library without them is an error."""
    global _bound
    L = capi.load()
    if _bound is not L:
        for name, res, args in _SYMBOLS:
            fn = getattr(L, name)   # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def bind(ctx, positions, normals, indices, bone_ids, weights, n_bones, n_tris=None):
    """trg_skin_bind / trg_group_skin_bind.  bone_ids [n_verts, 4] uint32, weights [n_verts, 4] float32.  n_tris: the count to pass (default:
    len(indices) / 3)."""
    L = load()
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    ids = np.ascontiguousarray(bone_ids, np.uint32).reshape(-1, 4)
    wts = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
    if idx.shape[0] % 3:
        raise ValueError("expected 3 indices per triangle")
    if ids.shape[0] != pos.shape[0] or wts.shape[0] != pos.shape[0]:
        raise ValueError("expected four bone ids and four weights for each of %d vertices" % pos.shape[0])
    nt = idx.shape[0] // 3 if n_tris is None else int(n_tris)
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nrm.shape[0] != idx.shape[0]:
            raise ValueError("expected 3*n_tris normals for %d triangles" % (idx.shape[0] // 3))
    args = (capi._ptr(pos), capi._ptr(nrm), capi._ptr(idx), pos.shape[0], nt, capi._ptr(ids), capi._ptr(wts), int(n_bones))
    ctx._skin_counts = None
    if isinstance(ctx, capi.Group):
        _group_chk(L, ctx, L.trg_group_skin_bind(ctx.g, *args))
    else:
        ctx._chk(L.trg_skin_bind(ctx.h_ctx, *args))
    # the C calls that follow carry no counts: what was bound is remembered here, so that apply and read can size and check their host arrays
    ctx._skin_counts = (pos.shape[0], nt, int(n_bones), nrm is not None)


def _counts(ctx):
    counts = getattr(ctx, "_skin_counts", None)
    if counts is None:
        raise capi.TrgError(capi.ERR_INVALID, "skin: nothing bound (trg_skin_bind, through bind of this module, first)")
    return counts


def apply(ctx, bones):
    """trg_skin_apply / trg_group_skin_apply: [n_bones, 12] (or [n_bones, 3, 4]) float32, one row per bound bone (ValueError otherwise: the C call
    reads n_bones x 12 floats)."""
    L = load()
    x = np.ascontiguousarray(bones, np.float32).reshape(-1, 12)
    n_bones = _counts(ctx)[2]
    if x.shape[0] != n_bones:
        raise ValueError("expected %d bones, as bound, got %d" % (n_bones, x.shape[0]))
    if isinstance(ctx, capi.Group):
        _group_chk(L, ctx, L.trg_group_skin_apply(ctx.g, capi._ptr(x)))
    else:
        ctx._chk(L.trg_skin_apply(ctx.h_ctx, capi._ptr(x)))


def buffers(ctx):
    """trg_skin_buffers: dict of device addresses (int, or None) -- pos, nrm, idx, prev_pos, prev_nrm."""
    L = load()
    out = [C.c_void_p() for _ in range(5)]
    ctx._chk(L.trg_skin_buffers(ctx.h_ctx, *[C.byref(p) for p in out]))
    return dict(zip(("pos", "nrm", "idx", "prev_pos", "prev_nrm"), (p.value for p in out)))


def read(ctx, n_verts=None, n_tris=None, normals=True):
    """trg_skin_read: (positions [n_verts, 3], normals [3 n_tris, 3] or None) of the current pose.  The arrays are sized by the counts bind
    remembered; n_verts / n_tris, if given, must be those (ValueError)."""
    L = load()
    nv, nt, _, has_nrm = _counts(ctx)
    if (n_verts is not None and n_verts != nv) or (n_tris is not None and n_tris != nt):
        raise ValueError("the binding has %d vertices and %d triangles" % (nv, nt))
    normals = normals and has_nrm
    pos = np.empty((nv, 3), np.float32)
    nrm = np.empty((3 * nt, 3), np.float32) if normals else None
    ctx._chk(L.trg_skin_read(ctx.h_ctx, capi._ptr(pos), capi._ptr(nrm)))
    return pos, nrm


def release(ctx):
    """Frees the binding of a context, or of every context of a group (the refit scratch stays: refit.release)."""
    L = load()
    ctx._skin_counts = None
    if isinstance(ctx, capi.Group):
        for r in range(ctx.n):
            L.trg_skin_release(L.trg_group_ctx(ctx.g, r))
    elif getattr(ctx, "h_ctx", None):
        L.trg_skin_release(ctx.h_ctx)


def check_binding(bone_ids, weights, n_bones):
    """The validators of trg_skin_bind: None, or (vertex, what) of the first offending vertex -- an id >= n_bones (all ids are looked at first, as
    the C call does), then per vertex a weight that is negative or not finite, or a sum, formed in double, further than 1e-4 from 1."""
    ids = np.asarray(bone_ids).reshape(-1, 4)
    wts = np.asarray(weights, np.float32).reshape(-1, 4)
    bad = np.flatnonzero((ids.astype(np.int64) >= n_bones).any(1) | (ids.astype(np.int64) < 0).any(1))
    if bad.size:
        return int(bad[0]), "id"
    with np.errstate(all="ignore"):
        w_bad = ~(np.isfinite(wts) & (wts >= 0)).all(1)
        s_bad = ~(np.abs(wts.astype(np.float64).sum(1) - 1.0) <= 1e-4)
    bad = np.flatnonzero(w_bad | s_bad)
    if bad.size:
        return int(bad[0]), "weight" if w_bad[bad[0]] else "sum"
    return None


def skin_reference(positions, normals, indices, bone_ids, weights, bones):
    """The skinned (positions, normals) in numpy float32, every operation rounded to float32 in the order include/trg_skin.h's arithmetic states it:
         M[k] = ((w0 B_b0[k] + w1 B_b1[k]) + w2 B_b2[k]) + w3 B_b3[k]         k = 0..11, per vertex; B row-major [A | t]
         x'   = ((M0 x + M1 y) + M2 z) + M3                                    per row of M
         C_ij = p q - r s (the cofactors of M's linear part);  det = (a00 C00 + a01 C01) + a02 C02;  s = -1 if det < 0 else +1
         n'   = s ((C_i0 nx + C_i1 ny) + C_i2 nz);  len = sqrt((n'x n'x + n'y n'y) + n'z n'z)
         the skinned normal is n' / len if len > 0 and finite, else the rest normal.
    Every vertex is skinned, named by a triangle or not; corner c of triangle t takes the matrix of vertex indices[3 t + c].  normals may be None
    (None is returned for them)."""
    f = np.float32
    pos = np.ascontiguousarray(positions, f).reshape(-1, 3)
    B = np.ascontiguousarray(bones, f).reshape(-1, 12)
    ids = np.asarray(bone_ids, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(weights, f).reshape(-1, 4)
    if ids.shape[0] != pos.shape[0] or w.shape[0] != pos.shape[0]:
        raise ValueError("expected four ids and four weights per vertex")
    if ids.min() < 0 or ids.max() >= B.shape[0]:
        raise ValueError("a bone id out of range")
    with np.errstate(all="ignore"):
        t0 = w[:, 0:1] * B[ids[:, 0]]
        t1 = w[:, 1:2] * B[ids[:, 1]]
        t2 = w[:, 2:3] * B[ids[:, 2]]
        t3 = w[:, 3:4] * B[ids[:, 3]]
        M = (((t0 + t1) + t2) + t3).reshape(-1, 3, 4)
        assert M.dtype == f
        cols = []
        for i in range(3):
            a, b, c = M[:, i, 0] * pos[:, 0], M[:, i, 1] * pos[:, 1], M[:, i, 2] * pos[:, 2]
            cols.append(((a + b) + c) + M[:, i, 3])
        out = np.ascontiguousarray(np.stack(cols, axis=1))
        assert out.dtype == f
        if normals is None:
            return out, None
        nrm = np.ascontiguousarray(normals, f).reshape(-1, 3)
        idx = np.asarray(indices, np.int64).reshape(-1)
        if idx.shape[0] != nrm.shape[0] or idx.min() < 0 or idx.max() >= pos.shape[0]:
            raise ValueError("expected one in-range index per corner normal")
        A = M[idx][:, :, :3]                                               # the corner's own vertex

        def cof(p_, q_, r_, s_):
            return A[:, p_[0], p_[1]] * A[:, q_[0], q_[1]] - A[:, r_[0], r_[1]] * A[:, s_[0], s_[1]]
        Cm = np.empty((A.shape[0], 3, 3), f)
        Cm[:, 0, 0] = cof((1, 1), (2, 2), (1, 2), (2, 1))
        Cm[:, 0, 1] = cof((1, 2), (2, 0), (1, 0), (2, 2))
        Cm[:, 0, 2] = cof((1, 0), (2, 1), (1, 1), (2, 0))
        Cm[:, 1, 0] = cof((0, 2), (2, 1), (0, 1), (2, 2))
        Cm[:, 1, 1] = cof((0, 0), (2, 2), (0, 2), (2, 0))
        Cm[:, 1, 2] = cof((0, 1), (2, 0), (0, 0), (2, 1))
        Cm[:, 2, 0] = cof((0, 1), (1, 2), (0, 2), (1, 1))
        Cm[:, 2, 1] = cof((0, 2), (1, 0), (0, 0), (1, 2))
        Cm[:, 2, 2] = cof((0, 0), (1, 1), (0, 1), (1, 0))
        det = (A[:, 0, 0] * Cm[:, 0, 0] + A[:, 0, 1] * Cm[:, 0, 1]) + A[:, 0, 2] * Cm[:, 0, 2]
        sign = np.where(det < 0, f(-1), f(1)).astype(f)
        v = np.stack([sign * ((Cm[:, i, 0] * nrm[:, 0] + Cm[:, i, 1] * nrm[:, 1]) + Cm[:, i, 2] * nrm[:, 2]) for i in range(3)], axis=1)
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ok = (length > 0) & np.isfinite(length)
        skinned = np.where(ok[:, None], v / np.where(ok, length, f(1))[:, None], nrm)
        assert skinned.dtype == f and v.dtype == f and length.dtype == f
    return out, np.ascontiguousarray(skinned)
