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

from . import _binding, capi

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


def load():
    """The library handle of capi.load() with the symbols of include/trg_skin.h bound.  No fallback: a library without them is an error."""
    return _binding.load(_SYMBOLS)


def bind(ctx, positions, normals, indices, bone_ids, weights, n_bones, n_tris=None):
    """trg_skin_bind / trg_group_skin_bind.  bone_ids [n_verts, 4] uint32, weights [n_verts, 4] float32.  n_tris: the count to pass (default:
    len(indices) / 3)."""
    L = load()
    pos, nrm, idx, nt = _binding.geometry(positions, normals, indices, n_tris)
    ids = np.ascontiguousarray(bone_ids, np.uint32).reshape(-1, 4)
    wts = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
    if ids.shape[0] != pos.shape[0] or wts.shape[0] != pos.shape[0]:
        raise ValueError("expected four bone ids and four weights for each of %d vertices" % pos.shape[0])
    _binding.remember(ctx, "skin", None)
    _binding.call(L, ctx, "skin_bind", capi._ptr(pos), capi._ptr(nrm), capi._ptr(idx), pos.shape[0], nt, capi._ptr(ids), capi._ptr(wts), int(n_bones))
    _binding.remember(ctx, "skin", (pos.shape[0], nt, int(n_bones), nrm is not None))


def apply(ctx, bones):
    """trg_skin_apply / trg_group_skin_apply: [n_bones, 12] (or [n_bones, 3, 4]) float32, one row per bound bone (ValueError otherwise: the C call
    reads n_bones x 12 floats)."""
    L = load()
    x = np.ascontiguousarray(bones, np.float32).reshape(-1, 12)
    n_bones = _binding.counts(ctx, "skin")[2]
    if x.shape[0] != n_bones:
        raise ValueError("expected %d bones, as bound, got %d" % (n_bones, x.shape[0]))
    _binding.call(L, ctx, "skin_apply", capi._ptr(x))


def buffers(ctx):
    """trg_skin_buffers: dict of device addresses (int, or None) -- pos, nrm, idx, prev_pos, prev_nrm."""
    return _binding.buffers(load(), ctx, "skin")


def read(ctx, n_verts=None, n_tris=None, normals=True):
    """trg_skin_read: (positions [n_verts, 3], normals [3 n_tris, 3] or None) of the current pose.  The arrays are sized by the counts bind
    remembered; n_verts / n_tris, if given, must be those (ValueError)."""
    return _binding.read(load(), ctx, "skin", n_verts, n_tris, normals)


def release(ctx):
    """Frees the binding of a context, or of every context of a group (the refit scratch stays: refit.release)."""
    _binding.remember(ctx, "skin", None)
    _binding.release(load(), ctx, "skin")


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
        skinned = _binding.transform_normals(M[idx][:, :, :3], nrm)         # the corner's own vertex
    return out, skinned
