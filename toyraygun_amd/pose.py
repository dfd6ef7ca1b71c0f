"""Poses of a loaded scene on the device (include/trg_pose.h).

    ctx.load_scene(positions, normals, colors, indices, material_ids)
    bind(ctx, positions, normals, indices, first)        # the REST geometry; object j is triangles [first[j], first[j + 1])
    apply(ctx, xforms)                                   # [n_objects, 12] float32, row-major [A | t]: 48 bytes per object go to the device
    pos, nrm = read(ctx)                                 # the current pose, from the device (the counts are remembered from bind)
    refit_scene_device(ctx, pos_t, nrm_t, idx_t)         # torch tensors on the context's device: trg_refit_scene without the upload

`ctx` is a capi.Context; bind and apply also take a capi.Group (every context of a group keeps its own copy).  A refused call raises capi.TrgError
and leaves the scene, the current and the previous pose as they were.  pose_reference is the arithmetic of toyraygun_amd/csrc/trg_pose_math.h in
numpy float32, written from that header's text: trg_pose_read must equal it bit for bit.
"""
import ctypes as C

import numpy as np

from . import _binding, capi

_P = C.c_void_p
_U = C.c_uint32
_PP = C.POINTER(C.c_void_p)
_SYMBOLS = [
    ("trg_refit_scene_device", C.c_int, [_P, _P, _P, _P, _U, _U]),
    ("trg_pose_bind", C.c_int, [_P, _P, _P, _P, _U, _U, _P, _U]),
    ("trg_pose_apply", C.c_int, [_P, _P]),
    ("trg_pose_read", C.c_int, [_P, _P, _P]),
    ("trg_pose_buffers", C.c_int, [_P, _PP, _PP, _PP, _PP, _PP]),
    ("trg_pose_release", C.c_int, [_P]),
    ("trg_group_pose_bind", C.c_int, [_P, _P, _P, _P, _U, _U, _P, _U]),
    ("trg_group_pose_apply", C.c_int, [_P, _P]),
]
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]


def load():
    """The library handle of capi.load() with the symbols of include/trg_pose.h bound.  No fallback: a library without them is an error."""
    return _binding.load(_SYMBOLS)


def _tensor(t, what, dtypes, device):
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch tensor, got %s" % (what, type(t).__name__))
    if t.device.type != "cuda" or (t.device.index or 0) != device:
        raise ValueError("%s: the tensor is on %s, the context on device %d" % (what, t.device, device))
    if t.dtype not in dtypes:
        raise TypeError("%s: dtype %s, expected one of %s" % (what, t.dtype, ", ".join(str(d) for d in dtypes)))
    if not t.is_contiguous():
        raise ValueError("%s: the tensor is not contiguous" % what)
    return t


def refit_scene_device(ctx, positions, normals, indices):
    """trg_refit_scene_device: float32 positions [n_verts, 3], float32 normals [3 n_tris, 3] or None, int32 / uint32 indices [3 n_tris], contiguous
    torch tensors on the context's device, passed by data_ptr().  The caller's stream must have finished writing them."""
    import torch
    L = load()
    device = int(ctx.device)
    pos = _tensor(positions, "positions", (torch.float32,), device)
    idx = _tensor(indices, "indices", tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None), device)
    if pos.numel() % 3 or idx.numel() % 3:
        raise ValueError("expected 3 floats per vertex and 3 indices per triangle")
    nt = idx.numel() // 3
    nrm = None
    if normals is not None:
        nrm = _tensor(normals, "normals", (torch.float32,), device)
        if nrm.numel() != 9 * nt:
            raise ValueError("expected 3*n_tris normals for %d triangles" % nt)
    ctx._chk(L.trg_refit_scene_device(ctx.h_ctx, pos.data_ptr(), nrm.data_ptr() if nrm is not None else None, idx.data_ptr(), pos.numel() // 3, nt))


def bind(ctx, positions, normals, indices, first, n_tris=None):
    """trg_pose_bind / trg_group_pose_bind.  first: n_objects + 1 triangle numbers.  n_tris: the count to pass (default: len(indices) / 3)."""
    L = load()
    tab = np.ascontiguousarray(first, np.uint32).reshape(-1)
    text = "expected 3 indices per triangle and a table of n_objects + 1 entries"
    if tab.shape[0] < 2:
        raise ValueError(text)
    pos, nrm, idx, nt = _binding.geometry(positions, normals, indices, n_tris, text)
    _binding.remember(ctx, "pose", None)
    _binding.call(L, ctx, "pose_bind", capi._ptr(pos), capi._ptr(nrm), capi._ptr(idx), pos.shape[0], nt, capi._ptr(tab), tab.shape[0] - 1)
    _binding.remember(ctx, "pose", (pos.shape[0], nt, tab.shape[0] - 1, nrm is not None))


def apply(ctx, xforms):
    """trg_pose_apply / trg_group_pose_apply: [n_objects, 12] (or [n_objects, 3, 4]) float32, one row per bound object (ValueError otherwise:
    the C call reads n_objects x 12 floats)."""
    L = load()
    x = np.ascontiguousarray(xforms, np.float32).reshape(-1, 12)
    n_objects = _binding.counts(ctx, "pose")[2]
    if x.shape[0] != n_objects:
        raise ValueError("expected %d transforms, one per bound object, got %d" % (n_objects, x.shape[0]))
    _binding.call(L, ctx, "pose_apply", capi._ptr(x))


def buffers(ctx):
    """trg_pose_buffers: dict of device addresses (int, or None) -- pos, nrm, idx, prev_pos, prev_nrm."""
    return _binding.buffers(load(), ctx, "pose")


def read(ctx, n_verts=None, n_tris=None, normals=True):
    """trg_pose_read: (positions [n_verts, 3], normals [3 n_tris, 3] or None) of the current pose.  The arrays are sized by the counts bind
    remembered; n_verts / n_tris, if given, must be those (ValueError)."""
    return _binding.read(load(), ctx, "pose", n_verts, n_tris, normals)


def release(ctx):
    """Frees the binding of a context, or of every context of a group (the refit scratch stays: refit.release)."""
    _binding.remember(ctx, "pose", None)
    _binding.release(load(), ctx, "pose")


def object_maps(indices, first, n_verts):
    """(triangle -> object [n_tris], vertex -> object [n_verts], -1: named by no triangle) of a valid table; ValueError names what is wrong with
    an invalid one, by the rules of trg_pose_bind."""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    tab = np.asarray(first, np.int64).reshape(-1)
    nt = idx.shape[0]
    if tab[0] != 0:
        raise ValueError("object 0 begins at triangle %d" % tab[0])
    if (np.diff(tab) <= 0).any():
        raise ValueError("object %d: the table is not strictly ascending" % int(np.flatnonzero(np.diff(tab) <= 0)[0]))
    if tab[-1] != nt:
        raise ValueError("the table ends at triangle %d of %d" % (tab[-1], nt))
    tri_obj = np.repeat(np.arange(tab.shape[0] - 1), np.diff(tab))
    if idx.min() < 0 or idx.max() >= n_verts:
        raise ValueError("an index out of range")
    vtx_obj = np.full(n_verts, -1, np.int64)
    lo = np.full(n_verts, tab.shape[0], np.int64)
    np.minimum.at(lo, idx.reshape(-1), np.repeat(tri_obj, 3))
    np.maximum.at(vtx_obj, idx.reshape(-1), np.repeat(tri_obj, 3))
    shared = np.flatnonzero((vtx_obj >= 0) & (lo != vtx_obj))
    if shared.size:
        raise ValueError("vertex %d is named by triangles of two objects" % int(shared[0]))
    return tri_obj, vtx_obj


def pose_reference(positions, normals, indices, first, xforms):
    """The posed (positions, normals) in numpy float32, every operation rounded to float32 in the order include/trg_pose.h's arithmetic states it:
         x'  = ((m0 x + m1 y) + m2 z) + m3                                   per row of the row-major [A | t]
         C_ij = p q - r s (the cofactors of A);  det = (a00 C00 + a01 C01) + a02 C02;  s = -1 if det < 0 else +1
         n'  = s ((C_i0 nx + C_i1 ny) + C_i2 nz);  len = sqrt((n'x n'x + n'y n'y) + n'z n'z)
         the posed normal is n' / len if len > 0 and finite, else the rest normal.
    A vertex takes the transform of the one object whose triangles name it (none: it stays), a corner normal that of its triangle.  normals may be
    None (None is returned for them)."""
    f = np.float32
    pos = np.ascontiguousarray(positions, f).reshape(-1, 3)
    M = np.ascontiguousarray(xforms, f).reshape(-1, 3, 4)
    tri_obj, vtx_obj = object_maps(indices, first, pos.shape[0])
    if M.shape[0] != len(np.asarray(first).reshape(-1)) - 1:
        raise ValueError("expected one transform per object")
    with np.errstate(all="ignore"):
        out = pos.copy()
        moved = vtx_obj >= 0
        m = M[vtx_obj[moved]]
        p = pos[moved]
        cols = []
        for i in range(3):
            a, b, c = m[:, i, 0] * p[:, 0], m[:, i, 1] * p[:, 1], m[:, i, 2] * p[:, 2]
            cols.append(((a + b) + c) + m[:, i, 3])
        out[moved] = np.stack(cols, axis=1)
        assert out.dtype == f
        if normals is None:
            return out, None
        nrm = np.ascontiguousarray(normals, f).reshape(-1, 3)
        posed = _binding.transform_normals(M[:, :, :3], nrm, np.repeat(tri_obj, 3))   # the transform of the corner's triangle
    return out, posed
