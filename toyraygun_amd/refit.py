"""Refit of a loaded scene from new vertex positions (include/trg_refit.h).

    ctx.load_scene(positions, normals, colors, indices, material_ids)
    refit_scene(ctx, moved_positions, moved_normals, indices)     # same topology; normals may be None: the loaded ones stay
    info = refit_last(ctx)                                        # {"path": DEVICE | REBUILD, "ms": ..., "area_ratio": ..., ...}

`ctx` is a capi.Context or a capi.Group (every context of a group refits its own copy).  A scene traversed from HBM is refitted on the device;
a scene small enough for the LDS tier is rebuilt by the host builder (microseconds).  A refused call -- an index out of range, a coordinate that
is not finite, a quad leaf or a box leaf of the loaded tree that the moved vertices no longer form -- raises capi.TrgError and leaves the loaded
scene as it was; the text names the first offending triangle.

The context's refit scratch belongs to the context: ctx.close() frees it, release(ctx) frees it earlier.
"""
import ctypes as C

import numpy as np

from . import capi

NONE, DEVICE, REBUILD = 0, 1, 2
PATH_NAMES = {NONE: "none", DEVICE: "device", REBUILD: "rebuild"}


class Info(C.Structure):
    _fields_ = [("path", C.c_uint32), ("n_records", C.c_uint32), ("n_quads", C.c_uint32), ("n_boxes", C.c_uint32), ("n_nodes", C.c_uint32),
                ("n_nodes_box", C.c_uint32), ("passes", C.c_uint32), ("reserved", C.c_uint32), ("lo", C.c_float * 3), ("hi", C.c_float * 3),
                ("pad", C.c_float), ("reserved_f", C.c_float), ("ms", C.c_double), ("area_ratio", C.c_double), ("area_ratio_box", C.c_double)]


_P = C.c_void_p
_U = C.c_uint32
_SYMBOLS = [
    ("trg_refit_scene", C.c_int, [_P, _P, _P, _P, _U, _U]),
    ("trg_refit_last", C.c_int, [_P, C.POINTER(Info)]),
    ("trg_refit_release", C.c_int, [_P]),
    ("trg_group_refit_scene", C.c_int, [_P, _P, _P, _P, _U, _U]),
]
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]

_bound = None


def load():
    """The library handle of capi.load() with the symbols of include/trg_refit.h bound.  No fallback: a library without them is an error."""
    global _bound
    L = capi.load()
    if _bound is not L:
        for name, res, args in _SYMBOLS:
            fn = getattr(L, name)   # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def _buffers(positions, normals, indices):
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    if idx.shape[0] % 3:
        raise ValueError("expected 3 indices per triangle")
    nt = idx.shape[0] // 3
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nrm.shape[0] != 3 * nt:
            raise ValueError("expected 3*n_tris normals for %d triangles" % nt)
    return pos, nrm, idx, nt


def refit_scene(ctx, positions, normals, indices, n_tris=None):
    """trg_refit_scene / trg_group_refit_scene.  n_tris: the count to pass (default: len(indices) / 3)."""
    L = load()
    pos, nrm, idx, nt = _buffers(positions, normals, indices)
    nt = nt if n_tris is None else int(n_tris)
    if isinstance(ctx, capi.Group):
        rc = L.trg_group_refit_scene(ctx.g, capi._ptr(pos), capi._ptr(nrm), capi._ptr(idx), pos.shape[0], nt)
        if rc != capi.OK:
            msg = ""
            for r in range(ctx.n):   # the text is the refusing context's
                msg = msg or (L.trg_last_error(L.trg_group_ctx(ctx.g, r)) or b"").decode()
            raise capi.TrgError(rc, msg)
        return
    ctx._chk(L.trg_refit_scene(ctx.h_ctx, capi._ptr(pos), capi._ptr(nrm), capi._ptr(idx), pos.shape[0], nt))


def refit_last(ctx, rank=0):
    """trg_refit_info of the context's (a group: of rank `rank`'s) last successful refit, as a dict; "path_name" names the path."""
    L = load()
    h = L.trg_group_ctx(ctx.g, rank) if isinstance(ctx, capi.Group) else ctx.h_ctx
    info = Info()
    rc = L.trg_refit_last(h, C.byref(info))
    if rc != capi.OK:
        raise capi.TrgError(rc, "trg_refit_last")
    out = {f: getattr(info, f) for f, _ in Info._fields_ if not f.startswith("reserved")}
    out["lo"], out["hi"] = tuple(info.lo), tuple(info.hi)
    out["path_name"] = PATH_NAMES.get(info.path, "?")
    return out


def release(ctx):
    """Frees the refit scratch of a context, or of every context of a group."""
    L = load()
    if isinstance(ctx, capi.Group):
        for r in range(ctx.n):
            L.trg_refit_release(L.trg_group_ctx(ctx.g, r))
    elif getattr(ctx, "h_ctx", None):
        L.trg_refit_release(ctx.h_ctx)
