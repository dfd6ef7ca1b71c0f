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

from . import _binding, capi

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


def load():
    """The library handle of capi.load() with the symbols of include/trg_refit.h bound.  No fallback: a library without them is an error."""
    return _binding.load(_SYMBOLS)


def refit_scene(ctx, positions, normals, indices, n_tris=None):
    """trg_refit_scene / trg_group_refit_scene.  n_tris: the count to pass (default: len(indices) / 3)."""
    L = load()
    pos, nrm, idx, nt = _binding.geometry(positions, normals, indices, n_tris)
    _binding.call(L, ctx, "refit_scene", capi._ptr(pos), capi._ptr(nrm), capi._ptr(idx), pos.shape[0], nt)


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
    _binding.release(load(), ctx, "refit")
