"""What refit.py, pose.py, skin.py and morph.py share: binding a module's symbols, the geometry arguments, the call on a context or on a group, the
calls every binding has (include/trg_pose.h, trg_skin.h and trg_morph.h keep ONE protocol: DESIGN.md, "Bindings") and the normal transform of the
references.  `unit` is "pose", "skin" or "morph": the word in the C names, in the texts and in the attribute that remembers the bound counts."""
import ctypes as C

import numpy as np

from . import capi

_bound = {}   # id of a module's symbol list -> the library handle it was bound on


def load(symbols):
    """The library handle of capi.load() with `symbols` bound.  No fallback: a library without them is an error."""
    L = capi.load()
    if _bound.get(id(symbols)) is not L:
        for name, res, args in symbols:
            fn = getattr(L, name)   # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound[id(symbols)] = L
    return L


def geometry(positions, normals, indices, n_tris=None, indices_text="expected 3 indices per triangle"):
    """(positions [n_verts, 3] float32, normals [3 n_tris, 3] float32 or None, indices [3 n_tris] uint32, n_tris), contiguous.  n_tris: the count to
    pass (default: len(indices) / 3)."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    if idx.shape[0] % 3:
        raise ValueError(indices_text)
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nrm.shape[0] != idx.shape[0]:
            raise ValueError("expected 3*n_tris normals for %d triangles" % (idx.shape[0] // 3))
    return pos, nrm, idx, idx.shape[0] // 3 if n_tris is None else int(n_tris)


def _group_chk(L, g, rc):
    if rc != capi.OK:
        msg = ""
        for r in range(g.n):   # the text is the refusing context's
            msg = msg or (L.trg_last_error(L.trg_group_ctx(g.g, r)) or b"").decode()
        raise capi.TrgError(rc, msg)


def call(L, ctx, name, *args):
    """trg_<name> on a context, trg_group_<name> on a group; a refusal raises capi.TrgError."""
    if isinstance(ctx, capi.Group):
        _group_chk(L, ctx, getattr(L, "trg_group_" + name)(ctx.g, *args))
    else:
        ctx._chk(getattr(L, "trg_" + name)(ctx.h_ctx, *args))


def remember(ctx, unit, counts):
    """The C calls after a bind carry no counts: what was bound -- (n_verts, n_tris, ..., has normals), None: nothing -- is remembered on `ctx`, so
    that apply and read can size and check their host arrays."""
    setattr(ctx, "_%s_counts" % unit, counts)


def counts(ctx, unit):
    bound = getattr(ctx, "_%s_counts" % unit, None)
    if bound is None:
        raise capi.TrgError(capi.ERR_INVALID, "%s: nothing bound (trg_%s_bind, through bind of this module, first)" % (unit, unit))
    return bound


def buffers(L, ctx, unit):
    out = [C.c_void_p() for _ in range(5)]
    ctx._chk(getattr(L, "trg_%s_buffers" % unit)(ctx.h_ctx, *[C.byref(p) for p in out]))
    return dict(zip(("pos", "nrm", "idx", "prev_pos", "prev_nrm"), (p.value for p in out)))


def read(L, ctx, unit, n_verts, n_tris, normals):
    bound = counts(ctx, unit)
    nv, nt, has_nrm = bound[0], bound[1], bound[-1]
    if (n_verts is not None and n_verts != nv) or (n_tris is not None and n_tris != nt):
        raise ValueError("the binding has %d vertices and %d triangles" % (nv, nt))
    pos = np.empty((nv, 3), np.float32)
    nrm = np.empty((3 * nt, 3), np.float32) if normals and has_nrm else None
    ctx._chk(getattr(L, "trg_%s_read" % unit)(ctx.h_ctx, capi._ptr(pos), capi._ptr(nrm)))
    return pos, nrm


def release(L, ctx, unit):
    """trg_<unit>_release of a context, or of every context of a group ("refit": the whole scratch)."""
    fn = getattr(L, "trg_%s_release" % unit)
    if isinstance(ctx, capi.Group):
        for r in range(ctx.n):
            fn(L.trg_group_ctx(ctx.g, r))
    elif getattr(ctx, "h_ctx", None):
        fn(ctx.h_ctx)


def transform_normals(A, nrm, of=None):
    """Normals [n, 3] float32 under the linear parts A [m, 3, 3] float32, every operation rounded to float32 in the order trg_pose_math.h states it:
         C_ij = p q - r s (the cofactors of A);  det = (a00 C00 + a01 C01) + a02 C02;  s = -1 if det < 0 else +1
         n'  = s ((C_i0 nx + C_i1 ny) + C_i2 nz);  len = sqrt((n'x n'x + n'y n'y) + n'z n'z)
         the result is n' / len if len > 0 and finite, else the normal as it came.
    Normal k takes matrix of[k] (of None: m = n and its own).  Called inside the caller's np.errstate."""
    f = np.float32

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
    if of is not None:
        Cm, sign = Cm[of], sign[of]
    v = np.stack([sign * ((Cm[:, i, 0] * nrm[:, 0] + Cm[:, i, 1] * nrm[:, 1]) + Cm[:, i, 2] * nrm[:, 2]) for i in range(3)], axis=1)
    length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    ok = (length > 0) & np.isfinite(length)
    out = np.where(ok[:, None], v / np.where(ok, length, f(1))[:, None], nrm)
    assert out.dtype == f and v.dtype == f and length.dtype == f
    return np.ascontiguousarray(out)
