"""Rigs: a keyframed joint forest evaluated on the device into the bones of the skin and morph bindings (include/trg_rig.h).

    bind(ctx, parent, key_first, keys, clock_of, n_clocks, inv_bind)   # once; independent of the loaded scene
    evaluate(ctx, clocks)                                # [n_clocks] float32: 4 bytes per clock go to the device, the bones stay there
    bones, world = read(ctx)                             # of the last evaluation, [n_joints, 12] float32 each
    skin_apply(ctx, clocks)                              # evaluate, then skin.apply from the rig's bones without the upload
    morph_apply(ctx, weights, clocks)                    # ... morph.apply (a binding with bones)
    skin_apply_device(ctx, bones) / morph_apply_device(ctx, weights, bones)   # bones the caller holds in a torch tensor on the context's device

`ctx` is a capi.Context; bind, skin_apply and morph_apply also take a capi.Group.  A refused call raises capi.TrgError and leaves the scene, the
current and the previous pose as they were.  rig_reference is the arithmetic of toyraygun_amd/csrc/trg_rig_math.h in numpy float32, written from
that header's text: read must equal it bit for bit.  check_rig restates trg_rig_bind's validators.
"""
import ctypes as C

import numpy as np

from . import _binding, capi, pose

_P = C.c_void_p
_U = C.c_uint32
_PP = C.POINTER(C.c_void_p)
_SYMBOLS = [
    ("trg_rig_bind", C.c_int, [_P, _P, _U, _P, _P, _U, _P, _U, _P]),
    ("trg_rig_evaluate", C.c_int, [_P, _P]),
    ("trg_rig_read", C.c_int, [_P, _P, _P]),
    ("trg_rig_buffers", C.c_int, [_P, _PP, _PP]),
    ("trg_rig_release", C.c_int, [_P]),
    ("trg_rig_skin_apply", C.c_int, [_P, _P]),
    ("trg_rig_morph_apply", C.c_int, [_P, _P, _P]),
    ("trg_rig_skin_apply_device", C.c_int, [_P, _P]),
    ("trg_rig_morph_apply_device", C.c_int, [_P, _P, _P]),
    ("trg_group_rig_bind", C.c_int, [_P, _P, _U, _P, _P, _U, _P, _U, _P]),
    ("trg_group_rig_skin_apply", C.c_int, [_P, _P]),
    ("trg_group_rig_morph_apply", C.c_int, [_P, _P, _P]),
]
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]
NO_PARENT = 0xFFFFFFFF
MAX_LEVELS = 64


def load():
    """The library handle of capi.load() with the symbols of include/trg_rig.h bound.  No fallback: a library without them is an error."""
    return _binding.load(_SYMBOLS)


def _tables(parent, key_first, keys, clock_of, inv_bind):
    par = np.ascontiguousarray(parent, np.uint32).reshape(-1)
    kf = np.ascontiguousarray(key_first, np.uint32).reshape(-1)
    ks = np.ascontiguousarray(keys, np.float32).reshape(-1, 12)
    co = np.ascontiguousarray(clock_of, np.uint32).reshape(-1)
    ib = None if inv_bind is None else np.ascontiguousarray(inv_bind, np.float32).reshape(-1, 12)
    if kf.shape[0] != par.shape[0] + 1 or co.shape[0] != par.shape[0] or (ib is not None and ib.shape[0] != par.shape[0]):
        raise ValueError("expected n_joints + 1 key ranges, n_joints clock ids and n_joints inverse binds for %d joints" % par.shape[0])
    return par, kf, ks, co, ib


def bind(ctx, parent, key_first, keys, clock_of, n_clocks, inv_bind=None, n_keys=None):
    """trg_rig_bind / trg_group_rig_bind.  parent [n_joints] uint32 (NO_PARENT: a root), key_first [n_joints + 1], keys [n_keys, 12] float32
    {time, T | R | S, 0}, clock_of [n_joints], inv_bind [n_joints, 12] or None.  n_keys: the count to pass (default: len(keys))."""
    L = load()
    par, kf, ks, co, ib = _tables(parent, key_first, keys, clock_of, inv_bind)
    # (a refused bind raises here and leaves the earlier rig, and its remembered counts, as they were)
    _binding.call(L, ctx, "rig_bind", capi._ptr(par), par.shape[0], capi._ptr(kf), capi._ptr(ks), ks.shape[0] if n_keys is None else int(n_keys), capi._ptr(co),
                  int(n_clocks), capi._ptr(ib))
    _binding.remember(ctx, "rig", (par.shape[0], int(n_clocks)))


def _clocks(ctx, clocks):
    x = np.ascontiguousarray(clocks, np.float32).reshape(-1)
    bound = getattr(ctx, "_rig_counts", None)
    if bound is not None and x.shape[0] != bound[1]:
        raise ValueError("expected %d clocks, as bound, got %d" % (bound[1], x.shape[0]))
    return x


def evaluate(ctx, clocks):
    """trg_rig_evaluate: [n_clocks] float32, finite.  Does not wait."""
    x = _clocks(ctx, clocks)
    ctx._chk(load().trg_rig_evaluate(ctx.h_ctx, capi._ptr(x)))


def read(ctx):
    """trg_rig_read: (bones, world) of the last evaluation, [n_joints, 12] float32 each."""
    n = _binding.counts(ctx, "rig")[0]
    bones, world = np.empty((n, 12), np.float32), np.empty((n, 12), np.float32)
    ctx._chk(load().trg_rig_read(ctx.h_ctx, capi._ptr(bones), capi._ptr(world)))
    return bones, world


def buffers(ctx):
    """trg_rig_buffers: dict of device addresses (int) -- bones, world."""
    out = [C.c_void_p(), C.c_void_p()]
    ctx._chk(load().trg_rig_buffers(ctx.h_ctx, C.byref(out[0]), C.byref(out[1])))
    return {"bones": out[0].value, "world": out[1].value}


def release(ctx):
    """Frees the rig of a context, or of every context of a group."""
    _binding.remember(ctx, "rig", None)
    _binding.release(load(), ctx, "rig")


def skin_apply(ctx, clocks):
    """trg_rig_skin_apply / trg_group_rig_skin_apply."""
    _binding.call(load(), ctx, "rig_skin_apply", capi._ptr(_clocks(ctx, clocks)))


def _weights(ctx, weights):
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    bound = getattr(ctx, "_morph_counts", None)
    if bound is not None and w.shape[0] != bound[2]:
        raise ValueError("expected %d target weights, as bound, got %d" % (bound[2], w.shape[0]))
    return w


def morph_apply(ctx, weights, clocks):
    """trg_rig_morph_apply / trg_group_rig_morph_apply: [n_targets] float32 and the clocks."""
    _binding.call(load(), ctx, "rig_morph_apply", capi._ptr(_weights(ctx, weights)), capi._ptr(_clocks(ctx, clocks)))


def _device_bones(ctx, bones, unit, at):
    import torch
    t = pose._tensor(bones, "bones", (torch.float32,), int(ctx.device))
    n_bones = _binding.counts(ctx, unit)[at]
    if t.numel() != 12 * n_bones:
        raise ValueError("expected %d bones of 12 floats, as bound, got %d floats" % (n_bones, t.numel()))
    return t


def skin_apply_device(ctx, bones):
    """trg_rig_skin_apply_device: a contiguous float32 torch tensor of n_bones x 12 on the context's device, passed by data_ptr().  The caller's
    stream must have finished writing it."""
    t = _device_bones(ctx, bones, "skin", 2)
    ctx._chk(load().trg_rig_skin_apply_device(ctx.h_ctx, t.data_ptr()))


def morph_apply_device(ctx, weights, bones):
    """trg_rig_morph_apply_device: the target weights on the host, the bones as for skin_apply_device."""
    t = _device_bones(ctx, bones, "morph", 3)
    ctx._chk(load().trg_rig_morph_apply_device(ctx.h_ctx, capi._ptr(_weights(ctx, weights)), t.data_ptr()))


def check_rig(parent, key_first, keys, clock_of, n_clocks, inv_bind=None, n_keys=None):
    """The validators of trg_rig_bind in its order: None, or (what, joint, key) of the first offender -- what is one of "counts", "parent",
    "table", "time", "ts", "rotation", "clock", "inv_bind", "depth" (the one that is TRG_ERR_RANGE); joint / key are None where the C text names
    none."""
    par = np.asarray(parent, np.int64).reshape(-1)
    kf = np.asarray(key_first, np.int64).reshape(-1)
    ks = np.asarray(keys, np.float32).reshape(-1, 12)
    co = np.asarray(clock_of, np.int64).reshape(-1)
    nj = par.shape[0]
    nk = ks.shape[0] if n_keys is None else int(n_keys)
    if nj == 0 or nk == 0 or int(n_clocks) == 0:
        return ("counts", None, None)
    j = np.arange(nj)
    bad = np.flatnonzero((par != NO_PARENT) & (par >= j))
    if bad.size:
        return ("parent", int(bad[0]), None)
    if kf[0] != 0:
        return ("table", 0, None)
    bad = np.flatnonzero(~(kf[:-1] < kf[1:]))
    if bad.size:
        return ("table", int(bad[0]), None)
    if kf[nj] != nk:
        return ("table", nj - 1, None)
    owner = np.repeat(j, np.diff(kf))
    first_of = np.zeros(nk, bool)
    first_of[kf[:-1]] = True
    with np.errstate(all="ignore"):
        t = ks[:nk, 0]
        ok = np.isfinite(t)
        ok[1:] &= first_of[1:] | (t[:-1] < t[1:])
        for what, good in (("time", ok), ("ts", np.isfinite(ks[:nk, [1, 2, 3, 8, 9, 10]]).all(1)),
                           ("rotation", np.isfinite(ks[:nk, 4:8]).all(1) & (np.abs((ks[:nk, 4:8].astype(np.float64) ** 2).sum(1) - 1.0) <= 1e-3))):
            bad = np.flatnonzero(~good)
            if bad.size:
                return (what, int(owner[bad[0]]), int(bad[0]))
    bad = np.flatnonzero(co >= int(n_clocks))
    if bad.size:
        return ("clock", int(bad[0]), None)
    if inv_bind is not None:
        bad = np.flatnonzero(~np.isfinite(np.asarray(inv_bind, np.float32).reshape(-1, 12)).all(1))
        if bad.size:
            return ("inv_bind", int(bad[0]), None)
    bad = np.flatnonzero(depths(par) >= MAX_LEVELS)
    if bad.size:
        return ("depth", int(bad[0]), None)
    return None


def depths(parent):
    """Depth of every joint of a forest that obeys the parent rule (a root: 0)."""
    par = np.asarray(parent, np.int64).reshape(-1)
    d = np.zeros(par.shape[0], np.int64)
    for j in range(par.shape[0]):
        if par[j] != NO_PARENT:
            d[j] = d[par[j]] + 1
    return d


def level_table(parent):
    """(order [n_joints], level_first [n_levels + 1]): the joints sorted by depth, ascending joint index within a level."""
    d = depths(parent)
    order = np.argsort(d, kind="stable").astype(np.uint32)
    return order, np.concatenate([[0], np.cumsum(np.bincount(d))]).astype(np.uint32)


def _compose(P, L):
    """P o L for [n, 12] float32: a_ik = (p_i0 l_0k + p_i1 l_1k) + p_i2 l_2k;  t_i = ((p_i0 lt_0 + p_i1 lt_1) + p_i2 lt_2) + pt_i."""
    P, L = P.reshape(-1, 3, 4), L.reshape(-1, 3, 4)
    out = np.empty_like(P)
    for i in range(3):
        for k in range(4):
            v = (P[:, i, 0] * L[:, 0, k] + P[:, i, 1] * L[:, 1, k]) + P[:, i, 2] * L[:, 2, k]
            out[:, i, k] = v + P[:, i, 3] if k == 3 else v
    return out.reshape(-1, 12)


def local_matrices(key_first, keys, clock_of, clocks):
    """[n_joints, 12] float32: every joint sampled at its clock and made a matrix, every operation rounded to float32 in the order
    trg_rig_math.h states it:
         t <= time[first]: the first key; t >= time[last]: the last; else i = the largest index with time[i] <= t, a = key i, b = key i + 1,
         u = (t - ta) / (tb - ta);  T = a.T + u (b.T - a.T);  S likewise
         d = ((ax bx + ay by) + az bz) + aw bw; b = -b if d < 0;  q = a + u (b - a);  len = sqrt(((qx qx + qy qy) + qz qz) + qw qw)
         R = q / len if len > 0 and finite, else a
         r00 = 1 - 2 (yy + zz), r01 = 2 (xy - wz), r02 = 2 (xz + wy), r10 = 2 (xy + wz), r11 = 1 - 2 (xx + zz), r12 = 2 (yz - wx),
         r20 = 2 (xz - wy), r21 = 2 (yz + wx), r22 = 1 - 2 (xx + yy);  a_ik = r_ik S[k];  t_i = T[i]."""
    f = np.float32
    kf = np.asarray(key_first, np.int64).reshape(-1)
    ks = np.ascontiguousarray(keys, f).reshape(-1, 12)
    t = np.ascontiguousarray(clocks, f).reshape(-1)[np.asarray(clock_of, np.int64).reshape(-1)]
    nj = kf.shape[0] - 1
    first, last = kf[:-1], kf[1:] - 1
    ia = np.empty(nj, np.int64)
    for j in range(nj):                                   # (the largest i of the joint's own track with time[i] <= t)
        ia[j] = first[j] + max(int(np.searchsorted(ks[first[j]:last[j] + 1, 0], t[j], side="right")) - 1, 0)
    before, after = t <= ks[first, 0], t >= ks[last, 0]
    ia = np.where(before, first, np.where(after, last, np.minimum(ia, last - 1)))
    same = before | after
    ib = np.where(same, ia, ia + 1)
    a, b = ks[ia], ks[ib]
    with np.errstate(all="ignore"):
        u = (t - a[:, 0]) / (b[:, 0] - a[:, 0])
        T = a[:, 1:4] + u[:, None] * (b[:, 1:4] - a[:, 1:4])
        S = a[:, 8:11] + u[:, None] * (b[:, 8:11] - a[:, 8:11])
        qa, qb = a[:, 4:8], b[:, 4:8]
        d = ((qa[:, 0] * qb[:, 0] + qa[:, 1] * qb[:, 1]) + qa[:, 2] * qb[:, 2]) + qa[:, 3] * qb[:, 3]
        qb = np.where((d < 0)[:, None], -qb, qb)
        q = qa + u[:, None] * (qb - qa)
        length = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        ok = (length > 0) & np.isfinite(length)
        R = np.where(ok[:, None], q / np.where(ok, length, f(1))[:, None], qa)
        T = np.where(same[:, None], a[:, 1:4], T)
        S = np.where(same[:, None], a[:, 8:11], S)
        R = np.where(same[:, None], qa, R)
        assert T.dtype == f and S.dtype == f and R.dtype == f and length.dtype == f
        x, y, z, w = R[:, 0], R[:, 1], R[:, 2], R[:, 3]
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        one, two = f(1), f(2)
        r = [[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
             [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
             [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]]
        Lm = np.empty((nj, 3, 4), f)
        for i in range(3):
            for k in range(3):
                Lm[:, i, k] = r[i][k] * S[:, k]
            Lm[:, i, 3] = T[:, i]
    return Lm.reshape(nj, 12)


def rig_reference(parent, key_first, keys, clock_of, clocks, inv_bind=None):
    """(bones, world), [n_joints, 12] float32 each: local_matrices, then level by level world[j] = world[parent[j]] o local[j] -- a root's world is
    its local, bits and all -- and bone[j] = world[j] o inv_bind[j], or the world's bits without inverse binds."""
    par = np.asarray(parent, np.int64).reshape(-1)
    Lm = local_matrices(key_first, keys, clock_of, clocks)
    world = np.empty_like(Lm)
    order, level_first = level_table(par)
    with np.errstate(all="ignore"):
        for l in range(level_first.shape[0] - 1):
            js = order[level_first[l]:level_first[l + 1]].astype(np.int64)
            world[js] = Lm[js] if l == 0 else _compose(world[par[js]], Lm[js])
        bones = world.copy() if inv_bind is None else _compose(world, np.ascontiguousarray(inv_bind, np.float32).reshape(-1, 12))
    assert world.dtype == np.float32 and bones.dtype == np.float32
    return bones, world
