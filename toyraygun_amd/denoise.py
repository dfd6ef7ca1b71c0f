"""First-hit guide buffers and the edge-avoiding a-trous denoiser of include/trg_denoise.h.

    g = guides(ctx, frame_index)                 # [2, h, w, 4]: G0 = normal xyz | hit distance, G1 = albedo rgb | primitive index bits
    out = denoise(ctx, color, g, iterations=5)   # [h, w, 4]
    out = render_denoised(ctx, 0, 4, 3)          # trg_render + guides + filter on one stream; the accumulation buffer is only read

    h = render_halves(ctx, 0, 4, 3)              # [2, h, w, 4]: the means of frames [0, 2) and [2, 4), rendered independently
    out = denoise_variance(ctx, h, g)            # the variance-guided filter (SVGF's weights, variance from the two halves)
    out = render_denoised_variance(ctx, 0, 4, 3) # halves + guides + that filter; the accumulation buffer is not touched

    g, x = guides_pos(ctx, frame_index)          # the guides and the world positions of the first hits [h, w, 4]
    vp = temporal_view_proj(uniforms)            # world -> clip of a frame's camera, for the call that comes after it
    out = temporal_denoise(ctx, color, g, x, vp) # one temporal step: reproject the state's history, accumulate, filter with the temporal variance
    out = render_temporal(ctx, k, 1, 3)          # render + guides + that step; the state remembers the camera; temporal_reset(ctx) forgets

    ctx.load_scene(...moved geometry...)         # moving geometry of unchanged topology keeps its history:
    temporal_set_previous_scene(ctx, old_positions, old_normals, indices)   # where every triangle was; arms the next render_temporal
    g, x, m = guides_motion(ctx, frame_index)    # the guides, X, and M0 / M1 [2, h, w, 4]: where each hit was and its normal then
    out = temporal_denoise(ctx, color, g, x, vp, motion=m)                  # the step looks for the history there

    temporal_set_lag_correction(ctx, 3.0)        # changing light: every later step corrects the accumulated colour by the gated lag of its
                                                 # 7 x 7 window (off again: a negative gate); lag_correct(...) is that stage alone
    temporal_set_variance_of_mean(ctx, True)     # a long history: the variance of the ACCUMULATED colour travels in Hm.z and steers the
                                                 # iterations, so the filter narrows as the history grows (a change forgets the history)

    temporal_set_coverage(ctx, 0.9)              # pixel footprints: render_temporal takes its guides from the pixel CENTRES (guides_centre:
                                                 # X.w = 1 where the frame's jittered ray agrees with the centre hit), the agreement is accumulated
                                                 # in Hm.w, and a pixel below 0.9 stays out of the filter (a change forgets the history)

numpy arrays go through temporary device copies and the call waits for the result; torch ROCm tensors (float32, contiguous) are used in place
through data_ptr() -- like trg_bind_accum -- and the call only enqueues on the context's current stream.  `reference_denoise`,
`reference_denoise_variance` (its iteration loop alone: `reference_atrous_variance`) and `reference_temporal` (with `reference_centre_rays` and `reference_agreement` for the centre guides) are the float64 numpy evaluations
of the definitions in the header: what the GPU tests compare the kernels with.

The context's denoise scratch belongs to the context: ctx.close() frees it, release(ctx) frees it earlier.
"""
import ctypes as C
import re

import numpy as np

from . import capi

MAX_ITERATIONS = 6
LUMA = (0.2126, 0.7152, 0.0722)
B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


class Params(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int32)]


class VarParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int32), ("prefilter", C.c_int32)]


class TemporalParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int32), ("alpha", C.c_float), ("alpha_moments", C.c_float), ("plane_tol", C.c_float),
                ("normal_tol", C.c_float), ("max_history", C.c_int32)]


_P = C.c_void_p
_PP = C.POINTER(Params)
_VP = C.POINTER(VarParams)
_TP = C.POINTER(TemporalParams)
_F16 = C.POINTER(C.c_float)
_U = C.c_uint32
_SYMBOLS = [
    ("trg_denoise_default_params", None, [_PP]),
    ("trg_guides_render", C.c_int, [_P, C.c_uint32, _P]),
    ("trg_denoise", C.c_int, [_P, _P, _P, _P, _PP]),
    ("trg_render_denoised", C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _PP]),
    ("trg_denoise_accum", C.c_int, [_P, C.c_uint32, _PP, C.POINTER(_P)]),
    ("trg_denoise_release", C.c_int, [_P]),
    ("trg_guides_read", C.c_int, [_P, C.c_uint32, _P]),
    ("trg_denoise_host", C.c_int, [_P, _P, _P, _P, _PP]),
    ("trg_render_denoised_read", C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _PP]),
    ("trg_denoise_var_default_params", None, [_VP]),
    ("trg_render_halves", C.c_int, [_P, _U, _U, _U, _P]),
    ("trg_denoise_variance", C.c_int, [_P, _P, _P, _P, _VP]),
    ("trg_render_denoised_variance", C.c_int, [_P, _U, _U, _U, _P, _VP]),
    ("trg_render_denoised_variance_own", C.c_int, [_P, _U, _U, _U, _VP, C.POINTER(_P)]),
    ("trg_render_halves_read", C.c_int, [_P, _U, _U, _U, _P]),
    ("trg_denoise_variance_host", C.c_int, [_P, _P, _P, _P, _P, _VP]),
    ("trg_render_denoised_variance_read", C.c_int, [_P, _U, _U, _U, _P, _VP]),
    ("trg_guides_render_pos", C.c_int, [_P, _U, _P, _P]),
    ("trg_temporal_view_proj", C.c_int, [_P, _F16]),
    ("trg_temporal_default_params", None, [_TP]),
    ("trg_temporal_reset", C.c_int, [_P]),
    ("trg_temporal_history_read", C.c_int, [_P, _P]),
    ("trg_temporal_denoise", C.c_int, [_P, _P, _P, _P, _F16, _P, _TP]),
    ("trg_render_temporal", C.c_int, [_P, _U, _U, _U, _P, _TP]),
    ("trg_render_temporal_own", C.c_int, [_P, _U, _U, _U, _TP, C.POINTER(_P)]),
    ("trg_guides_pos_read", C.c_int, [_P, _U, _P, _P]),
    ("trg_temporal_denoise_host", C.c_int, [_P, _P, _P, _P, _F16, _P, _P, _P, _TP]),
    ("trg_render_temporal_read", C.c_int, [_P, _U, _U, _U, _P, _TP]),
    ("trg_temporal_set_previous_scene", C.c_int, [_P, _P, _P, _P, _U, _U]),
    ("trg_temporal_set_previous_scene_device", C.c_int, [_P, _P, _P, _P, _U, _U]),
    ("trg_guides_render_motion", C.c_int, [_P, _U, _P, _P, _P]),
    ("trg_temporal_denoise_motion", C.c_int, [_P, _P, _P, _P, _P, _F16, _P, _TP]),
    ("trg_guides_motion_read", C.c_int, [_P, _U, _P, _P, _P]),
    ("trg_temporal_denoise_motion_host", C.c_int, [_P, _P, _P, _P, _P, _F16, _P, _P, _P, _TP]),
    ("trg_temporal_set_lag_correction", C.c_int, [_P, C.c_float]),
    ("trg_temporal_lag_correction", C.c_int, [_P, _F16]),
    ("trg_temporal_lag_correct_host", C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_int32, _P]),
    ("trg_temporal_set_variance_of_mean", C.c_int, [_P, C.c_int]),
    ("trg_temporal_variance_of_mean", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("trg_guides_render_centre", C.c_int, [_P, _U, C.c_float, C.c_float, _P, _P]),
    ("trg_guides_render_centre_motion", C.c_int, [_P, _U, C.c_float, C.c_float, _P, _P, _P]),
    ("trg_guides_centre_read", C.c_int, [_P, _U, C.c_float, C.c_float, _P, _P]),
    ("trg_guides_centre_motion_read", C.c_int, [_P, _U, C.c_float, C.c_float, _P, _P, _P]),
    ("trg_temporal_set_coverage", C.c_int, [_P, C.c_float]),
    ("trg_temporal_coverage", C.c_int, [_P, _F16]),
]
LAG_GATE_DEFAULT = 3.0   # TRG_TEMPORAL_LAG_GATE_DEFAULT
COVERAGE_MIN_DEFAULT = 0.9   # TRG_TEMPORAL_COVERAGE_MIN_DEFAULT
SYMBOL_NAMES = [s[0] for s in _SYMBOLS]

_bound = None


def load():
    """The library handle of capi.load() with the symbols of include/trg_denoise.h bound.  No fallback: a library without them is an error."""
    global _bound
    L = capi.load()
    if _bound is not L:
        for name, res, args in _SYMBOLS:
            fn = getattr(L, name)   # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def header_symbols(path):
    """The trg_* functions a C header declares with TRG_API."""
    with open(path) as f:
        return re.findall(r"TRG_API\s+[\w\s\*]*?\b(trg_\w+)\s*\(", f.read())


def default_params():
    p = Params()
    load().trg_denoise_default_params(C.byref(p))
    return p


def _unpack(params):
    return {f: getattr(params, f) for f, _ in params._fields_}


def _make(cls, defaults_symbol, ints, what, params, kw):
    """A `cls` from the library's defaults, a `cls` / dict, and keyword overrides."""
    p = cls()
    getattr(load(), defaults_symbol)(C.byref(p))
    src = _unpack(params) if isinstance(params, cls) else dict(params or {})
    src.update(kw)
    for k, v in src.items():
        if k not in dict(cls._fields_):
            raise TypeError("unknown %s parameter %r" % (what, k))
        setattr(p, k, int(v) if k in ints else float(v))
    return p


def make_params(params=None, **kw):
    """Params from the library's defaults, a Params / dict, and keyword overrides (iterations, sigma_color, sigma_normal, sigma_depth, demodulate)."""
    return _make(Params, "trg_denoise_default_params", ("iterations", "demodulate"), "denoise", params, kw)


# the header's defaults, for the references (no library needed)
_DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_normal=128.0, sigma_depth=1.0, demodulate=1)
_VAR_DEFAULTS = dict(iterations=5, sigma_lum=4.0, sigma_normal=128.0, sigma_depth=1.0, demodulate=1, prefilter=1)
_TEMPORAL_DEFAULTS = dict(iterations=5, sigma_lum=4.0, sigma_normal=128.0, sigma_depth=1.0, demodulate=1, alpha=0.2, alpha_moments=0.2,
                          plane_tol=0.02, normal_tol=0.9, max_history=32)


def make_var_params(params=None, **kw):
    """VarParams from the library's defaults, a VarParams / dict, and keyword overrides."""
    return _make(VarParams, "trg_denoise_var_default_params", ("iterations", "demodulate", "prefilter"), "variance-guided denoise", params, kw)


def make_temporal_params(params=None, **kw):
    """TemporalParams from the library's defaults, a TemporalParams / dict, and keyword overrides."""
    return _make(TemporalParams, "trg_temporal_default_params", ("iterations", "demodulate", "max_history"), "temporal denoise", params, kw)


def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _tensor_ptr(t, shape, what):
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda" or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a contiguous float32 ROCm tensor of shape %s" % (what, (tuple(shape),)))
    return C.c_void_p(t.data_ptr())


def _chk(ctx, rc):
    if rc != capi.OK:
        raise capi.TrgError(rc, (ctx.L.trg_last_error(ctx.h_ctx) or b"").decode())


def _run(ctx, device_entry, host_entry, outputs, inputs=(), head=(), mid=(), tail=(), host_only=(), host_only_error=None, shape_error=None):
    """The one fork of the bindings.  Both entry points take (ctx, *head, *inputs, *mid, *outputs, *tail); inputs and outputs are lists of
    (name, value, shape), host_only one of (wanted, shape) for the outputs that only the host entry point has, behind the others.
    Torch tensors -- the first input, or without inputs a given first output -- go in place through the device entry point, which only enqueues
    on the context's stream: every tensor is checked, an output that is None is allocated, a wanted host-only output is refused.  Otherwise the
    host entry point, which waits: the inputs as contiguous float32 numpy arrays of their shapes, the outputs new numpy arrays.
    Returns the outputs, the wanted host-only ones included, as a tuple; one output alone as itself."""
    L = load()
    first = inputs[0][1] if inputs else outputs[0][1]
    if device_entry and first is not None and _is_tensor(first):
        import torch
        if any(wanted for wanted, _ in host_only):
            raise ValueError(host_only_error)
        ptrs = [_tensor_ptr(t, shape, what) for what, t, shape in inputs]
        outs = [torch.empty(shape, dtype=torch.float32, device=first.device) if t is None else t for _, t, shape in outputs]
        ptrs += mid + tuple(_tensor_ptr(t, shape, what) for t, (what, _, shape) in zip(outs, outputs))
        _chk(ctx, getattr(L, device_entry)(ctx.h_ctx, *head, *ptrs, *tail))
    else:
        arrays = [np.ascontiguousarray(a, np.float32) for _, a, _ in inputs]
        if any(a.shape != shape for a, (_, _, shape) in zip(arrays, inputs)):
            raise ValueError(shape_error)
        outs = [np.empty(shape, np.float32) for _, _, shape in outputs] + [np.empty(shape, np.float32) if wanted else None for wanted, shape in host_only]
        ptrs = [a.ctypes.data for a in arrays] + list(mid) + [None if o is None else o.ctypes.data for o in outs]
        _chk(ctx, getattr(L, host_entry)(ctx.h_ctx, *head, *ptrs, *tail))
        outs = [o for o in outs if o is not None]
    return outs[0] if len(outs) == 1 else tuple(outs)


def _shapes(ctx):
    """The shapes of an image and of a pair of planes."""
    return (ctx.h, ctx.w, 4), (2, ctx.h, ctx.w, 4)


def _fill(ctx, device_entry, read_entry, args, out, planes, what, *params):
    """`out` a float32 ROCm tensor: filled in place through the device entry point, on the context's stream (and returned); None: a numpy array
    through the _read entry point, which waits.  planes = 2: [2, h, w, 4], 0: [h, w, 4]."""
    return _run(ctx, device_entry, read_entry, [(what, out, _shapes(ctx)[1 if planes else 0])], head=args, tail=params)


def guides(ctx, frame_index, out=None):
    """trg_guides_render.  out = a [2, h, w, 4] float32 ROCm tensor: filled in place on the context's stream (and returned); None: a numpy array."""
    return _fill(ctx, "trg_guides_render", "trg_guides_read", (frame_index,), out, 2, "guides")


def denoise(ctx, color, guides, out=None, params=None, **kw):
    """trg_denoise.  All tensors (then `out` is a tensor too, or is allocated like `color`; enqueued only) or all numpy (waits)."""
    p = make_params(params, **kw)
    cs, gs = _shapes(ctx)
    return _run(ctx, "trg_denoise", "trg_denoise_host", [("out", out, cs)], [("color", color, cs), ("guides", guides, gs)], tail=(C.byref(p),),
                shape_error="color must be %s and guides %s" % (cs, gs))


def render_denoised(ctx, frame_begin, spp, bounces, out=None, params=None, **kw):
    """trg_render_denoised: frames [frame_begin, frame_begin + spp) into the context's accumulation buffer, guides of frame_begin, the filter."""
    return _fill(ctx, "trg_render_denoised", "trg_render_denoised_read", (frame_begin, spp, bounces), out, 0, "out", C.byref(make_params(params, **kw)))


def render_halves(ctx, frame_begin, spp, bounces, out=None):
    """trg_render_halves: frames [frame_begin, frame_begin + spp/2) and [frame_begin + spp/2, frame_begin + spp) rendered from zeroed images of the
    state and scaled to the means of their samples -> [2, h, w, 4].  spp even, >= 2.  The bound accumulation buffer is not written; the rays count."""
    return _fill(ctx, "trg_render_halves", "trg_render_halves_read", (frame_begin, spp, bounces), out, 2, "halves")


def denoise_variance(ctx, halves, guides, out=None, params=None, return_variance=False, **kw):
    """trg_denoise_variance.  All tensors (enqueued only) or all numpy (waits).  return_variance (numpy only): also V_N [h, w], the variance the
    filter carried to its end."""
    p = make_var_params(params, **kw)
    cs, gs = _shapes(ctx)
    return _run(ctx, "trg_denoise_variance", "trg_denoise_variance_host", [("out", out, cs)], [("halves", halves, gs), ("guides", guides, gs)], tail=(C.byref(p),),
                host_only=[(return_variance, cs[:2])], host_only_error="return_variance needs numpy arrays (trg_denoise_variance_host)",
                shape_error="halves and guides must be %s" % (gs,))


def render_denoised_variance(ctx, frame_begin, spp, bounces, out=None, params=None, **kw):
    """trg_render_denoised_variance: render_halves, guides of frame_begin, denoise_variance, on one stream."""
    return _fill(ctx, "trg_render_denoised_variance", "trg_render_denoised_variance_read", (frame_begin, spp, bounces), out, 0, "out",
                 C.byref(make_var_params(params, **kw)))


def guides_pos(ctx, frame_index, out=None, pos=None):
    """trg_guides_render_pos -> (guides [2, h, w, 4], X [h, w, 4]).  out, pos = float32 ROCm tensors: filled in place on the context's stream
    (and returned); None: numpy arrays."""
    xs, gs = _shapes(ctx)
    return _run(ctx, "trg_guides_render_pos", "trg_guides_pos_read", [("guides", out, gs), ("pos", pos, xs)], head=(frame_index,))


def temporal_view_proj(uniforms):
    """trg_temporal_view_proj: the world -> clip matrix [16] float32 of a frame's uniforms (a capi.Uniforms, any ctypes structure of that layout,
    or its 176 bytes).  ValueError when the inverse view-projection is singular or not finite."""
    buf = C.create_string_buffer(bytes(uniforms) if isinstance(uniforms, (bytes, bytearray)) else bytes(memoryview(uniforms)), C.sizeof(capi.Uniforms))
    vp = np.empty(16, np.float32)
    if load().trg_temporal_view_proj(C.cast(buf, C.c_void_p), vp.ctypes.data_as(_F16)) != capi.OK:
        raise ValueError("the uniforms' inverse view-projection is singular or not finite")
    return vp


def temporal_reset(ctx):
    _chk(ctx, load().trg_temporal_reset(ctx.h_ctx))


def temporal_history(ctx):
    """trg_temporal_history_read -> [2, h, w, 4]: Hc = (I.rgb, N), Hm = (m1, m2, 0, 0) of the last step -- (m1, m2, Vc, 0) with the variance of the mean
    on.  Waits."""
    hist = np.empty((2, ctx.h, ctx.w, 4), np.float32)
    _chk(ctx, load().trg_temporal_history_read(ctx.h_ctx, hist.ctypes.data))
    return hist


def _vp_arg(prev_vp):
    vp = np.ascontiguousarray(np.zeros(16, np.float32) if prev_vp is None else prev_vp, np.float32).reshape(-1)
    if vp.shape != (16,):
        raise ValueError("prev_vp must hold 16 floats")
    return vp


def temporal_set_previous_scene(ctx, positions, normals, indices):
    """trg_temporal_set_previous_scene: where the triangles of the loaded scene were at the previous call -- positions [n_verts, 3], normals
    [3 * n_tris, 3] or None (unchanged), indices [3 * n_tris], in trg_load_scene's layouts.  Arms the state for the next render_temporal.
    positions = None: the previous scene is forgotten."""
    L = load()
    if positions is None:
        _chk(ctx, L.trg_temporal_set_previous_scene(ctx.h_ctx, None, None, None, 0, 0))
        return
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if idx.shape[0] % 3 or (nrm is not None and nrm.shape[0] != idx.shape[0]):
        raise ValueError("expected 3*n_tris indices and, with normals, 3*n_tris of them")
    _chk(ctx, L.trg_temporal_set_previous_scene(ctx.h_ctx, pos.ctypes.data, None if nrm is None else nrm.ctypes.data, idx.ctypes.data, pos.shape[0], idx.shape[0] // 3))


def temporal_set_previous_scene_device(ctx, positions, normals, indices, n_verts=None, n_tris=None):
    """trg_temporal_set_previous_scene_device: the same from buffers on the context's device, without a copy and without a wait.  positions,
    normals (or None), indices: contiguous float32 / float32 / int32-or-uint32 ROCm tensors in the layouts above -- or device addresses (int, as
    pose.buffers gives them) with n_verts and n_tris.  The caller keeps them unchanged until the context's stream has passed the call."""
    L = load()

    def address(x, floats):
        if x is None or isinstance(x, int):
            return x
        import torch
        ok = (torch.float32,) if floats else tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in ok and x.is_contiguous()):
            raise TypeError("expected a contiguous %s ROCm tensor or a device address" % ("float32" if floats else "int32 / uint32"))
        return x.data_ptr()
    if n_verts is None:
        n_verts = positions.numel() // 3
    if n_tris is None:
        n_tris = indices.numel() // 3
    _chk(ctx, L.trg_temporal_set_previous_scene_device(ctx.h_ctx, address(positions, True), address(normals, True), address(indices, False), int(n_verts), int(n_tris)))


def guides_motion(ctx, frame_index, out=None, pos=None, motion=None):
    """trg_guides_render_motion -> (guides [2, h, w, 4], X [h, w, 4], motion [2, h, w, 4] = M0, M1: where the hit was and its normal then, by the
    previous scene of temporal_set_previous_scene).  out, pos, motion = float32 ROCm tensors: filled in place on the context's stream (and
    returned); None: numpy arrays."""
    xs, gs = _shapes(ctx)
    return _run(ctx, "trg_guides_render_motion", "trg_guides_motion_read", [("guides", out, gs), ("pos", pos, xs), ("motion", motion, gs)], head=(frame_index,))


def temporal_denoise(ctx, color, guides, pos, prev_vp, out=None, params=None, return_iv=False, return_variance=False, motion=None, **kw):
    """trg_temporal_denoise; with motion [2, h, w, 4] (M0, M1 as guides_motion gives them) trg_temporal_denoise_motion.  All tensors (enqueued
    only) or all numpy (waits).  prev_vp: temporal_view_proj of the previous call's uniforms (host memory; None: zeros, for the first call
    after a reset).  numpy only: return_iv also gives (I.rgb, V_0) [h, w, 4], return_variance V_N [h, w]."""
    p = make_temporal_params(params, **kw)
    vp = _vp_arg(prev_vp)
    cs, gs = _shapes(ctx)
    name = "trg_temporal_denoise" if motion is None else "trg_temporal_denoise_motion"
    inputs = [("color", color, cs), ("guides", guides, gs), ("pos", pos, cs)] + ([] if motion is None else [("motion", motion, gs)])
    return _run(ctx, name, name + "_host", [("out", out, cs)], inputs, mid=(vp.ctypes.data_as(_F16),), tail=(C.byref(p),),
                host_only=[(return_iv, cs), (return_variance, cs[:2])], host_only_error="return_iv / return_variance need numpy arrays (trg_temporal_denoise_host)",
                shape_error="color and pos must be %s, guides and motion %s" % (cs, gs))


def render_temporal(ctx, frame_begin, spp, bounces, out=None, params=None, **kw):
    """trg_render_temporal: frames [frame_begin, frame_begin + spp) from a zeroed image of the state, guides and positions of frame_begin, one
    temporal step against the camera of the previous call.  The bound accumulation buffer is not touched; the rays count."""
    return _fill(ctx, "trg_render_temporal", "trg_render_temporal_read", (frame_begin, spp, bounces), out, 0, "out", C.byref(make_temporal_params(params, **kw)))


def temporal_set_lag_correction(ctx, gate=LAG_GATE_DEFAULT):
    """trg_temporal_set_lag_correction: gate >= 0 switches the gated lag correction of the accumulated colour on for every later temporal step of
    this context (a lighting change no longer waits for `alpha`), gate < 0 (or None) off -- the state of a new context.  NaN is refused."""
    _chk(ctx, load().trg_temporal_set_lag_correction(ctx.h_ctx, -1.0 if gate is None else float(gate)))


def temporal_lag_correction(ctx):
    """trg_temporal_lag_correction: the gate that is set; < 0 when the correction is off."""
    gate = C.c_float(0.0)
    _chk(ctx, load().trg_temporal_lag_correction(ctx.h_ctx, C.byref(gate)))
    return float(gate.value)


def lag_correct(ctx, color, guides, hc, gate, sigma_normal=128.0, sigma_depth=1.0, demodulate=1):
    """trg_temporal_lag_correct_host: the correction alone (stage-level; numpy; waits).  color [h, w, 4], guides [2, h, w, 4], hc [h, w, 4] =
    (I.rgb, N) -> (Ic.rgb, N) [h, w, 4].  The context's own setting and history play no part."""
    cs, gs = _shapes(ctx)
    return _run(ctx, None, "trg_temporal_lag_correct_host", [("out", None, cs)], [("color", color, cs), ("guides", guides, gs), ("hc", hc, cs)],
                mid=(float(gate), float(sigma_normal), float(sigma_depth), int(demodulate)), shape_error="color and hc must be %s and guides %s" % (cs, gs))


def temporal_set_variance_of_mean(ctx, on=True):
    """trg_temporal_set_variance_of_mean: every later temporal step of this context carries the variance of the ACCUMULATED colour through the
    history (Hm.z) and hands that to the iterations, so the filter narrows as the history grows.  Off: the state of a new context.  A call that
    changes the setting forgets the history like temporal_reset."""
    _chk(ctx, load().trg_temporal_set_variance_of_mean(ctx.h_ctx, 1 if on else 0))


def temporal_variance_of_mean(ctx):
    """trg_temporal_variance_of_mean: whether the setting is on."""
    on = C.c_int(-1)
    _chk(ctx, load().trg_temporal_variance_of_mean(ctx.h_ctx, C.byref(on)))
    return bool(on.value)


def guides_centre(ctx, frame_index, plane_tol=_TEMPORAL_DEFAULTS["plane_tol"], normal_tol=_TEMPORAL_DEFAULTS["normal_tol"], out=None, pos=None,
                  motion=None, with_motion=False):
    """trg_guides_render_centre -> (guides [2, h, w, 4], X [h, w, 4]) from the rays through the pixel CENTRES; X.w = A, 1 where the jittered
    primary ray of frame_index agrees with the centre hit under the two tolerances, else 0.  with_motion (or a `motion` tensor):
    trg_guides_render_centre_motion, which also gives M0, M1 [2, h, w, 4] from the centre hits.  out, pos, motion = float32 ROCm tensors: filled
    in place on the context's stream (and returned); None: numpy arrays."""
    xs, gs = _shapes(ctx)
    head = (frame_index, float(plane_tol), float(normal_tol))
    if motion is not None or with_motion:
        return _run(ctx, "trg_guides_render_centre_motion", "trg_guides_centre_motion_read", [("guides", out, gs), ("pos", pos, xs), ("motion", motion, gs)], head=head)
    return _run(ctx, "trg_guides_render_centre", "trg_guides_centre_read", [("guides", out, gs), ("pos", pos, xs)], head=head)


def temporal_set_coverage(ctx, cov_min=COVERAGE_MIN_DEFAULT):
    """trg_temporal_set_coverage: 0 <= cov_min < 1 switches the coverage history on for every later temporal step of this context -- render_temporal
    then takes its guides from the pixel centres, and a pixel whose accumulated agreement is below cov_min is kept out of the filter and shows its
    accumulated colour --, cov_min < 0 (or None) off, the state of a new context.  NaN and cov_min >= 1 are refused.  A call that changes the
    value forgets the history like temporal_reset."""
    _chk(ctx, load().trg_temporal_set_coverage(ctx.h_ctx, -1.0 if cov_min is None else float(cov_min)))


def temporal_coverage(ctx):
    """trg_temporal_coverage: the cov_min that is set; < 0 when the setting is off."""
    v = C.c_float(0.0)
    _chk(ctx, load().trg_temporal_coverage(ctx.h_ctx, C.byref(v)))
    return float(v.value)


def release(ctx):
    if getattr(ctx, "h_ctx", None):
        _chk(ctx, load().trg_denoise_release(ctx.h_ctx))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 reference, written from the definition in include/trg_denoise.h
# ---------------------------------------------------------------------------------------------------------------------------------------------
# Every function below takes the working precision `dtype`: np.float64 (the default: THE reference) or np.float32, where every intermediate is
# fp32, x ** sigma_normal is exp2(sigma_normal * log2 x) and exp(x) is exp2(x * log2 e) as the shipped build evaluates them -- a yardstick for
# how far fp32 arithmetic alone moves a result (the bars of tests/test_gpu_denoise_shapes.py), never a test subject.
_LOG2E = 1.4426950408889634


def _exp(x, dtype):
    return np.exp(x) if dtype is np.float64 else np.exp2(x * dtype(_LOG2E))


def _pow(x, y, dtype):
    return x ** y if dtype is np.float64 else np.exp2(dtype(y) * np.log2(x))


def _lum(I, dtype):
    if dtype is np.float64:
        return I @ np.array(LUMA)
    return (dtype(LUMA[0]) * I[..., 0] + dtype(LUMA[1]) * I[..., 1]) + dtype(LUMA[2]) * I[..., 2]


def _dtype(dtype):
    dtype = np.dtype(dtype).type
    if dtype not in (np.float64, np.float32):
        raise ValueError("dtype must be np.float64 or np.float32")
    return dtype


def _shift(a, dx, dy, fill=0.0):
    """b[y, x] = a[y + dy, x + dx] where that lies inside, else fill; and the inside mask."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]
        inside[ys:ye, xs:xe] = True
    return b, inside


def _depth_gradient(z):
    def along(dx, dy):
        fwd, fin = _shift(z, dx, dy, -1.0)
        bwd, bin_ = _shift(z, -dx, -dy, -1.0)
        f_ok, b_ok = fin & (fwd >= 0), bin_ & (bwd >= 0)
        return np.where(f_ok, fwd - z, np.where(b_ok, z - bwd, 0.0))
    return np.sqrt(along(1, 0) ** 2 + along(0, 1) ** 2)


def atrous_weights(I, g0, spacing, sigma_color, sigma_normal, sigma_depth, dtype=np.float64):
    """w[dy + 2, dx + 2, y, x] of one iteration on input I [h, w, 3] (of `dtype`); zero for skipped taps; rows of miss pixels are meaningless."""
    dtype = _dtype(dtype)
    h, w = I.shape[:2]
    lum = _lum(I, dtype)
    cnt = np.zeros((h, w), dtype)
    s1 = np.zeros((h, w), dtype)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            l, ins = _shift(lum, dx, dy)
            s1 += np.where(ins, l, 0.0); cnt += ins
    mean = s1 / cnt
    s2 = np.zeros((h, w), dtype)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            l, ins = _shift(lum, dx, dy)
            s2 += np.where(ins, (l - mean) ** 2, 0.0)
    var = s2 / cnt
    sc2 = sigma_color ** 2 if dtype is np.float64 else dtype(sigma_color) * dtype(sigma_color)
    W = geometry_weights(g0, spacing, sigma_normal, sigma_depth, dtype=dtype)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            Iq, _ = _shift(I, dx * spacing, dy * spacing)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                wc = _exp(-((I - Iq) ** 2).sum(-1) / (sc2 * (var + 1e-4)), dtype)
            W[dy + 2, dx + 2] = np.where(W[dy + 2, dx + 2] > 0, W[dy + 2, dx + 2] * wc, 0.0)
    return W


def geometry_weights(g0, spacing, sigma_normal, sigma_depth, kernel=B3, dtype=np.float64):
    """k(dx) k(dy) * w_n * w_z * w_id of the header for the (2r+1)^2 taps at `spacing`, r = len(kernel) // 2: [dy + r, dx + r, y, x]; zero for
    skipped taps (outside the image, a miss, n_p . n_q <= 0); rows of miss pixels are meaningless."""
    dtype = _dtype(dtype)
    h, w = g0.shape[:2]
    n, z = g0[..., :3], g0[..., 3]
    r = len(kernel) // 2
    grad = _depth_gradient(z)
    W = np.zeros((2 * r + 1, 2 * r + 1, h, w), dtype)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            gq, ins = _shift(g0, dx * spacing, dy * spacing, -1.0)
            nq, zq = gq[..., :3], gq[..., 3]
            dn = (n * nq).sum(-1)
            ok = ins & (zq >= 0) & (dn > 0)
            dist = dtype(np.sqrt(dtype(dx * dx + dy * dy)))
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                wn = _pow(np.where(dn > 0, np.abs(dn), 1.0), sigma_normal, dtype)
                wz = _exp(-np.abs(z - zq) / (sigma_depth * (grad * spacing * dist + 1e-6)), dtype)
                W[dy + r, dx + r] = np.where(ok, kernel[dx + r] * kernel[dy + r] * wn * wz, 0.0)
    return W


def emitter_mask(g1, material_ids):
    """[h, w] bool: pixels whose first hit (G1.w, int32 bits) is a primitive of material 2 (TRG_MATERIAL_EMISSIVE) of a scene with these ids."""
    prim = np.ascontiguousarray(np.asarray(g1, np.float32)[..., 3]).view(np.int32)
    mats = np.asarray(material_ids).reshape(-1)
    inside = (prim >= 0) & (prim < mats.shape[0])
    return inside & (mats[np.where(inside, prim, 0)] == 2)


def _options(defaults, cls, params, kw):
    """The header's defaults, then a `cls` structure or a dict, then keywords; the iteration count checked against the header's range."""
    q = dict(defaults)
    if isinstance(params, cls):
        params = _unpack(params)
    q.update(params or {}); q.update(kw)
    if not 0 <= int(q["iterations"]) <= MAX_ITERATIONS:
        raise ValueError("iterations must be 0..%d" % MAX_ITERATIONS)
    return q


def reference_denoise(color, g0, g1, params=None, material_ids=None, dtype=np.float64, **kw):
    """float64 evaluation of trg_denoise's definition.  color [h, w, 4], g0 / g1 [h, w, 4] (float32 as the device sees them); params: a Params,
    a dict or keywords; the defaults are the header's (no library needed); material_ids: those of the context's scene (None: no scene, no
    emitters); dtype: the working precision (see above).  Returns [h, w, 4] of `dtype`."""
    dtype = _dtype(dtype)
    q = _options(_DEFAULTS, Params, params, kw)
    it = int(q["iterations"])
    out = np.asarray(color).astype(dtype)
    if it == 0:
        return out
    # the parameters as the device holds them: fp32
    sc, sn, sd = (float(np.float32(q[k])) for k in ("sigma_color", "sigma_normal", "sigma_depth"))
    g0, alb, miss = _filter_inputs(g0, g1, material_ids, dtype)
    I = out[..., :3].copy()
    demod = bool(q["demodulate"])
    if demod:
        I = np.where(miss[..., None], I, I / alb)
    for i in range(it):
        s = 1 << i
        W = atrous_weights(I, g0, s, sc, sn, sd, dtype=dtype)
        wsum = W.sum((0, 1))
        keep = miss | ~(wsum > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            I = np.where(keep[..., None], I, _gather(W, I, s) / wsum[..., None])
    if demod:
        I = np.where(miss[..., None], I, I * alb)
    out[..., :3] = I
    return out


def _gather(W, a, spacing):
    r = W.shape[0] // 2
    acc = np.zeros_like(a)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            aq, _ = _shift(a, dx * spacing, dy * spacing)
            acc += (W[dy + r, dx + r][..., None] if a.ndim == 3 else W[dy + r, dx + r]) * aq
    return acc


def _atrous_variance_loop(I, V, g0, miss, alb, it, sl, sn, sd, demod, dtype):
    """Iterations 0 .. it-1 of the variance-guided filter and the remodulation, on arrays of `dtype` (g0 with the emitters already marked)."""
    binom = (0.25, 0.5, 0.25)
    valid = (~miss).astype(dtype)
    for i in range(it):
        s = 1 << i
        bs, vs = np.zeros_like(V), np.zeros_like(V)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, _ = _shift(V * valid, dx, dy)
                mq, _ = _shift(valid, dx, dy)
                vs += binom[dx + 1] * binom[dy + 1] * vq
                bs += binom[dx + 1] * binom[dy + 1] * mq
        with np.errstate(invalid="ignore", divide="ignore"):
            gv = np.where(bs > 0, vs / bs, 0.0)
        den = sl * np.sqrt(np.maximum(0.0, gv)) + float(np.float32(1e-3))
        lum = _lum(I, dtype)
        W = geometry_weights(g0, s, sn, sd, dtype=dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                lq, _ = _shift(lum, dx * s, dy * s)
                W[dy + 2, dx + 2] = W[dy + 2, dx + 2] * _exp(-np.abs(lum - lq) / den, dtype)
        wsum = W.sum((0, 1))
        keep = miss | ~(wsum > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            I = np.where(keep[..., None], I, _gather(W, I, s) / wsum[..., None])
            V = np.where(keep, V, _gather(W * W, V, s) / wsum ** 2)
    if demod:
        I = np.where(miss[..., None], I, I * alb)
    return I, V


def _filter_inputs(g0, g1, material_ids, dtype):
    """(the filter's G0 with the emitters marked as misses, the clamped albedo, the miss mask) in `dtype`."""
    g0 = np.asarray(g0, np.float32).astype(dtype)
    if material_ids is not None:                       # a directly seen emitter is kept out of the filter like a miss
        g0[emitter_mask(g1, material_ids), 3] = -1.0
    alb = np.maximum(np.asarray(g1, np.float32)[..., :3].astype(dtype), float(np.float32(1e-3)))
    return g0, alb, g0[..., 3] < 0


def reference_atrous_variance(I0, V0, g0, g1, params=None, material_ids=None, dtype=np.float64, **kw):
    """The iteration loop of trg_denoise_variance's definition on its own: (I_0 [h, w, 3], V_0 [h, w]) -- DEMODULATED when `demodulate` -- through
    iterations 0 .. N-1 and the remodulation.  params: a VarParams / TemporalParams, a dict or keywords; only iterations, sigma_lum,
    sigma_normal, sigma_depth and demodulate are read (defaults: the header's).  Returns (rgb [h, w, 3], V_N [h, w]) of `dtype`.
    reference_denoise_variance is its start, this loop, and the alpha channel; reference_temporal supplies another start."""
    dtype = _dtype(dtype)
    q = _options(_VAR_DEFAULTS, C.Structure, params, kw)
    sl, sn, sd = (float(np.float32(q[k])) for k in ("sigma_lum", "sigma_normal", "sigma_depth"))
    g0, alb, miss = _filter_inputs(g0, g1, material_ids, dtype)
    I = np.asarray(I0)[..., :3].astype(dtype)
    V = np.asarray(V0).astype(dtype)
    return _atrous_variance_loop(I, V, g0, miss, alb, int(q["iterations"]), sl, sn, sd, bool(q["demodulate"]), dtype)


def reference_denoise_variance(h1, h2, g0, g1, params=None, material_ids=None, return_variance=False, dtype=np.float64, **kw):
    """float64 evaluation of trg_denoise_variance's definition.  h1, h2 [h, w, 4] the half buffers, g0 / g1 [h, w, 4] (float32 as the device sees
    them); params: a VarParams, a dict or keywords over the header's defaults (no library needed); material_ids: those of the context's scene
    (None: no scene, no emitters); dtype: the working precision (see above).  Returns [h, w, 4] of `dtype` (and V_N [h, w] with return_variance)."""
    dtype = _dtype(dtype)
    q = _options(_VAR_DEFAULTS, VarParams, params, kw)
    it = int(q["iterations"])
    h1, h2 = np.asarray(h1).astype(dtype), np.asarray(h2).astype(dtype)
    out = np.empty_like(h1)
    out[..., 3] = h1[..., 3]
    sl, sn, sd = (float(np.float32(q[k])) for k in ("sigma_lum", "sigma_normal", "sigma_depth"))
    g0, alb, miss = _filter_inputs(g0, g1, material_ids, dtype)
    demod = bool(q["demodulate"])
    d1 = np.where(miss[..., None], h1[..., :3], h1[..., :3] / alb) if demod else h1[..., :3]
    d2 = np.where(miss[..., None], h2[..., :3], h2[..., :3] / alb) if demod else h2[..., :3]
    I = 0.5 * (d1 + d2)
    V = np.where(miss, 0.0, 0.25 * (_lum(d1, dtype) - _lum(d2, dtype)) ** 2)

    if q["prefilter"]:
        G = geometry_weights(g0, 1, sn, sd, kernel=(1.0,) * 7, dtype=dtype)
        gs = G.sum((0, 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            V = np.where(miss | ~(gs > 0), V, _gather(G, V, 1) / gs)
    if it == 0:
        out[..., :3] = 0.5 * (h1[..., :3] + h2[..., :3])
        return (out, V) if return_variance else out
    I, V = _atrous_variance_loop(I, V, g0, miss, alb, it, sl, sn, sd, demod, dtype)
    out[..., :3] = I
    return (out, V) if return_variance else out


NEAR = 1e-4   # reference_temporal: how close (relative) to its threshold a discrete decision counts as undecidable in fp32


def reference_motion(isect, prev_positions, prev_normals, indices, g0):
    """The motion planes of trg_guides_render_motion, fp32-exact by construction: every product and sum below is one float32 operation in the
    header's order.  isect: the hit records of the frame's primary rays (capi.ISECT_DTYPE, h*w of them: trg_raygen + trg_trace of the same frame
    index); prev_positions [n_verts, 3], prev_normals [3 * n_tris, 3] or None, indices [3 * n_tris]: what trg_temporal_set_previous_scene was
    given; g0 [h, w, 4]: the frame's G0 (M1 without previous normals).  Returns [2, h, w, 4] float32: M0, M1."""
    f = np.float32
    g0 = np.asarray(g0, np.float32)
    h, w = g0.shape[:2]
    pos = np.asarray(prev_positions, np.float32).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    dist = np.asarray(isect["distance"], np.float32).reshape(h, w)
    prim = np.asarray(isect["primitiveIndex"], np.int64).reshape(h, w)
    co = np.asarray(isect["coordinates"], np.float32).reshape(h, w, 2)
    hit = (dist >= 0) & (prim >= 0) & (prim < idx.shape[0])
    k = np.where(hit, prim, 0)
    c0, c1 = co[..., 0:1], co[..., 1:2]
    c2 = (f(1.0) - c0) - c1

    def blend(a):                                     # a [h, w, 3 corners, 3]
        return ((c0 * a[..., 0, :] + c1 * a[..., 1, :]) + c2 * a[..., 2, :]).astype(np.float32)
    m = np.zeros((2, h, w, 4), np.float32)
    m[0, ..., :3] = blend(pos[idx[k]])
    m[0, ..., 3] = 1.0
    if prev_normals is None:
        m[1, ..., :3] = g0[..., :3]
    else:
        m[1, ..., :3] = blend(np.asarray(prev_normals, np.float32).reshape(-1, 3, 3)[k])
    m[:, ~hit] = 0.0
    return m


def _lag(D, I, F, miss, gate, sn, sd, dtype):
    """The gated lag correction of the header (CHANGING LIGHT) on arrays of `dtype`: D, I [h, w, 3], F the filter's G0 with the emitters marked.
    Returns (Ic [h, w, 3], changed [h, w] bool)."""
    gate = dtype(np.float32(gate))
    Wg = geometry_weights(F, 1, sn, sd, kernel=(1.0,) * 7, dtype=dtype)
    # times 2^-k, k = the exponent of the centre's own weight within [-126, 126]: exact, and g * g stays inside fp32
    gc = Wg[3, 3]
    k = np.clip(np.frexp(np.where(np.isfinite(gc) & (gc > 0), gc, 1.0))[1] - 1, -126, 126)
    Wg = np.where(miss[None, None], 0.0, np.ldexp(Wg, -k[None, None])).astype(dtype)      # (the rows of misses are meaningless: none is corrected)
    h, w = miss.shape
    G, G2 = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
    E, A1, A2 = (np.zeros((h, w, 3), dtype) for _ in range(3))
    for dy in range(-3, 4):                                # rows outer, columns inner: the header's order
        for dx in range(-3, 4):
            g = Wg[dy + 3, dx + 3]
            Dq, _ = _shift(D, dx, dy)
            Iq, _ = _shift(I, dx, dy)
            t = Dq - D
            G += g
            G2 += g * g
            E += g[..., None] * (Dq - Iq)
            A1 += g[..., None] * t
            A2 += g[..., None] * (t * t)
    ok = ~miss & (G > 0)
    Gs = np.where(ok, G, 1.0).astype(dtype)[..., None]
    d, m1 = E / Gs, A1 / Gs
    se = np.sqrt(np.maximum(0.0, A2 / Gs - m1 * m1) * G2[..., None]) / Gs
    m = np.abs(d) - gate * se
    with np.errstate(invalid="ignore"):
        on = ok[..., None] & (m > 0)
    Ic = np.where(on, np.maximum(I + np.copysign(m, d), np.minimum(I, 0.0)), I).astype(dtype)
    return Ic, (Ic != I).any(-1)


def reference_lag(color, g0, g1, hc, gate, params=None, material_ids=None, dtype=np.float64, **kw):
    """float64 evaluation of the gated lag correction (the header's CHANGING LIGHT) on its own: color, g0, g1 [h, w, 4] of this call, hc [h, w, 4]
    = (I.rgb, N) as Accumulate left it (taken in the precision it comes in: the device's fp32 plane, or a float64 plane of reference_temporal); params: a TemporalParams, a dict or keywords -- sigma_normal, sigma_depth and demodulate are read (defaults:
    the header's); material_ids: those of the context's scene; dtype: the working precision.  Returns (Ic [h, w, 3] of `dtype`, the [h, w] bool
    mask of the pixels it changed)."""
    dtype = _dtype(dtype)
    q = _options(_TEMPORAL_DEFAULTS, TemporalParams, params, kw)
    sn, sd = float(np.float32(q["sigma_normal"])), float(np.float32(q["sigma_depth"]))
    C3 = np.asarray(color, np.float32)[..., :3].astype(dtype)
    F, alb, miss = _filter_inputs(g0, g1, material_ids, dtype)
    D = np.where(miss[..., None], C3, C3 / alb) if q["demodulate"] else C3
    return _lag(D, np.asarray(hc)[..., :3].astype(dtype), F, miss, gate, sn, sd, dtype)


def reference_centre_rays(uniforms, w, h):
    """The centre rays of trg_guides_render_centre, fp32-exact by construction: trg_raygen's arithmetic with 0.5 in place of both Halton values,
    every operation below one float32 operation in the header's order.  uniforms: a capi.Uniforms, any ctypes structure of that layout, or its
    176 bytes (width, height and frameIndex are not read: w, h say the size).  Returns w * h records of capi.RAY_DTYPE, row 0 first."""
    f = np.float32
    raw = bytes(uniforms) if isinstance(uniforms, (bytes, bytearray)) else bytes(memoryview(uniforms))
    cam = np.frombuffer(raw, np.float32, 3, 16)
    m = np.frombuffer(raw, np.float32, 16, 32)
    x, y = np.meshgrid(np.arange(w, dtype=f), np.arange(h, dtype=f))
    uvx = ((x + f(0.5)) / f(w)) * f(2.0) - f(1.0)
    uvy = ((y + f(0.5)) / f(h)) * f(2.0) - f(1.0)
    zero, one = np.zeros_like(uvx), np.ones_like(uvx)
    world = [((uvx * m[j * 4] + uvy * m[j * 4 + 1]) + zero * m[j * 4 + 2]) + one * m[j * 4 + 3] for j in range(4)]
    t = [world[k] / world[3] - cam[k] for k in range(3)]
    inv = f(1.0) / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    rays = np.zeros(w * h, capi.RAY_DTYPE)
    rays["origin"] = cam
    rays["mask"] = 3
    rays["direction"] = np.stack([(t[k] * inv).astype(f) for k in range(3)], -1).reshape(-1, 3)
    rays["maxDistance"] = np.inf
    rays["color"] = (1.0, 1.0, 1.0, 0.0)
    return rays


def reference_agreement(isect_centre, g0, pos, isect_jitter, rays_jitter, normals, material_ids, plane_tol=_TEMPORAL_DEFAULTS["plane_tol"],
                        normal_tol=_TEMPORAL_DEFAULTS["normal_tol"]):
    """The agreement flag A of trg_guides_render_centre.  isect_centre, isect_jitter: the hit records (capi.ISECT_DTYPE, h * w each) of the centre
    rays and of the frame's jittered primary rays; rays_jitter: those jittered rays (capi.RAY_DTYPE); g0, pos [h, w, 4]: the centre guides' G0
    and X (float32 as the device sees them); normals [3 * n_tris, 3], material_ids [n_tris]: the loaded scene's.  The jittered hit's n_j and
    X_j = o + z d are formed in fp32 as the gather forms them; the two tests are then evaluated in float64.
    Returns (A [h, w] float32 of 0 / 1, near [h, w] bool): near marks the pixels where the plane distance lies within NEAR of plane_tol z_c
    (relative) or the cosine within NEAR of normal_tol (absolute), the rule of reference_temporal's tap tests."""
    f = np.float32
    g0 = np.asarray(g0, np.float32)
    h, w = g0.shape[:2]
    mats = np.asarray(material_ids).reshape(-1)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3, 3)

    def fields(isect):
        dist = np.asarray(isect["distance"], np.float32).reshape(h, w)
        prim = np.asarray(isect["primitiveIndex"], np.int64).reshape(h, w)
        hit = (dist >= 0) & (prim >= 0) & (prim < mats.shape[0])
        return dist, np.where(hit, prim, 0), hit, np.asarray(isect["coordinates"], np.float32).reshape(h, w, 2)
    _, pc, hit_c, _ = fields(isect_centre)
    zj, pj, hit_j, co = fields(isect_jitter)
    c0, c1 = co[..., 0:1], co[..., 1:2]
    c2 = (f(1.0) - c0) - c1
    a = nrm[pj]
    nj = ((c0 * a[..., 0, :] + c1 * a[..., 1, :]) + c2 * a[..., 2, :]).astype(np.float32)
    o = np.asarray(rays_jitter["origin"], np.float32).reshape(h, w, 3)
    d = np.asarray(rays_jitter["direction"], np.float32).reshape(h, w, 3)
    Xj = (o + (zj[..., None] * d).astype(np.float32)).astype(np.float32)

    def unit(v):
        v = v.astype(np.float64)
        ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        ok = ln > 0
        return v / np.where(ok, ln, 1.0)[..., None], ok

    def dot3(p, q):
        return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]
    n, n_ok = unit(g0[..., :3])
    nq, nq_ok = unit(nj)
    both = hit_c & hit_j & ((mats[pc] == 2) == (mats[pj] == 2))
    tol = float(f(plane_tol)) * g0[..., 3].astype(np.float64)
    dist = np.abs(dot3(n, Xj.astype(np.float64) - np.asarray(pos, np.float32)[..., :3].astype(np.float64)))
    cosn = dot3(n, nq)
    with np.errstate(invalid="ignore"):
        agree = both & n_ok & nq_ok & (dist <= tol) & (cosn >= float(f(normal_tol)))
        near = both & n_ok & nq_ok & ((np.abs(dist - tol) <= NEAR * tol) | (np.abs(cosn - float(f(normal_tol))) <= NEAR))
    return agree.astype(np.float32), near


def reference_temporal(color, g0, g1, pos, history, prev_vp, params=None, material_ids=None, dtype=np.float64, near_parts=False, motion=None, lag=None,
                       track=False, coverage=None, **kw):
    """float64 evaluation of ONE step of trg_temporal_denoise's definition up to the filter: reprojection, accumulation, V_0.
    color, g0, g1, pos [h, w, 4] (float32 as the device sees them); history: the previous call's four planes (Hc, Hm, F, X), each [h, w, 4], or
    None; prev_vp: 16 floats; params: a TemporalParams, a dict or keywords over the header's defaults (no library needed); material_ids: those
    of the context's scene; dtype: the working precision (np.float32: the yardstick mode of the other references).
    Returns (new history [4, h, w, 4], iv [h, w, 4] = (I.rgb, V_0), near [h, w] bool) -- near marks the pixels where a discrete decision lies
    within NEAR of flipping: clip.w against 0, a relevant tap's plane distance against plane_tol z_p (relative to that bound) or its normal
    cosine against normal_tol (cosines of unit vectors: absolute), W against 0 (W is a sum of bilinear weights that add up to 1: absolute; the
    window test -1 <= f < size is the same decision, every tap it removes has a weight near 0), and N against 4 (relative).  The result then
    goes through reference_atrous_variance.  near_parts: the third result is the pair (near without the last decision, near of N against 4 alone)
    instead -- N against 4 chooses between the two forms of V_0 and nothing else, so colour, N and the moments of such a pixel are still decided.
    motion: None, or (M0, M1) [2, h, w, 4]: trg_temporal_denoise_motion's definition -- M0.xyz in place of X(p) in the projection and the plane
    test, M1.xyz in place of the pixel's normal in the plane and the normal test, no history where M0.w is not > 0; `near` marks the same
    decisions, on the substituted operands.
    lag: None, or the gate of the lag correction (trg_temporal_set_lag_correction): Ic takes I's place in the new Hc and in iv; the moments, N
    and V_0 are the uncorrected step's, and `near` gains nothing (the correction's one decision, G > 0, is the spatial estimate's).
    track: the variance of the mean (trg_temporal_set_variance_of_mean): history[1][..., 2] is read as Vc', the new Hm.z and iv[..., 3] are Vc of
    the header's definition -- S for N < 4 or without history, else ((1 - a)(1 - a)) Vh + (a a) S --; everything else, `near` included, is the
    plain step's exactly.  False: Hm.z is 0 and every array is what it was before the argument existed.
    coverage: None, or cov_min of the coverage history (trg_temporal_set_coverage): pos[..., 3] is read as the agreement flag A and history[1][..., 3]
    as cov'; the new Hm.w is cov; a hit with cov < cov_min is MIXED: a miss for the spatial estimate, the lag correction and (through the marked G0)
    the iterations, its iv.rgb remodulated, its V_0 the temporal form whatever N; `near` also marks cov within NEAR (absolute) of a cov_min > 0.
    Two more results then: (new history, iv, near, mixed [h, w] bool, the filter's G0 [h, w, 4] with emitters AND mixed pixels marked) -- hand
    that G0 to reference_atrous_variance with material_ids=None.  None: the result is what it was before the argument existed."""
    dtype = _dtype(dtype)
    q = _options(_TEMPORAL_DEFAULTS, TemporalParams, params, kw)
    alpha, alpha_m, plane_tol, normal_tol = (dtype(np.float32(q[k])) for k in ("alpha", "alpha_moments", "plane_tol", "normal_tol"))
    max_hist = dtype(int(q["max_history"]))
    sn, sd = float(np.float32(q["sigma_normal"])), float(np.float32(q["sigma_depth"]))
    demod = bool(q["demodulate"])
    C3 = np.asarray(color, np.float32)[..., :3].astype(dtype)
    F, alb, miss = _filter_inputs(g0, g1, material_ids, dtype)
    X = np.asarray(pos, np.float32)[..., :3].astype(dtype)
    h, w = miss.shape
    D = np.where(miss[..., None], C3, C3 / alb) if demod else C3
    l = _lum(D, dtype)
    near = np.zeros((h, w), bool)

    def unit(v):
        ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        ok = ln > 0
        return v / np.where(ok, ln, 1.0)[..., None], ok

    def dot3(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    W = np.zeros((h, w), dtype)
    acc = np.zeros((h, w, 6), dtype)                       # I.rgb, N, m1, m2
    vh = np.zeros((h, w), dtype)                           # track: the sum of b * Hm'.z
    covh = np.zeros((h, w), dtype)                         # coverage: the sum of b * Hm'.w
    if history is not None:
        Hc, Hm, Hf, Hx = (np.asarray(p, np.float32).astype(dtype) for p in history)
        vp = np.asarray(prev_vp, np.float32).reshape(16).astype(dtype)
        known = True
        R = X                                               # where the hit was when the history was written, and its normal then
        if motion is not None:
            M = np.asarray(motion, np.float32).astype(dtype)
            R, known = M[0, ..., :3], M[0, ..., 3] > 0
        n, n_ok = unit(F[..., :3] if motion is None else M[1, ..., :3])
        clip = [((vp[j * 4] * R[..., 0] + vp[j * 4 + 1] * R[..., 1]) + vp[j * 4 + 2] * R[..., 2]) + vp[j * 4 + 3] for j in (0, 1, 3)]
        cw = clip[2]
        cand = ~miss & n_ok & known                         # pixels that look for history at all
        scale = np.abs(vp[12] * R[..., 0]) + np.abs(vp[13] * R[..., 1]) + np.abs(vp[14] * R[..., 2]) + np.abs(vp[15])
        near |= cand & (np.abs(cw) <= NEAR * scale)
        front = cand & (cw > 0)
        cws = np.where(front, cw, 1.0)
        fx = (clip[0] / cws * dtype(0.5) + dtype(0.5)) * dtype(w) - dtype(0.5)
        fy = (clip[1] / cws * dtype(0.5) + dtype(0.5)) * dtype(h) - dtype(0.5)
        # (the definition's window -1 <= f < size says "some tap is inside"; taps outside are skipped below anyway, so a window one pixel wider
        #  gives the same sums and only keeps the integer conversion safe)
        with np.errstate(invalid="ignore"):
            window = front & (fx >= -2) & (fx < w + 1) & (fy >= -2) & (fy < h + 1)
        fxs, fys = np.where(window, fx, 0.0), np.where(window, fy, 0.0)
        flx, fly = np.floor(fxs), np.floor(fys)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        tx, ty = fxs - flx, fys - fly
        tol = plane_tol * F[..., 3]
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = window & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                fq, xq = Hf[cy, cx], Hx[cy, cx][..., :3]
                live = inside & (fq[..., 3] >= 0)
                dist = np.abs(dot3(n, xq - R))
                nq, nq_ok = unit(fq[..., :3])
                cosn = dot3(n, nq)
                with np.errstate(invalid="ignore"):
                    valid = live & (dist <= tol) & nq_ok & (cosn >= normal_tol)
                    near |= live & ((np.abs(dist - tol) <= NEAR * tol) | (nq_ok & (np.abs(cosn - normal_tol) <= NEAR)))
                b = (tx if i else 1 - tx) * (ty if j else 1 - ty)
                b = np.where(valid, b, 0.0)
                hc, hm = Hc[cy, cx], Hm[cy, cx]
                acc[..., :4] += b[..., None] * hc
                acc[..., 4] += b * hm[..., 0]
                acc[..., 5] += b * hm[..., 1]
                if track:
                    vh += b * hm[..., 2]
                if coverage is not None:
                    covh += b * hm[..., 3]
                W += b
        # W > 0: a sum of weights near 0 with a valid tap in it; or none in it while the sample sits within NEAR of a pixel centre's row or
        # column, where one rounding brings another tap pair into play with a weight near 0
        on_grid = (tx <= NEAR) | (tx >= 1 - NEAR) | (ty <= NEAR) | (ty >= 1 - NEAR)
        near |= window & (W <= NEAR) & ((W > 0) | on_grid)
    have = W > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        hist = acc / np.where(have, W, 1.0)[..., None]
    Nh = hist[..., 3]
    N = np.where(have, np.minimum(Nh + 1, max_hist), 1.0).astype(dtype)
    one = dtype(1.0)
    a = np.maximum(alpha, one / N)[..., None]
    am = np.maximum(alpha_m, one / N)
    I = np.where(have[..., None], hist[..., :3] + a * (D - hist[..., :3]), D)
    m1 = np.where(have, hist[..., 4] + am * (l - hist[..., 4]), l)
    m2 = np.where(have, hist[..., 5] + am * (l * l - hist[..., 5]), l * l)
    I = np.where(miss[..., None], C3, I)
    N = np.where(miss, 0.0, N).astype(dtype)
    m1, m2 = np.where(miss, 0.0, m1).astype(dtype), np.where(miss, 0.0, m2).astype(dtype)
    near_n = ~miss & (np.abs(N - 4) <= NEAR * 4)
    mixed = np.zeros((h, w), bool)
    hit = ~miss                                             # (below, `miss` gains the mixed pixels: what counts as a miss behind the reprojection)
    if coverage is not None:
        cov_min = dtype(np.float32(coverage))
        A = np.asarray(pos, np.float32)[..., 3].astype(dtype)
        ch = covh / np.where(have, W, 1.0)
        cov = np.where(miss, 0.0, np.where(have, ch + am * (A - ch), A)).astype(dtype)
        mixed = hit & (cov < cov_min)
        if cov_min > 0:
            near |= hit & (np.abs(cov - cov_min) <= NEAR)
        F_own = F
        F = F.copy()
        F[mixed, 3] = -1.0
        miss = miss | mixed
    # V_0: temporal from four frames on, else the spatial estimate over this call's moments with the prefilter's weights
    G = geometry_weights(F, 1, sn, sd, kernel=(1.0,) * 7, dtype=dtype)
    gs = G.sum((0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        M1, M2 = _gather(G, m1, 1) / gs, _gather(G, m2, 1) / gs
        spatial = np.where(gs > 0, np.maximum(0.0, M2 - M1 * M1) * dtype(4.0) / np.where(miss, 1.0, N), 0.0)
    V0 = np.where(~hit, 0.0, np.where((N >= 4) | mixed, np.maximum(0.0, m2 - m1 * m1), spatial)).astype(dtype)
    if lag is not None:
        I = _lag(D.astype(dtype), I.astype(dtype), F, miss, lag, sn, sd, dtype)[0]
    new = np.zeros((4, h, w, 4), dtype)
    if track:
        # the variance of the accumulated colour: the recursion from four frames on, the variance of one sample (S = V_0 as above) before
        ac = a[..., 0]
        Vh = vh / np.where(have, W, 1.0)
        Vc = ((one - ac) * (one - ac)) * Vh + (ac * ac) * V0
        V0 = np.where(~hit, 0.0, np.where(have & (N >= 4), Vc, V0)).astype(dtype)
        new[1, ..., 2] = V0
    new[0, ..., :3], new[0, ..., 3] = I, N
    new[1, ..., 0], new[1, ..., 1] = m1, m2
    new[2] = F
    new[3, ..., :3] = X
    new[3, ..., 3] = np.asarray(pos, np.float32)[..., 3].astype(dtype)
    if coverage is None:
        iv = np.concatenate([I, V0[..., None]], -1).astype(dtype)
        return new, iv, ((near, near_n) if near_parts else near | near_n)
    new[1, ..., 3] = cov
    new[2] = F_own                                          # the history keeps the unmarked guide
    Iv = np.where(mixed[..., None], I * alb, I) if demod else I
    iv = np.concatenate([Iv, V0[..., None]], -1).astype(dtype)
    return new, iv, ((near, near_n) if near_parts else near | near_n), mixed, F
