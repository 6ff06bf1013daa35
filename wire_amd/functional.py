"""torch.autograd.Functions over the libwire_hip C ABI.

PyTorch here is plumbing only: it owns device buffers (so the caching allocator
and stream semantics apply), records the autograd edge, and hands raw pointers
plus the current HIP stream to the library.  All arithmetic of the MLP stack --
forward and backward -- happens in the HIP kernels.

Backward runs on autograd's own thread; nothing here depends on thread-local
state except the library's error string.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import torch

from . import _lib


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.WireHipError(
            f"{what} is on {t.device}; wire_amd runs on an MI355X only (no CPU fallback). "
            "Move the model and its inputs to 'cuda'.")


def _no_second_order(what: str) -> None:
    # backward runs with grad mode on only under create_graph=True: the coordinate gradient is computed by kernels that
    # record no graph of their own, so a second-order request must fail instead of returning a gradient without one
    if torch.is_grad_enabled():
        raise NotImplementedError(
            f"{what}: the gradient with respect to the coordinates is first order only (create_graph=True is not "
            "supported when the coordinates require a gradient)")


def _native(t: torch.Tensor) -> torch.Tensor:
    """Contiguous tensor whose storage is the native layout the ABI expects
    (complex64 = interleaved floats)."""
    return t.detach().contiguous()


def _workspace(query: str, dev: torch.device, *shape) -> torch.Tensor:
    """A workspace for one call: ``query`` is the library's size query (a wire_*_ws_bytes name) and ``shape`` its
    arguments.  The size to hand to the entry point is the tensor's numel()."""
    return torch.empty(_lib.check(getattr(_lib.lib(), query)(*shape), query), dtype=torch.uint8, device=dev)


class _INRFunction(torch.autograd.Function):
    """Whole-network forward/backward: wire_mlp_fwd / wire_mlp_bwd."""

    @staticmethod
    def forward(ctx, coords: torch.Tensor, desc: _lib.NetDesc, grad_mode: bool, *params: torch.Tensor):
        L = _lib.lib()
        _require_cuda(coords, "coords")
        dev = coords.device
        D, O = desc.in_features, desc.out_features
        if coords.shape[-1] != D:
            raise ValueError(f"coords last dim {coords.shape[-1]} != in_features {D}")
        x = coords.detach().to(torch.float32).contiguous()
        n = x.numel() // D
        nat = [_native(p) for p in params]
        for p in nat:
            _require_cuda(p, "a parameter")
        stream = _stream_ptr(dev)
        packed = torch.empty(L.wire_packed_floats(C.byref(desc)), dtype=torch.float32, device=dev)
        _lib.check(L.wire_pack_params(stream, C.byref(desc), _lib.ptr_array([p.data_ptr() for p in nat]),
                                      packed.data_ptr()), "wire_pack_params")
        # (inside torch.no_grad() needs_input_grad still reports the parameters' requires_grad; no graph is recorded
        #  there, so nothing is saved and the forward-only kernels run.  grad_mode = torch.is_grad_enabled() at the call:
        #  inside forward() it is always off)
        # (the coordinates' own requires_grad counts too: a frozen field can still differentiate to its inputs)
        need_bwd = grad_mode and any(ctx.needs_input_grad)
        act_bytes = _lib.check(L.wire_act_bytes(C.byref(desc), n, int(need_bwd)), "wire_act_bytes")
        act = torch.empty(act_bytes, dtype=torch.uint8, device=dev)
        y = torch.empty(tuple(coords.shape[:-1]) + (O,), dtype=torch.float32, device=dev)
        _lib.check(L.wire_mlp_fwd(stream, C.byref(desc), packed.data_ptr(), x.data_ptr(), n,
                                  y.data_ptr(), act.data_ptr(), act_bytes, int(need_bwd)),
                   "wire_mlp_fwd")
        if need_bwd:
            ctx.desc, ctx.n = desc, n
            ctx.packed, ctx.act, ctx.x = packed, act, x
            ctx.meta = [(p.shape, p.dtype) for p in params]
            ctx.xmeta = (tuple(coords.shape), coords.dtype)
        return y

    @staticmethod
    def backward(ctx, g_y: torch.Tensor):
        L = _lib.lib()
        desc, n = ctx.desc, ctx.n
        dev = g_y.device
        gy = g_y.detach().to(torch.float32).contiguous()
        stream = _stream_ptr(dev)
        if ctx.needs_input_grad[0]:
            _no_second_order("wire_amd model")
            want_p = any(ctx.needs_input_grad[3:])
            grads = [torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in ctx.meta] if want_p else []
            g_x = torch.empty(n, desc.in_features, dtype=torch.float32, device=dev)
            sbytes = _lib.check(L.wire_bwd_coords_scratch_bytes(C.byref(desc), n), "wire_bwd_coords_scratch_bytes")
            scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
            # grads_host = NULL without trainable parameters: the data-gradient chain alone (no weight-gradient GEMM)
            _lib.check(L.wire_mlp_bwd_coords(stream, C.byref(desc), ctx.packed.data_ptr(), ctx.x.data_ptr(), n,
                                             gy.data_ptr(), ctx.act.data_ptr(), ctx.act.numel(), scratch.data_ptr(),
                                             sbytes, _lib.ptr_array([g.data_ptr() for g in grads]) if want_p else None,
                                             g_x.data_ptr()), "wire_mlp_bwd_coords")
            xshape, xdtype = ctx.xmeta
            g_coords = g_x.reshape(xshape).to(xdtype)
            return (g_coords, None, None, *(grads if want_p else [None] * len(ctx.meta)))
        # (bspline_mscale_HL: its first stage W0, b0 is frozen -- no gradient, a NULL slot for the library)
        frozen = 2 if desc.kind == _lib.KIND["bspline_mscale_HL"] else 0
        grads = [None if i < frozen else torch.empty(shape, dtype=dtype, device=dev)
                 for i, (shape, dtype) in enumerate(ctx.meta)]
        sbytes = _lib.check(L.wire_bwd_scratch_bytes(C.byref(desc), n), "wire_bwd_scratch_bytes")
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.wire_mlp_bwd(stream, C.byref(desc), ctx.packed.data_ptr(), ctx.x.data_ptr(), n,
                                  gy.data_ptr(), ctx.act.data_ptr(), ctx.act.numel(),
                                  scratch.data_ptr(), sbytes,
                                  _lib.ptr_array([None if g is None else g.data_ptr() for g in grads])),
                   "wire_mlp_bwd")
        # the saved buffers stay with the graph node (freed with it), so backward(retain_graph=True) can run again
        return (None, None, None, *grads)


def inr_forward(coords: torch.Tensor, desc: _lib.NetDesc, params: Sequence[torch.Tensor]) -> torch.Tensor:
    return _INRFunction.apply(coords, desc, torch.is_grad_enabled(), *params)


def mscale_first(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, scales: Sequence[float]) -> torch.Tensor:
    """The frozen first stage of bspline_mscale_HL (Scaled_Bsplines_form.forward) on the device:
    x [..., D] -> [..., SHF] through wire_mscale_first_fwd.  Records no graph: the stage passes no gradient."""
    L = _lib.lib()
    _require_cuda(x, "layer input")
    _require_cuda(W, "layer weight")
    out_f, in_f = W.shape
    if x.shape[-1] != in_f:
        raise ValueError(f"input last dim {x.shape[-1]} != in_features {in_f}")
    xin = x.detach().to(torch.float32).contiguous()
    n = xin.numel() // in_f
    sc = (C.c_float * len(scales))(*[float(v) for v in scales])
    out = torch.empty(tuple(x.shape[:-1]) + (out_f,), dtype=torch.float32, device=x.device)
    _lib.check(L.wire_mscale_first_fwd(_stream_ptr(x.device), xin.data_ptr(), _native(W).data_ptr(),
                                       _native(b).data_ptr(), n, in_f, out_f, len(scales), sc, out.data_ptr()),
               "wire_mscale_first_fwd")
    return out


class _M2CombineFunction(torch.autograd.Function):
    """AdaptiveScaleCombiner 'freq_combine' of bspline_mscale_2 (Linear(S O -> 128), ReLU, Linear(128 -> O) of the
    concatenated pass outputs): wire_m2_combine_fwd / wire_m2_combine_bwd on t [S][..., O], the outputs stacked."""

    @staticmethod
    def forward(ctx, t, W1, b1, W2, b2):
        L = _lib.lib()
        _require_cuda(t, "combiner input")
        _require_cuda(W1, "combiner weight")
        S, O = t.shape[0], t.shape[-1]
        if W1.shape != (128, S * O) or W2.shape != (O, 128):
            raise ValueError(f"combiner weights {tuple(W1.shape)} / {tuple(W2.shape)} do not take {S} outputs of {O}")
        tin = t.detach().to(torch.float32).contiguous()
        n = tin.numel() // (S * O)
        nat = [_native(w) for w in (W1, b1, W2, b2)]
        y = torch.empty(tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
        _lib.check(L.wire_m2_combine_fwd(_stream_ptr(t.device), S, O, *[w.data_ptr() for w in nat], tin.data_ptr(), n,
                                         y.data_ptr()), "wire_m2_combine_fwd")
        ctx.save_for_backward(tin, *nat)
        ctx.cfg = (S, O, n)
        return y

    @staticmethod
    def backward(ctx, g_y):
        L = _lib.lib()
        tin, W1, b1, W2, b2 = ctx.saved_tensors
        S, O, n = ctx.cfg
        dev = g_y.device
        gy = g_y.detach().to(torch.float32).contiguous()
        g_t = torch.empty_like(tin)
        gw = [torch.empty_like(w) for w in (W1, b1, W2, b2)]
        ws = _workspace("wire_m2_combine_ws_bytes", dev, S, O, n)
        _lib.check(L.wire_m2_combine_bwd(_stream_ptr(dev), S, O, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                                         b2.data_ptr(), tin.data_ptr(), n, gy.data_ptr(), g_t.data_ptr(),
                                         *[g.data_ptr() for g in gw], ws.data_ptr(), ws.numel()), "wire_m2_combine_bwd")
        return (g_t, *gw)


def m2_combine(outputs: Sequence[torch.Tensor], W1, b1, W2, b2) -> torch.Tensor:
    """freq_mlp(cat(outputs, -1)) of bspline_mscale_2's combiner; outputs: S tensors of one shape [..., O]."""
    return _M2CombineFunction.apply(torch.stack(list(outputs)), W1, b1, W2, b2)


# The two Gabor layer forms, ComplexGaborLayer (modules/wire.py) over the parameters (W, b) and ComplexGaborLayer2D
# (modules/wire2d.py:56-67) over (W, b, V, c): the module's name in messages, the entry points, and what wire_*_fwd takes
# between is_first and act_out (wire_gabor_fwd's lin_out).  Everything else about a form is the length of its parameter
# tuple; a new form is a row here and its public wrappers.
_GABOR_FORMS = {
    "gabor": dict(name="ComplexGaborLayer", ws="wire_layer_ws_bytes", fwd="wire_gabor_fwd", fwd_extra=(None,),
                  bwd="wire_gabor_bwd", first_coords="wire_gabor_bwd_first_coords", hparam="wire_gabor_hparam_grad"),
    "gabor2d": dict(name="ComplexGaborLayer2D", ws="wire_layer2d_ws_bytes", fwd="wire_gabor2d_fwd", fwd_extra=(),
                    bwd="wire_gabor2d_bwd", first_coords="wire_gabor2d_bwd_first_coords",
                    hparam="wire_gabor2d_hparam_grad"),
}


class _GaborFunction(torch.autograd.Function):
    """One Gabor layer of either form on native tensors: wire_gabor*_fwd / wire_gabor*_bwd, or
    wire_gabor*_bwd_first_coords for a first layer whose coordinates require a gradient.  ``trainable``: omega and scale
    are the layer's omega_0 / scale_0 tensors (trainable=True, modules/wire.py:80-81, wire2d.py:42-43) instead of floats,
    and the backward adds wire_gabor*_hparam_grad for their two gradients."""

    @staticmethod
    def forward(ctx, form: str, trainable: bool, x, omega, scale, is_first: bool, *params):
        f = _GABOR_FORMS[form]
        hshapes = None
        if trainable:
            hshapes = (omega.shape, scale.shape)
            omega, scale = float(omega.detach().reshape(-1)[0]), float(scale.detach().reshape(-1)[0])
        _require_cuda(x, "layer input")
        _require_cuda(params[0], "layer weight")
        dev = x.device
        out_f, in_f = params[0].shape
        xin = x.detach().to(torch.float32 if is_first else torch.complex64).contiguous()
        n = xin.numel() // in_f
        nat = [_native(p) for p in params]
        ws = _workspace(f["ws"], dev, n, in_f, out_f)
        act = torch.empty(tuple(x.shape[:-1]) + (out_f,), dtype=torch.complex64, device=dev)
        _lib.check(getattr(_lib.lib(), f["fwd"])(_stream_ptr(dev), xin.data_ptr(), *[p.data_ptr() for p in nat], omega,
                                                 scale, n, in_f, out_f, int(is_first), *f["fwd_extra"], act.data_ptr(),
                                                 ws.data_ptr(), ws.numel()), f["fwd"])
        ctx.save_for_backward(xin, *nat)
        ctx.cfg = (f, omega, scale, is_first, n, in_f, out_f, tuple(x.shape), hshapes)
        ctx.xdtype = x.dtype
        return act

    @staticmethod
    def backward(ctx, g_act):
        L = _lib.lib()
        xin, *nat = ctx.saved_tensors
        f, omega0, scale0, is_first, n, in_f, out_f, xshape, hshapes = ctx.cfg
        dev = g_act.device
        g = g_act.detach().to(torch.complex64).contiguous()
        ws = _workspace(f["ws"], dev, n, in_f, out_f)
        grads = [torch.empty_like(p) for p in nat]
        # every backward entry point opens with `layer` and closes with `wsp`
        layer = (_stream_ptr(dev), g.data_ptr(), xin.data_ptr(), *[p.data_ptr() for p in nat], omega0, scale0, n, in_f,
                 out_f)
        gptr, wsp = [t.data_ptr() for t in grads], (ws.data_ptr(), ws.numel())
        if is_first and ctx.needs_input_grad[2]:
            gx = _first_coords(L, f, layer, gptr, wsp, n, in_f, dev).reshape(xshape).to(ctx.xdtype)
        else:
            gx = None if is_first else torch.empty(xshape, dtype=torch.complex64, device=dev)
            _lib.check(getattr(L, f["bwd"])(*layer, int(is_first), None if gx is None else gx.data_ptr(), *gptr, *wsp),
                       f["bwd"])
        g_hp = (None, None)
        if hshapes is not None:
            hp = torch.empty(2, dtype=torch.float32, device=dev)
            _lib.check(getattr(L, f["hparam"])(*layer, int(is_first), hp.data_ptr(), *wsp), f["hparam"])
            g_hp = (hp[0].reshape(hshapes[0]), hp[1].reshape(hshapes[1]))
        return (None, None, gx, *g_hp, None, *grads)


def _first_coords(L, f, layer, gptr, wsp, n, in_f, dev):
    """First Gabor layer with the coordinate gradient: wire_gabor*_bwd_first_coords (g_x = g_u W, + g_p V for the 2-D
    form); returns g_x [n, in_f] float32."""
    _no_second_order(f"{f['name']} (is_first)")
    gx = torch.empty(n, in_f, dtype=torch.float32, device=dev)
    _lib.check(getattr(L, f["first_coords"])(*layer, gx.data_ptr(), *gptr, *wsp), f["first_coords"])
    return gx


def gabor_layer(x, W, b, omega0: float, scale0: float, is_first: bool):
    return _GaborFunction.apply("gabor", False, x, float(omega0), float(scale0), bool(is_first), W, b)


def gabor_layer_trainable(x, W, b, omega: torch.Tensor, scale: torch.Tensor, is_first: bool):
    return _GaborFunction.apply("gabor", True, x, omega, scale, bool(is_first), W, b)


def gabor2d_layer(x, W, b, V, c, omega0: float, scale0: float, is_first: bool):
    return _GaborFunction.apply("gabor2d", False, x, float(omega0), float(scale0), bool(is_first), W, b, V, c)


def gabor2d_layer_trainable(x, W, b, V, c, omega: torch.Tensor, scale: torch.Tensor, is_first: bool):
    return _GaborFunction.apply("gabor2d", True, x, omega, scale, bool(is_first), W, b, V, c)


class _FinalLinearFunction(torch.autograd.Function):
    """Re(z W_f^T + b_f): wire_final_fwd / wire_final_bwd."""

    @staticmethod
    def forward(ctx, z, Wf, bf):
        L = _lib.lib()
        _require_cuda(z, "final-layer input")
        dev = z.device
        out_f, in_f = Wf.shape
        zin = z.detach().to(torch.complex64).contiguous()
        n = zin.numel() // in_f
        Wn, bn = _native(Wf), _native(bf)
        ws = _workspace("wire_layer_ws_bytes", dev, n, in_f, out_f)
        y = torch.empty(tuple(z.shape[:-1]) + (out_f,), dtype=torch.float32, device=dev)
        _lib.check(L.wire_final_fwd(_stream_ptr(dev), zin.data_ptr(), Wn.data_ptr(), bn.data_ptr(), n,
                                    in_f, out_f, y.data_ptr(), ws.data_ptr(), ws.numel()),
                   "wire_final_fwd")
        ctx.save_for_backward(zin, Wn)
        ctx.cfg = (n, in_f, out_f, tuple(z.shape), bn.shape)
        return y

    @staticmethod
    def backward(ctx, g_y):
        L = _lib.lib()
        zin, Wn = ctx.saved_tensors
        n, in_f, out_f, zshape, bshape = ctx.cfg
        dev = g_y.device
        gy = g_y.detach().to(torch.float32).contiguous()
        ws = _workspace("wire_layer_ws_bytes", dev, n, in_f, out_f)
        gz = torch.empty(zshape, dtype=torch.complex64, device=dev)
        gW = torch.empty_like(Wn)
        gb = torch.empty(bshape, dtype=torch.complex64, device=dev)
        _lib.check(L.wire_final_bwd(_stream_ptr(dev), gy.data_ptr(), zin.data_ptr(), Wn.data_ptr(), n,
                                    in_f, out_f, gz.data_ptr(), gW.data_ptr(), gb.data_ptr(),
                                    ws.data_ptr(), ws.numel()), "wire_final_bwd")
        return gz, gW, gb


def final_linear_real(z, Wf, bf):
    return _FinalLinearFunction.apply(z, Wf, bf)


class _RealLayerFunction(torch.autograd.Function):
    """SineLayer / GaussLayer / ReLULayer on native tensors: wire_real_layer_fwd / _bwd."""

    @staticmethod
    def forward(ctx, x, W, b, kind: str, omega0: float, scale0: float):
        L = _lib.lib()
        _require_cuda(x, "layer input")
        _require_cuda(W, "layer weight")
        dev = x.device
        out_f, in_f = W.shape
        xin = x.detach().to(torch.float32).contiguous()
        n = xin.numel() // in_f
        Wn, bn = _native(W), _native(b)
        ws = _workspace("wire_layer_ws_bytes", dev, n, in_f, out_f)
        act = torch.empty(tuple(x.shape[:-1]) + (out_f,), dtype=torch.float32, device=dev)
        _lib.check(L.wire_real_layer_fwd(_stream_ptr(dev), _lib.KIND[kind], xin.data_ptr(), Wn.data_ptr(),
                                         bn.data_ptr(), omega0, scale0, n, in_f, out_f, act.data_ptr(),
                                         ws.data_ptr(), ws.numel()), "wire_real_layer_fwd")
        ctx.save_for_backward(xin, Wn, bn)
        ctx.cfg = (kind, omega0, scale0, n, in_f, out_f, tuple(x.shape), x.requires_grad)
        return act

    @staticmethod
    def backward(ctx, g_act):
        L = _lib.lib()
        xin, Wn, bn = ctx.saved_tensors
        kind, omega0, scale0, n, in_f, out_f, xshape, need_gx = ctx.cfg
        dev = g_act.device
        g = g_act.detach().to(torch.float32).contiguous()
        ws = _workspace("wire_layer_ws_bytes", dev, n, in_f, out_f)
        gW = torch.empty_like(Wn)
        gb = torch.empty_like(bn)
        gx = torch.empty(xshape, dtype=torch.float32, device=dev) if need_gx else None
        _lib.check(L.wire_real_layer_bwd(_stream_ptr(dev), _lib.KIND[kind], g.data_ptr(), xin.data_ptr(),
                                         Wn.data_ptr(), bn.data_ptr(), omega0, scale0, n, in_f, out_f,
                                         None if gx is None else gx.data_ptr(), gW.data_ptr(), gb.data_ptr(),
                                         ws.data_ptr(), ws.numel()), "wire_real_layer_bwd")
        return gx, gW, gb, None, None, None


def real_layer(kind: str, x, W, b, omega0: float, scale0: float):
    return _RealLayerFunction.apply(x, W, b, kind, float(omega0), float(scale0))


class _MfnFilterFunction(torch.autograd.Function):
    """GaborLayer.forward of the multiplicative filter network (modules/mfn.py:24-26) on native tensors:
    wire_mfn_filter_fwd / wire_mfn_filter_bwd.  x [n][D] -> [n][K]."""

    @staticmethod
    def forward(ctx, x, mu, gamma, w, c):
        L = _lib.lib()
        _require_cuda(x, "layer input")
        _require_cuda(mu, "layer parameter")
        K, D = mu.shape
        xin = x.detach().to(torch.float32).contiguous()
        n = xin.shape[0]
        nat = [_native(t) for t in (mu, gamma, w, c)]
        out = torch.empty(n, K, dtype=torch.float32, device=x.device)
        if n > 0:
            _lib.check(L.wire_mfn_filter_fwd(_stream_ptr(x.device), xin.data_ptr(), *[t.data_ptr() for t in nat], n, D, K,
                                             out.data_ptr()), "wire_mfn_filter_fwd")
        ctx.save_for_backward(xin, *nat)
        ctx.xdtype = x.dtype
        return out

    @staticmethod
    def backward(ctx, g_out):
        L = _lib.lib()
        xin, mu, gamma, w, c = ctx.saved_tensors
        K, D = mu.shape
        n = xin.shape[0]
        dev = g_out.device
        g = g_out.detach().to(torch.float32).contiguous()
        grads = [torch.zeros_like(t) for t in (mu, gamma, w, c)]
        gx = None
        if ctx.needs_input_grad[0]:
            _no_second_order("mfn GaborLayer")
            gx = torch.zeros(n, D, dtype=torch.float32, device=dev)
        if n > 0:
            ws = _workspace("wire_mfn_filter_ws_bytes", dev, n, K)
            _lib.check(L.wire_mfn_filter_bwd(_stream_ptr(dev), g.data_ptr(), xin.data_ptr(), mu.data_ptr(),
                                             gamma.data_ptr(), w.data_ptr(), c.data_ptr(), n, D, K,
                                             *[t.data_ptr() for t in grads], None if gx is None else gx.data_ptr(),
                                             ws.data_ptr(), ws.numel()), "wire_mfn_filter_bwd")
        return (None if gx is None else gx.to(ctx.xdtype), *grads)


def mfn_filter(x, mu, gamma, w, c):
    return _MfnFilterFunction.apply(x, mu, gamma, w, c)


# ---------------------------------------------------------------------------
# structural similarity on the device (wire_ssim)
# ---------------------------------------------------------------------------
_SSIM_WINDOWS = {}


def _ssim_window(window):
    """(taps, fp32 weights as a ctypes array, cov_norm) of a window spec: "gaussian" = (11, 1.5), "uniform" = (7, None),
    or a (taps, sigma_or_None) tuple -- a Gaussian of that sigma, or ``taps`` equal weights with the sample covariance."""
    key = {"gaussian": (11, 1.5), "uniform": (7, None)}.get(window, window) if isinstance(window, str) else window
    if not (isinstance(key, tuple) and len(key) == 2 and isinstance(key[0], int)):
        raise ValueError(f"window must be 'gaussian', 'uniform' or a (taps, sigma_or_None) tuple, not {window!r}")
    taps, sigma = key
    if taps < 3 or taps > 11 or taps % 2 == 0:
        raise ValueError(f"a window has an odd number of taps in 3..11, not {taps}")
    if key not in _SSIM_WINDOWS:
        if sigma is None:
            w = torch.full((taps,), 1.0 / taps, dtype=torch.float32)
            cov = taps * taps / (taps * taps - 1.0)
        else:
            # pytorch_msssim's _fspecial_gauss_1d, in fp32 throughout
            coords = torch.arange(taps, dtype=torch.float32) - (taps // 2)
            w = torch.exp(-(coords ** 2) / (2 * float(sigma) ** 2))
            w = w / w.sum()
            cov = 1.0
        _SSIM_WINDOWS[key] = (taps, (C.c_float * taps)(*w.tolist()), cov)
    return _SSIM_WINDOWS[key]


def _ssim_check(rec, gt, H, W, window, data_range):
    """The argument checks ssim() and ssim_loss() share; returns (H, W, O, taps, window, cov_norm, c1, c2)."""
    taps, win, cov = _ssim_window(window)
    uniform = window == "uniform" or (isinstance(window, tuple) and window[1] is None)
    if data_range is None:
        if uniform:
            raise ValueError("window='uniform' (skimage.metrics.structural_similarity) needs data_range: skimage derives "
                             "it from the dtype, 2.0 for float images in the release the drivers were written against")
        data_range = 1.0
    H, W = int(H), int(W)
    if H < taps or W < taps:
        raise ValueError(f"a {H} x {W} image is smaller than the {taps}-tap window")
    if rec.numel() != gt.numel() or rec.numel() % (H * W) != 0:
        raise ValueError(f"rec ({rec.numel()}) and gt ({gt.numel()}) must both hold H*W*O = {H * W}*O elements")
    O = rec.numel() // (H * W)
    if not 1 <= O <= 8:
        raise ValueError(f"{O} channels: the library takes 1..8")
    for t in (rec, gt):
        if tuple(t.shape) not in ((H * W, O), (1, H * W, O), (H, W, O)):
            raise ValueError(f"shape {tuple(t.shape)} is none of [H*W, O], [1, H*W, O], [H, W, O]")
    _require_cuda(rec, "rec")
    _require_cuda(gt, "gt")
    if rec.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError("rec and gt must be float32")
    return H, W, O, taps, win, cov, (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2


def _ssim(rec, gt, H, W, window, data_range, full, ws=None):
    """ssim() with a workspace the caller may keep between calls; returns (result, workspace)."""
    H, W, O, taps, win, cov, c1, c2 = _ssim_check(rec, gt, H, W, window, data_range)
    L = _lib.lib()
    dev = rec.device
    x, y = gt.detach().contiguous(), rec.detach().contiguous()
    ws_bytes = _lib.check(L.wire_ssim_ws_bytes(H, W, O, taps), "wire_ssim_ws_bytes")
    if ws is None or ws.numel() < ws_bytes or ws.device != dev:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    smap = torch.empty(H - taps + 1, W - taps + 1, O, dtype=torch.float32, device=dev) if full else None
    _lib.check(L.wire_ssim(_stream_ptr(dev), x.data_ptr(), y.data_ptr(), H, W, O, taps, win, cov, c1, c2, out.data_ptr(),
                           None if smap is None else smap.data_ptr(), ws.data_ptr(), ws.numel()), "wire_ssim")
    return ((out, smap) if full else out), ws


def ssim(rec: torch.Tensor, gt: torch.Tensor, H: int, W: int, window="gaussian", data_range=None, full: bool = False):
    """Structural similarity of two images on the device (wire_ssim): no copy to the host, no transposed copy, no sync.

    ``rec`` and ``gt`` are CUDA float32 tensors of H*W*O elements in the trainer's layout -- [H*W, O], [1, H*W, O] or
    [H, W, O], channel last, O <= 8.  Returns a 0-dim device tensor, or ``(ssim, map)`` with ``full=True``, the map
    [H - taps + 1, W - taps + 1, O] over the valid region.

    ``window="gaussian"``: ``pytorch_msssim.ssim(gt, rec, data_range=1, size_average=True)`` as the super-resolution
    drivers call it every epoch -- 11 taps, sigma 1.5, normalised in fp32, population covariance; ``data_range``
    defaults to 1.0, what the drivers pass.
    ``window="uniform"``: ``skimage.metrics.structural_similarity(gt, rec, multichannel=True)`` with its defaults, the
    drivers' final report -- a 7 x 7 uniform filter, sample covariance (49/48), the border of 3 cropped.  ``data_range``
    must be given (ValueError otherwise): skimage derives it from the dtype, and 2.0 is what the release the drivers
    were written against (the one that still takes ``multichannel=``) derives for float images.
    A ``(taps, sigma_or_None)`` tuple selects another odd size in 3..11: a Gaussian, or equal weights with the sample
    covariance.

    CPU tensors raise WireHipError.  An image smaller than the window raises ValueError; this is stricter than
    pytorch_msssim, which warns and skips the smoothing along that axis."""
    return _ssim(rec, gt, H, W, window, data_range, full)[0]


class _SsimLossFunction(torch.autograd.Function):
    """1 - ssim(rec, gt) and its gradient with respect to rec: wire_ssim forward, wire_ssim_bwd backward."""

    @staticmethod
    def forward(ctx, rec, gt, cfg):
        H, W, O, taps, win, cov, c1, c2 = cfg
        L = _lib.lib()
        dev = rec.device
        x, y = gt.detach().contiguous(), rec.detach().contiguous()
        ws = _workspace("wire_ssim_ws_bytes", dev, H, W, O, taps)
        out = torch.empty((), dtype=torch.float32, device=dev)
        _lib.check(L.wire_ssim(_stream_ptr(dev), x.data_ptr(), y.data_ptr(), H, W, O, taps, win, cov, c1, c2,
                               out.data_ptr(), None, ws.data_ptr(), ws.numel()), "wire_ssim")
        ctx.save_for_backward(x, y)
        ctx.cfg = cfg
        ctx.rec_shape = tuple(rec.shape)
        return 1.0 - out

    @staticmethod
    def backward(ctx, g_loss):
        x, y = ctx.saved_tensors
        H, W, O, taps, win, cov, c1, c2 = ctx.cfg
        _no_second_order("ssim_loss")
        L = _lib.lib()
        dev = y.device
        g = (-g_loss.detach().to(torch.float32)).reshape(1).contiguous()      # d(1 - ssim) = -d ssim; read on the device
        ws = _workspace("wire_ssim_bwd_ws_bytes", dev, H, W, O, taps)
        gy = torch.empty(H * W * O, dtype=torch.float32, device=dev)
        _lib.check(L.wire_ssim_bwd(_stream_ptr(dev), x.data_ptr(), y.data_ptr(), H, W, O, taps, win, cov, c1, c2,
                                   g.data_ptr(), gy.data_ptr(), ws.data_ptr(), ws.numel()), "wire_ssim_bwd")
        return gy.reshape(ctx.rec_shape), None, None


def ssim_loss(rec: torch.Tensor, gt: torch.Tensor, H: int, W: int, window="gaussian", data_range=None) -> torch.Tensor:
    """``1 - ssim(rec, gt, H, W, window, data_range)`` as a 0-dim device tensor that is differentiable with respect to
    ``rec`` (only): the perceptual term of ``loss = mse + lambda * ssim_loss(...)``.  Forward is wire_ssim, backward
    wire_ssim_bwd -- one HIP launch, the closed-form gradient of the mean index gathered per input pixel, the upstream
    gradient read on the device (no sync), the same bits for the same call.  First order only.

    Shapes, dtypes, window specs, ``data_range`` and errors are those of ``ssim``; the gradient has the shape of
    ``rec``.  ``gt`` receives no gradient."""
    cfg = _ssim_check(rec, gt, H, W, window, data_range)
    return _SsimLossFunction.apply(rec, gt, cfg)


# ---------------------------------------------------------------------------
# total variation on the device (wire_tv_fwd / wire_tv_bwd)
# ---------------------------------------------------------------------------
def _tv_layout(x: torch.Tensor):
    """(pix_stride, plane_stride) of a (B, C, H, W) tensor whose element (b, c, i, j) lies at
    (b*C + c) * plane_stride + (i*W + j) * pix_stride with planes and pixels that do not overlap, or None.  A contiguous
    tensor gives (1, H*W); ``y.reshape(1, H, W, O).permute(0, 3, 1, 2)`` of a contiguous [H*W, O] gives (O, 1)."""
    B, Cn, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if W > 1:
        ps, ok = sw, H == 1 or sh == W * sw
    else:
        ps, ok = (sh if H > 1 else 1), True
    if Cn > 1:
        qs = sc
        ok = ok and (B == 1 or sb == Cn * sc)
    else:
        qs = sb if B > 1 else 1
    planes, npix = B * Cn, H * W
    ok = ok and ps >= 1 and qs >= 1 and (qs >= (npix - 1) * ps + 1 or ps >= (planes - 1) * qs + 1
                                         or planes == 1 or npix == 1)
    return (ps, qs) if ok else None


class _TotalVariationFunction(torch.autograd.Function):
    """tv(x) of a (B, C, H, W) tensor and its gradient: wire_tv_fwd / wire_tv_bwd on the tensor's own memory when its
    strides have the (pix_stride, plane_stride) form, on a contiguous copy otherwise."""

    @staticmethod
    def forward(ctx, x):
        L = _lib.lib()
        xin = x.detach()
        lay = _tv_layout(xin)
        if lay is None:
            xin = xin.contiguous()
            lay = _tv_layout(xin)
        B, Cn, H, W = xin.shape
        out = torch.empty((), dtype=torch.float32, device=xin.device)
        partial = torch.empty(1024, dtype=torch.float32, device=xin.device)
        _lib.check(L.wire_tv_fwd(_stream_ptr(xin.device), xin.data_ptr(), B * Cn, H, W, lay[0], lay[1], out.data_ptr(),
                                 partial.data_ptr()), "wire_tv_fwd")
        ctx.save_for_backward(xin)
        ctx.lay = lay
        return out

    @staticmethod
    def backward(ctx, g_tv):
        L = _lib.lib()
        xin, = ctx.saved_tensors
        B, Cn, H, W = xin.shape
        _no_second_order("total_variation")
        g = g_tv.detach().to(torch.float32).reshape(1).contiguous()
        gx = torch.empty_strided(xin.shape, xin.stride(), dtype=torch.float32, device=xin.device)
        _lib.check(L.wire_tv_bwd(_stream_ptr(xin.device), xin.data_ptr(), B * Cn, H, W, ctx.lay[0], ctx.lay[1],
                                 g.data_ptr(), gx.data_ptr()), "wire_tv_bwd")
        return gx


def total_variation(x: torch.Tensor) -> torch.Tensor:
    """Anisotropic total variation of a (B, C, H, W) CUDA float32 tensor on the device, the reference's
    ``utils.total_variation_loss`` (modules/utils.py:360-369):
    ``sum |x[:, :, 1:, :] - x[:, :, :-1, :]| + sum |x[:, :, :, 1:] - x[:, :, :, :-1]|`` -- a sum, not a mean -- as a 0-dim
    device tensor, differentiable with respect to ``x`` with torch's ``d|u|/du = sign(u)`` (0 at a tie).  One HIP pass
    forward and one backward (the upstream gradient is read on the device: no sync).  A tensor whose strides have the
    form (b*C + c) * plane_stride + (i*W + j) * pix_stride is read where it lies -- a contiguous tensor, and the drivers'
    ``model(coords).reshape(1, H, W, O).permute(0, 3, 1, 2)`` view of the network's [H*W, O] output -- anything else is
    made contiguous first.  First order only.  CPU tensors raise WireHipError; other ranks or dtypes ValueError."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.numel() == 0:
        raise ValueError("total_variation expects a non-empty (B, C, H, W) tensor")
    _require_cuda(x, "image")
    if x.dtype != torch.float32:
        raise ValueError("image must be float32")
    return _TotalVariationFunction.apply(x)


# ---------------------------------------------------------------------------
# pointwise data terms with a per-sample weight (wire_point_loss_grad)
# ---------------------------------------------------------------------------
def _loss_kind(kind, delta):
    """(enum wire_loss_kind, delta as a float) of a data term named "mse" | "l1" | "huber" | "logistic"; ``delta`` is
    Huber's width and is checked for that kind alone."""
    if not isinstance(kind, str) or kind not in _lib.LOSS_KIND:
        raise ValueError(f"kind {kind!r}: one of {', '.join(repr(k) for k in _lib.LOSS_KIND)}")
    delta = float(delta)
    if kind == "huber" and not (delta > 0.0 and delta != float("inf")):
        raise ValueError(f"delta must be finite and > 0 for the Huber loss, not {delta}")
    return _lib.LOSS_KIND[kind], delta


def _loss_weight(weight, n: int, O: int, like: torch.Tensor, rows: str = "n"):
    """An optional weight table -> (detached tensor or None, weight_per_elem): [n] is one weight per row, [n, O] one per
    element; contiguous float32 on the device of ``like``."""
    if weight is None:
        return None, 0
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or not weight.is_contiguous() \
            or tuple(weight.shape) not in ((n,), (n, O)) or weight.device != like.device:
        raise ValueError(f"weight must be a contiguous float32 tensor [{rows}] or [{rows}, {O}] on the device of the "
                         "outputs")
    return weight.detach(), int(weight.dim() == 2)


class _PointLossFunction(torch.autograd.Function):
    """loss and dL/dy in one launch of wire_point_loss_grad; backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, y, target, weight, cfg):
        code, delta, wpe = cfg
        L = _lib.lib()
        dev = y.device
        yd = y.detach()
        n, O = int(yd.shape[0]), int(yd.shape[1])
        out = torch.empty((), dtype=torch.float32, device=dev)
        gy = torch.empty_like(yd)
        partial = torch.empty(4096, dtype=torch.float32, device=dev)
        _lib.check(L.wire_point_loss_grad(_stream_ptr(dev), code, delta, yd.data_ptr(), target.data_ptr(),
                                          weight.data_ptr() if weight is not None else None, wpe, None, 0, n, O, 1.0,
                                          gy.data_ptr(), out.data_ptr(), None, partial.data_ptr()),
                   "wire_point_loss_grad")
        ctx.save_for_backward(gy)
        return out

    @staticmethod
    def backward(ctx, g_loss):
        gy, = ctx.saved_tensors
        _no_second_order("point_loss")
        return g_loss.detach().to(torch.float32) * gy, None, None, None


def point_loss(y: torch.Tensor, target: torch.Tensor, kind: str = "mse", weight=None, delta: float = 1.0) -> torch.Tensor:
    """A pointwise data term of the outputs ``y`` [n, O] against ``target`` [n, O] as a 0-dim device tensor,
    ``sum_e w_e rho(y_e - t_e) / (n O)`` with rho by ``kind``:

        "mse"       d^2                                       torch.nn.MSELoss
        "l1"        |d|, gradient sign(d) with +0 at a tie     torch.nn.L1Loss
        "huber"     d^2 / 2 up to |d| = delta, linear beyond   torch.nn.HuberLoss(delta=delta)
        "logistic"  max(z,0) - t z + log1p(exp(-|z|)), z = y   torch.nn.BCEWithLogitsLoss (y a logit, target in [0, 1])

    ``weight`` is None, [n] (one per row) or [n, O] (one per element, a Bayer mosaic), any finite values; the mean runs
    over every element, those of weight 0 included (``MSELoss()(out * mask, gt * mask)``), so scale the weights for a
    mean over the kept ones.  All tensors contiguous CUDA float32.  One HIP launch (wire_point_loss_grad) gives the loss
    and dL/dy together; backward multiplies the stored gradient by the upstream scalar on the device (no sync).  The
    gradient flows to ``y`` only; first order only.  No atomics: the same call gives the same bits.  CPU tensors raise
    WireHipError; other dtypes, shapes, kinds or a bad ``delta`` ValueError, before any device access."""
    cfg = _loss_kind(kind, delta)
    if not isinstance(y, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise ValueError("point_loss expects two tensors")
    if y.dtype != torch.float32 or y.dim() != 2 or y.shape[0] < 1 or y.shape[1] < 1 or not y.is_contiguous():
        raise ValueError("y must be a contiguous float32 tensor [n, O] with n, O >= 1")
    if target.dtype != torch.float32 or target.shape != y.shape or not target.is_contiguous() \
            or target.device != y.device:
        raise ValueError(f"target must be a contiguous float32 tensor {list(y.shape)} on the device of y")
    w, wpe = _loss_weight(weight, int(y.shape[0]), int(y.shape[1]), y)
    _require_cuda(y, "y")
    return _PointLossFunction.apply(y, target.detach(), w, cfg + (wpe,))


# ---------------------------------------------------------------------------
# volume rendering: ray sampling and emission-absorption compositing (wire_render.hip)
# ---------------------------------------------------------------------------
def _density_mode(density) -> int:
    if not isinstance(density, str) or density not in _lib.DENSITY_MODE:
        raise ValueError(f"density {density!r}: one of {', '.join(repr(k) for k in _lib.DENSITY_MODE)}")
    return _lib.DENSITY_MODE[density]


def _ray_args(rays, near, far, n_samples, jitter):
    """The argument checks of the ray entry points -> (rays, bounds [R, 2] or None, near, far, R, S, jitter), detached
    and contiguous.  ``near`` / ``far`` are two finite numbers or two [R] tensors."""
    if not isinstance(rays, torch.Tensor) or rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[0] < 1 \
            or rays.shape[1] != 6 or not rays.is_contiguous():
        raise ValueError("rays must be a contiguous float32 tensor [R, 6] with R >= 1")
    R, S = int(rays.shape[0]), int(n_samples)
    if S < 1:
        raise ValueError("n_samples must be >= 1")
    tn, tf = isinstance(near, torch.Tensor), isinstance(far, torch.Tensor)
    if tn != tf:
        raise ValueError("near and far must both be numbers or both be [R] tensors")
    if tn:
        for name, t in (("near", near), ("far", far)):
            if t.dtype != torch.float32 or tuple(t.shape) != (R,) or t.device != rays.device:
                raise ValueError(f"{name} must be a float32 tensor [{R}] on the device of rays")
    else:
        near, far = float(near), float(far)
        if near != near or far != far or abs(near) == float("inf") or abs(far) == float("inf"):
            raise ValueError("near and far must be finite")
    if jitter is not None and (not isinstance(jitter, torch.Tensor) or jitter.dtype != torch.float32
                               or tuple(jitter.shape) != (R, S) or not jitter.is_contiguous()
                               or jitter.device != rays.device):
        raise ValueError(f"jitter must be a contiguous float32 tensor [{R}, {S}] on the device of rays")
    _require_cuda(rays, "rays")
    bounds = torch.stack([near.detach(), far.detach()], dim=1).contiguous() if tn else None
    return rays.detach(), bounds, (0.0 if tn else near), (0.0 if tn else far), R, S, \
        (jitter.detach() if jitter is not None else None)


def _background_arg(background, Cc: int, dev: torch.device):
    """``background`` None, a number, or [C] values -> a float32 [C] tensor on ``dev`` or None."""
    if background is None:
        return None
    bg = torch.as_tensor(background, dtype=torch.float32).detach()
    if bg.dim() == 0:
        bg = bg.expand(Cc)
    if tuple(bg.shape) != (Cc,):
        raise ValueError(f"background must be None, a number or {Cc} values")
    return bg.to(dev).contiguous()


def _ray_samples_into(stream, rays, bounds, near, far, jitter, R, S, coords, ts, deltas) -> None:
    _lib.check(_lib.lib().wire_ray_samples(stream, rays.data_ptr(), bounds.data_ptr() if bounds is not None else None,
                                           near, far, jitter.data_ptr() if jitter is not None else None, R, S,
                                           coords.data_ptr(), ts.data_ptr(), deltas.data_ptr()), "wire_ray_samples")


@torch.no_grad()
def ray_samples(rays: torch.Tensor, near, far, n_samples: int, jitter=None):
    """The sample points of R rays: ``rays`` [R, 6] = (origin, direction) (``utils.get_rays``), ``near`` / ``far`` two
    numbers or two [R] tensors (``utils.ray_box``), S = ``n_samples`` stratified samples per ray,

        t_s = near + (s + u_s) (far - near) / S,    u = ``jitter`` [R, S] in [0, 1) (``torch.rand``) or 0.5 (None)

    Returns ``(coords [R*S, 3], ts [R, S], deltas [R, S])``: the net's input rows ``o + t_s d``, the parameters, and
    the world-space lengths ``(t_{s+1} - t_s) |d|`` with ``far`` behind the last sample.  A ray with ``far <= near``
    gets zero lengths: it composites to the background and receives no gradient.  fp64 arithmetic rounded to fp32
    once (wire_ray_samples).  No gradient.  Contiguous CUDA float32 tensors; CPU tensors raise WireHipError, other
    shapes or dtypes ValueError."""
    r, bounds, nr, fr, R, S, u = _ray_args(rays, near, far, n_samples, jitter)
    dev = r.device
    coords = torch.empty(R * S, 3, dtype=torch.float32, device=dev)
    ts = torch.empty(R, S, dtype=torch.float32, device=dev)
    deltas = torch.empty(R, S, dtype=torch.float32, device=dev)
    _ray_samples_into(_stream_ptr(dev), r, bounds, nr, fr, u, R, S, coords, ts, deltas)
    return coords, ts, deltas


class _CompositeFunction(torch.autograd.Function):
    """wire_composite_fwd and its adjoint wire_composite_bwd."""

    @staticmethod
    def forward(ctx, y, ts, deltas, bg, mode):
        L = _lib.lib()
        yd = y.detach()
        if yd.data_ptr() % 16:                     # the kernels move a row as 16- or 8-byte words
            yd = yd.clone()
        dev = yd.device
        R, S, O = int(ts.shape[0]), int(ts.shape[1]), int(yd.shape[-1])
        rgb = torch.empty(R, O - 1, dtype=torch.float32, device=dev)
        acc = torch.empty(R, dtype=torch.float32, device=dev)
        depth = torch.empty(R, dtype=torch.float32, device=dev)
        _lib.check(L.wire_composite_fwd(_stream_ptr(dev), yd.data_ptr(), ts.data_ptr(), deltas.data_ptr(),
                                        bg.data_ptr() if bg is not None else None, R, S, O, mode, rgb.data_ptr(),
                                        acc.data_ptr(), depth.data_ptr()), "wire_composite_fwd")
        ctx.save_for_backward(yd, ts, deltas)
        ctx.bg, ctx.mode, ctx.shape = bg, mode, tuple(y.shape)
        return rgb, acc, depth

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth):
        L = _lib.lib()
        yd, ts, deltas = ctx.saved_tensors
        _no_second_order("composite")
        dev = yd.device
        R, S, O = int(ts.shape[0]), int(ts.shape[1]), int(yd.shape[-1])
        as_f32 = lambda g: None if g is None else g.detach().to(torch.float32).contiguous()
        g_rgb, g_acc, g_depth = as_f32(g_rgb), as_f32(g_acc), as_f32(g_depth)
        if g_rgb is None:
            g_rgb = torch.zeros(R, O - 1, dtype=torch.float32, device=dev)
        g_y = torch.empty(R * S, O, dtype=torch.float32, device=dev)
        opt = lambda t: t.data_ptr() if t is not None else None
        _lib.check(L.wire_composite_bwd(_stream_ptr(dev), yd.data_ptr(), ts.data_ptr(), deltas.data_ptr(), opt(ctx.bg),
                                        g_rgb.data_ptr(), opt(g_acc), opt(g_depth), R, S, O, ctx.mode, g_y.data_ptr()),
                   "wire_composite_bwd")
        return g_y.view(ctx.shape), None, None, None, None


def composite(y: torch.Tensor, ts: torch.Tensor, deltas: torch.Tensor, background=None, density: str = "softplus"):
    """Emission-absorption compositing of the net's rows along R rays of S samples: ``y`` [R*S, O] (or [R, S, O]) holds
    ``(c_raw[0..C), s_raw)`` per sample, C = O - 1, O in 2..8; ``ts`` and ``deltas`` [R, S] come from ``ray_samples``.

        sigma = softplus(s_raw) ("softplus") or max(s_raw, 0) ("relu"),    c = sigmoid(c_raw)
        T_s = exp(-sum_{j<s} sigma_j delta_j),    w_s = T_s (1 - exp(-sigma_s delta_s))
        rgb = sum_s w_s c_s + T_S background,    acc = 1 - T_S,    depth = sum_s w_s t_s

    Returns ``(rgb [R, C], acc [R], depth [R])``.  ``background`` is None (black), a number or [C] values.  Forward
    is wire_composite_fwd and backward wire_composite_bwd: a wave per ray, optical depth and transmittance in fp64, no
    [R, S] temporaries and no atomics (the same call gives the same bits).  The gradient reaches ``y`` only: ``ts`` or
    ``deltas`` that require grad, and second-order use, raise NotImplementedError.  Contiguous CUDA float32 tensors;
    CPU tensors raise WireHipError, other shapes or dtypes ValueError."""
    mode = _density_mode(density)
    if not all(isinstance(t, torch.Tensor) for t in (y, ts, deltas)):
        raise ValueError("composite expects three tensors")
    if ts.dtype != torch.float32 or ts.dim() != 2 or ts.shape[0] < 1 or ts.shape[1] < 1 or not ts.is_contiguous():
        raise ValueError("ts must be a contiguous float32 tensor [R, S] with R, S >= 1")
    R, S = int(ts.shape[0]), int(ts.shape[1])
    if deltas.dtype != torch.float32 or deltas.shape != ts.shape or not deltas.is_contiguous() \
            or deltas.device != ts.device:
        raise ValueError(f"deltas must be a contiguous float32 tensor [{R}, {S}] on the device of ts")
    if y.dtype != torch.float32 or y.dim() not in (2, 3) or not y.is_contiguous() or y.device != ts.device \
            or tuple(y.shape[:-1]) not in ((R * S,), (R, S)) or not 2 <= y.shape[-1] <= 8:
        raise ValueError(f"y must be a contiguous float32 tensor [{R * S}, O] or [{R}, {S}, O], O in 2..8, on the device "
                         "of ts")
    bg = _background_arg(background, int(y.shape[-1]) - 1, y.device)
    if torch.is_grad_enabled() and (ts.requires_grad or deltas.requires_grad):
        raise NotImplementedError("composite: the gradient reaches y only; ts and deltas that require grad are not "
                                  "supported (detach them)")
    _require_cuda(y, "y")
    return _CompositeFunction.apply(y, ts.detach(), deltas.detach(), bg, mode)


RESAMPLE_MAX = 1024            # wire_ray_resample keeps a ray's CDF and lists in LDS: S and Nf up to here


def _composite_weights_into(stream, y, deltas, R, S, O, mode, w) -> None:
    _lib.check(_lib.lib().wire_composite_weights(stream, y.data_ptr(), deltas.data_ptr(), R, S, O, mode, w.data_ptr()),
               "wire_composite_weights")


def _ray_resample_into(stream, rays, bounds, near, far, ts_c, w, jitter, eps, R, S, Nf, coords, ts, deltas) -> None:
    _lib.check(_lib.lib().wire_ray_resample(stream, rays.data_ptr(), bounds.data_ptr() if bounds is not None else None,
                                            near, far, ts_c.data_ptr(), w.data_ptr(),
                                            jitter.data_ptr() if jitter is not None else None, eps, R, S, Nf,
                                            coords.data_ptr(), ts.data_ptr(), deltas.data_ptr()), "wire_ray_resample")


def _resample_args(n_samples: int, n_importance: int, eps) -> float:
    """The limits of wire_ray_resample on S, Nf and eps -> eps as a float."""
    if not 1 <= int(n_samples) <= RESAMPLE_MAX or not 1 <= int(n_importance) <= RESAMPLE_MAX:
        raise ValueError(f"resampling takes 1..{RESAMPLE_MAX} coarse samples and 1..{RESAMPLE_MAX} fine samples per ray")
    eps = float(eps)
    if not 0.0 < eps < float("inf"):
        raise ValueError("eps must be a finite number > 0")
    return eps


@torch.no_grad()
def composite_weights(y: torch.Tensor, deltas: torch.Tensor, density: str = "softplus") -> torch.Tensor:
    """The compositing weights ``w_s = T_s (1 - exp(-sigma_s delta_s))`` of ``composite``, [R, S]: the summand of its
    ``rgb`` and ``acc``, from ``y`` [R*S, O] (or [R, S, O]; only the density column is read) and ``deltas`` [R, S], with
    the forward sweep's fp64 scan (wire_composite_weights).  They say where along a ray the colour came from, which is
    what ``ray_resample`` draws its second set of samples from.  No gradient: a ``y`` that requires grad is detached.
    Contiguous CUDA float32 tensors; CPU tensors raise WireHipError, other shapes or dtypes ValueError."""
    mode = _density_mode(density)
    if not isinstance(y, torch.Tensor) or not isinstance(deltas, torch.Tensor):
        raise ValueError("composite_weights expects two tensors")
    if deltas.dtype != torch.float32 or deltas.dim() != 2 or deltas.shape[0] < 1 or deltas.shape[1] < 1 \
            or not deltas.is_contiguous():
        raise ValueError("deltas must be a contiguous float32 tensor [R, S] with R, S >= 1")
    R, S = int(deltas.shape[0]), int(deltas.shape[1])
    if y.dtype != torch.float32 or y.dim() not in (2, 3) or not y.is_contiguous() or y.device != deltas.device \
            or tuple(y.shape[:-1]) not in ((R * S,), (R, S)) or not 2 <= y.shape[-1] <= 8:
        raise ValueError(f"y must be a contiguous float32 tensor [{R * S}, O] or [{R}, {S}, O], O in 2..8, on the device "
                         "of deltas")
    _require_cuda(y, "y")
    yd = y.detach()
    if yd.data_ptr() % 16:
        yd = yd.clone()
    w = torch.empty(R, S, dtype=torch.float32, device=yd.device)
    _composite_weights_into(_stream_ptr(yd.device), yd, deltas.detach(), R, S, int(yd.shape[-1]), mode, w)
    return w


@torch.no_grad()
def ray_resample(rays: torch.Tensor, near, far, ts: torch.Tensor, weights: torch.Tensor, n_importance: int,
                 jitter=None, eps: float = 1e-5):
    """Hierarchical sampling: ``n_importance`` = Nf further samples per ray, drawn where the coarse pass found something,
    merged with the coarse samples.  ``rays``, ``near`` / ``far`` as ``ray_samples``; ``ts`` [R, S] its coarse samples
    (nondecreasing inside [near, far]; not checked) and ``weights`` [R, S] their ``composite_weights``.  The bins are
    bounded by ``near``, the midpoints of consecutive coarse samples and ``far``, so that bin s surrounds sample s; the
    mass of a bin is ``max(w_s, 0) + eps`` (``eps``: NeRF's ``sample_pdf`` constant), and draw k inverts the piecewise
    linear CDF at ``(k + v_k) / Nf`` of the total, ``v`` = ``jitter`` [R, Nf] in [0, 1) (``torch.rand``) or 0.5 (None).

    Returns ``(coords [R*(S+Nf), 3], ts [R, S+Nf], deltas [R, S+Nf])`` of the sorted union, in ``ray_samples``'
    conventions (``far`` behind the last sample; a ray with ``far <= near`` gets zero lengths).  fp64 arithmetic rounded
    to fp32 once, no atomics: the same call gives the same bits (wire_ray_resample).  S and Nf up to 1024.  No gradient.
    Contiguous CUDA float32 tensors; CPU tensors raise WireHipError, other shapes or dtypes ValueError."""
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2:               # (_ray_args checks the rest of rays)
        raise ValueError("rays must be a contiguous float32 tensor [R, 6] with R >= 1")
    R = int(rays.shape[0])
    if not isinstance(ts, torch.Tensor) or ts.dtype != torch.float32 or ts.dim() != 2 or ts.shape[0] != R \
            or ts.shape[1] < 1 or not ts.is_contiguous() or ts.device != rays.device:
        raise ValueError(f"ts must be a contiguous float32 tensor [{R}, S] with S >= 1 on the device of rays")
    S = int(ts.shape[1])
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.shape != ts.shape \
            or not weights.is_contiguous() or weights.device != rays.device:
        raise ValueError(f"weights must be a contiguous float32 tensor [{R}, {S}] on the device of rays")
    eps = _resample_args(S, n_importance, eps)
    r, bounds, nr, fr, R, Nf, v = _ray_args(rays, near, far, n_importance, jitter)
    dev = r.device
    coords = torch.empty(R * (S + Nf), 3, dtype=torch.float32, device=dev)
    ts_out = torch.empty(R, S + Nf, dtype=torch.float32, device=dev)
    deltas = torch.empty(R, S + Nf, dtype=torch.float32, device=dev)
    _ray_resample_into(_stream_ptr(dev), r, bounds, nr, fr, ts.detach(), weights.detach(), v, eps, R, S, Nf, coords,
                       ts_out, deltas)
    return coords, ts_out, deltas


# ---------------------------------------------------------------------------
# a learnable registration of frames (wire_warp_coords_fwd / wire_warp_coords_bwd)
# ---------------------------------------------------------------------------
class _WarpCoordsFunction(torch.autograd.Function):
    """theta[f] (x, y, 1) of every row of frame f and its adjoint: wire_warp_coords_fwd / wire_warp_coords_bwd."""

    @staticmethod
    def forward(ctx, coords, theta):
        L = _lib.lib()
        x, t = coords.detach(), theta.detach()
        if x.data_ptr() % 8:                      # the kernels move a row as one 8-byte word
            x = x.clone()
        B, n_per = int(x.shape[0]), int(x.shape[1])
        out = torch.empty_like(x)
        _lib.check(L.wire_warp_coords_fwd(_stream_ptr(x.device), x.data_ptr(), t.data_ptr(), B, n_per, out.data_ptr()),
                   "wire_warp_coords_fwd")
        ctx.save_for_backward(x, t)
        return out

    @staticmethod
    def backward(ctx, g_out):
        L = _lib.lib()
        x, t = ctx.saved_tensors
        _no_second_order("warp_coords")
        B, n_per = int(x.shape[0]), int(x.shape[1])
        g = g_out.detach().to(torch.float32).contiguous()
        if g.data_ptr() % 8:
            g = g.clone()
        g_theta = torch.empty_like(t)
        g_in = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ws = _workspace("wire_warp_coords_bwd_ws_bytes", x.device, B, n_per)
        _lib.check(L.wire_warp_coords_bwd(_stream_ptr(x.device), x.data_ptr(), t.data_ptr(), g.data_ptr(), B, n_per, 0,
                                          g_theta.data_ptr(), g_in.data_ptr() if g_in is not None else None,
                                          ws.data_ptr(), ws.numel()), "wire_warp_coords_bwd")
        return g_in, g_theta


def warp_coords(coords: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """The coordinates of B frames, each moved by its own learnable 2 x 3 matrix: ``out[f, p] = theta[f] @ (x, y, 1)``
    for ``(x, y) = coords[f, p]``, the convention of ``motion.get_transformed_coords`` / ``F.affine_grid`` (``theta``
    acts on NORMALISED coordinates; the identity ``[[1, 0, 0], [0, 1, 0]]`` returns ``coords`` bit for bit).
    ``coords``: [B, n, 2], ``theta``: [B, 2, 3], both contiguous CUDA float32.  Returns a new [B, n, 2] tensor that is
    differentiable with respect to ``theta``, and to ``coords`` when they require a gradient: feed it to a model and a
    torch optimiser refines the registration with the net.  Forward is wire_warp_coords_fwd, backward
    wire_warp_coords_bwd -- fp64 arithmetic rounded to fp32 once, a deterministic reduction to the six numbers of
    every frame (no atomics: the same call gives the same bits), no frame pinned (zero ``theta.grad[0]`` or leave frame 0
    out of the optimiser to fix the gauge).  First order only.  CPU tensors raise WireHipError; other shapes, dtypes
    or strides ValueError."""
    if not isinstance(coords, torch.Tensor) or not isinstance(theta, torch.Tensor):
        raise ValueError("warp_coords expects two tensors")
    _require_cuda(coords, "coords")
    _require_cuda(theta, "theta")
    if coords.dtype != torch.float32 or coords.dim() != 3 or coords.shape[0] < 1 or coords.shape[1] < 1 \
            or coords.shape[2] != 2 or not coords.is_contiguous():
        raise ValueError("coords must be a contiguous float32 tensor [B, n, 2] with B, n >= 1")
    if theta.dtype != torch.float32 or tuple(theta.shape) != (coords.shape[0], 2, 3) or not theta.is_contiguous():
        raise ValueError(f"theta must be a contiguous float32 tensor [{coords.shape[0]}, 2, 3]")
    if theta.device != coords.device:
        raise ValueError("coords and theta must be on the same device")
    return _WarpCoordsFunction.apply(coords, theta)


# ---------------------------------------------------------------------------
# registering frames from their intensities: the bilinear resampler and one Gauss-Newton iteration (wire_register.hip)
# ---------------------------------------------------------------------------
class _RemapFunction(torch.autograd.Function):
    """Bilinear samples of an image at given coordinates and their coordinate gradient: wire_remap_bilinear_fwd /
    wire_remap_bilinear_bwd_xy."""

    @staticmethod
    def forward(ctx, img, xy, normalized):
        L = _lib.lib()
        im, x = img.detach(), xy.detach()
        if x.data_ptr() % 8:                      # the kernels move a coordinate pair as one 8-byte word
            x = x.clone()
        H, W, Cc = (int(v) for v in im.shape)
        n = x.numel() // 2
        out = torch.empty(tuple(x.shape[:-1]) + (Cc,), dtype=torch.float32, device=x.device)
        _lib.check(L.wire_remap_bilinear_fwd(_stream_ptr(x.device), im.data_ptr(), H, W, Cc, x.data_ptr(), n,
                                             int(normalized), out.data_ptr()), "wire_remap_bilinear_fwd")
        ctx.save_for_backward(im, x)
        ctx.normalized = int(normalized)
        return out

    @staticmethod
    def backward(ctx, g_out):
        L = _lib.lib()
        im, x = ctx.saved_tensors
        _no_second_order("remap")
        H, W, Cc = (int(v) for v in im.shape)
        g = g_out.detach().to(torch.float32).contiguous()
        g_xy = torch.empty_like(x)
        _lib.check(L.wire_remap_bilinear_bwd_xy(_stream_ptr(x.device), im.data_ptr(), H, W, Cc, x.data_ptr(),
                                                g.data_ptr(), x.numel() // 2, ctx.normalized, g_xy.data_ptr()),
                   "wire_remap_bilinear_bwd_xy")
        return None, g_xy, None


def remap(img: torch.Tensor, xy: torch.Tensor, normalized: bool = False) -> torch.Tensor:
    """Bilinear samples of ``img`` [H, W, C] (channel last, C = 1..8) at ``xy`` [..., 2] = (x, y): a new [..., C] tensor.

    ``normalized=False``: pixel coordinates with pixel centres at integers, ``cv2.remap(img, x, y, INTER_LINEAR)`` with
    ``BORDER_CONSTANT`` 0 -- but with exact weights, where cv2 quantises them to 1/32 pixel.  ``normalized=True``:
    ``F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False)``.  Taps outside the image contribute 0;
    a NaN or infinite coordinate gives 0 and a zero gradient.  fp64 arithmetic rounded to fp32 once
    (wire_remap_bilinear_fwd); the gradient reaches ``xy`` only (wire_remap_bilinear_bwd_xy: the derivative of the
    interpolant on the cell chosen by ``floor``, first order only).  There is no adjoint with respect to the image -- a
    general warp's would need atomics, and this library's adjoints are deterministic gathers -- so an ``img`` that
    requires grad raises NotImplementedError.  Contiguous CUDA float32 tensors; CPU tensors raise WireHipError."""
    if not isinstance(img, torch.Tensor) or not isinstance(xy, torch.Tensor):
        raise ValueError("remap expects two tensors")
    if normalized not in (False, True, 0, 1):
        raise ValueError("normalized must be a bool")
    if img.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(
            "remap: the gradient reaches xy only; there is no adjoint with respect to the image (a general warp's would "
            "need atomics, and this library's adjoints are deterministic gathers). Detach img.")
    _require_cuda(img, "img")
    _require_cuda(xy, "xy")
    if img.dtype != torch.float32 or img.dim() != 3 or min(img.shape) < 1 or not 1 <= img.shape[2] <= 8 \
            or not img.is_contiguous():
        raise ValueError("img must be a contiguous float32 tensor [H, W, C] with C in 1..8")
    if xy.dtype != torch.float32 or xy.dim() < 1 or xy.shape[-1] != 2 or xy.numel() < 2 or not xy.is_contiguous():
        raise ValueError("xy must be a contiguous float32 tensor [..., 2] with at least one row")
    if xy.device != img.device:
        raise ValueError("img and xy must be on the same device")
    return _RemapFunction.apply(img, xy, bool(normalized))


def _motion_model(model) -> int:
    if isinstance(model, str) and model in _lib.MOTION_MODEL:
        return _lib.MOTION_MODEL[model]
    if not isinstance(model, (bool, str)) and model in (0, 1, 2):
        return int(model)
    if not isinstance(model, (bool, str)) and model == 3:
        raise NotImplementedError("homography registration is out of scope: translation, euclidean or affine")
    raise ValueError(f"model must be one of {sorted(_lib.MOTION_MODEL)} (or cv2's 0 / 1 / 2), not {model!r}")


def register_gn_step(ref: torch.Tensor, frames: torch.Tensor, mats: torch.Tensor, weight=None, model="euclidean",
                     damping: float = 0.0, min_cover: float = 0.0, ws=None) -> torch.Tensor:
    """One Gauss-Newton iteration of the intensity registration of ``frames`` [B, H, W] onto ``ref`` [H, W]
    (wire_register_gn_step): ``mats`` -- CUDA float64 [B, K, 2, 3], pixel units, K start candidates per frame -- is
    UPDATED IN PLACE towards the minimum of ``sum w (ref(M (j, i, 1)) - frame(i, j))^2`` and the float64 stats
    [B, K, 4] = (mean weighted squared residual at the INPUT matrix, covered weight per pixel, step norm, valid) are
    returned.  ``weight``: [B, H, W] float32 or None.  ``model``: "translation" | "euclidean" | "affine" (or cv2's 0 / 1 /
    2).  An invalid candidate (singular system, covered fraction < ``min_cover``, non-finite values) keeps its matrix.
    No host synchronisation.  ``ws``: a uint8 workspace of wire_register_gn_ws_bytes(B, K, H, W) bytes to reuse across
    calls; after the call its first B * K * 29 doubles hold the normal equations' sums."""
    m = _motion_model(model)
    for t, what in ((ref, "ref"), (frames, "frames"), (mats, "mats")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what} must be a tensor")
        _require_cuda(t, what)
    if ref.dtype != torch.float32 or ref.dim() != 2 or ref.numel() < 1 or not ref.is_contiguous():
        raise ValueError("ref must be a contiguous float32 tensor [H, W]")
    H, W = int(ref.shape[0]), int(ref.shape[1])
    if frames.dtype != torch.float32 or frames.dim() != 3 or frames.shape[0] < 1 or tuple(frames.shape[1:]) != (H, W) \
            or not frames.is_contiguous():
        raise ValueError(f"frames must be a contiguous float32 tensor [B, {H}, {W}]")
    B = int(frames.shape[0])
    if mats.dtype != torch.float64 or mats.dim() != 4 or mats.shape[0] != B or mats.shape[1] < 1 \
            or tuple(mats.shape[2:]) != (2, 3) or not mats.is_contiguous():
        raise ValueError(f"mats must be a contiguous float64 tensor [{B}, K, 2, 3]")
    K = int(mats.shape[1])
    if weight is not None:
        if not isinstance(weight, torch.Tensor):
            raise ValueError("weight must be a tensor or None")
        _require_cuda(weight, "weight")
        if weight.dtype != torch.float32 or tuple(weight.shape) != (B, H, W) or not weight.is_contiguous():
            raise ValueError(f"weight must be a contiguous float32 tensor [{B}, {H}, {W}]")
    if not (float(damping) >= 0.0 and float(min_cover) >= 0.0):
        raise ValueError("damping and min_cover must be >= 0")
    dev = ref.device
    if any(t.device != dev for t in (frames, mats)) or (weight is not None and weight.device != dev):
        raise ValueError("all tensors must be on the same device")
    if ws is None:
        ws = _workspace("wire_register_gn_ws_bytes", dev, B, K, H, W)
    stats = torch.empty(B, K, 4, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().wire_register_gn_step(
        _stream_ptr(dev), ref.data_ptr(), frames.data_ptr(), weight.data_ptr() if weight is not None else None, B, K, H,
        W, m, float(damping), float(min_cover), mats.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel()),
        "wire_register_gn_step")
    return stats


# ---------------------------------------------------------------------------
# iso-surface extraction on the device (wire_iso_count / wire_iso_emit) and the blur of march_and_save's `smoothen`
# ---------------------------------------------------------------------------
def _check_volume(volume, what: str, min_side: int = 1) -> None:
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError(f"{what} expects a rank-3 (H, W, T) tensor")
    if min(volume.shape) < min_side:
        raise ValueError(f"{what}: a volume of shape {tuple(volume.shape)} (every side must be >= {min_side})")
    _require_cuda(volume, "volume")
    if volume.dtype != torch.float32:
        raise ValueError("volume must be float32")


def iso_surface(volume: torch.Tensor, thres: float):
    """The surface ``{volume >= thres}`` of a float32 CUDA tensor of shape (H, W, T) as a welded triangle mesh:
    ``(vertices [V, 3] float32, faces [F, 3] int32)``, both on the device.  Marching tetrahedra on the six-tetrahedron
    Kuhn split of every cell (csrc/wire_iso.hip): closed wherever the volume's boundary does not cut it, every triangle
    wound so that its normal points from inside (``>= thres``; NaN is outside) to outside, also when ``thres`` equals a
    data value.  Vertices are in index units (i, j, k), the PyMCubes convention, one per crossed lattice edge, ordered by
    (lower end, direction); faces by (cell, tetrahedron, triangle): the same input gives the same bits.  These are NOT
    PyMCubes' triangles.

    Two HIP passes with a device prefix sum between them.  The sizes of the outputs are only known after the first, so
    the call performs one host synchronisation -- the read of the two counts (the second pass checks them against
    the capacities it is given by reading the same 16 bytes once more, on a stream that has nothing left to wait for).
    That is acceptable at the end of a run, not inside a training loop.  Every side must be >= 2 and H W T <= 2^28.
    CPU tensors raise WireHipError; other ranks, dtypes or sizes ValueError."""
    _check_volume(volume, "iso_surface", 2)
    H, W, T = (int(s) for s in volume.shape)
    if H * W * T > 1 << 28:
        raise ValueError(f"iso_surface: a {H} x {W} x {T} volume has more than 2^28 points")
    thres = float(thres)
    if thres != thres:
        raise ValueError("iso_surface: the threshold is NaN")
    L = _lib.lib()
    vol = volume.detach().contiguous()
    dev, stream = vol.device, _stream_ptr(vol.device)
    ws = _workspace("wire_iso_ws_bytes", dev, H, W, T)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(L.wire_iso_count(stream, vol.data_ptr(), H, W, T, thres, ws.data_ptr(), counts.data_ptr()),
               "wire_iso_count")
    nv, nf = (int(c) for c in counts.tolist())           # the one host sync
    verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    if nv:
        _lib.check(L.wire_iso_emit(stream, vol.data_ptr(), H, W, T, thres, ws.data_ptr(), verts.data_ptr(), nv,
                                   faces.data_ptr(), nf), "wire_iso_emit")
    return verts, faces


def gauss3_blur(volume: torch.Tensor, sigma: float = 1.0) -> torch.Tensor:
    """Separable Gaussian blur of a float32 CUDA (H, W, T) tensor on the device (wire_gauss3_blur): truncated at
    4 sigma, edge values replicated, fp32.  Returns a new tensor."""
    _check_volume(volume, "gauss3_blur")
    if not 0.0 < float(sigma) <= 8.0:
        raise ValueError("gauss3_blur: sigma outside (0, 8]")
    L = _lib.lib()
    vol = volume.detach().contiguous()
    H, W, T = (int(s) for s in vol.shape)
    tmp, out = torch.empty_like(vol), torch.empty_like(vol)
    _lib.check(L.wire_gauss3_blur(_stream_ptr(vol.device), vol.data_ptr(), H, W, T, float(sigma), tmp.data_ptr(),
                                  out.data_ptr()), "wire_gauss3_blur")
    return out


# ---------------------------------------------------------------------------
# image-to-image resampling in cv2.resize's modes and its adjoint (wire_resize.hip)
# ---------------------------------------------------------------------------
def _resize_mode(interpolation) -> int:
    if isinstance(interpolation, str) and interpolation in _lib.RESIZE_MODE:
        return _lib.RESIZE_MODE[interpolation]
    if not isinstance(interpolation, (bool, str)) and interpolation in (0, 1, 2, 3):
        return int(interpolation)
    raise ValueError(f"interpolation must be one of {sorted(_lib.RESIZE_MODE)} or cv2's integer 0..3, "
                     f"not {interpolation!r}")


def resize_geometry(H: int, W: int, dsize=None, fx=None, fy=None, interpolation="linear"):
    """``(H, W, Hl, Wl, mode, sy, sx)`` as the wire_resize_* entry points take them, by cv2.resize's rules: an explicit
    ``dsize = (Wl, Hl)`` gives the scale ``n_in / n_out`` per axis; otherwise ``fx`` and ``fy`` give
    ``n_out = rint(n_in * f)`` (round half to even, cv2's cvRound) and the scale ``1 / f``.  ValueError for an output
    side < 1, a factor that is not finite or <= 0, an unknown interpolation, and ``area`` with an output larger than the
    input on either axis (cv2 silently switches to a linear variant there; this library does not imitate it).  Host
    only."""
    mode = _resize_mode(interpolation)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"resize: an image of {H} x {W}")
    if dsize is not None and tuple(dsize) != (0, 0):
        if len(dsize) != 2:
            raise ValueError("resize: dsize must be (Wl, Hl)")
        Wl, Hl = int(dsize[0]), int(dsize[1])
        if Hl < 1 or Wl < 1:
            raise ValueError(f"resize: an output of {Hl} x {Wl}")
        sy, sx = H / Hl, W / Wl
    else:
        if fx is None or fy is None:
            raise ValueError("resize needs dsize = (Wl, Hl) or both fx and fy")
        fx, fy = float(fx), float(fy)
        if not (0.0 < fx < float("inf") and 0.0 < fy < float("inf")):
            raise ValueError(f"resize: fx = {fx}, fy = {fy} must be finite and > 0")
        Hl, Wl = int(round(H * fy)), int(round(W * fx))       # Python's round is half to even, as cvRound
        if Hl < 1 or Wl < 1:
            raise ValueError(f"resize: fx = {fx}, fy = {fy} give an output of {Hl} x {Wl}")
        sy, sx = 1.0 / fy, 1.0 / fx
    if mode == _lib.RESIZE_MODE["area"] and (Hl > H or Wl > W):
        raise ValueError(f"resize: area does not up-scale ({H} x {W} -> {Hl} x {Wl}); cv2 switches to a linear variant "
                         "there, use interpolation='linear'")
    return H, W, Hl, Wl, mode, sy, sx


def resize_tables(geom, dev: torch.device) -> torch.Tensor:
    """The device tables of a geometry (wire_resize_tables): a uint8 tensor to pass wherever a wire_resize_* entry point
    takes ``tab``.  They depend on the geometry alone; keep them across calls."""
    L = _lib.lib()
    tab = torch.empty(_lib.check(L.wire_resize_tab_bytes(*geom), "wire_resize_tab_bytes"), dtype=torch.uint8, device=dev)
    _lib.check(L.wire_resize_tables(_stream_ptr(dev), *geom, tab.data_ptr()), "wire_resize_tables")
    return tab


def _resize_apply(entry: str, tab, geom, src: torch.Tensor, Cc: int, out_shape) -> torch.Tensor:
    out = torch.empty(out_shape, dtype=torch.float32, device=src.device)
    _lib.check(getattr(_lib.lib(), entry)(_stream_ptr(src.device), tab.data_ptr(), *geom, src.data_ptr(), Cc,
                                          out.data_ptr()), entry)
    return out


class _ResizeFunction(torch.autograd.Function):
    """y = R x (wire_resize_fwd) and g_x = R^T g_y (wire_resize_bwd), or the two swapped for the adjoint; both read the
    same tables."""

    @staticmethod
    def forward(ctx, img, geom, adjoint):
        x = img.detach()
        H, W, Hl, Wl = geom[:4]
        Cc = x.numel() // ((Hl * Wl) if adjoint else (H * W))
        tab = resize_tables(geom, x.device)
        shape = ((H, W) if adjoint else (Hl, Wl)) + tuple(x.shape[2:])
        ctx.save_for_backward(tab)
        ctx.geom, ctx.adjoint, ctx.Cc, ctx.in_shape = geom, adjoint, Cc, tuple(x.shape)
        return _resize_apply("wire_resize_bwd" if adjoint else "wire_resize_fwd", tab, geom, x, Cc, shape)

    @staticmethod
    def backward(ctx, g_out):
        tab, = ctx.saved_tensors
        _no_second_order("resize")
        g = g_out.detach().to(torch.float32).contiguous()
        return _resize_apply("wire_resize_fwd" if ctx.adjoint else "wire_resize_bwd", tab, ctx.geom, g, ctx.Cc,
                             ctx.in_shape), None, None


def _resize_image(img, what: str) -> None:
    if not isinstance(img, torch.Tensor) or img.dim() not in (2, 3) or img.numel() == 0:
        raise ValueError(f"{what} expects a non-empty [H, W] or [H, W, C] tensor")


def _resize_device(img: torch.Tensor, what: str) -> None:
    _require_cuda(img, what)
    if img.dtype != torch.float32 or not img.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor")


def resize(img: torch.Tensor, dsize=None, fx=None, fy=None, interpolation="linear") -> torch.Tensor:
    """``cv2.resize(img, dsize, fx=fx, fy=fy, interpolation=...)`` on the device: ``img`` is a contiguous CUDA float32
    [H, W] or [H, W, C] tensor (channel last, any C), the result a new [Hl, Wl] or [Hl, Wl, C] one.

    ``dsize = (Wl, Hl)`` is in cv2's order; ``None`` or ``(0, 0)`` takes the size from ``fx`` / ``fy`` instead,
    ``n_out = rint(n_in * f)``.  ``interpolation``: ``"nearest"``, ``"linear"``, ``"cubic"``, ``"area"`` or cv2's integer
    for them (0, 1, 2, 3).  The operator is the separable table include/wire_hip.h defines -- pixel centres at
    ``(d + 0.5) * scale - 0.5``, border replicated, the Keys cubic at A = -0.75, area as the exact overlap average --
    with fp32 weights and fp32 accumulation in a fixed order.  It agrees with cv2 BY CONSTRUCTION from cv2's documented
    formulas (and with ``F.interpolate(align_corners=False)`` / ``avg_pool2d``, which the tests measure); it has NOT been
    measured against cv2.  Two differences on purpose: cv2's non-integer INTER_AREA drops partial overlaps below 1e-3
    without renormalising, this operator keeps them; cv2's INTER_AREA up-scaling (silently a linear variant) is not
    provided -- ``area`` with an output side larger than the input raises ValueError.

    Differentiable with respect to ``img`` through the adjoint kernel (wire_resize_bwd: a gather, no atomics, the same
    bits every time), first order only.  CPU tensors raise WireHipError; other ranks, dtypes or sizes ValueError."""
    _resize_image(img, "resize")
    geom = resize_geometry(img.shape[0], img.shape[1], dsize, fx, fy, interpolation)
    _resize_device(img, "img")
    return _ResizeFunction.apply(img, geom, False)


def resize_adjoint(g: torch.Tensor, shape, dsize=None, fx=None, fy=None, interpolation="linear") -> torch.Tensor:
    """``R^T g`` for the ``R`` of ``resize`` on an image of ``shape = (H, W)``: ``g`` is [Hl, Wl] or [Hl, Wl, C] (the
    size ``resize`` would return for the same ``dsize`` / ``fx`` / ``fy``), the result [H, W] or [H, W, C].  The exact
    transpose: the same fp32 weights, gathered (wire_resize_bwd); a source that no output touches receives +0.0.
    Differentiable with respect to ``g`` (through the forward kernel), first order only."""
    _resize_image(g, "resize_adjoint")
    if len(shape) != 2:
        raise ValueError("resize_adjoint: shape must be (H, W)")
    geom = resize_geometry(shape[0], shape[1], dsize, fx, fy, interpolation)
    if (int(g.shape[0]), int(g.shape[1])) != (geom[2], geom[3]):
        raise ValueError(f"resize_adjoint: g is {tuple(g.shape[:2])}, the resized image is {(geom[2], geom[3])}")
    _resize_device(g, "g")
    return _ResizeFunction.apply(g, geom, True)
