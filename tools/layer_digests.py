#!/usr/bin/env python3
"""SHA-256 digests of what the per-layer path leaves behind, for comparing two builds of the package bit for bit: every
per-layer entry point of the C ABI (through wire_amd._lib) and every public layer function of wire_amd.functional
(forward, every gradient, and a first layer whose coordinates require a gradient), one line per output buffer, with
fixed seeds, at n = 129 and n = 4133 rows -- the two sides of the 4096-row line at which the 2 x fp16 kernels take over
-- under each GEMM family setting the tests use.  Hidden layers are 77 -> 101, first layers 3 -> 77, final layers
101 -> 3; the real kinds are siren, gauss, relu, bspline_form and bspline_cubic, the cubic also at 2 -> 64, where it
stays on the 3 x bf16 kernels.  None of these calls adds with atomics, so two runs of one build print the same lines.
It uses the public functions and the C ABI alone, so the same file runs against another checkout:
    python3 tools/layer_digests.py > head.txt
    python3 tools/layer_digests.py --root ../other-checkout > other.txt       # every line must be identical
--time prints, instead, the host's cost of the path where launch overhead dominates: a forward and a backward of each
public layer function at n = 129, the median over --blocks blocks of --iters iterations each (a device synchronise
ends a block), with the fastest and the slowest block.  Compare two checkouts in alternating runs:
    python3 tools/layer_digests.py --time; python3 tools/layer_digests.py --time --root ../other-checkout; ...
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose wire_amd is imported (default: this file's)")
ap.add_argument("--time", action="store_true", help="time the public layer functions at n = 129 instead")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--blocks", type=int, default=9)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch

from wire_amd import _lib
from wire_amd import functional as F

dev = torch.device("cuda:0")
L = _lib.lib()
ROWS = (129, 4133)
HID, FIRST, FINAL = (77, 101), (3, 77), (101, 3)
# the GEMM families of tests/_util.py's family_ctx: 2 x fp16 (the default), 3 x bf16, 3M, 4M
FAMILIES = [("default", {}), ("split_f16=0", dict(split_f16=0)), ("split_bf16=0 complex_3m=1", dict(split_bf16=0, complex_3m=1)),
            ("split_bf16=0 complex_3m=0", dict(split_bf16=0, complex_3m=0))]
# kind -> (omega_0, scale_0) of a layer call
REAL = {"siren": (30.0, 10.0), "gauss": (30.0, 3.0), "relu": (30.0, 10.0), "bspline_form": (1.0, 0.5),
        "bspline_cubic": (1.0, 15.0)}
OM, SC = 7.0, 6.0


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def rn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(dev).contiguous()


def out(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device=dev)


def call(name, *a):
    """One entry point on the current stream; tensors go as pointers."""
    _lib.check(getattr(L, name)(torch.cuda.current_stream().cuda_stream,
                                *[t.data_ptr() if isinstance(t, torch.Tensor) else t for t in a]), name)
    torch.cuda.synchronize()


def emit(tag, **bufs):
    for k, t in bufs.items():
        print(f"{tag} {k:6s} {sha(t)}", flush=True)


def layer_inputs(seed, n, i, o, cplx, two=False, wgain=0.5):
    """x [n, i], the parameters (W, b) or (W, b, V, c), and g_act [n, o]; complex tensors as [..., 2] floats."""
    g = torch.Generator().manual_seed(seed)
    c = (2,) if cplx else ()
    x = rn(g, n, i, *c)
    params = []
    for _ in range(2 if two else 1):
        params += [rn(g, o, i, *c, scale=wgain / i ** 0.5), rn(g, o, *c, scale=0.1)]
    return x, params, g


def cx(t):
    return torch.view_as_complex(t)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def abi_gabor(tag, n, two):
    q = "wire_layer2d_ws_bytes" if two else "wire_layer_ws_bytes"
    pre = "wire_gabor2d" if two else "wire_gabor"
    for first in (0, 1):
        i, o = FIRST if first else HID
        c = () if first else (2,)
        x, P, g = layer_inputs(n + 10 * first + two, n, i, o, not first, two)
        ga = rn(g, n, o, 2)
        wsb = _lib.check(getattr(L, q)(n, i, o), q)
        print(f"{tag} {q} n={n} {i}->{o} {wsb}", flush=True)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        t = f"{tag} {pre}%s {'first' if first else 'hidden'} n={n}"
        shape = (n, i, o, first)
        act, lin = out(n, o, 2), out(n, o, *c)
        call(pre + "_fwd", x, *P, OM, SC, *shape, *(() if two else (lin,)), act, ws, wsb)
        emit(t % "_fwd", act=act, **({} if two else dict(lin=lin)))
        grads = [torch.zeros_like(p) for p in P]
        gx = None if first else out(n, i, 2)
        call(pre + "_bwd", ga, x, *P, OM, SC, *shape, gx, *grads, ws, wsb)
        emit(t % "_bwd", **({} if first else dict(g_x=gx)), **{f"g_{k}": v for k, v in zip("WbVc", grads)})
        hp = out(2)
        call(pre + "_hparam_grad", ga, x, *P, OM, SC, *shape, hp, ws, wsb)
        emit(t % "_hparam_grad", out2=hp)
        if first:
            for wg in (True, False):
                grads = [torch.zeros_like(p) if wg else None for p in P]
                gx = out(n, i)
                call(pre + "_bwd_first_coords", ga, x, *P, OM, SC, n, i, o, gx, *grads, ws, wsb)
                emit(t % "_bwd_first_coords" + f" grads={wg}", g_x=gx,
                     **({f"g_{k}": v for k, v in zip("WbVc", grads)} if wg else {}))


def abi_final(tag, n):
    i, o = FINAL
    g = torch.Generator().manual_seed(n + 2)
    z, Wf, bf, gy = rn(g, n, i, 2), rn(g, o, i, 2, scale=0.1), rn(g, o, 2), rn(g, n, o)
    wsb = _lib.check(L.wire_layer_ws_bytes(n, i, o), "wire_layer_ws_bytes")
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    y = out(n, o)
    call("wire_final_fwd", z, Wf, bf, n, i, o, y, ws, wsb)
    emit(f"{tag} wire_final_fwd n={n}", y=y)
    gz, gW, gb = out(n, i, 2), out(o, i, 2), out(o, 2)
    call("wire_final_bwd", gy, z, Wf, n, i, o, gz, gW, gb, ws, wsb)
    emit(f"{tag} wire_final_bwd n={n}", g_z=gz, g_Wf=gW, g_bf=gb)


def real_shapes(kind):
    return [HID] + ([(2, 64)] if kind == "bspline_cubic" else [])


def abi_real(tag, n):
    for kind, (om, sc) in REAL.items():
        for i, o in real_shapes(kind):
            x, (W, b), g = layer_inputs(n + 3, n, i, o, False, wgain=0.3)
            ga = rn(g, n, o)
            wsb = _lib.check(L.wire_layer_ws_bytes(n, i, o), "wire_layer_ws_bytes")
            ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
            k, t = _lib.KIND[kind], f"{tag} wire_real_layer%s {kind} n={n} {i}->{o}"
            act = out(n, o)
            call("wire_real_layer_fwd", k, x, W, b, om, sc, n, i, o, act, ws, wsb)
            emit(t % "_fwd", act=act)
            gx, gW, gb = out(n, i), out(o, i), out(o)
            call("wire_real_layer_bwd", k, ga, x, W, b, om, sc, n, i, o, gx, gW, gb, ws, wsb)
            emit(t % "_bwd", g_x=gx, g_W=gW, g_b=gb)


# ---------------------------------------------------------------------------------------------------------------------
# the public layer functions
# ---------------------------------------------------------------------------------------------------------------------
def gabor_case(n, two, trainable, first, coords_grad=False):
    """(fn, leaves): fn() runs the public function on fresh leaves and returns (act, g_act); leaves name the inputs whose
    .grad the backward fills."""
    i, o = FIRST if first else HID
    x, P, g = layer_inputs(n + 20 + 10 * first + two, n, i, o, not first, two)
    ga = cx(rn(g, n, o, 2))
    leaves = {}

    def fn():
        xs = (x if first else cx(x)).clone().requires_grad_(coords_grad or not first)
        ps = [(p if first else cx(p)).clone().requires_grad_(True) for p in P]
        leaves.clear()
        leaves.update({"x": xs} if xs.requires_grad else {}, **{k: p for k, p in zip("WbVc", ps)})
        if trainable:
            om, sc = (torch.tensor([v], device=dev, requires_grad=True) for v in (OM, SC))
            leaves.update(omega=om, scale=sc)
        else:
            om, sc = OM, SC
        f = {(False, False): F.gabor_layer, (False, True): F.gabor_layer_trainable, (True, False): F.gabor2d_layer,
             (True, True): F.gabor2d_layer_trainable}[(two, trainable)]
        return f(xs, *ps, om, sc, bool(first)), ga
    return fn, leaves


def real_case(n, kind, i, o):
    om, sc = REAL[kind]
    x, P, g = layer_inputs(n + 23, n, i, o, False, wgain=0.3)
    ga = rn(g, n, o)
    leaves = {}

    def fn():
        xs, W, b = (t.clone().requires_grad_(True) for t in (x, *P))
        leaves.update(x=xs, W=W, b=b)
        return F.real_layer(kind, xs, W, b, om, sc), ga
    return fn, leaves


def final_case(n):
    i, o = FINAL
    g = torch.Generator().manual_seed(n + 22)
    z, Wf, bf, gy = cx(rn(g, n, i, 2)), cx(rn(g, o, i, 2, scale=0.1)), cx(rn(g, o, 2)), rn(g, n, o)
    leaves = {}

    def fn():
        zs, W, b = (t.clone().requires_grad_(True) for t in (z, Wf, bf))
        leaves.update(z=zs, Wf=W, bf=b)
        return F.final_linear_real(zs, W, b), gy
    return fn, leaves


def gabor_name(two, trainable, first, coords_grad):
    return (f"gabor{'2d' if two else ''}_layer{'_trainable' if trainable else ''} "
            f"{'first' if first else 'hidden'}{' coords' if coords_grad else ''}")


def public_cases(n):
    for two in (False, True):
        for trainable in (False, True):
            for first, cg in ((False, False), (True, False), (True, True)):
                yield gabor_name(two, trainable, first, cg), gabor_case(n, two, trainable, first, cg)
    for kind in REAL:
        for i, o in real_shapes(kind):
            yield f"real_layer {kind} {i}->{o}", real_case(n, kind, i, o)
    yield "final_linear_real", final_case(n)


def digest_public(tag, n):
    for name, (fn, leaves) in public_cases(n):
        act, ga = fn()
        act.backward(ga)
        torch.cuda.synchronize()
        emit(f"{tag} F.{name} n={n}", act=act, **{f"g_{k}": v.grad for k, v in leaves.items()})


def time_public(n=129):
    cases = [(gabor_name(two, tr, False, False), gabor_case(n, two, tr, False)) for two in (False, True)
             for tr in (False, True)]
    cases += [(gabor_name(False, False, True, True), gabor_case(n, False, False, True, True)),
              ("real_layer siren", real_case(n, "siren", *HID)), ("final_linear_real", final_case(n))]
    for name, (fn, _) in cases:
        def block():
            t0 = time.perf_counter()
            for _ in range(args.iters):
                act, ga = fn()
                act.backward(ga)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.iters * 1e6
        block()                                                          # warm-up: code objects, allocator
        us = sorted(block() for _ in range(args.blocks))
        print(f"time F.{name} n={n}: median {statistics.median(us):.1f} us per forward + backward "
              f"(min {us[0]:.1f}, max {us[-1]:.1f}; {args.blocks} blocks of {args.iters})", flush=True)


def main():
    if args.time:
        time_public()
        return
    for tag, knobs in FAMILIES:
        saved = {k: _lib.check(L.wire_tune_get(k.encode()), k) for k in knobs}
        for k, v in knobs.items():
            _lib.check(L.wire_tune_set(k.encode(), v), k)
        try:
            for n in ROWS:
                abi_gabor(f"[{tag}]", n, False)
                abi_gabor(f"[{tag}]", n, True)
                abi_final(f"[{tag}]", n)
                abi_real(f"[{tag}]", n)
                digest_public(f"[{tag}]", n)
        finally:
            for k, v in saved.items():
                _lib.check(L.wire_tune_set(k.encode(), v), k)


if __name__ == "__main__":
    main()
