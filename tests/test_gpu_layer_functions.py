"""The Gabor layer Function of wire_amd.functional, which gabor_layer, gabor_layer_trainable, gabor2d_layer and
gabor2d_layer_trainable share: the trainable variant is the plain one plus the hyper-parameter call, so at equal
omega_0 / scale_0 it returns the plain one's bits; its two extra gradients are the fp64 closed forms of
tests/glue_ref.py; a first layer hands the coordinates a gradient of their own shape and dtype, first order only.

Shapes: 3 -> 7 (first) and 5 -> 7 (hidden), one 64-column tile of every GEMM, at 129 rows (4 blocks of 32 rows and one
of 1) and the hidden layers once more at 4133 rows, past the 4096-row line where the 2 x fp16 kernels take over."""
import functools

import numpy as np
import pytest
import torch

from _util import within_ref
import glue_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUT = 7
OMEGA, SCALE = 9.0, 4.0          # exact in fp32: the plain call's floats and the trainable call's tensors hold the same


@functools.lru_cache(maxsize=None)
def _inputs(form, first, n):
    """Host arrays x, (W, b) or (W, b, V, c), g_act: the magnitudes of tests/test_gpu_glue.py's hyper-parameter test,
    with the weights rescaled from its 24 inputs to 5."""
    rng = np.random.default_rng(1000 * n + 10 * first + (form == "gabor2d"))
    fin = 3 if first else 5
    cplx = lambda *sh: (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)).astype(np.complex64)
    if first:
        x = rng.uniform(-1, 1, (n, fin)).astype(np.float32)
        mk = lambda *sh: (0.3 * rng.standard_normal(sh)).astype(np.float32)
    else:
        x = (0.5 * cplx(n, fin)).astype(np.complex64)
        mk = lambda *sh: (0.13 * cplx(*sh)).astype(np.complex64)
    params = [mk(OUT, fin), mk(OUT)]
    if form == "gabor2d":
        params += [mk(OUT, fin), mk(OUT)]
    return x, tuple(params), cplx(n, OUT)


def _run(form, trainable, first, n, coords_grad=True, xshape=None, xdtype=None):
    """One forward and backward of a public layer function on fresh leaves; returns (act, {name: gradient})."""
    from wire_amd import functional as F
    x, params, g = _inputs(form, first, n)
    xs = torch.tensor(x, device=DEV)
    if xshape is not None:
        xs = xs.reshape(xshape).to(xdtype)
    xs.requires_grad_(coords_grad or not first)
    ps = [torch.tensor(p, device=DEV, requires_grad=True) for p in params]
    leaves = dict(zip(("g_W", "g_b", "g_V", "g_c"), ps))
    if xs.requires_grad:
        leaves["g_x"] = xs
    if trainable:
        om, sc = (torch.tensor([v], dtype=torch.float32, device=DEV, requires_grad=True) for v in (OMEGA, SCALE))
        leaves.update(g_omega=om, g_scale=sc)
    else:
        om, sc = OMEGA, SCALE
    fn = getattr(F, f"{form}_layer" + ("_trainable" if trainable else ""))
    act = fn(xs, *ps, om, sc, first)
    act.backward(torch.tensor(g, device=DEV).reshape(act.shape))
    torch.cuda.synchronize()
    return act.detach(), {k: t.grad for k, t in leaves.items()}


def _bits(t):
    return t.contiguous().cpu().numpy().tobytes()


CASES = [(form, first, 129) for form in ("gabor", "gabor2d") for first in (True, False)] + \
        [("gabor", False, 4133), ("gabor2d", False, 4133)]


@pytest.mark.parametrize("form,first,n", CASES)
def test_trainable_returns_the_plain_bits(form, first, n):
    """act, g_x, g_W, g_b (and g_V, g_c) of the trainable function are those of the plain one, bit for bit: both make
    the same C calls on the same floats."""
    act_p, g_p = _run(form, False, first, n)
    act_t, g_t = _run(form, True, first, n)
    assert set(g_p) == {"g_x", "g_W", "g_b"} | ({"g_V", "g_c"} if form == "gabor2d" else set())
    assert set(g_t) == set(g_p) | {"g_omega", "g_scale"}
    assert _bits(act_t) == _bits(act_p), "act"
    for k, v in g_p.items():
        assert g_t[k].shape == v.shape and g_t[k].dtype == v.dtype and _bits(g_t[k]) == _bits(v), k


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("form", ["gabor", "gabor2d"])
def test_hparam_grads_of_the_trainable_functions(form, first):
    """omega_0.grad and scale_0.grad on 129 rows against the fp64 closed forms, by the bar of tests/test_gpu_glue.py's
    test_hparam_grads: each is one number, a sum of terms that partly cancel, so the error is relative to the sum of the
    terms' magnitudes and bounded by 2 x the same error of the fp32 restatement + 1e-6."""
    n = 129
    x, params, g = _inputs(form, first, n)
    closed = ref.gabor_hparam_grads if form == "gabor" else ref.gabor2d_hparam_grads
    v64, a64 = closed(x, *params, g, OMEGA, SCALE, True)
    v32 = closed(x, *params, g, OMEGA, SCALE, False)[0]
    assert min(a64) > 0 and all(abs(v) > 1e-3 * a for v, a in zip(v64, a64))       # the sums do not cancel to nothing
    _, grads = _run(form, True, first, n, coords_grad=False)
    for k, name in enumerate(("omega", "scale")):
        got = grads[f"g_{name}"]
        assert got.shape == (1,) and got.dtype == torch.float32
        eb = abs(float(got[0]) - float(v64[k])) / a64[k]
        er = abs(float(v32[k]) - float(v64[k])) / a64[k]
        print(f"hparam {form} first={first} dL/d{name}_0: {float(got[0]):.6e} (fp64 {float(v64[k]):.6e}) err {eb:.2e} ref {er:.2e}")
        within_ref(eb, er, f"layer function hparam {form} {'first' if first else 'hidden'} dL/d{name}_0 "
                           "[relative to sum |terms|]")


@pytest.mark.parametrize("trainable", [False, True])
@pytest.mark.parametrize("form", ["gabor", "gabor2d"])
def test_first_layer_coordinate_gradient(form, trainable):
    """coords.grad has the shape and the dtype of coords (a [3, 43, 3] float64 tensor here), and create_graph=True is
    refused: the coordinate gradient is first order only."""
    from wire_amd import functional as F
    _, grads = _run(form, trainable, True, 129, xshape=(3, 43, 3), xdtype=torch.float64)
    assert grads["g_x"].shape == (3, 43, 3) and grads["g_x"].dtype == torch.float64
    assert bool(torch.isfinite(grads["g_x"]).all()) and float(grads["g_x"].abs().max()) > 0

    x, params, g = _inputs(form, True, 129)
    xs = torch.tensor(x, device=DEV, requires_grad=True)
    ps = [torch.tensor(p, device=DEV, requires_grad=True) for p in params]
    om, sc = ((torch.tensor([v], device=DEV, requires_grad=True) for v in (OMEGA, SCALE)) if trainable
              else (OMEGA, SCALE))
    act = getattr(F, f"{form}_layer" + ("_trainable" if trainable else ""))(xs, *ps, om, sc, True)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(act, xs, torch.tensor(g, device=DEV), create_graph=True)
