"""Gradients with respect to the input coordinates (``coords.requires_grad_()`` + ``backward``), on every net kind and
GEMM family, against the fp64 eager oracle of oracle/torch_ref.py (err_build <= 2 err_ref + 1e-6).

The loss is ``sum(y * w)`` for a fixed random ``w``: its coordinate gradient is row-local, so the fp64 oracle runs in
row chunks without changing a single value."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _util
from _util import relmax, within_ref
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BENCH = dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)     # bench.py's regime
CLASS = dict(first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0)     # the classes' defaults


def _model(kind, D, hf, L, O=3, seed=0, pos_encode=False, outermost_linear=True, **kw):
    from wire_amd.modules import models
    torch.manual_seed(seed)
    extra = dict(pos_encode=True, sidelength=256) if pos_encode else {}
    return models.get_INR(nonlin=kind, in_features=D, out_features=O, hidden_features=hf, hidden_layers=L,
                          outermost_linear=outermost_linear, **extra, **kw).to(DEV)


def _coords(n, D, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, D, generator=g, dtype=torch.float64) * 2 - 1


def _weights(n, O, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, O, generator=g, dtype=torch.float64)


def _oracle_forward(kind, model, L, kw, nf, relu_masks=None, last_act=False):
    """The eager reference forward (oracle/torch_ref.py) with the model's parameters.  relu: ``relu_masks`` (per layer,
    [n, K] bool) imposes the build's own decisions on the oracle -- a decision at |lin| = round-off flips the gradient
    of its row, which neither precision settles (the protocol of the relu step test, tests/test_gpu_timed_kernels.py);
    ``last_act``: the net ends in an activation layer (outermost_linear=False)."""
    P = {k: v.detach().cpu() for k, v in model.state_dict().items() if "omega_0" not in k and "scale_0" not in k}
    om1, om, sc = kw.get("first_omega_0", 30.0), kw.get("hidden_omega_0", 30.0), kw.get("scale", 10.0)

    def fwd(c, double, rows=slice(None)):
        p = {k: (v.to(torch.complex128 if double else torch.complex64) if v.is_complex()
                 else v.to(torch.float64 if double else torch.float32)) for k, v in P.items()}
        if kind == "wire":
            return torch_ref.wire_forward(p, c, L, om1, om, sc)
        if kind == "wire2d":
            return torch_ref.wire2d_forward(p, c, L, om1, om, sc)
        if kind == "relu" and (relu_masks is not None or last_act):
            h = c if nf is None else torch_ref.posenc(c, nf)
            for l in range(L + (2 if last_act else 1)):
                lin = F.linear(h, p[f"net.{l}.linear.weight"], p[f"net.{l}.linear.bias"])
                h = F.relu(lin) if relu_masks is None else lin * torch.as_tensor(relu_masks[l][rows]).to(lin.dtype)
            if last_act:
                return h
            return F.linear(h, p[f"net.{L + 1}.weight"], p[f"net.{L + 1}.bias"])
        return torch_ref.realnet_forward(kind, p, c, L, om1, om, sc, nf)
    return fwd


def oracle_coords_grad(fwd, coords, w, double, chunk=16384):
    """d sum(y w) / d coords of the eager reference, fp64 or fp32, in row chunks (tests/_util.oracle_grads_chunked)."""
    dt = torch.float64 if double else torch.float32
    out = []
    with torch.enable_grad():
        for s in range(0, coords.shape[0], chunk):
            c = coords[s:s + chunk].to(dt).clone().requires_grad_(True)
            (fwd(c, double, slice(s, s + chunk)) * w[s:s + chunk].to(dt)).sum().backward()
            out.append(c.grad.to(torch.float64))
    return torch.cat(out).numpy()


def _abi_forward(model, coords):
    """wire_mlp_fwd(save_for_bwd = 1) on the model's packed parameters: what _INRFunction.forward runs."""
    from wire_amd import _lib
    from wire_amd.functional import _native, _stream_ptr
    L = _lib.lib()
    desc = model.net_desc()
    x = coords.to(torch.float32).to(DEV).contiguous()
    n = x.shape[0]
    nat = [_native(p) for p in model.param_tensors()]
    packed = torch.empty(L.wire_packed_floats(C.byref(desc)), dtype=torch.float32, device=DEV)
    s = _stream_ptr(torch.device(DEV))
    _lib.check(L.wire_pack_params(s, C.byref(desc), _lib.ptr_array([p.data_ptr() for p in nat]), packed.data_ptr()),
               "pack")
    ab = L.wire_act_bytes(C.byref(desc), n, 1)
    act = torch.empty(ab, dtype=torch.uint8, device=DEV)
    y = torch.empty(n, desc.out_features, device=DEV)
    _lib.check(L.wire_mlp_fwd(s, C.byref(desc), packed.data_ptr(), x.data_ptr(), n, y.data_ptr(), act.data_ptr(), ab, 1),
               "fwd")
    return L, desc, x, n, nat, packed, act, ab, s


def _relu_masks(model, coords, Ln):
    """The build's relu decisions out_l > 0 (l = 0 .. L) of the whole-net forward, read back from its activations."""
    from wire_amd import _lib
    L, desc, _, n, _, _, act, _, _ = _abi_forward(model, coords)
    torch.cuda.synchronize()
    K = model._arch["width"]
    P = (K + 63) // 64 * 64
    a = act.view(torch.float32)
    out = []
    for l in range(Ln + 1):
        off = _lib.check(L.wire_act_out_offset(C.byref(desc), n, l), "wire_act_out_offset")
        out.append((a[off:off + n * P].view(n, P)[:, :K] > 0).cpu().numpy())
    return out


def build_coords_grad(model, coords, w, shape=None, dtype=torch.float32):
    x = coords.to(dtype).to(DEV)
    if shape is not None:
        x = x.reshape(shape)
    x.requires_grad_(True)
    y = model(x)
    (y * w.to(torch.float32).to(DEV).reshape(y.shape)).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.dtype == dtype and x.grad.shape == x.shape
    return x.grad.detach().reshape(coords.shape).to(torch.float64).cpu().numpy()


def _layerwise_relu_masks(model, coords):
    """The same decisions for a layer-by-layer net (outermost_linear=False): each layer's output > 0."""
    with torch.no_grad():
        h = model.positional_encoding(coords.to(torch.float32).to(DEV).reshape(1, -1, coords.shape[1]))
        out = []
        for m in model.net:
            h = m(h)
            out.append((h.reshape(coords.shape[0], -1) > 0).cpu().numpy())
    return out


def check_case(label, kind, D, hf, L, n, kw, pos_encode=False, outermost_linear=True, seed=0, O=3):
    model = _model(kind, D, hf, L, O=O, seed=seed, pos_encode=pos_encode, outermost_linear=outermost_linear, **kw)
    nf = model.positional_encoding.num_frequencies if pos_encode else None
    coords, w = _coords(n, D), _weights(n, O)
    g = build_coords_grad(model, coords, w)
    masks = None
    if kind == "relu":
        masks = _relu_masks(model, coords, L) if outermost_linear else _layerwise_relu_masks(model, coords)
    fwd = _oracle_forward(kind, model, L, kw, nf, relu_masks=masks, last_act=not outermost_linear)
    g64 = oracle_coords_grad(fwd, coords, w, True)
    g32 = oracle_coords_grad(fwd, coords, w, False)
    assert np.abs(g64).max() > 0, f"{label}: the oracle's gradient is zero (a dead net compares nothing)"
    within_ref(relmax(g, g64), relmax(g32, g64), f"coords_grad {label}")


# ---- 1. against fp64, every kind ------------------------------------------------------------------------------------
CASES = [
    ("wire_4x256_n262144_bench", "wire", 2, 363, 4, 262144, BENCH, False),
    ("wire_K181_n16384_bench", "wire", 2, 256, 4, 16384, BENCH, False),
    ("wire_4x256_n4133_x3", "wire", 2, 363, 4, 4133, BENCH, False),
    ("wire_4x256_n8192_class", "wire", 2, 363, 4, 8192, CLASS, False),
    ("wire_d3_n8192", "wire", 3, 363, 3, 8192, dict(first_omega_0=10.0, hidden_omega_0=10.0, scale=10.0), False),
    ("wire2d_3x128_n8192", "wire2d", 2, 128, 3, 8192, dict(first_omega_0=10.0, hidden_omega_0=10.0, scale=10.0), False),
    ("siren_4x256_n16384_class", "siren", 2, 256, 4, 16384, CLASS, False),
    ("siren_d3_4x256_n8192", "siren", 3, 256, 4, 8192, CLASS, False),
    ("gauss_4x256_n16384", "gauss", 2, 256, 4, 16384, CLASS, False),
    ("relu_4x256_n16384", "relu", 2, 256, 4, 16384, CLASS, False),
    ("relu_posenc_4x256_n8192", "relu", 2, 256, 4, 8192, CLASS, True),
    ("relu_posenc_d3_2x128_n4133", "relu", 3, 128, 2, 4133, CLASS, True),
    ("wire_L0_n5000", "wire", 2, 64, 0, 5000, BENCH, False),
    ("siren_L0_n5000", "siren", 2, 64, 0, 5000, CLASS, False),
]


@pytest.mark.parametrize("label,kind,D,hf,L,n,kw,pe", CASES, ids=[c[0] for c in CASES])
def test_coords_grad_vs_fp64(label, kind, D, hf, L, n, kw, pe):
    check_case(label, kind, D, hf, L, n, kw, pos_encode=pe)


# ---- 2. the other GEMM families -------------------------------------------------------------------------------------
FAMILY_CASES = [("wire", 2, 363, 3), ("wire2d", 2, 128, 2), ("siren", 2, 256, 3), ("relu", 2, 128, 2)]
# (wire2d at the classes' omega_0 = 30 / scale_0 = 10 drives the fp32 eager oracle to nan: its own regime of case 1)
FAMILY_KW = {"wire": BENCH, "wire2d": dict(first_omega_0=10.0, hidden_omega_0=10.0, scale=10.0), "siren": CLASS,
             "relu": CLASS}


FAMILY_KNOBS = {"split_f16_0": dict(split_f16=0), "split_bf16_0": dict(split_bf16=0),
                "complex_3m_1": dict(split_bf16=0, complex_3m=1), "complex_3m_0": dict(split_bf16=0, complex_3m=0)}
FAMILIES = list(FAMILY_KNOBS)


@pytest.mark.parametrize("fam", FAMILIES)
def test_coords_grad_families(fam):
    with _util.tune(**FAMILY_KNOBS[fam]):
        for kind, D, hf, nl in FAMILY_CASES:
            check_case(f"{kind}_{fam}_n8192", kind, D, hf, nl, 8192, FAMILY_KW[kind])


# ---- 3. nothing that exists changes ----------------------------------------------------------------------------------
def _fwd_bwd(model, coords, w, want_x):
    for p in model.parameters():
        p.grad = None
    x = coords.to(torch.float32).to(DEV).requires_grad_(want_x)
    y = model(x)
    (y * w.to(torch.float32).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()
                              if p.grad is not None}, x.grad


@pytest.mark.parametrize("fam", ["default"] + FAMILIES)
def test_params_unchanged_by_coords_grad(fam):
    with _util.tune(**FAMILY_KNOBS.get(fam, {})):
        for kind, D, hf, nl in FAMILY_CASES:
            model = _model(kind, D, hf, nl, **FAMILY_KW[kind])
            coords, w = _coords(8192, D), _weights(8192, 3)
            y0, g0, _ = _fwd_bwd(model, coords, w, False)
            y1, g1, gx = _fwd_bwd(model, coords, w, True)
            assert gx is not None
            assert torch.equal(y0, y1), (kind, fam)
            assert g0.keys() == g1.keys() and len(g0) > 0
            for k in g0:
                assert torch.equal(g0[k], g1[k]), (kind, fam, k)


def _abi_run(model, coords, w, with_coords):
    """wire_mlp_bwd vs wire_mlp_bwd_coords(g_coords = NULL) on the same saved forward."""
    from wire_amd import _lib
    L, desc, x, n, nat, packed, act, ab, s = _abi_forward(model, coords)
    gy = w.to(torch.float32).to(DEV).contiguous()
    grads = [torch.empty_like(p) for p in nat]
    if with_coords:
        sb = L.wire_bwd_coords_scratch_bytes(C.byref(desc), n)
        sc = torch.empty(sb, dtype=torch.uint8, device=DEV)
        _lib.check(L.wire_mlp_bwd_coords(s, C.byref(desc), packed.data_ptr(), x.data_ptr(), n, gy.data_ptr(),
                                         act.data_ptr(), ab, sc.data_ptr(), sb,
                                         _lib.ptr_array([g.data_ptr() for g in grads]), None), "bwd_coords")
    else:
        sb = L.wire_bwd_scratch_bytes(C.byref(desc), n)
        sc = torch.empty(sb, dtype=torch.uint8, device=DEV)
        _lib.check(L.wire_mlp_bwd(s, C.byref(desc), packed.data_ptr(), x.data_ptr(), n, gy.data_ptr(), act.data_ptr(),
                                  ab, sc.data_ptr(), sb, _lib.ptr_array([g.data_ptr() for g in grads])), "bwd")
    torch.cuda.synchronize()
    return [g.cpu() for g in grads]


@pytest.mark.parametrize("kind,D,hf,nl", FAMILY_CASES + [("relu_pe", 2, 128, 2)])
def test_abi_null_coords_equals_mlp_bwd(kind, D, hf, nl):
    model = _model(kind.replace("_pe", ""), D, hf, nl, pos_encode=kind.endswith("_pe"),
                   **(BENCH if kind == "wire" else CLASS))
    coords, w = _coords(6000, D), _weights(6000, 3)
    a, b = _abi_run(model, coords, w, False), _abi_run(model, coords, w, True)
    for ga, gb in zip(a, b):
        assert torch.equal(ga, gb)


# ---- 4. frozen parameters: coordinate optimisation ------------------------------------------------------------------
@pytest.mark.parametrize("kind,D,hf,nl,n", [("wire", 2, 363, 4, 65537), ("siren", 2, 256, 4, 65537),
                                            ("wire2d", 2, 128, 2, 8192), ("relu_pe", 3, 128, 2, 4133),
                                            ("wire", 2, 64, 0, 3000)])
def test_frozen_params(kind, D, hf, nl, n):
    from wire_amd import _lib
    L = _lib.lib()
    pe = kind.endswith("_pe")
    model = _model(kind.replace("_pe", ""), D, hf, nl, pos_encode=pe, **(BENCH if kind == "wire" else CLASS))
    coords, w = _coords(n, D), _weights(n, 3)
    _, _, gx_train = _fwd_bwd(model, coords, w, True)
    for p in model.parameters():
        p.requires_grad_(False)
        p.grad = None
    x = coords.to(torch.float32).to(DEV).requires_grad_(True)
    y = model(x)
    torch.cuda.synchronize()
    _lib.check(L.wire_prof_read((C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()), "prof_read")
    _lib.check(L.wire_prof_enable(1), "prof_enable")
    try:
        (y * w.to(torch.float32).to(DEV)).sum().backward()
        torch.cuda.synchronize()
        ms, launches, fl = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()
        _lib.check(L.wire_prof_read(ms, launches, fl), "prof_read")
    finally:
        L.wire_prof_enable(0)
    assert launches[2] == 0, f"weight-gradient GEMMs launched: {launches[2]}"
    assert torch.equal(x.grad.cpu(), gx_train.cpu())
    assert all(p.grad is None for p in model.parameters())


# ---- 5. per-layer path ----------------------------------------------------------------------------------------------
def test_gabor_first_layer_trainable_and_plain():
    from wire_amd.modules.wire import ComplexGaborLayer
    for trainable in (False, True):
        torch.manual_seed(3)
        layer = ComplexGaborLayer(2, 40, is_first=True, omega0=9.0, sigma0=4.0, trainable=trainable).to(DEV)
        coords, = (_coords(5000, 2),)
        gw = torch.randn(5000, 40, dtype=torch.complex128, generator=torch.Generator().manual_seed(4))
        x = coords.to(torch.float32).to(DEV).requires_grad_(True)
        out = layer(x)
        (out * gw.to(torch.complex64).to(DEV)).real.sum().backward()
        Wt, bt = layer.linear.weight.detach().cpu(), layer.linear.bias.detach().cpu()

        def fwd(c, double, rows=None):
            dt = torch.float64 if double else torch.float32
            return (torch_ref.gabor(F.linear(c, Wt.to(dt), bt.to(dt)), 9.0, 4.0) *
                    gw.to(torch.complex128 if double else torch.complex64)).real.sum(-1, keepdim=True)
        one = torch.ones(5000, 1, dtype=torch.float64)
        g64, g32 = oracle_coords_grad(fwd, coords, one, True), oracle_coords_grad(fwd, coords, one, False)
        within_ref(relmax(x.grad.cpu().numpy(), g64), relmax(g32, g64), f"coords_grad gabor_first trainable={trainable}")
        assert layer.linear.weight.grad is not None


def test_gabor2d_first_layer():
    from wire_amd.modules.wire2d import ComplexGaborLayer2D
    torch.manual_seed(5)
    layer = ComplexGaborLayer2D(2, 32, is_first=True, omega0=7.0, sigma0=3.0).to(DEV)
    coords = _coords(5000, 2)
    gw = torch.randn(5000, 32, dtype=torch.complex128, generator=torch.Generator().manual_seed(6))
    x = coords.to(torch.float32).to(DEV).requires_grad_(True)
    (layer(x) * gw.to(torch.complex64).to(DEV)).real.sum().backward()
    sd = {k: v.detach().cpu() for k, v in layer.state_dict().items() if "omega_0" not in k and "scale_0" not in k}

    def fwd(c, double, rows=None):
        dt = torch.float64 if double else torch.float32
        lin = F.linear(c, sd["linear.weight"].to(dt), sd["linear.bias"].to(dt))
        sy = F.linear(c, sd["scale_orth.weight"].to(dt), sd["scale_orth.bias"].to(dt))
        return (torch_ref.gabor2d(lin, sy, 7.0, 3.0) * gw.to(torch.complex128 if double else torch.complex64)).real.sum(-1, keepdim=True)
    one = torch.ones(5000, 1, dtype=torch.float64)
    g64, g32 = oracle_coords_grad(fwd, coords, one, True), oracle_coords_grad(fwd, coords, one, False)
    within_ref(relmax(x.grad.cpu().numpy(), g64), relmax(g32, g64), "coords_grad gabor2d_first")


def test_layerwise_relu_posenc():
    # (seed 0 at width 256: the last relu layer is alive on about two thirds of the rows)
    check_case("relu_posenc_layerwise_2x256_n4133", "relu", 2, 256, 2, 4133, CLASS, pos_encode=True,
               outermost_linear=False)


@pytest.mark.parametrize("D", [2, 3])
def test_posencoding_alone(D):
    from wire_amd.modules.relu import PosEncoding
    pe = PosEncoding(D, sidelength=256)
    pe.num_frequencies, pe.out_dim = 10, D + 2 * D * 10
    coords = _coords(4133, D)
    w = torch.randn(4133, pe.out_dim, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    x = coords.to(torch.float32).to(DEV).reshape(1, 4133, D).requires_grad_(True)
    (pe(x) * w.to(torch.float32).to(DEV)).sum().backward()

    def fwd(c, double, rows=None):
        return torch_ref.posenc(c, 10)
    g64 = oracle_coords_grad(fwd, coords, w, True)
    g32 = oracle_coords_grad(fwd, coords, w, False)
    within_ref(relmax(x.grad.reshape(4133, D).cpu().numpy(), g64), relmax(g32, g64), f"coords_grad posenc D={D}")


# ---- 6. shapes, dtypes, determinism ---------------------------------------------------------------------------------
def test_shapes_dtypes_determinism():
    model = _model("wire", 2, 363, 4, **BENCH)
    for n in (4133, 65537, 262145):
        coords, w = _coords(n, 2), _weights(n, 3)
        a = build_coords_grad(model, coords, w)
        b = build_coords_grad(model, coords, w)
        assert np.array_equal(a, b), f"not deterministic at n={n}"
        c = build_coords_grad(model, coords, w, shape=(1, n, 2))
        assert np.array_equal(a, c)
        g64 = build_coords_grad(model, coords, w, dtype=torch.float64)
        assert np.array_equal(a, g64)
    # non-contiguous coordinates
    coords, w = _coords(8192, 2), _weights(8192, 3)
    base = coords.to(torch.float32).to(DEV)
    xt = base.t().contiguous().t().requires_grad_(True)
    assert not xt.is_contiguous()
    (model(xt) * w.to(torch.float32).to(DEV)).sum().backward()
    assert np.array_equal(xt.grad.cpu().to(torch.float64).numpy(), build_coords_grad(model, coords, w))


# ---- 7. second order is out of scope --------------------------------------------------------------------------------
def test_create_graph_raises():
    model = _model("siren", 2, 64, 2, **CLASS)
    x = _coords(4096, 2).to(torch.float32).to(DEV).requires_grad_(True)
    y = model(x).sum()
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(y, x, create_graph=True)
    # without a coordinate gradient create_graph behaves as before (no error from this path)
    x2 = x.detach()
    y2 = model(x2).sum()
    torch.autograd.grad(y2, list(model.parameters()), create_graph=True)


# ---- 8. end to end: fit a translation in front of a frozen siren ----------------------------------------------------
def test_fit_translation_frozen_siren():
    model = _model("siren", 2, 64, 2, O=1, **CLASS)
    for p in model.parameters():
        p.requires_grad_(False)
    n, steps, lr = 4096, 40, 1e-2
    coords = _coords(n, 2, seed=11) * 0.5
    t_true = torch.tensor([0.031, -0.022], dtype=torch.float64)
    fwd = _oracle_forward("siren", model, 2, CLASS, None)
    with torch.no_grad():
        target64 = fwd(coords + t_true, True)

    def loop(step_fn, dtype):
        t = torch.zeros(2, dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([t], lr=lr)
        for _ in range(steps):
            opt.zero_grad()
            step_fn(t).backward()
            opt.step()
        return t.detach().to(torch.float64)

    tgt = target64.to(torch.float32).to(DEV)
    c32 = coords.to(torch.float32).to(DEV)

    def gpu_step(t):
        td = t.to(DEV)
        return ((model(c32 + td) - tgt) ** 2).mean()
    t_gpu = loop(gpu_step, torch.float32)
    t64 = loop(lambda t: ((fwd(coords + t, True) - target64) ** 2).mean(), torch.float64)
    t32 = loop(lambda t: ((fwd(coords.float() + t, False) - target64.float()) ** 2).mean(), torch.float32)
    err_ref = float((t32 - t64).abs().max())
    err = float((t_gpu - t64).abs().max())
    _util.RATIO_LOG.append(("coords_grad fit_translation siren 2x64 [|t - t64|]", err, err_ref))
    assert err <= max(4 * err_ref, 1e-4), (t_gpu, t64, t32)
    assert float((t64 - t_true).abs().max()) < float(t_true.abs().max())      # the loop does move towards t_true
