"""The nets, widths and oracles of the shape-envelope tests (tests/test_gpu_shape_envelope.py on the GPU,
tests/test_shape_envelope_host.py on the host): make_plan accepts in_features 1..4 and out_features 1..8 for every net
kind, and these cases run the values no other test reaches.

Two restatements of every kind, both on the host:
  * numpy (``np_step``): oracle/wire_oracle.py and tests/{bspline,mscale,mscale2,hier,mfn}_ref.py -- output, MSE loss and
    every parameter gradient, fp64 (the oracle) or fp32 (the reference's own arithmetic, the yardstick err_ref);
  * eager torch (``eager_forward``): the same formulas as differentiable functions of the coordinates and of a dict of
    tensors, so autograd gives the gradient of ANY loss, the coordinates' included (oracle/torch_ref.py for the five
    plain kinds; the B-spline kinds and the filter network below, restating the numpy files operation by operation).
"""
import numpy as np
import torch
import torch.nn.functional as F

import bspline_ref as br
import hier_ref as hr
import mfn_ref as mfr
import mscale2_ref as m2r
import mscale_ref as msr
from _util import oracle_grads_chunked
from oracle import torch_ref
from oracle import wire_oracle as wo

LAYERS = 2
# every untested width: D = 1 and 4, O = 2 and 5..8; each new D meets a fused O (<= 4) and an unfused one
WIDTHS = [(1, 8), (4, 2), (4, 5), (3, 7), (2, 6)]
# 333: the small-batch 3 x bf16 32 x 32 kernels; 4096 + 37: the 2 x fp16 route and the whole-net kernels, ragged last tile
ROWS = [333, 4096 + 37]
HL_NET = dict(shf=130, st=[1.0, 2.0])
# name: kind, hidden_features, get_INR keywords -- each kind in the regime its own GPU tests use
NETS = {
    "wire_k90": dict(kind="wire", hf=128, kw=dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)),
    "wire_k256": dict(kind="wire", hf=363, kw=dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)),
    "wire2d": dict(kind="wire2d", hf=128, kw=dict(first_omega_0=10.0, hidden_omega_0=10.0, scale=10.0)),
    "siren": dict(kind="siren", hf=256, kw=dict(first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0)),
    "gauss": dict(kind="gauss", hf=256, kw=dict(first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0)),
    "relu": dict(kind="relu", hf=256, kw=dict(first_omega_0=30.0, hidden_omega_0=30.0, scale=10.0)),
    "bspline_form": dict(kind="bspline_form", hf=256, kw=dict(first_omega_0=-0.2, hidden_omega_0=-0.2, scale=0.25)),
    "bspline_mscale_HL": dict(kind="bspline_mscale_HL", hf=256, st=HL_NET["st"],
                              kw=dict(first_omega_0=-0.2, hidden_omega_0=-0.2, scale=1.0,
                                      scaled_hidden_features=HL_NET["shf"])),
    "bspline_mscale_2": dict(kind="bspline_mscale_2", hf=64, st=[1 / 9, 4.0],
                             kw=dict(first_omega_0=-0.2, hidden_omega_0=-0.2, scale=0.0, scaled_hidden_features=0)),
    "bspline_mscale_hier": dict(kind="bspline_mscale_hier", hf=64, st=[1 / 9, 4.0],
                                kw=dict(first_omega_0=-0.2, hidden_omega_0=-0.2, scale=0.0, scaled_hidden_features=0)),
    "mfn": dict(kind="mfn", hf=128, kw={}),
    # the positional encoding in front of relu (D = 1: 6 frequencies, 13 inputs; D = 3: 10 frequencies, 63 inputs)
    "relu_posenc": dict(kind="relu", hf=256, kw=dict(pos_encode=True, sidelength=256)),
    # the combiner at its maximum: 8 scales x 8 outputs = 64 = M2_MAXSO inputs
    "bspline_mscale_2_s8": dict(kind="bspline_mscale_2", hf=64, st=[1 / 9, 1 / 4, 1 / 2, 1.0, 2.0, 4.0, 8.0, 16.0],
                                kw=dict(first_omega_0=-0.2, hidden_omega_0=-0.2, scale=0.0, scaled_hidden_features=0)),
}
MAIN_NETS = [k for k in NETS if k not in ("relu_posenc", "bspline_mscale_2_s8")]
PLAIN = ("wire", "wire2d", "siren", "gauss", "relu")


def build(net, D, O, device="cpu", seed=0):
    """The wire_amd model of a case, as the kind's own tests build it (torch.manual_seed, then the constructor)."""
    from wire_amd.modules import mfn, models
    c = NETS[net]
    torch.manual_seed(seed)
    if c["kind"] == "mfn":
        return mfn.INR(D, c["hf"], LAYERS, O).to(device)
    kw = dict(c["kw"])
    if "st" in c:
        kw["scale_tensor"] = torch.tensor(c["st"])
    return models.get_INR(nonlin=c["kind"], in_features=D, out_features=O, hidden_features=c["hf"],
                          hidden_layers=LAYERS, **kw).to(device)


def coords(n, D, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, (n, D)).astype(np.float32)


M2_MARGIN = 2e-4


def case_coords(net, sd, n, D, seed=1):
    """The n coordinate rows of a case.  bspline_mscale_2 ends in Linear, ReLU, Linear: a hidden unit whose pre-activation h
    is round-off away from 0 gets its gradient from one correct implementation and 0 from another (what the forced
    decisions settle for the relu kind), and one such row moves g_coords of that row by O(1).  Its cases therefore keep
    the first n rows of the uniform draw on which every |h| of the fp64 restatement is at least M2_MARGIN -- some 20 x the
    fp32 restatement's own error in h -- so that the decision is the same in every arithmetic.  Every other net: the draw.
    (The build's own decisions cannot be imposed instead, as they are for the relu kind: the combiner kernel evaluates h in
    registers and stores neither h nor its sign, and a second evaluation in another order differs at exactly the round-off
    that decides.)  The filter is fp64 arithmetic on the host, so what it drops is fixed: at these seeds 11 - 40 of the
    first 344 - 373 rows drawn for a 333-row case, 232 - 458 of 4365 - 4591 for 4133 rows, 235 - 411 of 4331 - 4507 for
    the 4096-row sample (3 - 10 %); each call prints its count."""
    if NETS[net]["kind"] != "bspline_mscale_2":
        return coords(n, D, seed)
    x = coords(2 * n, D, seed)
    X = m2r.forward(sd, LAYERS, x.astype(np.float64), NETS[net]["st"], np.float64, keep=True)[1][0]
    h = X @ sd[m2r.COMB[0]].astype(np.float64).T + sd[m2r.COMB[1]].astype(np.float64)
    keep = np.abs(h).min(1) >= M2_MARGIN
    assert keep.sum() >= n, f"{net}: {int(keep.sum())} of {2 * n} rows have settled decisions, {n} needed"
    scanned = int(np.flatnonzero(keep)[n - 1]) + 1
    print(f"{net} D={D} n={n} seed={seed}: {scanned - n} of the first {scanned} rows drawn dropped (some |h| < {M2_MARGIN:g})")
    return x[keep][:n]


def targets(n, O, seed=2):
    return np.random.default_rng(seed).uniform(0, 1, (n, O)).astype(np.float32)


def state(model):
    """Every tensor the restatements read, by state_dict key, as numpy arrays (the hierarchical net's heads, which are in
    no state_dict, as "linears.{s}.*"); the layers' omega_0 / scale_0 entries travel in the descriptor, not here."""
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if "omega_0" not in k and "scale_0" not in k}
    for s, lin in enumerate(getattr(model, "linears", [])):
        sd[f"linears.{s}.weight"], sd[f"linears.{s}.bias"] = lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy()
    return sd


def posenc_freqs(net, D):
    c = NETS[net]
    return wo.posenc_num_frequencies(D, c["kw"]["sidelength"]) if c["kw"].get("pos_encode") else None


def final_bias_keys(net, sd):
    """The tensors that are a mean of dL/dy (tests/_util.final_bias_within_ref): the bias of the last linear."""
    kind = NETS[net]["kind"]
    if kind == "bspline_mscale_2":
        return [m2r.COMB[3]]
    if kind == "bspline_mscale_hier":
        return [k for k in sd if k.startswith("linears.") and k.endswith(".bias")]
    if kind == "mfn":
        return [f"linear.{LAYERS}.bias"]
    return [f"net.{LAYERS + 1}.bias"]


# ---------------------------------------------------------------------------------------------------------------------
# numpy: output, MSE loss and every parameter gradient
# ---------------------------------------------------------------------------------------------------------------------
def np_step(net, sd, x, t, double, relu_masks=None):
    """(y, loss, {key: gradient}) of mean((y - t)^2) over all rows, fp64 or fp32.  relu: ``relu_masks`` forces the
    decisions (oracle.realnet_backward)."""
    c = NETS[net]
    kind, kw = c["kind"], c["kw"]
    dt = np.float64 if double else np.float32
    xx, tt = x.astype(dt), t.astype(dt)
    if kind in PLAIN:
        y, loss, g = oracle_grads_chunked(kind, sd, x, t, LAYERS, kw.get("first_omega_0", 30.0),
                                          kw.get("hidden_omega_0", 30.0), kw.get("scale", 10.0), double,
                                          posenc_freqs(net, x.shape[1]), relu_masks=relu_masks)
        g.pop("flips", None), g.pop("flip_lin_max", None)
        return y, loss, g
    if kind == "bspline_form":
        return br.loss_and_grads(sd, LAYERS, xx, tt, kw["scale"], dt)
    if kind == "bspline_mscale_HL":
        return msr.loss_and_grads(sd, LAYERS, xx, tt, c["st"], kw["scale"], dt)
    if kind == "bspline_mscale_2":
        return m2r.loss_and_grads(sd, LAYERS, xx, tt, c["st"], dt)[:3]
    if kind == "bspline_mscale_hier":
        heads = {k: v for k, v in sd.items() if k.startswith("linears.")}
        return hr.loss_and_grads(sd, heads, LAYERS, xx, tt, c["st"], dt)[:3]
    if kind == "mfn":
        return mfr.loss_and_grads(sd, LAYERS, xx, tt, dt)[:3]
    raise ValueError(kind)


def relu_decisions(net, sd, x):
    """The fp64 oracle's own relu decisions lin_l > 0 (l = 0 .. L): imposed on BOTH precisions they make the fp32
    yardstick of a relu net a round-off figure instead of a count of flipped decisions."""
    kw = NETS[net]["kw"]
    _, cache = wo.realnet_forward("relu", wo.cast_params(sd, True), x.astype(np.float64), LAYERS, 30.0, 30.0,
                                  kw.get("scale", 10.0), posenc_freqs(net, x.shape[1]), keep=True)
    return [lin > 0 for lin in cache["lin"]]


# ---------------------------------------------------------------------------------------------------------------------
# eager torch: y as a differentiable function of the coordinates and the parameters
# ---------------------------------------------------------------------------------------------------------------------
def t_bspline(r, double):
    """B of tests/bspline_ref.py: the closed form in fp64, the reference's four-relu form in fp32."""
    if not double:
        q = lambda v: F.relu(v).square()
        return 0.5 * q(r + 1.5) - 1.5 * q(r + 0.5) + 1.5 * q(r - 0.5) - 0.5 * q(r - 1.5)
    a = r.abs()
    return torch.where(a <= 0.5, 0.75 - r * r, torch.where(a < 1.5, 0.5 * (1.5 - a).square(), torch.zeros_like(r)))


def _bchain(p, keys, h, s, double):
    for wk, bk in keys:
        h = t_bspline(F.linear(h, p[wk], p[bk]) / s, double)
    return h


def tensors(sd, double, requires_grad=False):
    """The numpy state as torch tensors of the run's precision."""
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        t = t.to(torch.complex128 if double else torch.complex64) if t.is_complex() else \
            t.to(torch.float64 if double else torch.float32)
        out[k] = t.clone().requires_grad_(requires_grad)
    return out


def eager_forward(net, p, x, double, relu_masks=None, rows=slice(None)):
    """y [n][O] of the net on coordinates x [n][D] with the tensors p (``tensors``).  relu: ``relu_masks`` (per layer
    [n][K] bool, rows ``rows`` of them) replaces the decisions, as tests/test_gpu_coords_grad._oracle_forward does."""
    c = NETS[net]
    kind, kw = c["kind"], c["kw"]
    L = LAYERS
    if kind in PLAIN:
        om1, om, sc = kw.get("first_omega_0", 30.0), kw.get("hidden_omega_0", 30.0), kw.get("scale", 10.0)
        if kind == "wire":
            return torch_ref.wire_forward(p, x, L, om1, om, sc)
        if kind == "wire2d":
            return torch_ref.wire2d_forward(p, x, L, om1, om, sc)
        nf = posenc_freqs(net, x.shape[1])
        if kind == "relu" and relu_masks is not None:
            h = x if nf is None else torch_ref.posenc(x, nf)
            for l in range(L + 1):
                lin = F.linear(h, p[f"net.{l}.linear.weight"], p[f"net.{l}.linear.bias"])
                h = lin * torch.as_tensor(relu_masks[l][rows]).to(lin.dtype)
            return F.linear(h, p[f"net.{L + 1}.weight"], p[f"net.{L + 1}.bias"])
        return torch_ref.realnet_forward(kind, p, x, L, om1, om, sc, nf)
    lk = lambda pre, l: (f"{pre}{l}.linear.weight", f"{pre}{l}.linear.bias")
    if kind == "bspline_form":
        h = _bchain(p, [lk("net.", l) for l in range(L + 1)], x, kw["scale"], double)
        return F.linear(h, p[f"net.{L + 1}.weight"], p[f"net.{L + 1}.bias"])
    if kind == "bspline_mscale_HL":
        W0 = p["net.0.linear.weight"]
        div = torch.as_tensor(c["st"], dtype=x.dtype)[torch.as_tensor(msr.column_groups(W0.shape[0], len(c["st"])))]
        with torch.no_grad():                       # the frozen first stage passes no gradient
            h = t_bspline(F.linear(x, W0, p["net.0.linear.bias"]) / div, double)
        nl = 1 + max(L - 1, 0)
        h = _bchain(p, [lk("net.", l) for l in range(1, nl + 1)], h, kw["scale"], double)
        return F.linear(h, p[f"net.{nl + 1}.weight"], p[f"net.{nl + 1}.bias"])
    if kind == "bspline_mscale_2":
        outs = []
        for s in c["st"]:
            h = _bchain(p, [lk("net.", l) for l in range(L + 1)], x, s, double)
            outs.append(F.linear(h, p[f"net.{L + 1}.weight"], p[f"net.{L + 1}.bias"]))
        h = F.relu(F.linear(torch.cat(outs, -1), p[m2r.COMB[0]], p[m2r.COMB[1]]))
        return F.linear(h, p[m2r.COMB[2]], p[m2r.COMB[3]])
    if kind == "bspline_mscale_hier":
        y, prev = None, None
        for s, sig in enumerate(c["st"]):
            h = x
            for l in hr.used_layers(s, L):
                if s > 0 and l == 1:
                    h = torch.cat([h, prev], -1)
                h = _bchain(p, [lk(f"stages.{s}.", l)], h, sig, double)
            prev = h
            v = F.linear(h, p[f"linears.{s}.weight"], p[f"linears.{s}.bias"])
            y = v if y is None else y + v
        return y
    if kind == "mfn":
        def filt(i):
            mu, gamma = p[f"gabon_filters.{i}.mu"], p[f"gabon_filters.{i}.gamma"]
            w, cc = p[f"gabon_filters.{i}.linear.weight"], p[f"gabon_filters.{i}.linear.bias"]
            nrm = (x ** 2).sum(1)[:, None] + (mu ** 2).sum(1)[None, :] - 2 * x @ mu.T
            return torch.exp(-gamma[None, :] / 2 * nrm) * torch.sin(F.linear(x, w, cc))
        z = filt(0)
        for i in range(L):
            z = F.linear(z, p[f"linear.{i}.weight"], p[f"linear.{i}.bias"]) * filt(i + 1)
        return F.linear(z, p[f"linear.{L}.weight"], p[f"linear.{L}.bias"])
    raise ValueError(kind)


def eager_grads(net, sd, x, double, loss_fn, relu_masks=None, chunk=2048):
    """Autograd of sum over row chunks of loss_fn(y_chunk, rows): (y, g_coords, {key: gradient}) as float64 numpy arrays
    (complex gradients in PyTorch's convention, as complex arrays).  A key no gradient reaches is absent."""
    dt = torch.float64 if double else torch.float32
    p = tensors(sd, double, requires_grad=True)
    ys, gxs = [], []
    for a in range(0, x.shape[0], chunk):
        rows = slice(a, a + chunk)
        xc = torch.as_tensor(x[rows]).to(dt).requires_grad_(True)
        y = eager_forward(net, p, xc, double, relu_masks, rows)
        loss_fn(y, rows).backward()
        ys.append(y.detach().to(torch.float64).numpy())
        gxs.append(None if xc.grad is None else xc.grad.to(torch.float64).numpy())
    gx = None if any(g is None for g in gxs) else np.concatenate(gxs, 0)
    grads = {k: (v.grad.to(torch.complex128) if v.is_complex() else v.grad.to(torch.float64)).numpy()
             for k, v in p.items() if v.grad is not None}
    return np.concatenate(ys, 0), gx, grads
