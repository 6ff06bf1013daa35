"""GPU checks of the SSIM metric (wire_ssim, functional.ssim, FusedTrainer.ssim) against the fp64 restatement of
tests/ssim_ref.py, with the fp32 restatement's own error as the yardstick."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import within_ref
import ssim_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (H, W, O).  The first five are the shapes the metric is specified on: one Gaussian window (a 1 x 1 map; 5 x 5 for the
# uniform window), one uniform window, interleaved channels with ragged sizes, an image narrower than a tile, and the
# channel limit.  The others follow the kernel's tile of 16 x 32 output pixels (wire_ssim.hip, SSIM_TR x SSIM_TC) and
# its chunks of 128 floats of an output row (SSIM_LC):
#   (47, 81, 3)  the Gaussian map is 37 x 71 = two full tiles plus a ragged remainder of 5 rows / 7 columns, the uniform
#                map 41 x 75 = two full tiles plus 9 / 11;
#   (17, 44, 8)  the channel limit on a full-width tile: 32 x 8 = 256 floats of a row = two full chunks (and the largest
#                LDS footprint), plus a second tile of 2 (Gaussian) / 6 (uniform) columns;
#   (18, 45, 5)  32 x 5 = 160 floats = one full chunk plus a ragged one of 32.
# The launcher does not cap its grid (one workgroup per tile, whatever their number), so there is no beyond-cap shape.
SHAPES = [(11, 11, 1), (7, 7, 1), (12, 29, 3), (33, 8, 2), (15, 16, 8), (47, 81, 3), (17, 44, 8), (18, 45, 5)]
CASES = [(s, k) for s in SHAPES for k in ("gaussian", "uniform") if min(s[0], s[1]) >= len(ref.window(k)[0])]


def _call(x, y, win, cov, data_range, want_map=True):
    """wire_ssim on two [H, W, O] arrays; returns (out as a float32 scalar array, map or None)."""
    from wire_amd import _lib
    L = _lib.lib()
    H, W, O = x.shape
    taps = len(win)
    xt, yt = torch.tensor(x, device=DEV), torch.tensor(y, device=DEV)
    out = torch.full((1,), 7.0, device=DEV)
    smap = torch.full((H - taps + 1, W - taps + 1, O), 7.0, device=DEV) if want_map else None
    ws_bytes = _lib.check(L.wire_ssim_ws_bytes(H, W, O, taps), "ws_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    wh = (C.c_float * taps)(*win.tolist())
    _lib.check(L.wire_ssim(torch.cuda.current_stream().cuda_stream, xt.data_ptr(), yt.data_ptr(), H, W, O, taps, wh,
                           cov, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, out.data_ptr(),
                           smap.data_ptr() if want_map else None, ws.data_ptr(), ws_bytes), "wire_ssim")
    torch.cuda.synchronize()
    return out.cpu().numpy(), smap.cpu().numpy() if want_map else None


def _check(label, out, smap, c):
    """The two bounds of every comparison: the map through within_ref against the fp32 restatement's worst map error;
    the mean against twice the restatement's MEAN absolute map error plus 1e-6 (the error of a mean is at most the mean
    absolute error of its terms, plus the rounding of one fp32 sum)."""
    d32 = np.abs(c["map32"] - c["map64"])
    if smap is not None:
        assert smap.shape == c["map64"].shape and not (smap == 7.0).any()
        eb = np.abs(smap.astype(np.float64) - c["map64"]).max()
        print(f"{label}: map err {eb:.3e} (restatement {d32.max():.3e})")
        within_ref(eb, d32.max(), label + " map")
    em = abs(float(out) - c["mean64"])
    print(f"{label}: mean err {em:.3e} (restatement's mean |map error| {d32.mean():.3e})")
    within_ref(em, d32.mean(), label + " mean")


@pytest.mark.parametrize("shape,kind", CASES)
def test_ssim_matches_restatement(shape, kind):
    for sigma in ref.SIGMAS:
        c = ref.case(shape, sigma, kind)
        win, cov, L = c["win"], c["cov"], c["data_range"]
        out, smap = _call(c["gt"], c["rec"], win, cov, L)
        _check(f"ssim {shape} {kind} sigma={sigma}", out[0], smap, c)
        # no map: the same mean, bit for bit; and the same call twice
        assert _call(c["gt"], c["rec"], win, cov, L, want_map=False)[0].tobytes() == out.tobytes()
        again = _call(c["gt"], c["rec"], win, cov, L)
        assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == smap.tobytes()
    one, _ = _call(c["gt"], c["gt"], win, cov, L)
    print(f"ssim {shape} {kind} rec = gt: |out - 1| = {abs(float(one[0]) - 1.0):.3e}")
    assert abs(float(one[0]) - 1.0) <= 1e-6


def test_other_window_sizes():
    """The odd sizes between the two definitions' (3, 5, 9 taps; uniform weights, sample covariance) on the two-tile
    shape: the same bounds."""
    shape = (47, 81, 3)
    gt, rec = ref.inputs(shape, 0.1)
    for taps in (3, 5, 9):
        win = torch.full((taps,), 1.0 / taps, dtype=torch.float32)
        cov = taps * taps / (taps * taps - 1.0)
        mean64, map64 = ref.ssim_map(gt, rec, win, cov, 1.0, torch.float64)
        _, map32 = ref.ssim_map(gt, rec, win, cov, 1.0, torch.float32)
        c = dict(mean64=mean64, map64=map64.numpy(), map32=map32.numpy().astype(np.float64))
        out, smap = _call(gt, rec, win, cov, 1.0)
        _check(f"ssim {shape} {taps} uniform taps", out[0], smap, c)


def test_python_entry_points():
    """FusedTrainer.ssim on a small real net's render() against the trainer's target == functional.ssim on the same
    tensors, bit for bit; both inside the bounds; full=True returns the map; every accepted shape is the same call."""
    from wire_amd import functional
    from wire_amd.modules import models
    from wire_amd.trainer import FusedTrainer
    H, W, O = 40, 37, 3
    gt, _ = ref.inputs((H, W, O), 0.1)
    torch.manual_seed(0)
    net = lambda D, out: models.get_INR(nonlin="wire", in_features=D, out_features=out, hidden_features=32,
                                        hidden_layers=1).to(DEV)
    tr = FusedTrainer(net(2, O), (H, W), torch.tensor(gt.reshape(H * W, O)))
    img = tr.render()
    assert img.shape == (H * W, O)
    x = img.cpu().numpy().reshape(H, W, O)
    for kind in ("gaussian", "uniform"):
        L = ref.DATA_RANGE[kind]
        kw = dict(window=kind, data_range=None if kind == "gaussian" else L)
        win, cov = ref.window(kind)
        mean64, map64 = ref.ssim_map(gt, x, win, cov, L, torch.float64)
        _, map32 = ref.ssim_map(gt, x, win, cov, L, torch.float32)
        c = dict(mean64=mean64, map64=map64.numpy(), map32=map32.numpy().astype(np.float64))
        a = tr.ssim(img, **kw)
        b = functional.ssim(img, tr.target, H, W, **kw)
        assert a.shape == () and a.is_cuda and a.dtype == torch.float32
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        a2, smap = tr.ssim(img, full=True, **kw)                       # (the kept workspace, a second time)
        assert smap.shape == (H - len(win) + 1, W - len(win) + 1, O)
        assert a2.cpu().numpy().tobytes() == a.cpu().numpy().tobytes()
        _check(f"FusedTrainer.ssim {kind}", a.cpu().numpy(), smap.cpu().numpy(), c)
        b3, smap3 = functional.ssim(img.reshape(H, W, O), tr.target.reshape(1, H * W, O), H, W, full=True, **kw)
        assert b3.cpu().numpy().tobytes() == a.cpu().numpy().tobytes() and torch.equal(smap3, smap)
        assert tr.ssim(img, gt=torch.tensor(gt, device=DEV), **kw).cpu().numpy().tobytes() == a.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="target"):
        FusedTrainer(net(2, O), (H, W), None).ssim(img)
    with pytest.raises(ValueError, match="3-D"):
        FusedTrainer(net(3, 1), (8, 8, 8), None).ssim(torch.zeros(512, 1, device=DEV))
