"""CPU-only checks of the SSIM metric: the restatement of tests/ssim_ref.py against closed forms and against
scipy's uniform filter, the two C-ABI symbols' argument checks (they return before any HIP call), and the argument
checks of the Python entry points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ssim_ref as ref


@pytest.mark.parametrize("kind", ["gaussian", "uniform"])
def test_restatement_closed_forms(kind):
    """Constant images x = a, y = b: every variance is 0, so S = (2ab + C1) / (a^2 + b^2 + C1) everywhere (the window is
    normalised in fp64 here so that its sum is 1 to rounding); y = x gives exactly 1."""
    win, cov = ref.window(kind)
    w64 = win.double() / win.double().sum()
    a, b, L = 0.3, 0.8, ref.DATA_RANGE[kind]
    x, y = np.full((15, 17, 2), a), np.full((15, 17, 2), b)
    mean, smap = ref.ssim_map(x, y, w64, cov, L, torch.float64)
    c1 = (0.01 * L) ** 2
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    assert smap.shape == (15 - len(win) + 1, 17 - len(win) + 1, 2)
    assert abs(smap.numpy() - want).max() <= 1e-12 and abs(mean - want) <= 1e-12
    gt, _ = ref.inputs((15, 17, 2), 0.1)
    for dtype in (torch.float64, torch.float32):
        mean, smap = ref.ssim_map(gt, gt, win, cov, L, dtype)
        assert mean == 1.0 and (smap == 1.0).all()


def test_uniform_crop_equals_valid_region():
    """skimage's route -- scipy.ndimage.uniform_filter(mode='reflect') of x, y, x^2, y^2, xy per channel, then the border
    of (7 - 1) / 2 = 3 cropped -- is the valid convolution of the restatement, to 1e-12 in fp64."""
    from scipy.ndimage import uniform_filter
    gt, rec = ref.inputs((19, 23, 3), 0.1)
    x, y = gt.astype(np.float64), rec.astype(np.float64)
    L, cov = 2.0, 49.0 / 48.0
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    maps = []
    for ch in range(3):
        a, b = x[..., ch], y[..., ch]
        f = lambda t: uniform_filter(t, size=7, mode="reflect")
        ux, uy = f(a), f(b)
        vx, vy, vxy = cov * (f(a * a) - ux * ux), cov * (f(b * b) - uy * uy), cov * (f(a * b) - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        maps.append(s[3:-3, 3:-3])
    want = np.stack(maps, -1)
    mean, smap = ref.ssim_map(x, y, torch.full((7,), 1.0 / 7.0, dtype=torch.float64), cov, L, torch.float64)
    assert abs(smap.numpy() - want).max() <= 1e-12
    assert abs(mean - np.mean([m.mean() for m in maps])) <= 1e-12        # the mean of per-channel means is the same number


def test_restatement_fp32_stays_inside_the_bounds():
    """The fp32 restatement's own error on the shared inputs is far below 1: the GPU bounds (2 x this + 1e-6) are tight."""
    for kind in ("gaussian", "uniform"):
        for sigma in ref.SIGMAS:
            c = ref.case((40, 37, 3), sigma, kind)
            assert np.abs(c["map32"] - c["map64"]).max() < 1e-4 and abs(c["mean32"] - c["mean64"]) < 1e-5


def test_abi_symbols_and_workspace_size():
    from wire_amd import _lib
    L = _lib.lib()
    for name in ("wire_ssim_ws_bytes", "wire_ssim"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    prev = 0
    for n in (11, 12, 27, 43, 100, 512, 4096):
        b = L.wire_ssim_ws_bytes(n, n, 3, 11)
        assert b > 0 and b >= prev
        assert L.wire_ssim_ws_bytes(n, 11, 3, 11) <= b and L.wire_ssim_ws_bytes(11, n, 3, 11) <= b
        prev = b
    for bad in [(10, 40, 3, 11), (40, 10, 3, 11), (40, 40, 0, 11), (40, 40, 9, 11), (40, 40, 3, 4), (40, 40, 3, 1),
                (40, 40, 3, 13)]:
        assert L.wire_ssim_ws_bytes(*bad) == -1
        assert b"wire_ssim_ws_bytes" in L.wire_last_error()


def test_abi_rejects_bad_arguments_before_any_hip_call():
    """Every refusal of include/wire_hip.h, on a machine without a GPU: the pointers are never dereferenced."""
    from wire_amd import _lib
    L = _lib.lib()
    win = (C.c_float * 11)(*ref.window("gaussian")[0].tolist())
    p = 4096                                  # stands for a device pointer; never read
    ws_bytes = L.wire_ssim_ws_bytes(40, 40, 3, 11)
    good = dict(stream=None, x=p, y=p, H=40, W=40, O=3, taps=11, window=win, cov=1.0, c1=1e-4, c2=9e-4, out1=p, map=None,
                ws=p, ws_bytes=ws_bytes)
    order = list(good)
    bad = [dict(x=None), dict(y=None), dict(window=None), dict(out1=None), dict(ws=None),
           dict(taps=4), dict(taps=10), dict(taps=1), dict(taps=13), dict(H=10), dict(W=10), dict(H=6, W=6, taps=7),
           dict(O=0), dict(O=9),
           dict(c1=math.nan), dict(c1=math.inf), dict(c2=math.nan), dict(c2=-math.inf), dict(cov=math.nan),
           dict(cov=math.inf)]
    for change in bad:
        args = dict(good, **change)
        L.wire_tune_get(b"no such knob")       # leaves another message behind
        assert L.wire_ssim(*[args[k] for k in order]) == -1, change
        assert b"wire_ssim" in L.wire_last_error(), change
    args = dict(good, ws_bytes=ws_bytes - 1)
    assert L.wire_ssim(*[args[k] for k in order]) == -3
    assert b"ws too small" in L.wire_last_error()


def test_python_entry_points_check_their_arguments():
    from wire_amd import _lib, functional
    from wire_amd.trainer import FusedTrainer
    assert callable(functional.ssim) and callable(FusedTrainer.ssim)
    a, b = torch.zeros(20 * 24, 3), torch.zeros(20 * 24, 3)
    with pytest.raises(_lib.WireHipError):
        functional.ssim(a, b, 20, 24)
    with pytest.raises(_lib.WireHipError):
        functional.ssim(a.reshape(20, 24, 3), b.reshape(1, 20 * 24, 3), 20, 24, window="uniform", data_range=2.0)
    with pytest.raises(ValueError, match="data_range"):
        functional.ssim(a, b, 20, 24, window="uniform")
    with pytest.raises(ValueError, match="smaller than"):
        functional.ssim(torch.zeros(100, 3), torch.zeros(100, 3), 10, 10)
    with pytest.raises(ValueError, match="smaller than"):
        functional.ssim(torch.zeros(24 * 6, 1), torch.zeros(24 * 6, 1), 24, 6, window="uniform", data_range=2.0)
    with pytest.raises(ValueError):
        functional.ssim(a, b[:-1], 20, 24)
    with pytest.raises(ValueError):
        functional.ssim(a, b, 20, 24, window=(4, 1.5))
    # the windows the library is handed are the restatement's, bit for bit
    for kind in ("gaussian", "uniform"):
        taps, w, cov = functional._ssim_window(kind)
        rw, rcov = ref.window(kind)
        assert taps == len(rw) and np.array(list(w), np.float32).tobytes() == rw.numpy().tobytes()
        assert np.float32(cov) == np.float32(rcov)
