"""CPU-only checks of the TV prior of the operator steps: the restatement of tests/tv_reg_ref.py against the 2-D one of
tests/tv_ref.py and against torch autograd in fp64, wire_tv_add_grad's declaration and its refusal of bad arguments
(before any HIP call, so on a machine without a GPU), and the keyword refusals of step_radon, step_downsampled and
step_coded that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _util import ROOT  # noqa: F401  (puts the repository on sys.path)
import tv_ref
import tv_reg_ref as ref


def test_restatement_matches_the_2d_one_and_autograd():
    """T = 1: tv_s, k_s and the fp32 gradient are those of tv_ref on the channel-first image, tv_t = 0 = k_t.  T > 1, in
    fp64: loss and accumulated gradient equal torch autograd of the three sums to 1e-12; pattern_from replaces the
    comparisons' image; k_s stays in -4 .. 4 and k_t in -2 .. 2, and ties give zeros."""
    rng = np.random.default_rng(5)
    H, W, O = 6, 5, 3
    y = (np.round(rng.standard_normal((H * W, O)) * 4) / 4).astype(np.float32)
    ks, kt = ref.sign_patterns(y, H, W, 1, O)
    k2 = tv_ref.tv_sign_pattern(tv_ref.channel_first(y, H, W, O)).transpose(1, 2, 0).reshape(H * W, O)
    assert np.array_equal(ks, k2) and not kt.any() and (ks == 0).any()
    tvs, tvt = ref.tv_sums(y, H, W, 1, O)
    assert tvs == float(tv_ref.total_variation(tv_ref.channel_first(y, H, W, O), True)) and tvt == 0.0
    _, _, _, g32 = ref.tv_add_grad(y, np.zeros_like(y), H, W, 1, O, 0.25, 0.0, double=False)
    assert g32.dtype == np.float32 and g32.tobytes() == (np.float32(0.25) * k2.astype(np.float32)).tobytes()

    H, W, T, O, ls, lt = 4, 5, 6, 2, 2.0 ** -3, 2.0 ** -5
    y = np.round(rng.standard_normal((H * W * T, O)) * 4) / 4
    g_in = rng.standard_normal(y.shape)
    yt = torch.tensor(y, requires_grad=True)
    x = yt.reshape(H, W, T, O)
    tv_s = (x[1:] - x[:-1]).abs().sum() + (x[:, 1:] - x[:, :-1]).abs().sum()
    tv_t = (x[:, :, 1:] - x[:, :, :-1]).abs().sum()
    total = 0.75 + ls * tv_s + lt * tv_t
    total.backward()
    loss, tvs, tvt, g = ref.tv_add_grad(y, g_in, H, W, T, O, ls, lt, data=0.75)
    assert abs(loss - total.item()) <= 1e-12 * abs(loss)
    assert abs(tvs - tv_s.item()) <= 1e-12 * tvs and abs(tvt - tv_t.item()) <= 1e-12 * tvt
    assert np.abs(g - (g_in + yt.grad.numpy())).max() <= 1e-12
    ks, kt = ref.sign_patterns(y, H, W, T, O)
    assert np.abs(ks).max() == 4 and np.abs(kt).max() == 2 and (ks == 0).any() and (kt == 0).any()
    _, _, _, gp = ref.tv_add_grad(y + 1e-9 * rng.standard_normal(y.shape), g_in, H, W, T, O, ls, lt, pattern_from=y)
    assert np.array_equal(gp, g)
    # the per-frame spatial sum is the reference's function on (T, O, H, W)
    frames = np.asarray(y).reshape(H, W, T, O).transpose(2, 3, 0, 1)
    assert abs(float(tv_ref.total_variation(frames, True)) - tvs) <= 1e-12 * tvs
    # the fp32 total is the header's expression
    l32 = ref.total_loss(0.75, ls, tvs, lt, tvt)
    assert l32.dtype == np.float32 and abs(float(l32) - loss) <= 1e-6 * loss


def test_header_declares_the_entry_point_and_lib_lists_it():
    from wire_amd import _lib
    text = open(os.path.join(ROOT, "include", "wire_hip.h")).read()
    m = re.search(r"\bint\s+wire_tv_add_grad\s*\(([^)]*)\)\s*;", text)
    assert m, "include/wire_hip.h does not declare wire_tv_add_grad"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["stream", "y", "H", "W", "T", "O", "lambda_s", "lambda_t",
                                                         "data_loss", "g_y", "loss_out", "partial"]
    assert "wire_tv_add_grad" in _lib.SYMBOLS
    L = _lib.lib()
    assert len(L.wire_tv_add_grad.argtypes) == len(args)


def test_wire_tv_add_grad_refuses_bad_arguments():
    """H, W, T or O < 1, O > 8, a lambda that is not finite, sizes beyond 63 bits and a NULL y, g_y, loss_out or partial
    return -1 and name the entry point in wire_last_error(), before any HIP call (NULL stream, host buffers)."""
    from wire_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    big = (1 << 31) - 1

    def op(y=p, H=4, W=5, T=3, O=2, ls=0.5, lt=0.25, data=p, g=p, loss=p, part=p):
        return L.wire_tv_add_grad(None, y, H, W, T, O, ls, lt, data, g, loss, part)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(H=0), dict(W=0), dict(T=0), dict(O=0), dict(H=-1), dict(W=-3), dict(T=-1), dict(O=-2), dict(O=9),
               dict(ls=nan), dict(lt=nan), dict(ls=inf), dict(lt=-inf), dict(ls=-inf), dict(lt=inf),
               dict(H=big, W=big, T=big, O=8), dict(H=big, W=big, T=3, O=1),
               dict(y=None), dict(g=None), dict(loss=None), dict(part=None)):
        assert op(**kw) == -1, kw
        assert b"wire_tv_add_grad" in L.wire_last_error()


class _Bare:
    """The attributes the three steps read before they touch the device."""

    def __init__(self, grid, world=1, O=1):
        self.grid, self.world, self.O = grid, world, O
        self.tz = object() if len(grid) == 3 else None


def _call(name, bare, *a, **kw):
    from wire_amd.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr.__dict__.update(bare.__dict__)
    return getattr(tr, name)(*a, **kw)


def test_keywords_and_their_defaults():
    from wire_amd.trainer import FusedTrainer
    for name, kws in (("step_radon", ["lambda_tv"]), ("step_downsampled", ["lambda_tv"]),
                      ("step_coded", ["lambda_tv", "lambda_tv_t"])):
        sig = inspect.signature(getattr(FusedTrainer, name))
        for k in kws:
            assert sig.parameters[k].default == 0.0, (name, k)
    assert "lambda_tv" not in inspect.signature(FusedTrainer.step_frames).parameters
    assert "canonical grid" in FusedTrainer.step_frames.__doc__


def test_step_refusals_without_a_device():
    """A non-finite lambda is a ValueError naming the argument; step_coded with a slab that splits the grid and a nonzero
    lambda is a ValueError naming slab; the grid-rank and world > 1 refusals stay, lambda or not."""
    x = torch.zeros(1)
    bad_values = (float("nan"), float("inf"), -float("inf"))
    for bad in bad_values:
        with pytest.raises(ValueError, match="lambda_tv must be finite"):
            _call("step_radon", _Bare((4, 5)), x, x, lambda_tv=bad)
        with pytest.raises(ValueError, match="lambda_tv must be finite"):
            _call("step_downsampled", _Bare((4, 5), O=3), x, 2, lambda_tv=bad)
        with pytest.raises(ValueError, match="lambda_tv must be finite"):
            _call("step_coded", _Bare((4, 5, 6)), x, x, 2, lambda_tv=bad)
        with pytest.raises(ValueError, match="lambda_tv_t must be finite"):
            _call("step_coded", _Bare((4, 5, 6)), x, x, 2, lambda_tv_t=bad)
    for kw in (dict(lambda_tv=0.1), dict(lambda_tv_t=0.1), dict(lambda_tv=-0.1, lambda_tv_t=0.2)):
        for slab in (1, 7, 19):
            with pytest.raises(ValueError, match="slab"):
                _call("step_coded", _Bare((4, 5, 6)), x, x, 2, slab=slab, **kw)
    # the existing refusals come first
    with pytest.raises(ValueError, match="2-D grid"):
        _call("step_radon", _Bare((4, 5, 6)), x, x, lambda_tv=0.1)
    with pytest.raises(ValueError, match="2-D grid"):
        _call("step_downsampled", _Bare((4, 5, 6)), x, 2, lambda_tv=0.1)
    with pytest.raises(ValueError, match="3-D grid"):
        _call("step_coded", _Bare((4, 5)), x, x, 2, lambda_tv=0.1)
    with pytest.raises(NotImplementedError, match="single-process"):
        _call("step_radon", _Bare((4, 5), world=2), x, x, lambda_tv=0.1)
    with pytest.raises(NotImplementedError, match="single-process"):
        _call("step_downsampled", _Bare((4, 5), world=2), x, 2, lambda_tv=0.1)
    with pytest.raises(NotImplementedError, match="single-process"):
        _call("step_coded", _Bare((4, 5, 6), world=2), x, x, 2, lambda_tv_t=0.1)
    # a slab that does not split the grid is not refused for its lambda: the next check (the coded tensor) speaks
    with pytest.raises(ValueError, match="coded must be"):
        _call("step_coded", _Bare((4, 5, 6)), x, x, 2, slab=20, lambda_tv=0.1)
    with pytest.raises(ValueError, match="coded must be"):
        _call("step_coded", _Bare((4, 5, 6)), x, x, 2, slab=3)
