"""CPU-only checks of volume CT: the per-slice restatement of tests/radon_volume_ref.py against oracle/torch_ref.radon
and fp64 autograd, the declarations of wire_radon_vol_fwd / wire_radon_vol_bwd and their refusal of bad arguments
(before any HIP call, so on a machine without a GPU), and the refusals of FusedTrainer.step_radon_volume and
lin_inverse.radon_volume that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _util import ROOT, relmax  # noqa: F401  (puts the repository on sys.path)
import radon_volume_ref as ref
from oracle import torch_ref

NAMES = ("wire_radon_vol_fwd", "wire_radon_vol_bwd")


@pytest.mark.parametrize("H,W,Cn", [(24, 30, 3), (5, 17, 4), (9, 6, 1)])
def test_restatement_equals_the_oracle_per_slice(H, W, Cn):
    """Channel c of the restatement == torch_ref.radon on slice c in fp64 to 1e-12 relative, the adjoint == fp64
    autograd of the oracle on the channel-last volume, and <A x, y> == <x, A^T y>."""
    vol, g, ang = ref.case(H, W, Cn)
    x = torch.tensor(vol, dtype=torch.float64, requires_grad=True)
    s = torch.stack([torch_ref.radon(x[:, :, c], torch.tensor(ang)) for c in range(Cn)], dim=2)
    s.backward(torch.tensor(g, dtype=torch.float64))
    mine = ref.radon_volume(vol, ang)
    assert mine.shape == (len(ang), W, Cn) and mine.dtype == np.float64
    assert relmax(mine, s.detach().numpy()) <= 1e-12
    adj = ref.radon_volume_adjoint(g, ang, H, W)
    assert adj.shape == (H, W, Cn) and relmax(adj, x.grad.numpy()) <= 1e-12
    lhs, rhs = float((mine * g).sum()), float((adj * vol).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    # the fp32 yardstick is a real error, not zero
    assert 0 < relmax(ref.radon_volume(vol, ang, np.float32), mine) < 1e-5


def test_header_declares_the_entry_points_and_lib_lists_them():
    from wire_amd import _lib
    text = open(os.path.join(ROOT, "include", "wire_hip.h")).read()
    L = _lib.lib()
    for name, first, last in ((NAMES[0], "vol", "sino"), (NAMES[1], "g_sino", "g_vol")):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"include/wire_hip.h does not declare {name}"
        args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
        assert args == ["stream", first, "angles_deg", "H", "W", "C", "nangles", last]
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == len(args)


def test_entry_points_refuse_bad_arguments():
    """H, W, C or nangles < 1, H W or nangles W beyond 31 bits and each NULL pointer return -1 and name the entry
    point in wire_last_error(), before any HIP call (NULL stream, host buffers that are never dereferenced)."""
    from wire_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    big = 1 << 16
    for name in NAMES:
        fn = getattr(L, name)

        def op(a=p, ang=p, H=4, W=5, Cn=3, A=2, b=p):
            return fn(None, a, ang, H, W, Cn, A, b)

        for kw in (dict(H=0), dict(W=0), dict(Cn=0), dict(A=0), dict(H=-1), dict(W=-3), dict(Cn=-1), dict(A=-2),
                   dict(H=big, W=big), dict(A=big, W=big), dict(a=None), dict(ang=None), dict(b=None)):
            assert op(**kw) == -1, (name, kw)
            assert name.encode() in L.wire_last_error(), (name, kw)


class _Bare:
    """The attributes the step reads before it touches the device."""

    def __init__(self, grid, world=1, O=1):
        self.grid, self.world, self.O = grid, world, O
        self.tz = object() if len(grid) == 3 else None


def _call(bare, *a, **kw):
    from wire_amd.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr.__dict__.update(bare.__dict__)
    return tr.step_radon_volume(*a, **kw)


def test_signature_and_docstring():
    from wire_amd.modules import lin_inverse
    from wire_amd.trainer import FusedTrainer
    sig = inspect.signature(FusedTrainer.step_radon_volume)
    assert list(sig.parameters) == ["self", "sinogram", "thetas", "slab", "lambda_tv", "lambda_tv_t"]
    assert sig.parameters["slab"].default is None
    assert sig.parameters["lambda_tv"].default == 0.0 and sig.parameters["lambda_tv_t"].default == 0.0
    doc = FusedTrainer.step_radon_volume.__doc__
    assert "EXTRA FORWARD" in doc and "self.y_vol" in doc
    assert "radon(v.permute(2, 0, 1)[None], angles, is_3d=True).permute(1, 2, 0)" in lin_inverse.radon_volume.__doc__


def test_step_refusals_without_a_device():
    """A 2-D grid, out_features != 1, world > 1, a sinogram of the wrong size (or not CUDA float32), a lambda that is not
    finite and slab < 1: each before the first device access, in the style of the other steps."""
    x, th = torch.zeros(1), torch.zeros(3)
    with pytest.raises(ValueError, match="3-D grid"):
        _call(_Bare((4, 5)), x, th)
    with pytest.raises(ValueError, match="out_features == 1"):
        _call(_Bare((4, 5, 6), O=3), x, th)
    with pytest.raises(NotImplementedError, match="single-process"):
        _call(_Bare((4, 5, 6), world=2), x, th)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="lambda_tv must be finite"):
            _call(_Bare((4, 5, 6)), x, th, lambda_tv=bad)
        with pytest.raises(ValueError, match="lambda_tv_t must be finite"):
            _call(_Bare((4, 5, 6)), x, th, lambda_tv_t=bad)
    for slab in (0, -1):
        with pytest.raises(ValueError, match="slab"):
            _call(_Bare((4, 5, 6)), x, th, slab=slab)
    with pytest.raises(ValueError, match="thetas"):
        _call(_Bare((4, 5, 6)), x, torch.zeros(0))
    # 3 angles x W = 5 x T = 6: 90 elements, CUDA float32 -- a host tensor of any size is refused, with or without
    # a slab and a prior (a prior does not refuse a slab here)
    for t in (x, torch.zeros(90), torch.zeros(89, dtype=torch.float64)):
        for kw in ({}, dict(slab=7), dict(slab=7, lambda_tv=0.1), dict(slab=20, lambda_tv_t=0.1)):
            with pytest.raises(ValueError, match="sinogram must be a CUDA float32 tensor of 3 x 5 x 6 elements"):
                _call(_Bare((4, 5, 6)), t, th, **kw)
    # step_radon keeps its 2-D-only check
    from wire_amd.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr.__dict__.update(_Bare((4, 5, 6)).__dict__)
    with pytest.raises(ValueError, match="2-D grid and out_features == 1"):
        tr.step_radon(x, th)


def test_radon_volume_refusals_without_a_device():
    from wire_amd import _lib
    from wire_amd.modules import lin_inverse
    th = torch.zeros(3)
    for bad in (torch.zeros(4, 5), torch.zeros(1, 2, 4, 5), torch.zeros(4, 0, 5), np.zeros((4, 5, 6))):
        with pytest.raises(ValueError, match=r"\(H, W, T\)"):
            lin_inverse.radon_volume(bad, th)
    with pytest.raises(ValueError, match="angle"):
        lin_inverse.radon_volume(torch.zeros(4, 5, 6), torch.zeros(0))
    with pytest.raises(_lib.WireHipError, match="no CPU path"):
        lin_inverse.radon_volume(torch.zeros(4, 5, 6), th)
