"""CPU-only checks of the learnable registration: the three entry points' declarations, their refusal of bad arguments
(before any HIP call, so on a machine without a GPU), the restatement of tests/frame_warp_ref.py against torch autograd
in fp64 and against motion.get_transformed_coords, and the Python layer's refusals that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from _util import ROOT
import frame_warp_ref as ref

NAMES = ["wire_warp_coords_fwd", "wire_warp_coords_bwd_ws_bytes", "wire_warp_coords_bwd"]


def test_header_declares_the_entry_points_and_lib_lists_them():
    from wire_amd import _lib
    text = open(os.path.join(ROOT, "include", "wire_hip.h")).read()
    want = {"wire_warp_coords_fwd": ("int", ["stream", "coords", "theta", "B", "n_per", "out"]),
            "wire_warp_coords_bwd_ws_bytes": ("int64_t", ["B", "n_per"]),
            "wire_warp_coords_bwd": ("int", ["stream", "coords", "theta", "g_out", "B", "n_per", "pin_first", "g_theta",
                                             "g_in", "ws", "ws_bytes"])}
    L = _lib.lib()
    for name, (ret, params) in want.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), text)
        assert m, f"include/wire_hip.h does not declare {ret} {name}"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == params
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(params)
    assert L.wire_warp_coords_bwd_ws_bytes.restype is C.c_int64
    assert L.wire_abi_version() == 1 and _lib.ABI_VERSION == 1


def test_entry_points_refuse_bad_arguments():
    """B or n_per < 1, sizes beyond 63 bits, more workgroups than a grid holds, pin_first not 0 / 1 and a NULL pointer
    other than g_in return WIRE_ERR_ARG (-1) and name the entry point; a ws that is too small WIRE_ERR_SIZE (-3).  NULL
    stream, host buffers: nothing reaches HIP."""
    from wire_amd import _lib
    L = _lib.lib()
    buf = (C.c_double * 4096)()
    p = C.addressof(buf)
    big = (1 << 31) - 1
    sizes = (dict(B=0), dict(B=-1), dict(n=0), dict(n=-5),
             dict(B=big, n=1 << 62), dict(B=1, n=1 << 60),      # B * n_per, and its bytes, beyond 63 bits
             dict(B=big, n=1 << 20))                               # 2^51 rows fit; their workgroups do not

    def fwd(c=p, t=p, B=3, n=100, out=p):
        return L.wire_warp_coords_fwd(None, c, t, B, n, out)

    def bwd(c=p, t=p, g=p, B=3, n=100, pin=1, gt=p, gi=p, ws=p, wb=4096 * 8):
        return L.wire_warp_coords_bwd(None, c, t, g, B, n, pin, gt, gi, ws, wb)

    for kw in sizes + (dict(B=1, n=1 << 40), dict(c=None), dict(t=None), dict(out=None)):
        assert fwd(**kw) == -1, kw
        assert b"wire_warp_coords_fwd" in L.wire_last_error()
    for kw in sizes + (dict(B=8, n=1 << 40), dict(pin=2), dict(pin=-1), dict(c=None), dict(t=None), dict(g=None),
                       dict(gt=None), dict(ws=None)):
        assert bwd(**kw) == -1, kw
        assert b"wire_warp_coords_bwd" in L.wire_last_error()
    for kw in sizes:
        assert L.wire_warp_coords_bwd_ws_bytes(kw.get("B", 3), kw.get("n", 100)) == -1, kw
        assert b"wire_warp_coords_bwd_ws_bytes" in L.wire_last_error()
    need = L.wire_warp_coords_bwd_ws_bytes(3, 100)
    for wb in (need - 1, 0, -1):
        assert bwd(wb=wb) == -3, wb
        assert b"wire_warp_coords_bwd" in L.wire_last_error()


def test_ws_bytes_positive_and_monotone():
    from wire_amd import _lib
    L = _lib.lib()
    ns = [1, 63, 256, 546, 2048, 2049, 90000, 393216, 1 << 24]
    prev_row = None
    for B in (1, 2, 3, 4, 17):
        row = [L.wire_warp_coords_bwd_ws_bytes(B, n) for n in ns]
        assert all(v > 0 for v in row) and all(a <= b for a, b in zip(row, row[1:]))
        if prev_row is not None:
            assert all(a <= b for a, b in zip(prev_row, row))
        prev_row = row
    # six fp64 partials per workgroup, at least one workgroup per frame
    assert L.wire_warp_coords_bwd_ws_bytes(3, 546) >= 3 * 48


def _inputs(rng, B, n):
    coords = rng.uniform(-1.2, 1.2, (B, n, 2)).astype(np.float32)
    theta = rng.uniform(-1, 1, (B, 2, 3)).astype(np.float32)
    theta[0] = [[1, 0, 0], [0, 1, 0]]
    g = (1e-3 * rng.standard_normal((B, n, 2))).astype(np.float32)
    return coords, theta, g


def test_restatement_backward_is_autograd_of_the_einsum():
    """S and g_in against torch autograd of einsum(theta, [coords, 1]) in fp64: 1e-12 relative (S), and g_in -- which the
    restatement rounds to fp32 -- within half an fp32 ulp.  pin_first zeroes frame 0 and nothing else; identity theta
    returns the coordinates' bits."""
    rng = np.random.default_rng(3)
    B, n = 3, 211
    coords, theta, g = _inputs(rng, B, n)
    g[1] = 0.0
    c = torch.tensor(coords, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    v = torch.cat([c, torch.ones(B, n, 1, dtype=torch.float64)], dim=-1)
    out = torch.einsum("fak,fpk->fpa", t, v)
    (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    S, A, g_in = ref.warp_bwd(coords, theta, g, 0)
    want = t.grad.numpy()
    assert np.abs(S - want).max() <= 1e-12 * np.abs(want).max()
    assert (A >= np.abs(S)).all() and not S[1].any() and not A[1].any()
    gi = c.grad.numpy()
    assert g_in.dtype == np.float32
    assert (np.abs(g_in.astype(np.float64) - gi) <= 0.5 * np.spacing(np.abs(gi).astype(np.float32)) + 1e-45).all()
    Sp, Ap, gp = ref.warp_bwd(coords, theta, g, 1)
    assert not Sp[0].any() and np.array_equal(Sp[1:], S[1:]) and np.array_equal(Ap, A) and np.array_equal(gp, g_in)
    w = ref.warp(coords, theta)
    assert w.dtype == np.float32 and w[0].tobytes() == coords[0].tobytes()
    assert np.abs(w.astype(np.float64) - out.detach().numpy()).max() <= 2.0 ** -24 * np.abs(out.detach().numpy()).max()


def test_restatement_forward_is_get_transformed_coords():
    """warp of the align_corners=False base grid against motion.get_transformed_coords(theta, (5, 7)), random theta:
    per component within 3 * 2^-24 * (|t_a0| + |t_a1| + |t_a2|), the error bound of affine_grid's three-term fp32 dot
    product (the base grid's entries are at most 1 in size)."""
    from wire_amd.modules import motion
    rng = np.random.default_rng(4)
    H, W, B = 5, 7, 6
    theta = rng.uniform(-1.5, 1.5, (B, 2, 3)).astype(np.float32)
    theta[0] = [[1, 0, 0], [0, 1, 0]]
    got = ref.warp(np.broadcast_to(ref.base_grid(H, W), (B, H * W, 2)), theta).astype(np.float64)
    want = motion.get_transformed_coords(torch.tensor(theta), (H, W)).numpy().astype(np.float64)
    assert want.shape == (B, H * W, 2)
    bound = 3 * 2.0 ** -24 * np.abs(theta.astype(np.float64)).sum(axis=2)            # [B, 2]
    err = np.abs(got - want)
    print(f"warp vs get_transformed_coords: worst err / bound {(err / bound[:, None, :]).max():.3f}")
    assert (err <= bound[:, None, :]).all()


class _Bare:
    """The attributes the step reads before it touches the device."""

    def __init__(self, grid, world=1, O=3):
        self.grid, self.world, self.O = grid, world, O
        self.tz = object() if len(grid) == 3 else None
        self.dev = torch.device("cpu")


def _call(name, bare, *a, **kw):
    from wire_amd.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr.__dict__.update(bare.__dict__)
    return getattr(tr, name)(*a, **kw)


def test_python_layer_exists_and_refuses_without_a_device():
    from wire_amd import _lib, functional
    from wire_amd.trainer import FrameRegistration, FusedTrainer
    sig = inspect.signature(FusedTrainer.step_frames_registered)
    assert list(sig.parameters) == ["self", "reg", "coords", "gt_lr", "scale", "mask", "rec_lr"]
    assert sig.parameters["mask"].default is None and sig.parameters["rec_lr"].default is None
    sig = inspect.signature(FusedTrainer.registration)
    assert list(sig.parameters) == ["self", "B", "lr", "pin_first", "theta"]
    assert sig.parameters["lr"].default == 1e-4 and sig.parameters["pin_first"].default is True \
        and sig.parameters["theta"].default is None
    # no CPU fallback: host tensors are refused the way the siblings refuse them
    c, t = torch.zeros(2, 35, 2), torch.zeros(2, 2, 3)
    with pytest.raises(_lib.WireHipError):
        functional.warp_coords(c, t)
    with pytest.raises(_lib.WireHipError):
        FrameRegistration(2, "cpu")
    with pytest.raises(ValueError, match="coords must be"):
        _call("step_frames_registered", _Bare((5, 7)), None, c, torch.zeros(2, 2, 3), 2)
    with pytest.raises(ValueError, match="2-D grid"):
        _call("step_frames_registered", _Bare((5, 7, 3)), None, c, c, 2)
    with pytest.raises(ValueError, match="2-D grid"):
        _call("registration", _Bare((5, 7, 3)), 2)
    with pytest.raises(NotImplementedError, match="single-process"):
        _call("step_frames_registered", _Bare((5, 7), world=2), None, c, c, 2)
    with pytest.raises(ValueError, match="scale"):
        _call("step_frames_registered", _Bare((5, 7)), None, c, c, 0)
    with pytest.raises(_lib.WireHipError):
        _call("registration", _Bare((5, 7)), 2)
    from wire_amd.modules import motion
    assert "step_frames_registered" in motion.__doc__ and "warp_coords" in motion.__doc__


def test_step_frames_signature_is_unchanged():
    from wire_amd.trainer import FusedTrainer
    sig = inspect.signature(FusedTrainer.step_frames)
    E = inspect.Parameter.empty
    assert [(p.name, str(p.annotation), p.default) for p in sig.parameters.values()] == [
        ("self", str(E), E), ("coords", "torch.Tensor", E), ("gt_lr", "torch.Tensor", E), ("scale", "int", E),
        ("mask", "Optional[torch.Tensor]", None), ("rec_lr", "Optional[torch.Tensor]", None)]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert sig.return_annotation == "torch.Tensor"
    assert "canonical grid" in FusedTrainer.step_frames.__doc__
