"""CPU-only half of the shape-envelope tests (tests/test_gpu_shape_envelope.py runs the kernels):

  * every numpy restatement the GPU module measures against, in fp64, against eager autograd of the same formula at the
    widths no other test reaches -- (D, O) = (1, 8), (4, 2), (4, 8) -- to 1e-10 relative, the figure
    tests/test_oracle_golden.py uses between fp64 twins;
  * the size queries of every case of the GPU module: positive, and monotone in the row count;
  * the limit of the final linear's forward kernel: it stages W_f [O][P] in the 64 KB of dynamic LDS a launch gets, so
    out_features x padded row width > 16384 is WIRE_ERR_ARG in make_plan (every kind) and in wire_final_fwd, before
    any HIP call.  The refused shapes are never launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import envelope_ref as er
from oracle import wire_oracle as wo

HOST_WIDTHS = [(1, 8), (4, 2), (4, 8)]
N = 96


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


# (the positional encoding at the two input widths the GPU module runs it at)
TWINS = [(net, D, O) for net in er.MAIN_NETS + ["bspline_mscale_2_s8"] for D, O in HOST_WIDTHS] + \
        [("relu_posenc", 1, 8), ("relu_posenc", 3, 8)]


@pytest.mark.parametrize("net,D,O", TWINS, ids=lambda v: str(v))
def test_restatement_equals_eager_autograd_fp64(net, D, O):
    model = er.build(net, D, O)
    sd = er.state(model)
    x, t = er.coords(N, D), er.targets(N, O)
    masks = er.relu_decisions(net, sd, x) if er.NETS[net]["kind"] == "relu" else None
    y, loss, g = er.np_step(net, sd, x, t, True, relu_masks=masks)
    t64 = torch.as_tensor(t, dtype=torch.float64)
    ye, _, ge = er.eager_grads(net, sd, x, True, lambda yy, rows: ((yy - t64[rows]) ** 2).sum() / t.size, masks, chunk=40)
    assert _rel(y, ye) <= 1e-10
    assert abs(loss - float(np.mean((ye - t) ** 2))) <= 1e-10 * loss
    assert sorted(g) == sorted(ge), (sorted(g), sorted(ge))
    for k in g:
        assert np.abs(ge[k]).max() > 0, f"{k}: the eager gradient is zero (a dead net compares nothing)"
        assert _rel(wo.as_real_pairs(g[k]), wo.as_real_pairs(ge[k])) <= 1e-10, k


def _cases():
    out = [(net, D, O) for net in er.MAIN_NETS for D, O in er.WIDTHS]
    return out + [("relu_posenc", 1, 8), ("relu_posenc", 3, 7), ("bspline_mscale_2_s8", 4, 8)]


@pytest.mark.parametrize("net,D,O", _cases(), ids=lambda v: str(v))
def test_size_queries_positive_and_monotone(net, D, O):
    from wire_amd import _lib
    lib = _lib.lib()
    d = er.build(net, D, O).net_desc()
    dp = C.byref(d)
    assert lib.wire_packed_floats(dp) > 0, lib.wire_last_error()
    queries = {"act1": lambda n: lib.wire_act_bytes(dp, n, 1), "act0": lambda n: lib.wire_act_bytes(dp, n, 0),
               "scratch": lambda n: lib.wire_bwd_scratch_bytes(dp, n),
               "coords_scratch": lambda n: lib.wire_bwd_coords_scratch_bytes(dp, n)}
    for name, q in queries.items():
        sizes = [q(n) for n in (1, 332, 333, 4096, 4133, 4134)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (name, sizes, lib.wire_last_error())
    # (include/wire_hip.h: the coordinate-gradient scratch is at least the plain backward's)
    assert lib.wire_bwd_coords_scratch_bytes(dp, 4133) >= lib.wire_bwd_scratch_bytes(dp, 4133)


def _queries(lib, d):
    dp = C.byref(d)
    return [lib.wire_packed_floats(dp), lib.wire_act_bytes(dp, 333, 1), lib.wire_act_bytes(dp, 333, 0),
            lib.wire_bwd_scratch_bytes(dp, 333), lib.wire_bwd_coords_scratch_bytes(dp, 333)]


def test_final_linear_lds_limit_wire():
    """hidden_features = 1500 -> K = 1060, P = 2176: 8 x 2176 = 17408 floats of W_f do not fit 64 KB; K = 1024 (P = 2048,
    hidden_features = 1449) is the widest 8-output wire net."""
    from wire_amd import _lib
    from wire_amd.modules import models
    lib = _lib.lib()
    wide = models.get_INR(nonlin="wire", in_features=2, out_features=8, hidden_features=1500, hidden_layers=1)
    assert wide._arch["width"] == 1060 and lib.wire_blocked_width(1060) == 2176
    for rc in _queries(lib, wide.net_desc()):
        assert rc == -1                                   # WIRE_ERR_ARG
        msg = lib.wire_last_error().decode()
        assert "out_features 8" in msg and "2176" in msg and "16384" in msg, msg
    ok = models.get_INR(nonlin="wire", in_features=2, out_features=8, hidden_features=1449, hidden_layers=1)
    assert ok._arch["width"] == 1024 and lib.wire_blocked_width(1024) == 2048
    assert all(rc > 0 for rc in _queries(lib, ok.net_desc())), lib.wire_last_error()
    # fewer outputs leave room for the wider net
    assert all(rc > 0 for rc in _queries(lib, _lib.make_desc("wire", 2, 1060, 1, 7, 20.0, 20.0, 30.0)))


@pytest.mark.parametrize("kind,k_ok,k_bad", [("mfn", 2048, 2049), ("siren", 2048, 2049), ("wire2d", 1024, 1025),
                                             ("bspline_form", 2048, 2049)])
def test_final_linear_lds_limit_every_kind(kind, k_ok, k_bad):
    from wire_amd import _lib
    lib = _lib.lib()
    assert all(rc > 0 for rc in _queries(lib, _lib.make_desc(kind, 2, k_ok, 1, 8, 30.0, 30.0, 10.0))), lib.wire_last_error()
    for rc in _queries(lib, _lib.make_desc(kind, 2, k_bad, 1, 8, 30.0, 30.0, 10.0)):
        assert rc == -1
        assert "out_features 8" in lib.wire_last_error().decode()
    assert all(rc > 0 for rc in _queries(lib, _lib.make_desc(kind, 2, k_bad, 1, 7, 30.0, 30.0, 10.0)))


def test_final_linear_lds_limit_scaled_kinds():
    from wire_amd import _lib
    lib = _lib.lib()
    for mk in (_lib.make_desc_m2, _lib.make_desc_hier):
        assert all(rc > 0 for rc in _queries(lib, mk(2, 2048, 2, 8, -0.2, -0.2, 0.0, [0.5, 2.0])))
        assert all(rc == -1 for rc in _queries(lib, mk(2, 2049, 2, 8, -0.2, -0.2, 0.0, [0.5, 2.0])))
    ms = lambda K: _lib.make_desc_ms(2, K, 2, 8, -0.2, -0.2, 1.0, 130, [1.0, 2.0])
    assert all(rc > 0 for rc in _queries(lib, ms(2048))[:4])
    assert all(rc == -1 for rc in _queries(lib, ms(2049)))


def test_wire_final_fwd_refuses_before_any_hip_call():
    """The per-layer entry point shares the kernel: the same refusal, decided from the shape alone (the pointers are never
    read: this runs without a GPU)."""
    from wire_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    assert lib.wire_final_fwd(None, p, p, p, 4, 1060, 8, p, p, 1 << 40) == -1
    msg = lib.wire_last_error().decode()
    assert "out_features 8" in msg and "2176" in msg and "16384" in msg, msg
    assert lib.wire_final_fwd(None, p, p, p, 4, 1025, 8, p, p, 1 << 40) == -1
    # an accepted shape gets past the check: it fails on the workspace size, still before anything is launched
    assert lib.wire_final_fwd(None, p, p, p, 4, 1024, 8, p, p, 0) == -3          # WIRE_ERR_SIZE
    assert lib.wire_final_fwd(None, p, p, p, 4, 1060, 7, p, p, 0) == -3
