"""The multiplicative filter network on the host: the closed form against the reference's fixtures, the module's init and
surface, the ABI's sizes.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mfn_ref as mr
from _util import GOLDEN, checksum


def _rel(a, b):
    return float(np.abs(np.asarray(a) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("D", [2, 3])
def test_closed_form_equals_reference_fp64(D):
    """Two fp64 evaluations of the same formula: 1e-10 relative, every output and every gradient."""
    rec = np.load(os.path.join(GOLDEN, "small_mfn.npz"))
    tag = f"d{D}"
    sd = {k[len(tag) + 5:]: rec[k] for k in rec.files if k.startswith(f"{tag}_sd__")}
    assert len(sd) == 18
    x, t = rec[f"{tag}_coords"], rec[f"{tag}_target"]
    y, loss, grads, gx = mr.loss_and_grads(sd, 2, x.astype(np.float64), t.astype(np.float64), np.float64, chunk=128)
    assert _rel(y, rec[f"{tag}_y64"]) <= 1e-10
    assert abs(loss - float(rec[f"{tag}_loss64"])) <= 1e-10 * float(rec[f"{tag}_loss64"])
    assert _rel(gx, rec[f"{tag}_gx64"]) <= 1e-10
    for k in sd:
        assert _rel(grads[k], rec[f"{tag}_g64__{k}"]) <= 1e-10, k
    fl, ln = mr.net_from_state(sd, 2)
    assert _rel(mr.forward(fl, ln, x, np.float64), rec[f"{tag}_y64"]) <= 1e-10
    # the fp32 evaluation is the reference's fp32 arithmetic up to the order of its sums
    assert _rel(mr.forward(fl, ln, x, np.float32), rec[f"{tag}_y64"]) <= 1e-4


def test_init_equals_reference_checksums():
    from wire_amd.modules import mfn
    rec = np.load(os.path.join(GOLDEN, "full_mfn_2x256.npz"))
    for seed in (0, 3):
        torch.manual_seed(seed)
        m = mfn.INR(2, 256, 2, 3)
        sd = m.state_dict()
        assert list(sd) == [str(k) for k in rec["names"]]
        assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in rec["shapes"]]
        for k, v in sd.items():
            assert np.array_equal(checksum(v.numpy()), rec[f"s{seed}__{k}"]), (seed, k)
    assert len(sd) == 18 and sum(p.numel() for p in m.parameters()) == int(rec["nparams"]) == 136963
    assert m.k == 3 and len(m.gabon_filters) == 3 and len(m.linear) == 3
    assert list(sd)[:4] == ["gabon_filters.0.mu", "gabon_filters.0.gamma", "gabon_filters.0.linear.weight",
                            "gabon_filters.0.linear.bias"]
    assert list(sd)[12:] == ["linear.0.weight", "linear.0.bias", "linear.1.weight", "linear.1.bias", "linear.2.weight",
                             "linear.2.bias"]


@pytest.mark.parametrize("D,K,L,O", [(2, 256, 2, 3), (3, 250, 0, 1), (4, 64, 4, 8)])
def test_param_tensors_follow_the_abi(D, K, L, O):
    from wire_amd import _lib
    from wire_amd.modules import mfn
    lib = _lib.lib()
    m = mfn.INR(D, K, L, O)
    d = m.net_desc()
    assert d.kind == _lib.KIND["mfn"] == 11
    tens = m.param_tensors()
    assert [id(t) for t in tens] == [id(v) for v in m.parameters()]       # = state_dict order
    assert lib.wire_num_param_tensors(C.byref(d)) == len(tens) == 4 * (L + 1) + 2 * L + 2
    for i, t in enumerate(tens):
        assert lib.wire_param_tensor_floats(C.byref(d), i) == t.numel(), i
    assert lib.wire_param_tensor_floats(C.byref(d), len(tens)) == -1


def test_size_queries():
    from wire_amd import _lib
    lib = _lib.lib()
    ok = _lib.make_desc("mfn", 2, 256, 2, 3, 0.0, 0.0, 0.0)                # a zero scale0 is accepted
    assert lib.wire_num_param_tensors(C.byref(ok)) == 18
    assert lib.wire_packed_floats(C.byref(ok)) > 0
    n = 65536
    a1, a0 = lib.wire_act_bytes(C.byref(ok), n, 1), lib.wire_act_bytes(C.byref(ok), n, 0)
    assert a1 >= (3 + 2) * n * 256 * 4 and 0 < a0 < a1                      # z_0 .. z_2, lin_0, lin_1
    sb = lib.wire_bwd_scratch_bytes(C.byref(ok), n)
    assert sb >= 3 * n * 256 * 4 and lib.wire_bwd_coords_scratch_bytes(C.byref(ok), n) >= sb
    assert [lib.wire_act_out_offset(C.byref(ok), n, l) for l in range(3)] == sorted(
        {lib.wire_act_out_offset(C.byref(ok), n, l) for l in range(3)})
    assert lib.wire_act_out_offset(C.byref(ok), n, 3) == -1
    # buffer sizes do not depend on the tuning knobs
    from _util import tune
    ref = (lib.wire_packed_floats(C.byref(ok)), a1, a0, sb)
    for knobs in ({"split_f16": 0}, {"split_bf16": 0}, {"fused_fwd": 0}, {"fused_train": 0}):
        with tune(**knobs):
            assert (lib.wire_packed_floats(C.byref(ok)), lib.wire_act_bytes(C.byref(ok), n, 1),
                    lib.wire_act_bytes(C.byref(ok), n, 0), lib.wire_bwd_scratch_bytes(C.byref(ok), n)) == ref
    zero_layers = _lib.make_desc("mfn", 2, 256, 0, 3, 0.0, 0.0, 1.0)
    assert lib.wire_num_param_tensors(C.byref(zero_layers)) == 6
    for bad in (dict(in_features=5), dict(out_features=9), dict(hidden_layers=-1), dict(width=0)):
        kw = dict(in_features=2, width=256, hidden_layers=2, out_features=3)
        kw.update(bad)
        d = _lib.make_desc("mfn", kw["in_features"], kw["width"], kw["hidden_layers"], kw["out_features"], 0.0, 0.0, 1.0)
        assert lib.wire_num_param_tensors(C.byref(d)) == -1 and lib.wire_last_error(), bad
        assert lib.wire_act_bytes(C.byref(d), 100, 1) == -1
    d7 = _lib.make_desc("mfn", 2, 256, 2, 3, 0.0, 0.0, 1.0)
    d7.kind = 7
    assert lib.wire_num_param_tensors(C.byref(d7)) == -1
    for name in ("wire_mfn_filter_fwd", "wire_mfn_filter_bwd", "wire_mfn_filter_ws_bytes"):
        assert name in _lib.SYMBOLS and getattr(lib, name)
    assert lib.wire_mfn_filter_ws_bytes(1000, 256) > 0


def test_factory_still_raises_and_names_the_constructor():
    from wire_amd.modules import models
    with pytest.raises(NotImplementedError, match=r"wire_amd\.modules\.mfn\.INR"):
        models.get_INR("mfn", 2, 64, 0, 2, 3)
    with pytest.raises(NotImplementedError, match="outside the MI355X hot path"):
        models.get_INR("bspline_cubic", 2, 64, 0, 2, 3)
    assert "mfn" not in models.model_dict


def test_input_shapes_and_no_cpu_fallback():
    from wire_amd import _lib
    from wire_amd.modules import mfn
    m = mfn.INR(2, 32, 1, 3)
    for shape in ((5, 2), (2, 5, 2), (1, 5, 3), (1, 1, 5, 2)):
        with pytest.raises(ValueError):
            m(torch.zeros(shape))
    with pytest.raises(_lib.WireHipError):
        m(torch.zeros(1, 5, 2))
    with pytest.raises(_lib.WireHipError):
        m.gabon_filters[0](torch.zeros(5, 2))
    with pytest.raises(ValueError):
        m.gabon_filters[0](torch.zeros(1, 5, 2))
    assert mfn.INR(2, 32, 0, 1).k == 1


def test_fused_trainer_accepts_a_model_without_net():
    """FusedTrainer's constructor reaches its device check for an mfn (which has no ``net``)."""
    from wire_amd import _lib
    from wire_amd.modules import mfn
    from wire_amd.trainer import FusedTrainer
    with pytest.raises(_lib.WireHipError, match="MI355X"):
        FusedTrainer(mfn.INR(2, 32, 1, 3), (8, 8), torch.zeros(64, 3))
