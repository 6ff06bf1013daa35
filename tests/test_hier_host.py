"""bspline_mscale_hier on the host: construction, state_dict and head parity with the reference, what raises, the
library's size queries and descriptor checks for kind 9 (no GPU needed).  Fixtures: tests/golden/make_hier_golden.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import checksum, load_golden
import hier_ref as hr


def _build(rec, call="kw", st_type="list", hl=None):
    from wire_amd.modules import models
    torch.manual_seed(int(rec["meta_seed"]))
    D, hf, L, O = int(rec["meta_D"]), int(rec["meta_hidden_features"]), int(rec["meta_L"]), int(rec["meta_O"])
    L = L if hl is None else hl
    st = [float(v) for v in rec["meta_scale_tensor"]]
    st = torch.tensor(st) if st_type == "tensor" else st
    if call == "kw":
        return models.get_INR(nonlin="bspline_mscale_hier", in_features=D, out_features=O, hidden_features=hf,
                              scaled_hidden_features=0, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                              scale=0.0, scale_tensor=st, pos_encode=False, sidelength=512)
    return models.get_INR("bspline_mscale_hier", D, hf, 0, L, O, True, -0.2, -0.2, 0.0, st)


@pytest.mark.parametrize("call,st_type", [("kw", "list"), ("pos", "list"), ("kw", "tensor"), ("pos", "tensor")])
def test_state_dict_and_heads_match_reference_bit_for_bit(call, st_type):
    rec = load_golden("small_hier")
    model = _build(rec, call, st_type)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in rec["sd_keys"]]
    for k, v in sd.items():
        ref = rec["sd__" + k]
        assert v.dtype == torch.float32 and ref.dtype == np.float32, k
        assert np.array_equal(v.numpy(), ref), k
    assert [k for k, _ in model.named_parameters()] == [str(k) for k in rec["param_names"]]
    assert [p.requires_grad for _, p in model.named_parameters()] == list(rec["param_requires_grad"])
    assert all(not p.requires_grad for k, p in model.named_parameters() if k.endswith("scale_0"))
    from wire_amd.modules import utils
    assert utils.count_parameters(model) == int(rec["count_parameters"])
    # the heads: a plain list, the reference's bits, in neither state_dict() nor parameters()
    assert isinstance(model.linears, list) and len(model.linears) == 3
    for s, lin in enumerate(model.linears):
        assert np.array_equal(lin.weight.detach().numpy(), rec[f"head__linears.{s}.weight"])
        assert np.array_equal(lin.bias.detach().numpy(), rec[f"head__linears.{s}.bias"])
    assert not any("linears" in k for k in sd)
    ids = {id(p) for p in model.parameters()}
    assert not any(id(p) in ids for lin in model.linears for p in lin.parameters())
    # indexable as the drivers index them
    assert len(list(model.stages[1].parameters())) == 9 and len(list(model.linears[1].parameters())) == 2
    assert model.stages[1][1].linear.weight.shape == (32, 64) and model.stages[0][1].linear.weight.shape == (32, 32)
    d = model.net_desc()
    assert d.kind == 9 and d.width == 32 and d.hidden_layers == 2 and d.out_features == 3
    h = d._b_base_
    assert h.first_width == 0 and h.nscales == 3
    assert list(h.scales)[:3] == [np.float32(v) for v in rec["meta_scale_tensor"]]
    # params[]: the stages' used layers in state_dict order, then the heads
    pt = model.param_tensors()
    want = [p for k, p in model.named_parameters() if "scale_0" not in k] + \
           [p for lin in model.linears for p in (lin.weight, lin.bias)]
    assert len(pt) == len(want) and all(a is b for a, b in zip(pt, want))


@pytest.mark.parametrize("name", ["full_hier_st4", "full_hier_st4_3"])
def test_config_net_checksums(name):
    rec = load_golden(name)
    model = _build(rec)
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.numpy()), rec["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)
    for s, lin in enumerate(model.linears):
        np.testing.assert_allclose(checksum(lin.weight.detach().numpy()), rec[f"head0_checksum__linears.{s}.weight"],
                                   rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(checksum(lin.bias.detach().numpy()), rec[f"head0_checksum__linears.{s}.bias"],
                                   rtol=1e-12, atol=1e-12)


def test_fp64_oracle_reproduces_reference_gradients():
    rec = load_golden("small_hier")
    sd = {k[4:]: v for k, v in rec.items() if k.startswith("sd__")}
    hd = {k[6:]: v for k, v in rec.items() if k.startswith("head__")}
    st = rec["meta_scale_tensor"]
    x, t = rec["coords"], rec["target"]
    y, loss, g, gx = hr.loss_and_grads(sd, hd, int(rec["meta_L"]), x.astype(np.float64), t.astype(np.float64), st, np.float64)
    np.testing.assert_allclose(y, rec["y64"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(loss, float(rec["loss64"]), rtol=1e-10)
    assert sorted(g) == sorted(str(k) for k in rec["grad_keys64"])
    for k, v in g.items():
        np.testing.assert_allclose(v, rec["g64__" + k], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(gx, rec["gcoords64"], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("name,st", [("full_hier_st4", [1 / 9, 4.0]), ("full_hier_st4_3", [1 / 8, 1 / 2, 4.0])])
def test_fp64_oracle_on_the_config_nets(name, st):
    rec = load_golden(name)
    model = _build(rec)
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    hd = {f"linears.{s}.{q}": getattr(lin, q).detach().numpy() for s, lin in enumerate(model.linears)
          for q in ("weight", "bias")}
    x, t = rec["coords"], rec["target"]
    y, _, g, gx = hr.loss_and_grads(sd, hd, 2, x.astype(np.float64), t.astype(np.float64), rec["meta_scale_tensor"],
                                    np.float64)
    np.testing.assert_allclose(y, rec["y64"], rtol=1e-9, atol=1e-12)
    for k, v in g.items():
        np.testing.assert_allclose(checksum(v), rec["g64_checksum__" + k], rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(checksum(gx), rec["gcoords_checksum64"], rtol=1e-7, atol=1e-12)


@pytest.mark.parametrize("kw,why", [
    (dict(scale_tensor=[]), "needs 1..8 scales, got 0"),
    (dict(scale_tensor=torch.tensor([])), "needs 1..8 scales, got 0"),
    (dict(scale_tensor=[1.0] * 9), "needs 1..8 scales, got 9"),
    (dict(scale_tensor=[1.0, 0.0]), "zero or not finite"),
    (dict(scale_tensor=[1.0, float("nan")]), "zero or not finite"),
    (dict(scale_tensor=torch.tensor([float("inf"), 2.0])), "zero or not finite"),
    (dict(hidden_layers=0), "hidden_layers >= 1"),
    (dict(hidden_layers=1), "hidden_layers == 1 and more than one scale"),
])
def test_unsupported_configurations_raise(kw, why):
    from wire_amd.modules import models
    args = dict(hidden_layers=2, out_features=3, scale=0.0, scale_tensor=[1 / 9, 4.0])
    models.get_INR("bspline_mscale_hier", 2, 64, **args)          # the valid sibling builds
    args.update(kw)
    with pytest.raises(NotImplementedError, match=why.replace("..", r"\.\.")):
        models.get_INR("bspline_mscale_hier", 2, 64, **args)


def test_layer_raises_and_single_stage_builds():
    from wire_amd.modules import bspline_mscale_hier as mh, models
    with pytest.raises(NotImplementedError, match="trainable"):
        mh.Bsplines_form(2, 32, trainable=True)
    m = models.get_INR("bspline_mscale_hier", 2, 64, 0, 1, 3, scale=0.0, scale_tensor=[0.5])
    assert len(m.param_tensors()) == 2 * 2 + 2
    for name in ("mfn", "bspline_cubic"):
        with pytest.raises(NotImplementedError):
            models.get_INR(name, 2, 64, 0, 2, 3)


def test_three_hidden_layers_unused_layers():
    """L = 3: stages[s > 0][3] is in the state_dict (the reference builds it) and is not an ABI tensor."""
    rec = load_golden("small_hier")
    model = _build(rec, hl=3)
    sd = model.state_dict()
    assert "stages.1.3.linear.weight" in sd and "stages.2.3.linear.bias" in sd and "stages.0.3.linear.weight" in sd
    pt = {id(p) for p in model.param_tensors()}
    assert id(model.stages[0][3].linear.weight) in pt
    for s in (1, 2):
        assert id(model.stages[s][3].linear.weight) not in pt and id(model.stages[s][3].linear.bias) not in pt
    from wire_amd import _lib
    L = _lib.lib()
    assert L.wire_num_param_tensors(C.byref(model.net_desc())) == len(model.param_tensors()) == 2 * 4 + 6 * 2 + 2 * 3


def test_load_state_dict_reaches_the_descriptor():
    from wire_amd.modules import models
    a = models.get_INR("bspline_mscale_hier", 2, 32, 0, 2, 3, scale=0.0, scale_tensor=[0.25, 3.0])
    b = models.get_INR("bspline_mscale_hier", 2, 32, 0, 2, 3, scale=0.0, scale_tensor=[1 / 9, 4.0])
    b.load_state_dict(a.state_dict())
    assert list(b.net_desc()._b_base_.scales)[:2] == [0.25, 3.0]
    sd = a.state_dict()
    sd["stages.1.2.scale_0"] = sd["stages.1.2.scale_0"] * 2
    with pytest.raises(NotImplementedError, match="differ"):
        b.load_state_dict(sd)


def _desc(S=2, scales=None, K=256, hl=2, O=3, first_width=0):
    from wire_amd import _lib
    sc = list(scales if scales is not None else [1 / 9, 4.0, 8.0, 16.0, 2.0, 3.0, 5.0, 7.0][:S])[:8]
    return _lib.NetDescMS(_lib.make_desc("bspline_mscale_hier", 2, K, hl, O, -0.2, -0.2, 0.0), first_width, S,
                          (C.c_float * 8)(*(sc + [0.0] * (8 - len(sc)))))


@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("hl", [2, 4])
def test_size_queries_kind9(S, hl):
    from wire_amd import _lib
    L = _lib.lib()
    d = _desc(S=S, hl=hl)
    b = C.byref(d.base)
    nt = L.wire_num_param_tensors(b)
    assert nt == 2 * (hl + 1) + 6 * (S - 1) + 2 * S, L.wire_last_error()
    sizes = [L.wire_param_tensor_floats(b, i) for i in range(nt)]
    assert sizes == [256 * 2, 256] + [256 * 256, 256] * hl + \
        [256 * 2, 256, 256 * 512, 256, 256 * 256, 256] * (S - 1) + [3 * 256, 3] * S
    assert L.wire_param_tensor_floats(b, nt) < 0
    assert L.wire_packed_floats(b) > 0
    gemm_layers = hl + 3 * (S - 1)            # K -> K layers, a join counting twice for its width
    for n in (1, 1000, 65536):
        assert L.wire_act_bytes(b, n, 1) > n * 4 * 256 * 2 * gemm_layers
        assert L.wire_act_bytes(b, n, 0) >= n * 4 * 256 * (2 if S == 1 else 6)
        assert L.wire_act_bytes(b, n, 0) < L.wire_act_bytes(b, n, 1)
        assert L.wire_bwd_scratch_bytes(b, n) > 3 * n * 4 * 256
        assert L.wire_bwd_coords_scratch_bytes(b, n) >= L.wire_bwd_scratch_bytes(b, n) + S * n * 2 * 4


@pytest.mark.parametrize("S,scales,first_width,hl,O,ok", [
    (1, [2.0], 0, 1, 3, True), (1, [2.0], 0, 2, 3, True), (2, [1 / 9, 4.0], 0, 2, 3, True), (8, [1.0] * 8, 0, 2, 8, True),
    (3, [-1.0, 2.0, -3.0], 0, 3, 3, True),
    (0, [], 0, 2, 3, False), (9, [1.0] * 8, 0, 2, 3, False), (2, [1.0, 0.0], 0, 2, 3, False),
    (2, [1.0, float("inf")], 0, 2, 3, False), (2, [float("nan"), 1.0], 0, 2, 3, False), (2, [1 / 9, 4.0], 384, 2, 3, False),
    (2, [1 / 9, 4.0], 0, 1, 3, False), (1, [2.0], 0, 0, 3, False), (2, [1 / 9, 4.0], 0, 2, 9, False),
])
def test_descriptor_checks_kind9(S, scales, first_width, hl, O, ok):
    from wire_amd import _lib
    L = _lib.lib()
    d = _desc(S=S, scales=scales, first_width=first_width, hl=hl, O=O)
    rc = L.wire_num_param_tensors(C.byref(d.base))
    assert (rc > 0) == ok, (rc, L.wire_last_error())
    if not ok:
        assert rc == -1 and L.wire_last_error()          # WIRE_ERR_ARG with a message
        assert L.wire_packed_floats(C.byref(d.base)) == -1 and L.wire_act_bytes(C.byref(d.base), 100, 1) == -1


def test_abi_unchanged():
    from wire_amd import _lib
    L = _lib.lib()
    assert L.wire_abi_version() == 1 and _lib.ABI_VERSION == 1
    assert C.sizeof(_lib.NetDescMS) == 76
    assert _lib.KIND["bspline_mscale_hier"] == 9 and 7 not in _lib.KIND.values()
    bad = _lib.make_desc("bspline_form", 2, 256, 2, 3, -0.2, -0.2, 0.5)
    bad.kind = 7
    assert L.wire_num_param_tensors(C.byref(bad)) == -1
    bad.kind = 10
    assert L.wire_num_param_tensors(C.byref(bad)) == -1
    d = _lib.make_desc_hier(2, 256, 2, 3, -0.2, -0.2, 0.0, [1 / 9, 4.0])
    assert d.kind == 9 and d._b_base_.nscales == 2 and d._b_base_.first_width == 0
    assert L.wire_num_param_tensors(C.byref(d)) == 16
    with pytest.raises(ValueError):
        _lib.make_desc_hier(2, 256, 2, 3, -0.2, -0.2, 0.0, [])
