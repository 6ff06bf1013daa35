"""bspline_mscale_2 on the host: construction, state_dict parity with the reference, what raises, the library's size
queries and descriptor checks for kind 8 (no GPU needed).  Fixtures: tests/golden/make_mscale2_golden.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import checksum, load_golden
import mscale2_ref as mr


def _build(rec, call="kw", st_type="tensor"):
    from wire_amd.modules import models
    torch.manual_seed(int(rec["meta_seed"]))
    D, hf, L, O, s = (int(rec["meta_D"]), int(rec["meta_hidden_features"]), int(rec["meta_L"]), int(rec["meta_O"]),
                      float(rec["meta_scale0"]))
    st = [float(v) for v in rec["meta_scale_tensor"]]
    st = torch.tensor(st) if st_type == "tensor" else st
    if call == "kw":      # bspline_SISR.py
        return models.get_INR(nonlin="bspline_mscale_2", in_features=D, out_features=O, hidden_features=hf,
                              scaled_hidden_features=0, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                              scale=s, scale_tensor=st, pos_encode=False, sidelength=512)
    return models.get_INR("bspline_mscale_2", D, hf, 0, L, O, True, -0.2, -0.2, s, st)   # positional


@pytest.mark.parametrize("call,st_type", [("kw", "tensor"), ("pos", "tensor"), ("kw", "list"), ("pos", "list")])
def test_state_dict_matches_reference_bit_for_bit(call, st_type):
    rec = load_golden("small_mscale2")
    model = _build(rec, call, st_type)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in rec["sd_keys"]]
    for k, v in sd.items():
        ref = rec["sd__" + k]
        assert v.dtype == torch.float32 and ref.dtype == np.float32, k
        assert np.array_equal(v.numpy(), ref), k
    assert [k for k, _ in model.named_parameters()] == [str(k) for k in rec["param_names"]]
    assert [p.requires_grad for _, p in model.named_parameters()] == list(rec["param_requires_grad"])
    from wire_amd.modules import utils
    assert utils.count_parameters(model) == int(rec["count_parameters"])
    assert model.scale0 == 0.0
    d = model.net_desc()
    assert d.kind == 8 and d.width == 32 and d.hidden_layers == 2 and d.out_features == 3
    m2 = d._b_base_
    assert m2.first_width == 0 and m2.nscales == 3
    assert list(m2.scales)[:3] == [np.float32(v) for v in rec["meta_scale_tensor"]]
    # params[]: freq_mlp's four tensors, then the trunk in kind 5's order
    ptrs = [t.data_ptr() for t in model.param_tensors()]
    names = {p.data_ptr(): k for k, p in model.named_parameters()}
    assert [names[q] for q in ptrs] == list(mr.COMB) + [k for k in sd if k.startswith("net.")]


def test_config_net_state_dict_checksums():
    rec = load_golden("full_mscale2_st4")
    model = _build(rec)
    keys = list(model.state_dict().keys())
    assert keys[0] == "combine_scales.scale_weights" and keys[-1] == "net.3.bias"
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.numpy()), rec["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)


def test_fp64_oracle_reproduces_reference_gradients():
    rec = load_golden("small_mscale2")
    sd = {k[4:]: v for k, v in rec.items() if k.startswith("sd__")}
    st = rec["meta_scale_tensor"]
    x, t = rec["coords"], rec["target"]
    y, _, g, gx = mr.loss_and_grads(sd, int(rec["meta_L"]), x, t.astype(np.float64), st, np.float64)
    np.testing.assert_allclose(y, rec["y64"], rtol=1e-10, atol=1e-12)
    assert sorted(g) == sorted(str(k) for k in rec["grad_keys64"])
    for k, v in g.items():
        np.testing.assert_allclose(v, rec["g64__" + k], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(gx, rec["gcoords64"], rtol=1e-8, atol=1e-12)
    # the parameters the reference's loop never updates get no gradient there either
    assert not any(k.startswith(("combine_scales.scale_weights", "combine_scales.refine")) for k in g)


@pytest.mark.parametrize("kw,why", [
    (dict(scale_tensor=[]), "needs 1..8 scales, got 0"),          # the default: S = 0
    (dict(scale_tensor=torch.tensor([])), "needs 1..8 scales, got 0"),
    (dict(scale_tensor=[1.0] * 9), "needs 1..8 scales, got 9"),   # S > 8
    (dict(scale_tensor=[1.0, 0.0]), "zero or not finite"),        # a zero scale
    (dict(scale_tensor=[1.0, float("nan")]), "zero or not finite"),
    (dict(scale_tensor=torch.tensor([float("inf"), 2.0])), "zero or not finite"),
    (dict(outermost_linear=False), "outermost_linear=False"),
])
def test_unsupported_configurations_raise(kw, why):
    from wire_amd.modules import models
    args = dict(hidden_layers=2, out_features=3, scale=0.0, scale_tensor=[1 / 9, 4.0])
    models.get_INR("bspline_mscale_2", 2, 256, **args)            # the valid sibling builds
    args.update(kw)
    with pytest.raises(NotImplementedError, match=why.replace("..", r"\.\.")):
        models.get_INR("bspline_mscale_2", 2, 256, **args)


def test_layer_and_combiner_raise():
    from wire_amd.modules import bspline_mscale_2 as m2
    with pytest.raises(NotImplementedError):
        m2.Bsplines_form(2, 32, trainable=True)
    comb = m2.AdaptiveScaleCombiner(2, 3, 512, 'both')
    outs = [torch.zeros(4, 3), torch.zeros(4, 3)]
    for mode in ("scale_weights", "both"):
        with pytest.raises(NotImplementedError):
            comb(outs, mode)


@pytest.mark.parametrize("st", [[1.0], [1 / 9, 2.0], [1 / 9, 4.0, 8.0], [1.0] * 8])
def test_scale_zero_builds(st):
    from wire_amd.modules import models
    m = models.get_INR("bspline_mscale_2", 2, 64, 0, 2, 3, True, -0.2, -0.2, 0.0, st)
    assert m.net_desc()._b_base_.nscales == len(st)


def _desc(S=2, scales=None, K=256, hl=2, O=3, first_width=0, s=0.0):
    from wire_amd import _lib
    sc = list(scales if scales is not None else [1 / 9, 4.0, 8.0, 16.0, 2.0, 3.0, 5.0, 7.0][:S])[:8]
    return _lib.NetDescMS(_lib.make_desc("bspline_mscale_2", 2, K, hl, O, -0.2, -0.2, s), first_width, S,
                          (C.c_float * 8)(*(sc + [0.0] * (8 - len(sc)))))


@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("hl", [0, 2])
def test_size_queries_kind8(S, hl):
    from wire_amd import _lib
    L = _lib.lib()
    d = _desc(S=S, hl=hl)
    b = C.byref(d.base)
    nt = L.wire_num_param_tensors(b)
    assert nt == 4 + 2 * (hl + 1) + 2, L.wire_last_error()
    sizes = [L.wire_param_tensor_floats(b, i) for i in range(nt)]
    assert sizes == [128 * S * 3, 128, 3 * 128, 3, 256 * 2, 256] + [256 * 256, 256] * hl + [3 * 256, 3]
    assert L.wire_param_tensor_floats(b, nt) < 0
    assert L.wire_packed_floats(b) > 0
    for n in (1, 1000, 65536):
        # the trunk's buffers hold S passes of n rows
        assert L.wire_act_bytes(b, n, 1) > S * n * 4 * 256 * (hl + 1)
        assert L.wire_act_bytes(b, n, 0) > 2 * S * n * 4 * 256
        assert L.wire_bwd_scratch_bytes(b, n) > 2 * S * n * 4 * 256
        assert L.wire_bwd_coords_scratch_bytes(b, n) > L.wire_bwd_scratch_bytes(b, n)
    from wire_amd.modules import models
    m = models.get_INR("bspline_mscale_2", 2, 256, 0, hl, 3, scale=0.0, scale_tensor=list(d.scales)[:S])
    md = m.net_desc()
    assert [t.numel() for t in m.param_tensors()] == [L.wire_param_tensor_floats(C.byref(md), i)
                                                      for i in range(len(m.param_tensors()))]


@pytest.mark.parametrize("S,scales,first_width,ok", [
    (1, [2.0], 0, True), (2, [1 / 9, 4.0], 0, True), (8, [1.0] * 8, 0, True), (3, [-1.0, 2.0, -3.0], 0, True),
    (0, [], 0, False), (9, [1.0] * 8, 0, False), (2, [1.0, 0.0], 0, False), (2, [1.0, float("inf")], 0, False),
    (2, [float("nan"), 1.0], 0, False), (2, [1 / 9, 4.0], 384, False), (2, [1 / 9, 4.0], -1, False),
])
def test_descriptor_checks_kind8(S, scales, first_width, ok):
    from wire_amd import _lib
    L = _lib.lib()
    d = _desc(S=S, scales=scales, first_width=first_width)
    rc = L.wire_num_param_tensors(C.byref(d.base))
    assert (rc > 0) == ok, (rc, L.wire_last_error())
    if not ok:
        assert rc == -1          # WIRE_ERR_ARG


def test_abi_unchanged():
    from wire_amd import _lib
    L = _lib.lib()
    assert L.wire_abi_version() == 1 and _lib.ABI_VERSION == 1
    assert C.sizeof(_lib.NetDescMS) == 76
    assert _lib.KIND["bspline_mscale_2"] == 8
    bad = _lib.make_desc("bspline_form", 2, 256, 2, 3, -0.2, -0.2, 0.5)
    bad.kind = 7
    assert L.wire_num_param_tensors(C.byref(bad)) == -1
    d = _lib.make_desc_m2(2, 256, 2, 3, -0.2, -0.2, 0.0, [1 / 9, 4.0])
    assert d.kind == 8 and d._b_base_.nscales == 2 and d._b_base_.first_width == 0
    assert L.wire_num_param_tensors(C.byref(d)) == 12
    with pytest.raises(ValueError):
        _lib.make_desc_m2(2, 256, 2, 3, -0.2, -0.2, 0.0, [])
