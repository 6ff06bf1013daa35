"""bspline_mscale_HL on the host: construction, state_dict parity with the reference, the first stage's column groups,
what raises, the library's size queries and descriptor checks for kind 6 (no GPU needed).
Fixtures: tests/golden/make_mscale_hl_golden.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import checksum, load_golden
import mscale_ref as mr


def _build(rec, call="kw", st_type="tensor"):
    from wire_amd.modules import models
    torch.manual_seed(int(rec["meta_seed"]))
    D, hf, shf, L, O, s = (int(rec["meta_D"]), int(rec["meta_hidden_features"]), int(rec["meta_shf"]),
                           int(rec["meta_L"]), int(rec["meta_O"]), float(rec["meta_scale0"]))
    st = [float(v) for v in rec["meta_scale_tensor"]]
    st = torch.tensor(st) if st_type == "tensor" else st
    if call == "kw":      # bspline_img_representation.py:98-111
        return models.get_INR(nonlin="bspline_mscale_HL", in_features=D, out_features=O, hidden_features=hf,
                              scaled_hidden_features=shf, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                              scale=s, scale_tensor=st, pos_encode=False, sidelength=512)
    return models.get_INR("bspline_mscale_HL", D, hf, shf, L, O, True, -0.2, -0.2, s, st)   # positional


@pytest.mark.parametrize("call,st_type", [("kw", "tensor"), ("pos", "tensor"), ("kw", "list")])
def test_state_dict_matches_reference_bit_for_bit(call, st_type):
    rec = load_golden("small_mscale_hl")
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
    assert model.net[0].scale_0.shape == (3,) and model.net[1].scale_0.shape == (1,)
    d = model.net_desc()
    assert d.kind == 6 and d.width == 32 and d.hidden_layers == 2 and d.scale0 == np.float32(0.25)
    ms = d._b_base_
    assert ms.first_width == 320 and ms.nscales == 3
    assert list(ms.scales)[:3] == [np.float32(v) for v in rec["meta_scale_tensor"]]


def test_config_net_state_dict_checksums():
    rec = load_golden("full_mscale_hl_384")
    model = _build(rec)
    keys = list(model.state_dict().keys())
    assert keys[:3] == ["net.0.scale_0", "net.0.linear.weight", "net.0.linear.bias"] and keys[-1] == "net.3.bias"
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.numpy()), rec["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shf", [130, 256, 300, 384, 450, 512])
@pytest.mark.parametrize("T", [2, 3])
def test_column_groups_match_reference_slicing(shf, T):
    from wire_amd.modules.bspline_mscale_HL import column_groups
    ref = load_golden("small_mscale_hl")[f"colmap__{shf}_{T}"]
    if shf > 256 and (shf - 256) % (T - 1):
        with pytest.raises(NotImplementedError):
            column_groups(shf, T)
        return
    assert np.array_equal(np.array(column_groups(shf, T)), ref)
    assert np.array_equal(mr.column_groups(shf, T), ref)


def test_fp64_oracle_reproduces_reference_gradients():
    rec = load_golden("small_mscale_hl")
    sd = {k[4:]: v for k, v in rec.items() if k.startswith("sd__")}
    st = rec["meta_scale_tensor"]
    x, t = rec["coords"], rec["target"]
    y, _, g = mr.loss_and_grads(sd, int(rec["meta_L"]), x.astype(np.float64), t.astype(np.float64), st,
                                float(rec["meta_scale0"]), np.float64)
    np.testing.assert_allclose(y, rec["y64"], rtol=1e-10, atol=1e-12)
    assert sorted(g) == sorted(str(k) for k in rec["grad_keys64"])
    for k, v in g.items():
        np.testing.assert_allclose(v, rec["g64__" + k], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("kw", [
    dict(scaled_hidden_features=0, scale_tensor=[]),             # the existing out-of-scope call: T = 0
    dict(scale_tensor=[2.0]),                                     # T < 2: the reference divides by T - 1
    dict(scale_tensor=torch.tensor([2.0])),
    dict(scaled_hidden_features=0),                               # SHF < 1
    dict(scaled_hidden_features=385),                             # 256 + 2 groups != 385
    dict(scaled_hidden_features=300, scale_tensor=[1.0, 2.0, 3.0, 4.0]),
    dict(scale_tensor=[1.0, 0.0, 2.0]),                           # a zero scale
    dict(scale_tensor=[1.0, float("nan"), 2.0]),
    dict(scale_tensor=[float("inf"), 1.0, 2.0]),
    dict(scale=0.0),                                              # zero hidden scale
    dict(outermost_linear=False),
])
def test_unsupported_configurations_raise(kw):
    from wire_amd.modules import models
    args = dict(scaled_hidden_features=384, hidden_layers=2, out_features=3, scale=0.5, scale_tensor=[1.0, 2.0, 3.0])
    args.update(kw)
    with pytest.raises(NotImplementedError):
        models.get_INR("bspline_mscale_HL", 2, 256, **args)
    from wire_amd.modules.bspline_mscale_HL import Scaled_Bsplines_form
    with pytest.raises(NotImplementedError):
        Scaled_Bsplines_form(2, 384, sigma0=torch.tensor([1.0, 2.0, 3.0]), trainable=True)


@pytest.mark.parametrize("hl", [0, 1, 2, 3])
def test_hidden_layers_zero_builds_the_net_of_one(hl):
    from wire_amd.modules import models
    m = models.get_INR("bspline_mscale_HL", 2, 64, 300, hl, 3, scale=0.5, scale_tensor=[1.0, 2.0, 3.0])
    assert len(m.net) == 3 + max(hl - 1, 0)
    assert len(m.param_tensors()) == 2 * (2 + max(hl - 1, 0)) + 2


def _desc(shf=384, T=3, scales=(1 / 9, 1 / 9, 4.0), K=256, hl=2, s=1 / 9):
    from wire_amd import _lib
    d = _lib.make_desc_ms(2, K, hl, 3, -0.2, -0.2, s, shf, list(scales) + [1.0] * (T - len(scales)))
    d._b_base_.nscales = T
    return d


def test_size_queries_kind6():
    from wire_amd import _lib
    L = _lib.lib()
    for hl in (0, 1, 2, 3):
        d = _desc(hl=hl)
        nl = 1 + max(hl - 1, 0)
        nt = L.wire_num_param_tensors(C.byref(d))
        assert nt == 2 + 2 * nl + 2
        sizes = [L.wire_param_tensor_floats(C.byref(d), i) for i in range(nt)]
        assert sizes == [384 * 2, 384, 256 * 384, 256] + [256 * 256, 256] * (nl - 1) + [3 * 256, 3]
        assert L.wire_param_tensor_floats(C.byref(d), nt) < 0
        assert L.wire_packed_floats(C.byref(d)) > 0
        for n in (1, 1000, 65536):
            assert L.wire_act_bytes(C.byref(d), n, 1) > n * 4 * 384
            assert L.wire_bwd_scratch_bytes(C.byref(d), n) > 0
    # the same sizes through a model
    from wire_amd.modules import models
    m = models.get_INR("bspline_mscale_HL", 2, 256, 384, 2, 3, scale=1 / 9, scale_tensor=[1 / 9, 1 / 9, 4.0])
    assert [t.numel() for t in m.param_tensors()] == [L.wire_param_tensor_floats(C.byref(m.net_desc()), i)
                                                      for i in range(len(m.param_tensors()))]


@pytest.mark.parametrize("shf,T,scales,ok", [
    (384, 3, (1.0, 2.0, 3.0), True), (450, 2, (1.0, 2.0), True), (130, 3, (1.0, 2.0, 3.0), True),
    (256, 2, (1.0, 2.0), True), (4096, 8, (1.0,) * 8, False), (4096, 6, (1.0,) * 6, True),
    (385, 3, (1.0, 2.0, 3.0), False), (384, 1, (1.0,), False), (384, 9, (1.0,) * 9, False), (0, 2, (1.0, 2.0), False),
    (4097, 2, (1.0, 2.0), False), (384, 3, (1.0, 0.0, 3.0), False), (384, 3, (1.0, float("inf"), 3.0), False),
    (384, 3, (-1.0, 2.0, -3.0), True),
])
def test_descriptor_checks_kind6(shf, T, scales, ok):
    from wire_amd import _lib
    L = _lib.lib()
    sc = list(scales)[:8]
    d = _lib.NetDescMS(_lib.make_desc("bspline_mscale_HL", 2, 256, 2, 3, -0.2, -0.2, 0.5), shf, T,
                       (C.c_float * 8)(*(sc + [0.0] * (8 - len(sc)))))
    rc = L.wire_num_param_tensors(C.byref(d.base))
    assert (rc > 0) == ok, (rc, L.wire_last_error())
    if not ok:
        assert rc == -1


def test_abi_unchanged_for_other_kinds():
    from wire_amd import _lib
    L = _lib.lib()
    assert L.wire_abi_version() == 1 and _lib.ABI_VERSION == 1
    assert C.sizeof(_lib.NetDesc) == 36 and C.sizeof(_lib.NetDescMS) == 36 + 8 + 32
    assert _lib.KIND["bspline_mscale_HL"] == 6
    # kind 7 is unknown; kind 6 with a zero hidden scale is refused
    bad = _lib.make_desc("bspline_form", 2, 256, 2, 3, -0.2, -0.2, 0.5)
    bad.kind = 7
    assert L.wire_num_param_tensors(C.byref(bad)) == -1
    assert L.wire_num_param_tensors(C.byref(_desc(s=0.0))) == -1
