"""bspline_cubic on the host: the oracle against the reference's recorded runs, state_dict parity with the reference, the
descriptor and the library's size queries, the error paths (no GPU needed).  Fixtures:
tests/golden/make_bspline_cubic_golden.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import checksum, load_golden
import bspline_cubic_ref as bc


def _build(rec, scale=None):
    from wire_amd.modules import bspline_cubic
    torch.manual_seed(int(rec["meta_seed"]))
    D, hf, L, O = int(rec["meta_D"]), int(rec["meta_hidden_features"]), int(rec["meta_L"]), int(rec["meta_O"])
    s = float(rec["meta_scale0"]) if scale is None else scale
    # the reference's own positional order: hidden_layers BEFORE scaled_hidden_features (modules/bspline_cubic.py:56-70)
    return bspline_cubic.INR(D, hf, L, 0, O, True, -0.2, -0.2, s)


# ---- the oracle against the reference ---------------------------------------------------------------------------------
def test_oracle_reproduces_the_fixture():
    rec = load_golden("small_bspline_cubic")
    sd = {str(k): rec["sd__" + str(k)] for k in rec["sd_keys"]}
    L, s = int(rec["meta_L"]), float(rec["meta_scale0"])
    x64, t64 = rec["coords"].astype(np.float64), rec["target"].astype(np.float64)
    # the fp64 oracle (piecewise closed form) equals the reference's double run (five cubed relus)
    y64, loss64, g64 = bc.loss_and_grads(sd, L, x64, t64, s, np.float64)
    np.testing.assert_allclose(y64, rec["y64"], rtol=0, atol=1e-12)
    assert abs(loss64 - float(rec["loss64"])) <= 1e-12
    assert sorted(g64) == sorted(k[5:] for k in rec if k.startswith("g64__"))
    for k, v in g64.items():
        np.testing.assert_allclose(v, rec["g64__" + k], rtol=1e-10, atol=1e-13)
    # so does the five-term form in fp64
    y64f, _, g64f = bc.loss_and_grads(sd, L, x64, t64, s, np.float64, form="five")
    np.testing.assert_allclose(y64f, rec["y64"], rtol=0, atol=1e-12)
    for k, v in g64f.items():
        np.testing.assert_allclose(v, rec["g64__" + k], rtol=1e-10, atol=1e-13)
    # the five-term fp32 oracle equals the reference's fp32 run
    y32, _, g32 = bc.loss_and_grads(sd, L, rec["coords"], rec["target"], s, np.float32, form="five")
    assert y32.dtype == np.float32
    assert np.abs(y32 - rec["y32"]).max() <= 1e-6
    for k, v in g32.items():
        assert np.abs(v - rec["g32__" + k]).max() <= 1e-6, k


def test_piecewise_form_properties():
    l = np.linspace(-40, 40, 8001)
    np.testing.assert_allclose(bc.bspline3(l), bc.bspline3(l, "five"), rtol=0, atol=1e-10)
    near = np.linspace(-3, 3, 6001)
    np.testing.assert_allclose(bc.bspline3(near), bc.bspline3(near, "five"), rtol=0, atol=2e-12)
    np.testing.assert_allclose(bc.bspline3_d(near), bc.bspline3_d(near, "five"), rtol=0, atol=2e-12)
    h = 1e-6
    fd = (bc.bspline3(near + h) - bc.bspline3(near - h)) / (2 * h)
    np.testing.assert_allclose(bc.bspline3_d(near), fd, rtol=0, atol=1e-6)
    assert bc.bspline3(np.float64(0.0)) == pytest.approx(2 / 3) and bc.bspline3(near).max() <= 2 / 3
    # outside the support the piecewise form is exactly 0 in fp32, the five-term form is not (it cancels from |l|^3)
    far = np.float32(np.linspace(2, 40, 200))
    assert np.all(bc.bspline3(far) == 0) and np.all(bc.bspline3_d(far) == 0)
    assert np.abs(bc.bspline3(far, "five")).max() > 1e-4
    # the scale multiplies the input, not the bias, and its sign matters
    W, b, x = np.array([[0.3]]), np.array([0.4]), np.array([[0.5]])
    for s in (4.0, -4.0):
        assert bc.forward([(W, b)], None, x, s)[0, 0] == pytest.approx(bc.bspline3(np.array(s * 0.15 + 0.4)))


# ---- the module -------------------------------------------------------------------------------------------------------
def test_state_dict_matches_reference_bit_for_bit():
    rec = load_golden("small_bspline_cubic")
    model = _build(rec)
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
    assert model.complex is False and model.pos_encode is False
    d = model.net_desc()
    assert d.kind == 12 and d.scale0 == np.float32(rec["meta_scale0"])
    assert (d.in_features, d.width, d.hidden_layers, d.out_features) == (2, 32, 2, 3)


def test_class_defaults_state_dict_checksums():
    from wire_amd.modules import bspline_cubic
    rec = load_golden("small_bspline_cubic")
    torch.manual_seed(0)
    model = bspline_cubic.INR(2, 256, 2, 0, 3)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in rec["default_sd_keys"]]
    for k, v in sd.items():
        np.testing.assert_allclose(checksum(v.numpy()), rec["default_sd0_checksum__" + k], rtol=1e-12, atol=1e-12)
    assert model.net_desc().scale0 == 15.0 and float(sd["net.0.scale_0"]) == 15.0
    # the layer's own defaults and its attribute surface
    lay = bspline_cubic.Bsplines_cubic(3, 5)
    assert float(lay.scale_0) == 6.0 and not lay.scale_0.requires_grad and lay.omega_0 == -0.2
    assert list(lay.state_dict().keys()) == ["scale_0", "linear.weight", "linear.bias"]


def test_psnr_fixture_state_dict_checksums():
    from wire_amd.modules import bspline_cubic
    z = load_golden("psnr_bspline_cubic")
    torch.manual_seed(int(z["seed"]))
    model = bspline_cubic.INR(2, int(z["hidden_features"]), int(z["hidden_layers"]), 0, 3, scale=float(z["scale"]))
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.numpy()), z["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)
    assert z["losses"].shape == z["losses64"].shape == (int(z["niters"]),)
    dev = np.max(np.abs(z["losses"] - z["losses64"]) / z["losses64"])
    assert dev == pytest.approx(float(z["ref32_dev_vs_double"]), rel=1e-12)


# ---- descriptor and ABI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{}, {"split_f16": 0}, {"split_bf16": 0}, {"fused_fwd": 0}])
@pytest.mark.parametrize("shape", [(2, 256, 2, 3), (3, 250, 4, 1), (2, 128, 1, 3), (4, 300, 0, 8)])
def test_size_queries_equal_bspline_form(shape, knobs):
    from _util import tune
    from wire_amd import _lib
    L = _lib.lib()
    assert L.wire_abi_version() == 1 and _lib.ABI_VERSION == 1 and _lib.KIND["bspline_cubic"] == 12
    D, K, Lh, O = shape
    with tune(**knobs):
        c = _lib.make_desc("bspline_cubic", D, K, Lh, O, -0.2, -0.2, 15.0)
        q = _lib.make_desc("bspline_form", D, K, Lh, O, -0.2, -0.2, 15.0)
        assert c.kind == 12 and C.sizeof(c) == 36
        nt = L.wire_num_param_tensors(C.byref(c))
        assert nt == L.wire_num_param_tensors(C.byref(q)) == 2 * (Lh + 1) + 2
        for t in range(nt):
            assert L.wire_param_tensor_floats(C.byref(c), t) == L.wire_param_tensor_floats(C.byref(q), t)
        assert L.wire_packed_floats(C.byref(c)) == L.wire_packed_floats(C.byref(q)) > 0
        for n in (1, 3001, 8229, 65536):
            for save in (0, 1):
                assert L.wire_act_bytes(C.byref(c), n, save) == L.wire_act_bytes(C.byref(q), n, save) > 0
            assert L.wire_bwd_scratch_bytes(C.byref(c), n) == L.wire_bwd_scratch_bytes(C.byref(q), n) > 0
            assert L.wire_bwd_coords_scratch_bytes(C.byref(c), n) == L.wire_bwd_coords_scratch_bytes(C.byref(q), n) > 0
        assert L.wire_act_out_offset(C.byref(c), 8229, Lh) == L.wire_act_out_offset(C.byref(q), 8229, Lh)


def test_bad_scale_is_err_arg_with_a_message():
    from wire_amd import _lib
    L = _lib.lib()
    for bad in (0.0, float("inf"), float("-inf"), float("nan")):
        d = _lib.make_desc("bspline_cubic", 2, 256, 2, 3, -0.2, -0.2, bad)
        assert L.wire_packed_floats(C.byref(d)) == -1          # WIRE_ERR_ARG
        assert b"scale0" in L.wire_last_error()
        assert L.wire_num_param_tensors(C.byref(d)) == -1
        assert L.wire_act_bytes(C.byref(d), 100, 1) == -1 and L.wire_bwd_scratch_bytes(C.byref(d), 100) == -1
    # a negative scale is a scale; posenc stays relu's
    d = _lib.make_desc("bspline_cubic", 2, 256, 2, 3, -0.2, -0.2, -4.0)
    assert L.wire_packed_floats(C.byref(d)) > 0
    d = _lib.make_desc("bspline_cubic", 2, 256, 2, 3, -0.2, -0.2, 4.0, 7)
    assert L.wire_packed_floats(C.byref(d)) == -1
    # the per-layer entry points refuse the same scales before they touch a pointer
    for bad in (0.0, float("inf"), float("nan")):
        assert L.wire_real_layer_fwd(None, 12, None, None, None, -0.2, bad, 8, 2, 4, None, None, 0) == -1
    assert L.wire_real_layer_fwd(None, 7, None, None, None, -0.2, 1.0, 8, 2, 4, None, None, 0) == -1
    assert L.wire_real_layer_fwd(None, 11, None, None, None, -0.2, 1.0, 8, 2, 4, None, None, 0) == -1


# ---- error paths ------------------------------------------------------------------------------------------------------
def test_trainable_and_factory_raise():
    from wire_amd.modules import bspline_cubic, models
    with pytest.raises(NotImplementedError):
        bspline_cubic.Bsplines_cubic(2, 8, trainable=True)
    with pytest.raises(NotImplementedError, match="outside the MI355X hot path"):
        models.get_INR("bspline_cubic", 2, 64, 0, 1, 3)
    assert "bspline_cubic" not in models.model_dict


def test_load_state_dict_reaches_descriptor_and_differing_scales_raise():
    rec = load_golden("small_bspline_cubic")
    model = _build(rec)
    sd = model.state_dict()
    for k in sd:
        if k.endswith("scale_0"):
            sd[k] = torch.full((1,), 0.3)
    model.load_state_dict(sd)
    assert model.net_desc().scale0 == np.float32(0.3)
    sd["net.1.scale_0"] = torch.full((1,), -0.3)              # the sign matters: |s| equal is not equal
    with pytest.raises(NotImplementedError):
        model.load_state_dict(sd)


def test_no_cpu_fallback():
    from wire_amd import _lib
    from wire_amd.modules import bspline_cubic
    model = _build(load_golden("small_bspline_cubic"))
    with pytest.raises(_lib.WireHipError):
        model(torch.zeros(8, 2))
    with pytest.raises(_lib.WireHipError):
        bspline_cubic.INR(2, 32, 1, 0, 3, outermost_linear=False)(torch.zeros(8, 2))
    with pytest.raises(_lib.WireHipError):
        bspline_cubic.Bsplines_cubic(2, 8)(torch.zeros(8, 2))
