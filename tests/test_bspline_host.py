"""bspline_form on the host: construction, state_dict parity with the reference, the closed form of B, the library's
size queries (no GPU needed).  Fixtures: tests/golden/make_bspline_golden.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import checksum, load_golden
import bspline_ref as br


def _build(rec, call="kw"):
    from wire_amd.modules import models
    torch.manual_seed(int(rec["meta_seed"]))
    D, hf, L, O, s = (int(rec["meta_D"]), int(rec["meta_hidden_features"]), int(rec["meta_L"]), int(rec["meta_O"]),
                      float(rec["meta_scale0"]))
    if call == "kw":      # bspline_img_representation.py:98-113
        return models.get_INR(nonlin="bspline_form", in_features=D, out_features=O, hidden_features=hf,
                              scaled_hidden_features=0, hidden_layers=L, first_omega_0=-0.2, hidden_omega_0=-0.2,
                              scale=s, scale_tensor=[0.0], pos_encode=False, sidelength=512)
    return models.get_INR("bspline_form", D, hf, 0, L, O, True, -0.2, -0.2, s, [0.0])   # positional, reference order


@pytest.mark.parametrize("call", ["kw", "pos"])
def test_state_dict_matches_reference_bit_for_bit(call):
    rec = load_golden("small_bspline_form")
    model = _build(rec, call)
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
    assert model.net_desc().kind == 5 and model.net_desc().scale0 == np.float32(rec["meta_scale0"])


def test_full_config_net_state_dict_checksums():
    rec = load_golden("full_bspline_form_2x256")
    model = _build(rec)
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(checksum(v.numpy()), rec["sd0_checksum__" + k], rtol=1e-12, atol=1e-12)


def test_closed_form_equals_four_term_form_in_fp64():
    rec = load_golden("small_bspline_form")
    r = rec["r_grid"]
    np.testing.assert_allclose(br.bspline(r), rec["B_four64"], rtol=0, atol=1e-12)
    # the derivative against central differences of the closed form (B is C1)
    h = 1e-6
    fd = (br.bspline(r + h) - br.bspline(r - h)) / (2 * h)
    np.testing.assert_allclose(br.bspline_d(r), fd, rtol=0, atol=1e-6)
    # outside the support the closed form is exactly 0, the fp32 four-term form is not
    far = np.float32(np.linspace(2, 40, 200))
    assert np.all(br.bspline(far) == 0)


def test_oracle_reproduces_the_fixture():
    rec = load_golden("small_bspline_form")
    sd = {str(k): rec["sd__" + str(k)] for k in rec["sd_keys"]}
    L, s = int(rec["meta_L"]), float(rec["meta_scale0"])
    y64, loss64, g64 = br.loss_and_grads(sd, L, rec["coords"].astype(np.float64), rec["target"].astype(np.float64),
                                         s, np.float64)
    np.testing.assert_allclose(y64, rec["y64"], rtol=0, atol=1e-12)
    for k, v in g64.items():
        np.testing.assert_allclose(v, rec["g64__" + k], rtol=1e-10, atol=1e-13)
    y32, _, g32 = br.loss_and_grads(sd, L, rec["coords"], rec["target"], s, np.float32)
    assert np.abs(y32 - rec["y32"]).max() <= 1e-6


def test_out_of_scope_kinds_and_trainable_raise():
    from wire_amd.modules import bspline_form, models
    for k in ("mfn", "bspline_mscale_HL", "bspline_cubic"):
        with pytest.raises(NotImplementedError):
            models.get_INR(k, 2, 64, 0, 1, 3)
    with pytest.raises(NotImplementedError):
        bspline_form.Bsplines_form(2, 8, trainable=True)


def test_load_state_dict_reaches_descriptor_and_differing_scales_raise():
    rec = load_golden("small_bspline_form")
    model = _build(rec)
    sd = model.state_dict()
    for k in sd:
        if k.endswith("scale_0"):
            sd[k] = torch.full((1,), 0.5)
    model.load_state_dict(sd)
    assert model.net_desc().scale0 == 0.5
    sd["net.1.scale_0"] = torch.full((1,), 0.75)
    with pytest.raises(NotImplementedError):
        model.load_state_dict(sd)


def test_size_queries_accept_kind_5_and_reject_zero_scale():
    from wire_amd import _lib
    L = _lib.lib()
    d = _lib.make_desc("bspline_form", 2, 256, 2, 3, -0.2, -0.2, 1 / 9)
    assert L.wire_num_param_tensors(C.byref(d)) == 8
    assert L.wire_param_tensor_floats(C.byref(d), 2) == 256 * 256
    assert L.wire_packed_floats(C.byref(d)) > 0
    assert L.wire_act_bytes(C.byref(d), 65536, 1) > 0
    assert L.wire_bwd_scratch_bytes(C.byref(d), 65536) > 0
    for bad in (0.0, float("inf"), float("nan")):
        d = _lib.make_desc("bspline_form", 2, 256, 2, 3, -0.2, -0.2, bad)
        assert L.wire_packed_floats(C.byref(d)) == -1          # WIRE_ERR_ARG
        assert L.wire_num_param_tensors(C.byref(d)) < 0
