"""Multi-pass quadratic B-spline INR -- drop-in for the reference's modules/bspline_mscale_2.py.

  Bsplines_form(in_features, out_features, bias, is_first, omega0, init_weights, trainable)
      forward(input, scale) = B(linear(input) / scale) -- no scale_0 Parameter of its own
  AdaptiveScaleCombiner(num_scales, out_features, image_size, type)
      scale_weights [S], freq_mlp = Linear(S O -> 128), ReLU, Linear(128 -> O), refine = Linear(O -> 128), ReLU,
      Linear(128 -> O); forward(outputs, 'freq_combine') = freq_mlp([outputs[0] | outputs[1] | ..])
  INR(in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features, outermost_linear,
      first_omega_0, hidden_omega_0, scale, scale_tensor, pos_encode, multiscale, sidelength, fn_samples, use_nyquist)
      combine_scales, then net = Bsplines_form(D -> K), hidden_layers x Bsplines_form(K -> K), nn.Linear(K -> O);
      forward(x) runs the whole net once per entry of scale_tensor and combines the S outputs

Same ``state_dict`` keys, order and RNG stream as the reference (the combiner is built before ``net``).  The whole net
runs as WIRE_KIND_BSPLINE_M2 (include/wire_hip.h): the trunk's passes, the combiner and their backward in HIP, with
freq_mlp's tensors first in the ABI's params[].  ``scale_weights`` and ``refine`` never receive a gradient, as in the
reference's loop.  ``scale`` is kept as ``scale0`` and not used.  No scale (the default ``scale_tensor=[]``), more than
eight, a zero or non-finite one, ``outermost_linear=False``, ``trainable=True`` and the combiner's 'scale_weights' /
'both' modes raise NotImplementedError.
"""
from __future__ import annotations

from typing import List

import torch
from torch import nn

from .. import _lib, functional as Fh
from ._base import ActivationLayer, FinalLinear, HipINR, check_scales, scale_list

__all__ = ["Bsplines_form", "AdaptiveScaleCombiner", "INR"]


class Bsplines_form(ActivationLayer):
    kind = "bspline_form"

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega0=-0.2, init_weights=False,
                 trainable=False):
        super().__init__()
        if trainable:
            raise NotImplementedError("bspline_mscale_2 Bsplines_form(trainable=True) is not on the MI355X path")
        self.is_first = is_first
        self.in_features = in_features
        self.out_features = out_features
        self.linear = self._build_linear(in_features, out_features, bias, complex_dtype=False)
        self.omega_0 = omega0
        if init_weights:
            self.init_weights()

    def init_weights(self):
        with torch.no_grad():
            if self.is_first:
                self.linear.weight.normal_(mean=0.0, std=2 / (self.in_features))

    def abi_tensors(self):
        return [self.linear.weight, self._bias_or_zeros(self.linear)]

    def forward(self, input, scale):
        s = float(scale)
        check_scales("bspline_mscale_2", [s], 1)
        return Fh.real_layer(self.kind, input, self.linear.weight, self._bias_or_zeros(self.linear),
                             float(self.omega_0), s)


class AdaptiveScaleCombiner(nn.Module):
    def __init__(self, num_scales, out_features, image_size, type):
        super().__init__()
        self.num_scales = num_scales
        self.out_features = out_features
        self.image_size = image_size
        self.type = type
        self.scale_weights = nn.Parameter(torch.ones(num_scales))
        self.freq_mlp = nn.Sequential(nn.Linear(num_scales * out_features, 128), nn.ReLU(), nn.Linear(128, out_features))
        self.refine = nn.Sequential(nn.Linear(out_features, 128), nn.ReLU(), nn.Linear(128, out_features))

    def abi_tensors(self):
        """freq_mlp's tensors, the first four of the ABI's params[]."""
        return [self.freq_mlp[0].weight, self.freq_mlp[0].bias, self.freq_mlp[2].weight, self.freq_mlp[2].bias]

    def forward(self, outputs, type):
        if type != 'freq_combine':
            raise NotImplementedError(f"AdaptiveScaleCombiner mode '{type}': only 'freq_combine' (the one the "
                                      "reference's INR calls) is on the MI355X path")
        return Fh.m2_combine(list(outputs), *self.abi_tensors())


class INR(HipINR):
    kind = "bspline_mscale_2"

    def __init__(self, in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features,
                 outermost_linear=True, first_omega_0=-0.2, hidden_omega_0=-0.2, scale=15.0, scale_tensor=[],
                 pos_encode=False, multiscale=True, sidelength=512, fn_samples=None, use_nyquist=True):
        super().__init__()
        if not outermost_linear:
            raise NotImplementedError("bspline_mscale_2 with outermost_linear=False is not on the MI355X path")
        scales = scale_list(scale_tensor)
        check_scales(self.kind, scales, 1)
        self.nonlin = Bsplines_form
        self.complex = False
        self.pos_encode = False
        self.scale0 = scale
        self.scale_tensor = scale_tensor
        self.outermost_linear = outermost_linear
        self.in_features = in_features
        # before `net`, as the reference builds it: the RNG stream and the state_dict start with the combiner
        self.combine_scales = AdaptiveScaleCombiner(len(scales), out_features, sidelength, 'both')
        layers = [Bsplines_form(in_features, hidden_features, omega0=first_omega_0)]
        layers += [Bsplines_form(hidden_features, hidden_features, omega0=hidden_omega_0)
                   for _ in range(int(hidden_layers))]
        layers.append(FinalLinear(hidden_features, out_features, dtype=torch.float))
        self._scales = scales
        self._finish(layers, in_features, hidden_features, hidden_layers, out_features,
                     first_omega_0, hidden_omega_0, scale)

    def net_desc(self) -> _lib.NetDesc:
        a = self._arch
        return _lib.make_desc_m2(a["in_features"], a["width"], a["hidden_layers"], a["out_features"],
                                 a["first_omega0"], a["hidden_omega0"], a["scale0"], self._scales)

    def param_tensors(self) -> List[torch.Tensor]:
        return self.combine_scales.abi_tensors() + super().param_tensors()
