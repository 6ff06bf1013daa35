"""Quadratic B-spline INR -- drop-in for the reference's modules/bspline_form.py.

  Bsplines_form(in_features, out_features, bias, is_first, omega0, sigma0,
                init_weights, trainable)                 modules/bspline_form.py:3-49
      B(linear(x) / scale_0), B the centred quadratic B-spline
  INR(in_features, hidden_features, scaled_hidden_features, hidden_layers,
      out_features, ...)                                  :51-114

``scale_0`` is a non-trainable Parameter registered before ``linear`` (same
``state_dict`` keys, order and RNG stream as the reference); its value reaches
the fused path's descriptor at construction and after ``load_state_dict``.
``omega0`` / ``is_first`` have no effect, as in the reference.  The HIP kernels
evaluate B piecewise (exactly 0 outside |r| < 1.5) where the reference sums
four squared relus in fp32 (DESIGN.md section on bspline_form).
"""
from __future__ import annotations

import torch

from ._base import ActivationLayer, FinalLinear, HipINR, _param_value, _scalar_param


class Bsplines_form(ActivationLayer):
    kind = "bspline_form"

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega0=-0.2, sigma0=6.0,
                 init_weights=False, trainable=False):
        super().__init__()
        if trainable:
            # the reference's INR never builds one; a trainable scale_0 needs its own gradient column sums
            raise NotImplementedError("Bsplines_form(trainable=True): a trainable scale_0 is not on the MI355X path")
        self.omega_0 = omega0
        self.is_first = is_first
        self.in_features = in_features
        self.out_features = out_features
        self.scale_0 = _scalar_param(sigma0, False)            # modules/bspline_form.py:23, before the Linear
        self.linear = self._build_linear(in_features, out_features, bias, complex_dtype=False)
        self._w = float(omega0)
        self._s = float(sigma0)
        if init_weights:
            self.init_weights()

    def init_weights(self):                                     # modules/bspline_form.py:29-36
        with torch.no_grad():
            if self.is_first:
                self.linear.weight.normal_(mean=0.0, std=2 / (self.in_features))

    def refresh_hparams(self):
        self._s = _param_value(self.scale_0)

    def abi_tensors(self):
        return [self.linear.weight, self._bias_or_zeros(self.linear)]

    def forward(self, input):
        from .. import functional as Fh
        return Fh.real_layer(self.kind, input, self.linear.weight, self._bias_or_zeros(self.linear),
                             self._w, self._s)


class INR(HipINR):
    kind = "bspline_form"

    def __init__(self, in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features,
                 outermost_linear=True, first_omega_0=-0.2, hidden_omega_0=-0.2, scale=15.0, scale_tensor=[],
                 pos_encode=False, sidelength=512, fn_samples=None, use_nyquist=True):
        super().__init__()
        self.complex = False
        self.pos_encode = False      # legacy flag, always False (modules/bspline_form.py:76)
        self.nonlin = Bsplines_form
        layers = [Bsplines_form(in_features, hidden_features, omega0=first_omega_0, sigma0=scale, is_first=True,
                                trainable=False)]
        layers += [Bsplines_form(hidden_features, hidden_features, omega0=hidden_omega_0, sigma0=scale)
                   for _ in range(hidden_layers)]
        if outermost_linear:
            layers.append(FinalLinear(hidden_features, out_features, dtype=torch.float))
        else:                                   # modules/bspline_form.py:104-109
            layers.append(Bsplines_form(hidden_features, out_features, omega0=hidden_omega_0, sigma0=scale))
        self._finish(layers, in_features, hidden_features, hidden_layers, out_features,
                     first_omega_0, hidden_omega_0, scale, outermost_linear=outermost_linear)
