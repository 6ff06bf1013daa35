"""Cubic B-spline INR -- drop-in for the reference's modules/bspline_cubic.py.

  Bsplines_cubic(in_features, out_features, bias, is_first, omega0, sigma0,
                 init_weights, trainable)                modules/bspline_cubic.py:7-52
      B(linear(scale_0 * x)), B the centred cubic B-spline
  INR(in_features, hidden_features, hidden_layers, scaled_hidden_features,
      out_features, ...)                                  :54-121

The positional order is the reference's own: ``hidden_layers`` comes BEFORE
``scaled_hidden_features`` here, unlike every other B-spline module, which is why
the reference's ``get_INR`` cannot build this net and why it is reached through
this constructor (``models.get_INR('bspline_cubic', ...)`` keeps raising).

``scale_0`` multiplies the layer's INPUT: ``lin = scale_0 (x W^T) + b`` -- the bias
is not scaled and the sign of ``scale_0`` matters.  It is a non-trainable
Parameter registered before ``linear`` (same ``state_dict`` keys, order and RNG
stream as the reference); its value reaches the fused path's descriptor at
construction and after ``load_state_dict``.  ``omega0`` / ``is_first`` /
``init_weights`` have no effect, as in the reference.  The HIP kernels evaluate
B piecewise (exactly 0 outside |lin| < 2) where the reference sums five cubed
relus in fp32 (DESIGN.md section on bspline_cubic).
"""
from __future__ import annotations

import torch

from ._base import ActivationLayer, FinalLinear, HipINR, _param_value, _scalar_param


class Bsplines_cubic(ActivationLayer):
    kind = "bspline_cubic"

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega0=-0.2, sigma0=6.0,
                 init_weights=True, trainable=False):
        super().__init__()
        if trainable:
            # the reference's INR never builds one; a trainable scale_0 needs its own gradient sums
            raise NotImplementedError("Bsplines_cubic(trainable=True): a trainable scale_0 is not on the MI355X path")
        self.omega_0 = omega0
        self.is_first = is_first
        self.in_features = in_features
        self.out_features = out_features
        self.scale_0 = _scalar_param(sigma0, False)            # modules/bspline_cubic.py:27, before the Linear
        self.linear = self._build_linear(in_features, out_features, bias, complex_dtype=False)
        self._w = float(omega0)
        self._s = float(sigma0)
        # init_weights: the reference's own initialiser is commented out (modules/bspline_cubic.py:29-39)

    def refresh_hparams(self):
        self._s = _param_value(self.scale_0)

    def abi_tensors(self):
        return [self.linear.weight, self._bias_or_zeros(self.linear)]

    def forward(self, input):
        from .. import functional as Fh
        return Fh.real_layer(self.kind, input, self.linear.weight, self._bias_or_zeros(self.linear),
                             self._w, self._s)


class INR(HipINR):
    kind = "bspline_cubic"

    def __init__(self, in_features, hidden_features, hidden_layers, scaled_hidden_features, out_features,
                 outermost_linear=True, first_omega_0=-0.2, hidden_omega_0=-0.2, scale=15.0, scale_tensor=[],
                 pos_encode=False, sidelength=512, fn_samples=None, use_nyquist=True):
        super().__init__()
        self.complex = False
        self.pos_encode = False      # legacy flag, always False (modules/bspline_cubic.py:84)
        self.nonlin = Bsplines_cubic
        layers = [Bsplines_cubic(in_features, hidden_features, omega0=first_omega_0, sigma0=scale, is_first=True,
                                 trainable=False)]
        layers += [Bsplines_cubic(hidden_features, hidden_features, omega0=hidden_omega_0, sigma0=scale)
                   for _ in range(hidden_layers)]
        if outermost_linear:
            layers.append(FinalLinear(hidden_features, out_features, dtype=torch.float))
        else:                                   # modules/bspline_cubic.py:110-115
            layers.append(Bsplines_cubic(hidden_features, out_features, omega0=hidden_omega_0, sigma0=scale))
        self._finish(layers, in_features, hidden_features, hidden_layers, out_features,
                     first_omega_0, hidden_omega_0, scale, outermost_linear=outermost_linear)
