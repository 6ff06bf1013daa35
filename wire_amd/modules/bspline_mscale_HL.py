"""Multi-scale quadratic B-spline INR -- drop-in for the reference's modules/bspline_mscale_HL.py.

  Bsplines_form(in_features, out_features, ...)            the layer of modules/bspline_form.py (same class here)
  Scaled_Bsplines_form(in_features, out_features, bias, is_first, omega0, sigma0, init_weights, trainable)
      lin = linear(x); column j divided by sigma0[g(j)], g = 0 on [0, min(256, out)), then T - 1 equal groups over
      [256, out); B of each -- computed on a detached copy: no gradient reaches linear or the input
  INR(in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features, outermost_linear,
      first_omega_0, hidden_omega_0, scale, scale_tensor, pos_encode, multiscale, sidelength, fn_samples,
      use_nyquist)
      net = Scaled_Bsplines_form(D -> SHF), Bsplines_form(SHF -> K), max(L - 1, 0) x Bsplines_form(K -> K),
            nn.Linear(K -> O)

Same ``state_dict`` keys, order, dtypes and RNG stream as the reference (``scale_0`` of the first stage is the [T]
scale tensor, of the others a [1] Parameter; all non-trainable).  The whole net runs as WIRE_KIND_BSPLINE_MS
(include/wire_hip.h): the first stage is a HIP kernel that writes the feature map of the SHF -> K GEMM, and the
backward stops at that GEMM's weight gradient, so ``net[0].linear`` and the coordinates never receive a gradient.
What the reference cannot run (fewer than two scales, a column split that does not add up to SHF, a zero or
non-finite scale) and ``outermost_linear=False`` raise NotImplementedError; a plain list is accepted as scale_tensor.
"""
from __future__ import annotations

from typing import List

import torch
from torch import nn

from .. import _lib
from ._base import ActivationLayer, FinalLinear, HipINR, check_scales, scale_list
from .bspline_form import Bsplines_form

__all__ = ["Bsplines_form", "Scaled_Bsplines_form", "INR", "column_groups"]


def column_groups(out_features: int, nscales: int) -> List[int]:
    """Scale index of every output column of the first stage (the reference's slicing), or NotImplementedError for the
    shapes the reference cannot build a net from."""
    shf, T = int(out_features), int(nscales)
    if T < 2 or T > _lib.MS_MAX_SCALES:
        raise NotImplementedError(f"bspline_mscale_HL needs 2..{_lib.MS_MAX_SCALES} scales, got {T}")
    if shf < 1:
        raise NotImplementedError(f"bspline_mscale_HL needs scaled_hidden_features >= 1, got {shf}")
    if shf <= 256:
        return [0] * shf
    split = (shf - 256) // (T - 1)
    if split < 1 or 256 + (T - 1) * split != shf:
        raise NotImplementedError(f"scaled_hidden_features {shf} is not 256 + {T - 1} equal column groups")
    return [0] * 256 + [1 + (j - 256) // split for j in range(256, shf)]


class Scaled_Bsplines_form(ActivationLayer):
    kind = "bspline_mscale_HL"

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega0=-0.2, sigma0=[],
                 init_weights=False, trainable=False):
        super().__init__()
        if trainable:
            raise NotImplementedError("Scaled_Bsplines_form(trainable=True): trainable scales are not on the MI355X path")
        scales = scale_list(sigma0)
        column_groups(out_features, len(scales))
        check_scales(self.kind, scales)
        self.is_first = is_first
        self.in_features = in_features
        self.out_features = out_features
        st = sigma0.detach().clone() if isinstance(sigma0, torch.Tensor) else torch.tensor(scales)
        self.scale_0 = nn.Parameter(st, False)          # before the Linear, as the reference registers it
        self.linear = self._build_linear(in_features, out_features, bias, complex_dtype=False)
        self.omega_0 = omega0
        self._w = float(omega0)
        self._scales = scales

    def refresh_hparams(self):
        scales = scale_list(self.scale_0)
        column_groups(self.out_features, len(scales))
        check_scales(self.kind, scales)
        self._scales = scales
        self._s = scales[0]

    def abi_tensors(self):
        return [self.linear.weight, self._bias_or_zeros(self.linear)]

    def forward(self, input):
        from .. import functional as Fh
        return Fh.mscale_first(input, self.linear.weight, self._bias_or_zeros(self.linear), self._scales)


class INR(HipINR):
    kind = "bspline_mscale_HL"

    def __init__(self, in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features,
                 outermost_linear=True, first_omega_0=-0.2, hidden_omega_0=-0.2, scale=15.0, scale_tensor=[],
                 pos_encode=False, multiscale=True, sidelength=512, fn_samples=None, use_nyquist=True):
        super().__init__()
        if not outermost_linear:
            raise NotImplementedError("bspline_mscale_HL with outermost_linear=False is not on the MI355X path")
        scales = scale_list(scale_tensor)
        column_groups(scaled_hidden_features, len(scales))
        check_scales(self.kind, scales + [float(scale)])
        self.nonlin = Bsplines_form
        self.nonlin_first = Scaled_Bsplines_form
        self.scale_tensor = scale_tensor
        self.in_features = in_features
        self.complex = False
        self.pos_encode = False
        layers = [Scaled_Bsplines_form(in_features, scaled_hidden_features, omega0=first_omega_0, sigma0=scale_tensor,
                                       is_first=True, trainable=False),
                  Bsplines_form(scaled_hidden_features, hidden_features, omega0=hidden_omega_0, sigma0=scale)]
        layers += [Bsplines_form(hidden_features, hidden_features, omega0=hidden_omega_0, sigma0=scale)
                   for _ in range(hidden_layers - 1)]
        layers.append(FinalLinear(hidden_features, out_features, dtype=torch.float))
        self._shf = int(scaled_hidden_features)
        self._finish(layers, in_features, hidden_features, hidden_layers, out_features,
                     first_omega_0, hidden_omega_0, scale)

    def refresh_hparams(self) -> None:
        """Stage 0's [T] scales and the one hidden scale (every later layer's ``scale_0``) into the descriptor."""
        first, rest = self.net[0], [m for m in list(self.net)[1:] if isinstance(m, Bsplines_form)]
        first.refresh_hparams()
        for m in rest:
            m.refresh_hparams()
        if len({m._s for m in rest}) > 1:
            raise NotImplementedError("per-layer scale_0 values differ; the fused path supports one hidden scale")
        check_scales(self.kind, [rest[0]._s])
        self._arch["scale0"] = rest[0]._s

    def net_desc(self) -> _lib.NetDesc:
        a = self._arch
        return _lib.make_desc_ms(a["in_features"], a["width"], a["hidden_layers"], a["out_features"],
                                 a["first_omega0"], a["hidden_omega0"], a["scale0"], self._shf, self.net[0]._scales)

    def forward(self, coords: torch.Tensor) -> torch.Tensor:
        # the first stage works on detached slices (modules/bspline_mscale_HL.py): the coordinates get no gradient
        return super().forward(coords.detach())
