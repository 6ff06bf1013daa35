"""Hierarchical quadratic B-spline INR -- drop-in for the reference's modules/bspline_mscale_hier.py.

  Bsplines_form(in_features, out_features, bias, is_first, omega0, sigma0, init_weights, trainable)
      B(linear(x) / scale_0), scale_0 a non-trainable Parameter registered before ``linear``
  INR(in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features, outermost_linear,
      first_omega_0, hidden_omega_0, scale, scale_tensor, pos_encode, multiscale, sidelength, fn_samples, use_nyquist)
      per entry sigma_s of scale_tensor a stage ``stages[s]`` = Bsplines_form(D -> K), Bsplines_form(K -> K, or 2K -> K
      for s > 0), (hidden_layers - 1) x Bsplines_form(K -> K), every layer with sigma_s, and a head
      ``linears[s]`` = nn.Linear(K -> O) built right behind it.  forward: stage 0 runs all its layers on the coordinates;
      stage s > 0 runs its layer 0 on the coordinates, its layer 1 on [that | the previous stage's output] and its layer
      2; the result is the sum of the heads.

Same ``state_dict`` keys, order and RNG stream as the reference.  ``linears`` is a plain Python list, as there: the heads
are in neither ``state_dict()`` nor ``parameters()``, ``.cuda()`` does not move them, and ``forward`` (and
``param_tensors``) move them to where the stages are.  The whole net runs as WIRE_KIND_BSPLINE_HIER (include/wire_hip.h)
with the heads at the end of the ABI's params[].  For ``hidden_layers > 2`` the layers ``stages[s > 0][3:]`` exist (the
reference builds them and never runs them) and are not ABI tensors.  ``scale``, ``scaled_hidden_features``, both omegas,
``pos_encode`` and ``outermost_linear`` are accepted and ignored, as in the reference.  The reference's ``cat(dim=2)``
needs a [1][n][D] input when there is more than one stage; here any [..., D] input is taken as rows of D coordinates.
No scale (the default ``scale_tensor=[]``), more than eight, a zero or non-finite one, ``hidden_layers < 1``,
``hidden_layers == 1`` with more than one scale and ``trainable=True`` raise NotImplementedError.
"""
from __future__ import annotations

from typing import List

import torch
from torch import nn

from .. import _lib, functional as Fh
from ._base import ActivationLayer, HipINR, _param_value, _scalar_param, check_scales, scale_list

__all__ = ["Bsplines_form", "INR"]


class Bsplines_form(ActivationLayer):
    kind = "bspline_form"

    def __init__(self, in_features, out_features, bias=True, is_first=False, omega0=-0.2, sigma0=6.0,
                 init_weights=False, trainable=False):
        super().__init__()
        if trainable:
            raise NotImplementedError("bspline_mscale_hier Bsplines_form(trainable=True): a trainable scale_0 is not on "
                                      "the MI355X path")
        self.omega_0 = omega0
        self.is_first = is_first
        self.in_features = in_features
        self.out_features = out_features
        self.scale_0 = _scalar_param(sigma0, False)            # before the Linear, as the reference registers it
        self.linear = self._build_linear(in_features, out_features, bias, complex_dtype=False)
        self._w = float(omega0)
        self._s = float(sigma0)
        if init_weights:
            self.init_weights()

    def init_weights(self):
        with torch.no_grad():
            if self.is_first:
                self.linear.weight.normal_(mean=0.0, std=2 / (self.in_features))

    def refresh_hparams(self):
        self._s = _param_value(self.scale_0)

    def abi_tensors(self):
        return [self.linear.weight, self._bias_or_zeros(self.linear)]

    def forward(self, input):
        return Fh.real_layer(self.kind, input, self.linear.weight, self._bias_or_zeros(self.linear), self._w, self._s)


class INR(HipINR):
    kind = "bspline_mscale_hier"

    def __init__(self, in_features, hidden_features, scaled_hidden_features, hidden_layers, out_features,
                 outermost_linear=True, first_omega_0=-0.2, hidden_omega_0=-0.2, scale=15.0, scale_tensor=[],
                 pos_encode=False, multiscale=True, sidelength=512, fn_samples=None, use_nyquist=True):
        super().__init__()
        scales = scale_list(scale_tensor)
        check_scales(self.kind, scales, 1)
        hidden_layers = int(hidden_layers)
        if hidden_layers < 1:
            raise NotImplementedError(f"bspline_mscale_hier needs hidden_layers >= 1, got {hidden_layers}")
        if hidden_layers == 1 and len(scales) > 1:
            raise NotImplementedError("bspline_mscale_hier with hidden_layers == 1 and more than one scale: a later stage "
                                      "runs its layers 0, 1 and 2 (the reference's forward raises IndexError)")
        self.stages = nn.ModuleList()
        self.linears = []                                   # a plain list, as in the reference
        self.nonlin = Bsplines_form
        self.scale_tensor = scale_tensor
        self.complex = False
        self.pos_encode = False
        self.num_stages = len(scales)
        self.scale0 = scale
        for s, sigma in enumerate(scales):
            layers = [Bsplines_form(in_features, hidden_features, omega0=first_omega_0, sigma0=sigma),
                      Bsplines_form(hidden_features * 2 if s != 0 else hidden_features, hidden_features,
                                    omega0=hidden_omega_0, sigma0=sigma)]
            layers += [Bsplines_form(hidden_features, hidden_features, omega0=hidden_omega_0, sigma0=sigma)
                       for _ in range(hidden_layers - 1)]
            self.stages.append(nn.Sequential(*layers))
            self.linears.append(nn.Linear(hidden_features, out_features))
        self._scales = scales
        self._arch = dict(in_features=int(in_features), width=int(hidden_features), hidden_layers=hidden_layers,
                          out_features=int(out_features), first_omega0=float(first_omega_0),
                          hidden_omega0=float(hidden_omega_0), scale0=float(scale), posenc_freqs=0)
        self._layerwise = False
        self.register_load_state_dict_post_hook(lambda m, _keys: m.refresh_hparams())

    @property
    def net(self):
        """The layers the forward runs, stage by stage (a list, not a registered module)."""
        return [m for s, st in enumerate(self.stages) for m in self._used(s, st)]

    def _used(self, s: int, stage) -> list:
        return list(stage) if s == 0 else list(stage)[:3]

    def refresh_hparams(self) -> None:
        """Re-read every stage's scale_0 into the descriptor (after ``load_state_dict`` -- done automatically -- or a
        manual edit).  One divisor per stage: values that differ within a stage raise."""
        scales = []
        for s, stage in enumerate(self.stages):
            for m in stage:
                m.refresh_hparams()
            vals = {m._s for m in self._used(s, stage)}
            if len(vals) > 1:
                raise NotImplementedError(f"bspline_mscale_hier stage {s}: per-layer scale_0 values differ "
                                          f"({sorted(vals)}); the MI355X path takes one divisor per stage")
            scales.append(vals.pop())
        check_scales(self.kind, scales, 1)
        self._scales = scales

    def net_desc(self) -> _lib.NetDesc:
        a = self._arch
        return _lib.make_desc_hier(a["in_features"], a["width"], a["hidden_layers"], a["out_features"],
                                   a["first_omega0"], a["hidden_omega0"], a["scale0"], self._scales)

    def _heads_to(self, device) -> None:
        for i, lin in enumerate(self.linears):
            self.linears[i] = lin.to(device)

    def param_tensors(self) -> List[torch.Tensor]:
        """The ABI's params[]: every stage's used layers, then the heads (moved to where the stages are)."""
        self._heads_to(self.stages[0][0].linear.weight.device)
        out: List[torch.Tensor] = []
        for m in self.net:
            out += m.abi_tensors()
        for lin in self.linears:
            out += [lin.weight, lin.bias]
        return out

    def forward(self, coords: torch.Tensor) -> torch.Tensor:
        return Fh.inr_forward(coords, self.net_desc(), self.param_tensors())
