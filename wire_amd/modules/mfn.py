"""Multiplicative filter network -- drop-in for the reference's modules/mfn.py.

  GaborLayer(in_dim, out_dim, padding, alpha, beta=1.0, bias=False)
      g(x)_j = exp(-gamma_j / 2 |x - mu_j|^2) sin(x . w_j + c_j) with trained mu [out][in], gamma [out],
      linear.weight = w [out][in], linear.bias = c [out]
  INR(in_features, hidden_features, hidden_layers, out_features, outermost_linear, first_omega_0, hidden_omega_0, scale,
      pos_encode, sidelength, fn_samples, use_nyquist)
      k = hidden_layers + 1 filters ``gabon_filters`` (sic) of the COORDINATES and k linears ``linear``:
      z_0 = g_0(x), z_{i+1} = linear[i](z_i) * g_{i+1}(x), y = linear[k - 1](z_{k-1})

Same ``state_dict`` keys, order and RNG stream as the reference (same ``torch.manual_seed`` -> the same bits).  The whole
net runs as WIRE_KIND_MFN (include/wire_hip.h); ``GaborLayer.forward`` on its own runs ``wire_mfn_filter_fwd`` with its
own autograd node.  Every argument behind ``out_features`` is accepted and ignored, as in the reference.  The reference
evaluates ``x[0, ...]`` and returns ``[None, ...]``: here the input is [1][n][D] and anything else is a ValueError (the
reference would silently drop the other batch entries, or take the first row of a 2-D input for the batch).
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch
from torch import nn

from .. import _lib, functional as Fh
from ._base import HipINR

__all__ = ["GaborLayer", "INR"]


class GaborLayer(nn.Module):
    def __init__(self, in_dim, out_dim, padding, alpha, beta=1.0, bias=False):
        super().__init__()
        self.mu = nn.Parameter(torch.rand((out_dim, in_dim)) * 2 - 1)
        self.gamma = nn.Parameter(torch.distributions.gamma.Gamma(alpha, beta).sample((out_dim, )))
        self.linear = torch.nn.Linear(in_dim, out_dim)
        self.linear.weight.data *= 128. * torch.sqrt(self.gamma.unsqueeze(-1))
        self.linear.bias.data.uniform_(-np.pi, np.pi)

    def abi_tensors(self) -> List[torch.Tensor]:
        return [self.mu, self.gamma, self.linear.weight, self.linear.bias]

    def forward(self, input):
        if input.dim() != 2 or input.shape[1] != self.mu.shape[1]:
            raise ValueError(f"GaborLayer takes [n][{self.mu.shape[1]}] coordinates, got {tuple(input.shape)}")
        return Fh.mfn_filter(input, self.mu, self.gamma, self.linear.weight, self.linear.bias)


class INR(HipINR):
    kind = "mfn"

    def __init__(self, in_features=2, hidden_features=256, hidden_layers=4, out_features=1, outermost_linear=True,
                 first_omega_0=0, hidden_omega_0=0, scale=1, pos_encode=False, sidelength=1, fn_samples=None,
                 use_nyquist=None):
        super().__init__()
        hidden_layers = int(hidden_layers)
        if hidden_layers < 0:
            raise ValueError(f"mfn needs hidden_layers >= 0, got {hidden_layers}")
        self.k = hidden_layers + 1
        self.gabon_filters = nn.ModuleList([GaborLayer(in_features, hidden_features, 0, alpha=6.0 / self.k)
                                            for _ in range(self.k)])
        self.linear = nn.ModuleList([torch.nn.Linear(hidden_features, hidden_features) for _ in range(self.k - 1)] +
                                    [torch.nn.Linear(hidden_features, out_features)])
        for lin in self.linear[:self.k - 1]:
            lin.weight.data.uniform_(-np.sqrt(1.0 / hidden_features), np.sqrt(1.0 / hidden_features))
        self._arch = dict(in_features=int(in_features), width=int(hidden_features), hidden_layers=hidden_layers,
                          out_features=int(out_features), first_omega0=float(first_omega_0),
                          hidden_omega0=float(hidden_omega_0), scale0=float(scale), posenc_freqs=0)
        self._layerwise = False

    def param_tensors(self) -> List[torch.Tensor]:
        """The ABI's params[]: the filters (mu, gamma, w, c each), the hidden linears, the final linear."""
        out: List[torch.Tensor] = []
        for f in self.gabon_filters:
            out += f.abi_tensors()
        for lin in self.linear:
            out += [lin.weight, lin.bias]
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        D = self._arch["in_features"]
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[2] != D:
            raise ValueError(f"mfn.INR takes [1][n][{D}] coordinates, got {tuple(x.shape)}")
        return Fh.inr_forward(x, self.net_desc(), self.param_tensors())
