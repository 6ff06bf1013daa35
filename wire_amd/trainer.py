"""Sync-free fused training step for the image-fit / occupancy loops.

Restates the inner loop of the reference's drivers
(wire_image_denoise.py:142-157, wire_occupancy.py:137-158):

    b_coords = coords[b_indices]; pix = model(b_coords); rec[b_indices] = pix
    loss = ((pix - gt[b_indices])**2).mean(); zero_grad; backward; Adam.step

as a fixed sequence of libwire_hip launches on one HIP stream with no host
synchronisation: coordinates are generated on the device from the flat indices
(per-axis linspace tables, bit-identical to the reference's grids), the MSE
gradient, the whole backward and a flat Adam update (complex parameters as real
pairs, exactly torch.optim.Adam's arithmetic) are HIP kernels.  The host gather
+ H2D copy and the per-step ``loss.item()`` of the reference are gone.

Multi-GPU: one process per GPU; the global batch is sharded contiguously
(parallel.shard_bounds), each shard's gradient is pre-scaled by n_g/B and the flat
gradient buffer is all-reduced (SUM) over RCCL: in one piece on the compute stream
after the backward (default), layer by layer on a side stream as soon as the backward
has produced each slice (WIRE_DP_OVERLAP=layer, wire_train_fwd_bwd_hooked), or -- with
``micro_shards > 1`` -- micro-shard i's under the forward and backward of micro-shard i+1.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, functional
from .modules._base import HipINR
from .modules.utils import axis_tables
from .parallel import FlatGradAllReducer, replicas_identical, shard_bounds


class FrameRegistration:
    """The device state of a learnable registration of B frames (``FusedTrainer.step_frames_registered``): ``theta``
    [B, 2, 3] float32, one matrix per frame acting on the frame's NORMALISED coordinates -- the convention of
    ``motion.get_transformed_coords`` / ``F.affine_grid``, the identity unless given -- its gradient ``grad`` (written by
    every step), Adam's ``exp_avg`` / ``exp_avg_sq`` and step count ``t``, the rate ``lr`` (a plain attribute: set it
    between steps for a schedule), ``betas`` and ``eps``.  ``pin_first`` fixes the gauge as the reference does ("Ensure
    first shift and theta are zero"): frame 0 receives a zero gradient, its moments stay zero and its matrix keeps its
    bits.  ``FusedTrainer.registration`` builds one on the trainer's device."""

    def __init__(self, B: int, device, lr: float = 1e-4, pin_first: bool = True, theta=None,
                 betas=(0.9, 0.999), eps: float = 1e-8):
        B = int(B)
        if B < 1:
            raise ValueError(f"a registration needs B >= 1 frames, not {B}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.WireHipError("FrameRegistration needs an MI355X device ('cuda')")
        self.B = B
        if theta is None:
            host = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float32).repeat(B, 1, 1)
        else:
            host = torch.as_tensor(theta).detach().to(torch.float32)
            if tuple(host.shape) != (B, 2, 3):
                raise ValueError(f"theta must be [{B}, 2, 3]")
        self.theta = host.to(device).contiguous().clone()
        self.grad = torch.zeros_like(self.theta)
        self.exp_avg = torch.zeros_like(self.theta)
        self.exp_avg_sq = torch.zeros_like(self.theta)
        self.t = 0
        self.lr = float(lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.pin_first = bool(pin_first)


class FusedTrainer:
    """``lr`` is a number for every net kind.  bspline_mscale_hier also takes a sequence of one rate per stage, the two
    loops of the reference's bspline_*.py drivers: a number steps the stages' tensors only -- the heads are not in
    ``model.parameters()`` there and keep their initial values, though their gradients are computed and present in
    ``flat_grad`` -- and a sequence steps stage s and head s with ``lr[s]`` (times the schedule's factor).  A sequence
    for any other kind, or of the wrong length, is a ValueError.  ``step_downsampled``, ``step_tv``, ``step_radon``,
    ``step_frames``, ``step_coded`` and ``step_radon_volume`` work for bspline_mscale_hier as for the other kinds.

    ``target`` is the [npoints, O] signal of ``step`` / ``step_hashed`` and the default ``gt`` of the metrics.  The
    operator steps and ``step_samples`` bring their own data, so a trainer that only runs those may pass
    ``target=None``; ``step``, ``step_hashed``, ``step_loss`` and a metric called without ``gt`` then raise ValueError."""

    def __init__(self, model: HipINR, grid: Sequence[int], target: Optional[torch.Tensor], lr: float = 5e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8, gamma: float = 0.1, niters: int = 2000,
                 coords_style: str = "torch", keep_rec: bool = False, micro_shards: int = 1,
                 group: Optional[dist.ProcessGroup] = None):
        self.L = _lib.lib()
        # the fused step runs net = first layer, L hidden layers, final LINEAR with omega / scale taken from the
        # descriptor: a net that HipINR.forward runs layer by layer is a different function here
        if getattr(model, "_layerwise", False):
            raise NotImplementedError("FusedTrainer needs outermost_linear=True: this net ends in an activation layer "
                                      "(modules/siren.py:81-84, gauss.py:63-66, relu.py:116-119) and runs layer by layer; "
                                      "train it through model(coords) + torch.optim")
        # (mfn.INR has no ``net``: its filters and linears carry no trainable omega_0 / scale_0)
        if any(getattr(m, "trainable", False) for m in getattr(model, "net", ())):
            raise NotImplementedError("FusedTrainer keeps omega_0 / scale_0 fixed (they are not in its flat parameter "
                                      "buffer); a net with trainable=True layers (modules/wire.py:80-81) trains through "
                                      "model(coords) + torch.optim")
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise _lib.WireHipError("FusedTrainer needs the model on an MI355X ('cuda')")
        self.model = model
        self.dev = p0.device
        self.desc = model.net_desc()
        self.grid = tuple(int(g) for g in grid)
        if len(self.grid) not in (2, 3) or len(self.grid) != self.desc.in_features:
            raise ValueError("grid must be (H, W) for 2 inputs or (H, W, T) for 3")
        H, W = self.grid[0], self.grid[1]
        T = self.grid[2] if len(self.grid) == 3 else None
        tx, ty, tz = axis_tables(H, W, T, style=coords_style)
        self.tx, self.ty = tx.to(self.dev), ty.to(self.dev)
        self.tz = tz.to(self.dev) if tz is not None else None
        self.npoints = H * W * (T or 1)
        self.O = self.desc.out_features
        self.target = None if target is None else \
            target.to(self.dev, torch.float32).reshape(self.npoints, self.O).contiguous()
        self.rec = torch.zeros(self.npoints, self.O, dtype=torch.float32, device=self.dev) if keep_rec else None

        # ---- flat parameter / gradient / Adam-state buffers; parameters become views
        tensors = model.param_tensors()
        self.sizes = [int(_lib.check(self.L.wire_param_tensor_floats(C.byref(self.desc), i)))
                      for i in range(len(tensors))]
        # every tensor starts on a 16-byte boundary (complex views need an even
        # float offset); the pad floats stay zero in params, grads and Adam state
        padded = [(sz + 3) // 4 * 4 for sz in self.sizes]
        self.count = sum(padded)
        self.flat = torch.zeros(self.count, dtype=torch.float32, device=self.dev)
        off = 0
        self.offsets: List[int] = []
        with torch.no_grad():
            for t, sz in zip(tensors, self.sizes):
                src = torch.view_as_real(t.detach()).reshape(-1) if t.is_complex() else t.detach().reshape(-1)
                if src.numel() != sz:
                    raise _lib.WireHipError("parameter size does not match the ABI's layout")
                view = self.flat[off:off + sz]
                view.copy_(src)
                t.data = torch.view_as_complex(view.view(*t.shape, 2)) if t.is_complex() \
                    else view.view(t.shape)
                self.offsets.append(off)
                off += (sz + 3) // 4 * 4
        self.micro = max(1, int(micro_shards))
        # +1: the loss rides at the end of each gradient buffer through the all-reduce
        self.gbuf = [torch.zeros(self.count + 1, dtype=torch.float32, device=self.dev)
                     for _ in range(self.micro)]
        self.exp_avg = torch.zeros(self.count, dtype=torch.float32, device=self.dev)
        self.exp_avg_sq = torch.zeros(self.count, dtype=torch.float32, device=self.dev)
        fp = self.flat.data_ptr()
        self.param_ptrs = _lib.ptr_array([fp + 4 * o for o in self.offsets])
        self.grad_ptrs = [_lib.ptr_array([g.data_ptr() + 4 * o for o in self.offsets]) for g in self.gbuf]
        self.packed = torch.empty(self.L.wire_packed_floats(C.byref(self.desc)), dtype=torch.float32,
                                  device=self.dev)
        self.partial = torch.empty(4096, dtype=torch.float32, device=self.dev)

        self.betas, self.eps = betas, float(eps)
        self._set_lr(lr)
        self.gamma, self.niters = float(gamma), int(niters)
        self.epoch = 0
        self.t = 0
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        # one micro-shard: nothing to overlap the collective with, so it is issued from the compute stream
        # (two cross-stream hand-offs fewer per step); several: a side stream overlaps it with the next shard
        side = self.micro > 1 and os.environ.get("WIRE_DP_SIDE_STREAM", "1") != "0" or \
            os.environ.get("WIRE_DP_SIDE_STREAM", "") == "1"
        # WIRE_DP_OVERLAP=layer (one micro-shard): PER-LAYER overlap -- wire_train_fwd_bwd_hooked announces each layer's
        # gradient as soon as its last kernel is enqueued, and that slice of the flat buffer is all-reduced on a side stream
        # while the compute stream runs the backward of the layers below it; only the first layer's (smallest, last) slice is
        # exposed.  Default "none": one all-reduce of the whole 2.1 MB buffer after the backward -- measured on the one-rank
        # communicator (tools/dp_overhead.sh) the six cross-stream hand-offs of "layer" cost 0.07 - 0.09 ms per step, as
        # much as the whole latency-bound all-reduce they would hide.
        self.overlap = self.micro == 1 and os.environ.get("WIRE_DP_OVERLAP", "none") == "layer"
        self.reducers = [FlatGradAllReducer(g, group, use_side_stream=side or self.overlap) for g in self.gbuf]
        # (host-staged exchange -- the gloo rehearsal with device gradients -- would block inside the announcement callback,
        #  which must not wait for the device (include/wire_hip.h): one reduction after the backward instead)
        self.overlap = self.overlap and self.reducers[0].active and not self.reducers[0].stage_host
        self._cb_err: Optional[BaseException] = None
        # the C callback only exists with the per-layer overlap, and holds the trainer weakly: no reference cycle, so
        # `del trainer` releases the act / scratch / gradient buffers at once
        self._ready_cb = None
        if self.overlap:
            import weakref
            ref = weakref.ref(self)

            def _cb(user, first, n):
                tr = ref()
                if tr is not None:
                    tr._on_grad_ready(user, first, n)
            self._ready_cb = _lib.GRAD_READY_FN(_cb)
        # WIRE_DP_CHECK=k: every k optimizer steps the replicas compare a checksum of their parameters (one host sync);
        # a divergence raises instead of training on silently
        self.check_every = max(0, int(os.environ.get("WIRE_DP_CHECK", "0")))
        self._cap = 0
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self._hidx: Optional[torch.Tensor] = None
        if self.world > 1:
            # replicas start from rank 0's parameters whatever seed each rank was built under; they stay
            # identical because every rank applies the same Adam update to the same reduced gradient
            self._broadcast_from_rank0(self.flat)

    def _set_lr(self, lr) -> None:
        """base_lr and the slices (lo, hi, rate) of the flat buffer that Adam steps."""
        hier = self.desc.kind == _lib.KIND["bspline_mscale_hier"]
        if isinstance(lr, (list, tuple)) or (isinstance(lr, torch.Tensor) and lr.dim() > 0):
            rates = [float(v) for v in lr]
            S = int(self.desc._b_base_.nscales) if hier else 0
            if not hier:
                raise ValueError("a sequence of learning rates is the per-stage loop of bspline_mscale_hier only")
            if len(rates) != S:
                raise ValueError(f"{len(rates)} learning rates for {S} stages")
        else:
            rates = None
        self.base_lr = rates if rates is not None else float(lr)
        if not hier:
            self._adam_slices = [(0, self.count, self.base_lr)]
            return
        S, L = int(self.desc._b_base_.nscales), int(self.desc.hidden_layers)
        first, _, head0 = _lib.hier_tensor_map(L, S)                         # first tensor of each stage, of the heads
        lo = [self.offsets[t] for t in first] + [self.offsets[head0]]
        if rates is None:                                                    # the stages alone: the heads keep their bits
            self._adam_slices = [(0, lo[-1], self.base_lr)]
            return
        hl = [self.offsets[head0 + 2 * s] for s in range(S)] + [self.count]
        self._adam_slices = [(lo[s], lo[s + 1], rates[s]) for s in range(S)] + \
                            [(hl[s], hl[s + 1], rates[s]) for s in range(S)]

    def _adam(self, stream, g: torch.Tensor) -> None:
        """torch.optim.Adam's step over the slices of the flat buffer, each with its rate times the schedule's factor."""
        f = self.lr_factor()
        for lo, hi, rate in self._adam_slices:
            _lib.check(self.L.wire_adam_step_flat(stream, self.flat.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo,
                                                  self.exp_avg.data_ptr() + 4 * lo, self.exp_avg_sq.data_ptr() + 4 * lo,
                                                  hi - lo, rate * f, self.betas[0], self.betas[1], self.eps, self.t),
                       "adam")

    def _broadcast_from_rank0(self, t: torch.Tensor) -> None:
        if dist.get_backend(self.group) == "gloo" and t.is_cuda:     # rehearsal backend: stage through the host
            host = t.detach().cpu()
            dist.broadcast(host, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0,
                           group=self.group)
            t.copy_(host)
        else:
            dist.broadcast(t, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0,
                           group=self.group)

    def _ready_order(self):
        """(first_tensor, n_tensors) in the order wire_train_fwd_bwd_hooked announces them (include/wire_hip.h)."""
        nt = len(self.offsets)
        hidden = int(self.desc.hidden_layers)
        if self.desc.kind == _lib.KIND["bspline_mscale_hier"]:
            # the heads (one block at the end), then the stages from the last to the first, each from its last layer
            S = int(self.desc._b_base_.nscales)
            first, last, _ = _lib.hier_tensor_map(hidden, S)
            yield nt - 2 * S, 2 * S
            for s in range(S - 1, -1, -1):
                for l in range(last[s], -1, -1):
                    yield first[s] + 2 * l, 2
            return
        if self.desc.kind == _lib.KIND["mfn"]:
            # the final linear; then for i = L-1 .. 0 the pair {W_i, b_i} and the four tensors of filter i + 1; filter 0
            yield nt - 2, 2
            for i in range(hidden - 1, -1, -1):
                yield 4 * (hidden + 1) + 2 * i, 2
                yield 4 * (i + 1), 4
            yield 0, 4
            return
        t0 = 0
        if self.desc.kind == _lib.KIND["bspline_mscale_HL"]:   # its frozen first stage (tensors 0, 1) comes last
            t0, hidden = 2, max(hidden - 1, 0)
        m2 = self.desc.kind == _lib.KIND["bspline_mscale_2"]
        if m2:                                                  # its combiner (tensors 0 .. 3) comes first
            t0 = 4
            yield 0, t0
        per = (nt - 2 - t0) // (hidden + 1)
        yield nt - 2, 2
        for l in range(hidden, 0, -1):
            yield t0 + per * l, per
        yield t0, per
        if t0 and not m2:
            yield 0, t0

    def _on_grad_ready(self, user, first: int, n: int) -> None:
        """wire_grad_ready_fn: parameter tensors [first, first + n) have their final gradient enqueued on the compute
        stream -> start the all-reduce of their slice of the flat buffer (the loss rides behind the last tensor)."""
        try:
            lo = self.offsets[first]
            hi = self.offsets[first + n] if first + n < len(self.offsets) else self.count + 1
            self.reducers[0].launch_range(lo, hi)
        except BaseException as e:                       # noqa: BLE001 -- must not propagate through the C frame
            self._cb_err = e

    # ------------------------------------------------------------------ buffers
    def _reserve(self, n: int) -> None:
        if n <= self._cap:
            return
        d = C.byref(self.desc)
        self.act_bytes = _lib.check(self.L.wire_act_bytes(d, n, 1))
        self.scr_bytes = _lib.check(self.L.wire_bwd_scratch_bytes(d, n))
        self.act = torch.empty(self.act_bytes, dtype=torch.uint8, device=self.dev)
        self.scratch = torch.empty(self.scr_bytes, dtype=torch.uint8, device=self.dev)
        self.coords = torch.empty(n * self.desc.in_features, dtype=torch.float32, device=self.dev)
        self.y = torch.empty(n * self.O, dtype=torch.float32, device=self.dev)
        self.gy = torch.empty(n * self.O, dtype=torch.float32, device=self.dev)
        self._cap = n

    # ------------------------------------------------------------------ permutations
    def permutation(self, n: Optional[int] = None) -> torch.Tensor:
        """torch.randperm(n) for the next epoch (wire_image_denoise.py:142), generated on a side
        stream while the current step computes: returns the permutation prepared by the previous
        call (made visible to the compute stream) and starts the next one.  Same generator, same
        sequence as calling torch.randperm(n, device=...) in a loop."""
        n = self.npoints if n is None else int(n)
        cur = torch.cuda.current_stream(self.dev)
        if getattr(self, "_perm_stream", None) is None:
            self._perm_stream = torch.cuda.Stream(device=self.dev)
            self._perm_next = None
        if self._perm_next is None or self._perm_next.numel() != n:
            with torch.cuda.stream(self._perm_stream):
                self._perm_next = torch.randperm(n, device=self.dev)
        cur.wait_stream(self._perm_stream)
        out = self._perm_next
        out.record_stream(cur)
        with torch.cuda.stream(self._perm_stream):
            self._perm_next = torch.randperm(n, device=self.dev)
        return out

    # ------------------------------------------------------------------ schedule
    def lr_factor(self) -> float:
        """LambdaLR(lambda x: gamma**min(x/niters, 1)) (wire_image_denoise.py:128)."""
        return self.gamma ** min(self.epoch / self.niters, 1)

    def current_lr(self):
        """The rate of the next step (a list for the per-stage rates of bspline_mscale_hier)."""
        f = self.lr_factor()
        return [r * f for r in self.base_lr] if isinstance(self.base_lr, list) else self.base_lr * f

    def scheduler_step(self) -> None:
        self.epoch += 1

    def _need_target(self, what: str) -> None:
        if self.target is None:
            raise ValueError(f"{what} needs the trainer's target; this trainer was built with target=None")

    # ------------------------------------------------------------------ one step
    def step(self, indices: Optional[torch.Tensor] = None, first: int = 0,
             count: Optional[int] = None) -> torch.Tensor:
        """One optimizer step on a global batch: rows ``indices`` (contiguous int64 device
        tensor of flat grid indices, every rank passes the same one) or the range
        [first, first+count).  Returns the (device-resident, all-reduced) batch loss; no host sync."""
        self._need_target("step")
        if indices is not None:
            if indices.dtype != torch.int64 or not indices.is_cuda or indices.dim() != 1:
                raise ValueError("indices must be a 1-D CUDA int64 tensor")
            if not indices.is_contiguous():
                raise ValueError("indices must be contiguous (a strided view such as perm[::2] would be read "
                                 "as its underlying storage); call .contiguous()")
            B = indices.numel()
            if os.environ.get("WIRE_CHECK_INDICES", "0") == "1" and B > 0:
                # opt-in (one host sync): the kernels trust the indices, an out-of-range one reads / writes
                # outside the target and rec buffers
                lo_i, hi_i = int(indices.min()), int(indices.max())
                if lo_i < 0 or hi_i >= self.npoints:
                    raise ValueError(f"indices span [{lo_i}, {hi_i}] outside the grid of {self.npoints} points")
        else:
            B = int(count if count is not None else self.npoints - first)
            if first < 0 or first + B > self.npoints:
                raise ValueError(f"rows [{first}, {first + B}) outside the grid of {self.npoints} points")
        lo, hi = shard_bounds(B, self.world, self.rank)
        idx_ptr = (indices.data_ptr() + 8 * lo) if indices is not None else None
        return self._step_local(idx_ptr, first + lo, hi - lo, B)

    def step_hashed(self, seed: int, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """One optimizer step on positions [first, first+count) of the epoch's shuffle ``pi_seed`` -- the
        reference's ``indices = torch.randperm(H*W); b_indices = indices[b_idx:b_idx+maxpoints]``
        (wire_image_denoise.py:142-146, wire_occupancy.py:137-142) with the permutation evaluated per position on
        the device (wire_perm_indices): this rank generates only ITS shard of the batch, so the cost of the
        shuffle does not grow with the world size or with the grid (512^3: no 1 GB index vector).  ``seed`` is
        the epoch counter; every rank passes the same (seed, first, count).  No host sync."""
        self._need_target("step_hashed")
        B = int(count if count is not None else self.npoints - first)
        if first < 0 or first + B > self.npoints:
            raise ValueError(f"positions [{first}, {first + B}) outside the epoch of {self.npoints} points")
        lo, hi = shard_bounds(B, self.world, self.rank)
        nloc = hi - lo
        hidx = self._buf("_hidx", max(nloc, 1), torch.int64)
        _lib.check(self.L.wire_perm_indices(self._stream(), int(seed) & 0xFFFFFFFFFFFFFFFF, self.npoints, first + lo,
                                            nloc, hidx.data_ptr()), "perm_indices")
        return self._step_local(hidx.data_ptr(), 0, nloc, B)

    def _step_local(self, idx_ptr: Optional[int], first: int, nloc: int, B: int) -> torch.Tensor:
        """This rank's shard of a global batch of B rows: ``nloc`` rows whose flat grid indices are the int64
        device array at ``idx_ptr`` (or the range starting at ``first`` when None)."""
        L, d = self.L, C.byref(self.desc)
        stream = self._stream()
        self._pack(stream)
        per = (nloc + self.micro - 1) // self.micro
        self._reserve(max(per, 1))
        for m in range(self.micro):
            mlo = m * per
            n = max(0, min(nloc, mlo + per) - mlo)
            g = self.gbuf[m]
            if n == 0:
                g.zero_()
                if self.overlap:                         # the same slices in the same order as the ranks that have rows
                    for t0, nt in self._ready_order():
                        self._on_grad_ready(None, t0, nt)
                    if self._cb_err is not None:
                        raise self._cb_err
                    continue
            else:
                ip = (idx_ptr + 8 * mlo) if idx_ptr is not None else None
                self._grid_coords(stream, first + mlo, n, self.coords, ip)
                args = (stream, d, self.packed.data_ptr(), self.coords.data_ptr(), n, self.target.data_ptr(),
                        ip, first + mlo, n / float(B), self.y.data_ptr(), self.gy.data_ptr(),
                        self._loss_slot(g)[0],
                        self.rec.data_ptr() if self.rec is not None else None, self.partial.data_ptr(),
                        self.act.data_ptr(), self.act_bytes, self.scratch.data_ptr(), self.scr_bytes,
                        self.grad_ptrs[m])
                if self.overlap:
                    self._cb_err = None
                    _lib.check(L.wire_train_fwd_bwd_hooked(*args, self._ready_cb, None), "train_fwd_bwd")
                    if self._cb_err is not None:
                        raise self._cb_err
                    continue                             # every slice is on its way: wait() below joins the streams
                _lib.check(L.wire_train_fwd_bwd(*args), "train_fwd_bwd")
            self.reducers[m].launch()
        for r in self.reducers:
            r.wait()
        gsum = self.gbuf[0]
        for m in range(1, self.micro):
            gsum.add_(self.gbuf[m])
        self._finish(stream, gsum, self._loss_slot(gsum)[1])
        if self.check_every and self.world > 1 and self.t % self.check_every == 0:
            if not replicas_identical(self.flat, self.group):
                raise RuntimeError(f"data-parallel replicas diverged at optimizer step {self.t} (WIRE_DP_CHECK)")
        return self.loss

    # ------------------------------------------------------------------ the step skeleton
    # An operator step checks its arguments, then names its loss: a callable loss(stream, g) that reads self.y, writes
    # dL/dy to self.gy and a device loss (into the slot behind g, or into a buffer of its own).
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _buf(self, name: str, numel: int, dtype=torch.float32, zero: bool = False, exact: bool = False) -> torch.Tensor:
        """The lazily made device buffer ``self.<name>`` of at least ``numel`` elements (``exact``: of exactly that
        many), zero-filled when it is made if ``zero``; it only grows."""
        b = getattr(self, name, None)
        if b is None or (b.numel() != numel if exact else b.numel() < numel):
            b = (torch.zeros if zero else torch.empty)(numel, dtype=dtype, device=self.dev)
            setattr(self, name, b)
        return b

    def _pack(self, stream) -> None:
        _lib.check(self.L.wire_pack_params(stream, C.byref(self.desc), self.param_ptrs, self.packed.data_ptr()), "pack")

    def _grid_coords(self, stream, first: int, n: int, out: torch.Tensor, idx_ptr: Optional[int] = None) -> None:
        """The coordinates of grid rows [first, first + n), or of the n flat indices at ``idx_ptr``, into ``out``."""
        _lib.check(self.L.wire_coords_from_index(stream, idx_ptr, first, n, self.tx.data_ptr(), self.grid[1],
                                                 self.ty.data_ptr(), self.grid[0],
                                                 self.tz.data_ptr() if self.tz is not None else None,
                                                 self.grid[2] if self.tz is not None else 1, out.data_ptr()), "coords")

    def _loss_slot(self, g: torch.Tensor):
        """(pointer to, view of) the float behind the last gradient of the flat buffer ``g``; made once per buffer (the
        view keeps the storage, so its address stays this buffer's)."""
        slots = self.__dict__.setdefault("_slots", {})
        key = g.data_ptr()
        if key not in slots:
            slots[key] = (key + 4 * self.count, g[self.count:self.count + 1])
        return slots[key]

    def _fwd_loss_bwd(self, stream, coords_ptr: int, n: int, loss, g: torch.Tensor, gp, prior=None,
                      coords_grad: bool = False, gy_ptr: Optional[int] = None) -> torch.Tensor:
        """Forward of the ``n`` rows at ``coords_ptr`` into ``self.y``, ``loss(stream, g)``, the TV prior
        ``(H, W, T, lam_s, lam_t)`` on top of it when one of its weights is nonzero, and the backward into the
        gradient buffer ``g`` (``gp``: its pointer array; ``coords_grad``: also dL/dcoords into ``self.g_coords``).
        ``loss=None`` with ``gy_ptr``: the rows' dL/dy exists already, at that address (a range of a full-grid buffer),
        and the backward reads it there instead of ``self.gy``.
        Returns the view that holds the step's loss: ``tv_parts[0:1]`` with a prior, else the slot behind ``g``."""
        L, d = self.L, C.byref(self.desc)
        _lib.check(L.wire_mlp_fwd(stream, d, self.packed.data_ptr(), coords_ptr, n, self.y.data_ptr(),
                                  self.act.data_ptr(), self.act_bytes, 1), "fwd")
        if loss is not None:
            loss(stream, g)
        if gy_ptr is None:
            gy_ptr = self.gy.data_ptr()
        slot, src = self._loss_slot(g)
        if prior is not None and (prior[3] != 0.0 or prior[4] != 0.0):
            self._tv_add_grad(stream, *prior, slot)
            src = self.tv_parts[0:1]
        if coords_grad:
            _lib.check(L.wire_mlp_bwd_coords(stream, d, self.packed.data_ptr(), coords_ptr, n, gy_ptr,
                                             self.act.data_ptr(), self.act_bytes, self.coords_scratch.data_ptr(),
                                             self.coords_scr_bytes, gp, self.g_coords.data_ptr()), "bwd_coords")
        else:
            _lib.check(L.wire_mlp_bwd(stream, d, self.packed.data_ptr(), coords_ptr, n, gy_ptr,
                                      self.act.data_ptr(), self.act_bytes, self.scratch.data_ptr(), self.scr_bytes, gp),
                       "bwd")
        return src

    def _finish(self, stream, g: torch.Tensor, loss_src: torch.Tensor) -> torch.Tensor:
        """Adam on the gradient in ``g``; the step's loss is a copy of ``loss_src``, which the next step overwrites."""
        self.t += 1
        self._adam(stream, g)
        self.loss = loss_src.clone()
        return self.loss

    def _raster_step(self, loss, prior=None, loss_src: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A whole step over the 2-D grid in raster order: pack, coordinates, ``_fwd_loss_bwd``, ``_finish``.  The
        loss is read from ``loss_src`` when the step's loss kernel keeps it in a buffer of its own."""
        n = int(self.grid[0]) * int(self.grid[1])
        stream = self._stream()
        self._reserve(n)
        g = self.gbuf[0]
        self._pack(stream)
        self._grid_coords(stream, 0, n, self.coords)
        src = self._fwd_loss_bwd(stream, self.coords.data_ptr(), n, loss, g, self.grad_ptrs[0], prior)
        return self._finish(stream, g, src if loss_src is None else loss_src)

    # ---- argument checks: they read grid, world, O, tz and target alone, and come before the first device access
    def _need_grid(self, what: str, rank: int = 2, one_output: bool = False, single_process: bool = True) -> None:
        needs = ("a 3-D grid (H, W, T)" if rank == 3 else "a 2-D grid") + \
            (" and out_features == 1" if one_output else "")
        if (self.tz is None) == (rank == 3) or len(self.grid) != rank or (one_output and self.O != 1):
            raise ValueError(f"{what} needs {needs}")
        if single_process and self.world != 1:
            raise NotImplementedError(f"{what} is single-process")

    @staticmethod
    def _rows_arg(indices, first, count, n: int):
        """The rows of ``step_tv`` / ``step_ssim`` -> (indices, first, B): ``indices`` or the range [first, first+B)."""
        if indices is not None:
            if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64 or not indices.is_cuda \
                    or indices.dim() != 1 or not indices.is_contiguous():
                raise ValueError("indices must be a 1-D contiguous CUDA int64 tensor")
            B = indices.numel()
            if B > n:
                raise ValueError(f"{B} indices for a grid of {n} points: the rows of indices must be distinct")
            return indices, 0, B
        first = int(first)
        B = int(count if count is not None else n - first)
        if first < 0 or B < 0 or first + B > n:
            raise ValueError(f"rows [{first}, {first + B}) outside the grid of {n} points")
        return None, first, B

    @staticmethod
    def _scale_arg(scale, H: int, W: int) -> int:
        scale = int(scale)
        if scale < 1 or scale > min(H, W):
            raise ValueError(f"scale {scale} outside 1..min(H, W)")
        return scale

    @staticmethod
    def _f32_elems(name: str, t, *dims: int) -> torch.Tensor:
        """``t`` as a detached contiguous tensor, if it is CUDA float32 of dims[0] x dims[1] ... elements."""
        numel = 1
        for v in dims:
            numel *= v
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.numel() != numel:
            raise ValueError(f"{name} must be a CUDA float32 tensor of {' x '.join(str(v) for v in dims)} elements")
        return t.detach().contiguous()

    @staticmethod
    def _f32_like(name: str, t, like: torch.Tensor, like_name: str) -> None:
        """An optional output ``t``: contiguous CUDA float32 with the elements of ``like``."""
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.numel() != like.numel()
                              or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous CUDA float32 tensor shaped like {like_name}")

    @staticmethod
    def _opt_ptr(t: Optional[torch.Tensor]) -> Optional[int]:
        return t.data_ptr() if t is not None else None

    # ------------------------------------------------------------------ the TV prior of the operator steps
    @staticmethod
    def _tv_weight(name: str, value) -> float:
        lam = float(value)
        if not np.isfinite(lam):
            raise ValueError(f"{name} must be finite, not {lam}")
        return lam

    def _tv_add_grad(self, stream, H: int, W: int, T: int, lam_s: float, lam_t: float, data_loss: int,
                     y: Optional[torch.Tensor] = None, gy: Optional[torch.Tensor] = None) -> None:
        """The TV term of the (H, W, T) grid in ``self.y``, added to the ``self.gy`` the operator's backward has left
        (wire_tv_add_grad); ``self.tv_parts`` receives [loss, data, tv_s, tv_t], data being the device scalar at
        ``data_loss``.  ``y`` / ``gy``: full-grid buffers that stand in for ``self.y`` / ``self.gy``."""
        tv_parts = self._buf("tv_parts", 4, zero=True)
        y, gy = self.y if y is None else y, self.gy if gy is None else gy
        _lib.check(self.L.wire_tv_add_grad(stream, y.data_ptr(), H, W, T, self.O, lam_s, lam_t, data_loss,
                                           gy.data_ptr(), tv_parts.data_ptr(), self.partial.data_ptr()),
                   "tv_add_grad")

    # ------------------------------------------------------------------ super-resolution step
    def step_downsampled(self, gt_lr: torch.Tensor, scale: int,
                         rec_lr: Optional[torch.Tensor] = None, lambda_tv: float = 0.0) -> torch.Tensor:
        """One optimizer step of the super-resolution loop (wire_SISR.py:151-178): the model is
        evaluated on the WHOLE high-resolution grid in raster order, ``torch.nn.AvgPool2d(scale)``
        brings the reconstruction to the resolution of ``gt_lr`` ([H//scale * W//scale, O], device
        float32), loss = mean squared error there; backward through the pooling and the network,
        Adam.  The high-resolution reconstruction of this step stays in ``self.y`` ([H*W, O]).
        ``lambda_tv`` != 0 adds ``lambda_tv * utils.total_variation_loss`` of the high-resolution reconstruction
        (bspline_SISR.py's ``lambda_tv``) to the loss and its gradient to dL/dy (wire_tv_add_grad, between the pooled
        loss and the backward); the returned loss is the total and ``self.tv_parts`` holds [loss, mse, tv, 0].  With
        0.0 that kernel is not launched and the step is the plain one, bit for bit.
        2-D grids, single process (a pooled window must not straddle two shards)."""
        self._need_grid("step_downsampled")
        lam = self._tv_weight("lambda_tv", lambda_tv)
        H, W = int(self.grid[0]), int(self.grid[1])
        scale = self._scale_arg(scale, H, W)
        gt = self._f32_elems("gt_lr", gt_lr, (H // scale) * (W // scale), self.O)
        self._f32_like("rec_lr", rec_lr, gt, "gt_lr")

        def loss(stream, g):
            _lib.check(self.L.wire_avgpool_mse_grad(stream, self.y.data_ptr(), H, W, self.O, scale, gt.data_ptr(),
                                                    self.gy.data_ptr(), self._opt_ptr(rec_lr), self._loss_slot(g)[0],
                                                    self.partial.data_ptr()), "avgpool_mse_grad")
        return self._raster_step(loss, prior=(H, W, 1, lam, 0.0))

    def step_resized(self, gt_lr: torch.Tensor, size, interpolation="area", rec_lr: Optional[torch.Tensor] = None,
                     lambda_tv: float = 0.0) -> torch.Tensor:
        """``step_downsampled`` under any of ``cv2.resize``'s degradations: the model is evaluated on the WHOLE
        high-resolution grid in raster order, ``functional.resize`` with ``interpolation`` ("nearest", "linear",
        "cubic", "area" or cv2's integer) brings the reconstruction to ``size = (Hl, Wl)``, the resolution of ``gt_lr``
        ([Hl*Wl, O], device float32), at the scale ``n_in / n_out`` per axis -- a non-integer factor and sides that the
        factor does not divide are fine -- and loss = mean squared error there; backward through the operator's exact
        adjoint (wire_resize_mse_grad: a gather, no atomics) and the network, Adam.  ``area`` needs
        ``Hl <= H and Wl <= W`` (ValueError otherwise: cv2's INTER_AREA up-scaling is not provided).  The operator
        follows cv2's documented formulas and has not been measured against cv2; its non-integer ``area`` keeps the
        partial overlaps below 1e-3 that cv2 drops without renormalising.
        The high-resolution reconstruction of this step stays in ``self.y`` ([H*W, O]); ``rec_lr`` (optional) receives
        the resized one.  ``lambda_tv`` as in ``step_downsampled``: != 0 adds ``lambda_tv *
        utils.total_variation_loss`` of the high-resolution reconstruction, the returned loss is the total and
        ``self.tv_parts`` holds [loss, mse, tv, 0]; with 0.0 that kernel is not launched.  The tables and the workspace
        are made once per (size, interpolation) and reused.
        2-D grids, single process (an output's taps must not straddle two shards)."""
        self._need_grid("step_resized")
        lam = self._tv_weight("lambda_tv", lambda_tv)
        H, W = int(self.grid[0]), int(self.grid[1])
        if len(size) != 2:
            raise ValueError("size must be (Hl, Wl)")
        Hl, Wl = int(size[0]), int(size[1])
        geom = functional.resize_geometry(H, W, (Wl, Hl), None, None, interpolation)
        gt = self._f32_elems("gt_lr", gt_lr, Hl * Wl, self.O)
        self._f32_like("rec_lr", rec_lr, gt, "gt_lr")
        name = f"_resize_tab_{Hl}x{Wl}_{geom[4]}"                         # one table per (size, interpolation), kept
        if getattr(self, name, None) is None:
            nb = _lib.check(self.L.wire_resize_tab_bytes(*geom), "wire_resize_tab_bytes")
            try:
                _lib.check(self.L.wire_resize_tables(self._stream(), *geom,
                                                     self._buf(name, nb, torch.uint8).data_ptr()), "resize_tables")
            except Exception:
                self.__dict__.pop(name, None)                                # never keep a table that was not written
                raise
        tab = getattr(self, name)
        wsb = _lib.check(self.L.wire_resize_mse_grad_ws_bytes(Hl, Wl, self.O), "wire_resize_mse_grad_ws_bytes")
        ws = self._buf("_resize_ws", wsb, torch.uint8)

        def loss(stream, g):
            _lib.check(self.L.wire_resize_mse_grad(stream, tab.data_ptr(), *geom, self.y.data_ptr(), self.O,
                                                   gt.data_ptr(), self.gy.data_ptr(), self._opt_ptr(rec_lr),
                                                   self._loss_slot(g)[0], ws.data_ptr(), ws.numel(),
                                                   self.partial.data_ptr()), "resize_mse_grad")
        return self._raster_step(loss, prior=(H, W, 1, lam, 0.0))

    # ------------------------------------------------------------------ total-variation regularised step
    def step_tv(self, lambda_tv: float, indices: Optional[torch.Tensor] = None, first: int = 0,
                count: Optional[int] = None) -> torch.Tensor:
        """One optimizer step of the TV-regularised image loop (bspline_image_denoise.py:160-172,
        bspline_img_representation.py:147-158): the model is evaluated on the WHOLE 2-D grid in raster order and

            loss = mse + lambda_tv * utils.total_variation_loss(model(coords).reshape(1, H, W, O).permute(0, 3, 1, 2))

        with the mean squared error against ``self.target`` on the rows ``indices`` (contiguous int64 device tensor of
        DISTINCT flat grid indices, such as a slice of a permutation) or the range [first, first+count) -- given exactly
        as ``step`` takes them, all rows by default -- and the total variation (a sum, not a mean) of the full
        reconstruction.  Loss and its gradient come from one fused kernel (wire_tv_mse_grad); backward through the
        network, Adam.  The reference's drivers evaluate the TV term under ``torch.no_grad()``, where it changes the
        reported loss and no gradient; here it acts on the weights, which is what their ``tvl`` switch was written for.
        ``step_tv(0.0)`` on all rows is the plain full-grid MSE step.

        Returns the device loss (no host sync); ``self.loss_parts`` holds [loss, mse, tv], the full reconstruction of
        the step stays in ``self.y`` ([H*W, O]), and with ``keep_rec`` the selected rows go to ``self.rec``.
        2-D grids, single process (a neighbour pair must not straddle two shards)."""
        self._need_grid("step_tv")
        self._need_target("step_tv")
        lam = self._tv_weight("lambda_tv", lambda_tv)
        H, W = int(self.grid[0]), int(self.grid[1])
        indices, first, B = self._rows_arg(indices, first, count, H * W)
        parts = self._buf("loss_parts", 3, zero=True)

        def loss(stream, g):
            _lib.check(self.L.wire_tv_mse_grad(stream, self.y.data_ptr(), H, W, self.O, self.target.data_ptr(),
                                               self._opt_ptr(indices), first, B, lam, self.gy.data_ptr(),
                                               parts.data_ptr(), self._opt_ptr(self.rec), self.partial.data_ptr()),
                       "tv_mse_grad")
        return self._raster_step(loss, loss_src=parts[0:1])

    # ------------------------------------------------------------------ SSIM-regularised step
    def step_ssim(self, lambda_ssim: float, indices: Optional[torch.Tensor] = None, first: int = 0,
                  count: Optional[int] = None, window="gaussian", data_range=None) -> torch.Tensor:
        """One optimizer step of an image loop with the perceptual term: the model is evaluated on the WHOLE 2-D grid in
        raster order and

            loss = mse + lambda_ssim * (1 - ssim(model(coords), target))

        with the mean squared error against ``self.target`` on the rows ``indices`` or the range [first, first+count)
        -- given exactly as ``step_tv`` takes them, all rows by default -- and the structural similarity
        (``functional.ssim``: ``window`` and ``data_range`` as there) of the full reconstruction against the full
        target.  Loss and its gradient come from one fused kernel (wire_ssim_mse_grad); backward through the network,
        Adam.  With ``lambda_ssim == 0.0`` the index is not evaluated: the step leaves the parameters that
        ``step_tv(0.0)`` leaves, and ``loss_parts[2]`` is 0.

        Returns the device loss (no host sync); ``self.loss_parts`` holds [loss, mse, ssim], the full reconstruction of
        the step stays in ``self.y`` ([H*W, O]), and with ``keep_rec`` the selected rows go to ``self.rec``.
        2-D grids, single process (a window must not straddle two shards)."""
        self._need_grid("step_ssim")
        self._need_target("step_ssim")
        lam = self._tv_weight("lambda_ssim", lambda_ssim)
        H, W = int(self.grid[0]), int(self.grid[1])
        taps, win, cov = functional._ssim_window(window)
        if data_range is None:
            if window == "uniform" or (isinstance(window, tuple) and window[1] is None):
                raise ValueError("a uniform window needs data_range (see functional.ssim)")
            data_range = 1.0
        if H < taps or W < taps:
            raise ValueError(f"a {H} x {W} grid is smaller than the {taps}-tap window")
        if not 1 <= self.O <= 8:
            raise ValueError(f"{self.O} channels: the library takes 1..8")
        indices, first, B = self._rows_arg(indices, first, count, H * W)
        parts = self._buf("loss_parts", 3, zero=True)
        ws = self._buf("_ssim_loss_ws", _lib.check(self.L.wire_ssim_mse_grad_ws_bytes(H, W, self.O, taps),
                                                   "ssim_mse_grad_ws_bytes"), torch.uint8)
        c1, c2 = (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2

        def loss(stream, g):
            _lib.check(self.L.wire_ssim_mse_grad(stream, self.y.data_ptr(), H, W, self.O, self.target.data_ptr(), taps,
                                                 win, cov, c1, c2, self._opt_ptr(indices), first, B, lam,
                                                 self.gy.data_ptr(), parts.data_ptr(), self._opt_ptr(self.rec),
                                                 ws.data_ptr(), ws.numel()), "ssim_mse_grad")
        return self._raster_step(loss, loss_src=parts[0:1])

    # ------------------------------------------------------------------ steps that choose their data term
    def _point_loss(self, code: int, delta: float, table: torch.Tensor, w: Optional[torch.Tensor], wpe: int,
                    idx_ptr: Optional[int], first: int, n: int, rec: Optional[torch.Tensor]):
        """The pointwise loss of ``n`` rows of ``self.y`` against the rows of ``table`` (and of the weight table ``w``)
        that ``idx_ptr`` / ``first`` name (wire_point_loss_grad)."""
        def loss(stream, g):
            _lib.check(self.L.wire_point_loss_grad(stream, code, delta, self.y.data_ptr(), table.data_ptr(),
                                                   self._opt_ptr(w), wpe, idx_ptr, first, n, self.O, 1.0,
                                                   self.gy.data_ptr(), self._loss_slot(g)[0], self._opt_ptr(rec),
                                                   self.partial.data_ptr()), "point_loss_grad")
        return loss

    def _point_step(self, coords_ptr: int, n: int, loss) -> torch.Tensor:
        """Pack, ``_fwd_loss_bwd`` on the ``n`` rows at ``coords_ptr``, ``_finish``."""
        stream = self._stream()
        g = self.gbuf[0]
        self._pack(stream)
        src = self._fwd_loss_bwd(stream, coords_ptr, n, loss, g, self.grad_ptrs[0])
        return self._finish(stream, g, src)

    def step_loss(self, kind: str, indices: Optional[torch.Tensor] = None, first: int = 0,
                  count: Optional[int] = None, weight: Optional[torch.Tensor] = None,
                  delta: float = 1.0) -> torch.Tensor:
        """``step`` with a chosen data term and an optional per-sample weight: the rows ``indices`` (contiguous int64
        device tensor of DISTINCT flat grid indices, such as a slice of a permutation) or the range
        [first, first+count) -- given exactly as ``step`` takes them, all rows by default -- are evaluated, and only
        those, and

            loss = sum_e w_e rho(y_e - target_e) / (rows * O)

        with rho by ``kind``: "mse", "l1" (impulse noise: ``utils.add_salt_and_pepper_noise``), "huber" (quadratic up to
        ``delta``, linear beyond) or "logistic" (the output is a logit and the target a probability in [0, 1]: the
        occupancy loop; ``functional.point_loss`` lists the formulas).  ``weight`` is a full-grid table [npoints] or
        [npoints, O] of any finite values, gathered by the same rows -- ``utils.get_inpainting_mask`` flattened, or a
        per-channel mosaic; the mean runs over every evaluated element, those of weight 0 included.  Loss and gradient
        come from one kernel (wire_point_loss_grad); backward through the network, Adam.  ``step_loss("mse")`` without
        a weight leaves the parameters that ``step_tv(0.0)`` leaves on the same rows.

        Returns the device loss (no host sync); the rows' outputs stay in ``self.y[:rows*O]`` and with ``keep_rec`` go
        to ``self.rec``.  Any grid, single process."""
        if self.world != 1:
            raise NotImplementedError("step_loss is single-process")
        code, delta = functional._loss_kind(kind, delta)
        self._need_target("step_loss")
        indices, first, B = self._rows_arg(indices, first, count, self.npoints)
        if B < 1:
            raise ValueError("step_loss needs at least one row")
        w, wpe = functional._loss_weight(weight, self.npoints, self.O, self.target, rows="npoints")
        self._reserve(B)
        ip = self._opt_ptr(indices)
        self._grid_coords(self._stream(), first, B, self.coords, ip)
        return self._point_step(self.coords.data_ptr(), B,
                                self._point_loss(code, delta, self.target, w, wpe, ip, first, B, self.rec))

    def step_samples(self, coords: torch.Tensor, values: torch.Tensor, kind: str = "mse",
                     weight: Optional[torch.Tensor] = None, delta: float = 1.0) -> torch.Tensor:
        """One optimizer step on scattered samples: ``coords`` [n, in_features] may lie anywhere -- jittered grid
        points, surface samples of a point cloud, the registered low-resolution pixels of a multi-image loop -- and are
        read where they are (no copy, no grid lookup); ``values`` [n, O] are their targets, ``weight`` None, [n] or
        [n, O]; all contiguous CUDA float32, n >= 1, and n may change from call to call.  The data term is ``kind``
        with ``delta``, as in ``step_loss``.  The trainer's grid and target are not used, so a trainer built with
        ``target=None`` serves.  Returns the device loss (no host sync); the outputs of the step stay in
        ``self.y[:n*O]``.  Single process."""
        if self.world != 1:
            raise NotImplementedError("step_samples is single-process")
        code, delta = functional._loss_kind(kind, delta)
        D = int(self.desc.in_features)
        if not isinstance(coords, torch.Tensor) or coords.dtype != torch.float32 or coords.dim() != 2 \
                or coords.shape[0] < 1 or coords.shape[1] != D or not coords.is_contiguous() or not coords.is_cuda:
            raise ValueError(f"coords must be a contiguous CUDA float32 tensor [n, {D}] with n >= 1")
        n = int(coords.shape[0])
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or tuple(values.shape) != (n, self.O) \
                or not values.is_contiguous() or values.device != coords.device:
            raise ValueError(f"values must be a contiguous float32 tensor [{n}, {self.O}] on the device of coords")
        w, wpe = functional._loss_weight(weight, n, self.O, coords)
        xy, tab = coords.detach(), values.detach()
        self._reserve(n)
        return self._point_step(xy.data_ptr(), n, self._point_loss(code, delta, tab, w, wpe, None, 0, n, None))

    # ------------------------------------------------------------------ volume rendering: a net seen through camera rays
    def _rays_args(self, what: str, rays, near, far, n_samples, jitter, background, density):
        """The argument checks of the ray entry points -> (functional._ray_args' tuple, background, density mode)."""
        if self.world != 1:
            raise NotImplementedError(f"{what} is single-process")
        if int(self.desc.in_features) != 3 or not 2 <= self.O <= 8:
            raise ValueError(f"{what} needs in_features == 3 and out_features == C + 1 in 2..8 (C colours and a density)")
        mode = functional._density_mode(density)
        args = functional._ray_args(rays, near, far, n_samples, jitter)
        if args[0].device != self.dev:
            raise ValueError("rays must be on the trainer's device")
        return args, functional._background_arg(background, self.O - 1, self.dev), mode

    def _reserve_rays(self, n: int) -> None:
        """ts and deltas of n samples, beside the buffers of ``_reserve``."""
        self._reserve(n)
        if n > getattr(self, "_ray_cap", 0):
            self.ray_ts = torch.empty(n, dtype=torch.float32, device=self.dev)
            self.ray_deltas = torch.empty(n, dtype=torch.float32, device=self.dev)
            self._ray_cap = n

    def step_rays(self, rays: torch.Tensor, target: torch.Tensor, near, far, n_samples: int, jitter=None,
                  background=None, density: str = "softplus", n_importance: int = 0,
                  jitter_fine=None) -> torch.Tensor:
        """One optimizer step of a radiance field: the net maps a point of space to ``(c_raw[0..C), s_raw)`` and is seen
        only through the colours of R camera rays.  ``rays`` [R, 6] (``utils.get_rays``), ``near`` / ``far`` two numbers
        or two [R] tensors (``utils.ray_box``), ``n_samples`` = S stratified samples per ray with ``jitter`` [R, S]
        (``torch.rand``) or midpoints, as ``functional.ray_samples``; ``target`` [R, C] the rays' colours;
        ``background`` and ``density`` as ``functional.composite``.

            loss = mean((composite(net(o + t_s d)) - target)^2)

        Launches: pack, wire_ray_samples into ``self.coords``, the forward of R*S rows, wire_composite_mse_grad (forward
        sweep, loss and adjoint in one kernel, dL/dy into ``self.gy``), the backward, Adam.  Returns the device loss (no
        host sync); the rendered colours of the step stay in ``self.ray_rgb`` [R, C], the net's rows in ``self.y``.
        R and S may change from call to call.  The trainer's grid and target are not used (``target=None`` serves).
        Needs ``in_features == 3`` and ``out_features == C + 1``; single process; no TV prior; no gradient to the rays.

        ``n_importance`` = Nf > 0 makes the step hierarchical: a coarse pass tells a second pass
        where to look.  Launches: pack, wire_ray_samples into coarse buffers of their own, a forward-only pass of the R*S
        coarse rows with no saved activations, wire_composite_weights into ``self.ray_w`` [R, S], wire_ray_resample
        (``functional.ray_resample``; ``jitter_fine`` [R, Nf] or midpoints of the strata) into ``self.coords`` /
        ``self.ray_ts`` / ``self.ray_deltas`` with S + Nf sorted samples per ray, then the step above on those
        R*(S+Nf) rows.  ONE net serves both passes.  The loss is on the second pass only, whose samples include the
        coarse ones; the coarse pass carries no gradient, and no gradient flows through the sample positions.  S and Nf
        up to 1024 each; R, S and Nf may change from call to call; still no host sync.  ``n_importance=0`` is the step
        without the argument, launch for launch."""
        (r, bounds, nr, fr, R, S, u), bg, mode = self._rays_args("step_rays", rays, near, far, n_samples, jitter,
                                                                 background, density)
        tgt = self._f32_elems("target", target, R, self.O - 1)
        Nf = int(n_importance)
        if Nf < 0:
            raise ValueError("n_importance must be >= 0")
        if Nf > 0:
            return self._step_rays_hier(r, bounds, nr, fr, R, S, u, Nf, jitter_fine, tgt, bg, mode)
        if jitter_fine is not None:
            raise ValueError("jitter_fine needs n_importance > 0")
        n = R * S
        self._reserve_rays(n)
        self.ray_rgb = torch.empty(R, self.O - 1, dtype=torch.float32, device=self.dev)
        functional._ray_samples_into(self._stream(), r, bounds, nr, fr, u, R, S, self.coords, self.ray_ts,
                                     self.ray_deltas)
        return self._point_step(self.coords.data_ptr(), n, self._composite_loss(tgt, bg, R, S, mode))

    def _composite_loss(self, tgt, bg, R: int, S: int, mode: int):
        """The loss callable of the ray steps: wire_composite_mse_grad on ``self.y`` with S samples per ray."""
        def loss(stream, g):
            _lib.check(self.L.wire_composite_mse_grad(stream, self.y.data_ptr(), self.ray_ts.data_ptr(),
                                                      self.ray_deltas.data_ptr(), self._opt_ptr(bg), tgt.data_ptr(), R,
                                                      S, self.O, mode, 1.0, self.gy.data_ptr(), self._loss_slot(g)[0],
                                                      self.ray_rgb.data_ptr(), self.partial.data_ptr()),
                       "composite_mse_grad")
        return loss

    def _coarse_pass(self, stream, rays, bounds, nr, fr, jitter, R: int, S: int, mode: int, buf: dict) -> None:
        """wire_ray_samples, a forward-only pass of the R*S rows on the packed parameters and wire_composite_weights,
        all into the buffers of ``buf`` (coords, ts, deltas, y, act, w)."""
        functional._ray_samples_into(stream, rays, bounds, nr, fr, jitter, R, S, buf["coords"], buf["ts"], buf["deltas"])
        _lib.check(self.L.wire_mlp_fwd(stream, C.byref(self.desc), self.packed.data_ptr(), buf["coords"].data_ptr(),
                                       R * S, buf["y"].data_ptr(), buf["act"].data_ptr(), buf["act_bytes"], 0), "fwd")
        functional._composite_weights_into(stream, buf["y"], buf["deltas"], R, S, self.O, mode, buf["w"])

    def _step_rays_hier(self, r, bounds, nr, fr, R: int, S: int, u, Nf: int, jitter_fine, tgt, bg, mode: int):
        """``step_rays`` with ``n_importance`` = Nf > 0; the arguments are checked and detached."""
        eps = functional._resample_args(S, Nf, 1e-5)
        if jitter_fine is not None:
            if not isinstance(jitter_fine, torch.Tensor) or jitter_fine.dtype != torch.float32 \
                    or tuple(jitter_fine.shape) != (R, Nf) or not jitter_fine.is_contiguous() \
                    or jitter_fine.device != self.dev:
                raise ValueError(f"jitter_fine must be a contiguous float32 tensor [{R}, {Nf}] on the trainer's device")
            jitter_fine = jitter_fine.detach()
        nc, M = R * S, S + Nf
        n = R * M
        self._reserve_rays(n)
        self.ray_rgb = torch.empty(R, self.O - 1, dtype=torch.float32, device=self.dev)
        ab = _lib.check(self.L.wire_act_bytes(C.byref(self.desc), nc, 0))
        buf = dict(coords=self._buf("ray_coords_c", nc * 3), ts=self._buf("ray_ts_c", nc),
                   deltas=self._buf("ray_deltas_c", nc), y=self._buf("ray_y_c", nc * self.O),
                   act=self._buf("ray_act_c", max(ab, 16), dtype=torch.uint8), act_bytes=ab,
                   w=self._buf("_ray_w", nc))
        self.ray_w = buf["w"][:nc].view(R, S)
        stream = self._stream()
        g = self.gbuf[0]
        self._pack(stream)
        self._coarse_pass(stream, r, bounds, nr, fr, u, R, S, mode, buf)
        functional._ray_resample_into(stream, r, bounds, nr, fr, buf["ts"], buf["w"], jitter_fine, eps, R, S, Nf,
                                      self.coords, self.ray_ts, self.ray_deltas)
        src = self._fwd_loss_bwd(stream, self.coords.data_ptr(), n, self._composite_loss(tgt, bg, R, M, mode), g,
                                 self.grad_ptrs[0])
        return self._finish(stream, g, src)

    @torch.no_grad()
    def render_rays(self, rays: torch.Tensor, near, far, n_samples: int, tile_rays: int = 4096, background=None,
                    density: str = "softplus", n_importance: int = 0):
        """Forward-only rendering of ``rays`` [R, 6] at midpoint samples, ``tile_rays`` rays at a time with no saved
        activations (as ``render``): ``(rgb [R, C], acc [R], depth [R])``.  The compositing of a ray does not depend on
        the tiling, so the result has the same bits for every ``tile_rays`` that keeps the net's forward on one GEMM
        family (the library picks it by the rows of a call, ``tile_rays * n_samples``, with the switch at 4096 rows).
        ``n_importance`` = Nf > 0 renders hierarchically, as ``step_rays`` trains: per tile a coarse pass at the S
        midpoints, its weights, Nf draws at the midpoints of the strata, and the colours of the S + Nf merged samples
        (two forward calls per tile, of ``tile_rays * S`` and ``tile_rays * (S + Nf)`` rows).  Arguments as
        ``step_rays``."""
        (r, bounds, nr, fr, R, S, _), bg, mode = self._rays_args("render_rays", rays, near, far, n_samples, None,
                                                                 background, density)
        Nf = int(n_importance)
        if Nf < 0:
            raise ValueError("n_importance must be >= 0")
        eps = functional._resample_args(S, Nf, 1e-5) if Nf else 0.0
        tile = max(1, min(int(tile_rays), R))
        L, d = self.L, C.byref(self.desc)
        stream = self._stream()
        Cc, M = self.O - 1, S + Nf
        f32 = dict(dtype=torch.float32, device=self.dev)
        rgb, acc, depth = torch.empty(R, Cc, **f32), torch.empty(R, **f32), torch.empty(R, **f32)
        self._pack(stream)
        ab = _lib.check(L.wire_act_bytes(d, tile * M, 0))
        act = torch.empty(ab, dtype=torch.uint8, device=self.dev)
        coords = torch.empty(tile * M, 3, **f32)
        ts, deltas = torch.empty(tile * M, **f32), torch.empty(tile * M, **f32)
        y = torch.empty(tile * M, self.O, **f32)
        if Nf:
            abc = _lib.check(L.wire_act_bytes(d, tile * S, 0))
            cb = dict(coords=torch.empty(tile * S, 3, **f32), ts=torch.empty(tile * S, **f32),
                      deltas=torch.empty(tile * S, **f32), y=torch.empty(tile * S, self.O, **f32),
                      act=torch.empty(max(abc, 16), dtype=torch.uint8, device=self.dev), act_bytes=abc,
                      w=torch.empty(tile * S, **f32))
        for r0 in range(0, R, tile):
            nr_ = min(tile, R - r0)
            rt, bt = r[r0:r0 + nr_], None if bounds is None else bounds[r0:r0 + nr_]
            if Nf:
                self._coarse_pass(stream, rt, bt, nr, fr, None, nr_, S, mode, cb)
                functional._ray_resample_into(stream, rt, bt, nr, fr, cb["ts"], cb["w"], None, eps, nr_, S, Nf, coords,
                                              ts, deltas)
            else:
                functional._ray_samples_into(stream, rt, bt, nr, fr, None, nr_, S, coords, ts, deltas)
            _lib.check(L.wire_mlp_fwd(stream, d, self.packed.data_ptr(), coords.data_ptr(), nr_ * M, y.data_ptr(),
                                      act.data_ptr(), ab, 0), "fwd")
            _lib.check(L.wire_composite_fwd(stream, y.data_ptr(), ts.data_ptr(), deltas.data_ptr(), self._opt_ptr(bg),
                                            nr_, M, self.O, mode, rgb.data_ptr() + 4 * r0 * Cc,
                                            acc.data_ptr() + 4 * r0, depth.data_ptr() + 4 * r0), "composite_fwd")
        return rgb, acc, depth

    # ------------------------------------------------------------------ multi-image super-resolution step
    def affine_coords(self, mats) -> torch.Tensor:
        """The coordinates of B frames of the trainer's grid, each moved by its 2 x 3 matrix -- ``motion.get_imstack``'s
        ``Xstack`` / ``Ystack`` at scale 1 (modules/motion.py:284-318, wire_multi_sr.py:74-78) as ``ImageSRDataset``
        stacks them -- computed on the device in fp64 (wire_affine_coords): the 2 x 3 matrices are all that crosses the
        bus.  ``mats``: [B, 2, 3] array or tensor.  Returns the contiguous float32 device tensor [B, H*W, 2]."""
        self._need_grid("affine_coords", single_process=False)
        m = torch.as_tensor(mats).detach().to(self.dev, torch.float64)
        if m.dim() != 3 or tuple(m.shape[1:]) != (2, 3) or m.shape[0] < 1:
            raise ValueError("mats must be [B, 2, 3] with B >= 1")
        m = m.contiguous()
        H, W = int(self.grid[0]), int(self.grid[1])
        out = torch.empty(m.shape[0], H * W, 2, dtype=torch.float32, device=self.dev)
        _lib.check(self.L.wire_affine_coords(self._stream(), m.data_ptr(), m.shape[0], H, W, out.data_ptr()), "affine_coords")
        return out

    def _frames_args(self, what: str, coords, gt_lr, scale, mask, rec_lr):
        """The argument checks of the multi-image steps -> (H, W, scale, coords, B, gt_lr, mask), detached and
        contiguous."""
        self._need_grid(what)
        H, W = int(self.grid[0]), int(self.grid[1])
        scale = self._scale_arg(scale, H, W)
        H2, W2 = H // scale, W // scale
        if not isinstance(coords, torch.Tensor) or not coords.is_cuda or coords.dtype != torch.float32 \
                or coords.dim() != 3 or coords.shape[0] < 1 or tuple(coords.shape[1:]) != (H * W, 2) \
                or not coords.is_contiguous():
            raise ValueError(f"coords must be a contiguous CUDA float32 tensor [B, {H * W}, 2]")
        xy = coords.detach()
        B = int(xy.shape[0])
        gt = self._f32_elems("gt_lr", gt_lr, B, H2 * W2, self.O)
        mk = None if mask is None else self._f32_elems("mask", mask, B, H2 * W2, self.O)
        self._f32_like("rec_lr", rec_lr, gt, "gt_lr")
        return H, W, scale, xy, B, gt, mk

    def step_frames(self, coords: torch.Tensor, gt_lr: torch.Tensor, scale: int, mask: Optional[torch.Tensor] = None,
                    rec_lr: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimizer step of the multi-image super-resolution loop (wire_multi_sr.py:190-208) on a batch of B frames:
        ``coords`` [B, H*W, 2] (contiguous device float32; frame f's rows are the trainer's grid moved by that frame's
        motion -- ``affine_coords`` makes them) go through the model in ONE forward of B*H*W rows,
        ``torch.nn.AvgPool2d(scale)`` brings every frame to the resolution of ``gt_lr`` ([B, H//scale * W//scale, O]),
        loss = ``MSELoss()(output*mask, gt_lr*mask)`` (``mask`` shaped like ``gt_lr``, any values; None = ones); backward
        through the pooling and the network, Adam.  ``rec_lr`` (optional, shaped like ``gt_lr``) receives the unmasked
        pooled frames, and the high-resolution frames of this step stay in ``self.y`` ([B*H*W, O]).  B is read from
        ``coords`` and may change from call to call (a last, smaller batch).  2-D grids, single process.
        No TV prior here (``step_downsampled``, ``step_radon`` and ``step_coded`` take one): the frames are warped
        copies, and a prior belongs on the canonical grid, which this step never evaluates."""
        H, W, scale, xy, B, gt, mk = self._frames_args("step_frames", coords, gt_lr, scale, mask, rec_lr)
        stream = self._stream()
        n = B * H * W
        self._reserve(n)
        g = self.gbuf[0]
        self._pack(stream)
        src = self._fwd_loss_bwd(stream, xy.data_ptr(), n, self._frames_loss(B, H, W, scale, gt, mk, rec_lr), g,
                                 self.grad_ptrs[0])
        return self._finish(stream, g, src)

    def _frames_loss(self, B: int, H: int, W: int, scale: int, gt, mk, rec_lr):
        """The masked, pooled loss of the multi-image steps."""
        def loss(stream, g):
            _lib.check(self.L.wire_avgpool_mse_grad_frames(stream, self.y.data_ptr(), B, H, W, self.O, scale,
                                                           gt.data_ptr(), self._opt_ptr(mk), self.gy.data_ptr(),
                                                           self._opt_ptr(rec_lr), self._loss_slot(g)[0],
                                                           self.partial.data_ptr()), "avgpool_mse_grad_frames")
        return loss

    # ------------------------------------------------------------------ multi-image step with a learnable registration
    def registration(self, B: int, lr: float = 1e-4, pin_first: bool = True, theta=None) -> "FrameRegistration":
        """The registration state of B frames on the trainer's device, for ``step_frames_registered``: one 2 x 3 matrix
        per frame in normalised coordinates, the identity unless ``theta`` ([B, 2, 3]) is given, with its own Adam
        state and rate ``lr``.  ``pin_first`` keeps frame 0 where it is (the gauge).  2-D grids."""
        self._need_grid("registration", single_process=False)
        return FrameRegistration(B, self.dev, lr=lr, pin_first=pin_first, theta=theta)

    def _reserve_registered(self, n: int, B: int) -> None:
        """The buffers only the registered step needs: dL/dcoords of n rows, the scratch of the backward that computes it
        (wire_bwd_coords_scratch_bytes >= wire_bwd_scratch_bytes) and the workspace of the reduction to B frames."""
        if n > getattr(self, "_reg_cap", 0):
            self.coords_scr_bytes = _lib.check(self.L.wire_bwd_coords_scratch_bytes(C.byref(self.desc), n))
            self.coords_scratch = torch.empty(self.coords_scr_bytes, dtype=torch.uint8, device=self.dev)
            self.g_coords = torch.empty(n, 2, dtype=torch.float32, device=self.dev)
            self._reg_cap = n
        # (frames of one grid: the workspace grows with B alone)
        self._buf("warp_ws", _lib.check(self.L.wire_warp_coords_bwd_ws_bytes(B, n // B), "warp_coords_bwd_ws_bytes"),
                  torch.uint8)

    def step_frames_registered(self, reg: "FrameRegistration", coords: torch.Tensor, gt_lr: torch.Tensor, scale: int,
                               mask: Optional[torch.Tensor] = None,
                               rec_lr: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``step_frames`` with the frames' registration learned jointly with the net: ``coords`` [B, H*W, 2] are the
        BASE coordinates (``affine_coords`` of an external registration, a plain grid ...), frame f's rows are moved by
        ``reg.theta[f]`` -- a 2 x 3 matrix on the normalised coordinates, ``motion.get_transformed_coords``'
        convention -- and the step goes on as ``step_frames`` does; the backward also gives dL/dcoords
        (wire_mlp_bwd_coords), which a deterministic reduction turns into the six numbers dL/dtheta of every frame
        (wire_warp_coords_bwd), and two Adam updates follow: the net's with the trainer's rate and schedule, and
        ``reg.theta``'s with ``reg.lr`` (``lr = 0`` freezes either).  With ``reg.pin_first`` frame 0 receives a zero
        gradient and keeps its matrix exactly.  One fixed sequence of launches, no host synchronisation.

        Arguments, shapes and errors are those of ``step_frames``, and ``coords.shape[0]`` must be ``reg.B`` (every
        call steps all the frames of the registration).  After the step ``self.coords`` holds the warped coordinates,
        ``self.g_coords[:B*H*W]`` dL/d(warped coords), ``reg.grad`` dL/dtheta and ``self.y`` the high-resolution
        frames.  Returns the device loss.  2-D grids, single process."""
        H, W, scale, xy, B, gt, mk = self._frames_args("step_frames_registered", coords, gt_lr, scale, mask, rec_lr)
        if not isinstance(reg, FrameRegistration) or reg.theta.device != self.dev:
            raise ValueError("reg must be a FrameRegistration on the trainer's device (FusedTrainer.registration)")
        if B != reg.B:
            raise ValueError(f"coords hold {B} frames, the registration {reg.B}")
        L = self.L
        stream = self._stream()
        n = B * H * W
        self._reserve(n)
        self._reserve_registered(n, B)
        g = self.gbuf[0]
        self._pack(stream)
        _lib.check(L.wire_warp_coords_fwd(stream, xy.data_ptr(), reg.theta.data_ptr(), B, H * W,
                                          self.coords.data_ptr()), "warp_coords_fwd")
        src = self._fwd_loss_bwd(stream, self.coords.data_ptr(), n, self._frames_loss(B, H, W, scale, gt, mk, rec_lr),
                                 g, self.grad_ptrs[0], coords_grad=True)
        _lib.check(L.wire_warp_coords_bwd(stream, xy.data_ptr(), reg.theta.data_ptr(), self.g_coords.data_ptr(), B,
                                          H * W, int(reg.pin_first), reg.grad.data_ptr(), None,
                                          self.warp_ws.data_ptr(), self.warp_ws.numel()), "warp_coords_bwd")
        self._finish(stream, g, src)
        reg.t += 1
        _lib.check(L.wire_adam_step_flat(stream, reg.theta.data_ptr(), reg.grad.data_ptr(), reg.exp_avg.data_ptr(),
                                         reg.exp_avg_sq.data_ptr(), 6 * B, float(reg.lr), reg.betas[0], reg.betas[1],
                                         reg.eps, reg.t), "adam (registration)")
        return self.loss

    # ------------------------------------------------------------------ CT step
    def step_radon(self, sinogram: torch.Tensor, thetas: torch.Tensor, lambda_tv: float = 0.0) -> torch.Tensor:
        """One optimizer step of the CT loop (wire_ct.py:128-139): the model is evaluated on the WHOLE grid in raster
        order (``img_estim = model(coords).reshape(-1, H, W)``), ``lin_inverse.radon`` turns it into a sinogram
        ([nangles, W]), loss = mean squared error against ``sinogram``; backward through the adjoint Radon kernel
        and the network, Adam.  The image estimate of this step stays in ``self.y`` ([H*W, 1]).
        ``lambda_tv`` != 0 adds ``lambda_tv * utils.total_variation_loss(img_estim)`` (bspline_ct.py's ``lambda_tv``)
        to the loss and its gradient to the adjoint's dL/dy (wire_tv_add_grad, between the adjoint and the backward);
        the returned loss is the total and ``self.tv_parts`` holds [loss, mse, tv, 0].  With 0.0 that kernel is not
        launched and the step issues the launches of the plain one.  2-D grids, one output feature, single process."""
        self._need_grid("step_radon", one_output=True)
        lam = self._tv_weight("lambda_tv", lambda_tv)
        H, W = int(self.grid[0]), int(self.grid[1])
        th = thetas.detach().to(self.dev, torch.float32).contiguous()
        A = th.numel()
        tgt = self._f32_elems("sinogram", sinogram, A, W)
        # (of exactly A * W elements: tests/test_gpu_workspace_fill.py fills the two whole)
        sino, gsino = self._buf("_sino", A * W, exact=True), self._buf("_gsino", A * W, exact=True)

        def loss(stream, g):
            L = self.L
            _lib.check(L.wire_radon_fwd(stream, self.y.data_ptr(), th.data_ptr(), H, W, A, sino.data_ptr()), "radon")
            _lib.check(L.wire_mse_grad(stream, sino.data_ptr(), tgt.data_ptr(), None, 0, A * W, 1, 1.0,
                                       gsino.data_ptr(), self._loss_slot(g)[0], None, self.partial.data_ptr()),
                       "mse_grad")
            _lib.check(L.wire_radon_bwd(stream, gsino.data_ptr(), th.data_ptr(), H, W, A, self.gy.data_ptr()),
                       "radon_bwd")
        return self._raster_step(loss, prior=(H, W, 1, lam, 0.0))

    # ------------------------------------------------------------------ volume CT step
    def step_radon_volume(self, sinogram: torch.Tensor, thetas: torch.Tensor, slab: Optional[int] = None,
                          lambda_tv: float = 0.0, lambda_tv_t: float = 0.0) -> torch.Tensor:
        """One optimizer step of CT on a volume: the model is evaluated on the WHOLE (H, W, T) grid in row order (row
        (i*W + j)*T + k), so its output is the volume as [H][W][T] with the slice index innermost;
        ``lin_inverse.radon_volume`` turns it into the stack of sinograms ([nangles, W, T]: the reference's
        ``radon(..., is_3d=True)`` with the slice last, wire_radon_vol_fwd), loss = mean squared error against
        ``sinogram`` (CUDA float32 of nangles * W * T elements in that order); backward through the gather adjoint
        (wire_radon_vol_bwd) and the network, Adam.  No transpose of the volume is made either way, and unlike
        ``step_radon`` the step is reproducible: the same call gives the same bits.

        ``slab=None``: one pass, and the volume estimate of the step stays in ``self.y`` ([H*W*T, 1]).  ``slab`` = a
        number of pixels, 1 <= slab < H*W: the operator mixes all pixels, but it is linear, so dL/dy of the whole volume
        needs no stored activations.  Pass 1 renders the volume forward-only, slab by slab, into ``self.y_vol``
        ([H*W*T]); the operator, the loss, the adjoint and the prior run on the full buffers and leave dL/dy of every
        row; pass 2 walks the pixel ranges [p0, p0 + slab), each a contiguous row range of whole pixels, runs the
        storing forward and the backward against that range of dL/dy, sums the gradients and runs Adam once.  The
        activations then hold ``slab * T`` rows instead of ``H*W*T``, at the price of ONE EXTRA FORWARD and of 8 bytes
        per row for the two full buffers; the full volume of the step is in ``self.y_vol``, and ``self.y`` holds the
        last slab only.  ``slab >= H*W`` is the one-pass path.

        ``lambda_tv`` / ``lambda_tv_t`` != 0 add ``step_coded``'s prior, ``lambda_tv * tv_s + lambda_tv_t * tv_t`` of
        the (H, W, T) volume (wire_tv_add_grad, between the adjoint and the backward); the full volume and the full
        dL/dy exist on both paths, so the prior works with slabs too.  The returned loss is the total and
        ``self.tv_parts`` holds [loss, mse, tv_s, tv_t].  With both 0.0 that kernel is not launched.
        3-D grids, one output feature, single process."""
        self._need_grid("step_radon_volume", rank=3, one_output=True)
        H, W, T = (int(v) for v in self.grid)
        NP, n = H * W, H * W * T
        lam_s, lam_t = self._tv_weight("lambda_tv", lambda_tv), self._tv_weight("lambda_tv_t", lambda_tv_t)
        prior = lam_s != 0.0 or lam_t != 0.0
        per = NP if slab is None else int(slab)
        if per < 1:
            raise ValueError(f"slab {per} must be >= 1 pixel")
        per = min(per, NP)
        if not isinstance(thetas, torch.Tensor) or thetas.numel() < 1:
            raise ValueError("thetas must be a tensor of at least one angle (degrees)")
        A = thetas.numel()
        tgt = self._f32_elems("sinogram", sinogram, A, W, T)
        th = thetas.detach().to(self.dev, torch.float32).contiguous()
        L, d = self.L, C.byref(self.desc)
        sino, gsino = self._buf("_vsino", A * W * T), self._buf("_gvsino", A * W * T)
        stream = self._stream()
        self._reserve(per * T)
        g0 = self.gbuf[0]

        def operator(y: torch.Tensor, gy: torch.Tensor):
            """y -> sinograms -> loss (behind g0) and its gradient -> dL/dy into gy, all on the full grid."""
            def loss(stream, g):
                _lib.check(L.wire_radon_vol_fwd(stream, y.data_ptr(), th.data_ptr(), H, W, T, A, sino.data_ptr()),
                           "radon_vol_fwd")
                _lib.check(L.wire_mse_grad(stream, sino.data_ptr(), tgt.data_ptr(), None, 0, A * W * T, 1, 1.0,
                                           gsino.data_ptr(), self._loss_slot(g)[0], None, self.partial.data_ptr()),
                           "mse_grad")
                _lib.check(L.wire_radon_vol_bwd(stream, gsino.data_ptr(), th.data_ptr(), H, W, T, A, gy.data_ptr()),
                           "radon_vol_bwd")
            return loss

        self._pack(stream)
        if per == NP:
            self._grid_coords(stream, 0, n, self.coords)
            src = self._fwd_loss_bwd(stream, self.coords.data_ptr(), n, operator(self.y, self.gy), g0,
                                     self.grad_ptrs[0], (H, W, T, lam_s, lam_t))
            return self._finish(stream, g0, src)
        rows = per * T
        yv, gv = self._buf("y_vol", n, exact=True), self._buf("_gy_vol", n, exact=True)
        # pass 1: the volume, forward-only (no stored activations: the step's act buffer is more than that takes)
        ab = _lib.check(L.wire_act_bytes(d, rows, 0))
        act = self.act if ab <= self.act_bytes else self._buf("_act_fwd", ab, torch.uint8)
        for r0 in range(0, n, rows):
            nr = min(rows, n - r0)
            self._grid_coords(stream, r0, nr, self.coords)
            _lib.check(L.wire_mlp_fwd(stream, d, self.packed.data_ptr(), self.coords.data_ptr(), nr,
                                      yv.data_ptr() + 4 * r0, act.data_ptr(), act.numel(), 0), "fwd")
        operator(yv, gv)(stream, g0)
        slot, src = self._loss_slot(g0)
        if prior:
            self._tv_add_grad(stream, H, W, T, lam_s, lam_t, slot, yv, gv)
            src = self.tv_parts[0:1]
        # pass 2: storing forward and backward, slab by slab, against dL/dy of the slab's rows
        if getattr(self, "_gslab_ptrs", None) is None:
            # wire_mlp_bwd overwrites its gradients: the slabs after the first write here and are added to gbuf[0]
            gs = self._buf("_gslab", self.count + 1, zero=True)
            self._gslab_ptrs = _lib.ptr_array([gs.data_ptr() + 4 * o for o in self.offsets])
        for r0 in range(0, n, rows):
            nr = min(rows, n - r0)
            g, gp = (g0, self.grad_ptrs[0]) if r0 == 0 else (self._gslab, self._gslab_ptrs)
            self._grid_coords(stream, r0, nr, self.coords)
            self._fwd_loss_bwd(stream, self.coords.data_ptr(), nr, None, g, gp, gy_ptr=gv.data_ptr() + 4 * r0)
            if r0 > 0:
                # (the gradients alone: the float behind them is the loss slot, which step_coded's slabs use)
                g0[:self.count].add_(g[:self.count])
        return self._finish(stream, g0, src)

    # ------------------------------------------------------------------ video compressive-sensing step
    def step_coded(self, coded: torch.Tensor, masks, nframes: int, dup_last: bool = True,
                   slab: Optional[int] = None, est: Optional[torch.Tensor] = None, lambda_tv: float = 0.0,
                   lambda_tv_t: float = 0.0) -> torch.Tensor:
        """One optimizer step of video compressive sensing (the coded exposure of modules/lin_inverse.py:42-95): the
        model is evaluated on the WHOLE (H, W, T) grid in row order (row (i*W + j)*T + k), every pixel's T frames are
        multiplied by its mask and summed in groups of ``nframes`` -- ``lin_inverse.video2codedvideo`` -- and the loss
        is the mean squared error against ``coded``; backward through the coding and the network, Adam.  In this row
        order the operator is one pass over contiguous memory (wire_coded_mse_grad): the driver's
        ``reshape(H, W, T).permute(2, 0, 1)`` into the reference's (1, T, H, W) is not made.

        ``coded``: CUDA float32 of C' * H*W * O elements, frame-major ([C'][H*W][O]; for O = 1 exactly the reference's
        (1, C', H, W)), C' = ceil(T / nframes) + dup_last.  ``dup_last=True`` is the reference's coded video, whose last
        group comes twice; False the plain C frames.  ``masks``: H*W*T elements in (H, W, T) order, shared by the
        channels -- the numpy array of ``lin_inverse.get_video_coding_frames`` (uploaded once and kept while the same
        array object is passed; change the masks by passing a new array) or a CUDA float32 tensor.  ``est`` (optional,
        shaped like ``coded``) receives the coded estimate.

        ``slab=None``: one pass, and the video estimate of the step stays in ``self.y`` ([H*W*T, O]).  ``slab`` = a
        number of pixels: the step walks the pixel ranges [p0, p0 + slab), each a contiguous row range of whole pixels,
        sums their gradients and losses and runs Adam once, so the activations hold ``slab * T`` rows instead of
        ``H*W*T``; ``self.y`` then holds the last slab only -- ``render()`` gives the whole video.  ``slab >= H*W`` is
        the one-pass path.

        ``lambda_tv`` / ``lambda_tv_t`` != 0 add ``lambda_tv * tv_s + lambda_tv_t * tv_t`` to the loss: tv_s is
        ``utils.total_variation_loss`` of every frame, tv_t the same sum of absolute differences between consecutive
        frames (ours; the reference has no video prior).  Its gradient is added to the coding's dL/dy
        (wire_tv_add_grad, between the coded loss and the backward); the returned loss is the total and
        ``self.tv_parts`` holds [loss, mse, tv_s, tv_t].  With both 0.0 that kernel is not launched and the step is the
        plain one, bit for bit.  A prior needs the one-pass path: neighbour pairs would straddle the slabs.
        3-D grids, single process."""
        self._need_grid("step_coded", rank=3)
        H, W, T = (int(v) for v in self.grid)
        NP = H * W
        nframes = int(nframes)
        if nframes < 1:
            raise ValueError(f"nframes {nframes} must be >= 1")
        lam_s, lam_t = self._tv_weight("lambda_tv", lambda_tv), self._tv_weight("lambda_tv_t", lambda_tv_t)
        prior = lam_s != 0.0 or lam_t != 0.0
        if prior and slab is not None and 1 <= int(slab) < NP:
            raise ValueError(f"slab {int(slab)} splits the grid of {NP} pixels: a TV prior (lambda_tv, lambda_tv_t) "
                             f"needs the one-pass path, slab=None or slab >= H*W")
        dup = int(bool(dup_last))
        Cp = (T + nframes - 1) // nframes + dup
        gt = self._f32_elems("coded", coded, Cp, NP, self.O)
        if isinstance(masks, torch.Tensor):
            mk = masks.detach()
            if not mk.is_cuda or mk.dtype != torch.float32 or mk.numel() != NP * T:
                raise ValueError(f"masks must be a numpy array or a CUDA float32 tensor of {NP} x {T} elements")
            mk = mk.contiguous()
        else:
            if getattr(self, "_coded_masks_src", None) is not masks:
                arr = np.asarray(masks)
                if arr.size != NP * T:
                    raise ValueError(f"masks must be a numpy array or a CUDA float32 tensor of {NP} x {T} elements")
                self._coded_masks_dev = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)) \
                    .to(self.dev)
                self._coded_masks_src = masks
            mk = self._coded_masks_dev
        self._f32_like("est", est, gt, "coded")
        per = NP if slab is None else int(slab)
        if per < 1:
            raise ValueError(f"slab {per} must be >= 1 pixel")
        per = min(per, NP)
        stream = self._stream()
        self._reserve(per * T)
        g0 = self.gbuf[0]
        if per < NP and getattr(self, "_gslab_ptrs", None) is None:
            # wire_mlp_bwd overwrites its gradients: the slabs after the first write here and are added to gbuf[0]
            gs = self._buf("_gslab", self.count + 1, zero=True)
            self._gslab_ptrs = _lib.ptr_array([gs.data_ptr() + 4 * o for o in self.offsets])
        self._pack(stream)
        for p0 in range(0, NP, per):
            npix = min(per, NP - p0)
            g, gp = (g0, self.grad_ptrs[0]) if p0 == 0 else (self._gslab, self._gslab_ptrs)

            def loss(stream, g):
                _lib.check(self.L.wire_coded_mse_grad(stream, self.y.data_ptr(), p0, npix, NP, T, self.O, nframes, dup,
                                                      mk.data_ptr(), gt.data_ptr(), self.gy.data_ptr(),
                                                      self._opt_ptr(est), self._loss_slot(g)[0],
                                                      self.partial.data_ptr()), "coded_mse_grad")
            self._grid_coords(stream, p0 * T, npix * T, self.coords)
            # (a prior means one pass: p0 == 0 and y holds the whole grid)
            src = self._fwd_loss_bwd(stream, self.coords.data_ptr(), npix * T, loss, g, gp, (H, W, T, lam_s, lam_t))
            if p0 > 0:
                g0.add_(g)
        # (one pass, or no prior: the total is in the slot behind gbuf[0])
        return self._finish(stream, g0, src if prior else self._loss_slot(g0)[1])

    @property
    def flat_grad(self) -> torch.Tensor:
        return self.gbuf[0][:self.count]

    # ------------------------------------------------------------------ metrics
    def psnr(self, rec: torch.Tensor, gt: Optional[torch.Tensor] = None) -> torch.Tensor:
        """utils.psnr(gt, rec) = 10 log10(max(gt) / mse) (modules/utils.py:67-82) computed on the
        device; returns a 0-dim device tensor (no host sync, no image copy)."""
        if gt is None:
            self._need_target("psnr without gt")
        out = self._metric(0, rec, self.target if gt is None else gt, 0.0)
        return 10.0 * torch.log10(out[1] / (out[0] / rec.numel()))

    def iou(self, pred: torch.Tensor, gt: Optional[torch.Tensor] = None, thres: float = 0.5) -> torch.Tensor:
        """volutils.get_IoU(pred, gt, thres) (modules/volutils.py:74-91) on the device; ``pred`` is
        left untouched (the reference binarises it in place)."""
        if gt is None:
            self._need_target("iou without gt")
        out = self._metric(1, pred, self.target if gt is None else gt, thres)
        return out[0] / out[1]

    def ssim(self, rec: torch.Tensor, gt: Optional[torch.Tensor] = None, window="gaussian", data_range=None,
             full: bool = False):
        """functional.ssim(rec, gt, H, W, ...) on the trainer's (H, W) grid (a 3-D grid is a ValueError): the
        structural similarity the super-resolution drivers log every epoch (``window="gaussian"``,
        wire_SISR.py:169) and every driver reports at the end (``window="uniform"``, which needs ``data_range``),
        computed on the device from the channel-last ``render()`` / ``rec`` as it is.  ``gt=None`` compares against the
        trainer's target.  Returns a 0-dim device tensor (no host sync), or ``(ssim, map)`` with ``full=True``; the
        workspace is kept between calls.  ``update_best`` keeps the SMALLEST metric, so a caller that tracks the best
        image by SSIM passes ``-ssim``."""
        if len(self.grid) != 2:
            raise ValueError("ssim compares 2-D images; this trainer's grid is 3-D")
        if gt is None:
            self._need_target("ssim without gt")
            gt = self.target
        res, self._ssim_ws = functional._ssim(rec, gt, self.grid[0], self.grid[1], window, data_range, full,
                                              getattr(self, "_ssim_ws", None))
        return res

    def _metric(self, mode: int, rec: torch.Tensor, gt: torch.Tensor, thres: float) -> torch.Tensor:
        rec = rec.detach().to(torch.float32).contiguous()
        gt = gt.detach().to(self.dev, torch.float32).contiguous()
        if rec.numel() != gt.numel():
            raise ValueError("metric operands differ in size")
        out = torch.empty(2, dtype=torch.float32, device=self.dev)
        stream = self._stream()
        _lib.check(self.L.wire_eval_metric(stream, mode, rec.data_ptr(), gt.data_ptr(), rec.numel(), thres,
                                           out.data_ptr(), self.partial.data_ptr()), "metric")
        return out

    # ------------------------------------------------------------------ best-so-far tracking
    def update_best(self, metric: torch.Tensor, image: torch.Tensor, force: bool = False) -> None:
        """Device-side restatement of the drivers' best-result bookkeeping -- ``if (mse_array[epoch] < best_mse) or
        (epoch == 0): best_mse = mse_array[epoch]; best_img = imrec`` (wire_image_denoise.py:176-178; pass
        ``force=(epoch == 0)``) and ``if lossval < best_mse: ...; best_img = copy.deepcopy(im_estim)``
        (wire_occupancy.py:170-172): ``metric`` is a 1-element device tensor (an MSE, ``tr.loss`` ...), ``image`` the
        reconstruction (``tr.rec``, a render).  No ``.item()``, no per-epoch copy of the image to the host: a
        compare-and-copy kernel keeps ``self.best_metric`` / ``self.best_img`` current."""
        img = image.detach()
        if not img.is_cuda or img.dtype != torch.float32 or not img.is_contiguous():
            raise ValueError("image must be a contiguous CUDA float32 tensor")
        m = metric.detach().reshape(-1)
        if not m.is_cuda or m.dtype != torch.float32 or m.numel() != 1:
            raise ValueError("metric must be a 1-element CUDA float32 tensor")
        if getattr(self, "best_img", None) is None or self.best_img.numel() != img.numel():
            self.best_img = torch.zeros_like(img)
            self.best_metric = torch.full((1,), float("inf"), dtype=torch.float32, device=self.dev)
        stream = self._stream()
        _lib.check(self.L.wire_track_best(stream, m.data_ptr(), self.best_metric.data_ptr(), int(bool(force)),
                                          img.data_ptr(), self.best_img.data_ptr(), img.numel(), None), "track_best")

    # ------------------------------------------------------------------ mesh of a trained occupancy
    def extract_mesh(self, thres: float = 0.5, volume: Optional[torch.Tensor] = None, smoothen: bool = False):
        """The iso-surface of the trainer's (H, W, T) volume at ``thres`` as ``(vertices [V, 3] float32, faces [F, 3]
        int32)`` on the device -- what the occupancy driver's last lines hand to ``march_and_save``
        (wire_occupancy.py:198-201), without the copy of the volume to the host; ``volutils.save_mesh`` writes it.
        ``volume=None`` takes the best tracked image (``update_best``) if there is one, else ``rec`` (``keep_rec=True``);
        with neither it is a ValueError.  A 3-D grid with one output only.  ``smoothen`` as in
        ``volutils.march_and_save``.  One host sync (functional.iso_surface)."""
        from .modules import volutils
        if self.tz is None or len(self.grid) != 3 or self.O != 1:
            raise ValueError("extract_mesh needs a 3-D grid (H, W, T) and out_features == 1")
        if volume is None:
            volume = getattr(self, "best_img", None)
            if volume is None:
                volume = self.rec
            if volume is None:
                raise ValueError("extract_mesh: no volume -- pass one, track one with update_best, or build the trainer "
                                 "with keep_rec=True")
        if not isinstance(volume, torch.Tensor) or volume.numel() != self.npoints:
            raise ValueError(f"extract_mesh: the volume must be a tensor of {self.npoints} values")
        return volutils.march(volume.reshape(*self.grid), thres, smoothen)

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def render(self, first: int = 0, count: Optional[int] = None, tile: int = 1 << 20,
               sigmoid: bool = False) -> torch.Tensor:
        """Forward-only dense query of grid rows [first, first+count) in tiles
        (no saved activations): the reference's full-image / volume evaluation.  ``sigmoid=True`` applies
        ``torch.sigmoid`` to the result, the occupancy cube ``export_mesh`` hands to marching cubes
        (modules/volutils.py:124-133; ``extract_mesh`` / ``volutils.march_and_save`` mesh it)."""
        L, d = self.L, C.byref(self.desc)
        stream = self._stream()
        count = int(count if count is not None else self.npoints - first)
        out = torch.empty(count, self.O, dtype=torch.float32, device=self.dev)
        self._pack(stream)
        tile = min(tile, max(count, 1))
        ab = _lib.check(L.wire_act_bytes(d, tile, 0))
        act = torch.empty(ab, dtype=torch.uint8, device=self.dev)
        coords = torch.empty(tile * self.desc.in_features, dtype=torch.float32, device=self.dev)
        for s in range(0, count, tile):
            n = min(tile, count - s)
            self._grid_coords(stream, first + s, n, coords)
            _lib.check(L.wire_mlp_fwd(stream, d, self.packed.data_ptr(), coords.data_ptr(), n,
                                      out.data_ptr() + 4 * s * self.O, act.data_ptr(), ab, 0), "fwd")
        if sigmoid:
            _lib.check(L.wire_sigmoid_inplace(stream, out.data_ptr(), out.numel()), "sigmoid")
        return out
