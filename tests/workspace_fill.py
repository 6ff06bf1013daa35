"""Fill patterns for the caller-allocated workspaces of libwire_hip (``packed``, ``act``, ``scratch``, ``partial``, ``ws``)
and the helpers of tests/test_gpu_workspace_fill.py.

include/wire_hip.h promises that no call reads a byte of a workspace that the same call (for ``act``: the forward it
belongs to) has not written.  A test that allocates with ``torch.empty`` cannot see a violation: the allocator hands out
zero pages or small finite leftovers, and a stray read multiplies them by a zero weight.  ``fill`` writes the bytes of a
device tensor in place with a pattern that does show:

  ZERO   every byte 0x00: the baseline.
  ONES   every byte 0xFF: NaN as fp32, NaN as each fp16 half, the largest unsigned value (it wins every atomicMax where a
         zeroing is missing).
  BIG    the fp32 word 0x7F000000 = 2^127, finite: larger than any real maximum (a stale maximum slot gives a wrong
         scale), overflows in a sum, and survives fmaxf and relu, which swallow NaN.
  STALE  not a fill: the buffers stay as a PREVIOUS CALL of the same entry point left them -- on more rows, with targets
         (or upstream gradients) 4096 times larger, and on the other GEMM family where the case has a knob for it, so
         the layout of the leftovers differs.  ``fill`` refuses it; the tests run that previous call themselves.
"""
import ctypes as C

import torch

ZERO, ONES, BIG, STALE = "ZERO", "ONES", "BIG", "STALE"
FILLS = (ZERO, ONES, BIG)                      # what fill() writes
PATTERNS = (ZERO, ONES, BIG, STALE)
BIG_WORD = 0x7F000000                          # 2^127 as fp32
STALE_GAIN = 4096.0                            # the previous call's targets: gradients and maxima 2^12 larger
DEV = "cuda"


def _bytes_of(t):
    if not t.is_contiguous():
        raise ValueError("fill needs a contiguous tensor (a strided view would be written through its gaps)")
    return t.reshape(-1).view(torch.uint8)


def fill(t, pattern):
    """Write every byte of tensor ``t`` (any dtype, any device) in place.  BIG lays the word 00 00 00 7F (little endian)
    from the tensor's first byte, which must lie on a 4-byte boundary; a tail of 1 - 3 bytes continues the word."""
    b = _bytes_of(t)
    if pattern == ZERO:
        b.fill_(0)
    elif pattern == ONES:
        b.fill_(0xFF)
    elif pattern == BIG:
        if t.data_ptr() % 4:
            raise ValueError("BIG needs a tensor that starts on a 4-byte boundary")
        b.fill_(0)
        b[3::4] = BIG_WORD >> 24
    elif pattern == STALE:
        raise ValueError("STALE is not a fill: run the previous call instead")
    else:
        raise ValueError(f"unknown pattern {pattern!r}")
    return t


def fill_all(tensors, pattern, only=None):
    """fill() over a {name: tensor} dict; ``only`` = a name: that buffer gets ``pattern`` and the others ZERO -- for
    finding WHICH buffer a failing result depends on."""
    for k, t in tensors.items():
        fill(t, pattern if only in (None, k) else ZERO)


def same_bits(a, b):
    """Bit identity of two tensors of 4-byte elements (NaN == NaN of the same payload, -0 != +0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nan_like(shape, device=DEV):
    return torch.full(shape if isinstance(shape, (tuple, list)) else (int(shape),), float("nan"), dtype=torch.float32,
                      device=device)


def other_family(knobs):
    """The knob setting a STALE call runs under: the 3 x bf16 family for a case on the defaults (2 x fp16 at >= 4096 rows),
    the defaults for every other case."""
    return {} if knobs else dict(split_f16=0)


def first_difference(got, want):
    """'name: k of n words differ, first at i (got .. want ..)' for the first output of two dicts that differs."""
    for k in want:
        a, b = got[k].contiguous().view(torch.int32).reshape(-1), want[k].contiguous().view(torch.int32).reshape(-1)
        if a.shape != b.shape:
            return f"{k}: shape {tuple(got[k].shape)} != {tuple(want[k].shape)}"
        d = (a != b).nonzero()
        if d.numel():
            i = int(d[0])
            return (f"{k}: {d.numel()} of {a.numel()} words differ, first at {i}: "
                    f"{got[k].reshape(-1)[i].item()!r} != {want[k].reshape(-1)[i].item()!r}")
    return None


def check_patterns(run, stale, label, patterns=PATTERNS):
    """The criterion of every bit-exact case.  ``run(pattern)`` fills the workspaces (nothing for STALE), makes the call
    and returns {name: output tensor (a clone)}; ``stale()`` makes the previous call.  ZERO twice must agree (the
    determinism the header states); ONES, BIG and STALE must agree with ZERO."""
    base = run(ZERO)
    bad = []
    d = first_difference(run(ZERO), base)
    if d:
        bad.append(f"ZERO twice: {d}")
    for p in patterns:
        if p == ZERO:
            continue
        if p == STALE:
            stale()
        d = first_difference(run(p), base)
        if d:
            bad.append(f"{p}: {d}")
    assert not bad, f"{label}: the result depends on what the workspaces held before -- " + "; ".join(bad)
    return base


# ---------------------------------------------------------------------------------------------------------------------
# FusedTrainer
# ---------------------------------------------------------------------------------------------------------------------
def trainer_buffers(tr, frozen=()):
    """{name: tensor} of everything a step works in.  Of the flat gradient buffer only each trainable tensor's own slice:
    Adam steps over the alignment gaps (and the ``frozen`` tensors' slices, which no backward writes), and 0 x NaN would
    reach the parameters."""
    bufs = dict(packed=tr.packed, partial=tr.partial, act=tr.act, scratch=tr.scratch, coords=tr.coords, y=tr.y, gy=tr.gy)
    for i, (o, sz) in enumerate(zip(tr.offsets, tr.sizes)):
        if i not in frozen:
            bufs[f"grad{i}"] = tr.gbuf[0][o:o + sz]
    return bufs


def frozen_tensors(tr):
    from wire_amd import _lib
    return (0, 1) if tr.desc.kind == _lib.KIND["bspline_mscale_HL"] else ()


class TrainerCase:
    """One FusedTrainer (lr = 0) on a grid, its buffers reserved once for the whole grid (or ``reserve`` rows), and the
    run / stale pair of check_patterns for any of its steps: ``run(step, outputs, pattern)`` fills the buffers, makes the
    call ``step(tr)`` (which returns the loss) under the case's knobs and returns clones of the loss and of
    ``outputs(tr)``; ``stale(step)`` makes the previous call on the other GEMM family, the trainer's target (if it has
    one) STALE_GAIN times larger."""

    def __init__(self, model, grid, target, knobs, keep_rec=True, reserve=None):
        from wire_amd.trainer import FusedTrainer
        self.knobs = dict(knobs)
        self.tr = tr = FusedTrainer(model, grid, target, lr=0.0, keep_rec=keep_rec)
        tr._reserve(int(reserve if reserve is not None else tr.npoints))
        self.bufs = trainer_buffers(tr, frozen_tensors(tr))
        self.flat0 = tr.flat.clone()
        self.target = tr.target
        self.big_target = None if tr.target is None else tr.target * STALE_GAIN

    def _after(self):
        # lr = 0 keeps the parameters, except that 0 x NaN is NaN: a poisoned gradient must fail ITS comparison, not
        # every one after it
        torch.cuda.synchronize()
        self.tr.flat.copy_(self.flat0)
        self.tr.exp_avg.zero_()
        self.tr.exp_avg_sq.zero_()

    def run(self, step, outputs, pattern, only=None):
        from _util import tune
        tr = self.tr
        if pattern != STALE:
            fill_all(self.bufs, pattern, only)
        if tr.rec is not None:
            tr.rec.fill_(float("nan"))
        tr.gbuf[0][tr.count:].fill_(float("nan"))
        with tune(**self.knobs):
            loss = step(tr)
        out = dict(loss=loss.clone())
        out.update({k: v.clone() for k, v in outputs(tr).items()})
        self._after()
        return out

    def stale(self, step):
        from _util import tune
        tr = self.tr
        tr.target = self.big_target
        try:
            with tune(**other_family(self.knobs)):
                step(tr)
        finally:
            tr.target = self.target
        self._after()


# ---------------------------------------------------------------------------------------------------------------------
# the whole-net calls through ctypes (functional.py allocates inside the call, so a test cannot reach its buffers)
# ---------------------------------------------------------------------------------------------------------------------
class AbiNet:
    """wire_pack_params / wire_mlp_fwd / wire_mlp_bwd / wire_mlp_bwd_coords on a model's parameters, in buffers reserved
    once for ``cap`` rows (as a trainer keeps them) and used for n <= cap rows."""

    def __init__(self, model, cap, coords_grad):
        from wire_amd import _lib
        from wire_amd.functional import _native, _stream_ptr
        self.L = L = _lib.lib()
        self.check = _lib.check
        self.desc = model.net_desc()
        self.dp = dp = C.byref(self.desc)
        self.D, self.O = int(self.desc.in_features), int(self.desc.out_features)
        self.nat = [_native(p) for p in model.param_tensors()]
        self.params = _lib.ptr_array([p.data_ptr() for p in self.nat])
        self.s = _stream_ptr(torch.device(DEV))
        u8 = dict(dtype=torch.uint8, device=DEV)
        self.packed = torch.empty(L.wire_packed_floats(dp), dtype=torch.float32, device=DEV)
        self.ab = {sv: _lib.check(L.wire_act_bytes(dp, cap, sv), "wire_act_bytes") for sv in (0, 1)}
        self.act = {sv: torch.empty(self.ab[sv], **u8) for sv in (0, 1)}
        self.sb = _lib.check((L.wire_bwd_coords_scratch_bytes if coords_grad else L.wire_bwd_scratch_bytes)(dp, cap),
                             "scratch_bytes")
        self.scratch = torch.empty(self.sb, **u8)
        self.frozen = (0, 1) if self.desc.kind == _lib.KIND["bspline_mscale_HL"] else ()
        self.ptr_array = _lib.ptr_array

    def buffers(self):
        return dict(packed=self.packed, act0=self.act[0], act1=self.act[1], scratch=self.scratch)

    def pack(self):
        self.check(self.L.wire_pack_params(self.s, self.dp, self.params, self.packed.data_ptr()), "pack")

    def fwd(self, x, save):
        n = x.shape[0]
        y = nan_like((n, self.O))
        self.check(self.L.wire_mlp_fwd(self.s, self.dp, self.packed.data_ptr(), x.data_ptr(), n, y.data_ptr(),
                                       self.act[save].data_ptr(), self.ab[save], save), "fwd")
        return y

    def _grads(self):
        """NaN-prefilled gradient tensors and their pointer array (NULL for the frozen tensors, which no backward
        writes)."""
        g = [nan_like(p.numel() * (2 if p.is_complex() else 1)) for p in self.nat]
        return g, self.ptr_array([None if i in self.frozen else t.data_ptr() for i, t in enumerate(g)])

    def bwd(self, x, gy, coords=None, with_grads=True):
        """wire_mlp_bwd (coords None) or wire_mlp_bwd_coords (coords True) after fwd(x, 1); {name: output}."""
        n = x.shape[0]
        g, gp = self._grads() if with_grads else ([], None)
        a = (self.s, self.dp, self.packed.data_ptr(), x.data_ptr(), n, gy.data_ptr(), self.act[1].data_ptr(), self.ab[1],
             self.scratch.data_ptr(), self.sb, gp)
        out = {}
        if coords is None:
            self.check(self.L.wire_mlp_bwd(*a), "bwd")
        else:
            out["g_coords"] = nan_like((n, self.D))
            self.check(self.L.wire_mlp_bwd_coords(*a, out["g_coords"].data_ptr()), "bwd_coords")
        out.update({f"grad{i}": t for i, t in enumerate(g) if i not in self.frozen})
        return out
