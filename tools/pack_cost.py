#!/usr/bin/env python3
"""What wire_pack_params costs per optimizer step on the headline net (4 x 256 complex WIRE): the stream time of N
back-to-back calls by events, per call.  Set against the sum of its kernels' own durations in a rocprofv3 kernel trace
(profiles/r05_rocprofv3_kernel_stats.csv) the difference is what its launches cost in gaps -- the most that packing in
fewer launches could save per step.
    python3 tools/pack_cost.py [calls]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib
from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=363, hidden_layers=4,
                       first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(dev)
tr = FusedTrainer(model, (512, 512), torch.rand(512 * 512, 3), lr=5e-3, niters=2000)
L = _lib.lib()
stream = torch.cuda.current_stream(dev).cuda_stream


def pack():
    _lib.check(L.wire_pack_params(stream, C.byref(tr.desc), tr.param_ptrs, tr.packed.data_ptr()), "pack")


for _ in range(10):
    pack()
torch.cuda.synchronize()
out = []
for rep in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        pack()
    e1.record()
    torch.cuda.synchronize()
    out.append(e0.elapsed_time(e1) / calls * 1e3)
launches = None
try:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _util import _prof
    launches = _prof(pack)
except Exception:
    pass
print(f"wire_pack_params, {calls} back-to-back calls x 5: us per call {' '.join(f'{x:.1f}' for x in out)}  (min {min(out):.1f})"
      + (f"  profiled launches per call (class other): {launches[3]}" if launches else ""))
