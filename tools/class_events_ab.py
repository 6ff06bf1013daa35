#!/usr/bin/env python3
"""Interleaved A/B of tuning knobs on the headline training step, read per launch class: the HIP-event time
(wire_prof_enable / wire_prof_read) of the forward GEMMs, the data gradients, the weight gradients and everything else,
in ONE process on one box.  Same scheme as tools/knob_ab.py: 6 alternating blocks per setting, 3 unprofiled steps after
each switch, then 10 instrumented steps.
    python3 tools/class_events_ab.py first_dn bwd_lookahead first_dn+bwd_lookahead
One A/B (1 against 0) per argument; keys joined by "+" are switched together.  (profiles/r05_dgrad_events_ab.txt)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib
from wire_amd.modules import models
from wire_amd.trainer import FusedTrainer

dev = torch.device("cuda:0")
torch.manual_seed(0)
model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=363, hidden_layers=4,
                       first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0).to(dev)
tr = FusedTrainer(model, (512, 512), torch.rand(512 * 512, 3), lr=5e-3, niters=2000)
L = _lib.lib()
STEPS = 10


def read():
    ms, cnt, fl = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_double * 4)()
    L.wire_prof_read(ms, cnt, fl)
    return list(ms), list(cnt)


for arg in sys.argv[1:]:
    keys = arg.encode().split(b"+")
    default = [L.wire_tune_get(k) for k in keys]
    res = {1: [], 0: []}
    for rep in range(6):
        for v in (1, 0):
            for k in keys:
                _lib.check(L.wire_tune_set(k, v))
            for i in range(3):
                tr.step_hashed(rep * 100 + i)
            torch.cuda.synchronize()
            read()
            L.wire_prof_enable(1)
            for i in range(STEPS):
                tr.step_hashed(rep * 100 + 10 + i)
            torch.cuda.synchronize()
            L.wire_prof_enable(0)
            ms, cnt = read()
            res[v].append([m / STEPS for m in ms] + [c // STEPS for c in cnt])
    for k, dv in zip(keys, default):
        _lib.check(L.wire_tune_set(k, dv))
    for v in (1, 0):
        for cls, nm in enumerate(("fwd", "dgrad", "wgrad", "other")):
            xs = [r[cls] for r in res[v]]
            print(f"{arg} = {v}: class {nm} ({res[v][0][4 + cls]} launches) ms/step mean {sum(xs) / len(xs):.4f} "
                  f"min {min(xs):.4f}  [{' '.join(f'{x:.4f}' for x in xs)}]")
