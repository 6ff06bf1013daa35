"""The cases of tests/test_gpu_dispatch_map.py and of its recorder tests/golden/make_dispatch_golden.py: which kernels one
FusedTrainer.step launches, per net kind, width, row count and GEMM-family knob setting.

Every net has D = 2 inputs, 2 hidden layers and 3 outputs.  Widths: the real kinds and mfn at 256 (P = 256: whole-net
kernels, the chain, stored r) and at 64 (P = 64: layer by layer); wire at K = 128 (hidden_features 182 / sqrt 2), wire2d
at K = 64 (hidden_features 128 / 2).  Rows: 4096 (at the M >= 4096 line of the 16 x 16 x 32 and 2 x fp16 kernels) and
1024 (below it)."""
import json
import re

import torch

from _util import kernel_names, tune

DEV = "cuda"
GRID = (64, 64)                                                  # 4096 points
ROWS = (4096, 1024)
LAYERS, OUT = 2, 3
KINDS = ("wire", "wire2d", "siren", "gauss", "relu", "bspline_form", "bspline_cubic", "mfn")
WIDTHS = {"wire": (182,), "wire2d": (128,)}                      # hidden_features; every other kind: (256, 64)
KNOBS = {"default": {}, "split_f16=0": dict(split_f16=0), "split_bf16=0": dict(split_bf16=0)}
WIRE_KNOBS = {"complex_3m=0": dict(complex_3m=0), "split_bf16=0,complex_3m=0": dict(split_bf16=0, complex_3m=0)}
# torch's own kernels, copies, and the runtime calls the profiler lists beside the kernels (hipLaunchKernel, ...): everything
# else a step launches is the library's
NOT_OURS = re.compile(r"\bat::|\bc10::|rocprim|hipcub|thrust|Memcpy|Memset|memcpy|memset|^hip[A-Z]\w*$")


def ours(names):
    return sorted({k for k in names if not NOT_OURS.search(k)})


def write_map(sets, path):
    """{case id: [names]} as one table of the distinct names and, per case, indices into it (a name has ~200 characters
    and recurs in most cases)."""
    names = sorted({k for v in sets.values() for k in v})
    ix = {k: i for i, k in enumerate(names)}
    with open(path, "w") as f:
        f.write('{"names": [\n' + ",\n".join(json.dumps(k) for k in names) + '\n],\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(c)}: {json.dumps([ix[k] for k in v])}" for c, v in sorted(sets.items())))
        f.write("\n}}\n")


def read_map(path):
    with open(path) as f:
        m = json.load(f)
    return {c: [m["names"][i] for i in v] for c, v in m["cases"].items()}


def model_of(kind, hf):
    from wire_amd.modules import bspline_cubic, mfn, models
    torch.manual_seed(5)
    if kind == "mfn":
        return mfn.INR(2, hf, LAYERS, OUT).to(DEV)
    if kind == "bspline_cubic":
        return bspline_cubic.INR(2, hf, LAYERS, 0, OUT).to(DEV)
    return models.get_INR(nonlin=kind, in_features=2, out_features=OUT, hidden_features=hf, hidden_layers=LAYERS).to(DEV)


def case_ids(kind):
    knobs = dict(KNOBS, **(WIRE_KNOBS if kind == "wire" else {}))
    return [(f"{kind}/hf{hf}/n{n}/{k}", hf, n, kv) for hf in WIDTHS.get(kind, (256, 64)) for n in ROWS
            for k, kv in knobs.items()]


def run_kind(kind, with_results=False):
    """{case id: sorted kernel names of one step}; with_results also {case id: (loss, rec, flat_grad) of that step}."""
    from wire_amd.trainer import FusedTrainer
    g = torch.Generator().manual_seed(11)
    target = torch.rand(GRID[0] * GRID[1], OUT, generator=g)
    perm = torch.randperm(GRID[0] * GRID[1], generator=g)
    sets, results = {}, {}
    for cid, hf, n, kv in case_ids(kind):
        idx = perm[:n].contiguous().to(DEV)
        with tune(**kv):
            tr = FusedTrainer(model_of(kind, hf), GRID, target, lr=0.0, keep_rec=True)
            names = kernel_names(lambda: tr.step(idx))
            if with_results:
                loss = tr.step(idx)
                torch.cuda.synchronize()
                results[cid] = (loss.clone(), tr.rec.clone(), tr.flat_grad.clone())
        sets[cid] = ours(names)
    return (sets, results) if with_results else sets
