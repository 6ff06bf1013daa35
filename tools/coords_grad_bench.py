"""Cost of the coordinate gradient.

Times, with HIP events, one backward of the whole-net path at the bench workload (wire 4 x 256 complex features,
262 144 rows), at the reference-API width (wire K = 181) and for siren 4 x 256, in three forms:
  params      -- the parameters' gradients only (what the project ran before: wire_mlp_bwd);
  params+x    -- the same plus the coordinate gradient (wire_mlp_bwd_coords with both);
  x_only      -- frozen parameters, the coordinate gradient alone (wire_mlp_bwd_coords, grads_host = NULL).
Each form runs backward(retain_graph=True) on one recorded forward, so only the backward is timed.
Prints one JSON line per configuration (and writes them to --out when given).

    python tools/coords_grad_bench.py [--iters 20] [--warmup 5] [--out profiles/coords_grad_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [
    ("wire_4x256_bench", "wire", 363, dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)),
    ("wire_K181_api", "wire", 256, dict(first_omega_0=20.0, hidden_omega_0=20.0, scale=30.0)),
    ("siren_4x256", "siren", 256, dict(first_omega_0=30.0, hidden_omega_0=30.0)),
]


def time_backward(model, coords, w, want_x, want_p, iters, warmup):
    for p in model.parameters():
        p.requires_grad_(want_p)
        p.grad = None
    x = coords.clone().requires_grad_(want_x)
    loss = (model(x) * w).sum()
    for _ in range(warmup):
        loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):
        a.record()
        loss.backward(retain_graph=True)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=512 * 512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from wire_amd.modules import models
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    coords = (torch.rand(a.n, 2, generator=g) * 2 - 1).to(dev)
    w = torch.randn(a.n, 3, generator=g).to(dev)
    lines = []
    for label, kind, hf, kw in CONFIGS:
        torch.manual_seed(0)
        model = models.get_INR(nonlin=kind, in_features=2, out_features=3, hidden_features=hf, hidden_layers=4,
                               **kw).to(dev)
        res = {"config": label, "n": a.n, "iters": a.iters}
        res["params"] = time_backward(model, coords, w, False, True, a.iters, a.warmup)
        res["params+x"] = time_backward(model, coords, w, True, True, a.iters, a.warmup)
        res["x_only"] = time_backward(model, coords, w, True, False, a.iters, a.warmup)
        base = res["params"]["median_ms"]
        res["coords_overhead"] = res["params+x"]["median_ms"] / base - 1.0
        res["x_only_over_params"] = res["x_only"]["median_ms"] / base
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
