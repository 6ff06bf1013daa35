#!/usr/bin/env python3
"""Times the two passes of the iso-surface extraction (wire_iso_count, wire_iso_emit) at the occupancy driver's shapes:
512 x 320 x 320 with a ball and with a noisy ball, and 512^3 with a ball.  Per pass: the median of 20 runs between
device events after 3 warm-up runs, the workspace and the outputs allocated once; the algorithmic bytes --
  count: the volume read once (4 N), the mask written once (N), both offset arrays written once (8 N)
  emit:  the volume read once (4 N), the mask and the offsets read once (9 N), vertices and faces written once (12 V + 12 F)
(N lattice points, V vertices, F faces; what the scans re-read of the mask and what the neighbour loads hit in the
caches is not counted) -- and the rate those bytes imply, beside the 5.0 - 5.2 TB/s that the project's stream probe
reads for mixed read / write traffic on this chip (profiles/r03_hbm_stream_probe.txt).  wire_iso_emit's time includes
its own 16-byte read-back of the counts.  A measurement, not a gate: it prints what it finds.
    python3 tools/iso_ab.py                       # the three cases
    python3 tools/iso_ab.py --shapes 64,40,40     # a small shape
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wire_amd import _lib

dev = torch.device("cuda:0")
STREAM_TBS = "5.0 - 5.2"


def ball(shape, noise):
    """sigmoid((r0 - r) / 1.5) around an off-lattice centre, r0 = 0.37 of the shortest side; `noise` adds that much
    uniform noise, which crinkles the surface and sprinkles small shells around it."""
    ax = [torch.arange(n, device=dev, dtype=torch.float32) - (n / 2 - 0.3) for n in shape]
    r = torch.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
    vol = torch.sigmoid((0.37 * min(shape) - r) / 1.5)
    del r
    if noise:
        g = torch.Generator(device=dev).manual_seed(0)
        vol += noise * (torch.rand(shape, device=dev, generator=g) - 0.5)
    return vol.contiguous()


def median_ms(fn, warm=3, runs=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def case(shape, noise, label):
    L = _lib.lib()
    H, W, T = shape
    N = H * W * T
    vol = ball(shape, noise)
    s = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(_lib.check(L.wire_iso_ws_bytes(H, W, T)), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)

    def count():
        _lib.check(L.wire_iso_count(s, vol.data_ptr(), H, W, T, 0.5, ws.data_ptr(), counts.data_ptr()), "count")

    count()
    V, F = counts.tolist()
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(F, 1), 3, dtype=torch.int32, device=dev)

    def emit():
        _lib.check(L.wire_iso_emit(s, vol.data_ptr(), H, W, T, 0.5, ws.data_ptr(), verts.data_ptr(), V,
                                   faces.data_ptr(), F), "emit")

    print(f"{label}: {H} x {W} x {T} = {N} points, {V} vertices, {F} faces, workspace {ws.numel() / 1e6:.0f} MB")
    for name, fn, nbytes in (("wire_iso_count", count, 13 * N), ("wire_iso_emit", emit, 13 * N + 12 * V + 12 * F)):
        med, lo, hi = median_ms(fn)
        print(f"  {name:15s} median {med:8.3f} ms  (min {lo:.3f}, max {hi:.3f}; 20 runs)   {nbytes / 1e9:7.3f} GB "
              f"algorithmic -> {nbytes / med / 1e9:6.3f} TB/s   (stream probe: {STREAM_TBS} TB/s)")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=None, help="H,W,T ... (default: the driver's three cases)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("iso_ab.py measures on the GPU; none is visible")
    print(f"# {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    if a.shapes:
        for sh in a.shapes:
            shape = tuple(int(x) for x in sh.split(","))
            case(shape, 0.0, "ball")
            case(shape, 0.6, "noisy ball")
    else:
        case((512, 320, 320), 0.0, "ball")
        case((512, 320, 320), 0.6, "noisy ball")
        case((512, 512, 512), 0.0, "ball")


if __name__ == "__main__":
    main()
