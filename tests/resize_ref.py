"""numpy restatement of the resize operator of include/wire_hip.h (wire_resize.hip): the tables of one
axis in fp64 with the weights rounded to fp32 once, the device's table layout, dense R_v / R_h for an fp64 oracle, and an
fp32 evaluation in the header's tap order (rows outer, columns inner, ascending) whose distance to that oracle is the
`err_ref` of the project's protocol  err_build <= 2 err_ref + 1e-6.

Written from the definition, not from the kernel: taps first, then clamping and merging, then the ranges by counting."""
import math

import numpy as np

NEAREST, LINEAR, CUBIC, AREA = 0, 1, 2, 3
MODES = {"nearest": NEAREST, "linear": LINEAR, "cubic": CUBIC, "area": AREA}


def out_size(n_in, f):
    """cv2's dsize from fx / fy: cvRound(n_in * f), round half to even."""
    return int(np.rint(n_in * f))


def _taps(mode, n_in, s, d):
    """[(index before clamping, fp64 weight)] of output d, in tap order."""
    if s == 1.0:
        return [(d, 1.0)]
    if mode == NEAREST:
        return [(min(math.floor(d * s), n_in - 1), 1.0)]
    if mode == AREA:
        a, b = d * s, min((d + 1) * s, float(n_in))
        taps = []
        for i in range(math.floor(a), math.ceil(b)):
            ov = min(i + 1.0, b) - max(float(i), a)
            if ov > 0:
                taps.append((i, ov / (b - a)))
        return taps
    x = (d + 0.5) * s - 0.5
    i = math.floor(x)
    f = x - i
    if i < -4 or i > n_in + 4:                 # far outside: weight 1 on the border pixel
        return [(i, 1.0)]
    if mode == LINEAR:
        return [(i, 1.0 - f), (i + 1, f)]
    A = -0.75
    w0 = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A
    w1 = ((A + 2) * f - (A + 3)) * f * f + 1
    g = 1.0 - f
    w2 = ((A + 2) * g - (A + 3)) * g * g + 1
    return [(i - 1, w0), (i, w1), (i + 1, w2), (i + 2, 1.0 - w0 - w1 - w2)]


class Axis:
    """One axis' table: start, count [n_out] int32; w [n_out, K] float32 (zeros behind count), w64 the same before the
    rounding; lo, hi [n_in] int32 (lo = hi + 1: no output touches the source)."""

    def __init__(self, mode, n_in, n_out, s):
        mode = MODES.get(mode, mode)
        if n_in < 1 or n_out < 1 or not (math.isfinite(s) and s > 0):
            raise ValueError("bad axis")
        if mode == AREA and (n_out > n_in or not (n_out - 1) * s < n_in):
            raise ValueError("area does not up-scale")
        self.mode, self.n_in, self.n_out, self.s = mode, n_in, n_out, float(s)
        runs = []
        for d in range(n_out):
            merged = {}
            for i, w in _taps(mode, n_in, self.s, d):
                i = min(max(i, 0), n_in - 1)
                merged[i] = merged.get(i, 0.0) + w
            idx = sorted(merged)
            assert idx == list(range(idx[0], idx[0] + len(idx)))
            runs.append((idx[0], [merged[i] for i in idx]))
        self.K = max(len(w) for _, w in runs)
        self.start = np.array([r[0] for r in runs], np.int32)
        self.count = np.array([len(r[1]) for r in runs], np.int32)
        self.w64 = np.zeros((n_out, self.K))
        for d, (_, w) in enumerate(runs):
            self.w64[d, :len(w)] = w
        self.w = self.w64.astype(np.float32)
        end = self.start + self.count
        src = np.arange(n_in)
        self.lo = (end[None, :] <= src[:, None]).sum(1).astype(np.int32)
        self.hi = ((self.start[None, :] <= src[:, None]).sum(1) - 1).astype(np.int32)

    def words(self):
        """The axis as it lies in the device table: int32 words."""
        return np.concatenate([self.start, self.count, self.lo, self.hi, self.w.reshape(-1).view(np.int32)])

    def dense(self, rounded=True):
        """R of the axis [n_out, n_in] in fp64, from the fp32 weights (the operator the kernels apply) or the unrounded."""
        R = np.zeros((self.n_out, self.n_in))
        w = self.w.astype(np.float64) if rounded else self.w64
        for d in range(self.n_out):
            R[d, self.start[d]:self.start[d] + self.count[d]] = w[d, :self.count[d]]
        return R


class Resize:
    """R = R_v (x) R_h from (H, W) to (Hl, Wl); sy, sx default to n_in / n_out."""

    def __init__(self, mode, H, W, Hl, Wl, sy=None, sx=None):
        self.mode = MODES.get(mode, mode)
        self.H, self.W, self.Hl, self.Wl = H, W, Hl, Wl
        self.sy = H / Hl if sy is None else float(sy)
        self.sx = W / Wl if sx is None else float(sx)
        self.v = Axis(self.mode, H, Hl, self.sy)
        self.h = Axis(self.mode, W, Wl, self.sx)

    @classmethod
    def from_factors(cls, mode, H, W, fx, fy):
        return cls(mode, H, W, out_size(H, fy), out_size(W, fx), 1.0 / fy, 1.0 / fx)

    def geom(self):
        return (self.H, self.W, self.Hl, self.Wl, self.mode, self.sy, self.sx)

    def tab_words(self):
        return np.concatenate([self.v.words(), self.h.words()])

    def tab_bytes(self):
        return 4 * self.tab_words().size

    # ---- the fp64 oracle
    def fwd64(self, x, rounded=True):
        return np.einsum("ai,bj,ijc->abc", self.v.dense(rounded), self.h.dense(rounded), np.asarray(x, np.float64))

    def bwd64(self, g, rounded=True):
        return np.einsum("ai,bj,abc->ijc", self.v.dense(rounded), self.h.dense(rounded), np.asarray(g, np.float64))

    def mse_grad64(self, y, gt):
        """(loss, dL/dy, rec) of loss = mean((R y - gt)^2), all fp64."""
        rec = self.fwd64(y)
        d = rec - np.asarray(gt, np.float64)
        return (d * d).mean(), self.bwd64(2.0 * d / d.size), rec

    # ---- fp32 in the header's order: acc = fl(acc + fl(wv[a] * r_a)), r_a = fl(r_a + fl(wh[b] * x[a][b])), from 0
    def fwd32(self, x):
        x = np.asarray(x, np.float32)
        out = np.zeros((self.Hl, self.Wl, x.shape[2]), np.float32)
        for di in range(self.Hl):
            for dj in range(self.Wl):
                acc = np.zeros(x.shape[2], np.float32)
                for a in range(self.v.count[di]):
                    ra = np.zeros(x.shape[2], np.float32)
                    for b in range(self.h.count[dj]):
                        ra = ra + self.h.w[dj, b] * x[self.v.start[di] + a, self.h.start[dj] + b]
                    acc = acc + self.v.w[di, a] * ra
                out[di, dj] = acc
        return out

    def bwd32(self, g):
        g = np.asarray(g, np.float32)
        out = np.zeros((self.H, self.W, g.shape[2]), np.float32)
        for i in range(self.H):
            for j in range(self.W):
                acc = np.zeros(g.shape[2], np.float32)
                for dr in range(self.v.lo[i], self.v.hi[i] + 1):
                    ra = np.zeros(g.shape[2], np.float32)
                    for dc in range(self.h.lo[j], self.h.hi[j] + 1):
                        ra = ra + self.h.w[dc, j - self.h.start[dc]] * g[dr, dc]
                    acc = acc + self.v.w[dr, i - self.v.start[dr]] * ra
                out[i, j] = acc
        return out


def protocol_ok(got, want64, ref32):
    """err_build <= 2 err_ref + 1e-6, max-abs errors against the fp64 oracle; returns
    (ok, err_build, err_ref)."""
    eb = float(np.abs(np.asarray(got, np.float64) - want64).max())
    er = float(np.abs(np.asarray(ref32, np.float64) - want64).max())
    return eb <= 2 * er + 1e-6, eb, er


# ---- the short super-resolution run of tests/test_gpu_step_resized.py, on the CPU in fp64 ----------------------------------
SR = dict(H=16, W=16, Hl=8, Wl=8, mode="cubic", kind="siren", hf=64, layers=2, omega=30.0, lr=2e-4, steps=200)


def sr_image():
    """A smooth 16 x 16 image, two low-frequency sinusoids, and its 2 x bicubic down-sampling as fp32 [Hl*Wl, 1]."""
    H, W = SR["H"], SR["W"]
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = 0.5 + 0.25 * np.sin(2 * np.pi * j / W) + 0.2 * np.cos(2 * np.pi * i / H + 0.5)
    op = Resize(SR["mode"], H, W, SR["Hl"], SR["Wl"])
    return img, op.fwd64(img[:, :, None]).reshape(-1, 1).astype(np.float32), op


def sr_model():
    """The run's net, built on the CPU under torch.manual_seed(0): the GPU run starts from the same state_dict."""
    import torch
    from wire_amd.modules import models
    torch.manual_seed(0)
    return models.get_INR(nonlin=SR["kind"], in_features=2, out_features=1, hidden_features=SR["hf"],
                          hidden_layers=SR["layers"], first_omega_0=SR["omega"], hidden_omega_0=SR["omega"], scale=10.0)


def sr_oracle_losses(state, coords):
    """``steps`` Adam steps (torch.optim.Adam, constant lr) of oracle/torch_ref's fp64 forward under the dense R: the loss
    of every step.  ``state``: {name: numpy array}, ``coords`` [H*W, 2]."""
    import torch
    from oracle import torch_ref
    _, gt, op = sr_image()
    Rv, Rh = torch.tensor(op.v.dense()), torch.tensor(op.h.dense())
    p = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in state.items()
         if "omega_0" not in k and "scale_0" not in k}
    x, t = torch.tensor(np.asarray(coords), dtype=torch.float64), torch.tensor(gt, dtype=torch.float64)
    opt = torch.optim.Adam(list(p.values()), lr=SR["lr"])
    losses = []
    for _ in range(SR["steps"]):
        y = torch_ref.realnet_forward(SR["kind"], p, x, SR["layers"], SR["omega"], SR["omega"], 10.0)
        rec = torch.einsum("ai,bj,ijc->abc", Rv, Rh, y.reshape(SR["H"], SR["W"], 1)).reshape(-1, 1)
        loss = ((rec - t) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from _util import _grid_coords
    ls = sr_oracle_losses({k: v.detach().numpy() for k, v in sr_model().state_dict().items()},
                          _grid_coords(SR["H"], SR["W"]))
    print(f"fp64 oracle, {SR}: first loss {ls[0]:.6e}, loss of step {len(ls)} {ls[-1]:.6e}, min {min(ls):.6e}")
