"""GPU checks of the resize operator (wire_resize.hip): the device tables bit for bit against the restatement of
tests/resize_ref.py, the forward, the adjoint and the fused loss against the fp64 oracle built from the dense R_v / R_h
by the project's protocol (err_build <= 2 err_ref + 1e-6 on max|error| / max|value|, err_ref being the restatement's own
fp32 evaluation in the header's tap order), the transpose identity, and the Python layer (functional.resize /
resize_adjoint, utils.resize)."""
import numpy as np
import pytest
import torch

from _util import relmax, within_ref
import resize_ref as ref
from workspace_fill import BIG, ONES, ZERO, fill, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["nearest", "linear", "cubic", "area"]

# (H, W, Hl, Wl, C) by explicit size, or (H, W, fx, fy, C) by factors.
#   (1,1,1,1,1)        one element                        (5,7,13,20,3)    up-scaling (no area): borders clamp and merge
#   (7,7,7,7,3)        the identity                       (70,130,33,61,5) several workgroups on both sides, the last
#   (12,18,3,6,1)      integer factors 4 and 3                             ragged, C no power of two
#   (13,17,5,7,3)      non-integer factors                (64,9,9,9,1)     eight-tap area rows, identity columns
#   (9,4,2,1,2)        one output column
SIZES = [(1, 1, 1, 1, 1), (7, 7, 7, 7, 3), (12, 18, 3, 6, 1), (13, 17, 5, 7, 3), (9, 4, 2, 1, 2), (5, 7, 13, 20, 3),
         (70, 130, 33, 61, 5), (64, 9, 9, 9, 1)]
FACTORS = [(13, 17, 0.5, 0.5, 3), (5, 7, 2.6, 2.6, 2)]


def _cases():
    out = []
    for mode in MODES:
        for H, W, Hl, Wl, Cc in SIZES:
            if mode != "area" or (Hl <= H and Wl <= W):
                out.append(pytest.param(mode, (H, W, Hl, Wl), None, Cc, id=f"{mode}-{H}x{W}-{Hl}x{Wl}x{Cc}"))
        for H, W, fx, fy, Cc in FACTORS:
            if mode != "area" or fx <= 1:
                out.append(pytest.param(mode, (H, W), (fx, fy), Cc, id=f"{mode}-{H}x{W}-by{fx}x{Cc}"))
    return out


def _lib():
    from wire_amd import _lib
    return _lib, _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_OPS = {}


def _op(mode, dims, factors):
    """The restatement of a case, made once and shared."""
    key = (mode, dims, factors)
    if key not in _OPS:
        _OPS[key] = ref.Resize(mode, *dims) if factors is None else ref.Resize.from_factors(mode, *dims, *factors)
    return _OPS[key]


def _tables(r):
    lib, L = _lib()
    nb = lib.check(L.wire_resize_tab_bytes(*r.geom()), "wire_resize_tab_bytes")
    assert nb == r.tab_bytes()
    tab = torch.full((nb // 4 + 16,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    lib.check(L.wire_resize_tables(_stream(), *r.geom(), tab.data_ptr()), "wire_resize_tables")
    return tab


def _apply(entry, r, tab, src, Cc, n_out):
    lib, L = _lib()
    out = torch.full((n_out + 16,), 7.0, device=DEV)
    lib.check(getattr(L, entry)(_stream(), tab.data_ptr(), *r.geom(), src.data_ptr(), Cc, out.data_ptr()), entry)
    torch.cuda.synchronize()
    assert (out[n_out:] == 7.0).all(), f"{entry} wrote past its output"
    return out[:n_out].cpu().numpy()


@pytest.mark.parametrize("mode,dims,factors,Cc", _cases())
def test_tables_forward_adjoint(mode, dims, factors, Cc):
    """Tables: every int32 equal and every fp32 weight the same bits as the restatement's, nothing written behind them.
    Forward and adjoint within the protocol bound of the fp64 oracle on unit-scale normal inputs; sources that no output
    touches receive exactly +0.0; <R x, g> = <x, R^T g> with both sides summed in fp64 from the device's outputs, within
    the protocol bound of each factor times the L1 norm of the other: sum|g| (2 err_ref_fwd + 1e-6) max|Rx| +
    sum|x| (2 err_ref_bwd + 1e-6) max|R^T g|; the same call twice gives the same bits."""
    r = _op(mode, dims, factors)
    H, W, Hl, Wl = r.H, r.W, r.Hl, r.Wl
    label = f"resize {mode} {H}x{W}->{Hl}x{Wl}x{Cc}"
    tab = _tables(r)
    got = tab.cpu().numpy()
    want = r.tab_words()
    assert (got[want.size:] == 0x7F7F7F7F).all(), "wire_resize_tables wrote past the tables"
    assert np.array_equal(got[:want.size], want), f"{label}: {(got[:want.size] != want).sum()} table words differ"

    rng = np.random.default_rng(H * 1000 + W * 10 + Hl + Cc)
    x = rng.standard_normal((H, W, Cc)).astype(np.float32)
    g = rng.standard_normal((Hl, Wl, Cc)).astype(np.float32)
    xd, gd = torch.tensor(x, device=DEV), torch.tensor(g, device=DEV)
    y = _apply("wire_resize_fwd", r, tab, xd, Cc, g.size).reshape(g.shape)
    gx = _apply("wire_resize_bwd", r, tab, gd, Cc, x.size).reshape(x.shape)
    y64, gx64 = r.fwd64(x), r.bwd64(g)
    ef, eb = relmax(r.fwd32(x), y64), relmax(r.bwd32(g), gx64)
    print(f"{label}: fwd err {relmax(y, y64):.2e} (ref {ef:.2e})  bwd err {relmax(gx, gx64):.2e} (ref {eb:.2e})")
    within_ref(relmax(y, y64), ef, label + " fwd")
    within_ref(relmax(gx, gx64), eb, label + " bwd")
    untouched = (r.v.hi < r.v.lo)[:, None] | (r.h.hi < r.h.lo)[None, :]
    assert (gx.view(np.uint32)[untouched] == 0).all(), "an untouched source did not receive +0.0"
    if mode == "nearest" and (H, Hl) == (13, 5):
        assert untouched.sum() == 13 * 17 - 5 * 7
    lhs = (y.astype(np.float64) * g).sum()
    rhs = (x.astype(np.float64) * gx).sum()
    bound = np.abs(g).sum() * (2 * ef + 1e-6) * np.abs(y64).max() + np.abs(x).sum() * (2 * eb + 1e-6) * np.abs(gx64).max()
    print(f"{label}: <Rx, g> - <x, R^T g> = {lhs - rhs:.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    assert y.tobytes() == _apply("wire_resize_fwd", r, tab, xd, Cc, g.size).tobytes()
    assert gx.tobytes() == _apply("wire_resize_bwd", r, tab, gd, Cc, x.size).tobytes()
    if (H, W) == (Hl, Wl) and r.sy == 1.0 and r.sx == 1.0:                 # the identity shape: bit-exact in every mode
        assert y.tobytes() == x.tobytes() and gx.tobytes() == g.tobytes()


def test_an_image_of_more_than_2_31_elements():
    """32769 x 65536 x 1 floats (8.6 GB): the 64-bit index kernels.  nearest at sy = 16384.5, sx = 32768 to 3 x 2 reads
    rows 0, 16384 and 32768 (clamped) and columns 0 and 32768, so output (2, 1) is the element at flat index
    2^31 + 32768; its adjoint writes all 2^31 + 65536 elements, six of them nonzero."""
    lib, L = _lib()
    H, W = 32769, 65536
    geom = (H, W, 3, 2, ref.NEAREST, 16384.5, 32768.0)
    rows, cols = [0, 16384, 32768], [0, 32768]
    tab = torch.empty(lib.check(L.wire_resize_tab_bytes(*geom), "wire_resize_tab_bytes"), dtype=torch.uint8, device=DEV)
    lib.check(L.wire_resize_tables(_stream(), *geom, tab.data_ptr()), "wire_resize_tables")
    x = torch.zeros(H, W, device=DEV)
    want = torch.arange(1.0, 7.0, device=DEV).reshape(3, 2)
    for a, i in enumerate(rows):
        for b, j in enumerate(cols):
            x[i, j] = want[a, b]
    y = torch.full((3, 2), 7.0, device=DEV)
    lib.check(L.wire_resize_fwd(_stream(), tab.data_ptr(), *geom, x.data_ptr(), 1, y.data_ptr()), "wire_resize_fwd")
    assert torch.equal(y, want)
    x.fill_(float("nan"))
    lib.check(L.wire_resize_bwd(_stream(), tab.data_ptr(), *geom, want.data_ptr(), 1, x.data_ptr()), "wire_resize_bwd")
    got = torch.stack([torch.stack([x[i, j] for j in cols]) for i in rows])
    assert torch.equal(got, want)
    assert int(torch.count_nonzero(x)) == 6 and float(x.sum(dtype=torch.float64)) == 21.0


# ---- the fused loss -------------------------------------------------------------------------------------------------------
class _Loss:
    """wire_resize_mse_grad on one case; the workspaces and outputs are tensors of this object so a test can fill them."""

    def __init__(self, r, O, seed):
        self.lib, self.L = _lib()
        self.r, self.O = r, O
        rng = np.random.default_rng(seed)
        self.y = rng.standard_normal((r.H, r.W, O)).astype(np.float32)
        self.gt = rng.standard_normal((r.Hl, r.Wl, O)).astype(np.float32)
        self.yd, self.gtd = torch.tensor(self.y, device=DEV), torch.tensor(self.gt, device=DEV)
        self.tab = _tables(r)
        wsb = self.lib.check(self.L.wire_resize_mse_grad_ws_bytes(r.Hl, r.Wl, O), "ws_bytes")
        assert wsb == 4 * self.gt.size
        self.bufs = dict(ws=torch.empty(wsb, dtype=torch.uint8, device=DEV), partial=torch.empty(1024, device=DEV),
                         g_y=torch.empty(self.y.size, device=DEV), rec=torch.empty(self.gt.size, device=DEV),
                         loss=torch.empty(1, device=DEV))

    def call(self, pattern=None, with_rec=True):
        b = self.bufs
        if pattern is not None:
            for t in b.values():
                fill(t, pattern)
        self.lib.check(self.L.wire_resize_mse_grad(
            _stream(), self.tab.data_ptr(), *self.r.geom(), self.yd.data_ptr(), self.O, self.gtd.data_ptr(),
            b["g_y"].data_ptr(), b["rec"].data_ptr() if with_rec else None, b["loss"].data_ptr(), b["ws"].data_ptr(),
            b["ws"].numel(), b["partial"].data_ptr()), "wire_resize_mse_grad")
        torch.cuda.synchronize()
        return b["loss"].clone(), b["g_y"].clone(), b["rec"].clone()

    def ref32(self):
        """The restatement in fp32: rec, the residual, the loss as an fp32 sum, the adjoint of the scaled residual."""
        rec = self.r.fwd32(self.y)
        d = rec - self.gt
        loss = np.float32(np.sum(d * d, dtype=np.float32) * np.float32(1.0 / d.size))
        return loss, self.r.bwd32(np.float32(2.0 / d.size) * d), rec

    def check(self, label):
        loss, gy, rec = self.call(ZERO)
        l64, g64, rec64 = self.r.mse_grad64(self.y, self.gt)
        l32, g32, rec32 = self.ref32()
        lossv, gyv, recv = float(loss.item()), gy.cpu().numpy().reshape(self.y.shape), rec.cpu().numpy().reshape(self.gt.shape)
        print(f"{label}: loss {lossv:.6e} rel err {abs(lossv - l64) / l64:.2e} (ref {abs(float(l32) - l64) / l64:.2e})  "
              f"g_y err {relmax(gyv, g64):.2e} (ref {relmax(g32, g64):.2e})  rec err {relmax(recv, rec64):.2e}")
        within_ref(abs(lossv - l64) / l64, abs(float(l32) - l64) / l64, label + " loss")
        within_ref(relmax(gyv, g64), relmax(g32, g64), label + " g_y")
        within_ref(relmax(recv, rec64), relmax(rec32, rec64), label + " rec_lr")
        return loss, gy, rec


@pytest.mark.parametrize("mode,dims,factors,Cc", _cases())
def test_mse_grad(mode, dims, factors, Cc):
    """loss, rec_lr and g_y within the protocol bound of the fp64 oracle; rec_lr = NULL gives the same g_y and loss bits
    and leaves rec_lr alone; the call twice gives the same bits; workspaces and outputs prefilled with 0xFF bytes and with
    2^127 leave every result unchanged; untouched sources receive +0.0."""
    r = _op(mode, dims, factors)
    c = _Loss(r, Cc, r.H * 100 + r.W + Cc)
    label = f"resize_mse_grad {mode} {r.H}x{r.W}->{r.Hl}x{r.Wl}x{Cc}"
    loss, gy, rec = c.check(label)
    for pattern in (ZERO, ONES, BIG):
        l2, g2, r2 = c.call(pattern)
        assert same_bits(l2, loss) and same_bits(g2, gy) and same_bits(r2, rec), f"{label}: differs after {pattern}"
    l3, g3, r3 = c.call(ONES, with_rec=False)
    assert same_bits(l3, loss) and same_bits(g3, gy)
    assert (r3.view(torch.int32) == -1).all()                                # rec_lr = NULL: nothing written there
    untouched = torch.tensor((r.v.hi < r.v.lo)[:, None] | (r.h.hi < r.h.lo)[None, :], device=DEV)
    assert (gy.view(torch.int32).reshape(r.H, r.W, Cc)[untouched] == 0).all()


@pytest.mark.parametrize("H,W,scale", [(16, 16, 4), (12, 18, 3)])
def test_area_and_avgpool_against_the_same_oracle(H, W, scale):
    """At an integer factor the area operator IS AvgPool2d(scale): wire_resize_mse_grad(area) and wire_avgpool_mse_grad on
    the same y and gt_lr, each against the fp64 oracle (not against each other: they add in different orders).
    wire_avgpool_mse_grad takes ONE integer scale for both axes, so the 12 x 18 image is pooled by 3 to 4 x 6 here; its
    3 x 6 target (factors 4 and 3), which only the resize kernel can reach, is a case of test_mse_grad."""
    lib, L = _lib()
    O = 3
    r = _op("area", (H, W, H // scale, W // scale), None)
    c = _Loss(r, O, H + W)
    label = f"area vs avgpool {H}x{W}/{scale}"
    c.check(label + " [resize]")
    l64, g64, _ = r.mse_grad64(c.y, c.gt)
    l32, g32, _ = c.ref32()
    gy, loss, part = torch.empty(c.y.size, device=DEV), torch.empty(1, device=DEV), torch.empty(1024, device=DEV)
    lib.check(L.wire_avgpool_mse_grad(_stream(), c.yd.data_ptr(), H, W, O, scale, c.gtd.data_ptr(), gy.data_ptr(), None,
                                      loss.data_ptr(), part.data_ptr()), "wire_avgpool_mse_grad")
    torch.cuda.synchronize()
    lossv, gyv = float(loss.item()), gy.cpu().numpy().reshape(c.y.shape)
    print(f"{label} [avgpool]: loss rel err {abs(lossv - l64) / l64:.2e}  g_y err {relmax(gyv, g64):.2e}")
    within_ref(abs(lossv - l64) / l64, abs(float(l32) - l64) / l64, label + " [avgpool] loss")
    within_ref(relmax(gyv, g64), relmax(g32, g64), label + " [avgpool] g_y")


# ---- the Python layer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_functional_resize_value_and_gradient(mode):
    """functional.resize on [H, W, C] and [H, W]: the value and img.grad against the restatement (protocol bound); the
    name and cv2's integer give the same bits; dsize is (Wl, Hl); the fx / fy form; resize_adjoint is R^T and its
    gradient is R; create_graph=True raises."""
    from wire_amd import functional
    r = _op(mode, (13, 17, 5, 7), None)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((13, 17, 3)).astype(np.float32)
    g = rng.standard_normal((5, 7, 3)).astype(np.float32)
    img = torch.tensor(x, device=DEV, requires_grad=True)
    out = functional.resize(img, (7, 5), interpolation=mode)
    assert out.shape == (5, 7, 3) and out.requires_grad
    out.backward(torch.tensor(g, device=DEV))
    within_ref(relmax(out.detach().cpu().numpy(), r.fwd64(x)), relmax(r.fwd32(x), r.fwd64(x)), f"functional.resize {mode}")
    within_ref(relmax(img.grad.cpu().numpy(), r.bwd64(g)), relmax(r.bwd32(g), r.bwd64(g)), f"functional.resize {mode} grad")
    again = functional.resize(img.detach(), (7, 5), interpolation=ref.MODES[mode])
    assert same_bits(again, out.detach())
    plane = functional.resize(img.detach()[:, :, 1].contiguous(), (7, 5), interpolation=mode)
    assert plane.shape == (5, 7) and same_bits(plane, out.detach()[:, :, 1])
    adj = functional.resize_adjoint(torch.tensor(g, device=DEV), (13, 17), (7, 5), interpolation=mode)
    assert adj.shape == (13, 17, 3) and same_bits(adj, img.grad)
    gt = torch.tensor(g, device=DEV, requires_grad=True)
    functional.resize_adjoint(gt, (13, 17), (7, 5), interpolation=mode).backward(img.detach())
    assert same_bits(gt.grad, out.detach())
    if mode != "area":
        rf = _op(mode, (5, 7), (2.6, 2.6))
        small = torch.tensor(x[:5, :7].copy(), device=DEV)
        up = functional.resize(small, None, fx=2.6, fy=2.6, interpolation=mode)
        assert up.shape == (13, 18, 3)
        within_ref(relmax(up.cpu().numpy(), rf.fwd64(x[:5, :7])), relmax(rf.fwd32(x[:5, :7]), rf.fwd64(x[:5, :7])),
                   f"functional.resize {mode} by 2.6")
    img2 = torch.tensor(x, device=DEV, requires_grad=True)
    o2 = functional.resize(img2, (7, 5), interpolation=mode)
    with pytest.raises(NotImplementedError, match="first order only"):
        torch.autograd.grad(o2.sum(), img2, create_graph=True)


def test_utils_resize_numpy_and_tensor():
    from wire_amd.modules import utils
    r = _op("area", (13, 17), (0.5, 0.5))
    cube = np.random.default_rng(4).standard_normal((13, 17, 4))
    want = r.fwd64(cube.astype(np.float32))
    out = utils.resize(cube, 0.5)
    assert isinstance(out, np.ndarray) and out.dtype == cube.dtype and out.shape == (6, 8, 4)
    ref32 = r.fwd32(cube.astype(np.float32))
    within_ref(relmax(out, want), relmax(ref32, want), "utils.resize numpy")
    t = utils.resize(torch.tensor(cube, dtype=torch.float32, device=DEV), 0.5)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.shape == (6, 8, 4)
    assert np.array_equal(t.cpu().numpy().astype(np.float64), out)
