"""GPU checks of the device registration (wire_register.hip): the bilinear resampler and its coordinate gradient bit for
bit against the numpy restatement of tests/register_ref.py, functional.remap, the 29 sums and the solve of
wire_register_gn_step, its refusals and its independence of what the workspace held, and motion.register_stack_ecc end
to end against the restatement's twin and against the truth -- single start, multi-start, a frame of noise, and the
wiring into FusedTrainer.affine_coords / step_frames."""
import math

import numpy as np
import pytest
import torch

import register_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# one row; several channels and two workgroups, the second ragged; 274 workgroups
REMAP_SHAPES = [(5, 7, 1, 1), (9, 13, 3, 257), (48, 64, 3, 70001)]
# one ragged chunk; three chunks per (frame, candidate), K = 2, odd sizes; six full chunks
GN_SHAPES = [(1, 1, 20, 24), (3, 2, 61, 97), (2, 1, 96, 128)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the resampler ---------------------------------------------------------------------------------------------------
def _special_pixels(H, W):
    """Exact integers, the last row / column, the half-open border bands, far outside, NaN and infinities."""
    inf, nan = np.inf, np.nan
    return np.array([[0, 0], [1, 2], [W - 1, H - 1], [W - 1, 0.5], [0.25, H - 1], [W - 2, H - 2], [-0.5, 1], [-1e-3, 0],
                     [W - 0.5, 1.25], [W - 1 + 1e-3, H - 1 + 1e-3], [1, -0.75], [2, H - 0.25], [-1, 0], [W, 1], [0, -1],
                     [1, H], [-1 - 1e-6, 0], [-7.5, 2], [3, 1e4], [1e30, 1], [-1e38, -1e38], [nan, 1], [1, nan],
                     [nan, nan], [inf, 0], [0, -inf], [0.5, 0.5], [W - 1.5, H - 1.5]], dtype=np.float32)


def _remap_inputs(H, W, Cc, n, normalized):
    rng = np.random.default_rng(H * 1009 + W * 31 + Cc + n)
    img = rng.standard_normal((H, W, Cc)).astype(np.float32)
    xy = np.stack((rng.uniform(-2, W + 1, n), rng.uniform(-2, H + 1, n)), axis=1).astype(np.float32)
    sp = _special_pixels(H, W)
    if n >= 2 * sp.shape[0]:
        xy[:sp.shape[0]] = sp
        xy[-sp.shape[0]:] = sp[::-1]                                    # in the last, ragged workgroup too
        xy[sp.shape[0]:sp.shape[0] + 40] = np.rint(xy[sp.shape[0]:sp.shape[0] + 40])
    if normalized:
        with np.errstate(invalid="ignore", over="ignore"):
            xy = np.stack(((2 * xy[:, 0] + 1) / np.float32(W) - 1, (2 * xy[:, 1] + 1) / np.float32(H) - 1), 1).astype(np.float32)
        if n >= 8:
            xy[5:8] = [[-1, -1], [1, 1], [0, 0]]
    g = rng.standard_normal((n, Cc)).astype(np.float32)
    return img, xy, g


def _remap_dev(img, xy, g, normalized):
    from wire_amd import _lib
    L = _lib.lib()
    H, W, Cc = img.shape
    n = xy.shape[0]
    ti, tx, tg = (torch.tensor(a, device=DEV) for a in (img, xy, g))
    out = torch.full((n, Cc), 7.0, device=DEV)
    gxy = torch.full((n, 2), 7.0, device=DEV)
    _lib.check(L.wire_remap_bilinear_fwd(_stream(), ti.data_ptr(), H, W, Cc, tx.data_ptr(), n, normalized,
                                         out.data_ptr()), "remap_fwd")
    _lib.check(L.wire_remap_bilinear_bwd_xy(_stream(), ti.data_ptr(), H, W, Cc, tx.data_ptr(), tg.data_ptr(), n,
                                            normalized, gxy.data_ptr()), "remap_bwd")
    torch.cuda.synchronize()
    return out.cpu().numpy(), gxy.cpu().numpy()


@pytest.mark.parametrize("normalized", [0, 1])
@pytest.mark.parametrize("H,W,Cc,n", REMAP_SHAPES)
def test_remap_kernels_reproduce_the_restatement_bit_for_bit(H, W, Cc, n, normalized):
    if n == 1:
        img, _, g = _remap_inputs(H, W, Cc, 1, 0)
        cases = [(img, p[None].copy(), g) for p in _special_pixels(H, W)[[0, 2, 6, 9, 12, 18, 21, 26]]]
        if normalized:
            with np.errstate(invalid="ignore", over="ignore"):
                cases = [(im, ((2 * p + 1) / np.float32([W, H]) - 1).astype(np.float32), g) for im, p, g in cases]
    else:
        cases = [_remap_inputs(H, W, Cc, n, normalized)]
    nonzero = 0
    for img, xy, g in cases:
        out, gxy = _remap_dev(img, xy, g, normalized)
        want, gwant = ref.remap(img, xy, bool(normalized)), ref.remap_bwd_xy(img, xy, g, bool(normalized))
        assert np.array_equal(_bits(out), _bits(want)), np.abs(out - want).max()
        assert np.array_equal(_bits(gxy), _bits(gwant)), np.abs(gxy - gwant).max()
        assert np.isfinite(out).all() and np.isfinite(gxy).all()
        bad = ~np.isfinite(xy).all(axis=1)
        assert not out[bad].any() and not gxy[bad].any()
        nonzero += int((out != 0).sum())
    assert nonzero > 0
    if n > 1 and not normalized:
        img, xy, g = cases[0]
        out, _ = _remap_dev(img, xy, g, 0)
        assert np.array_equal(out[0], img[0, 0]) and np.array_equal(out[2], img[H - 1, W - 1])


def test_functional_remap_forward_gradient_and_refusals():
    """functional.remap against the restatement: forward bits, xy.grad bits for a random cotangent (a finite-difference
    gradcheck has no meaning in fp32), any leading shape, both modes; an image that requires grad and a second-order
    request are refused."""
    from wire_amd import functional
    H, W, Cc, n = 9, 13, 3, 257
    for normalized in (False, True):
        img, xy, g = _remap_inputs(H, W, Cc, n + 1, int(normalized))
        ti = torch.tensor(img, device=DEV)
        tx = torch.tensor(xy.reshape(2, 129, 2), device=DEV, requires_grad=True)
        out = functional.remap(ti, tx, normalized=normalized)
        assert out.shape == (2, 129, Cc) and out.dtype == torch.float32
        (out * torch.tensor(g.reshape(2, 129, Cc), device=DEV)).sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.detach().cpu().numpy().reshape(-1, Cc)), _bits(ref.remap(img, xy, normalized)))
        assert np.array_equal(_bits(tx.grad.cpu().numpy().reshape(-1, 2)), _bits(ref.remap_bwd_xy(img, xy, g, normalized)))
    with pytest.raises(NotImplementedError, match="adjoint with respect to the image"):
        functional.remap(ti.clone().requires_grad_(), tx)
    out = functional.remap(ti, tx)
    with pytest.raises(NotImplementedError, match="first order only"):
        torch.autograd.grad(out.sum(), tx, create_graph=True)
    with pytest.raises(ValueError, match="C in 1..8"):
        functional.remap(torch.zeros(4, 4, 9, device=DEV), tx.detach())
    with pytest.raises(ValueError, match=r"\[\.\.\., 2\]"):
        functional.remap(ti, torch.zeros(5, 3, device=DEV))


# ---- one Gauss-Newton iteration ----------------------------------------------------------------------------------------
def _gn_inputs(B, K, H, W, weighted):
    """Frames of the synthetic image under known motions; candidate 0 near the truth, candidate 1 (or, with K = 1, every
    odd frame) far from it: a rotation of 0.4 rad about the centre and a shift."""
    rng = np.random.default_rng(B * 1000 + K * 100 + H)
    truth = np.stack([ref.euclid(0, (0, 0))] + [ref.euclid(rng.uniform(-0.05, 0.05), rng.uniform(-3, 3, 2))
                                                 for _ in range(B)])
    st = ref.synth_stack(H, W, truth, 1, seed=H)
    near = truth[1:] + rng.uniform(-1, 1, (B, 2, 3)) * np.array([2e-3, 2e-3, 0.4])
    far = ref.seed_mats([0.4], H, W)[0] + np.array([[0, 0, 4.0], [0, 0, -3.0]])
    mats = np.zeros((B, K, 2, 3))
    for b in range(B):
        for k in range(K):
            mats[b, k] = far if (k == 1 or (K == 1 and b % 2 == 1)) else near[b]
    weight = None
    if weighted:
        weight = rng.choice(np.array([0, 0.5, 1, 2], dtype=np.float32), size=(B, H, W))
    return st[0], st[1:], weight, mats


def _gn_dev(r, f, w, mats, model, damping=0.0, min_cover=0.0, fill=0, calls=1):
    from wire_amd import _lib
    L = _lib.lib()
    B, K = mats.shape[:2]
    H, W = r.shape
    tr, tf = torch.tensor(r, device=DEV), torch.tensor(f, device=DEV)
    tw = None if w is None else torch.tensor(w, device=DEV)
    tm = torch.tensor(mats, dtype=torch.float64, device=DEV)
    stats = torch.full((B, K, 4), 7.0, dtype=torch.float64, device=DEV)
    nb = _lib.check(L.wire_register_gn_ws_bytes(B, K, H, W), "ws_bytes")
    ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
    for _ in range(calls):
        _lib.check(L.wire_register_gn_step(_stream(), tr.data_ptr(), tf.data_ptr(), None if tw is None else tw.data_ptr(),
                                           B, K, H, W, model, damping, min_cover, tm.data_ptr(), stats.data_ptr(),
                                           ws.data_ptr(), nb), "gn_step")
    torch.cuda.synchronize()
    S = ws.view(torch.float64)[:B * K * ref.NSUM].reshape(B, K, ref.NSUM).cpu().numpy()
    return tm.cpu().numpy(), stats.cpu().numpy(), S


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,K,H,W", GN_SHAPES)
def test_gn_sums_and_solve(B, K, H, W, weighted):
    """All 29 sums (read from the head of ws) against the restatement's exactly added terms, within
    c 2^-52 sum |terms|, c = (8 + 6 + 2 + ceil(chunks / 64) + 6 + 2) / 2 (every addition a term passes
    through rounds by 2^-53 of the partial sum -- the thread's chain of 8, 6 shuffle levels, 2 levels over the waves, the
    chunk chain, 6 shuffle levels -- plus the restatement's own rounding and the product's; the terms themselves have the
    restatement's bits).  Then the updated matrix against the restatement's solve OF THE KERNEL'S OWN SUMS, 1e-12
    relative, for the three models; the stats likewise."""
    r, f, w, mats = _gn_inputs(B, K, H, W, weighted)
    want_S, A = ref.gn_sums(r, f, w, mats)
    chunks = (H * W - 1) // 2048 + 1
    c = (8 + 6 + 2 + math.ceil(chunks / 64) + 6 + 2) / 2
    worst = 0.0
    for model in (0, 1, 2):
        out, stats, S = _gn_dev(r, f, w, mats, model, damping=1e-6, min_cover=0.05)
        err = np.abs(S - want_S)
        bound = c * 2.0 ** -52 * A
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
        worst = max(worst, (err[A > 0] / bound[A > 0]).max())
        assert (A > 0).all() and np.isfinite(S).all()
        for b in range(B):
            for k in range(K):
                wm, ws_ = ref.gn_solve(S[b, k], mats[b, k], H, W, model, 1e-6, 0.05)
                rel = np.abs(out[b, k] - wm).max() / np.abs(wm).max()
                assert rel <= 1e-12, (model, b, k, rel)
                assert ws_[3] == 1 and stats[b, k, 3] == 1 and not np.array_equal(out[b, k], mats[b, k])
                assert np.abs(stats[b, k] - ws_).max() <= 1e-12 * np.abs(ws_).max()
                if model == 0:
                    assert np.array_equal(out[b, k, :, :2], mats[b, k, :, :2])
                if model == 1:
                    assert abs(out[b, k, 0, 0] ** 2 + out[b, k, 1, 0] ** 2 - 1) <= 1e-15
        if weighted:
            assert (stats[..., 1] < 1).all()
    print(f"gn sums ({B}, {K}, {H}, {W}) weighted={weighted}: worst measured / bound {worst:.3f} (c = {c})")


@pytest.mark.parametrize("B,K,H,W", GN_SHAPES[1:])
def test_gn_step_is_bit_stable_and_ignores_the_workspace(B, K, H, W):
    r, f, w, mats = _gn_inputs(B, K, H, W, True)
    first = _gn_dev(r, f, w, mats, 1, 1e-6, 0.05, fill=0)
    for fill in (0, 0xFF):
        again = _gn_dev(r, f, w, mats, 1, 1e-6, 0.05, fill=fill)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("model", [0, 1, 2])
def test_gn_step_refuses_what_it_cannot_solve(model):
    """A frame of zeros, a weight of zeros and a matrix that maps everything outside: valid = 0, the matrix untouched, no
    NaN anywhere; a covered fraction below min_cover likewise; the other frame of the same call is solved."""
    B, K, H, W = 2, 2, 61, 97
    r, f, w, mats = _gn_inputs(B, K, H, W, True)
    outside = mats.copy()
    outside[0, :, :, 2] += 1e5
    zf = f.copy()
    zf[0] = 0
    zw = w.copy()
    zw[0] = 0
    for frames, weight, M, cover in ((zf, w, mats, 0.0), (f, zw, mats, 0.0), (f, w, outside, 0.0), (zf, None, mats, 0.0)):
        out, stats, S = _gn_dev(r, frames, weight, M, model, 1e-6, cover)
        assert np.isfinite(out).all() and np.isfinite(stats).all() and np.isfinite(S).all()
        assert out[0].tobytes() == M[0].tobytes() and not stats[0, :, 3].any() and not S[0].any()
        assert not stats[0, :, :3].any()
        assert stats[1, :, 3].all() and (out[1] != M[1]).any()
    # candidate 1 (rotated by 0.4 rad) covers less of the reference than candidate 0
    _, st0, _ = _gn_dev(r, f, None, mats, model, 1e-6, 0.0)
    assert (st0[:, 1, 1] < st0[:, 0, 1]).all()
    cut = (st0[:, 1, 1].max() + st0[:, 0, 1].min()) / 2
    out, stats, _ = _gn_dev(r, f, None, mats, model, 1e-6, cut)
    assert stats[:, 0, 3].all() and not stats[:, 1, 3].any() and out[:, 1].tobytes() == mats[:, 1].tobytes()
    assert np.array_equal(stats[:, 1, :2], st0[:, 1, :2])


def test_euclidean_updates_stay_rotations():
    """30 in-place Euclidean calls: m00^2 + m10^2 = 1 to 1e-15, m11 = m00, m01 = -m10, and the near candidate converges."""
    B, K, H, W = 3, 2, 61, 97
    r, f, _, mats = _gn_inputs(B, K, H, W, False)
    out, stats, _ = _gn_dev(r, f, None, mats, 1, 1e-6, 0.05, calls=30)
    assert (np.abs(out[..., 0, 0] ** 2 + out[..., 1, 0] ** 2 - 1) <= 1e-15).all()
    assert np.array_equal(out[..., 0, 0], out[..., 1, 1]) and np.array_equal(out[..., 0, 1], -out[..., 1, 0])
    assert (stats[:, 0, 2] < 1e-4).all() and stats[:, 0, 3].all()


def test_functional_register_gn_step_is_the_entry_point():
    from wire_amd import functional
    B, K, H, W = 3, 2, 61, 97
    r, f, w, mats = _gn_inputs(B, K, H, W, True)
    want_m, want_s, _ = _gn_dev(r, f, w, mats, 2, 1e-6, 0.05)
    tm = torch.tensor(mats, dtype=torch.float64, device=DEV)
    stats = functional.register_gn_step(torch.tensor(r, device=DEV), torch.tensor(f, device=DEV), tm,
                                        torch.tensor(w, device=DEV), "affine", 1e-6, 0.05)
    torch.cuda.synchronize()
    assert tm.cpu().numpy().tobytes() == want_m.tobytes() and stats.cpu().numpy().tobytes() == want_s.tobytes()
    with pytest.raises(ValueError, match="mats must be"):
        functional.register_gn_step(torch.tensor(r, device=DEV), torch.tensor(f, device=DEV), tm.float())
    with pytest.raises(ValueError, match="frames must be"):
        functional.register_gn_step(torch.tensor(r, device=DEV), torch.tensor(f[:, :-1], device=DEV).contiguous(), tm)


# ---- end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euclidean", "affine"])
def test_register_stack_ecc_matches_the_twin_and_the_truth(method):
    """The host test's stack: per frame, the corner displacement between the device's matrices and the twin's is at most
    a tenth of the twin's own corner error against the truth (the arithmetic sits below the method's discretisation
    floor), and the device's error against the truth is < 0.05 px."""
    from wire_amd.modules import motion
    H, W = ref.HOST_SHAPE
    truth = ref.host_motions()
    tmask, tecc, terr = ref.host_case(method)
    Xs, Ys, mask, ecc, err = motion.register_stack_ecc(ref.host_stack(), (H, W), method=method, levels=3, iters=30)
    twin_err = ref.corner_error(tecc, truth, H, W)
    disp = ref.corner_error(ecc, tecc, H, W)
    dev_err = ref.corner_error(ecc, truth, H, W)
    print(f"register_stack_ecc {method}: vs twin {disp[1:].max():.3e} px (twin's own error {twin_err[1:].min():.4f} .. "
          f"{twin_err[1:].max():.4f}), vs truth {dev_err.max():.4f} px")
    assert mask.tolist() == [1] * 7 and np.array_equal(ecc[0], [[1, 0, 0], [0, 1, 0]]) and ecc.dtype == np.float64
    assert (disp[1:] <= 0.1 * twin_err[1:]).all()
    assert dev_err.max() < 0.05
    assert np.abs(err - terr).max() <= 1e-5 and err[0] == 0
    assert Xs.shape == Ys.shape == (7, 48, 64) and Xs.dtype == np.float32
    wx, wy = motion._centre_coords(ecc, (H, W), (48, 64))
    assert np.array_equal(Xs, wx) and np.array_equal(Ys, wy)
    assert abs(Xs[0, 0, 0] - (2 * 0.5 / W - 1)) < 1e-7 and abs(Ys[0, -1, 0] - (2 * (H - 1.5) / H - 1)) < 1e-7
    # the cv2 integers name the same models, and a channel axis is averaged away
    code = {"euclidean": 1, "affine": 2}[method]
    _, _, _, ecc2, _ = motion.register_stack_ecc(np.repeat(ref.host_stack()[:3, None], 3, axis=1), (H, W), method=code)
    assert np.abs(ecc2 - ecc[:3]).max() < 1e-4


def test_register_stack_ecc_multi_start():
    """192 x 256 pooled by 4, |angle| up to pi / 12, seven seeds: the device resolves to < 0.1 px every frame the twin
    resolves, and among those is one that a single start at the identity leaves further than 1 px from the truth."""
    from wire_amd.modules import motion
    H, W = ref.MULTI_SHAPE
    truth, tmask, tecc, e, e1 = ref.multi_start_case()
    good = e < 0.1
    assert good[1:].sum() >= 4 and (e1[good] > 1.0).any()
    _, _, mask, ecc, _ = motion.register_stack_ecc(ref.multi_stack(), (H, W), method="euclidean", levels=3, iters=30,
                                                   seeds=ref.MULTI_SEEDS)
    dev = ref.corner_error(ecc, truth, H, W)
    print(f"multi-start: device {dev[1:].round(4).tolist()}, twin {e[1:].round(4).tolist()}, "
          f"identity only (twin) {e1[1:].round(2).tolist()}")
    assert (dev[good] < 0.1).all() and mask[good].all()


def test_noise_frame_is_flagged_and_pruned():
    from wire_amd.modules import motion
    H, W = ref.HOST_SHAPE
    noise = np.random.default_rng(1).uniform(0.02, 1.0, (1, 48, 64)).astype(np.float32)
    stack = np.concatenate((ref.host_stack(), noise))
    _, _, mask, ecc, err = motion.register_stack_ecc(stack, (H, W), levels=3, iters=30)
    print(f"alignment_err: registered {err[1:-1].round(5).tolist()}, noise {err[-1]:.4f}, mask {mask.tolist()}")
    assert mask[:-1].all() and err[-1] >= 5 * err[1:-1].max() and err[1:-1].min() > 0
    kept, kept_mats, keep, imdiff = motion.prune_stack(stack, ecc, (H, W), thres=0.5)
    assert keep.tolist() == [True] * 7 + [False]
    assert kept.shape == (7, 48, 64) and kept_mats.shape == (7, 2, 3) and imdiff.shape == (7, 48, 64)
    assert np.array_equal(kept, stack[:-1]) and np.array_equal(kept_mats, ecc[:-1]) and not imdiff[0].any()


def test_registered_matrices_feed_the_trainer():
    """register_stack_ecc -> ecc_mats -> FusedTrainer.affine_coords -> step_frames: the coordinates of the recovered
    matrices are within 2 * 0.05 / min(H, W) of those of the true ones, and one step on them returns a finite loss."""
    from wire_amd.modules import models, motion
    from wire_amd.trainer import FusedTrainer
    H, W = ref.HOST_SHAPE
    truth = ref.host_motions()
    stack = ref.host_stack()
    _, _, mask, ecc, _ = motion.register_stack_ecc(stack, (H, W))
    torch.manual_seed(0)
    model = models.get_INR(nonlin="wire", in_features=2, out_features=3, hidden_features=64, hidden_layers=1).to(DEV)
    tr = FusedTrainer(model, (H, W), None, lr=1e-3)
    got, want = tr.affine_coords(ecc), tr.affine_coords(truth)
    diff = (got - want).abs().max().item()
    print(f"affine_coords(ecc_mats) vs the truth: {diff:.3e} (bound {2 * 0.05 / min(H, W):.3e})")
    assert diff < 2 * 0.05 / min(H, W)
    gt = torch.tensor(np.repeat(stack.reshape(7, -1, 1), 3, axis=2), device=DEV).contiguous()
    loss = tr.step_frames(got, gt, 2)
    torch.cuda.synchronize()
    assert math.isfinite(loss.item()) and loss.item() > 0
    # interp_lr is the reference's body on the same resampler
    class R:
        integrator = torch.nn.AvgPool2d(2)
    ref0 = torch.tensor(stack[0], device=DEV)[None, None]
    lr = motion.interp_lr(ref0, got[:2].reshape(2, H, W, 2), R)
    want_lr = R.integrator(torch.nn.functional.grid_sample(ref0.repeat(2, 1, 1, 1), got[:2].reshape(2, H, W, 2),
                                                            mode="bilinear", align_corners=False))
    assert lr.shape == (2, 1, H // 2, W // 2) and (lr - want_lr).abs().max().item() < 1e-5
