"""CPU-only checks of the video compressive-sensing step: the numpy restatement of its loss (tests/video_cs_ref.py)
against torch ops + autograd in float64 and against the coded video the reference itself makes
(tests/golden/video_cs.npz), the host-side masks of lin_inverse.get_video_coding_frames against the reference's, and the
three new entry points' refusal of bad arguments (before any HIP call, so on a machine without a GPU)."""
import numpy as np
import pytest
import torch

from _util import ROOT, load_golden  # noqa: F401  (puts the repository on sys.path)
import video_cs_ref as ref


def _torch_coded(video, masks, nframes, dup_last):
    """(1, T, H, W) video and masks -> (1, C', H, W): every group of nframes frames of video * masks summed; with
    dup_last the last group once more."""
    T = video.shape[1]
    prod = video * masks
    frames = [prod[:, s:s + nframes].sum(1, keepdim=True) for s in range(0, T, nframes)]
    if dup_last:
        frames.append(frames[-1])
    return torch.cat(frames, dim=1)


@pytest.mark.parametrize("dup_last", [True, False])
@pytest.mark.parametrize("H,W,T,O,nframes", [(3, 4, 10, 1, 4), (2, 3, 5, 2, 8)])
def test_restatement_matches_torch(H, W, T, O, nframes, dup_last):
    """fp64 restatement == the coded video built from y.reshape(H, W, T).permute(2, 0, 1) per channel with
    ((coded - gt)**2).mean() + autograd in float64, to 1e-12 relative; mask values 0, 0.5 and 1."""
    rng = np.random.default_rng(H * 100 + T)
    NP = H * W
    Cp = ref.nchunks(T, nframes) + int(dup_last)
    y = rng.standard_normal((NP * T, O))
    gt = rng.standard_normal((Cp, NP, O))
    m = ref.make_mask(rng, NP, T).astype(np.float64)
    assert set(np.unique(m)) == {0.0, 0.5, 1.0}
    yt = torch.tensor(y, requires_grad=True)
    masks = torch.tensor(m).reshape(H, W, T).permute(2, 0, 1)[None]
    coded = torch.stack([_torch_coded(yt[:, o].reshape(H, W, T).permute(2, 0, 1)[None], masks, nframes, dup_last)[0]
                         for o in range(O)], dim=-1)                                  # (C', H, W, O)
    assert coded.shape == (Cp, H, W, O)
    loss = ((coded - torch.tensor(gt).reshape(Cp, H, W, O)) ** 2).mean()
    loss.backward()
    l64, g64, e64 = ref.coded_loss_and_grad(y, m, gt, T, nframes, dup_last, double=True)
    assert abs(loss.item() - l64) <= 1e-12 * abs(l64)
    assert np.abs(yt.grad.numpy() - g64).max() <= 1e-12 * np.abs(g64).max()
    assert np.abs(coded.detach().numpy().reshape(Cp, NP, O) - e64).max() <= 1e-12 * np.abs(e64).max()
    # pixel 0 is closed in every frame: exactly no gradient
    assert not g64[:T].any() and not yt.grad.numpy()[:T].any()
    # the fp32 restatement is the same function
    l32, g32, e32 = ref.coded_loss_and_grad(y.astype(np.float32), m.astype(np.float32), gt.astype(np.float32), T,
                                            nframes, dup_last, double=False)
    assert g32.dtype == np.float32 and e32.dtype == np.float32
    assert abs(l32 - l64) <= 1e-5 * l64 and np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max()
    # the frame-major adjoint is the same gradient for g_coded = 2 d / count
    if O == 1:
        d = (e64 - gt)[..., 0]
        gv = ref.coded_adjoint(2.0 * d / d.size, m.T, T, nframes, dup_last)           # [T, NP]
        assert np.abs(gv.T.reshape(-1, 1) - g64).max() <= 1e-12 * np.abs(g64).max()


def test_golden_coded_video_matches_restatement():
    """The coded video the reference makes has C + 1 frames, the last two equal, and equals the restatement with
    dup_last on to 1e-6 relative to its maximum."""
    z = load_golden("video_cs")
    H, W, T = (int(v) for v in z["video_size"])
    nframes = int(z["nframes"])
    C = ref.nchunks(T, nframes)
    coded = z["coded"]
    assert coded.shape == (1, C + 1, H, W)
    assert np.array_equal(coded[0, C], coded[0, C - 1])
    y = z["video"][0].transpose(1, 2, 0).reshape(H * W * T, 1)                        # row (i W + j) T + k
    est = ref.coded_estimate(y, z["masks"].reshape(H * W, T), T, nframes, dup_last=True)
    assert np.abs(est[..., 0].reshape(C + 1, H, W) - coded[0]).max() <= 1e-6 * np.abs(coded).max()
    plain = ref.coded_estimate(y, z["masks"].reshape(H * W, T), T, nframes, dup_last=False)
    assert plain.shape[0] == C and np.array_equal(plain, est[:C])


def test_coding_frames_match_reference_draw():
    """get_video_coding_frames under np.random.seed(0) == the reference's masks, exactly; every pixel is open in exactly
    one frame of each full chunk (and at most one of the ragged last one)."""
    from wire_amd.modules import lin_inverse
    z = load_golden("video_cs")
    size, nframes = tuple(int(v) for v in z["video_size"]), int(z["nframes"])
    np.random.seed(0)
    masks = lin_inverse.get_video_coding_frames(size, nframes)
    assert masks.dtype == np.float64 and masks.shape == size
    assert np.array_equal(masks, z["masks"])
    assert set(np.unique(masks)) == {0.0, 1.0}
    T = size[2]
    for c in range(T // nframes):
        assert (masks[..., c * nframes:(c + 1) * nframes].sum(-1) == 1).all()
    assert (masks[..., (T // nframes) * nframes:].sum(-1) <= 1).all()
    # a chunk as long as the video, and frames that divide it
    np.random.seed(3)
    assert (lin_inverse.get_video_coding_frames((4, 3, 8), 8).sum(-1) == 1).all()
    assert lin_inverse.get_video_coding_frames((4, 3, 8), 2).shape == (4, 3, 8)


def test_new_entry_points_refuse_bad_arguments():
    """wire_coded_mse_grad, wire_coded_fwd and wire_coded_bwd return -1 and name themselves in wire_last_error(), before
    any HIP call (NULL stream, host buffers), for T, O, nframes, n_pix or NP < 1, p0 < 0, p0 + n_pix > NP, dup_last not
    0 / 1 and a NULL pointer other than est."""
    import ctypes as C
    from wire_amd import _lib
    L = _lib.lib()
    NP, T, O = 6, 5, 2
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)

    def op(p0=0, n_pix=NP, NP=NP, T=T, O=O, nframes=2, dup=1, y=p, mask=p, gt=p, g=p, est=p, loss=p, part=p):
        return L.wire_coded_mse_grad(None, y, p0, n_pix, NP, T, O, nframes, dup, mask, gt, g, est, loss, part)

    for kw in (dict(T=0), dict(O=0), dict(nframes=0), dict(n_pix=0), dict(NP=0), dict(T=-1), dict(p0=-1),
               dict(p0=1), dict(p0=4, n_pix=3), dict(n_pix=NP + 1), dict(dup=2), dict(dup=-1), dict(y=None),
               dict(mask=None), dict(gt=None), dict(g=None), dict(loss=None), dict(part=None)):
        assert op(**kw) == -1, kw
        assert b"wire_coded_mse_grad" in L.wire_last_error()

    def fwd(fn, a=p, masks=p, T=T, NP=NP, nframes=2, dup=1, out=p):
        return fn(None, a, masks, T, NP, nframes, dup, out)

    for fn, name in ((L.wire_coded_fwd, b"wire_coded_fwd"), (L.wire_coded_bwd, b"wire_coded_bwd")):
        for kw in (dict(T=0), dict(NP=0), dict(nframes=0), dict(dup=2), dict(dup=-1), dict(a=None), dict(masks=None),
                   dict(out=None), dict(T=3, NP=1 << 40)):
            assert fwd(fn, **kw) == -1, (name, kw)
            assert name in L.wire_last_error()
