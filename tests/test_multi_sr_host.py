"""CPU-only checks of the multi-image super-resolution step: the numpy restatement of its loss against torch, the two new
entry points' refusal of bad arguments (before any HIP call, so on a machine without a GPU), and the data helpers of
wire_amd/modules/motion.py against closed forms."""
import numpy as np
import pytest
import torch

from _util import ROOT  # noqa: F401  (puts the repository on sys.path)
import multi_sr_ref as ref


@pytest.mark.parametrize("B,H,W,O,scale", [(3, 10, 13, 3, 4), (1, 8, 8, 1, 2)])
def test_restatement_matches_torch(B, H, W, O, scale):
    """fp64 restatement == AvgPool2d(scale) + MSELoss()(output*mask, gt*mask) + autograd in float64, to 1e-12 relative;
    mask values 0, 1 and 0.5 with one frame masked entirely (B = 1: a third of its pixels)."""
    rng = np.random.default_rng(B * 100 + H)
    H2, W2 = H // scale, W // scale
    y = rng.standard_normal((B, H * W, O))
    gt = rng.standard_normal((B, H2 * W2, O))
    m = ref.make_mask(rng, B, H2 * W2, O).astype(np.float64)
    assert set(np.unique(m)) == {0.0, 0.5, 1.0}
    yt = torch.tensor(y, requires_grad=True)
    out_hr = yt.reshape(-1, H, W, O).permute(0, 3, 1, 2)
    out = torch.nn.AvgPool2d(scale)(out_hr).permute(0, 2, 3, 1).reshape(-1, H2 * W2, O)
    mt = torch.tensor(m)
    loss = torch.nn.MSELoss()(out * mt, torch.tensor(gt) * mt)
    loss.backward()
    l64, g64, r64 = ref.frames_loss_and_grad(y, B, H, W, scale, gt, m, double=True)
    assert abs(loss.item() - l64) <= 1e-12 * abs(l64)
    assert np.abs(yt.grad.numpy() - g64).max() <= 1e-12 * np.abs(g64).max()
    assert np.abs(out.detach().numpy() - r64).max() <= 1e-12 * np.abs(r64).max()
    if B == 1:
        # one frame, masked entirely: exactly no loss and no gradient on both sides
        z = torch.zeros_like(mt)
        yz = torch.tensor(y, requires_grad=True)
        oz = torch.nn.AvgPool2d(scale)(yz.reshape(-1, H, W, O).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).reshape(-1, H2 * W2, O)
        lz = torch.nn.MSELoss()(oz * z, torch.tensor(gt) * z)
        lz.backward()
        l0, g0, _ = ref.frames_loss_and_grad(y, B, H, W, scale, gt, np.zeros_like(m))
        assert lz.item() == 0.0 == l0 and not yz.grad.numpy().any() and not g0.any()
    # the fp32 restatement is the same function
    l32, g32, r32 = ref.frames_loss_and_grad(y.astype(np.float32), B, H, W, scale, gt.astype(np.float32),
                                             m.astype(np.float32), double=False)
    assert g32.dtype == np.float32 and abs(l32 - l64) <= 1e-5 * l64
    assert np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max()
    # no mask == a mask of ones
    a = ref.frames_loss_and_grad(y, B, H, W, scale, gt, None)
    b = ref.frames_loss_and_grad(y, B, H, W, scale, gt, np.ones_like(gt))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_new_entry_points_refuse_bad_arguments():
    """wire_avgpool_mse_grad_frames and wire_affine_coords return a negative status, before any HIP call, for
    scale = 0, scale = H + 1, B = 0 and a NULL y / mats / coords."""
    import ctypes as C
    from wire_amd import _lib
    L = _lib.lib()
    B, H, W, O = 2, 8, 12, 3
    buf = (C.c_float * (B * H * W * O))()
    p = C.addressof(buf)

    def frames(B=B, H=H, W=W, O=O, scale=2, y=p, gt=p, mask=p, g=p, rec=p, loss=p, part=p):
        return L.wire_avgpool_mse_grad_frames(None, y, B, H, W, O, scale, gt, mask, g, rec, loss, part)

    for kw in (dict(scale=0), dict(scale=H + 1), dict(scale=W + 1, H=W + 4), dict(B=0), dict(O=0), dict(y=None),
               dict(gt=None), dict(g=None), dict(loss=None), dict(part=None)):
        assert frames(**kw) == -1, kw
        assert b"wire_avgpool_mse_grad_frames" in L.wire_last_error()
    mats = (C.c_double * (B * 6))()
    pm = C.addressof(mats)
    for args in ((None, B, H, W, p), (pm, 0, H, W, p), (pm, B, 0, W, p), (pm, B, H, 0, p), (pm, B, H, W, None)):
        assert L.wire_affine_coords(None, *args) == -1, args
        assert b"wire_affine_coords" in L.wire_last_error()


def test_image_sr_dataset_tuple_and_element_order():
    from wire_amd.modules import motion
    nimg, Hl, Wl, H, W = 3, 4, 5, 8, 10
    imstack = np.arange(nimg * 3 * Hl * Wl, dtype=np.float32).reshape(nimg, 3, Hl, Wl)
    X = np.arange(nimg * H * W, dtype=np.float32).reshape(nimg, H, W)
    Y = -X
    masks = (imstack % 2).astype(np.float32)
    ds = motion.ImageSRDataset(imstack, X, Y, masks, jitter=False)
    assert len(ds) == nimg and (ds.H, ds.W) == (Hl, Wl) and ds.xjitter == 1 / Wl and ds.yjitter == 1 / Hl
    coords, pixels, mask = ds[1]
    assert coords.shape == (H * W, 2) and pixels.shape == (Hl * Wl, 3) and mask.shape == (Hl * Wl, 3)
    # img[None].permute(0, 2, 3, 1).view(-1, 3): row i*Wl + j holds the three channels of pixel (i, j)
    for (i, j) in ((0, 0), (2, 3), (3, 4)):
        np.testing.assert_array_equal(pixels[i * Wl + j].numpy(), imstack[1, :, i, j])
        np.testing.assert_array_equal(mask[i * Wl + j].numpy(), masks[1, :, i, j])
    np.testing.assert_array_equal(coords[:, 0].numpy(), X[1].ravel())
    np.testing.assert_array_equal(coords[:, 1].numpy(), Y[1].ravel())
    # stacks that were not given come back as zeros(1); get_indices appends the index
    c0, p0, m0, idx = motion.ImageSRDataset(imstack, get_indices=True)[2]
    assert idx == 2 and c0.shape == (1,) and m0.shape == (1,) and float(c0) == 0.0 and p0.shape == (Hl * Wl, 3)
    # a DataLoader batches the tuple as the driver reads it
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2)))
    assert batch[0].shape == (2, H * W, 2) and batch[1].shape == (2, Hl * Wl, 3) and batch[2].shape == (2, Hl * Wl, 3)


def test_rigid_matrices_invert_to_identity():
    from wire_amd.modules import motion
    thetas = [0.0, np.pi / 10, -np.pi / 12, 1.3]
    shifts = [(0, 0), (20, -7), (-3.5, 12), (1e3, -1e3)]
    mats = np.stack([motion.getEuclidianMatrix(t, s) for t, s in zip(thetas, shifts)])
    assert mats.shape == (4, 2, 3)
    np.testing.assert_allclose(mats[1], [[np.cos(np.pi / 10), -np.sin(np.pi / 10), 20],
                                         [np.sin(np.pi / 10), np.cos(np.pi / 10), -7]], rtol=0, atol=0)
    inv = motion.invert_regstack(mats)
    assert inv.shape == mats.shape
    last = np.array([[0.0, 0.0, 1.0]])
    for a, b in zip(mats, inv):
        prod = np.vstack((b, last)) @ np.vstack((a, last))
        assert np.abs(prod - np.eye(3)).max() <= 1e-12 * max(1.0, np.abs(a).max())
    ang, tr = motion.affine2rigid(mats)
    np.testing.assert_allclose(ang, np.abs(thetas), atol=1e-12)
    np.testing.assert_array_equal(tr, mats[:, :, 2])


def test_xy_mgrid_and_transformed_coords():
    from wire_amd.modules import motion
    g = motion.xy_mgrid(3, 5)
    want = [(x, y) for y in (-1.0, 0.0, 1.0) for x in (-1.0, -0.5, 0.0, 0.5, 1.0)]
    assert g.dtype == torch.float32 and g.shape == (15, 2)
    np.testing.assert_array_equal(g.numpy(), np.array(want, np.float32))
    # the identity: affine_grid's pixel centres (align_corners=False), x fastest
    c = motion.get_transformed_coords(torch.tensor([[[1.0, 0, 0], [0, 1.0, 0]]] * 2), (2, 4))
    assert c.shape == (2, 8, 2)
    np.testing.assert_allclose(c[1, :, 0].numpy(), [-0.75, -0.25, 0.25, 0.75] * 2, atol=1e-7)
    np.testing.assert_allclose(c[1, :, 1].numpy(), [-0.5] * 4 + [0.5] * 4, atol=1e-7)


def test_coordinate_restatement_closed_form():
    """The restatement of the coordinate stack: frame 0 (the identity) is 2 j / W - 1, 2 i / H - 1."""
    H, W = 4, 6
    c = ref.affine_coords(np.array([[[1.0, 0, 0], [0, 1.0, 0]], [[0.0, -1.0, 2.0], [1.0, 0.0, -1.0]]]), H, W)
    i, j = np.mgrid[:H, :W]
    np.testing.assert_array_equal(c[0, :, 0], (2.0 * j / W - 1).ravel())
    np.testing.assert_array_equal(c[0, :, 1], (2.0 * i / H - 1).ravel())
    np.testing.assert_array_equal(c[1, :, 0], (2.0 * (2.0 - i) / W - 1).ravel())
    np.testing.assert_array_equal(c[1, :, 1], (2.0 * (j - 1.0) / H - 1).ravel())
