"""CPU-only checks of the resize operator (wire_resize.hip, functional.resize, utils.resize, FusedTrainer.step_resized):
the restatement of tests/resize_ref.py against torch.nn.functional.interpolate / avg_pool2d in fp64, the structure of
its tables (rows that sum to 1, the identity, the adjoint's ranges), cv2's size rule, the declarations and bindings of the
six entry points, and every refusal that comes before the first HIP call or device access."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import ROOT
import resize_ref as ref

GEOM = ["H", "W", "Hl", "Wl", "mode", "sy", "sx"]
WANT = {
    "wire_resize_tab_bytes": ("int64_t", GEOM),
    "wire_resize_mse_grad_ws_bytes": ("int64_t", ["Hl", "Wl", "O"]),
    "wire_resize_tables": ("int", ["stream"] + GEOM + ["tab"]),
    "wire_resize_fwd": ("int", ["stream", "tab"] + GEOM + ["x", "C", "y"]),
    "wire_resize_bwd": ("int", ["stream", "tab"] + GEOM + ["g_y", "C", "g_x"]),
    "wire_resize_mse_grad": ("int", ["stream", "tab"] + GEOM + ["y", "O", "gt_lr", "g_y", "rec_lr", "loss_out", "ws",
                                                                "ws_bytes", "partial"]),
}
PAIRS = [(12, 18, 3, 6), (13, 17, 5, 7), (5, 7, 13, 20), (16, 16, 16, 16), (9, 4, 2, 1)]
AXES = [(13, 5), (17, 7), (5, 13), (64, 9), (7, 7), (100, 33)]


# ---- the restatement against torch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,Hl,Wl", PAIRS)
@pytest.mark.parametrize("mode,tmode", [("nearest", "nearest"), ("linear", "bilinear"), ("cubic", "bicubic")])
def test_restatement_is_interpolate(mode, tmode, H, W, Hl, Wl):
    """The unrounded fp64 tables against F.interpolate(align_corners=False) in fp64 on unit-scale normal inputs: 1e-12."""
    x = np.random.default_rng(H * 100 + W).standard_normal((H, W, 3))
    t = torch.tensor(x).permute(2, 0, 1)[None]
    kw = {} if tmode == "nearest" else dict(align_corners=False)
    want = F.interpolate(t, size=(Hl, Wl), mode=tmode, **kw)[0].permute(1, 2, 0).numpy()
    got = ref.Resize(mode, H, W, Hl, Wl).fwd64(x, rounded=False)
    err = np.abs(got - want).max()
    print(f"{mode} {H}x{W} -> {Hl}x{Wl}: max |restatement - interpolate| {err:.2e}")
    assert err <= 1e-12


def test_restatement_area_is_avg_pool():
    x = np.random.default_rng(5).standard_normal((12, 18, 2))
    want = F.avg_pool2d(torch.tensor(x).permute(2, 0, 1)[None], (4, 3))[0].permute(1, 2, 0).numpy()
    err = np.abs(ref.Resize("area", 12, 18, 3, 6).fwd64(x, rounded=False) - want).max()
    print(f"area 12x18 -> 3x6: max |restatement - avg_pool2d| {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("n_in,n_out", [(13, 5), (17, 7), (64, 9), (7, 7), (100, 33), (12, 3), (130, 61)])
def test_area_rows_sum_to_one(n_in, n_out):
    ax = ref.Axis("area", n_in, n_out, n_in / n_out)
    assert np.abs(ax.w64.sum(1) - 1).max() <= 1e-12 and (ax.w64[ax.w64 != 0] > 0).all()
    assert ax.count.max() == ax.K and (ax.count >= 1).all()


@pytest.mark.parametrize("mode", sorted(ref.MODES))
def test_equal_sizes_give_one_tap_of_weight_one(mode):
    ax = ref.Axis(mode, 7, 7, 1.0)
    assert ax.K == 1 and ax.count.tolist() == [1] * 7 and ax.start.tolist() == list(range(7))
    assert ax.w.view(np.uint32).tolist() == [[0x3F800000]] * 7
    assert ax.lo.tolist() == list(range(7)) and ax.hi.tolist() == list(range(7))


@pytest.mark.parametrize("n_in,n_out", AXES)
@pytest.mark.parametrize("mode", sorted(ref.MODES))
def test_ranges_are_the_outputs_whose_run_contains_the_source(mode, n_in, n_out):
    if mode == "area" and n_out > n_in:
        with pytest.raises(ValueError):
            ref.Axis(mode, n_in, n_out, n_in / n_out)
        return
    ax = ref.Axis(mode, n_in, n_out, n_in / n_out)
    end = ax.start + ax.count
    assert (np.diff(ax.start) >= 0).all() and (np.diff(end) >= 0).all()
    assert ax.start.min() >= 0 and end.max() <= n_in
    for i in range(n_in):
        touching = [d for d in range(n_out) if ax.start[d] <= i < end[d]]
        assert list(range(ax.lo[i], ax.hi[i] + 1)) == touching, (i, ax.lo[i], ax.hi[i], touching)
    assert int(ax.count.sum()) == int((ax.hi - ax.lo + 1).sum())
    # the dense matrix' transpose is what the ranges gather
    R = ax.dense()
    for i in range(n_in):
        assert np.array_equal(np.nonzero(R[:, i])[0], [d for d in range(ax.lo[i], ax.hi[i] + 1) if R[d, i] != 0])
    if mode == "nearest" and (n_in, n_out) == (13, 5):
        assert int((ax.hi < ax.lo).sum()) == 8                             # 8 of 13 sources are untouched


def test_size_from_factors_rounds_half_to_even():
    from wire_amd import functional
    assert ref.out_size(5, 0.5) == 2 and ref.out_size(7, 0.5) == 4 and ref.out_size(13, 0.5) == 6
    assert ref.out_size(5, 2.6) == 13 and ref.out_size(7, 2.6) == 18
    assert functional.resize_geometry(5, 7, None, 0.5, 0.5, "area") == (5, 7, 2, 4, 3, 2.0, 2.0)
    r = ref.Resize.from_factors("area", 5, 7, 0.5, 0.5)
    assert (r.Hl, r.Wl, r.sy, r.sx) == (2, 4, 2.0, 2.0)
    # 5 sources at scale 2 into 2 outputs: the cells [0, 2) and [2, 4); source 4 is untouched
    assert r.v.start.tolist() == [0, 2] and r.v.count.tolist() == [2, 2] and r.v.hi[4] < r.v.lo[4]
    assert functional.resize_geometry(12, 18, (6, 3), None, None, 2) == (12, 18, 3, 6, 2, 4.0, 3.0)   # dsize = (Wl, Hl)
    assert functional.resize_geometry(12, 18, (0, 0), 0.5, 0.25, "nearest") == (12, 18, 3, 9, 0, 4.0, 2.0)
    assert [functional._resize_mode(m) for m in ("nearest", "linear", "cubic", "area", 0, 1, 2, 3)] == [0, 1, 2, 3] * 2


# ---- declarations and bindings ----------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_lib_lists_them():
    from wire_amd import _lib
    text = open(os.path.join(ROOT, "include", "wire_hip.h")).read()
    L = _lib.lib()
    for name, (ret, params) in WANT.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), text)
        assert m, f"include/wire_hip.h does not declare {ret} {name}"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == params
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(params)
    assert L.wire_resize_tab_bytes.restype is C.c_int64 and L.wire_resize_mse_grad_ws_bytes.restype is C.c_int64
    assert L.wire_resize_fwd.argtypes[7] is C.c_double and L.wire_resize_fwd.argtypes[8] is C.c_double
    for k, v in dict(NEAREST=0, LINEAR=1, CUBIC=2, AREA=3).items():
        assert re.search(r"WIRE_RESIZE_%s\s*=\s*%d\b" % (k, v), text)
    assert _lib.RESIZE_MODE == ref.MODES
    assert "wire_resize.hip" in open(os.path.join(ROOT, "wire_amd", "csrc", "Makefile")).read()
    for word in ("by construction", "1e-3", "refused"):                     # the three cv2 caveats
        assert word in text[text.index("Image-to-image resampling"):text.index("typedef enum wire_resize_mode")]


def test_size_queries_return_the_restatements_sizes():
    from wire_amd import _lib
    L = _lib.lib()
    for mode in range(4):
        for H, W, Hl, Wl in PAIRS + [(70, 130, 33, 61), (64, 9, 9, 9), (1, 1, 1, 1)]:
            if mode == ref.AREA and (Hl > H or Wl > W):
                continue
            r = ref.Resize(mode, H, W, Hl, Wl)
            assert L.wire_resize_tab_bytes(*r.geom()) == r.tab_bytes(), (mode, H, W, Hl, Wl)
        for fx, fy in ((0.5, 0.5), (2.6, 2.6)):
            if mode == ref.AREA and fx > 1:
                continue
            r = ref.Resize.from_factors(mode, 13, 17, fx, fy)
            assert L.wire_resize_tab_bytes(*r.geom()) == r.tab_bytes()
    assert ref.Resize("area", 64, 9, 9, 9).v.K == 8                          # eight-tap area rows
    assert L.wire_resize_mse_grad_ws_bytes(5, 7, 3) == 4 * 5 * 7 * 3


def test_entry_points_refuse_bad_arguments():
    """A side < 1, C < 1, an unknown mode, area up-scaling, a scale that is not finite or <= 0, sizes beyond 63 bits, a ws
    that is too small, a NULL pointer other than rec_lr: WIRE_ERR_ARG (-1) naming the entry point.  NULL stream, host
    buffers: nothing reaches HIP."""
    from wire_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    big = (1 << 31) - 1
    nan, inf = float("nan"), float("inf")
    geoms = (dict(H=0), dict(H=-1), dict(W=0), dict(Hl=0), dict(Wl=0), dict(Wl=-3), dict(mode=4), dict(mode=-1),
             dict(mode=3, Hl=14, sy=13 / 14), dict(mode=3, Wl=18, sx=17 / 18), dict(mode=3, sy=10.0),
             dict(sy=0.0), dict(sy=-1.0), dict(sy=nan), dict(sy=inf), dict(sx=0.0), dict(sx=nan), dict(sx=-inf))

    def geom(kw):
        g = dict(H=13, W=17, Hl=5, Wl=7, mode=1, sy=13 / 5, sx=17 / 7)
        g.update({k: v for k, v in kw.items() if k in g})
        return [g[k] for k in GEOM]

    def tables(tab=p, **kw):
        return L.wire_resize_tables(None, *geom(kw), tab)

    def fwd(tab=p, x=p, Cc=3, y=p, **kw):
        return L.wire_resize_fwd(None, tab, *geom(kw), x, Cc, y)

    def bwd(tab=p, g=p, Cc=3, gx=p, **kw):
        return L.wire_resize_bwd(None, tab, *geom(kw), g, Cc, gx)

    def mse(tab=p, y=p, O=3, gt=p, gy=p, rec=None, loss=p, ws=p, wb=4 * 5 * 7 * 3, part=p, **kw):
        return L.wire_resize_mse_grad(None, tab, *geom(kw), y, O, gt, gy, rec, loss, ws, wb, part)

    huge = dict(H=big, W=big, Hl=big, Wl=big, sy=1.0, sx=1.0)               # H W C overflows 63 bits at C = 3
    cases = {
        "wire_resize_tables": (tables, geoms + (dict(tab=None),)),
        "wire_resize_fwd": (fwd, geoms + (dict(Cc=0), dict(Cc=-2), dict(tab=None), dict(x=None), dict(y=None), huge)),
        "wire_resize_bwd": (bwd, geoms + (dict(Cc=0), dict(tab=None), dict(g=None), dict(gx=None), huge)),
        "wire_resize_mse_grad": (mse, geoms + (dict(O=0), dict(O=-1), dict(tab=None), dict(y=None), dict(gt=None),
                                              dict(gy=None), dict(loss=None), dict(ws=None), dict(part=None),
                                              dict(wb=4 * 5 * 7 * 3 - 1), dict(wb=0), dict(wb=-8), huge)),
    }
    for name, (fn, kws) in cases.items():
        for kw in kws:
            assert fn(**kw) == -1, (name, kw)
            assert name.encode() in L.wire_last_error(), (name, kw)
    for kw in geoms:
        assert L.wire_resize_tab_bytes(*geom(kw)) == -1, kw
        assert b"wire_resize_tab_bytes" in L.wire_last_error()
    for a in ((0, 7, 3), (5, 0, 3), (5, 7, 0), (-1, 7, 3), (big, big, big)):
        assert L.wire_resize_mse_grad_ws_bytes(*a) == -1, a
        assert b"wire_resize_mse_grad_ws_bytes" in L.wire_last_error()


# ---- the Python layer without a device --------------------------------------------------------------------------------
class _Bare:
    """The attributes step_resized reads before it touches the device."""

    def __init__(self, grid, world=1, O=3):
        self.grid, self.world, self.O = grid, world, O
        self.tz = object() if len(grid) == 3 else None
        self.target = None


def _step(bare, *a, **kw):
    from wire_amd.trainer import FusedTrainer
    tr = object.__new__(FusedTrainer)
    tr.__dict__.update(bare.__dict__)
    return tr.step_resized(*a, **kw)


def test_python_layer_refuses_without_a_device():
    from wire_amd import _lib, functional
    from wire_amd.modules import utils
    img = torch.zeros(13, 17, 3)
    with pytest.raises(_lib.WireHipError):
        functional.resize(img, (7, 5))
    with pytest.raises(_lib.WireHipError):
        functional.resize_adjoint(torch.zeros(5, 7, 3), (13, 17), (7, 5))
    with pytest.raises(_lib.WireHipError):
        utils.resize(img, 0.5)
    for bad in (dict(dsize=(0, 5)), dict(dsize=(7, -1)), dict(), dict(fx=0.5), dict(fx=0.5, fy=0.0),
                dict(fx=float("nan"), fy=0.5), dict(fx=float("inf"), fy=0.5), dict(fx=0.01, fy=0.01),
                dict(dsize=(7, 5), interpolation="lanczos"), dict(dsize=(7, 5), interpolation=4),
                dict(dsize=(7, 5), interpolation=True), dict(dsize=(18, 5), interpolation="area"),
                dict(dsize=(7, 14), interpolation=3), dict(fx=1.5, fy=0.5, interpolation="area")):
        with pytest.raises(ValueError):
            functional.resize(img, **bad)
    with pytest.raises(ValueError, match="does not up-scale"):
        functional.resize(img, (18, 5), interpolation="area")
    with pytest.raises(ValueError):
        functional.resize(torch.zeros(4), (2, 2))
    with pytest.raises(ValueError):
        functional.resize(np.zeros((4, 4)), (2, 2))
    with pytest.raises(ValueError, match="resized image is"):
        functional.resize_adjoint(torch.zeros(5, 6, 3), (13, 17), (7, 5))
    with pytest.raises(ValueError, match="does not up-scale"):
        utils.resize(np.zeros((4, 4, 2), np.float32), 1.5)
    with pytest.raises(ValueError):
        utils.resize(np.zeros((4, 4), np.float32), 0.5)
    with pytest.raises(ValueError):
        utils.resize(np.zeros((4, 4, 1), np.float32), 0.01)
    for text in (functional.resize.__doc__, utils.resize.__doc__):
        text = " ".join(text.split()).replace("NOT", "not")
        assert "1e-3" in text and "not been measured" in text and "up-scal" in text
    assert "resize" in utils.__doc__

    # step_resized: every refusal before the first device access
    x = torch.zeros(1)
    with pytest.raises(ValueError, match="2-D grid"):
        _step(_Bare((4, 5, 6)), x, (2, 2))
    with pytest.raises(NotImplementedError, match="step_resized is single-process"):
        _step(_Bare((4, 5), world=2), x, (2, 2))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_tv must be finite"):
            _step(_Bare((4, 5)), x, (2, 2), lambda_tv=bad)
    with pytest.raises(ValueError, match="does not up-scale"):
        _step(_Bare((4, 5)), x, (5, 5))
    with pytest.raises(ValueError, match="does not up-scale"):
        _step(_Bare((4, 5)), x, (2, 6), "area")
    with pytest.raises(ValueError, match="interpolation must be"):
        _step(_Bare((4, 5)), x, (2, 2), "lanczos")
    with pytest.raises(ValueError):
        _step(_Bare((4, 5)), x, (0, 2), "linear")
    with pytest.raises(ValueError, match="size must be"):
        _step(_Bare((4, 5)), x, (2, 2, 2))
    with pytest.raises(ValueError, match="gt_lr must be a CUDA float32 tensor of 4 x 3 elements"):
        _step(_Bare((4, 5)), torch.zeros(4, 3), (2, 2), "cubic")
