"""Host side of the coordinate-gradient ABI: exports, size queries, argument validation -- no device is touched (every
call below fails its checks before any launch)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["wire_bwd_coords_scratch_bytes", "wire_mlp_bwd_coords", "wire_posenc_bwd", "wire_gabor_bwd_first_coords",
       "wire_gabor2d_bwd_first_coords"]


def _lib():
    from wire_amd import _lib
    return _lib, _lib.lib()


def test_new_exports_in_header_and_library():
    _l, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "wire_hip.h")).read()
    declared = set(re.findall(r"\b(wire_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _l.SYMBOLS and hasattr(lib, name), name
    assert lib.wire_abi_version() == 1


@pytest.mark.parametrize("kind,D,K,L,F", [("wire", 2, 256, 4, 0), ("wire", 3, 181, 4, 0), ("wire2d", 2, 128, 3, 0),
                                          ("siren", 2, 256, 4, 0), ("relu", 3, 128, 2, 10), ("wire", 2, 64, 0, 0)])
def test_coords_scratch_size(kind, D, K, L, F):
    _l, lib = _lib()
    d = _l.make_desc(kind, D, K, L, 3, 30.0, 30.0, 10.0, F)
    prev = 0
    for n in (1, 4133, 65537, 262144, 262145):
        full = lib.wire_bwd_coords_scratch_bytes(C.byref(d), n)
        base = lib.wire_bwd_scratch_bytes(C.byref(d), n)
        assert base > 0 and full >= base + 4 * n * D, (n, full, base)
        # (wire_bwd_scratch_bytes itself is not monotone in n: the weight-gradient split counts vary; what the
        #  coordinate gradient adds on top of it grows with n)
        assert full - base > prev
        prev = full - base
    assert lib.wire_bwd_coords_scratch_bytes(C.byref(d), -1) < 0


def _err(lib):
    return lib.wire_last_error().decode()


def test_bad_arguments_fail_on_the_host():
    _l, lib = _lib()
    d = _l.make_desc("wire", 2, 64, 2, 3, 20.0, 20.0, 30.0)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    n = 5000
    sb = lib.wire_bwd_coords_scratch_bytes(C.byref(d), n)
    ab = lib.wire_act_bytes(C.byref(d), n, 1)
    grads = _l.ptr_array([0x1000] * lib.wire_num_param_tensors(C.byref(d)))
    # neither grads_host nor g_coords
    assert lib.wire_mlp_bwd_coords(None, C.byref(d), fake, fake, n, fake, fake, ab, fake, sb, None, None) != 0
    assert "neither" in _err(lib)
    # null packed / coords
    assert lib.wire_mlp_bwd_coords(None, C.byref(d), None, fake, n, fake, fake, ab, fake, sb, None, fake) != 0
    assert "null" in _err(lib)
    assert lib.wire_mlp_bwd_coords(None, C.byref(d), fake, None, n, fake, fake, ab, fake, sb, grads, fake) != 0
    # scratch of wire_bwd_scratch_bytes is too small once g_coords is asked for
    small = lib.wire_bwd_scratch_bytes(C.byref(d), n)
    assert lib.wire_mlp_bwd_coords(None, C.byref(d), fake, fake, n, fake, fake, ab, fake, small, None, fake) != 0
    assert "scratch" in _err(lib)
    # ... and enough without it (then the call would run: not made here)
    # D = 5
    d5 = _l.make_desc("wire", 5, 64, 2, 3, 20.0, 20.0, 30.0)
    assert lib.wire_bwd_coords_scratch_bytes(C.byref(d5), n) < 0
    assert lib.wire_mlp_bwd_coords(None, C.byref(d5), fake, fake, n, fake, fake, ab, fake, sb, None, fake) != 0
    assert "in_features" in _err(lib)
    # posenc_bwd: D = 5, F = 31, nulls
    assert lib.wire_posenc_bwd(None, fake, n, 5, 10, fake, fake) != 0
    assert "wire_posenc_bwd" in _err(lib)
    assert lib.wire_posenc_bwd(None, fake, n, 2, 31, fake, fake) != 0
    assert lib.wire_posenc_bwd(None, None, n, 2, 10, fake, fake) != 0
    assert lib.wire_posenc_bwd(None, fake, n, 2, 10, fake, None) != 0
    # per-layer first layers: in_features > 4, null g_x, partial parameter-gradient sets, workspace too small
    ws = lib.wire_layer_ws_bytes(n, 2, 40)
    assert lib.wire_gabor_bwd_first_coords(None, fake, fake, fake, fake, 9.0, 4.0, n, 5, 40, fake, fake, fake, fake,
                                           ws) != 0
    assert lib.wire_gabor_bwd_first_coords(None, fake, fake, fake, fake, 9.0, 4.0, n, 2, 40, None, fake, fake, fake,
                                           ws) != 0
    assert lib.wire_gabor_bwd_first_coords(None, fake, fake, fake, fake, 9.0, 4.0, n, 2, 40, fake, fake, None, fake,
                                           ws) != 0
    assert lib.wire_gabor_bwd_first_coords(None, fake, fake, fake, fake, 9.0, 4.0, n, 2, 40, fake, None, None, fake,
                                           ws - 1024) != 0
    assert "workspace" in _err(lib)
    ws2 = lib.wire_layer2d_ws_bytes(n, 2, 40)
    assert lib.wire_gabor2d_bwd_first_coords(None, fake, fake, fake, fake, fake, fake, 9.0, 4.0, n, 2, 40, fake, fake,
                                             None, None, None, fake, ws2) != 0
    assert lib.wire_gabor2d_bwd_first_coords(None, fake, fake, fake, fake, fake, fake, 9.0, 4.0, n, 2, 40, None, None,
                                             None, None, None, fake, ws2) != 0
    # the existing entry keeps its contract: grads == NULL is still an argument error
    assert lib.wire_mlp_bwd(None, C.byref(d), fake, fake, n, fake, fake, ab, fake, sb, None) != 0
