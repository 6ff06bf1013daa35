"""CPU-only checks of the tuning-knob table of libwire_hip (wire_amd/csrc/wire_knobs.hip): every key that wire_tune_set
accepts reads back through wire_tune_get, each accepts exactly its documented values, and the environment goes through
the same validation at load (a rejected value keeps the default and is named on stderr)."""
import os
import subprocess
import sys

import pytest

from _util import ROOT

INT_MAX = 2**31 - 1
FLAG = None   # any integer; a non-zero value is stored as 1
# key: (environment variable, default, accepted values, rejected values) -- written out here, not read from the library
KNOBS = {
    "complex_3m": (None, 1, FLAG, []),
    "split_bf16": ("WIRE_SPLIT_BF16", 1, FLAG, []),
    "split_f16": ("WIRE_SPLIT_F16", 1, FLAG, []),
    "split_out": ("WIRE_SPLIT_OUT", 1, FLAG, []),
    "recompute_out": ("WIRE_RECOMPUTE_OUT", 1, FLAG, []),
    "first_sums": ("WIRE_FIRST_SUMS", 1, FLAG, []),
    "fused_rstore": ("WIRE_FUSED_RSTORE", 1, FLAG, []),
    "wgrad_batch": ("WIRE_WGRAD_BATCH", 1, FLAG, []),
    "fused_train_p384": ("WIRE_FUSED_TRAIN_P384", 0, FLAG, []),
    "fused_fwd": ("WIRE_FUSED_FWD", 1, [0, 1], [-1, 2]),
    "fused_train": ("WIRE_FUSED_TRAIN", 1, [0, 1], [-1, 2]),
    "fused_final": ("WIRE_FUSED_FINAL", 0, [0, 1], [-1, 2]),
    "fused_bwd": ("WIRE_FUSED_BWD", 1, [0, 1], [-1, 2]),
    "fused_bwd_w": ("WIRE_FUSED_BWD_W", 8, [4, 8], [0, 2, 6, 16]),
    "nt_bk": ("WIRE_NT_BK", 16, [16, 32], [0, 8, 24, 64]),
    "x2_amode": ("WIRE_X2_AMODE", 2, [0, 1, 2], [-1, 3]),
    "x2_tn_rows": ("WIRE_X2_TN_ROWS", 0, [0, 256, 257, 4096, INT_MAX], [-1, 1, 128, 255]),
    "x2_tn_p384": ("WIRE_X2_TN_P384", 8, [6, 8], [0, 4, 7]),
    "x3_tall": ("WIRE_X3_TALL", 1, [0, 1], [-1, 2]),
    "x3_tall_real": ("WIRE_X3_TALL_REAL", 0, [0, 1], [-1, 2]),
    "x3_tn_tall": ("WIRE_X3_TN_TALL", 0, [0, 1], [-1, 2]),
    "x3_tn16": ("WIRE_X3_TN16", 1, [0, 1], [-1, 2]),
    "x3_h16": ("WIRE_X3_H16", 15, list(range(16)), [-1, 16]),
    "x3h_stagger": ("WIRE_X3H_STAGGER", 0, [0, 1, 100, INT_MAX], [-1]),
}


def _lib():
    from wire_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("key", list(KNOBS))
def test_knob_get_set_round_trip(key):
    L = _lib()
    env, default, accepted, rejected = KNOBS[key]
    k = key.encode()
    if env is None or env not in os.environ:
        assert L.wire_tune_get(k) == default
    start = L.wire_tune_get(k)
    try:
        for v in ([0, 1, 2, -1, 7] if accepted is FLAG else accepted):
            assert L.wire_tune_set(k, v) == 0, (key, v)
            assert L.wire_tune_get(k) == (int(v != 0) if accepted is FLAG else v), (key, v)
        for v in rejected:
            assert L.wire_tune_set(k, default) == 0
            assert L.wire_tune_set(k, v) < 0, (key, v)
            assert b"unknown tuning key or bad value" in L.wire_last_error()
            assert L.wire_tune_get(k) == default, (key, v)
    finally:
        assert L.wire_tune_set(k, start) == 0
    assert L.wire_tune_get(k) == start


def test_unknown_key_is_refused():
    L = _lib()
    assert L.wire_tune_get(b"no_such_knob") < 0
    assert b"unknown tuning key: no_such_knob" in L.wire_last_error()
    assert L.wire_tune_set(b"no_such_knob", 0) < 0
    assert b"unknown tuning key or bad value" in L.wire_last_error()


def _fresh_process(env_vars, keys):
    """wire_tune_get of `keys` in a new Python process whose environment holds `env_vars` and no other WIRE_ variable.
    Only the library is loaded: no device is touched."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("WIRE_")}
    env.update(env_vars)
    env["PYTHONPATH"] = ROOT
    code = ("from wire_amd import _lib\nL = _lib.lib()\n"
            f"print(' '.join(str(L.wire_tune_get(k.encode())) for k in {list(keys)!r}))\n")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return [int(v) for v in r.stdout.split()], r.stderr


def test_valid_environment_values_are_honoured():
    vals, err = _fresh_process({"WIRE_X2_TN_P384": "6", "WIRE_SPLIT_OUT": "5", "WIRE_FUSED_TRAIN_P384": "1",
                                "WIRE_X2_TN_ROWS": "512"},
                               ["x2_tn_p384", "split_out", "fused_train_p384", "x2_tn_rows", "fused_bwd_w"])
    assert vals == [6, 1, 1, 512, 8]
    assert "WIRE_" not in err


def test_rejected_environment_values_keep_the_default():
    vals, err = _fresh_process({"WIRE_FUSED_BWD_W": "16", "WIRE_NT_BK": "24", "WIRE_X3_H16": "abc"},
                               ["fused_bwd_w", "nt_bk", "x3_h16"])
    assert vals == [8, 16, 15]
    lines = err.splitlines()
    assert any("WIRE_FUSED_BWD_W=16" in s and "4 or 8" in s for s in lines), err
    assert any("WIRE_NT_BK=24" in s and "16 or 32" in s for s in lines), err
    assert any("WIRE_X3_H16=abc" in s and "0..15" in s for s in lines), err
