"""CPU-only checks of the two knobs of the 2 x fp16 NT GEMMs' loosened waits ("nt_bfirst", "epi_early";
wire_amd/csrc/wire_knobs.hip): flags, default 1, read from the environment at load like every other row of the table
(tests/test_tune_knobs.py holds the rows that were there before)."""
import os
import subprocess
import sys

import pytest

from _util import ROOT

KNOBS = {"nt_bfirst": "WIRE_NT_BFIRST", "epi_early": "WIRE_EPI_EARLY"}


@pytest.mark.parametrize("key", list(KNOBS))
def test_flag_round_trip(key):
    from wire_amd import _lib
    L = _lib.lib()
    k = key.encode()
    if KNOBS[key] not in os.environ:
        assert L.wire_tune_get(k) == 1
    start = L.wire_tune_get(k)
    try:
        for v in (0, 1, 2, -1, 7):
            assert L.wire_tune_set(k, v) == 0, (key, v)
            assert L.wire_tune_get(k) == int(v != 0), (key, v)
    finally:
        assert L.wire_tune_set(k, start) == 0
    assert L.wire_tune_get(k) == start


def test_environment_is_honoured():
    env = {k: v for k, v in os.environ.items() if not k.startswith("WIRE_")}
    env.update({"WIRE_NT_BFIRST": "0", "WIRE_EPI_EARLY": "x", "PYTHONPATH": ROOT})
    code = ("from wire_amd import _lib\nL = _lib.lib()\n"
            "print(L.wire_tune_get(b'nt_bfirst'), L.wire_tune_get(b'epi_early'))\n")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["0", "1"]
    assert any("WIRE_EPI_EARLY=x" in s and "any integer" in s for s in r.stderr.splitlines()), r.stderr
