"""CPU-only: the three buffer-size queries (packed floats, activation bytes, backward scratch bytes) of the nets the
data-gradient epilogue and pack tests run on answer exactly what tests/golden/size_queries.json records -- a change to an
epilogue, a route or a knob must not move a size (tests/test_host_sizes.py checks the whole table; this file names the
nets and the three queries a training call sizes its buffers with, at both settings of the knobs)."""
import ctypes as C
import json

import pytest

from _util import tune
from test_host_sizes import GOLDEN, ROWS, net_descs

# width 256 through the descriptor: wire K = 256 (P = 512); width 64: the ragged small width of the host tests.  The
# golden table has no K = 181 entry: hidden_features = 256 through the module API reaches the library as width 181,
# which the table's two widths bracket
NETS = ("wire", "wire2d", "siren", "relu_posenc", "bspline_mscale_HL", "bspline_mscale_2")
WIDTHS = (64, 256)


@pytest.mark.parametrize("knobs", [1, 0])
@pytest.mark.parametrize("width", WIDTHS)
def test_the_three_size_queries_of_the_tested_nets(width, knobs):
    from wire_amd import _lib
    lib = _lib.lib()
    with open(GOLDEN) as f:
        want = json.load(f)
    descs = net_descs(width)
    with tune(first_dn=knobs, bwd_lookahead=knobs):
        for label in NETS:
            d = descs[label]
            assert lib.wire_packed_floats(C.byref(d)) == want[f"{label}/{width}"]["wire_packed_floats"], label
            for n in ROWS:
                rec = want[f"{label}/{width}/{n}"]
                assert lib.wire_act_bytes(C.byref(d), n, 1) == rec["wire_act_bytes_save1"], (label, n)
                assert lib.wire_act_bytes(C.byref(d), n, 0) == rec["wire_act_bytes_save0"], (label, n)
                assert lib.wire_bwd_scratch_bytes(C.byref(d), n) == rec["wire_bwd_scratch_bytes"], (label, n)
