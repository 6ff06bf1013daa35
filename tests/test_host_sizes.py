"""CPU-only: every buffer-size query of the C ABI returns exactly the recorded value, for every net kind, on both sides of
the block and pre-reduction constants the sizes are built from (wire_point.h: WIRE_FB_ROWS, PRE_CHUNKS).  A smaller value
would be an out-of-bounds write on the GPU that no result check is sure to notice.  tests/golden/size_queries.json was
recorded by tools/record_size_queries.py on the commit before wire_point.hip was split; record it again only when a size is
meant to change."""
import ctypes as C
import json
import os

from _util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "size_queries.json")
WIDTHS = (64, 256)          # the host tests' small width, and one the fused paths take
# 1 and 255 / 256 / 257: around one 256-row block; 16 384 + 21: 65 blocks, the first count above 2 * PRE_CHUNKS, where
# the pre-reduction starts; 262 144: the benchmark's batch
ROWS = (1, 255, 256, 257, 16384 + 21, 262144)
D, O, LAYERS = 2, 3, 2


def net_descs(width):
    """label -> descriptor of every net kind the library accepts, D = 2 inputs and O = 3 outputs."""
    from wire_amd import _lib
    d = {k: _lib.make_desc(k, D, width, LAYERS, O, 30.0, 30.0, 10.0) for k in ("wire", "wire2d", "siren", "gauss", "relu")}
    d["relu_posenc"] = _lib.make_desc("relu", D, width, LAYERS, O, 30.0, 30.0, 10.0, posenc_freqs=4)
    d["bspline_form"] = _lib.make_desc("bspline_form", D, width, LAYERS, O, -0.2, -0.2, 1 / 9)
    d["bspline_mscale_HL"] = _lib.make_desc_ms(D, width, LAYERS, O, -0.2, -0.2, 1 / 9, 384, [1 / 9, 1 / 9, 4.0])
    d["bspline_mscale_2"] = _lib.make_desc_m2(D, width, LAYERS, O, -0.2, -0.2, 0.0, [1 / 9, 4.0])
    d["bspline_mscale_hier"] = _lib.make_desc_hier(D, width, LAYERS, O, -0.2, -0.2, 0.0, [1 / 9, 4.0])
    d["mfn"] = _lib.make_desc("mfn", D, width, LAYERS, O, 0.0, 0.0, 1.0)
    return d


def size_table(lib):
    """{"<what>/<width>[/<n>]": {query: value}} over every kind, width and row count above."""
    t = {}
    for w in WIDTHS:
        for label, d in net_descs(w).items():
            t[f"{label}/{w}"] = {"wire_packed_floats": lib.wire_packed_floats(C.byref(d))}
            for n in ROWS:
                t[f"{label}/{w}/{n}"] = {
                    "wire_act_bytes_save0": lib.wire_act_bytes(C.byref(d), n, 0),
                    "wire_act_bytes_save1": lib.wire_act_bytes(C.byref(d), n, 1),
                    "wire_bwd_scratch_bytes": lib.wire_bwd_scratch_bytes(C.byref(d), n),
                    "wire_bwd_coords_scratch_bytes": lib.wire_bwd_coords_scratch_bytes(C.byref(d), n),
                }
        for n in ROWS:
            t[f"layer/{w}/{n}"] = {
                "wire_layer_ws_bytes_first": lib.wire_layer_ws_bytes(n, D, w),
                "wire_layer_ws_bytes_hidden": lib.wire_layer_ws_bytes(n, w, w),
                "wire_layer2d_ws_bytes_first": lib.wire_layer2d_ws_bytes(n, D, w),
                "wire_layer2d_ws_bytes_hidden": lib.wire_layer2d_ws_bytes(n, w, w),
                "wire_mfn_filter_ws_bytes": lib.wire_mfn_filter_ws_bytes(n, w),
                "wire_m2_combine_ws_bytes": lib.wire_m2_combine_ws_bytes(2, O, n),
            }
    return t


def test_size_queries_return_the_recorded_values():
    from wire_amd import _lib
    got = size_table(_lib.lib())
    assert len(net_descs(64)) == 11
    # (what a descriptor's net does not have is recorded as it is answered -- but no query may refuse these shapes)
    assert all(v > 0 for q in got.values() for v in q.values())
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong
