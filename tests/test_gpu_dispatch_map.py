"""Which kernels a training step runs, per net kind: the sorted set of the library's kernel names (template arguments
included) that one FusedTrainer.step launches in every case of tests/dispatch_cases.py must equal the set recorded in
tests/golden/dispatch_map.json (tests/golden/make_dispatch_golden.py, run before the kinds' codes moved into one table).
The parity tests pin what a step computes; for the real kinds nothing else pins the route it takes."""
import os

import pytest

import dispatch_cases as dc
from _util import GOLDEN


@pytest.fixture(scope="module")
def golden():
    # (the file is kept as recorded; its lists pass through the same name filter as a run's)
    return {cid: dc.ours(names) for cid, names in dc.read_map(os.path.join(GOLDEN, "dispatch_map.json")).items()}


def test_golden_holds_every_case(golden):
    assert set(golden) == {cid for kind in dc.KINDS for cid, *_ in dc.case_ids(kind)}
    # (the name filter is applied to the recording too: widening it must not empty a case of what the test is about)
    for cid, names in golden.items():
        assert any("gemm" in k for k in names), cid


@pytest.mark.gpu
@pytest.mark.parametrize("kind", dc.KINDS)
def test_step_runs_the_recorded_kernels(golden, kind):
    got = dc.run_kind(kind)
    for cid, names in got.items():
        # (a profiler that reports nothing must not pass: no set is empty, and a default step on 4096 rows runs the
        #  2 x fp16 NT GEMM or the whole-net forward)
        assert names, cid
        if cid.endswith("/n4096/default"):
            assert any("gemmx2h_nt_kernel" in k or "fused_fwd_kernel" in k for k in names), (cid, names)
        want = golden[cid]
        assert names == want, f"{cid}: only now {sorted(set(names) - set(want))}, only recorded {sorted(set(want) - set(names))}"
