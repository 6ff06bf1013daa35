"""Records tests/golden/dispatch_map.json: the kernels one FusedTrainer.step launches in every case of
tests/dispatch_cases.py.  Run once on an MI355X, from the repository root, on the commit whose routing is to be pinned:

    python tests/golden/make_dispatch_golden.py [OUT.json]

tests/test_gpu_dispatch_map.py compares later trees with the file; it is not regenerated from the code under test."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dispatch_cases as dc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "dispatch_map.json")
    rec = {}
    for kind in dc.KINDS:
        rec.update(dc.run_kind(kind))
        print(kind, "recorded", flush=True)
    assert all(rec.values()), [k for k, v in rec.items() if not v]
    dc.write_map(rec, out)
    print(len(rec), "cases ->", out)


if __name__ == "__main__":
    main()
