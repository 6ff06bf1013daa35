#!/usr/bin/env python3
"""Records tests/golden/size_queries.json: what every buffer-size query of libwire_hip.so answers over the grid of
tests/test_host_sizes.py.  Run it on the commit whose sizes are the reference (before a change that must keep them), from
the repo root, after `make -C wire_amd/csrc`:

    python tools/record_size_queries.py [--lib path/to/libwire_hip.so] [--out tests/golden/size_queries.json]

--lib: a library built from another checkout (the Python layer of this one describes the nets).  No GPU is needed; the
test never runs this script."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "size_queries.json"))
    a = ap.parse_args()
    from wire_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from test_host_sizes import size_table
    table = size_table(_lib.lib())
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {sum(len(v) for v in table.values())} values from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
