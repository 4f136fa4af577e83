"""Record tests/golden/moment_passes.npz: the outputs of the moment passes at the cases of tests/moment_passes_cases.py,
one byte string per case (tests/test_moment_passes_gpu.py compares against it bit for bit).  Needs the GPU.

    python tools/record_moment_passes.py [--out PATH]

Run it only for a deliberate change of a summation order; see the test's docstring.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import moment_passes_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "moment_passes.npz"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    entries = {}
    for name in cases.case_names():
        fields = cases.compute(name, dev)
        again = cases.compute(name, dev)
        assert fields == again, f"{name}: two runs differ"
        entries[name] = np.frombuffer(b"".join(b for _, b in fields), dtype=np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **entries)
    print(f"{len(entries)} cases, {sum(e.size for e in entries.values())} bytes of outputs, "
          f"{os.path.getsize(args.out)} bytes in {args.out}")


if __name__ == "__main__":
    main()
