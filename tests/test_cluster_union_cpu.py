"""The lock-free union-find of csrc/cluster_union.h on the host: tests/native/cluster_union_main.cpp, compiled with the
hipcc and flags of pytorch3d_pointops_amd/build.py, once plain and once with ThreadSanitizer on the host side of the
translation unit.  Eight host threads union random edges at once; every root must be the smallest index of its
component; index-ordered chains must stay within the load bound that path halving gives (derived in the program's
header).  The program launches no kernel and needs no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "cluster_union_main.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "tsan"])
def test_cluster_union_roots_are_smallest_indices(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "cluster_union")
    extra = ["-Xarch_host", "-fsanitize=thread", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
