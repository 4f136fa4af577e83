"""The per-point arithmetic of iss_keypoints (csrc/iss_saliency.h) on the host: tests/native/iss_saliency_main.cpp, which
includes that header and nothing else of the library, compiled with the hipcc and flags of
pytorch3d_pointops_amd/build.py, once plain and once with the host sanitizers (UBSan + ASan on the host side of the
translation unit only) as a program of its own.  It launches no kernel and needs no GPU; its header lists the cases and
derives the bound."""
import os
import subprocess

import pytest

from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "iss_saliency_main.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_iss_saliency_arithmetic_holds(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "iss_saliency")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout
