"""The frame and key arithmetic of voxel_downsample (csrc/voxel_key.h) on the host: tests/native/voxel_key_main.cpp, which
includes that header and nothing else of the library, compiled with the hipcc and flags of
pytorch3d_pointops_amd/build.py, once plain and once with the host sanitizers (UBSan + ASan on the host side of the
translation unit only) as a program of its own.  It launches no kernel and needs no GPU; its header lists the cases and
says what each one pins."""
import os
import subprocess

import pytest

from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "voxel_key_main.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_voxel_key_arithmetic_holds(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "voxel_key")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout
