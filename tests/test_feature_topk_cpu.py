"""knn_features without a GPU:
    host half    csrc/feature_topk.h on the host: tests/native/feature_topk_main.cpp (the 2 S-way merge, r_K and the
                 certificate against a brute-force top K), compiled with the hipcc and flags of
                 pytorch3d_pointops_amd/build.py, once plain and once with the host sanitizers as a program of its own
    checker      the counts of tests/feature_topk_ref.py on named draws: what the GPU test holds the kernel's stats to
    arguments    the entries the boundary declares and the errors of the Python API that need no device
No test here loads sanitized code into Python: the sanitized build is a program with its own main."""
import os
import subprocess

import numpy as np
import pytest
import torch

import feature_topk_ref as tref
import match_cases as cases
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "feature_topk_main.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_topk_header_merges_and_certifies(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "feature_topk")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout


def named_draws():
    """256 queries over 1000 targets: three 11-bin histograms (D = 33) and unit rows (D = 32)."""
    rng = np.random.default_rng(18)
    return {"fpfh_like": (cases.fpfh_like(rng, (1, 256)), cases.fpfh_like(rng, (1, 1000))),
            "unit_rows": (cases.unit_rows(rng, (1, 256)), cases.unit_rows(rng, (1, 1000)))}


@pytest.mark.parametrize("K,S", [(16, 1), (20, 4), (32, 4)])
def test_the_checker_lists_no_row_of_the_named_draws(K, S):
    for name, (a, b) in named_draws().items():
        assert int(tref.uncertified_rows(a, b, K=K, S=S).sum()) == 0, f"{name} K={K} S={S}"


def test_the_checker_on_exact_inputs_and_the_list_map():
    assert [int(tref.list_of(np.int64(j), 4)) for j in (0, 4, 37, 64, 127, 128)] == [0, 1, 3, 4, 7, 0]
    assert [int(tref.list_of(np.int64(j), 1)) for j in (0, 4, 36, 40)] == [0, 1, 1, 0]
    a, b = cases.all_duplicates()  # every distance ties: no cut separates the K-th from a dropped target
    assert tref.uncertified_rows(a, b, K=2, S=1).all() and tref.uncertified_rows(a, b, K=20, S=4).all()
    a, b = cases.integer_no_fallback()
    assert int(tref.uncertified_rows(a[:, :100], b, K=2, S=1).sum()) == 0
    # two lists of 16 keys hold at most 32 targets, 17 nearest rarely sit in them with room to certify: S = 1 lists rows
    # at K = 32 that S = 4 certifies
    a, b = named_draws()["unit_rows"]
    assert int(tref.uncertified_rows(a, b, K=32, S=1).sum()) > 0


def test_the_boundary_declares_the_entries():
    from pytorch3d_pointops_amd import _C, _C_feature_topk, functions

    assert {"pointops_feature_topk", "pointops_feature_topk_workspace_bytes"} <= set(_C.exported_symbols())
    assert "knn_features" in functions.__all__
    sizer = _C._lib.pointops_feature_topk_workspace_bytes
    assert sizer(2, 100, 200, 33, 20) >= 4 * (2 * 100 + 2 * 200 + 4 + 2 * 100)  # norms, n2max and count, the row list
    for bad in ((-1, 8, 8, 33, 1), (1, 8, 8, 0, 1), (1, 8, 8, 33, 0), (1, 2 ** 31, 8, 33, 1), (0, 8, 8, 33, 1)):
        assert sizer(*bad) == 0
    assert (_C_feature_topk.SCREEN_MAX_D, _C_feature_topk.SCREEN_MAX_K) == (128, 32)


def test_argument_errors_need_no_device():
    from pytorch3d_pointops_amd import _C_feature_topk
    from pytorch3d_pointops_amd import functions as f

    a, b = torch.zeros(2, 5, 33), torch.zeros(2, 7, 33)
    with pytest.raises(ValueError, match=r"\(N, P, D\)"):
        f.knn_features(a[0], b)
    with pytest.raises(ValueError, match="K has to be"):
        f.knn_features(a, b, K=0)
    with pytest.raises(ValueError, match="same batch dimension"):  # (knn_points' own text: CPU tensors go there)
        f.knn_features(a, b[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f.knn_features(a, b, K=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C_feature_topk.feature_topk(a, b, torch.tensor([5, 5]), torch.tensor([7, 7]), 3)
