"""knn_in_radius without a GPU:
    checker      tests/knn_in_radius_ref.py against the CPU oracle on every finite case of tests/knn_in_radius_cases.py:
                 it equals the oracle's knn_points masked by the header's identity, and wherever the oracle's ball_query
                 with the same K and radius returns fewer than K hits -- the whole ball -- its index SET is the checker's
    list         csrc/knn_radius_list.h on the host: tests/native/knn_in_radius_list_main.cpp, which includes that header
                 and nothing else of the library, compiled with the hipcc and flags of pytorch3d_pointops_amd/build.py,
                 once plain and once with the host sanitizers as a program of its own
    arguments    the errors of the Python API that need no device"""
import os
import subprocess

import numpy as np
import pytest
import torch

import knn_in_radius_cases as cases
import knn_in_radius_ref as ref
from conftest import ROOT
from oracle.oracle import Oracle
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "knn_in_radius_list_main.cpp")
CASES = cases.build_cases()
FINITE = [n for n, c in CASES.items() if c.finite and n != cases.AUTO]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.mark.parametrize("name", FINITE)
def test_checker_equals_the_masked_oracle_and_ball_query_sets(oracle, name):
    c = CASES[name]
    want = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    oi, od = oracle.knn_points_idx(c.p1, c.p2, c.lengths1, c.lengths2, 2, c.K)
    masked = ref.mask_knn(oi, od, c.lengths1, c.lengths2, c.radius)
    for k in cases.KEYS:
        assert want[k].dtype == masked[k].dtype and want[k].tobytes() == masked[k].tobytes(), f"{name}: {k}"
    bi, _ = oracle.ball_query(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    whole = (bi >= 0).sum(2) < c.K  # fewer than K hits: ball_query returned the whole ball
    assert np.array_equal(np.sort(bi[whole], 1), np.sort(want["idx"][whole], 1)), f"{name}: ball_query's sets"
    assert np.array_equal(want["counts"][whole], (bi[whole] >= 0).sum(1))
    # the rule itself: counts = the valid slots, ascending (d2, j)
    assert np.array_equal(want["counts"], (want["idx"] >= 0).sum(2))
    valid = want["idx"][..., 1:] >= 0
    d0, d1 = want["dists"][..., :-1], want["dists"][..., 1:]
    assert np.all(~valid | (d0 < d1) | ((d0 == d1) & (want["idx"][..., :-1] < want["idx"][..., 1:])))


def test_the_cases_show_what_they_are_meant_to():
    """Ties cut by K on the lattice, pairs at d2 == r2 left out, rows with fewer and with more than K candidates."""
    c = CASES["lattice-r1.0-2^0"]
    w = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    assert w["counts"].max() == 1 == w["counts"].min() and float(w["dists"].max()) == 0.0  # (six rows at d2 == r2)
    c = CASES["lattice-r1.5-2^10"]
    w = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    assert w["counts"].max() == 17 and np.any(w["dists"][..., 16] == w["dists"][..., 15])
    c = CASES["uniform-D3-K8"]
    w = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    assert (w["counts"][0] < 8).any() and (w["counts"][0] == 8).any() and w["counts"][2].max() == 0 == w["counts"][3].max()
    assert w["counts"][1, :300].max() <= 8 and w["counts"][1, 300:].max() == 0
    for name in ("no-neighbours", "r2-underflows"):
        c = CASES[name]
        assert ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)["counts"].max() == 0
    assert ref.r2_of(CASES["r2-underflows"].radius) == 0.0 and np.isinf(ref.r2_of(CASES["r2-is-inf"].radius))
    c = CASES["surface-and-clutter-K1"]
    w = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    assert 0.15 < (w["counts"][0] == 0).mean() < 0.35  # the clutter rows
    c = CASES["nan-and-inf-rows"]
    w = ref.knn_in_radius(c.p1, c.p2, c.lengths1, c.lengths2, c.K, c.radius)
    assert w["counts"][0, 3] == 0 and not (w["idx"][1] == 17).any() and not (w["idx"][2] == 5).any()
    assert sorted({c.K for c in CASES.values()} & set(cases.EDGE_K)) == sorted(cases.EDGE_K)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_list_header_equals_std_sort(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "knn_in_radius_list")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout


def test_argument_errors_need_no_device():
    from pytorch3d_pointops_amd import functions as f

    a, b = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for radius in (0.0, -1.0, float("inf"), float("nan"), 1e39, 1e-46, "wide"):
        with pytest.raises(ValueError, match="radius"):
            f.knn_in_radius(a, b, K=1, radius=radius)
    for K in (0, -3):
        with pytest.raises(ValueError, match="K has to be"):
            f.knn_in_radius(a, b, K=K, radius=0.1)
    with pytest.raises(ValueError, match="batch dimension"):
        f.knn_in_radius(a, b[:1], K=1, radius=0.1)
    with pytest.raises(ValueError, match="point dimension"):
        f.knn_in_radius(a, b[..., :2], K=1, radius=0.1)
    with pytest.raises(ValueError, match=r"\(N, P, D\)"):
        f.knn_in_radius(a[0], b, K=1, radius=0.1)
    with pytest.raises(ValueError, match="float32"):
        f.knn_in_radius(a.double(), b.double(), K=1, radius=0.1)
    with pytest.raises(ValueError, match=r"shape \(N,\)"):
        f.knn_in_radius(a, b, torch.tensor([5]), None, K=1, radius=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # every argument is fine: the GPU-only error
        f.knn_in_radius(a, b, K=1, radius=0.1)
    for call in (lambda: f.registration_icp(a, b, 0.1, estimation="point_to_point", search="nonsense"),
                 lambda: f.evaluate_registration(a, b, 0.1, search="nonsense")):
        with pytest.raises(ValueError, match="search must be one of"):
            call()
