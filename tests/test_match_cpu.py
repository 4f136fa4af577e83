"""match_features without a GPU:
    checker      tests/match_ref.py against the CPU oracle: its K = 2 and K = 1 searches equal the oracle's
                 knn_points_idx byte for byte on every finite case of tests/match_cases.py, and the filters do what the
                 definition (the FEATURE MATCHING block of include/pointops_amd.h) says on cases built to show it
    screen       csrc/feature_screen.h on the host: tests/native/feature_screen_main.cpp, which includes that header and
                 nothing else of the library, compiled with the hipcc and flags of pytorch3d_pointops_amd/build.py, once
                 plain and once with the host sanitizers as a program of its own
    arguments    the errors of the Python API that need no device
No test here loads sanitized code into Python: the sanitized build is a program with its own main."""
import os
import subprocess

import numpy as np
import pytest
import torch

import match_cases as cases
import match_ref as ref
from conftest import ROOT
from oracle.oracle import Oracle
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "feature_screen_main.cpp")
CASES = cases.build_cases()
FINITE = [n for n, c in CASES.items() if c.finite and c.f1.shape[0] > 0]


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.mark.parametrize("name", FINITE)
def test_checker_search_equals_the_oracle(oracle, name):
    c = CASES[name]
    for K in (1, 2):
        gi, gd = ref.knn(c.f1, c.f2, c.lengths1, c.lengths2, K)
        oi, od = oracle.knn_points_idx(c.f1, c.f2, c.lengths1.astype(np.int64), c.lengths2.astype(np.int64), 2, K)
        assert gi.dtype == oi.dtype and gi.tobytes() == np.ascontiguousarray(oi).tobytes(), f"{name}: idx, K={K}"
        assert gd.dtype == od.dtype and gd.tobytes() == np.ascontiguousarray(od).tobytes(), f"{name}: dists, K={K}"


def test_the_cases_show_what_they_are_meant_to():
    # ties cut by index: the second distance equals the first on many rows, and the lower index comes first
    c = next(v for k, v in CASES.items() if k.startswith("ties-1000x"))
    idx, d = ref.knn(c.f1, c.f2, c.lengths1, c.lengths2, 2)
    tied = (d[0, :, 0] == d[0, :, 1])
    assert tied.mean() > 0.05 and (idx[0, tied, 0] < idx[0, tied, 1]).all()
    # ratio exactly at the boundary: fl(0.5^2) * 4 == 1 == d1 fails the strict comparison, one ulp more passes
    f1, f2, l1, l2 = cases.ratio_boundary()
    at = ref.match_features(f1, f2, l1, l2, mutual=False, ratio=0.5)
    above = ref.match_features(f1, f2, l1, l2, mutual=False, ratio=float(np.nextafter(np.float32(0.5), np.float32(1))))
    assert at["dists"][0, 0] == 1.0 and at["second"][0, 0] == 4.0
    assert at["corr"].tolist() == [[-1, -1], [0, 0]] and above["corr"].tolist() == [[1, -1], [0, 0]]
    assert at["num_matches"].tolist() == [0, 2] and above["num_matches"].tolist() == [1, 2]
    # ... and a cloud with ONE target has no second: +inf, and its rows pass the ratio test
    assert np.isinf(at["second"][1]).all() and at["dists"][1].tolist() == [25.0, 25.0]
    # the distance cap is ball query's strict comparison on fl(m * m)
    assert ref.match_features(f1, f2, l1, l2, mutual=False, max_distance=1.0)["corr"][0, 0] == -1
    assert ref.match_features(f1, f2, l1, l2, mutual=False, max_distance=1.0001)["corr"][0, 0] == 1
    # lengths2 in {0, 1, 2}: no nearest (0, 0, -1), a nearest without a second, both
    c = CASES["ragged"]
    m = ref.match_features(c.f1, c.f2, c.lengths1, c.lengths2, mutual=False)
    assert c.lengths2[:3].tolist() == [0, 1, 2]
    assert (m["corr"][0] == -1).all() and not m["dists"][0].any() and not m["second"][0].any()  # no targets
    assert (m["corr"][1] == -1).all() and m["num_matches"][1] == 0                                # no queries
    assert m["corr"][2, 0] >= 0 and np.isfinite(m["second"][2, 0]) and (m["corr"][2, 1:] == -1).all()
    one_target = ref.match_features(c.f1[1:2], c.f2[1:2], np.array([40]), np.array([1]), mutual=False)
    assert (one_target["corr"] == 0).all() and np.isinf(one_target["second"]).all() and (one_target["dists"] > 0).all()
    # the mutual check removes rows, and never adds one
    both = ref.match_features(c.f1, c.f2, c.lengths1, c.lengths2)
    assert ((both["corr"] >= 0) <= (m["corr"] >= 0)).all() and both["num_matches"].sum() < m["num_matches"].sum()
    # the scene of the end-to-end test: the ratio test removes wrong matches that the mutual check keeps
    f1, f2, truth = cases.replaced_scene()
    counts = {}
    for key, kw in (("mutual", {}), ("ratio", dict(ratio=0.8)), ("all", dict(ratio=0.8, max_distance=30.0))):
        corr = ref.match_features(f1, f2, **kw)["corr"][0]
        found = corr >= 0
        counts[key] = (int(found.sum()), int((found & (corr != truth)).sum()))
    assert counts == {"mutual": (883, 43), "ratio": (841, 1), "all": (840, 0)}


def test_the_certificate_of_the_checker_on_exact_inputs():
    """Small integers: every product and sum is exact, so s == r, and the certificate fails exactly where a tie or a
    near-tie crosses the lists.  The counts the GPU test holds the kernel's stats to."""
    a, b = cases.integer_no_fallback()
    s, _, _ = ref.screen_values(a[0, :100], b[0])
    assert (s == ref.pair_distances(a[0, :100], b[0])).all()
    assert int(ref.uncertified_rows(a, b, K=2).sum()) == 0
    a, b = cases.integer_ties()
    assert int(ref.uncertified_rows(a, b, K=2).sum()) == 49
    a, b = cases.all_duplicates()
    assert ref.uncertified_rows(a, b, K=1).all() and ref.uncertified_rows(a, b, K=2).all()
    c = CASES["huge"]
    assert ref.uncertified_rows(c.f1, c.f2, c.lengths1, c.lengths2, K=1)[0].all()


def test_fma32_is_one_rounding():
    """The checker's fmaf against exact rational arithmetic, ties of the float64 sum included."""
    from fractions import Fraction

    rng = np.random.default_rng(3)
    x, y, z = (rng.standard_normal(3000).astype(np.float32) for _ in range(3))
    # a float64 sum that sits exactly on a float32 tie while the true sum does not: the product is 2^-24 - 2^-64, the
    # float64 sum with 1 + 2^-23 rounds to 1 + 3 * 2^-24, which ties to even UP; the true sum is below the tie: DOWN
    x[0], y[0] = np.float32(2.0 ** -12 * (1 + 2.0 ** -20)), np.float32(2.0 ** -12 * (1 - 2.0 ** -20))
    z[0] = np.nextafter(np.float32(1), np.float32(2))
    x[1], y[1], z[1] = -x[0], y[0], -z[0]  # (and mirrored)
    x[2], y[2], z[2] = np.float32(2.0 ** -12), np.float32(2.0 ** -12), np.float32(1.0)  # exactly on the tie: to even
    assert ref.fma32(x[:1], y[:1], z[:1])[0] == z[0] and np.float32(np.float64(x[0]) * np.float64(y[0]) + np.float64(z[0])) > z[0]
    got = ref.fma32(x, y, z)
    for i in range(len(x)):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        lo = np.float32(float(exact))  # (float() of a Fraction rounds correctly to float64; then the neighbours decide)
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        want = min(cands, key=lambda f: (abs(Fraction(float(f)) - exact), int(np.float32(f).view(np.uint32)) & 1))
        assert got[i] == want, (i, x[i], y[i], z[i], got[i], want)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_screen_header_holds_its_bound(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "feature_screen")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout


def test_the_boundary_declares_the_entries():
    from pytorch3d_pointops_amd import _C, _C_match, functions

    assert {"pointops_feature_knn", "pointops_feature_knn_workspace_bytes",
            "pointops_feature_screen_values"} <= set(_C.exported_symbols())
    assert {"match_features", "FeatureMatches"} <= set(functions.__all__)
    sizer = _C._lib.pointops_feature_knn_workspace_bytes
    assert sizer(2, 100, 200, 33, 2) >= 4 * (2 * 100 + 2 * 200 + 4 + 2 * 100)  # norms, n2max and count, the row list
    for bad in ((-1, 8, 8, 33, 1), (1, 8, 8, 0, 1), (1, 8, 8, 33, 0), (1, 8, 8, 33, 3), (1, 2 ** 31, 8, 33, 1), (0, 8, 8, 33, 1)):
        assert sizer(*bad) == 0
    assert _C_match.MAX_K == 2


def test_argument_errors_need_no_device():
    from pytorch3d_pointops_amd import functions as f

    a, b = torch.zeros(2, 5, 33), torch.zeros(2, 7, 33)
    for ratio in (0.0, -0.5, 1.0001, 2, float("nan"), float("inf"), 1e-46, "wide"):
        with pytest.raises(ValueError, match="ratio"):
            f.match_features(a, b, ratio=ratio)
    for m in (0.0, -1.0, float("inf"), float("nan"), 1e39, 1e-46, "far"):
        with pytest.raises(ValueError, match="max_distance"):
            f.match_features(a, b, max_distance=m)
    with pytest.raises(ValueError, match="batch and feature"):
        f.match_features(a, b[:1])
    with pytest.raises(ValueError, match="batch and feature"):
        f.match_features(a, b[..., :32])
    with pytest.raises(ValueError, match=r"\(N, P, D\)"):
        f.match_features(a[0], b)
    with pytest.raises(ValueError, match="float32"):
        f.match_features(a.double(), b.double())
    with pytest.raises(ValueError, match=r"shape \(N,\)"):
        f.match_features(a, b, torch.tensor([5]), None)
    with pytest.raises(ValueError, match=r"shape \(N,\)"):
        f.match_features(a, b, None, torch.tensor([5.0, 7.0]))
    with pytest.raises(TypeError):
        f.match_features(a, b, None, None, True)  # the filters are keyword-only
    for kw in (dict(), dict(ratio=1.0, max_distance=3.0, mutual=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # every argument is fine: the GPU-only error
            f.match_features(a, b, **kw)
