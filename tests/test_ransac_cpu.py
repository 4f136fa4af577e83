"""CPU suite of ransac_alignment: the checker (tests/ransac_ref.py) on a hand case, the hash and the draws against
literal values, the reachability of what the GPU suite asserts on its scenes -- computed by the checker alone --, the
argument validation of the public function, and the per-lane routines of csrc/ransac_hypothesis.h as a native host
program (tests/native/ransac_hypothesis_main.cpp, plain and under the host sanitizers; nothing is loaded into Python)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ransac_ref as ref
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "ransac_hypothesis_main.cpp")


# ------------------------------------------------------------------------------------------------ hand case
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("offset, count", [(0.25, 4), (0.25 - 2.0 ** -20, 4), (0.25 + 2.0 ** -20, 3)],
                         ids=["on", "inside", "outside"])
def test_hand_case_translation(offset, count, dtype):
    """Three pairs under a pure translation: R = I, T exact.  thr = 0.25, thr2 = 2^-4; a fourth pair sits `offset`
    off along x: d2 = offset^2 is 2^-4, 2^-4 - 2^-21 + 2^-40 or 2^-4 + 2^-21 + 2^-40 -- in fp32 2^-4, 2^-4 - 2^-21
    and 2^-4 + 2^-21 (the ulp there is 2^-28) --, every coordinate and difference is exact."""
    T = np.array([0.5, -0.25, 2.0])
    X = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]]], np.float32)
    Y = (X.astype(np.float64) + T).astype(np.float32)
    Y[0, 3, 0] = np.float32(0.5 + offset)
    Y[0, 4] = 5.0  # a wrong match: |x0 - x4|^2 = 4 against about 57
    assert float(Y[0, 3, 0]) == 0.5 + offset
    samples = np.array([[[0, 1, 2], [2, 2, 1], [0, 1, 7], [0, 1, 4]]], np.int64)
    r = ref.run(X, Y, thr=0.25, samples=samples, ratio=0.0, refine_steps=0, dtype=dtype)
    hR, hT, hs = r["hyp"]
    assert np.abs(hR[0, 0] - np.eye(3)).max() < 1e-15 and np.array_equal(hT[0, 0].astype(np.float32), T.astype(np.float32))
    assert hs[0, 0] == 1.0
    assert r["valid"].tolist() == [[True, False, False, True]]  # a repeated row, a row outside the cloud
    assert r["counts"][0, 0] == count and r["counts"][0, 1] == -1 and r["counts"][0, 2] == -1
    assert 0 <= r["counts"][0, 3] < 3  # the triangles are not congruent: not even its own three pairs fit
    assert r["best"][0] == 0 and r["num_inliers"][0] == count
    assert r["mask"][0].tolist() == [True, True, True, count == 4, False]
    assert r["rmse"][0] == pytest.approx(np.sqrt(offset * offset / 4) if count == 4 else 0.0, abs=1e-7)
    # the edge test throws the incongruent triple out
    e = ref.run(X, Y, thr=0.25, samples=samples, ratio=0.9, refine_steps=0, dtype=dtype)
    assert e["valid"].tolist() == [[True, False, False, False]] and e["counts"][0, 3] == -1 and e["best"][0] == 0


def test_no_valid_hypothesis_is_the_identity():
    X = np.random.default_rng(0).uniform(size=(2, 6, 3)).astype(np.float32)
    corr = np.full((2, 6), -1, np.int64)
    corr[1, :2] = [3, 4]  # two valid rows: not enough
    r = ref.run(X, X + 1, corr, H=8, dtype=np.float32)
    assert (r["samples"] == -1).all() and (r["counts"] == -1).all() and r["best"].tolist() == [-1, -1]
    assert np.array_equal(r["R"], np.stack([np.eye(3)] * 2)) and not r["T"].any() and (r["s"] == 1).all()
    assert not r["mask"].any() and not r["num_inliers"].any() and not r["rmse"].any()


# ------------------------------------------------------------------------------------------------ hash and draws
KNOWN = [((0, 0, 0, 0), 246052113), ((0, 0, 0, 1), 1618519239), ((1, 2, 3, 2), 2304317301),
         ((12345, 70000, 4095, 0), 3934780713), (((1 << 32) + 5, 1, 1, 1), 609416146),
         (((1 << 62) + 7, 65536, 17, 2), 3197956988)]


def test_hash32_known_answers():
    """The same literals as tests/native/ransac_hypothesis_main.cpp holds csrc/ransac_hypothesis.h to."""
    for args, want in KNOWN:
        assert int(ref.hash32(*args)) == want, args
    assert int(ref.hash32((1 << 32) + 5, 1, 1, 1)) != int(ref.hash32(5, 1, 1, 1))  # the high word of the seed counts
    assert ref.draw(0, 0, 4, 5).tolist() == [[0, 2, 4], [4, 0, 2], [2, 4, 3], [3, 0, 1]]
    assert ref.draw(7, 3, 1, (1 << 31) - 1).tolist() == [[237027451, 1901222351, 602237762]]


@pytest.mark.parametrize("M", [3, 4, 5, 1000, (1 << 31) - 1])
def test_draws_are_distinct_and_in_range(M):
    for seed, n in ((0, 0), (1 << 40, 69999)):
        d = ref.draw(seed, n, 20000, M)
        assert d.min() >= 0 and d.max() < M
        assert (d[:, 0] != d[:, 1]).all() and (d[:, 0] != d[:, 2]).all() and (d[:, 1] != d[:, 2]).all()


def test_draws_are_roughly_uniform():
    """M = 5: each of the 60 ordered triples is expected 1000 times in 60 000 draws (sigma 31: +-200 is 6 sigma); each
    position of M = 1000 in deciles."""
    d = ref.draw(3, 1, 60000, 5)
    codes = d[:, 0] * 25 + d[:, 1] * 5 + d[:, 2]
    hist = np.bincount(codes, minlength=125)
    assert (hist > 0).sum() == 60 and np.abs(hist[hist > 0] - 1000).max() < 200
    d = ref.draw(4, 2, 50000, 1000)
    for k in range(3):
        dec = np.bincount(d[:, k] // 100, minlength=10)
        assert np.abs(dec - 5000).max() < 400  # sigma 67


# ------------------------------------------------------------------------------------------------ reachability
@pytest.mark.parametrize("name", [k for k, v in ref.SCENES.items() if v.get("planted", True)])
def test_gpu_scene_is_reachable(name):
    """What tests/test_ransac_gpu.py asserts on its scenes, established by the checker alone: planted inliers lie within
    0.25 thr and every other valid row beyond 4 thr of the planted motion; the float64 winner counts exactly the planted
    set and its refined mask is the planted set; at most 1 % of the drawn triples are ill determined; and the float32
    counts equal the float64 counts (no row sits on the threshold)."""
    sc, kw = ref.make_scene(name)
    worst_in, best_out = ref.scene_margins(sc)
    assert worst_in <= 0.25 and best_out >= 4.0, (worst_in, best_out)
    r64 = ref.run(sc["X"], sc["Y"], sc["corr"], sc["len1"], sc["len2"], dtype=np.float64, **kw)
    planted = sc["planted"].sum(1)
    n = np.arange(len(planted))
    assert np.array_equal(r64["counts"][n, r64["best"]], planted), (r64["counts"].max(1), planted)
    assert np.array_equal(r64["mask"], sc["planted"])
    ill = r64["valid"] & ~ref.well_determined(r64["sing"])
    assert ill.sum() <= 0.01 * r64["valid"].sum(), (ill.sum(), r64["valid"].sum())
    r32 = ref.run(sc["X"], sc["Y"], sc["corr"], sc["len1"], sc["len2"], dtype=np.float32, **kw)
    assert np.array_equal(r32["counts"], r64["counts"]) and np.array_equal(r32["mask"], r64["mask"])


def test_chunk_scenes_have_the_sizes_they_are_named_for():
    from pytorch3d_pointops_amd import _C_ransac

    c = _C_ransac.RANSAC_CHUNK
    assert c == ref.CHUNK
    for name, want in (("chunk-1", c - 1), ("chunk", c), ("chunk+1", c + 1), ("2chunk+1", 2 * c + 1)):
        sc, _ = ref.make_scene(name)
        tgt = ref.targets(sc["corr"], *(ref.lengths_of(None, 1, p) for p in (sc["X"].shape[1], sc["Y"].shape[1])), 1,
                          sc["X"].shape[1])
        assert (tgt >= 0).sum() == want, name


def test_rejected_refit_scene_rejects():
    """The scene of the GPU suite's rejected refinement: the float64 and the float32 checker both reject the first
    refit (it loses an inlier) and keep the winner, with room to spare on both sides of the threshold."""
    X, Y, samples, thr = ref.rejected_refit_scene()
    for dtype in (np.float32, np.float64):
        r = ref.run(X, Y, thr=thr, samples=samples, ratio=0.0, refine_steps=3, dtype=dtype)
        assert r["accepted"].tolist() == [0] and r["num_inliers"].tolist() == [X.shape[1]]
        tgt = r["tgt"]
        Rc, Tc, sc, _ = ref.fit_mask(X, Y, tgt, r["mask"], False)
        d = np.sqrt(ref.residual_d2(Rc[0], Tc[0], sc[0], X[0], Y[0], np.float64))
        assert (d > thr).sum() == 1 and np.abs(d - thr).min() > 0.05 * thr


# ------------------------------------------------------------------------------------------------ the public function
def test_exports():
    from pytorch3d_pointops_amd import functions

    assert "ransac_alignment" in functions.__all__ and "RansacSolution" in functions.__all__
    assert functions.RansacSolution._fields == ("RTs", "inliers", "num_inliers", "rmse", "best", "counts", "hypotheses",
                                                "samples")


def test_validation_errors():
    from pytorch3d_pointops_amd.functions import ransac_alignment

    X, Y = torch.rand(2, 8, 3), torch.rand(2, 9, 3)
    corr = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(TypeError):
        ransac_alignment(X, Y, corr)  # inlier_threshold is required
    with pytest.raises(ValueError, match=r"shape \(N, P, 3\)"):
        ransac_alignment(X[0], Y, corr, inlier_threshold=0.1)
    with pytest.raises(ValueError, match="float32"):
        ransac_alignment(X.double(), Y, corr, inlier_threshold=0.1)
    with pytest.raises(ValueError, match="same batch dimension"):
        ransac_alignment(X, Y[:1], corr, inlier_threshold=0.1)
    with pytest.raises(ValueError, match="same number of rows"):
        ransac_alignment(X, Y, inlier_threshold=0.1)
    with pytest.raises(ValueError, match=r"corr must be an int64 tensor of shape \(N, P1\)"):
        ransac_alignment(X, Y, corr.int(), inlier_threshold=0.1)
    with pytest.raises(ValueError, match=r"corr must be an int64 tensor of shape \(N, P1\)"):
        ransac_alignment(X, Y, corr[:, :7], inlier_threshold=0.1)
    with pytest.raises(ValueError, match=r"samples must be an int64 tensor of shape \(N, H, 3\)"):
        ransac_alignment(X, Y, corr, inlier_threshold=0.1, samples=torch.zeros(2, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="num_hypotheses"):
        ransac_alignment(X, Y, corr, inlier_threshold=0.1, num_hypotheses=0)
    with pytest.raises(ValueError, match="inlier_threshold"):
        ransac_alignment(X, Y, corr, inlier_threshold=-1.0)
    with pytest.raises(ValueError, match="inlier_threshold"):
        ransac_alignment(X, Y, corr, inlier_threshold=float("nan"))
    with pytest.raises(ValueError, match="edge_length_ratio"):
        ransac_alignment(X, Y, corr, inlier_threshold=0.1, edge_length_ratio=1.5)
    with pytest.raises(ValueError, match="refine_steps"):
        ransac_alignment(X, Y, corr, inlier_threshold=0.1, refine_steps=-1)
    with pytest.raises(ValueError, match="seed"):
        ransac_alignment(X, Y, corr, inlier_threshold=0.1, seed=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ransac_alignment(X, Y, corr, inlier_threshold=0.1)


def test_workspace_sizer_and_shape_limits():
    from pytorch3d_pointops_amd import _C

    size = _C._lib.pointops_ransac_workspace_bytes
    assert size(2, 1000, 64) > 2 * 1000 * 32 and size(1, 0, 1) > 0
    assert size(2, 1000, 128) > size(2, 1000, 64) and size(4, 1000, 64) > size(2, 1000, 64)
    assert size(65536, 4, 4) == 0 and size(1, 4, 0) == 0 and size(1, 4, (1 << 24) + 1) == 0


# ------------------------------------------------------------------------------------------------ native program
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_hypothesis_routines_hold_their_bounds(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "ransac_hypothesis")
    extra = ["-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] \
        if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout
