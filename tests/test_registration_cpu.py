"""registration_icp without a GPU.

    certificate  tests/registration_ref.py, the numpy checker of the REGISTRATION block of include/pointops_amd.h, run on
                 the very scenes tests/test_registration_gpu.py uses.  These are conditions of the INPUTS, asserted
                 here so that the GPU test cannot pass by accident: point-to-plane freezes as converged within 10
                 updates at the true pose, with and without clutter; trimmed point-to-point reaches the same pose; the
                 untrimmed run on the clutter case is off by more than 0.1; the planar target is refused.
    native       tests/native/icp_plane_main.cpp -- csrc/icp_plane.h and nothing else of the library -- compiled with the
                 hipcc and flags of pytorch3d_pointops_amd/build.py, once plain and once with the host sanitizers
                 (UBSan + ASan on the host side only) as a program of its own; its header derives every bound.
    checker      the checker's Cholesky against numpy's solve, its rotation and compose against each other
    arguments    the public functions refuse bad arguments with ValueError, CPU tensors with RuntimeError
"""
import ast
import os
import subprocess

import numpy as np
import pytest
import torch

import registration_ref as ref
from conftest import ROOT
from pytorch3d_pointops_amd import build as hip_build

SRC = os.path.join(ROOT, "tests", "native", "icp_plane_main.cpp")
SHAPES = ((2500, 3000), (700, 1100), (300, 400))  # the ragged base shape of the GPU test
SEED = 7


# ------------------------------------------------------------------------------------------------ the certificate
@pytest.mark.parametrize("clutter", [False, True], ids=["clean", "clutter"])
@pytest.mark.parametrize("P1,P2", SHAPES)
def test_point_to_plane_freezes_at_the_true_pose(P1, P2, clutter):
    sc = ref.scene(SEED, P1, P2, clutter)
    r = ref.icp(sc.X, sc.Y, P1, P2, ref.R_MAX, "point_to_plane", sc.normals)
    eR, eT = ref.pose_error(r.R, r.T, sc)
    print(f"point_to_plane {P1}x{P2} clutter={clutter}: {r.iterations} updates, |R-R*|={eR:.2e}, |T-T*|={eT:.2e}")
    assert r.status == ref.CONVERGED and r.iterations <= 10
    assert eR <= 1e-5 and eT <= 1e-5
    assert float(r.fitness) == sc.overlap / P1 and r.c == sc.overlap  # the overlap share, exactly
    assert float(r.inlier_rmse) < 1e-6


@pytest.mark.parametrize("clutter", [False, True], ids=["clean", "clutter"])
@pytest.mark.parametrize("P1,P2", SHAPES)
def test_trimmed_point_to_point_reaches_the_same_pose(P1, P2, clutter):
    sc = ref.scene(SEED, P1, P2, clutter)
    r = ref.icp(sc.X, sc.Y, P1, P2, ref.R_MAX, "point_to_point", max_iterations=60)
    eR, eT = ref.pose_error(r.R, r.T, sc)
    print(f"point_to_point {P1}x{P2} clutter={clutter}: {r.iterations} updates, |R-R*|={eR:.2e}, |T-T*|={eT:.2e}")
    assert r.status == ref.CONVERGED and eR <= 1e-5 and eT <= 1e-5
    plane = ref.icp(sc.X, sc.Y, P1, P2, ref.R_MAX, "point_to_plane", sc.normals)
    assert plane.iterations < r.iterations  # the reason for point-to-plane


@pytest.mark.parametrize("P1,P2", SHAPES)
def test_untrimmed_point_to_point_is_dragged_off_by_the_clutter(P1, P2):
    sc = ref.scene(SEED, P1, P2, True)
    r = ref.icp(sc.X, sc.Y, P1, P2, 1e3, "point_to_point", max_iterations=40)  # every row pulls
    eR, eT = ref.pose_error(r.R, r.T, sc)
    print(f"untrimmed {P1}x{P2}: |R-R*|={eR:.2f}, |T-T*|={eT:.2f}")
    assert eR > 0.1


def test_planar_target_trips_the_degeneracy_rule():
    P1, P2 = SHAPES[2]
    sc = ref.planar_scene(SEED, P1, P2)
    r = ref.icp(sc.X, sc.Y, P1, P2, ref.R_MAX, "point_to_plane", sc.normals)
    assert r.status == ref.DEGENERATE and r.iterations == 0 and r.c >= 6
    assert np.array_equal(r.R, np.eye(3)) and not r.T.any()
    idx, d2 = ref.nearest(sc.X, sc.Y, P1, P2)
    mask = ref.evaluate(d2, P1, P2, ref.R_MAX)[0]
    m = ref.plane_moments(sc.X, sc.Y, sc.normals, idx, mask)
    assert np.linalg.matrix_rank(m.A, tol=1e-9 * np.abs(m.A).max()) == 3


# ------------------------------------------------------------------------------------------------ the checker
def test_checker_cholesky_against_numpy():
    rng = np.random.default_rng(3)
    for cond in (1.0, 1e3, 1e6):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        A = (Q * cond ** (-np.arange(6) / 5.0)) @ Q.T
        A = (A + A.T) / 2
        b = rng.standard_normal(6)
        x, want = ref.cholesky_solve(A, b), np.linalg.solve(A, b)
        assert np.linalg.norm(x - want) <= 64 * cond * ref.U52 * np.linalg.norm(want)
    v = rng.standard_normal((3, 6))
    assert ref.cholesky_solve(v.T @ v, np.ones(6)) is None  # rank 3
    assert ref.cholesky_solve(np.zeros((6, 6)), np.ones(6)) is None


def test_checker_rotation_and_compose():
    rng = np.random.default_rng(4)
    for _ in range(50):
        a, b, g = rng.uniform(-3, 3, 3)
        Rd = ref.rotation_delta(a, b, g)
        assert np.abs(Rd @ Rd.T - np.eye(3)).max() <= 4 * ref.U52 and np.linalg.det(Rd) > 0
        # first order: x -> x Rd moves x by omega x x with omega = (a, b, g)
        eps = 1e-7
        x = rng.standard_normal(3)
        small = ref.rotation_delta(eps * a, eps * b, eps * g)
        assert np.allclose((x @ small - x) / eps, np.cross([a, b, g], x), atol=1e-5)
        R, T, c0, t = ref.rotation([1, 2, 3], 0.7), rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3)
        Rn, Tn = ref.compose(R, T, Rd, c0, t)
        assert np.allclose(x @ Rn + Tn, (x @ R + T - c0) @ Rd + c0 + t, atol=1e-13)


def test_checker_apply_and_evaluate():
    sc = ref.scene(1, 40, 60, True)
    Xt = ref.apply(sc.X, sc.R_true, sc.T_true, 37)
    assert Xt.dtype == np.float32 and not Xt[37:].any()
    idx, d2 = ref.nearest(Xt, sc.Y, 37, 60)
    full = ((Xt[:37, None].astype(np.float64) - sc.Y[None].astype(np.float64)) ** 2).sum(2)
    assert np.array_equal(idx[:37], full.argmin(1)) and not idx[37:].any() and not d2[37:].any()
    mask, c, fit, rmse, s = ref.evaluate(d2, 37, 60, ref.R_MAX)
    assert c == int(mask.sum()) and not mask[37:].any() and fit == np.float32(c / 37)
    assert ref.evaluate(d2, 37, 0, ref.R_MAX)[1] == 0 and ref.evaluate(d2, 0, 60, ref.R_MAX)[2] == 0


# ------------------------------------------------------------------------------------------------ the header, natively
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan+asan"])
def test_icp_plane_header_holds_its_bounds(tmp_path, sanitize):
    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "icp_plane")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    cmd = [hip_build.HIPCC] + hip_build.CXXFLAGS + extra + [SRC, "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, " ".join(cmd) + "\n" + c.stdout + c.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "no violation" in r.stdout and "VIOLATION" not in r.stdout


def test_the_degeneracy_constant_is_stated_once_everywhere():
    from pytorch3d_pointops_amd import _C_registration

    hdr = open(os.path.join(ROOT, "include", "pointops_amd.h")).read()
    h = open(os.path.join(ROOT, "pytorch3d_pointops_amd", "csrc", "icp_plane.h")).read()
    assert "constexpr double kIcpDegeneratePivot = 1e-10;" in h and "kIcpDegeneratePivot = 1e-10" in hdr
    assert ref.DEGENERATE_PIVOT == 1e-10 == _C_registration.DEGENERATE_PIVOT
    assert ref.MIN_INLIERS == _C_registration.MIN_INLIERS
    assert (ref.RUNNING, ref.CONVERGED, ref.DEGENERATE) == (_C_registration.RUNNING, _C_registration.CONVERGED,
                                                            _C_registration.DEGENERATE)


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_validation():
    from pytorch3d_pointops_amd.functions import (SimilarityTransform, evaluate_registration, registration_icp)
    from pytorch3d_pointops_amd.structures import Pointclouds

    x, y, n = torch.rand(2, 8, 3), torch.rand(2, 9, 3), torch.rand(2, 9, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        registration_icp(x, y, 0.1, target_normals=n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_registration(x, y, 0.1)
    with pytest.raises(ValueError, match="estimate_pointcloud_normals"):
        registration_icp(x, y, 0.1)
    with pytest.raises(ValueError, match="estimate_pointcloud_normals"):
        registration_icp(Pointclouds(list(x)), Pointclouds(list(y)), 0.1)
    with pytest.raises(ValueError, match="estimation must be one of"):
        registration_icp(x, y, 0.1, estimation="plane")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e39, "wide"):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            registration_icp(x, y, bad, estimation="point_to_point")
    with pytest.raises(ValueError, match="float32 clouds of dimension 3"):
        registration_icp(x.double(), y.double(), 0.1, estimation="point_to_point")
    with pytest.raises(ValueError, match="float32 clouds of dimension 3"):
        registration_icp(x[..., :2], y[..., :2], 0.1, estimation="point_to_point")
    with pytest.raises(ValueError, match="1 <= N < 65536"):
        registration_icp(x[:0], y[:0], 0.1, estimation="point_to_point")
    with pytest.raises(ValueError, match="same batch size"):
        registration_icp(x, y[:1], 0.1, estimation="point_to_point")
    with pytest.raises(ValueError, match="target_normals must be float32"):
        registration_icp(x, y, 0.1, target_normals=n[:, :5])
    with pytest.raises(ValueError, match="max_iterations"):
        registration_icp(x, y, 0.1, target_normals=n, max_iterations=0)
    with pytest.raises(ValueError, match="check_every"):
        registration_icp(x, y, 0.1, target_normals=n, check_every=-1)
    eye, zero = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError, match="scale s has to be 1"):
        registration_icp(x, y, 0.1, SimilarityTransform(eye, zero, torch.tensor([1.0, 2.0])), target_normals=n)
    with pytest.raises(ValueError, match="init_transform"):
        registration_icp(x, y, 0.1, (eye,), target_normals=n)
    with pytest.raises(ValueError, match="init_transform"):
        registration_icp(x, y, 0.1, (eye[:1], zero), target_normals=n)
    with pytest.raises(ValueError, match="transform"):
        evaluate_registration(x, y, 0.1, (eye, zero[:, :2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (a valid transform gets as far as the device check)
        registration_icp(x, y, 0.1, SimilarityTransform(eye, zero, torch.ones(2)), target_normals=n)


def test_functions_registration_allocates_nothing_itself():
    path = os.path.join(ROOT, "pytorch3d_pointops_amd", "functions", "registration.py")
    banned = {"empty", "empty_like", "new_empty", "zeros", "zeros_like", "new_zeros"}
    names = {n.attr for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Attribute)}
    names |= {n.id for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Name)}
    assert not names & banned, names & banned


def test_exports_and_container_methods():
    import pytorch3d_pointops_amd.functions as F
    from pytorch3d_pointops_amd.structures import Pointclouds

    assert F.RegistrationResult._fields == ("R", "T", "fitness", "inlier_rmse", "num_correspondences",
                                            "correspondences", "converged", "iterations", "status", "Xt", "history")
    assert F.RegistrationHistory._fields == ("R", "T", "fitness", "inlier_rmse")
    assert callable(F.registration_icp) and callable(F.evaluate_registration)
    assert callable(Pointclouds.registration_icp) and callable(Pointclouds.evaluate_registration)
