"""CPU suite of the registration feature (functions/points_alignment.py, csrc/points_alignment.hip): the float64
checker checked against known transforms and SVD-free closed forms, the public names and defaults, every ValueError
(raised before any device work), the torch composition against the checker, and the C ABI entries."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import points_alignment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _random_rotations(N, seed, max_angle=3.0):
    g = torch.Generator().manual_seed(seed)
    axes = torch.randn((N, 3), generator=g, dtype=torch.float64)
    angles = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * max_angle
    return torch.stack([ref.rotation(axes[n], angles[n]) for n in range(N)])


# ------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("estimate_scale", [False, True])
def test_checker_recovers_known_transform(estimate_scale):
    N, P = 4, 50
    X = _rand((N, P, 3), 1)
    R = _random_rotations(N, 2)
    T = _rand((N, 3), 3) - 0.5
    s = 0.5 + _rand((N,), 4) if estimate_scale else torch.ones(N, dtype=torch.float64)
    Y = ref.apply(X, R, T, s)
    w = _rand((N, P), 5)
    for weights in (None, w):
        R2, T2, s2, S = ref.alignment(X, Y, weights, estimate_scale=estimate_scale)
        assert bool(ref.well_determined(S).all())
        assert float((R2 - R).abs().max()) <= 1e-12
        assert float((T2 - T).abs().max()) <= 1e-12
        assert float((s2 - s).abs().max()) <= 1e-12


def test_checker_mirrored_input():
    N, P = 3, 40
    X = _rand((N, P, 3), 6) - 0.5
    Y = X * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64) + 0.25  # a reflection
    R, T, s, _ = ref.alignment(X, Y)
    assert torch.allclose(torch.linalg.det(R), torch.ones(N, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(N, 3, 3), atol=1e-12)
    R, T, s, _ = ref.alignment(X, Y, allow_reflection=True)
    assert torch.allclose(torch.linalg.det(R), -torch.ones(N, dtype=torch.float64), atol=1e-12)
    assert float((ref.apply(X, R, T, s) - Y).abs().max()) <= 1e-12


def test_checker_two_points_closed_form():
    """Two points: C = dx dy^T / 4, so s = |dy| / |dx| and both points are mapped exactly -- no SVD needed."""
    x = torch.tensor([[[0.1, 0.2, 0.3], [0.9, -0.4, 0.5]]], dtype=torch.float64)
    Rt = ref.rotation([1.0, 2.0, -1.0], 0.7)
    y = 1.7 * (x @ Rt) + torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    R, T, s, S = ref.alignment(x, y, estimate_scale=True)
    dx, dy = x[0, 1] - x[0, 0], y[0, 1] - y[0, 0]
    assert abs(float(s[0]) - float(dy.norm() / dx.norm())) <= 1e-12
    assert abs(float(S[0, 0]) - float(dx.norm() * dy.norm() / 4)) <= 1e-12 and float(S[0, 1]) <= 1e-15
    assert float((ref.apply(x, R, T, s) - y).abs().max()) <= 1e-12
    assert abs(float(torch.linalg.det(R)[0]) - 1) <= 1e-12


def test_checker_collinear_closed_form():
    """Points t_i u + a against k t_i v + b: s = k, u R = v and every point is mapped exactly."""
    t = torch.linspace(-1, 2, 9, dtype=torch.float64)
    u = torch.tensor([1.0, 2.0, 2.0], dtype=torch.float64) / 3
    v = torch.tensor([-2.0, 1.0, 2.0], dtype=torch.float64) / 3
    x = (t[:, None] * u + torch.tensor([0.5, 0.1, -0.3], dtype=torch.float64))[None]
    y = (1.3 * t[:, None] * v + torch.tensor([-0.2, 0.4, 0.6], dtype=torch.float64))[None]
    R, T, s, S = ref.alignment(x, y, estimate_scale=True)
    assert abs(float(s[0]) - 1.3) <= 1e-12
    assert float((u @ R[0] - v).abs().max()) <= 1e-12
    assert float((ref.apply(x, R, T, s) - y).abs().max()) <= 1e-12
    assert not bool(ref.well_determined(S)[0])


def test_checker_icp_recovers_small_motion():
    Y = _rand((2, 300, 3), 7)
    Rt = torch.stack([ref.rotation([1.0, 0.5, -0.2], 0.05), ref.rotation([0.0, 1.0, 1.0], -0.04)])
    Tt = torch.tensor([[0.01, -0.01, 0.005], [0.0, 0.01, -0.01]], dtype=torch.float64)
    X = (Y[:, :200] - Tt[:, None]) @ Rt.transpose(1, 2)  # X R + T = Y rows
    sol = ref.icp(X, Y, len_x=[200, 150], len_y=[300, 280])
    assert sol.converged and sol.iterations == len(sol.history)
    assert float((sol.R - Rt).abs().max()) <= 1e-9 and float((sol.T - Tt).abs().max()) <= 1e-9
    assert float(sol.rmse.max()) <= 1e-9
    assert bool((sol.Xt[1, 150:] == 0).all())


# ------------------------------------------------------------------------------------------------ the public API
def test_public_names_and_defaults():
    from pytorch3d_pointops_amd import functions
    from pytorch3d_pointops_amd.functions import points_alignment as pa

    names = {"corresponding_points_alignment", "iterative_closest_point", "SimilarityTransform", "ICPSolution",
             "convert_pointclouds_to_tensor"}
    assert names <= set(functions.__all__)
    assert pa.SimilarityTransform._fields == ("R", "T", "s")
    assert pa.ICPSolution._fields == ("converged", "rmse", "Xt", "RTs", "t_history")
    sig = inspect.signature(pa.corresponding_points_alignment)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [
        ("X", inspect.Parameter.empty), ("Y", inspect.Parameter.empty), ("weights", None), ("estimate_scale", False),
        ("allow_reflection", False), ("eps", 1e-9)]
    sig = inspect.signature(pa.iterative_closest_point)
    public = [(k, v.default) for k, v in sig.parameters.items() if v.kind is not inspect.Parameter.KEYWORD_ONLY]
    assert public == [("X", inspect.Parameter.empty), ("Y", inspect.Parameter.empty), ("init_transform", None),
                      ("max_iterations", 100), ("relative_rmse_thr", 1e-6), ("estimate_scale", False),
                      ("allow_reflection", False), ("verbose", False)]
    assert "differentiable" in pa.iterative_closest_point.__doc__


def test_convert_pointclouds_to_tensor():
    from pytorch3d_pointops_amd.functions import convert_pointclouds_to_tensor
    from pytorch3d_pointops_amd.structures import Pointclouds

    t = torch.rand(2, 5, 3)
    padded, lengths = convert_pointclouds_to_tensor(t)
    assert padded is t and lengths.tolist() == [5, 5] and lengths.dtype == torch.int64
    pc = Pointclouds([torch.rand(4, 3), torch.rand(2, 3)])
    padded, lengths = convert_pointclouds_to_tensor(pc)
    assert padded.shape == (2, 4, 3) and lengths.tolist() == [4, 2]
    with pytest.raises(ValueError):
        convert_pointclouds_to_tensor([t])
    with pytest.raises(ValueError):
        convert_pointclouds_to_tensor(torch.rand(5, 3))


def test_value_errors():
    from pytorch3d_pointops_amd.functions import corresponding_points_alignment as cpa
    from pytorch3d_pointops_amd.functions import iterative_closest_point as icp
    from pytorch3d_pointops_amd.functions.points_alignment import SimilarityTransform
    from pytorch3d_pointops_amd.structures import Pointclouds

    X = torch.rand(2, 10, 3)
    with pytest.raises(ValueError):
        cpa(X, torch.rand(2, 11, 3))
    with pytest.raises(ValueError):
        cpa(X, torch.rand(3, 10, 3))
    with pytest.raises(ValueError):
        cpa(X, torch.rand(2, 10, 2))
    with pytest.raises(ValueError):
        cpa(X, X, weights=torch.rand(2, 9))
    with pytest.raises(ValueError):  # equal padded shapes, different lengths
        cpa(Pointclouds([torch.rand(10, 3), torch.rand(7, 3)]), Pointclouds([torch.rand(10, 3), torch.rand(8, 3)]))
    with pytest.raises(ValueError):
        cpa("X", X)

    with pytest.raises(ValueError):
        icp(X, torch.rand(3, 12, 3))
    with pytest.raises(ValueError):
        icp(X, torch.rand(2, 12, 2))
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_iterations"):
            icp(X, torch.rand(2, 12, 3), max_iterations=bad)
    eye, zero, one = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.ones(2)
    for init in (SimilarityTransform(torch.eye(3), zero, one), SimilarityTransform(eye, torch.zeros(2, 2), one),
                 SimilarityTransform(eye, zero, torch.ones(3)), (eye, zero), SimilarityTransform(eye, zero, 1.0)):
        with pytest.raises(ValueError, match="init_transform"):
            icp(X, torch.rand(2, 12, 3), init_transform=init)
    # valid arguments reach the search, which has no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        icp(X, torch.rand(2, 12, 3))


@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("estimate_scale,allow_reflection", [(False, False), (True, False), (True, True)])
def test_torch_composition_against_checker(d, estimate_scale, allow_reflection):
    """CPU float64 tensors take the torch composition: it must be the checker's definition."""
    from pytorch3d_pointops_amd.functions import corresponding_points_alignment as cpa
    from pytorch3d_pointops_amd.structures import Pointclouds

    N, P = 3, 30
    X, Y = _rand((N, P, d), 10 + d), _rand((N, P, d), 20 + d) * 2 - 0.3
    w = _rand((N, P), 30 + d)
    for weights in (None, w):
        got = cpa(X, Y, weights, estimate_scale, allow_reflection)
        R, T, s, _ = ref.alignment(X, Y, weights, estimate_scale, allow_reflection)
        assert torch.allclose(got.R, R, atol=1e-10) and torch.allclose(got.T, T, atol=1e-10)
        assert torch.allclose(got.s, s, atol=1e-10)
    if d == 3:  # containers: rows past the lengths weigh nothing
        lens = [30, 17, 5]
        pcx = Pointclouds([X[n, :lens[n]].float() for n in range(N)])
        pcy = Pointclouds([Y[n, :lens[n]].float() for n in range(N)])
        got = cpa(pcx, pcy, None, estimate_scale, allow_reflection)
        mask = ref.valid_mask(lens, P).double()
        R, T, s, _ = ref.alignment(X.float(), Y.float(), mask, estimate_scale, allow_reflection)
        assert got.R.dtype == torch.float32
        assert torch.allclose(got.R.double(), R, atol=1e-4) and torch.allclose(got.T.double(), T, atol=1e-4)
        assert torch.allclose(got.s.double(), s, atol=1e-4)


def test_torch_composition_gradients_against_checker():
    from pytorch3d_pointops_amd.functions import corresponding_points_alignment as cpa

    X, Y, w = _rand((2, 25, 3), 40), _rand((2, 25, 3), 41), _rand((2, 25), 42)
    gR, gT, gs = _rand((2, 3, 3), 43) - 0.5, _rand((2, 3), 44) - 0.5, _rand((2,), 45) - 0.5

    def grads(fn):
        leaves = [t.clone().requires_grad_(True) for t in (X, Y, w)]
        R, T, s = fn(*leaves)[:3]
        return torch.autograd.grad((R * gR).sum() + (T * gT).sum() + (s * gs).sum(), leaves)

    ours = grads(lambda a, b, c: cpa(a, b, c, estimate_scale=True))
    want = grads(lambda a, b, c: ref.alignment(a, b, c, estimate_scale=True))
    for u, v in zip(ours, want):
        assert float((u - v).abs().max()) <= 1e-9 * max(1.0, float(v.abs().max()))


def test_low_rank_warnings():
    from pytorch3d_pointops_amd.functions import corresponding_points_alignment as cpa

    with pytest.warns(UserWarning, match="dim\\+1"):
        cpa(torch.rand(1, 3, 3, dtype=torch.float64), torch.rand(1, 3, 3, dtype=torch.float64))
    line = torch.linspace(0, 1, 8, dtype=torch.float64)[None, :, None] * torch.ones(3, dtype=torch.float64)
    with pytest.warns(UserWarning, match="low rank"):
        cpa(line, line + 1.0)


def test_module_is_self_contained():
    text = open(os.path.join(ROOT, "pytorch3d_pointops_amd", "functions", "points_alignment.py")).read()
    assert "oracle" not in text.lower()


def test_c_abi_entries_declared_and_exported():
    from pytorch3d_pointops_amd import _C

    hdr = open(os.path.join(ROOT, "include", "pointops_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pointops_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ("pointops_points_alignment_workspace_bytes", "pointops_points_alignment",
                 "pointops_points_alignment_backward", "pointops_icp_workspace_bytes", "pointops_icp_iteration"):
        assert name in declared and name in _C.exported_symbols() and hasattr(lib, name)
    lib.pointops_points_alignment_workspace_bytes.restype = ctypes.c_size_t
    lib.pointops_points_alignment_workspace_bytes.argtypes = [ctypes.c_int64] * 3
    lib.pointops_icp_workspace_bytes.restype = ctypes.c_size_t
    lib.pointops_icp_workspace_bytes.argtypes = [ctypes.c_int64] * 3
    # one layout per operator (arrays padded to 256 bytes): 24 fp64 moments per block partial, and the ICP layout
    # adds the residual partials
    assert lib.pointops_points_alignment_workspace_bytes(2, 100, 3) == 512 >= 2 * 24 * 8
    assert lib.pointops_points_alignment_workspace_bytes(8, 65536, 3) == 8 * 32 * 24 * 8
    assert lib.pointops_icp_workspace_bytes(8, 65536, 3) == 8 * 32 * 24 * 8 + 8 * 32 * 8
    assert lib.pointops_points_alignment_workspace_bytes(2, 100, 4) == 0  # d = 4 is the torch composition's
