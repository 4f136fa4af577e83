"""GPU suite of the normals / local-frames feature (functions/points_normals.py, csrc/local_frames.hip).

The float64 reference is built from the SAME centred cloud and the SAME knn_points indices: get_point_covariances
(fp32, bit-equal to the covariance the fused kernel forms) -> float64 -> torch.linalg.eigh on the CPU -> the upstream
disambiguation rule in float64.  Gradients are compared with float64 autograd through that composition."""
import math

import numpy as np
import pytest
import torch

import cases
from pytorch3d_pointops_amd import synth

pytestmark = pytest.mark.gpu


def _api():
    from pytorch3d_pointops_amd.functions import points_normals

    return points_normals


def _clouds(name, N, P, seed):
    if name == "lattice":
        return cases.lattice(seed, N, P)
    return np.stack([synth.distribution(name, seed + n, P) for n in range(N)])


def _reference(points, lengths, K):
    """(centred, idx, knn, lam, V) -- V[..., :, j] = float64 eigenvector j of the fp32 covariance (CPU)."""
    from pytorch3d_pointops_amd.functions import get_point_covariances, knn_points

    c = _api().centre_clouds(points, lengths)
    idx = knn_points(c, c, lengths, lengths, K=K).idx
    cov, knn = get_point_covariances(c, lengths, K)
    lam, V = torch.linalg.eigh(cov.double().cpu())
    return c, idx, knn, lam, V


def _projections(c, knn, V):
    """(N,P,K,3) float64 projections (x_k - x_i) . v_j."""
    d = knn.double().cpu() - c.double().cpu()[:, :, None, :]
    return torch.einsum("npkd,npdj->npkj", d, V)


def _gaps(lam):
    """(N,P,3) distance of each eigenvalue to the nearest other one, and (N,P,1) largest |eigenvalue|."""
    g = torch.stack([torch.minimum((lam[..., i] - lam[..., (i + 1) % 3]).abs(),
                                   (lam[..., i] - lam[..., (i + 2) % 3]).abs()) for i in range(3)], -1)
    return g, lam.abs().amax(-1, keepdim=True)


def _valid(lengths, P):
    return (torch.arange(P)[None, :] < lengths.cpu()[:, None])


FORWARD_CASES = [(name, K) for name in ("uniform", "sphere", "planes", "aniso_100", "lattice") for K in (3, 8, 16, 50)]


@pytest.mark.parametrize("name,K", FORWARD_CASES + [("uniform", 80), ("sphere", 80)])
def test_against_float64_eigh(dev, name, K):
    from pytorch3d_pointops_amd.structures import Pointclouds

    N, P = 3, (300 if name == "lattice" else 700)
    pts = torch.from_numpy(_clouds(name, N, P, 4000 + K)).to(dev)
    lens = [P, P - 137, K + 1]
    pc = Pointclouds([pts[n, :lens[n]] for n in range(N)])
    lengths = pc.num_points_per_cloud()
    curv, frames = _api().estimate_pointcloud_local_coord_frames(pc, K)
    _, raw = _api().estimate_pointcloud_local_coord_frames(pc, K, False)
    c, idx, knn, lam, V = _reference(pc.points_padded(), lengths, K)
    valid = _valid(lengths, P)
    curv, frames, raw = curv.double().cpu(), frames.double().cpu(), raw.double().cpu()

    lmax = lam.abs().amax(-1, keepdim=True)
    err = (curv - lam).abs()
    assert bool((err[valid] <= 1e-5 * lmax[valid] + 1e-12).all()), float((err - 1e-5 * lmax)[valid].max())
    gap, _ = _gaps(lam)
    sep = (gap >= 1e-3 * lmax) & valid[..., None]
    for f in (frames, raw):
        dots = (f * V).sum(-2).abs()  # |v_j . v_ref_j| per column
        assert bool((1 - dots[sep] <= 1e-5).all()), float((1 - dots)[sep].max())
        assert torch.allclose((f * f).sum(-2)[valid], torch.ones(3, dtype=torch.float64), atol=1e-6)

    # disambiguated signs: the upstream rule in float64 on the reference eigenvectors
    proj = _projections(c, knn, V)
    flip = (proj > 0).sum(2) < 0.5 * K  # (N,P,3)
    want = V * torch.where(flip, -1.0, 1.0)[..., None, :]
    clear = (proj.abs() > 1e-6).all(2) & sep  # no projection near zero, well separated eigenvalue
    for j in (0, 2):
        agree = (frames[..., :, j] * want[..., :, j]).sum(-1) > 0
        assert bool(agree[clear[..., j]].all()), (j, int((~agree & clear[..., j]).sum()))
    # y = n x z
    y = torch.cross(frames[..., :, 0], frames[..., :, 2], dim=-1)
    assert torch.allclose(frames[..., :, 1][valid], y[valid], atol=1e-6)
    # padded rows are zero
    assert bool((curv[~valid] == 0).all()) and bool((frames[~valid] == 0).all())


def test_sphere_and_planes_geometry(dev):
    """Sphere: normals radial (99 % within 1 degree, all within 2: the fit is radial at the neighbourhood, not exactly
    at the point).  The majority rule orients a convex surface's normals to its inside -- every neighbour lies below
    the outward tangent plane --, so the disambiguated normals point to the centre on >= 99 % of points.
    Planes (noise 1e-3 of the plane extent): normals are +-z, at K = 50 99 % within 1 degree, all within 2."""
    est = _api().estimate_pointcloud_normals
    p = torch.from_numpy(synth.distribution("sphere", 3, 60000)).to(dev)[None]
    nrm = est(p, 16)
    radial = p - 0.5
    radial = radial / radial.norm(dim=-1, keepdim=True)
    cosv = (nrm * radial).sum(-1)
    ang = torch.rad2deg(torch.arccos(cosv.abs().clamp(max=1.0)))
    assert float((ang <= 1.0).float().mean()) >= 0.99 and float(ang.max()) <= 2.0
    assert float((cosv < 0).float().mean()) >= 0.99
    assert torch.allclose(nrm.norm(dim=-1), torch.ones_like(cosv), atol=1e-5)

    p = torch.from_numpy(synth.distribution("planes", 4, 20000)).to(dev)[None]
    nrm = est(p, 50)
    ang = torch.rad2deg(torch.arccos(nrm[..., 2].abs().clamp(max=1.0)))
    assert float((ang <= 1.0).float().mean()) >= 0.99 and float(ang.max()) <= 2.0


def test_container_and_edge_rows(dev):
    from pytorch3d_pointops_amd.structures import Pointclouds

    api = _api()
    # padded rows are zero
    pts = torch.from_numpy(cases.cloud(4101, (2, 500, 3))).to(dev)
    pc = Pointclouds([pts[0], pts[1, :321]])
    curv, frames = api.estimate_pointcloud_local_coord_frames(pc, 12)
    assert bool((curv[1, 321:] == 0).all()) and bool((frames[1, 321:] == 0).all())
    assert bool((curv[1, :321, 2] > 0).all())
    # a cloud of identical points: zero covariance -> zero curvatures, identity frame before disambiguation
    same = torch.tensor([0.5, 0.25, -1.0], device=dev).expand(1, 64, 3).contiguous()
    curv, frames = api.estimate_pointcloud_local_coord_frames(same, 8, False)
    assert bool((curv == 0).all())
    assert torch.equal(frames, torch.eye(3, device=dev).expand(1, 64, 3, 3))
    # Pointclouds and tensor inputs give identical results
    full = pts.clone()
    a = api.estimate_pointcloud_local_coord_frames(full, 16)
    b = api.estimate_pointcloud_local_coord_frames(Pointclouds(full), 16)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(api.estimate_pointcloud_normals(full, 16), a[1][..., :, 0])
    # estimate_normals(assign_to_self=True) stores the padded feature "normals", replacing an existing one
    pc = Pointclouds(full, features={"normals": torch.zeros_like(full)})
    nrm = pc.estimate_normals(16, assign_to_self=True)
    assert torch.equal(nrm, a[1][..., :, 0])
    assert torch.equal(pc.features_padded()["normals"], nrm)
    assert torch.equal(pc.features_packed()["normals"], nrm.reshape(-1, 3))
    pc2 = Pointclouds([pts[0], pts[1, :321]])
    nrm2 = pc2.estimate_normals(12, disambiguate_directions=True)
    assert pc2.feature_names() == [] and nrm2.shape == (2, 500, 3)


def _reference_grads(leaves, lengths, idx, K, disambiguate, frames_ours, g_curv, g_frames):
    """float64 autograd through centring, gather, covariance, eigh and the frame assembly (CPU)."""
    api = _api()
    N = len(leaves)
    P = max(t.shape[0] for t in leaves)
    x = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    padded = torch.nn.utils.rnn.pad_sequence(x, batch_first=True)
    lens = lengths.cpu()
    c = api.centre_clouds(padded, lens)
    ii = idx.cpu()
    knn = torch.stack([c[n][ii[n]] for n in range(N)])  # (N,P,K,3)
    d = knn - knn.mean(2, keepdim=True)
    cov = (d[..., :, None] * d[..., None, :]).mean(2)
    valid = _valid(lens, P)
    cov = torch.where(valid[..., None, None], cov, torch.diag(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)))
    lam, V = torch.linalg.eigh(cov)
    fo = frames_ours.double().cpu()
    sign = torch.where((V * fo).sum(-2) < 0, -1.0, 1.0).detach()  # the kernel's signs (piecewise constant)
    V = V * sign[..., None, :]
    if disambiguate:
        n, z = V[..., :, 0], V[..., :, 2]
        V = torch.stack([n, torch.cross(n, z, dim=-1), z], -1)
    loss = (lam * g_curv.double().cpu()).sum() + (V * g_frames.double().cpu()).sum()
    loss.backward()
    return [t.grad for t in x], lam.detach()


@pytest.mark.parametrize("disambiguate", [True, False])
def test_gradients_against_float64(dev, disambiguate):
    from pytorch3d_pointops_amd.functions import knn_points
    from pytorch3d_pointops_amd.structures import Pointclouds

    K, P = 16, 400
    base = torch.from_numpy(cases.cloud(4201, (2, P, 3))).to(dev)
    leaves = [base[0].clone().requires_grad_(True), base[1, :333].clone().requires_grad_(True)]
    pc = Pointclouds(leaves)
    lengths = pc.num_points_per_cloud()
    curv, frames = _api().estimate_pointcloud_local_coord_frames(pc, K, disambiguate)
    c = _api().centre_clouds(pc.points_padded().detach(), lengths)
    idx = knn_points(c, c, lengths, lengths, K=K).idx

    g = torch.Generator().manual_seed(17)
    g_curv = torch.randn(curv.shape, generator=g, dtype=torch.float64)
    g_frames = torch.randn(frames.shape, generator=g, dtype=torch.float64)
    lam = curv.detach().double().cpu()
    gap, lmax = _gaps(lam)
    ill = (gap.amin(-1) < 1e-2 * lmax[..., 0]) | ~_valid(lengths, P)
    g_curv[ill] = 0
    g_frames[ill] = 0
    ref, _ = _reference_grads(leaves, lengths, idx, K, disambiguate, frames.detach(), g_curv, g_frames)
    got = torch.autograd.grad((curv * g_curv.float().to(dev)).sum() + (frames * g_frames.float().to(dev)).sum(),
                              leaves)
    for u, v in zip(got, ref):
        assert bool(torch.isfinite(u).all())
        scale = float(v.abs().max())
        assert scale > 0 and float((u.double().cpu() - v).abs().max()) <= 1e-3 * scale


def test_reproducible(dev):
    api = _api()
    pts = torch.from_numpy(cases.cloud(4301, (2, 3000, 3))).to(dev)
    a = api.estimate_pointcloud_local_coord_frames(pts, 16)
    b = api.estimate_pointcloud_local_coord_frames(pts, 16)
    assert all(torch.equal(u, v) for u, v in zip(a, b))

    def grad():
        p = pts.clone().requires_grad_(True)
        curv, frames = api.estimate_pointcloud_local_coord_frames(p, 16)
        w = torch.linspace(-1, 1, frames.numel(), device=dev).reshape(frames.shape)
        (curv.sum() + (frames * w).sum()).backward()
        return p.grad

    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        g1, g2 = grad(), grad()
    finally:
        torch.use_deterministic_algorithms(prev)
    assert torch.equal(g1, g2) and bool(torch.isfinite(g1).all())


def test_graph_capture_and_compile(dev):
    from pytorch3d_pointops_amd import graphs, ops
    from pytorch3d_pointops_amd.functions import knn_points

    assert {"local_frames", "local_frames_backward"} <= set(ops.registered_ops())
    est = _api().estimate_pointcloud_normals

    def fn(p):
        return est(p, 16)

    g = torch.Generator().manual_seed(5)
    a = torch.rand((2, 2048, 3), generator=g).to(dev)
    step = graphs.capture(fn, (a,))
    assert torch.equal(step(), fn(a))
    a2 = torch.rand((2, 2048, 3), generator=g).to(dev) ** 2
    want = fn(a2)
    assert torch.equal(step(a2), want)

    # torch.compile traces the public function through the registered ops (aot_eager: eager numerics)
    b = a2.clone().requires_grad_(True)
    out = torch.compile(fn, backend="aot_eager")(b)
    assert torch.equal(out, want)
    out.sum().backward()
    b2 = a2.clone().requires_grad_(True)
    fn(b2).sum().backward()
    assert torch.allclose(b.grad, b2.grad, rtol=1e-5, atol=1e-5 * float(b2.grad.abs().max()))
    # the raw op is differentiable on its own as well
    c = a2.clone().requires_grad_(True)
    lengths = torch.full((2,), 2048, dtype=torch.int64, device=dev)
    cen = _api().centre_clouds(c, lengths)
    idx = knn_points(cen.detach(), cen.detach(), lengths, lengths, K=16).idx
    curv, frames = torch.ops.pointops_amd.local_frames(cen, lengths, idx, True)
    assert torch.equal(frames[..., :, 0], want)
    frames[..., :, 0].sum().backward()
    assert torch.allclose(c.grad, b2.grad, rtol=1e-5, atol=1e-5 * float(b2.grad.abs().max()))
    assert not math.isnan(float(c.grad.sum()))
