"""Randomised soak of the derived operators -- cluster_dbscan, remove_radius_outlier, iss_keypoints, voxel_downsample,
the statistical filter's boundary, mask_to_index, segment_plane, ransac_alignment and the evaluate-only step of
registration_icp -- on the ragged cases of tests/fuzz_derived_cases.py (certified on the CPU by
tests/test_fuzz_derived_cpu.py).  Every case asserts

  (a) the result equals the numpy checker, by the rule of the operator's own suite (imported, not restated: no bound is
      set in this file)
  (b) every path a knob of csrc/debug.h can force gives the bytes of the path the library chooses
  (c) on every third case, a caller whose tensors are strided views -- points as `wide[..., :D]` of an xyz+rgb tensor or
      as a transposed storage, lengths as `long[1::2]`, features, masks, tables, samples and origins likewise -- gets the
      bytes of the contiguous call, and keeps its tensors as they were
  (d) where the documentation promises it (filters, voxel, ISS, cluster, registration), one random live cloud alone, at
      the same P and its own length, gives the rows it has in the batch

and prints the dict that reproduces the case when it fails.  POINTOPS_FUZZ_SOAK=<int> draws fresh cases."""
import numpy as np
import pytest
import torch

import cluster_ref
import filters_ref
import fuzz_derived_cases as gen
import registration_ref
import voxel_ref
from filters_cases import KEYS as RADIUS_KEYS
from test_cluster_gpu import _assert_equal as assert_cluster_equal
from test_filters_gpu import _assert_equal as assert_filters_equal
from test_iss_gpu import KEYS as ISS_KEYS
from test_iss_gpu import _check_stages as check_iss_stages
from test_plane_gpu import NAMES as PLANE_KEYS
from test_plane_gpu import check_stages as check_plane_stages
from test_ransac_gpu import check_stages as check_ransac_stages
from test_voxel_gpu import KEYS as VOXEL_KEYS
from test_voxel_gpu import _check_stages as check_voxel_stages

pytestmark = pytest.mark.gpu

RANSAC_KEYS = "R T s mask num_inliers rmse best counts hyp_R hyp_T hyp_s samples".split()
STAT_KEYS = ("mask", "index", "num_kept", "mean_distance", "threshold", "stats")


def _T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same_bytes(got, want, what):
    for k, a in got.items():
        b = want[k]
        if a is None or b is None:
            assert a is None and b is None, (what, k)
            continue
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
            f"{what}: {k} is not byte-equal ({int((a != b).sum()) if a.shape == b.shape else 'shapes differ'} places)"


# ------------------------------------------------------------------------------------------------ strided callers
def _filler(t):
    if t.dtype == torch.bool:
        return True
    return 7 if t.dtype == torch.int64 else 7.5


def _interleaved(t, dim):
    """(`long[..., 1::2]` along `dim` of a storage twice as long there, holding `t`'s values; the storage)"""
    shape = list(t.shape)
    shape[dim] = 2 * shape[dim] + 1
    base = torch.full(shape, _filler(t), dtype=t.dtype, device=t.device)
    view = base[(slice(None),) * dim + (slice(1, None, 2),)]
    view.copy_(t)
    return view, base


def _wide(t):
    """(`wide[..., :D]` of an (..., D + 3) tensor, the wide tensor)"""
    base = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), _filler(t), dtype=t.dtype, device=t.device)
    base[..., :t.shape[-1]] = t
    return base[..., :t.shape[-1]], base


def _transposed(t):
    """(an (N, P, D) view of an (N, D, P) storage, the storage)"""
    base = t.transpose(1, 2).contiguous()
    return base.transpose(1, 2), base


def _strided(tensors, turn, rows=("points", "X", "Y", "normals", "features", "dists")):
    """Every tensor of the call as a view of the same values in a larger or permuted storage -> (views, storages)."""
    views, bases = {}, {}
    for j, (k, t) in enumerate(tensors.items()):
        if t is None:
            views[k] = None
            continue
        if k in rows:
            views[k], bases[k] = (_wide, _transposed)[(turn + j) % 2](t)
        else:  # lengths, masks, corr, samples, origins: every other element along the first or the last dimension
            views[k], bases[k] = _interleaved(t, 0 if t.dim() == 1 else t.dim() - 1)
        assert torch.equal(views[k], t)
    return views, bases


def _soak(dev, monkeypatch, cases, tensors, call, check, knobs=(), alone=None, shared=lambda c: (), public=None,
          handed_back=()):
    """(a)-(d) of the module docstring over `cases`.  tensors(case) -> {name: numpy or None}; call(case, {name: tensor})
    -> {key: numpy}; check(case, result) asserts (a); alone(case) -> the lengths (d) picks a live cloud by, shared(case)
    -> the tensors that cloud keeps whole; `public`: the call a strided caller makes where it is another than `call`
    (its keys are a subset); `handed_back`: outputs the strided caller passes in again, as views, under the same names."""
    for i, c in enumerate(cases):
        t = {k: _T(v, dev) for k, v in tensors(c).items()}
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
        first = call(c, t)
        try:
            check(c, first)
        except AssertionError as e:
            if str(c.what) in str(e):
                raise
            raise AssertionError(f"{c.what}: {e}") from e
        for knob in knobs:
            monkeypatch.setenv("POINTOPS_DEBUG", knob)
            _same_bytes(call(c, t), first, f"{c.what} [{knob}]")
        monkeypatch.delenv("POINTOPS_DEBUG", raising=False)
        if i % 3 == 0:
            views, bases = _strided({**t, **{k: _T(first[k], dev) for k in handed_back}}, i // 3)
            before = {k: b.clone() for k, b in bases.items()}
            _same_bytes((public or call)(c, views), first, f"{c.what} [strided caller]")
            for k, b in bases.items():
                assert torch.equal(b, before[k]), f"{c.what}: the caller's {k} was written"
        if alone is not None and (alone(c) > 0).any():
            n = int(np.random.default_rng(i).choice(np.flatnonzero(alone(c) > 0)))
            one = {k: v if v is None or k in shared(c) else v[n:n + 1] for k, v in t.items()}
            _same_bytes(call(c, one), {k: None if v is None else v[n:n + 1] for k, v in first.items()},
                        f"{c.what} [cloud {n} alone]")


# ------------------------------------------------------------------------------------------------ the radius family
@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_cluster_dbscan(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import functions as f

    def call(c, t):
        r = f.cluster_dbscan(t["points"], c.radius, c.min_points, lengths=t["lengths"])
        return dict(labels=_np(r.labels), num_clusters=_np(r.num_clusters), core_mask=_np(r.core_mask))

    def check(c, got):
        want = cluster_ref.dbscan(c.points, c.lengths, c.radius, c.min_points)
        assert_cluster_equal(tuple(got.values()), want, str(c.what))

    _soak(dev, monkeypatch, gen.radius_family_cases(seed), lambda c: dict(points=c.points, lengths=c.lengths), call, check,
          knobs=("cluster_grid=0", "cluster_grid=1"), alone=lambda c: c.lengths)


@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_remove_radius_outlier(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import functions as f

    def call(c, t):
        r = f.remove_radius_outlier(t["points"], t["lengths"], radius=c.radius, min_neighbors=c.min_points,
                                    return_counts=True)
        early = f.remove_radius_outlier(t["points"], t["lengths"], radius=c.radius, min_neighbors=c.min_points)
        assert early.counts is None and torch.equal(early.mask, r.mask) and torch.equal(early.index, r.index), c.what
        return {k: _np(getattr(r, k)) for k in RADIUS_KEYS}

    def check(c, got):
        want = filters_ref.radius(c.points, c.lengths, c.radius, c.min_points)
        assert_filters_equal(got, want, RADIUS_KEYS, str(c.what))

    _soak(dev, monkeypatch, gen.radius_family_cases(seed), lambda c: dict(points=c.points, lengths=c.lengths), call, check,
          knobs=("filter_grid=0", "filter_grid=1"), alone=lambda c: c.lengths)


@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_iss_keypoints(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import _C_iss
    from pytorch3d_pointops_amd import functions as f

    g = 0.975

    def call(c, t):  # the boundary: it has the diagnostic moments
        out = _C_iss.iss_keypoints(t["points"], t["lengths"], c.radius, c.rn, g, g, c.min_points, want_moments=True)
        return dict(zip(ISS_KEYS, (_np(x) for x in out)))

    def public(c, t):
        r = f.iss_keypoints(t["points"], t["lengths"], salient_radius=c.radius, non_max_radius=c.rn, gamma_21=g, gamma_32=g,
                            min_neighbors=c.min_points)
        assert np.array_equal(_np(r.num_keypoints), _np(r.mask).sum(1)), c.what
        return {k: _np(getattr(r, k)) for k in ISS_KEYS[:3]}

    def check(c, got):
        check_iss_stages(got, None, (c.points, c.lengths, c.radius, c.rn, g, g, c.min_points), str(c.what))

    cases = [c for c in gen.radius_family_cases(seed) if c.D == 3]
    _soak(dev, monkeypatch, cases, lambda c: dict(points=c.points, lengths=c.lengths), call, check,
          knobs=("iss_grid=0", "iss_grid=1"), alone=lambda c: c.lengths, public=public)


def _two_small_clouds(P, ragged):
    """N = 2 uniform clouds of P rows, lengths None or (0, P); a radius whose ball holds about 4 of a cloud's points, or
    the whole unit cube where there are no 4 (the pair of P = 2 are neighbours)."""
    rng = np.random.default_rng(70 + P)
    pts = np.stack([gen.cloud(rng, "uniform", P, 3) for _ in range(2)])
    lengths = np.array([0, P], np.int64) if ragged else None
    if ragged:
        pts[0] = gen.PAD
    return pts, lengths, 2.0 if P < 4 else float(np.float32(gen.radius_for(4.0, P, 3)))


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("P", [1, 2, 65])
def test_radius_family_on_two_small_clouds_with_and_without_a_grid(dev, monkeypatch, P, ragged):
    """The shapes below everything the cases above draw: one point, a pair, one lane past a wave; `lengths` absent (the
    clamp's null path) or with an empty cloud.  Each operator equals its checker under *_grid=0 and under *_grid=1,
    where P = 1 is the smallest grid there is."""
    from pytorch3d_pointops_amd import _C_iss
    from pytorch3d_pointops_amd import functions as f

    pts, lengths, radius = _two_small_clouds(P, ragged)
    rn, mp, g = float(np.float32(0.6 * radius)), 2, 0.975
    p, L = _T(pts, dev), _T(lengths, dev)
    want_cluster = cluster_ref.dbscan(pts, lengths, radius, mp)
    want_radius = filters_ref.radius(pts, lengths, radius, mp)
    for value in (0, 1):
        what = f"N = 2, P = {P}, lengths {None if lengths is None else lengths.tolist()}, *_grid={value}"
        monkeypatch.setenv("POINTOPS_DEBUG", f"cluster_grid={value},filter_grid={value},iss_grid={value}")
        r = f.cluster_dbscan(p, radius, mp, lengths=L)
        assert_cluster_equal((_np(r.labels), _np(r.num_clusters), _np(r.core_mask)), want_cluster, what)
        r = f.remove_radius_outlier(p, L, radius=radius, min_neighbors=mp, return_counts=True)
        assert_filters_equal({k: _np(getattr(r, k)) for k in RADIUS_KEYS}, want_radius, RADIUS_KEYS, what)
        out = _C_iss.iss_keypoints(p, L, radius, rn, g, g, mp, want_moments=True)
        check_iss_stages(dict(zip(ISS_KEYS, (_np(x) for x in out))), None, (pts, lengths, radius, rn, g, g, mp), what)


# ------------------------------------------------------------------------------------------------ voxel_downsample
@pytest.mark.parametrize("P", [1, 2, 65])
def test_voxel_downsample_on_two_small_clouds_without_lengths(dev, P):
    """The null `lengths` of the shared clamp, at the shapes of the test above."""
    from pytorch3d_pointops_amd import functions as f

    pts = _two_small_clouds(P, False)[0]
    scene = (pts, None, 0.3, None, None)
    r = f.voxel_downsample(_T(pts, dev), None, voxel_size=0.3)
    out = dict(num_voxels=r.num_voxels, status=r.status, inverse=r.inverse, counts=r.counts,
               first_index=r.first_index, coords=r.coords, centroids=r.points, pooled=r.features)
    check_voxel_stages({k: _np(out[k]) for k in VOXEL_KEYS}, scene, voxel_ref.downsample(*scene), f"N = 2, P = {P}")


@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_voxel_downsample(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import functions as f

    def call(c, t):
        r = f.voxel_downsample(t["points"], t["lengths"], voxel_size=c.voxel_size, features=t["features"],
                               origin=t["origin"])
        out = dict(num_voxels=r.num_voxels, status=r.status, inverse=r.inverse, counts=r.counts,
                   first_index=r.first_index, coords=r.coords, centroids=r.points, pooled=r.features)
        return {k: _np(out[k]) for k in VOXEL_KEYS}

    def check(c, got):
        scene = (c.points, c.lengths, c.voxel_size, c.features, c.origin)
        check_voxel_stages(got, scene, voxel_ref.downsample(*scene), str(c.what))

    _soak(dev, monkeypatch, gen.voxel_cases(seed),
          lambda c: dict(points=c.points, lengths=c.lengths, features=c.features, origin=c.origin), call, check,
          knobs=("voxel_long=0", "voxel_long=1"), alone=lambda c: c.lengths,
          shared=lambda c: ("origin",) if c.origin is not None and c.origin.ndim == 1 else ())


# ------------------------------------------------------------------------------------------------ statistics, compaction
@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_statistical_outlier_boundary(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import _C_filters

    def call(c, t):
        mask, index, num_kept, md, thr, stats = _C_filters.statistical_outlier(t["dists"], t["lengths"], c.std_ratio)
        return dict(zip(STAT_KEYS, (_np(x) for x in (mask, index, num_kept, md, thr, stats))))

    def check(c, got):
        assert_filters_equal(got, filters_ref.statistical_from_dists(c.dists, c.lengths, c.std_ratio), STAT_KEYS, str(c.what))

    _soak(dev, monkeypatch, gen.statistical_cases(seed), lambda c: dict(dists=c.dists, lengths=c.lengths), call, check,
          alone=lambda c: c.lengths)


@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_mask_to_index(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import functions as f

    def call(c, t):
        index, num_kept = f.mask_to_index(t["mask"])
        return dict(index=_np(index), num_kept=_np(num_kept))

    def check(c, got):
        index, num_kept = filters_ref.compact(c.mask)
        assert_filters_equal(got, dict(index=index, num_kept=num_kept), ("index", "num_kept"), str(c.what))

    _soak(dev, monkeypatch, gen.compact_cases(seed), lambda c: dict(mask=c.mask), call, check,
          alone=lambda c: np.ones(len(c.mask), np.int64))


# ------------------------------------------------------------------------------------------------ the consensus operators
@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_segment_plane(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import _C_plane

    def call(c, t):
        kw = c.kw
        out = _C_plane.segment_plane(t["points"], t["lengths"], t["mask"], t.get("samples"), kw["H"], kw["seed"],
                                     float(np.float32(kw["thr"])), None, None, kw["refine_steps"], want_hypotheses=True)
        return dict(zip(PLANE_KEYS, (_np(x) for x in out)))

    def check(c, got):
        check_plane_stages(got, c.X, c.lengths, c.mask, c.kw, chain=False)

    cases = [c for c in gen.consensus_cases(seed) if c.op == "plane"]
    # (the strided caller also hands the drawn triples back, as a view: they are read, not drawn again)
    _soak(dev, monkeypatch, cases, lambda c: dict(points=c.X, lengths=c.lengths, mask=c.mask), call, check,
          knobs=("plane_lds=0", "plane_lds=1", "plane_hpl=1", "plane_hpl=2", "plane_lds=0,plane_hpl=2"),
          handed_back=("samples",))


@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_ransac_alignment(dev, monkeypatch, seed):
    from pytorch3d_pointops_amd import _C_ransac

    def call(c, t):
        kw = c.kw
        out = _C_ransac.ransac_alignment(t["X"], t["Y"], t["corr"], t["len1"], t["len2"], t.get("samples"), kw["H"],
                                         kw["seed"], kw["thr"], kw["ratio"], kw["estimate_scale"], kw["refine_steps"],
                                         want_hypotheses=True)
        return dict(zip(RANSAC_KEYS, (_np(x) for x in out)))

    def check(c, got):
        check_ransac_stages(got, c.X, c.Y, c.corr, c.len1, c.len2, c.kw, chain=False)

    cases = [c for c in gen.consensus_cases(seed) if c.op == "ransac"]
    _soak(dev, monkeypatch, cases, lambda c: dict(X=c.X, Y=c.Y, corr=c.corr, len1=c.len1, len2=c.len2), call, check,
          knobs=("ransac_lds=1",), handed_back=("samples",))


# ------------------------------------------------------------------------------------------------ registration
@pytest.mark.parametrize("seed", gen.SEEDS)
def test_fuzz_registration_evaluate_step(dev, monkeypatch, seed):
    """One step(update=False) of RegistrationState: the search equals knn_points(K=1) and registration_ref.nearest;
    correspondences, their number and the fitness equal registration_ref.evaluate bit for bit, in both search families
    (the fp64 sums, the solve and convergence stay with test_registration_gpu.py)."""
    from pytorch3d_pointops_amd import _C_registration
    from pytorch3d_pointops_amd.functions import knn_points

    names = ("Xt", "idx", "dists", "correspondences", "num_correspondences", "status", "iterations")

    def call(c, t):
        st = _C_registration.RegistrationState(t["X"], t["Y"], t["normals"], t["len_x"], t["len_y"], None, None, c.r_max,
                                               c.estimation, 1, 1e-6, 1e-6)
        st.step(update=False)
        out = {k: _np(getattr(st, k)) for k in names}
        out.update(fitness=_np(st.fitness[0]), inlier_rmse=_np(st.inlier_rmse[0]), R=_np(st.R[0]), T=_np(st.T[0]))
        return out

    def check(c, got):
        what = str(c.what)
        knn = knn_points(_T(got["Xt"], dev), _T(c.Y, dev), _T(c.len_x, dev), _T(c.len_y, dev), K=1)
        assert np.array_equal(got["idx"], _np(knn.idx)[..., 0]), f"{what}: idx differs from knn_points"
        assert got["dists"].tobytes() == _np(knn.dists)[..., 0].tobytes(), f"{what}: d2 differs from knn_points"
        eye, zero = np.eye(3), np.zeros(3)
        for n, (a, b) in enumerate(zip(c.len_x, c.len_y)):
            tag = f"{what}, cloud {n}"
            Xt = registration_ref.apply(c.X[n], eye, zero, a)
            assert got["Xt"][n].tobytes() == Xt.tobytes(), tag
            idx, d2 = registration_ref.nearest(Xt, c.Y[n], a, b)
            assert np.array_equal(got["idx"][n], idx) and got["dists"][n].tobytes() == d2.tobytes(), tag
            mask, cnt, fit, _, _ = registration_ref.evaluate(got["dists"][n], a, b, c.r_max)
            assert np.array_equal(got["correspondences"][n], np.where(mask, idx, -1)), tag
            assert got["num_correspondences"][n] == cnt, tag
            assert np.float32(got["fitness"][n]).tobytes() == np.float32(fit).tobytes(), tag
            assert got["iterations"][n] == 0, tag

    _soak(dev, monkeypatch, gen.registration_cases(seed),
          lambda c: dict(X=c.X, Y=c.Y, normals=c.normals, len_x=c.len_x, len_y=c.len_y), call, check,
          knobs=("registration_grid=1",), alone=lambda c: c.len_x)
