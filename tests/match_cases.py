"""Inputs of the match_features tests (tests/test_match_cpu.py, tests/test_match_gpu.py), each with what it exists to
show.  Built once per process; nothing here reads the library.

The screen of csrc/feature_match.hip works in 32 x 32 blocks (one wave: 32 queries) and LDS tiles of 64 targets, its
lists hold M = 8 keys per lane, its template instances take D <= 4, 16, 32, 34, 64 and 128, and D > 128 never reaches it:
the sizes below sit on both sides of each.  Its workgroups hold 32 queries (64 lanes) while the batch has fewer than
1024 groups of 128 queries and 128 queries (256 lanes: four waves, another stepping of the tile loader) from there on:
the "wide-groups" cases are the smallest batches on the far side -- 64 clouds of 1999 queries -- every other case is
on the near side."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "f1 f2 lengths1 lengths2 finite same shows")

POINTS = (1, 31, 32, 33, 63, 65, 257, 1000, 1037, 64, 127, 128, 129)
DIMS = (1, 2, 3, 32, 33, 64, 127, 128, 129, 4, 5, 16, 17, 34, 35)


def _lengths(rng, N, P, ragged):
    l = np.full(N, P, np.int64)
    if ragged and N > 1:
        l[1:] = rng.integers(0, P + 1, N - 1)
    return l


def fpfh_like(rng, shape):
    """Rows of three 11-bin histograms that sum to 100 each: what fpfh_features returns."""
    rows = rng.dirichlet(np.full(11, 0.5), size=shape + (3,)) * 100.0
    return rows.reshape(shape + (33,)).astype(np.float32)


def unit_rows(rng, shape, D=32):
    v = rng.standard_normal(shape + (D,))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def quantised(rng, shape):
    """Multiples of 2^-8 in [-4, 4): every product of two is exact in float32."""
    return (rng.integers(-1024, 1024, shape) / 256.0).astype(np.float32)


def build_cases():
    rng = np.random.default_rng(20250611)
    cases = {}
    # every P on either side and every D once; lengths ragged in the second cloud
    for i, D in enumerate(DIMS):
        P1, P2 = POINTS[i % len(POINTS)], POINTS[(i + 5) % len(POINTS)]
        f1, f2 = rng.standard_normal((2, P1, D)).astype(np.float32), rng.standard_normal((2, P2, D)).astype(np.float32)
        cases[f"normal-{P1}x{P2}-D{D}"] = Case(f1, f2, _lengths(rng, 2, P1, True), _lengths(rng, 2, P2, True), True, False,
                                               "tile, block and instance edges")
    for i, P1 in enumerate(POINTS):  # the other pairing, on small integers (ties cut by index all over)
        P2, D = POINTS[(i + 9) % len(POINTS)], DIMS[(2 * i + 3) % len(DIMS)]
        f1 = rng.integers(0, 3, (2, P1, D)).astype(np.float32)
        f2 = rng.integers(0, 3, (2, P2, D)).astype(np.float32)
        cases[f"ties-{P1}x{P2}-D{D}"] = Case(f1, f2, _lengths(rng, 2, P1, True), _lengths(rng, 2, P2, False), True, False,
                                             "equal distances cut by index, across blocks and tiles")
    # 0, 1, K - 1, M and M + 1 targets, zero queries
    f1, f2 = fpfh_like(rng, (8, 40)), fpfh_like(rng, (8, 70))
    cases["ragged"] = Case(f1, f2, np.array([40, 0, 1, 40, 33, 40, 40, 40]), np.array([0, 1, 2, 8, 9, 70, 64, 65]), True,
                           False, "lengths2 in {0, 1, 2, M, M + 1, tile, tile + 1}, a cloud without queries")
    cases["N0"] = Case(np.zeros((0, 5, 33), np.float32), np.zeros((0, 7, 33), np.float32), np.zeros(0, np.int64),
                       np.zeros(0, np.int64), True, False, "an empty batch")
    cases["N1"] = Case(fpfh_like(rng, (1, 300)), fpfh_like(rng, (1, 257)), np.array([300]), np.array([257]), True, False,
                       "one cloud")
    f = fpfh_like(rng, (2, 300))
    cases["self"] = Case(f, f, np.array([300, 211]), np.array([300, 211]), True, True, "f1 is f2: every row finds itself")
    # rows of NaN and of +-inf on either side
    f1, f2 = fpfh_like(rng, (3, 90)), fpfh_like(rng, (3, 130))
    f1[0, 3] = np.nan
    f1[0, 70, 5] = np.inf
    f2[1, 17] = np.nan
    f2[1, 100, 0] = -np.inf
    f2[2, 64] = np.inf
    f1[2, 0] = -np.inf
    cases["nan-and-inf-rows"] = Case(f1, f2, np.array([90, 90, 80]), np.array([130, 120, 130]), False, False,
                                     "rows that are not finite take the exact kernel, with its semantics")
    # one case shifted and rescaled
    f1, f2 = fpfh_like(rng, (2, 257)), fpfh_like(rng, (2, 300))
    l1, l2 = np.array([257, 100]), np.array([300, 299])
    for tag, fn in (("x1", lambda a: a), ("x2^10", lambda a: a * np.float32(1024)), ("x2^-10", lambda a: a / np.float32(1024)),
                    ("+1000", lambda a: a + np.float32(1000))):
        cases[f"frames-{tag}"] = Case(fn(f1), fn(f2), l1, l2, True, False, "the same descriptors in another frame")
    # huge but finite: the norms pass 2^126, nothing may be certified, nothing may differ
    # (unit rows times 2^63: n1 + n2max = 2^127, every distance stays finite -- at most 4 * 2^126 only for opposite rows)
    cases["huge"] = Case(unit_rows(rng, (2, 100)) * np.float32(2.0 ** 63), unit_rows(rng, (2, 150)) * np.float32(2.0 ** 63),
                         np.array([100, 57]), np.array([150, 150]), True, False, "norms above 2^126: no row is certified")
    # 64 x ceil(1999 / 128) = 1024 workgroups: 256 lanes each, queries in every wave, a last workgroup that is part
    # full (1999 = 15 x 128 + 79), three target tiles with a ragged last one
    for D in (33, 128):
        f1 = fpfh_like(rng, (64, 1999)) if D == 33 else unit_rows(rng, (64, 1999), D)
        f2 = fpfh_like(rng, (64, 150)) if D == 33 else unit_rows(rng, (64, 150), D)
        l1, l2 = _lengths(rng, 64, 1999, True), _lengths(rng, 64, 150, True)
        l2[1:4] = (129, 64, 65)
        cases[f"wide-groups-D{D}"] = Case(f1, f2, l1, l2, True, False, "256-lane workgroups: wave > 0, loader steps of 256")
    return cases


def integer_no_fallback():
    rng = np.random.default_rng(33)
    return (rng.integers(0, 16, (1, 1000, 33)).astype(np.float32), rng.integers(0, 16, (1, 1037, 33)).astype(np.float32))


def integer_ties():
    f = np.random.default_rng(5).integers(0, 4, (1, 1000, 5)).astype(np.float32)
    return f, f.copy()


def all_duplicates():
    row = fpfh_like(np.random.default_rng(8), (1, 1))
    return np.repeat(row, 100, axis=1), np.repeat(row, 150, axis=1)


def ratio_boundary():
    """One query at the origin, targets at squared distances 1, 4 and 9: ratio = 0.5 gives fl(0.25) * 4 = 1 = d1, the
    strict comparison fails; the next float32 above 0.5 passes.  A second cloud has one target: no second, passes."""
    f1 = np.zeros((2, 2, 2), np.float32)
    f2 = np.array([[[0, 2], [1, 0], [3, 0]], [[0, 5], [7, 7], [9, 9]]], np.float32)
    return f1, f2, np.array([1, 2]), np.array([3, 1])


def replaced_scene(P=1200, replaced=0.3, noise=1.0, seed=21):
    """f2 describes a permuted copy of the points of f1 with noisy descriptors, the first `replaced` share of its rows
    replaced by descriptors of something else.  truth[i] = the row of f2 that describes point i, or -1 if replaced."""
    rng = np.random.default_rng(seed)
    f1 = fpfh_like(rng, (1, P))
    perm = rng.permutation(P)
    f2 = np.abs(f1[:, perm] + rng.normal(0, noise, (1, P, 33)).astype(np.float32))
    cut = int(P * replaced)
    f2[:, :cut] = fpfh_like(rng, (1, cut))
    truth = np.full(P, -1, np.int64)
    truth[perm[cut:]] = np.arange(cut, P)
    return f1, f2, truth
