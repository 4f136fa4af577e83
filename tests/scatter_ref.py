"""Float64 references of the two scatter-add backward passes, the exact-input generators and the error bound the GPU
tests of tests/test_scatter_backward_gpu.py use.  Plain numpy; no project code.

The rules are the reference's CPU rules (csrc/knn/knn_cpu.cpp:75-128, functions/knn.py:236-248, functions/utils.py:53-63):
rows i >= l1[n] give nothing, entries k >= min(l2[n], K) give nothing, idx < 0 gives nothing; the L2 addend is
2 g (a - b), the L1 addend g * (a > b ? 1 : -1) (so the tie a == b gives -1); grad_p2 receives the negated addend.

Besides the sums every function returns, per element, the count of addends n and A = sum |addend|: what the bound needs.

EXACT INPUTS.  Coordinates integers(0..4) * 0.25, gradients integers in [-4, 4]: every addend is a multiple of 0.5 (L2:
2 g (a - b) with a - b a multiple of 0.25) or of 1 (L1, gather), at most 8 in magnitude and computed without rounding.
While max A < 2^22 every partial sum of any subset in any order is a multiple of 0.5 below 2^22 in magnitude, i.e. an
integer count of halves below 2^23 < 2^24: an exact fp32 number.  No addition rounds, so every plan -- device atomics, LDS
tiles, any row split, the sequential deterministic form -- must give the SAME bits: the float64 sum cast to fp32.  The
generators assert the condition and raise when a case breaks it: it is a precondition, not a measurement.

BOUND for arbitrary fp32 inputs, per element: |fp32 result - float64 sum| <= (n + S + 4) * 2^-24 * A.  With u = 2^-24,
an addend carries at most two roundings (a - b, then the product with 2 g: 2 g itself is exact), a relative error of at
most 2u + u^2; a sum of n terms in ANY order adds at most (n - 1) u times the sum of magnitudes (Higham, Accuracy and
Stability, eq. 4.4 to first order), and the S partial tiles of a row split meet in at most S further additions:
(2 + n - 1 + S) u A = (n + S + 1) u A to first order; the three extra units cover the second-order terms
(n u << 1 for every n here) and the difference between A over exact and over rounded addends.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 22

KnnBackwardRef = namedtuple("KnnBackwardRef", "g1 n1 A1 g2 n2 A2")
GatherBackwardRef = namedtuple("GatherBackwardRef", "gx n A")


def _entry_mask(idx, l1, l2):
    """(N, L, K) bool: the entries that contribute."""
    N, L, K = idx.shape
    ok = idx >= 0
    if l1 is not None:
        ok &= (np.arange(L)[None, :] < np.asarray(l1)[:, None])[:, :, None]
    if l2 is not None:
        ok &= (np.arange(K)[None, :] < np.minimum(np.asarray(l2), K)[:, None])[:, None, :]
    return ok


def _scatter(rows, add, nrows, shape):
    """float64 sums, sums of magnitudes and counts of the addends `add` (entries x C) per target row."""
    C = add.shape[1]
    g, A = np.zeros((nrows, C), np.float64), np.zeros((nrows, C), np.float64)
    for c in range(C):
        g[:, c] = np.bincount(rows, weights=add[:, c], minlength=nrows)
        A[:, c] = np.bincount(rows, weights=np.abs(add[:, c]), minlength=nrows)
    n = np.repeat(np.bincount(rows, minlength=nrows)[:, None], C, axis=1)
    return g.reshape(shape), A.reshape(shape), n.reshape(shape).astype(np.int64)


def knn_backward_ref(p1, p2, l1, l2, idx, norm, grad):
    p1, p2, grad = (np.asarray(a, np.float64) for a in (p1, p2, grad))
    idx = np.asarray(idx, np.int64)
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    ok = _entry_mask(idx, l1, l2)
    n_, i_, k_ = np.nonzero(ok)  # C order = (n, i, k) = the CPU loop's order
    j_ = idx[n_, i_, k_]
    a, b, g = p1[n_, i_], p2[n_, j_], grad[n_, i_, k_][:, None]
    if norm == 2:
        add = 2.0 * g * (a - b)
    elif norm == 1:
        add = g * np.where(a > b, 1.0, -1.0)
    else:
        raise ValueError("norm must be 1 or 2")
    q1, q2 = (n_ * P1 + i_), (n_ * P2 + j_)
    g1, A1, n1 = _scatter(q1, add, N * P1, (N, P1, D))
    g2, A2, n2 = _scatter(q2, -add, N * P2, (N, P2, D))
    return KnnBackwardRef(g1, n1, A1, g2, n2, A2)


def gather_backward_ref(grad_out, idx, lengths, M):
    grad_out = np.asarray(grad_out, np.float64)
    idx = np.asarray(idx, np.int64)
    N, L, K, C = grad_out.shape
    n_, l_, k_ = np.nonzero(_entry_mask(idx, None, lengths))
    j_ = idx[n_, l_, k_]
    add = grad_out[n_, l_, k_]
    gx, A, n = _scatter(n_ * M + j_, add, N * M, (N, M, C))
    return GatherBackwardRef(gx, n, A)


def gather_backward_sequential_f32(grad_out, idx, lengths, M):
    """fp32 sums in table order: ufunc.at is unbuffered and sequential, so every target row receives its addends one
    after the other in (l, k) order starting from +0 -- the order the deterministic kernel claims."""
    grad_out = np.asarray(grad_out, np.float32)
    idx = np.asarray(idx, np.int64)
    N, L, K, C = grad_out.shape
    n_, l_, k_ = np.nonzero(_entry_mask(idx, None, lengths))
    gx = np.zeros((N, M, C), np.float32)
    np.add.at(gx, (n_, idx[n_, l_, k_]), grad_out[n_, l_, k_])
    return gx


def knn_backward_p2_sequential_f32(p1, p2, l1, l2, idx, norm, grad):
    """grad_p2 of an EXACT case as fp32 np.add.at (no addend rounds, so fp32 arithmetic on the addends is exact too)."""
    p1, p2, grad = (np.asarray(a, np.float32) for a in (p1, p2, grad))
    idx = np.asarray(idx, np.int64)
    n_, i_, k_ = np.nonzero(_entry_mask(idx, l1, l2))
    j_ = idx[n_, i_, k_]
    a, b, g = p1[n_, i_], p2[n_, j_], grad[n_, i_, k_][:, None]
    add = np.float32(2.0) * g * (a - b) if norm == 2 else g * np.where(a > b, np.float32(1.0), np.float32(-1.0))
    g2 = np.zeros(p2.shape, np.float32)
    np.add.at(g2, (n_, j_), -add.astype(np.float32))
    return g2


def knn_backward_p1_sequential_f32(p1, p2, l1, l2, idx, norm, grad):
    """grad_p1 as the CPU loop computes it: fp32 addends (2 g first, then the difference's product) added in k order
    from +0.  For float inputs the cast float64 sum is NOT this number (the fp32 addend rounds twice, the float64 one
    not at all), so bit equality of grad_p1 is stated against this form and the float64 sum is held to `bound`."""
    p1, p2, grad = (np.asarray(a, np.float32) for a in (p1, p2, grad))
    idx = np.asarray(idx, np.int64)
    N, P1, D = p1.shape
    ok = _entry_mask(idx, l1, l2)
    acc = np.zeros((N, P1, D), np.float32)
    rows = np.arange(N)[:, None]
    for k in range(idx.shape[2]):
        b = p2[rows, np.where(ok[:, :, k], idx[:, :, k], 0)]
        g = grad[:, :, k][:, :, None]
        if norm == 2:
            add = (np.float32(2.0) * g) * (p1 - b)
        else:
            add = g * np.where(p1 > b, np.float32(1.0), np.float32(-1.0))
        acc = np.where(ok[:, :, k][:, :, None], acc + add.astype(np.float32), acc)
    return acc


def bound(n, A, S=1):
    return (np.asarray(n, np.float64) + S + 4.0) * U * np.asarray(A, np.float64)


def within_bound(got, want, n, A, S=1):
    """(ok, worst ratio |got - want| / bound over the elements with a non-zero bound, count of violations)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    b = bound(n, A, S)
    bad = err > b
    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    return not bad.any(), ratio, int(bad.sum())


# ---------------------------------------------------------------- tables and exact inputs
TILE_ROWS = {1: 24576, 2: 12288, 3: 8192, 4: 6144}  # tiled_tile_rows(C) of csrc/tiled_scatter.h


def tile_rows(C):
    return TILE_ROWS[C]


def target_sizes(C):
    t = tile_rows(C)
    return {"1": 1, "63": 63, "64": 64, "65": 65, "tile-1": t - 1, "tile": t, "tile+1": t + 1, "2tile+1": 2 * t + 1}


def empty_split(L):
    """Smallest S above 5 for which a FULL cloud of L rows leaves its last split without rows
    (rows_per = ceil(L / S); split S - 1 starts at (S - 1) * rows_per >= L)."""
    S = 6
    while (S - 1) * (-(-L // S)) < L:
        S += 1
    return S


def table(seed, N, L, K, M, tile):
    """A synthetic neighbour table (N, L, K) with indices in [-1, M): uniform targets; a HUB block (the first L // 4 rows
    of every cloud all point at one row); an EDGE block (the next L // 4 rows alternate between the last row of the first
    tile and the first row of the next, where M has them); ball-query padding (every third row keeps a random prefix and
    is -1 after it)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, M, (N, L, K), dtype=np.int64)
    h = L // 4
    idx[:, :h, :] = (M // 3 + np.arange(N)[:, None, None]) % M
    edge = np.array([min(tile - 1, M - 1), min(tile, M - 1)], np.int64)
    idx[:, h:2 * h, :] = edge[(np.arange(h)[:, None] + np.arange(K)[None, :]) % 2][None]
    keep = rng.integers(0, K + 1, (N, L))
    pad = (np.arange(K)[None, None, :] >= keep[:, :, None]) & (np.arange(L) % 3 == 1)[None, :, None]
    idx[pad] = -1
    return idx


def ragged_lengths(N, L, K, M):
    """l1: ragged, an empty cloud, a cloud of three rows (smaller than every split count used), a FULL cloud last.
    l2: below K on cloud 0, the whole target elsewhere."""
    l1 = np.array(([L - 37, 0, 3] * N)[:N - 1] + [L], np.int64)
    l2 = np.array([K - 1] + [max(M, K)] * (N - 1), np.int64)
    return l1, l2


def _assert_exact(A, what):
    worst = float(A.max()) if A.size else 0.0
    if not worst < EXACT_LIMIT:
        raise AssertionError(f"{what}: max A = {worst} is not below 2^22: the case is not order-free in fp32")


def exact_knn_inputs(seed, N, L, K, M, D, norm, tile=None):
    """(p1, p2, l1, l2, idx, grad, ref) on the exact lattice; raises unless max A < 2^22."""
    rng = np.random.default_rng(seed + 1)
    p1 = (rng.integers(0, 5, (N, L, D)) * 0.25).astype(np.float32)
    p2 = (rng.integers(0, 5, (N, M, D)) * 0.25).astype(np.float32)
    grad = rng.integers(-4, 5, (N, L, K)).astype(np.float32)
    idx = table(seed, N, L, K, M, tile if tile is not None else tile_rows(min(D, 4)))
    l1, l2 = ragged_lengths(N, L, K, M)
    ref = knn_backward_ref(p1, p2, l1, l2, idx, norm, grad)
    _assert_exact(ref.A1, "exact_knn_inputs(grad_p1)")
    _assert_exact(ref.A2, "exact_knn_inputs(grad_p2)")
    return p1, p2, l1, l2, idx, grad, ref


def exact_gather_inputs(seed, N, L, K, M, C, with_lengths=True, tile=None):
    """(grad_out, idx, lengths, ref) with integer gradients; raises unless max A < 2^22."""
    rng = np.random.default_rng(seed + 2)
    grad_out = rng.integers(-4, 5, (N, L, K, C)).astype(np.float32)
    idx = table(seed, N, L, K, M, tile if tile is not None else tile_rows(min(C, 4)))
    lengths = ragged_lengths(N, L, K, M)[1] if with_lengths else None
    ref = gather_backward_ref(grad_out, idx, lengths, M)
    _assert_exact(ref.A, "exact_gather_inputs")
    return grad_out, idx, lengths, ref


# ---------------------------------------------------------------- the case lists of the GPU matrix
N_CLOUDS, L_ROWS = 4, 1500
K_LIST = (1, 3, 8, 21)


def matrix_cases():
    """(C, M name, K, norm) of the exact matrix: every M with every C at K = 8, every K and norm at tile + 1."""
    out = []
    for C in (1, 2, 3, 4):
        for name in target_sizes(C):
            out.append((C, name, 8, 2))
        for K in K_LIST:
            for norm in (1, 2):
                if (K, norm) != (8, 2):
                    out.append((C, "tile+1", K, norm))
    return out


def wide_cases(op):
    """(C, M, K, norm) beyond four channels (device atomics and the deterministic form only): D in {5, 7} for knn,
    U in {5, 64} for gather."""
    return [(C, M, K, norm) for C in ((5, 7) if op == "knn" else (5, 64))
            for M, K, norm in ((65, 8, 2), (6145, 3, 1), (6145, 21, 2), (6145, 1, 2))]


def case_seed(C, M, K, norm):
    return 7000 + 1000 * C + 37 * K + norm + M % 997
