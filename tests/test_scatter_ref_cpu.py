"""tests/scatter_ref.py against the oracle and the reference's goldens, and the exactness condition of every case of the
GPU matrix (tests/test_scatter_backward_gpu.py).  This checks the checker; no GPU."""
import numpy as np
import pytest

import cases
import scatter_ref as R
from conftest import bits, load_golden
from pytorch3d_pointops_amd import synth


@pytest.mark.parametrize("name", sorted(cases.knn_backward_cases()))
def test_reference_reproduces_knn_backward_goldens(oracle, name):
    """Float inputs.  grad_p1: the reference's fp32 k-ordered sum is the oracle's (= the golden's) bit for bit.  (The
    cast FLOAT64 sum is not: an fp32 addend 2 g (a - b) rounds twice, the float64 one not at all -- measured worst
    |fp32 - float64| / bound(n, A) over these goldens 0.08 .. 0.22 for grad_p1, 0.05 .. 0.20 for grad_p2 -- so the
    float64 sums are held to bound(n, A), element by element, for both gradients; on exact inputs, next test, the
    cast is the answer.)"""
    g = load_golden("knn_backward")
    c = cases.knn_backward_cases()[name]
    idx, dists = oracle.knn_points_idx(c["p1"], c["p2"], c["l1"], c["l2"], c["norm"], c["K"])
    grad = cases.grad_for(name, dists.shape)
    o1, o2 = oracle.knn_points_backward(c["p1"], c["p2"], c["l1"], c["l2"], idx, c["norm"], grad)
    assert np.array_equal(bits(o1), bits(g[name + "/grad_p1"])) and np.array_equal(bits(o2), bits(g[name + "/grad_p2"]))
    s1 = R.knn_backward_p1_sequential_f32(c["p1"], c["p2"], c["l1"], c["l2"], idx, c["norm"], grad)
    assert np.array_equal(bits(s1), bits(o1)), name
    r = R.knn_backward_ref(c["p1"], c["p2"], c["l1"], c["l2"], idx, c["norm"], grad)
    ok1, ratio1, bad1 = R.within_bound(o1, r.g1, r.n1, r.A1)
    ok2, ratio2, bad2 = R.within_bound(o2, r.g2, r.n2, r.A2)
    print(f"{name}: grad_p1 worst err/bound {ratio1:.3f}, grad_p2 worst err/bound {ratio2:.3f}")
    assert ok1, (name, ratio1, bad1)
    assert ok2, (name, ratio2, bad2)
    # nothing is added where the reference adds nothing
    assert not o1[r.n1 == 0].any() and not o2[r.n2 == 0].any()
    if c["norm"] == 1:  # addends are +-g: one addend per element is the element, exactly
        one = r.n1 == 1
        assert np.array_equal(bits(o1[one]), bits(r.g1[one].astype(np.float32)))


def test_reference_reproduces_knn_backward_exactly_on_exact_inputs(oracle):
    """On the exact lattice nothing rounds: the oracle's fp32 loop and the cast float64 sums agree bit for bit, grad_p1
    and grad_p2, both norms."""
    for norm in (1, 2):
        p1, p2, l1, l2, idx, grad, r = R.exact_knn_inputs(41 + norm, 3, 300, 5, 65, 3, norm)
        o1, o2 = oracle.knn_points_backward(p1, p2, l1, l2, idx, norm, grad)
        assert np.array_equal(bits(o1), bits(r.g1.astype(np.float32)))
        assert np.array_equal(bits(o2), bits(r.g2.astype(np.float32)))


def test_reference_reproduces_gather_goldens():
    """knn_gather (k >= lengths masked) and masked_gather (-1 masked) gradient goldens: grad_out is the upstream
    tensor of the fixture (tests/test_gpu_parity.py::test_knn_gather_and_masked_gather)."""
    g = load_golden("gather")
    idx = synth.randint(602, 0, 49, (2, 30, 4))
    lengths = np.array([50, 2])
    up = cases.grad_for("kg", (2, 30, 4, 5))
    r = R.gather_backward_ref(up, idx, lengths, 50)
    ok, ratio, bad = R.within_bound(g["knn_gather/grad_x"], r.gx, r.n, r.A)
    assert ok, (ratio, bad)
    assert np.array_equal(bits(R.gather_backward_sequential_f32(up, idx, lengths, 50)), bits(g["knn_gather/grad_x"]))
    midx = idx.copy()
    midx[0, ::3, 1] = -1
    midx[1, :, 3] = -1
    r = R.gather_backward_ref(up, midx, None, 50)
    ok, ratio, bad = R.within_bound(g["masked_gather3/grad_x"], r.gx, r.n, r.A)
    assert ok, (ratio, bad)
    assert not g["masked_gather3/grad_x"][r.n == 0].any()


def test_mask_rules():
    """Each rule on a table small enough to read: i >= l1, k >= min(l2, K), idx < 0, the L1 tie, the negated grad_p2."""
    p1 = np.array([[[0.5], [0.25], [1.0]]], np.float32)
    p2 = np.array([[[0.5], [0.75]]], np.float32)
    idx = np.array([[[0, 1], [1, -1], [0, 1]]])
    grad = np.array([[[1.0, 2.0], [3.0, 5.0], [7.0, 11.0]]], np.float32)
    r = R.knn_backward_ref(p1, p2, np.array([2]), np.array([5]), idx, 1, grad)
    # row 0: tie with target 0 -> -1; below target 1 -> -2.  row 1: below target 1 -> -3; -1 skipped.  row 2: i >= l1.
    assert r.g1[0, :, 0].tolist() == [-3.0, -3.0, 0.0] and r.n1[0, :, 0].tolist() == [2, 1, 0]
    assert r.g2[0, :, 0].tolist() == [1.0, 5.0] and r.n2[0, :, 0].tolist() == [1, 2] and r.A2[0, :, 0].tolist() == [1.0, 5.0]
    r = R.knn_backward_ref(p1, p2, np.array([3]), np.array([1]), idx, 2, grad)  # k >= l2 = 1 gives nothing
    assert r.g1[0, :, 0].tolist() == [0.0, 2 * 3 * -0.5, 2 * 7 * 0.5] and r.g2[0, :, 0].tolist() == [-7.0, 3.0]
    go = np.arange(1.0, 13.0, dtype=np.float32).reshape(1, 3, 2, 2)
    r = R.gather_backward_ref(go, idx, np.array([1]), 2)
    assert r.gx[0].tolist() == [[1.0 + 9.0, 2.0 + 10.0], [5.0, 6.0]] and r.n[0, :, 0].tolist() == [2, 1]
    r = R.gather_backward_ref(go, idx, None, 2)
    assert r.n[0, :, 0].tolist() == [2, 3]
    assert float(R.bound(3, 2.0, S=5)) == 12 * 2.0 ** -24 * 2.0


def test_generated_tables_have_the_edges():
    """What the GPU cases rely on: indices inside [-1, M), an empty cloud, a three-row cloud, a full cloud last, l2 < K
    on a cloud, -1 padding, a hub row with hundreds of addends, both sides of the first tile boundary, and a split
    count that leaves the last split of the FULL cloud without rows."""
    L, K = R.L_ROWS, 8
    for C in (1, 2, 3, 4):
        t = R.tile_rows(C)
        for name, M in R.target_sizes(C).items():
            idx = R.table(5, R.N_CLOUDS, L, K, M, t)
            assert idx.min() == -1 and idx.max() < M
            l1, l2 = R.ragged_lengths(R.N_CLOUDS, L, K, M)
            assert l1.tolist() == [L - 37, 0, 3, L] and l2[0] < K and (l2[1:] >= M).all()
            r = R.gather_backward_ref(np.ones((R.N_CLOUDS, L, K, 1), np.float32), idx, None, M)
            assert r.n.max() >= (L // 4) * K // 2  # a hub (padding may take some of its entries)
            if M > t:
                assert r.n[-1, t - 1, 0] > 100 and r.n[-1, t, 0] > 100
    S = R.empty_split(L)
    rows_per = -(-L // S)
    assert S > 5 and (S - 1) * rows_per >= L and S > 3  # the full cloud's and the three-row cloud's splits run dry


@pytest.mark.parametrize("C,name,K,norm", R.matrix_cases())
def test_exact_condition_of_the_matrix(C, name, K, norm):
    """Every case of the exact matrix meets max A < 2^22 (the generators raise otherwise), values sit on the lattice,
    zero gradients occur, and the fp32 np.add.at of the case equals the cast float64 sums bit for bit."""
    M = R.target_sizes(C)[name]
    seed = R.case_seed(C, M, K, norm)
    p1, p2, l1, l2, idx, grad, r = R.exact_knn_inputs(seed, R.N_CLOUDS, R.L_ROWS, K, M, C, norm)
    assert max(r.A1.max(), r.A2.max()) < R.EXACT_LIMIT
    assert np.array_equal(p1 * 4, np.round(p1 * 4)) and p1.min() >= 0 and p1.max() <= 1
    assert np.array_equal(grad, np.round(grad)) and np.abs(grad).max() <= 4 and (grad == 0).any()
    assert np.array_equal(bits(R.knn_backward_p2_sequential_f32(p1, p2, l1, l2, idx, norm, grad)),
                          bits(r.g2.astype(np.float32)))
    if norm == 2:  # (the gather side has no norm: once per (C, M, K))
        go, gidx, lengths, gr = R.exact_gather_inputs(seed, R.N_CLOUDS, R.L_ROWS, K, M, C)
        assert gr.A.max() < R.EXACT_LIMIT and (go == 0).any()
        assert np.array_equal(bits(R.gather_backward_sequential_f32(go, gidx, lengths, M)), bits(gr.gx.astype(np.float32)))


@pytest.mark.parametrize("op", ["knn", "gather"])
def test_exact_condition_of_the_wide_cases(op):
    for C, M, K, norm in R.wide_cases(op):
        seed = R.case_seed(C, M, K, norm)
        if op == "knn":
            p1, p2, l1, l2, idx, grad, r = R.exact_knn_inputs(seed, R.N_CLOUDS, R.L_ROWS, K, M, C, norm)
            assert max(r.A1.max(), r.A2.max()) < R.EXACT_LIMIT
            assert np.array_equal(bits(R.knn_backward_p2_sequential_f32(p1, p2, l1, l2, idx, norm, grad)),
                                  bits(r.g2.astype(np.float32)))
        else:
            go, gidx, lengths, gr = R.exact_gather_inputs(seed, R.N_CLOUDS, R.L_ROWS, K, M, C)
            assert gr.A.max() < R.EXACT_LIMIT
            assert np.array_equal(bits(R.gather_backward_sequential_f32(go, gidx, lengths, M)),
                                  bits(gr.gx.astype(np.float32)))


def test_exact_generator_raises_when_the_condition_breaks():
    with pytest.raises(AssertionError, match="not below 2\\^22"):
        R._assert_exact(np.array([2.0 ** 22]), "case")
    R._assert_exact(np.array([2.0 ** 22 - 0.5]), "case")
