"""Sample arguments and documented outputs of every registered operator (pytorch3d_pointops_amd/ops.py), shared by
test_registered_ops_cpu.py (fake tensors, no device) and test_registered_ops_gpu.py.

`TABLE[name]` is an `Op`: `samples(to)` builds the argument tuples -- numpy arrays from `cases.cloud` / `synth`, placed
by `to` (the GPU tests copy them to the device, the CPU tests make fake CUDA tensors of the same shape and dtype) --,
`outputs(*args)` is what the comment of the matching entry of include/pointops_amd.h documents for those arguments:
one `(shape, dtype)` per output, dense row-major on the device of the inputs (`None`: the call returns nothing and writes
`outputs` in place; `UNBACKED`: a size known only on the device).  Neighbour tables are computed here in numpy, so the
samples need no other operator.

Sizes are the smallest that still cross a wave (64 lanes) and a padding boundary: N = 3, P1 = 70, P2 = 90, D = 3, K = 5
for the searches, lengths full / partial / 0 and a target cloud shorter than K, every Optional argument as None and as a
tensor, and the degenerate shapes the C ABI accepts (N = 0, P1 = 0, K = 1).
"""
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

import cases
from pytorch3d_pointops_amd import synth

UNBACKED = "unbacked"
F32, F64, I64 = torch.float32, torch.float64, torch.int64

N, P1, P2, D, K = 3, 70, 90, 3, 5
L1_FULL, L1_RAGGED = np.array([P1] * N), np.array([P1, 33, 0])
L2_FULL, L2_RAGGED = np.array([P2] * N), np.array([P2, 3, 0])  # 3 < K: a target cloud with fewer than K points


class Op(NamedTuple):
    samples: Callable  # to -> {sample name: argument tuple}
    outputs: Callable  # *args -> [(shape, dtype), ...] or None
    c_name: Optional[str] = None  # the `_C` callable (default: the same name)
    differentiable: Tuple[int, ...] = ()  # positions of the arguments the registered autograd formula differentiates
    opcheck_skip: Dict[str, str] = {}  # opcheck utility -> why it cannot express this operator
    opcheck_forward_only: Dict[str, str] = {}  # opcheck utility -> why it runs without differentiable leaves


# ------------------------------------------------------------------------------------------------ numpy tables
def knn_table(p1, p2, l1, l2, k, norm=2):
    """(N,P1,k) int64 neighbour table in ascending distance order; 0 in rows >= l1[n] and slots >= l2[n]."""
    idx = np.zeros((p1.shape[0], p1.shape[1], k), np.int64)
    for n in range(p1.shape[0]):
        m = min(int(l2[n]), k)
        if l1[n] == 0 or m == 0:
            continue
        diff = p1[n, :l1[n], None, :].astype(np.float64) - p2[n, None, :l2[n], :].astype(np.float64)
        d = np.abs(diff).sum(-1) if norm == 1 else (diff * diff).sum(-1)
        idx[n, :l1[n], :m] = np.argsort(d, axis=1, kind="stable")[:, :m]
    return idx


def ball_table(p1, p2, l1, l2, k, radius):
    """(N,P1,k) int64: the first k points of p2 inside the ball, in index order, padded with -1."""
    idx = np.full((p1.shape[0], p1.shape[1], k), -1, np.int64)
    for n in range(p1.shape[0]):
        for i in range(int(l1[n])):
            diff = p2[n, :l2[n]].astype(np.float64) - p1[n, i].astype(np.float64)
            hit = np.nonzero((diff * diff).sum(-1) < radius * radius)[0][:k]
            idx[n, i, :len(hit)] = hit
    return idx


def _pair(seed=7101, n=N, p1=P1, p2=P2, d=D):
    return cases.cloud(seed, (n, p1, d)), cases.cloud(seed + 1, (n, p2, d))


def _signed(seed, shape):
    return (synth.uniform_f32(seed, shape) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)


def _place(to, *arrays):
    return tuple(None if a is None else (to(a) if isinstance(a, np.ndarray) else a) for a in arrays)


# ------------------------------------------------------------------------------------------------ searches
def _search_shapes():
    """name -> (p1, p2, l1, l2, K)"""
    a, b = _pair()
    return {
        "full": (a, b, L1_FULL, L2_FULL, K),
        "ragged": (a, b, L1_RAGGED, L2_RAGGED, K),
        "k1": (a, b, L1_RAGGED, L2_RAGGED, 1),
        "n0": (a[:0], b[:0], L1_FULL[:0], L2_FULL[:0], K),
        "p1_0": (a[:, :0], b, np.zeros(N, np.int64), L2_RAGGED, K),
    }


def _knn_samples(to):
    out = {}
    for name, (a, b, l1, l2, k) in _search_shapes().items():
        for norm in (2, 1) if name in ("ragged", "full") else (2,):
            out[f"{name}_l{norm}"] = _place(to, a, b, l1, l2) + (norm, k, -1)
    return out


def _knn_backward_samples(to):
    out = {}
    for name, (a, b, l1, l2, k) in _search_shapes().items():
        for norm in (2, 1) if name == "ragged" else (2,):
            idx = knn_table(a, b, l1, l2, k, norm)
            out[f"{name}_l{norm}"] = _place(to, a, b, l1, l2, idx) + (norm, to(_signed(7110, idx.shape)))
    a, b = _pair()
    idx = ball_table(a, b, L1_RAGGED, L2_RAGGED, K, 0.3)  # a table with -1 padding
    out["ball_table"] = _place(to, a, b, L1_RAGGED, L2_RAGGED, idx) + (2, to(_signed(7111, idx.shape)))
    return out


def _ball_samples(to):
    out = {name: _place(to, a, b, l1, l2) + (k, 0.3) for name, (a, b, l1, l2, k) in _search_shapes().items()}
    a, b = _pair()
    out["empty_balls"] = _place(to, a, b, L1_FULL, L2_FULL) + (K, 1e-4)  # every row padding
    return out


def _nk(p1, p2, l1, l2, *rest):
    k = rest[1] if len(rest) == 3 else rest[0]  # (norm, K, version) or (K, radius)
    return [((p1.shape[0], p1.shape[1], k), I64), ((p1.shape[0], p1.shape[1], k), F32)]


# ------------------------------------------------------------------------------------------------ FPS
def _fps_samples(to):
    pts = cases.cloud(7201, (N, P1, D))
    zero = np.zeros(N, np.int64)
    return {
        "full": _place(to, pts, L1_FULL, np.array([K] * N), zero) + (K,),
        "ragged_unknown_max": _place(to, pts, L1_RAGGED, np.array([K, 40, 2]), np.array([69, 5, 0])) + (None,),
        "ragged_known_max": _place(to, pts, L1_RAGGED, np.array([K, 40, 2]), np.array([69, 5, 0])) + (40,),
        "k1": _place(to, pts, L1_RAGGED, np.array([1] * N), zero) + (1,),
        "n0": _place(to, pts[:0], zero[:0], zero[:0], zero[:0]) + (None,),
    }


def _fps_outputs(points, lengths, k, start, max_k):
    return [((points.shape[0], 0 if points.shape[0] == 0 else UNBACKED if max_k is None else max_k), I64)]


# ------------------------------------------------------------------------------------------------ packed <-> padded
_LENS = np.array([5, 0, 70, 3])  # an empty cloud, one past a wave
_FIRST = np.concatenate([[0], np.cumsum(_LENS)[:-1]]).astype(np.int64)


def _packed_samples(to):
    out = {}
    for u in (1, 3, 5):
        out[f"u{u}"] = _place(to, cases.cloud(7300 + u, (int(_LENS.sum()), u)), _FIRST) + (70,)
    out["short_pad"] = _place(to, cases.cloud(7306, (int(_LENS.sum()), 3)), _FIRST) + (8,)  # max_size < a cloud: cut
    out["b0"] = _place(to, cases.cloud(7307, (4, 3)), _FIRST[:0]) + (6,)
    out["f0"] = _place(to, cases.cloud(7308, (0, 3)), np.zeros(2, np.int64)) + (4,)
    return out


def _padded_samples(to):
    out = {}
    for u in (1, 3, 5):
        out[f"u{u}"] = _place(to, cases.cloud(7310 + u, (len(_LENS), 70, u)), _FIRST) + (int(_LENS.sum()),)
    out["unowned_rows"] = _place(to, cases.cloud(7316, (len(_LENS), 70, 3)), _FIRST + 2) + (int(_LENS.sum()) + 2,)
    out["b0"] = _place(to, cases.cloud(7317, (0, 6, 3)), _FIRST[:0]) + (4,)
    out["f0"] = _place(to, cases.cloud(7318, (2, 4, 3)), np.zeros(2, np.int64)) + (0,)
    return out


# ------------------------------------------------------------------------------------------------ gathers
def _gather_shapes():
    """name -> (x (N,M,U), idx (N,L,K), lengths or None)"""
    a, b = _pair()
    out = {}
    for u in (1, 3, 5):
        x = _signed(7400 + u, (N, P2, u))
        out[f"u{u}_lengths"] = (x, knn_table(a, b, L1_RAGGED, L2_RAGGED, K), L2_RAGGED)
        out[f"u{u}_none"] = (x, ball_table(a, b, L1_RAGGED, L2_RAGGED, K, 0.3), None)  # -1 padding
    x = _signed(7406, (N, P2, 3))
    out["k1"] = (x, knn_table(a, b, L1_RAGGED, L2_RAGGED, 1), L2_RAGGED)
    out["n0"] = (x[:0], np.zeros((0, P1, K), np.int64), None)
    out["l0"] = (x, np.zeros((N, 0, K), np.int64), L2_RAGGED)
    return out


def _gather_samples(to):
    return {name: _place(to, *args) for name, args in _gather_shapes().items()}


def _gather_backward_samples(to):
    return {name: _place(to, _signed(7410, idx.shape + (x.shape[2],)), idx, lengths) + (x.shape[1],)
            for name, (x, idx, lengths) in _gather_shapes().items()}


# ------------------------------------------------------------------------------------------------ covariances, frames
def _neighbourhoods():
    """name -> knn (N,P,K,D)"""
    return {"d3_k5": _signed(7501, (N, P1, K, 3)), "d1_k8": _signed(7502, (2, 70, 8, 1)),
            "d5_k1": _signed(7503, (2, 33, 1, 5)), "n0": _signed(7504, (0, 7, K, 3)), "p0": _signed(7505, (2, 0, K, 3))}


def _cov_samples(to):
    return {name: _place(to, knn) for name, knn in _neighbourhoods().items()}


def _cov_backward_samples(to):
    return {name: _place(to, knn, _signed(7510, knn.shape[:2] + (knn.shape[3],) * 2))
            for name, knn in _neighbourhoods().items()}


FRAMES_P, FRAMES_K = 200, 8


def frames_clouds():
    """name -> (points (N,P,3), lengths, K): centred clouds, every non-empty cloud longer than K."""
    pts = _signed(7601, (N, FRAMES_P, 3))
    return {"full": (pts, np.array([FRAMES_P] * N), FRAMES_K), "ragged": (pts, np.array([FRAMES_P, 77, 0]), FRAMES_K),
            "k1": (pts[:, :70], np.array([70, 33, 0]), 1), "n0": (pts[:0], np.zeros(0, np.int64), FRAMES_K),
            "p0": (pts[:, :0], np.zeros(N, np.int64), FRAMES_K)}


def _frames_samples(to):
    out = {}
    for name, (pts, lens, k) in frames_clouds().items():
        idx = knn_table(pts, pts, lens, lens, k)
        for flag in (True, False) if name == "ragged" else (True,):
            out[f"{name}_{'disambiguated' if flag else 'raw'}"] = _place(to, pts, lens, idx) + (flag,)
    return out


def _frames_backward_samples(to):
    """Unit frames and ascending, well separated curvatures (any orthonormal frame is a valid saved output)."""
    out = {}
    for name, (pts, lens, _k) in frames_clouds().items():
        n, p = pts.shape[:2]
        q = np.linalg.qr(_signed(7610, (n, p, 3, 3)).astype(np.float64))[0].astype(np.float32)
        curv = (np.sort(synth.uniform_f32(7611, (n, p, 3)), axis=-1) + np.arange(3, dtype=np.float32)).astype(np.float32)
        out[name] = _place(to, curv, q, _signed(7612, (n, p, 3)), _signed(7613, (n, p, 3, 3)), lens) + (name != "k1",)
    return out


# ------------------------------------------------------------------------------------------------ alignment
def _alignment_samples(to):
    out = {}
    for d in (3, 2):
        x, y = _signed(7700 + d, (N, P1, d)), _signed(7710 + d, (N, P1, d))
        w = synth.uniform_f32(7720 + d, (N, P1))
        out[f"d{d}_plain"] = _place(to, x, y, None, None, None) + (False, False, 1e-9)
        out[f"d{d}_lengths_weights_scale"] = _place(to, x, y, None, L1_RAGGED, w) + (True, False, 1e-9)
    x, y = _signed(7731, (N, P1, 3)), _signed(7732, (N, P2, 3))
    idx = knn_table(x, y, L1_FULL, L2_FULL, 1)[..., 0]
    out["idx_reflection"] = _place(to, x, y, idx, L1_RAGGED, None) + (False, True, 1e-9)
    out["n0"] = _place(to, x[:0], x[:0], None, None, None) + (True, False, 1e-9)
    return out


def _alignment_outputs(x, y, idx, lengths, weights, *flags):
    n, _, d = x.shape
    return [((n, d, d), F32), ((n, d), F32), ((n,), F32), ((n, d), F32), ((n, 3 + 4 * d + d * d), F64)]


def _alignment_backward_samples(to):
    out = {}
    for d in (3, 2):
        x, y = _signed(7740 + d, (N, P1, d)), _signed(7750 + d, (N, P1, d))
        gm = _signed(7760 + d, (N, 3 + 4 * d + d * d)).astype(np.float64)
        out[f"d{d}_plain"] = _place(to, x, y, None, None, gm)
        out[f"d{d}_lengths_weights"] = _place(to, x, y, L1_RAGGED, synth.uniform_f32(7770 + d, (N, P1)), gm)
    out["n0"] = _place(to, x[:0], y[:0], None, None, gm[:0])
    return out


# ------------------------------------------------------------------------------------------------ chamfer
def _chamfer_inputs():
    a, b = _pair(7801)
    idx = knn_table(a, b, L1_RAGGED, np.array([P2, 3, 1]), 1)[..., 0]
    feats = ([_signed(7803, (N, P1, 3)), _signed(7804, (N, P1, 1))], [_signed(7805, (N, P2, 3)), _signed(7806, (N, P2, 1))])
    return a, b, idx, L1_RAGGED, np.array([P2, 3, 1]), np.array([1.0, 0.5, 2.0], np.float32), feats


def _chamfer_reduce_samples(to):
    dists = synth.uniform_f32(7810, (N, P1))
    w = np.array([1.0, 0.5, 2.0], np.float32)
    return {"mean_weights": _place(to, dists, L1_RAGGED, w) + (True,), "sum_none": _place(to, dists, L1_RAGGED, None) + (False,),
            "mean_full": _place(to, dists, L1_FULL, None) + (True,), "n0": _place(to, dists[:0], L1_FULL[:0], None) + (True,)}


def _chamfer_forward_samples(to):
    a, b, idx, xl, yl, w, (xf, yf) = _chamfer_inputs()
    dists = synth.uniform_f32(7811, (N, P1))
    out = {}
    for f in (0, 1):
        fx, fy = [to(t) for t in xf[:f]], [to(t) for t in yf[:f]]
        out[f"f{f}_weights_mean"] = _place(to, dists, idx, xl, yl, w) + (fx, fy, True, True)
        out[f"f{f}_none_sum"] = _place(to, dists, idx, xl, yl, None) + (fx, fy, False, False)
    out["n0"] = _place(to, dists[:0], idx[:0], xl[:0], yl[:0], None) + ([], [], True, True)
    return out


def _chamfer_backward_samples(to):
    a, b, idx, xl, yl, w, (xf, yf) = _chamfer_inputs()
    out = {}
    for f in (0, 1):
        fx, fy = [to(t) for t in xf[:f]], [to(t) for t in yf[:f]]
        g = _signed(7812, (1 + f, N))
        out[f"f{f}_weights_mean_l2"] = _place(to, a, b, idx, xl, yl, w, g) + (2, fx, fy, True, True)
        out[f"f{f}_none_sum_l1"] = _place(to, a, b, idx, xl, yl, None, g) + (1, fx, fy, False, False)
    out["n0"] = _place(to, a[:0], b[:0], idx[:0], xl[:0], yl[:0], None, _signed(7813, (1, 0))) + (2, [], [], True, True)
    return out


# ------------------------------------------------------------------------------------------------ sample_pdf
def _pdf_samples(to):
    def one(seed, batch, nb, ns):
        bins = np.sort(synth.uniform_f32(seed, (batch, nb + 1)), axis=1).astype(np.float32)
        w = synth.uniform_f32(seed + 1, (batch, nb))
        w[:1, : nb // 3] = 0.0
        u = synth.uniform_f32(seed + 2, (batch, ns))
        if u.size:
            u[0, 0], u[0, -1] = 0.0, 1.0
        return _place(to, bins, w, u) + (1e-5,)

    return {"b4_7x33": one(7901, 4, 7, 33), "b1_1x1": one(7904, 1, 1, 1), "b0": one(7907, 0, 7, 33)}


# opcheck's AOT utility sums every output into ONE accumulator that takes the dtype of the first output: an int64 index
# table in front of fp32 distances raises inside the utility as soon as a backward pass is asked for.  The forward runs
# through it; the AOT backward of these two is pinned by test_compiled_equals_eager (aot_eager, gradients included).
_INDEX_FIRST = {"test_aot_dispatch_dynamic": "the first output is the int64 index table: the utility's accumulator cannot "
                                             "add the fp32 distances to it (test_compiled_equals_eager covers the backward)"}

TABLE = {
    "knn_points_idx": Op(_knn_samples, _nk, differentiable=(0, 1), opcheck_forward_only=_INDEX_FIRST),
    "knn_points_backward": Op(_knn_backward_samples,
                              lambda p1, p2, l1, l2, idx, norm, g: [(tuple(p1.shape), F32), (tuple(p2.shape), F32)]),
    "ball_query": Op(_ball_samples, _nk, differentiable=(0, 1), opcheck_forward_only=_INDEX_FIRST),
    "sample_farthest_points": Op(_fps_samples, _fps_outputs, opcheck_skip={
        "test_aot_dispatch_dynamic": "max(K) is an unbacked size: AOT dispatch compares outputs of data-dependent shape "
                                     "(test_fps_unbacked_dimension_is_max_k checks the property directly)"}),
    "packed_to_padded": Op(_packed_samples, lambda x, first, size: [((first.shape[0], size, x.shape[1]), F32)],
                           differentiable=(0,)),
    "padded_to_packed": Op(_padded_samples, lambda x, first, rows: [((rows, x.shape[2]), F32)], differentiable=(0,)),
    "gather_neighbors": Op(_gather_samples, lambda x, idx, lengths: [(tuple(idx.shape) + (x.shape[2],), F32)],
                           differentiable=(0,)),
    "gather_neighbors_backward": Op(_gather_backward_samples,
                                    lambda g, idx, lengths, m: [((g.shape[0], m, g.shape[3]), F32)]),
    "point_covariances": Op(_cov_samples, lambda knn: [(tuple(knn.shape[:2]) + (knn.shape[3],) * 2, F32)],
                            differentiable=(0,)),
    "point_covariances_backward": Op(_cov_backward_samples, lambda knn, g: [(tuple(knn.shape), F32)]),
    "local_frames": Op(_frames_samples, lambda pts, lens, idx, flag: [(tuple(pts.shape[:2]) + (3,), F32),
                                                                      (tuple(pts.shape[:2]) + (3, 3), F32)],
                       differentiable=(0,)),
    "local_frames_backward": Op(_frames_backward_samples,
                                lambda curv, frames, gc, gf, lens, flag: [(tuple(frames.shape), F32)]),
    "points_alignment": Op(_alignment_samples, _alignment_outputs, differentiable=(0, 1, 4)),
    "points_alignment_backward": Op(_alignment_backward_samples, lambda x, y, lens, w, gm: [
        (tuple(x.shape), F32), (tuple(y.shape), F32)] + ([] if w is None else [(tuple(w.shape), F32)])),
    "chamfer_reduce": Op(_chamfer_reduce_samples, lambda d, lens, w, mean: [((d.shape[0],), F32)], differentiable=(0,)),
    "chamfer_forward": Op(_chamfer_forward_samples,
                          lambda d, idx, xl, yl, w, xf, yf, ac, mean: [((1 + len(xf), d.shape[0]), F32)]),
    "chamfer_backward": Op(_chamfer_backward_samples, lambda x, y, idx, xl, yl, w, g, norm, xf, yf, ac, mean: [
        (tuple(t.shape), F32) for t in (x, y, *xf, *yf)]),
    "sample_pdf": Op(_pdf_samples, lambda bins, w, outputs, eps: None),
}

# What each schema must say (checked against the inferred schemas and against what `_C` accepts as None).
OPTIONAL_ARGUMENTS = {
    "sample_farthest_points": {"max_K"}, "gather_neighbors": {"lengths"}, "gather_neighbors_backward": {"lengths"},
    "points_alignment": {"idx", "lengths", "weights"}, "points_alignment_backward": {"lengths", "weights"},
    "chamfer_reduce": {"weights"}, "chamfer_forward": {"weights"}, "chamfer_backward": {"weights"},
}
MUTATED_ARGUMENTS = {"sample_pdf": {"outputs"}}
# Parameters of the `_C` callable that the registered op does not take (the op reads them from torch's global state
# or fixes them), by op.
C_ONLY_PARAMETERS = {
    "knn_points_backward": {"deterministic"},  # torch.are_deterministic_algorithms_enabled()
    "gather_neighbors_backward": {"deterministic"},
    "points_alignment": {"want_moments"},  # always True: the registered backward starts from the moments
    "chamfer_backward": {"into"},  # the accumulating form writes into caller buffers: eager `_chamfer_pair` only
}
