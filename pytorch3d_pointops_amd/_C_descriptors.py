"""Operator boundary of the shape descriptors (csrc/fpfh.hip; C ABI: pointops_spfh / pointops_fpfh in
include/pointops_amd.h).

The two wrappers live beside `_C.py`, not in it: they are eager-only building blocks of functions/fpfh.py, not
registered operators.  Everything they use is `_C`'s -- the argument normalisers, the native-call namespace and the
output seam -- looked up on the module at call time, so whatever patches `_C._out` or `_C._call` sees these calls too.
There is no CPU implementation: CPU tensors raise RuntimeError.
"""
import torch

from . import _C

SPFH_BINS = 33
SPFH_MAX_K = 255


def _check(what, points, idx, lengths):
    if points.dim() != 3 or points.shape[2] != 3 or idx.dim() != 3 or idx.shape[:2] != points.shape[:2] \
            or (lengths is not None and lengths.shape != points.shape[:1]):
        raise RuntimeError(f"{what}: need points (N,P,3), idx (N,P,K) and lengths (N,)")
    N, P, K = idx.shape
    if not 1 <= K <= SPFH_MAX_K:
        raise RuntimeError(f"{what}: K must be in 1..{SPFH_MAX_K}")
    return N, P, K


def spfh(points, normals, idx, lengths=None, want_pair_features: bool = False):
    """points, normals (N,P,3) fp32, idx (N,P,K) int64, lengths (N,) or None -> (pair_features (N,P,K,4) or None,
    spfh (N,P,33))."""
    dev = _C._require_gpu(points, normals, idx, lengths)
    points, normals = _C._f32c(points, "points"), _C._f32c(normals, "normals")
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    N, P, K = _check("spfh", points, idx, lengths)
    if normals.shape != points.shape:
        raise RuntimeError("spfh: normals must have the shape of points")
    pair = _C._out((N, P, K, 4), dtype=torch.float32, device=dev) if want_pair_features else None
    hist = _C._out((N, P, SPFH_BINS), dtype=torch.float32, device=dev)
    _C._call.spfh("spfh", dev, points, normals, idx, lengths, N, P, K, pair, hist)
    return pair, hist


def fpfh(points, idx, lengths, spfh):
    """points (N,P,3) fp32, idx (N,P,K) int64, lengths (N,) or None, spfh (N,P,33) fp32 -> fpfh (N,P,33)."""
    dev = _C._require_gpu(points, idx, lengths, spfh)
    points, spfh = _C._f32c(points, "points"), _C._f32c(spfh, "spfh")
    idx, lengths = _C._i64c(idx, "idx"), _C._i64c(lengths, "lengths")
    N, P, K = _check("fpfh", points, idx, lengths)
    if spfh.shape != (N, P, SPFH_BINS):
        raise RuntimeError("fpfh: spfh must be (N,P,33)")
    out = _C._out((N, P, SPFH_BINS), dtype=torch.float32, device=dev)
    _C._call.fpfh("fpfh", dev, points, idx, lengths, spfh, N, P, K, out)
    return out
