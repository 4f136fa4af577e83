"""Operator boundary: the same callables as the reference's pybind11 module
``pytorch3d_pointops._C`` (reference: csrc/ext.cpp:15-27), implemented as ctypes
calls into ``lib/libpointops_amd.so`` (C ABI: include/pointops_amd.h).

PyTorch is plumbing only here: it owns device memory (outputs are fresh tensors on
the input device, like the reference's ``at::zeros`` / ``at::full``), the current
HIP stream and the device guard.  There is NO CPU implementation behind these
functions: CPU tensors raise ``RuntimeError`` (the mirror image of the reference's
"Not compiled with GPU support." -- csrc/knn/knn.h:74), and a missing shared
library raises at import of this module.
"""
import collections
import ctypes
import os
import types
import weakref

import torch  # must be imported first: loads the process-wide HIP runtime (libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
# POINTOPS_AMD_LIB: another build of the same library (tools/build_variant.py tuning experiments)
LIB_PATH = os.environ.get("POINTOPS_AMD_LIB") or os.path.join(_HERE, "lib", "libpointops_amd.so")

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f32 = ctypes.c_float
_f64 = ctypes.c_double
_sz = ctypes.c_size_t

# name -> (restype, argtypes): every prototype of include/pointops_amd.h, type by type (tests/test_boundary_cpu.py
# parses the header and compares)
_SIGNATURES = {
    "pointops_abi_version": (_int, []),
    "pointops_target_arch": (ctypes.c_char_p, []),
    "pointops_last_error": (ctypes.c_char_p, []),
    "pointops_knn_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64, _int]),
    "pointops_knn_points_idx": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _i64, _int,
                                       _vp, _vp, _vp, _sz, _vp]),
    "pointops_knn_plan": (_int, [_i64, _i64, _i64, _i64, _i64, _int, _vp, _vp]),
    "pointops_knn_uses_grid": (_int, [_i64, _i64, _i64, _i64, _i64, _int]),
    "pointops_knn_points_idx_reuse": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _i64, _int,
                                             _vp, _vp, _vp, _sz, _int, _vp]),
    "pointops_knn_check_version": (_int, [_int, _i64, _i64]),
    "pointops_knn_grid_fallback_counts": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_knn_grid_stats": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_knn_points_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64,
                                            _i64, _int, _vp, _vp, _vp]),
    "pointops_ball_query_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "pointops_ball_query": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _sz,
                                  _vp]),
    "pointops_fps_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_sample_farthest_points": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp,
                                               _sz, _vp]),
    "pointops_packed_to_padded": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_padded_to_packed": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_gather_neighbors": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_gather_neighbors_backward": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp,
                                                  _vp]),
    "pointops_backward_det_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "pointops_knn_points_backward_det": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp,
                                                _vp, _vp, _sz, _vp]),
    "pointops_gather_neighbors_backward_det": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "pointops_chamfer_reduce": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp, _vp]),
    "pointops_sample_pdf": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _f32, _vp]),
    "pointops_point_covariances": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_point_covariances_backward": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "pointops_local_frames": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "pointops_local_frames_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _vp, _vp]),
    "pointops_points_alignment_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_points_alignment": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _f64, _vp, _vp,
                                         _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_points_alignment_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "pointops_icp_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_icp_iteration": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _f32,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "pointops_registration_search_version": (_int, []),
    "pointops_registration_workspace_bytes": (_sz, [_i64, _i64]),
    "pointops_registration_step": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _f32, _f64, _f64, _int,
                                          _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "pointops_spfh": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "pointops_fpfh": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "pointops_ransac_chunk": (_i64, []),
    "pointops_ransac_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_ransac_alignment": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _f32,
                                         _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _sz, _vp]),
    "pointops_cluster_workspace_bytes": (_sz, [_i64, _i64]),
    "pointops_cluster_dbscan": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_iss_workspace_bytes": (_sz, [_i64, _i64]),
    "pointops_iss_keypoints": (_int, [_vp, _vp, _i64, _i64, _f32, _f32, _f32, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _sz,
                                      _vp]),
    "pointops_mls_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_mls_smooth": (_int, [_vp, _vp, _i64, _i64, _f32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_voxel_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_voxel_downsample": (_int, [_vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _sz, _vp]),
    "pointops_mask_compact": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "pointops_radius_outlier_workspace_bytes": (_sz, [_i64, _i64]),
    "pointops_radius_outlier": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_statistical_outlier_workspace_bytes": (_sz, [_i64, _i64]),
    "pointops_statistical_outlier": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                            _vp]),
    "pointops_knn_in_radius_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "pointops_knn_in_radius": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _sz,
                                      _int, _vp]),
    "pointops_feature_knn_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "pointops_feature_knn": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_feature_screen_values": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pointops_plane_chunk": (_i64, []),
    "pointops_plane_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "pointops_segment_plane": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _int, _f32, _f32, _f32,
                                      _f32, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_chamfer_workspace_bytes": (_sz, [_i64, _i64]),
    "pointops_chamfer_forward": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _int,
                                        _int, _vp, _vp, _sz, _vp]),
    "pointops_chamfer_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int,
                                         _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "pointops_chamfer_backward_accumulate": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int,
                                                    _int, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "pointops_chamfer_pair_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int]),
    "pointops_chamfer_pair_backward_workspace_bytes": (_sz, [_i64, _int]),
    "pointops_chamfer_pair_forward": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _vp, _vp,
                                             _int, _int, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pointops_chamfer_pair_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int,
                                              _vp, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m pytorch3d_pointops_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.pointops_abi_version() != 1:
        raise ImportError("libpointops_amd.so ABI version mismatch")
    return lib


_lib = _load()


def exported_symbols():
    return sorted(_SIGNATURES)


def _check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed ({code}): {_lib.pointops_last_error().decode()}")


# ---------------------------------------------------------------------------
# Argument normalisers.  None (an optional tensor) passes through all of them.
# ---------------------------------------------------------------------------
def _require_gpu(*tensors):
    """The one device of the tensors; this check comes first in every wrapper."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "pytorch3d_pointops_amd is a GPU-only (MI355X / gfx950) implementation: got a CPU "
                "tensor and there is no CPU fallback."
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("All tensors must be on the same GPU device")
    return dev


def _contig(t, name):
    """`t` itself, which must be contiguous already: where the reference raises (CHECK_CONTIGUOUS) or the call writes
    into the caller's tensor, a silent copy would be wrong."""
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


def _f32c(t, name, copy=True):
    """fp32 + contiguous view of a device tensor whose data pointer goes to a kernel (`copy=False`: see _contig)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError(f"expected scalar type Float for {name}")  # CPU ref: same restriction
    return t.contiguous() if copy else _contig(t, name)


def _i64c(t, name):
    """The kernels read int64 through raw pointers: any other integer type would be read past its buffer (the
    reference's accessor<int64_t, 1> raises: knn_cpu.cpp:84-88)."""
    if t is None:
        return None
    if t.dtype != torch.int64:
        raise RuntimeError(f"{name} must be int64")
    return t.contiguous()


# ---------------------------------------------------------------------------
# The native call: device guard, current stream, pointers, error check.
# ---------------------------------------------------------------------------
class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(dev):
    """Device guard for the launches: torch.cuda.device(dev) only when `dev` is not already current (its constructor,
    __enter__ and __exit__ cost ~4 us of a small call; the usual single-GPU process never needs the switch).  None: the
    caller holds the guard already."""
    return _NO_GUARD if dev is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (as an int)."""
    if _raw_stream is not None:  # one C call instead of building a torch.cuda.Stream object
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _bind(name, argtypes):
    """Python caller `f(what, dev, *args)` of one stream-taking entry: under the guard of `dev`, with every pointer
    argument's data_ptr() (None: a null pointer; a bool goes as an int by itself) and the current stream appended,
    raising through _check under the display name `what`.  It is compiled once from the entry's argtypes because these
    calls are host-bound at small sizes: converting in a loop with a type test per argument costs 1-2 us of a 13 us
    knn_points call (tools/host_overhead.py), this costs what the hand-written call did."""
    names = [f"a{i}" for i in range(len(argtypes) - 1)]  # (the last argument is the stream)
    conv = [f"{n}.data_ptr() if {n} is not None else None" if t is _vp else n for n, t in zip(names, argtypes)]
    scope = {}
    exec(f"def {name}(what, dev, {', '.join(names)}):\n"
         f"    with _on(dev):\n"
         f"        _check(_lib.{name}({', '.join(conv)}, _stream()), what)\n", globals(), scope)
    return scope[name]


# entries that return a code and end in a pointer which is a HOST output, not a stream: they launch nothing
_HOST_QUERIES = ("pointops_knn_plan",)

# _call.<entry without "pointops_">(what, dev, *args) for every entry that launches (returns a code, takes a stream)
_call = types.SimpleNamespace(**{name[len("pointops_"):]: _bind(name, args) for name, (res, args) in _SIGNATURES.items()
                                 if res is _int and args and args[-1] is _vp and name not in _HOST_QUERIES})


# The three names every device buffer that a native call writes comes through -- outputs (_out, _out_like) and scratch
# (_workspace): uninitialised memory, which the C ABI permits ("outputs are FULLY written by the call", scratch needs no
# particular contents).  Plain aliases, no Python frame (these calls are host-bound: tools/host_overhead.py);
# tests/buffers.py patches them to hand out guarded, poisoned buffers.
_out = torch.empty
_out_like = torch.empty_like


def _workspace(nbytes: int, dev):
    """Device scratch of one native call, or None when it needs none.  A fresh tensor per call: the caching allocator
    is stream-ordered (the block is handed out again only behind this call's launches), and inside a HIP-graph capture
    it comes from the graph's private pool (graphs.py)."""
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None


def _scratch(dev, sizer, *dims):
    """(workspace, workspace_bytes) of one native call, sized by the library's own `sizer(*dims)`: the adjacent pair
    of arguments every entry with scratch takes."""
    nbytes = sizer(*dims)
    return _workspace(nbytes, dev), nbytes


# ---------------------------------------------------------------------------
# Grid reuse (opt-in): the cell grid of the exact search is an index over p2 -- bounding boxes, cell tables, the
# cell-sorted copy of the cloud, refined cells: 123 us of a 705 us call at B=32, N=M=65536, K=16 -- that a second
# query of the SAME target cloud does not have to rebuild (chamfer against a fixed ground truth, knn_points followed
# by further queries).  With the switch on, knn_points_idx keeps the workspaces of its last few grid calls and hands
# them back to the C ABI (pointops_knn_points_idx_reuse) when the target tensors are provably the ones it was built
# from: the same tensor OBJECTS (weak references), the same data pointers and the same autograd version counters --
# every in-place op of PyTorch bumps that counter.  It is OFF by default because some writes are invisible to it
# (set_grid_cache lists them), and a stale grid then answers for the OLD points (the reference's stateless operator
# has no such failure mode).
#   pytorch3d_pointops_amd.set_grid_cache(True [, max_entries])      or      POINTOPS_GRID_CACHE=1
# ---------------------------------------------------------------------------
_GRID_CACHE = collections.OrderedDict()
_GRID_CACHE_ON = os.environ.get("POINTOPS_GRID_CACHE", "0") not in ("", "0")
_GRID_CACHE_MAX = 2
grid_cache_stats = {"miss": 0, "points": 0, "both": 0}


def set_grid_cache(enabled: bool, max_entries: int = 2) -> None:
    """Switch the grid reuse of knn_points_idx on or off (off: the default; cached workspaces are dropped).

    The cache trusts a target tensor whose object, data pointer and version counter are unchanged.  Writes that change
    its bytes without bumping the counter are NOT seen, and the reused grid then answers for the old points:
    `p2.data.copy_(...)`, a raw-pointer write from another library, a HIP-graph replay that rewrites `p2` (graphs.py),
    and writes through a DLPack or numpy alias of its storage."""
    global _GRID_CACHE_ON, _GRID_CACHE_MAX
    _GRID_CACHE_ON = bool(enabled)
    _GRID_CACHE_MAX = max(1, int(max_entries))
    if not enabled:
        _GRID_CACHE.clear()


def grid_cache_enabled() -> bool:
    return _GRID_CACHE_ON


def _sig(t):
    return (id(t), t._version, t.data_ptr(), tuple(t.shape))


def _grid_workspace(p1, p2, lengths1, lengths2, shape, ws_bytes, dev):
    """(workspace, reuse level, cache key) for a grid call: level 2 when both point sets are the cached call's, 1 when
    the target side is, 0 (a fresh workspace, remembered) otherwise.  The caller drops the key if its call fails."""
    key = (_sig(p2), _sig(lengths2), shape, _stream(), str(dev))
    hit = _GRID_CACHE.get(key)
    if hit is not None and hit["p2"]() is p2 and hit["l2"]() is lengths2 and hit["ws"].numel() == ws_bytes:
        _GRID_CACHE.move_to_end(key)
        q = (_sig(p1), _sig(lengths1))
        level = 2 if (hit["q"] == q and hit["p1"]() is p1 and hit["l1"]() is lengths1) else 1
        hit.update(q=q, p1=weakref.ref(p1), l1=weakref.ref(lengths1))
        grid_cache_stats["both" if level == 2 else "points"] += 1
        return hit["ws"], level, key
    grid_cache_stats["miss"] += 1
    for k in [k for k, v in _GRID_CACHE.items() if v["p2"]() is None]:
        del _GRID_CACHE[k]  # entries whose target tensor has died
    ws = _workspace(ws_bytes, dev)
    _GRID_CACHE[key] = dict(ws=ws, p2=weakref.ref(p2), l2=weakref.ref(lengths2), q=(_sig(p1), _sig(lengths1)),
                            p1=weakref.ref(p1), l1=weakref.ref(lengths1))
    while len(_GRID_CACHE) > _GRID_CACHE_MAX:
        _GRID_CACHE.popitem(last=False)
    return ws, 0, key


# ---------------------------------------------------------------------------
# reference: csrc/knn/knn.h:59-80 -- returns (idx, dists), NOT (dists, idx)
# ---------------------------------------------------------------------------
def knn_points_idx(p1, p2, lengths1, lengths2, norm: int, K: int, version: int = -1):
    dev = _require_gpu(p1, p2, lengths1, lengths2)
    # (a self-query -- the same storage for both point sets and both lengths -- is recognised by the C ABI from pointer
    # equality and sorts the cloud once: .contiguous() of a contiguous tensor is the tensor itself)
    p1, p2 = _f32c(p1, "p1"), _f32c(p2, "p2")  # reference CUDA path: knn.cu:373-376
    lengths1, lengths2 = _i64c(lengths1, "lengths1"), _i64c(lengths2, "lengths2")
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    if p2.shape[0] != N or p2.shape[2] != D or lengths1.shape != (N,) or lengths2.shape != (N,):
        raise RuntimeError("knn_points_idx: inconsistent shapes")
    K, version = int(K), int(version)
    idxs = _out((N, P1, K), dtype=torch.int64, device=dev)
    dists = _out((N, P1, K), dtype=torch.float32, device=dev)
    ws_bytes = _lib.pointops_knn_workspace_bytes(N, P1, P2, D, K, version)
    with _on(dev):  # (the cache keys on the current stream of `dev`)
        if _GRID_CACHE_ON and ws_bytes and _lib.pointops_knn_uses_grid(N, P1, P2, D, K, version) \
                and not torch.cuda.is_current_stream_capturing():  # (a captured call must not bake a reuse level in)
            ws, reuse, key = _grid_workspace(p1, p2, lengths1, lengths2, (N, P1, P2, D, K, version), ws_bytes, dev)
        else:
            ws, reuse, key = _workspace(ws_bytes, dev), 0, None
        try:
            _call.knn_points_idx_reuse("knn_points_idx", None, p1, p2, lengths1, lengths2, N, P1, P2, D, int(norm), K,
                                       version, idxs, dists, ws, ws_bytes, reuse)
        except Exception:
            _GRID_CACHE.pop(key, None)  # a failed call may have left the grid half built
            raise
    return idxs, dists


def _grid_diagnostics(p1, p2, lengths1, lengths2, norm, K, out_shape, read, what):
    """Run the grid family (version 3), then `read` copies what it left in its workspace into an int32 tensor."""
    dev = _require_gpu(p1, p2, lengths1, lengths2)
    p1 = p1.contiguous()
    p2 = p1 if p2 is p1 else p2.contiguous()
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    K = int(K)
    if not knn_check_version(3, D, K):
        raise RuntimeError("grid family needs D <= 3 and K <= 128")
    idxs = _out((N, P1, K), dtype=torch.int64, device=dev)
    dists = _out((N, P1, K), dtype=torch.float32, device=dev)
    out = _out(out_shape(N), dtype=torch.int32, device=dev)
    ws, ws_bytes = _scratch(dev, _lib.pointops_knn_workspace_bytes, N, P1, P2, D, K, 3)
    with _on(dev):  # (both calls on one stream)
        _call.knn_points_idx("knn_points_idx", None, p1, p2, lengths1, lengths2, N, P1, P2, D, int(norm), K, 3, idxs,
                             dists, ws, ws_bytes)
        read(what, None, ws, N, P1, P2, K, out)
    return idxs, dists, out


def knn_grid_fallback_counts(p1, p2, lengths1, lengths2, norm: int, K: int):
    """Diagnostics: run the grid family (version 3) and return (idx, dists, counts) where
    counts[0, n] = queries of cloud n re-searched wave-per-query on a growing cell cube,
    counts[1, n] = queries that ended in the whole-cloud scan."""
    return _grid_diagnostics(p1, p2, lengths1, lengths2, norm, K, lambda N: (2, N),
                             _call.knn_grid_fallback_counts, "knn_grid_fallback_counts")


def knn_grid_stats(p1, p2, lengths1, lengths2, norm: int, K: int):
    """Diagnostics: run the grid family and return (idx, dists, stats (N, 14) int32): cells per dimension (3),
    cell count, grid used, queries uncertified after the lane pass / the quad + box passes / sent to the whole-cloud
    scan, queries deferred to the box search, refined cells, bins of the point / query sort, crowded bins of the
    point / query sort."""
    return _grid_diagnostics(p1, p2, lengths1, lengths2, norm, K, lambda N: (N, 14), _call.knn_grid_stats,
                             "knn_grid_stats")


KNN_FAMILIES = ("none", "grid", "wide", "generic", "small", "scan")  # POINTOPS_KNN_FAMILY_* of the header, in order


def knn_plan(N: int, P1: int, P2: int, D: int, K: int, version: int = -1):
    """(family name, p2 slices) of the knn_points_idx call of this shape: the dispatch's own answer, debug knobs
    included (pointops_knn_plan).  Host only: nothing is launched."""
    family, splits = ctypes.c_int(-1), ctypes.c_int(-1)
    _check(_lib.pointops_knn_plan(int(N), int(P1), int(P2), int(D), int(K), int(version), ctypes.byref(family),
                                  ctypes.byref(splits)), "knn_plan")
    return KNN_FAMILIES[family.value], splits.value


def knn_check_version(version: int, D: int, K: int) -> bool:
    """reference: csrc/knn/knn.h:161 (GPU builds only)."""
    return bool(_lib.pointops_knn_check_version(int(version), int(D), int(K)))


# reference: csrc/knn/knn.h:127-149
def knn_points_backward(p1, p2, lengths1, lengths2, idxs, norm: int, grad_dists, deterministic: bool = False):
    """`deterministic`: grad_p2 through the inverted neighbour table (csrc/backward_det.hip) -- reproducible and
    bit-equal to the reference's CPU kernel -- instead of fp32 scatter-adds (LDS tiles / device atomics)."""
    dev = _require_gpu(p1, p2, lengths1, lengths2, idxs, grad_dists)
    p1, p2, grad_dists = _f32c(p1, "p1"), _f32c(p2, "p2"), _f32c(grad_dists, "grad_dists")
    lengths1, lengths2, idxs = _i64c(lengths1, "lengths1"), _i64c(lengths2, "lengths2"), _i64c(idxs, "idxs")
    if p1.dim() != 3 or p2.dim() != 3 or idxs.dim() != 3:
        raise RuntimeError("knn_points_backward: p1, p2 and idxs must be 3-dimensional")
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    K = idxs.shape[2]
    if (p2.shape[0] != N or p2.shape[2] != D or idxs.shape != (N, P1, K) or grad_dists.shape != (N, P1, K)
            or lengths1.shape != (N,) or lengths2.shape != (N,)):
        raise RuntimeError("knn_points_backward: inconsistent shapes")
    grad_p1 = _out((N, P1, D), dtype=torch.float32, device=dev)
    grad_p2 = _out((N, P2, D), dtype=torch.float32, device=dev)
    if deterministic:
        entry, what = _call.knn_points_backward_det, "knn_points_backward(deterministic)"
        scratch = _scratch(dev, _lib.pointops_backward_det_workspace_bytes, N, P1, K, P2)
    else:
        entry, what, scratch = _call.knn_points_backward, "knn_points_backward", ()
    entry(what, dev, p1, p2, lengths1, lengths2, idxs, grad_dists, N, P1, P2, D, K, int(norm), grad_p1, grad_p2,
          *scratch)
    return grad_p1, grad_p2


# reference: csrc/ball_query/ball_query.h:62-93 -- returns (idx, dists)
def ball_query(p1, p2, lengths1, lengths2, K: int, radius: float):
    dev = _require_gpu(p1, p2, lengths1, lengths2)
    p1, p2 = _f32c(p1, "p1"), _f32c(p2, "p2")  # ball_query.h:74-77
    lengths1, lengths2 = _i64c(lengths1, "lengths1"), _i64c(lengths2, "lengths2")
    if p1.dim() != 3 or p2.dim() != 3:
        raise RuntimeError("ball_query: p1 and p2 must be 3-dimensional")
    N, P1, D = p1.shape
    P2 = p2.shape[1]
    if p2.shape[0] != N or p2.shape[2] != D or lengths1.shape != (N,) or lengths2.shape != (N,):
        raise RuntimeError("ball_query: inconsistent shapes")
    K = int(K)
    if K < 0:
        raise RuntimeError("ball_query: K must be non-negative")
    idxs = _out((N, P1, K), dtype=torch.int64, device=dev)
    dists = _out((N, P1, K), dtype=torch.float32, device=dev)
    _call.ball_query("ball_query", dev, p1, p2, lengths1, lengths2, N, P1, P2, D, K, float(radius), idxs, dists,
                     *_scratch(dev, _lib.pointops_ball_query_workspace_bytes, N, P1, P2, D, K))
    return idxs, dists


# reference: csrc/sample_farthest_points/sample_farthest_points.h:55-76
def sample_farthest_points(points, lengths, K, start_idxs, max_K=None):
    dev = _require_gpu(points, lengths, K, start_idxs)
    points = _f32c(points, "points")
    lengths, K, start_idxs = _i64c(lengths, "lengths"), _i64c(K, "K"), _i64c(start_idxs, "start_idxs")
    if points.dim() != 3:
        raise RuntimeError("sample_farthest_points: points must be 3-dimensional")
    N, P, D = points.shape
    if lengths.shape != (N,) or K.shape != (N,) or start_idxs.shape != (N,):
        raise RuntimeError("sample_farthest_points: lengths, K and start_idxs must have shape (N,)")
    # host sync, as in the reference (sample_farthest_points.cu:132) -- unless the caller knows the maximum (an int or a
    # list K: no device-to-host read, and the call can be captured into a HIP graph)
    if max_K is None:
        max_K = int(K.max().item()) if N > 0 else 0
    max_K = int(max_K) if N > 0 else 0
    idxs = _out((N, max_K), dtype=torch.int64, device=dev)
    _call.sample_farthest_points("sample_farthest_points", dev, points, lengths, K, start_idxs, N, P, D, max_K, idxs,
                                 *_scratch(dev, _lib.pointops_fps_workspace_bytes, N, P, max_K))
    return idxs


# reference: csrc/packed_to_padded_tensor/packed_to_padded_tensor.h:78-94
def packed_to_padded(inputs_packed, first_idxs, max_size: int):
    dev = _require_gpu(inputs_packed, first_idxs)
    if inputs_packed.dim() != 2:
        raise RuntimeError("inputs_packed must be a 2-dimensional tensor")
    _contig(inputs_packed, "inputs_packed")
    _contig(first_idxs, "first_idxs")
    F, D = inputs_packed.shape
    B = first_idxs.shape[0]
    out = _out((B, max_size, D), dtype=torch.float32, device=dev)
    _call.packed_to_padded("packed_to_padded", dev, inputs_packed, first_idxs, F, B, int(max_size), D, out)
    return out


# reference: csrc/packed_to_padded_tensor/packed_to_padded_tensor.h:97-113
def padded_to_packed(inputs_padded, first_idxs, num_inputs: int):
    dev = _require_gpu(inputs_padded, first_idxs)
    if inputs_padded.dim() != 3:
        raise RuntimeError("inputs_padded must be a 3-dimensional tensor")
    _contig(inputs_padded, "inputs_padded")
    _contig(first_idxs, "first_idxs")
    B, M, D = inputs_padded.shape
    out = _out((int(num_inputs), D), dtype=torch.float32, device=dev)
    _call.padded_to_packed("padded_to_packed", dev, inputs_padded, first_idxs, int(num_inputs), B, M, D, out)
    return out


# reference: csrc/sample_pdf/sample_pdf.h:58-78 -- in place on `outputs`, returns None
def sample_pdf(bins, weights, outputs, eps: float):
    dev = _require_gpu(bins, weights, outputs)
    bins, weights = _f32c(bins, "bins"), _f32c(weights, "weights")
    _f32c(outputs, "outputs", copy=False)  # CHECK_CONTIGUOUS (sample_pdf.h:74): written in place
    batch, n_bins = weights.shape
    if bins.shape != (batch, n_bins + 1) or outputs.shape[0] != batch:
        raise RuntimeError("sample_pdf: inconsistent shapes")
    _call.sample_pdf("sample_pdf", dev, bins, weights, outputs, batch, n_bins, outputs.shape[1], float(eps))


# --- fused device half of get_point_covariances (functions/utils.py:111-153) -------
POINT_COVARIANCES_MAX_D = 8


def point_covariances(knn):
    """knn (N,P,K,D) fp32 -> cov (N,P,D,D)."""
    dev = _require_gpu(knn)
    knn = knn.contiguous()
    N, P, K, D = knn.shape
    cov = _out((N, P, D, D), dtype=torch.float32, device=dev)
    _call.point_covariances("point_covariances", dev, knn, N, P, K, D, cov)
    return cov


def point_covariances_backward(knn, grad_cov):
    dev = _require_gpu(knn, grad_cov)
    knn, grad_cov = knn.contiguous(), grad_cov.contiguous()
    N, P, K, D = knn.shape
    grad_knn = _out_like(knn)
    _call.point_covariances_backward("point_covariances_backward", dev, knn, grad_cov, N, P, K, D, grad_knn)
    return grad_knn


# --- fused local frames of functions/points_normals.py (csrc/local_frames.hip) -------
def local_frames(points, lengths, idx, disambiguate: bool):
    """points (N,P,3) fp32, lengths (N,), idx (N,P,K) -> curvatures (N,P,3), frames (N,P,3,3)."""
    dev = _require_gpu(points, lengths, idx)
    points, lengths, idx = _f32c(points, "points"), _i64c(lengths, "lengths"), _i64c(idx, "idx")
    N, P, D = points.shape
    if D != 3 or idx.dim() != 3 or idx.shape[:2] != (N, P) or lengths.shape != (N,):
        raise RuntimeError("local_frames: need points (N,P,3), lengths (N,) and idx (N,P,K)")
    curvatures = _out((N, P, 3), dtype=torch.float32, device=dev)
    frames = _out((N, P, 3, 3), dtype=torch.float32, device=dev)
    _call.local_frames("local_frames", dev, points, lengths, idx, N, P, idx.shape[2], bool(disambiguate), curvatures,
                       frames)
    return curvatures, frames


def local_frames_backward(curvatures, frames, grad_curvatures, grad_frames, lengths, disambiguate: bool):
    """-> grad_cov (N,P,3,3), the gradient of the per-point covariance (csrc/local_frames.hip)."""
    dev = _require_gpu(curvatures, frames, grad_curvatures, grad_frames, lengths)
    curvatures, frames = _f32c(curvatures, "curvatures"), _f32c(frames, "frames")
    grad_curvatures, grad_frames = _f32c(grad_curvatures, "grad_curvatures"), _f32c(grad_frames, "grad_frames")
    lengths = _i64c(lengths, "lengths")
    N, P = curvatures.shape[:2]
    if (curvatures.shape != (N, P, 3) or grad_curvatures.shape != (N, P, 3) or frames.shape != (N, P, 3, 3)
            or grad_frames.shape != (N, P, 3, 3) or lengths.shape != (N,)):
        raise RuntimeError("local_frames_backward: inconsistent shapes")
    grad_cov = _out((N, P, 3, 3), dtype=torch.float32, device=dev)
    _call.local_frames_backward("local_frames_backward", dev, curvatures, frames, grad_curvatures, grad_frames, lengths,
                                N, P, bool(disambiguate), grad_cov)
    return grad_cov


# --- fused registration of functions/points_alignment.py (csrc/points_alignment.hip) -------
POINTS_ALIGNMENT_DIMS = (2, 3)


def alignment_moment_count(D: int) -> int:
    return 3 + 4 * D + D * D


# The alignment entries take N < 65536 clouds (include/pointops_amd.h): a bigger batch goes to them in slices of this
# many clouds, each a contiguous view of the inputs and of the outputs, one after the other through one workspace.
ALIGNMENT_MAX_CLOUDS = 65535


def _cloud_slices(N: int):
    """[(slice or None, clouds)]: None = the whole batch as it is (no views made on the usual, host-bound path)."""
    if N <= ALIGNMENT_MAX_CLOUDS:
        return [(None, N)]
    return [(slice(a, min(a + ALIGNMENT_MAX_CLOUDS, N)), min(ALIGNMENT_MAX_CLOUDS, N - a))
            for a in range(0, N, ALIGNMENT_MAX_CLOUDS)]


def _rows(t, sl):
    return t if t is None or sl is None else t[sl]


def points_alignment(X, Y, idx, lengths, weights, estimate_scale: bool, allow_reflection: bool, eps: float,
                     want_moments: bool = False):
    """X (N,P,D), Y (N,P2,D) fp32, idx (N,P) int64 or None (row i of X <-> Y[n, idx[n,i]]; None: Y[n,i]), lengths
    (N,) or None, weights (N,P) or None -> R (N,D,D), T (N,D), s (N,), singular values (N,D) and, with `want_moments`,
    the fp64 moments (N, 3+4D+D*D) the backward starts from (else None)."""
    dev = _require_gpu(X, Y, idx, lengths, weights)
    X, Y, weights = _f32c(X, "X"), _f32c(Y, "Y"), _f32c(weights, "weights")
    idx, lengths = _i64c(idx, "idx"), _i64c(lengths, "lengths")
    if X.dim() != 3 or Y.dim() != 3:
        raise RuntimeError("points_alignment: X and Y must be 3-dimensional")
    N, P, D = X.shape
    P2 = Y.shape[1]
    if (Y.shape[0] != N or Y.shape[2] != D or D not in POINTS_ALIGNMENT_DIMS or (idx is None and P2 != P)
            or (idx is not None and idx.shape != (N, P)) or (lengths is not None and lengths.shape != (N,))
            or (weights is not None and weights.shape != (N, P))):
        raise RuntimeError("points_alignment: need X (N,P,D), Y (N,P2,D), D in {2,3}, idx (N,P), lengths (N,), "
                           "weights (N,P)")
    R = _out((N, D, D), dtype=torch.float32, device=dev)
    T = _out((N, D), dtype=torch.float32, device=dev)
    s = _out((N,), dtype=torch.float32, device=dev)
    sing = _out((N, D), dtype=torch.float32, device=dev)
    moments = _out((N, alignment_moment_count(D)), dtype=torch.float64, device=dev) if want_moments else None
    scratch = _scratch(dev, _lib.pointops_points_alignment_workspace_bytes, min(N, ALIGNMENT_MAX_CLOUDS), P, D)
    for sl, n in _cloud_slices(N):
        _call.points_alignment("points_alignment", dev, _rows(X, sl), _rows(Y, sl), _rows(idx, sl), _rows(lengths, sl),
                               _rows(weights, sl), n, P, P2, D, bool(estimate_scale), bool(allow_reflection),
                               float(eps), _rows(R, sl), _rows(T, sl), _rows(s, sl), _rows(moments, sl),
                               _rows(sing, sl), *scratch)
    return R, T, s, sing, moments


def points_alignment_backward(X, Y, lengths, weights, grad_moments):
    """grad_moments (N, 3+4D+D*D) fp64 -> grad_X, grad_Y (N,P,D) and grad_weights (N,P) (None without weights)."""
    dev = _require_gpu(X, Y, grad_moments, lengths, weights)
    X, Y, weights = _f32c(X, "X"), _f32c(Y, "Y"), _f32c(weights, "weights")
    lengths = _i64c(lengths, "lengths")
    N, P, D = X.shape
    if (Y.shape != X.shape or D not in POINTS_ALIGNMENT_DIMS or grad_moments.dtype != torch.float64
            or grad_moments.shape != (N, alignment_moment_count(D))):
        raise RuntimeError("points_alignment_backward: inconsistent shapes")
    grad_moments = grad_moments.contiguous()
    grad_X, grad_Y = _out_like(X), _out_like(Y)
    grad_w = _out_like(weights) if weights is not None else None
    for sl, n in _cloud_slices(N):
        _call.points_alignment_backward("points_alignment_backward", dev, _rows(X, sl), _rows(Y, sl),
                                        _rows(lengths, sl), _rows(weights, sl), _rows(grad_moments, sl), n, P, D,
                                        _rows(grad_X, sl), _rows(grad_Y, sl), _rows(grad_w, sl))
    return grad_X, grad_Y, grad_w


class IcpState:
    """Device buffers of one iterative_closest_point run and the stepping primitive over them.  The run OWNS its
    search workspace -- the grid over the target cloud `Y` is built by the first step and reused by the later ones
    (pointops_knn_points_idx_reuse) -- and never touches the grid cache above or its statistics.  `Y` and `lengths_y`
    must not be written between steps.  History entry i lives in R[i], T[i], s[i]."""

    def __init__(self, X_init, Xt, Y, lengths_x, lengths_y, max_iterations: int, estimate_scale: bool,
                 allow_reflection: bool, relative_rmse_thr: float, reuse_grid: bool = True):
        dev = _require_gpu(X_init, Xt, Y, lengths_x, lengths_y)
        self.X_init, self.Y = _f32c(X_init, "X"), _f32c(Y, "Y")
        if Xt.dtype != torch.float32 or not Xt.is_contiguous() or Xt.shape != X_init.shape \
                or Xt.data_ptr() in (self.X_init.data_ptr(), self.Y.data_ptr()):
            raise RuntimeError("icp: Xt must be a contiguous fp32 buffer of X's shape, distinct from X and Y")
        self.Xt = Xt
        self.lengths_x, self.lengths_y = _i64c(lengths_x, "lengths_x"), _i64c(lengths_y, "lengths_y")
        N, P1, D = self.X_init.shape
        P2 = self.Y.shape[1]
        if (self.Y.dim() != 3 or self.Y.shape[0] != N or self.Y.shape[2] != D or D not in POINTS_ALIGNMENT_DIMS
                or min(N, P1, P2) < 1 or self.lengths_x.shape != (N,) or self.lengths_y.shape != (N,)):
            raise RuntimeError("icp: need X (N,P1,D), Y (N,P2,D) with N, P1, P2 >= 1, D in {2,3} and lengths (N,)")
        self.dev, self.shape = dev, (N, P1, P2, D)
        self.flags = (bool(estimate_scale), bool(allow_reflection))
        self.thr = float(relative_rmse_thr)
        self.steps = 0
        self.searched = False  # the search workspace holds a grid over Y
        self.R = _out((max_iterations, N, D, D), dtype=torch.float32, device=dev)
        self.T = _out((max_iterations, N, D), dtype=torch.float32, device=dev)
        self.s = _out((max_iterations, N), dtype=torch.float32, device=dev)
        self.idx = _out((N, P1), dtype=torch.int64, device=dev)
        self.dists = _out((N, P1), dtype=torch.float32, device=dev)
        self.rmse = _out((N,), dtype=torch.float32, device=dev)  # (read only from the second step on: `first`)
        self.converged = _out((1,), dtype=torch.int32, device=dev)
        self.knn_ws, self.knn_ws_bytes = _scratch(dev, _lib.pointops_knn_workspace_bytes, N, P1, P2, D, 1, -1)
        self.ws, self.ws_bytes = _scratch(dev, _lib.pointops_icp_workspace_bytes, N, P1, D)
        self.uses_grid = bool(_lib.pointops_knn_uses_grid(N, P1, P2, D, 1, -1))
        self.reuse_grid = bool(reuse_grid) and self.uses_grid

    def step(self, search: bool = True) -> None:
        """Enqueue one iteration (no synchronisation).  `search=False`: align to the neighbour table already in
        `self.idx` (diagnostics and benchmarks)."""
        N, P1, P2, D = self.shape
        i = self.steps
        if i >= self.R.shape[0]:
            raise RuntimeError("icp: more steps than max_iterations")
        reuse = -1 if not search else (1 if (self.reuse_grid and self.searched) else 0)
        _call.icp_iteration("icp_iteration", self.dev, self.X_init, self.Xt, self.Y, self.lengths_x, self.lengths_y, N,
                            P1, P2, D, self.flags[0], self.flags[1], i == 0, reuse, self.thr, self.idx, self.dists,
                            self.R[i], self.T[i], self.s[i], self.rmse, self.converged, self.knn_ws, self.knn_ws_bytes,
                            self.ws, self.ws_bytes)
        self.searched = self.searched or search
        self.steps = i + 1


# --- device halves of knn_gather / masked_gather (functions/knn.py:200-250) -------
def gather_neighbors(x, idx, lengths=None):
    dev = _require_gpu(x, idx, lengths)
    x, idx, lengths = _f32c(x, "x"), _i64c(idx, "idx"), _i64c(lengths, "lengths")
    N, M, U = x.shape
    _, L, K = idx.shape
    out = _out((N, L, K, U), dtype=torch.float32, device=dev)
    _call.gather_neighbors("gather_neighbors", dev, x, idx, lengths, N, M, U, L, K, out)
    return out


def gather_neighbors_backward(grad_out, idx, lengths, M: int, deterministic: bool = False):
    dev = _require_gpu(grad_out, idx, lengths)
    grad_out, idx, lengths = _f32c(grad_out, "grad_out"), _i64c(idx, "idx"), _i64c(lengths, "lengths")
    N, L, K, U = grad_out.shape
    grad_x = _out((N, M, U), dtype=torch.float32, device=dev)
    if deterministic:  # inverted neighbour table: every row of x sums its addends in table order
        entry, what = _call.gather_neighbors_backward_det, "gather_neighbors_backward(deterministic)"
        scratch = _scratch(dev, _lib.pointops_backward_det_workspace_bytes, N, L, K, M)
    else:
        entry, what, scratch = _call.gather_neighbors_backward, "gather_neighbors_backward", ()
    entry(what, dev, grad_out, idx, lengths, N, M, U, L, K, grad_x, *scratch)
    return grad_x


def chamfer_reduce(dists, lengths, weights, mean: bool):
    """dists (N,P) fp32 -> (N,) per-cloud masked sum [* weights] [/ max(len,1)]."""
    dev = _require_gpu(dists, lengths, weights)
    dists, lengths, weights = _f32c(dists, "dists"), _i64c(lengths, "lengths"), _f32c(weights, "weights")
    N, P = dists.shape
    if lengths.shape != (N,) or (weights is not None and weights.shape != (N,)):
        raise RuntimeError("chamfer_reduce: lengths / weights must have shape (N,)")
    out = _out((N,), dtype=torch.float32, device=dev)
    _call.chamfer_reduce("chamfer_reduce", dev, dists, lengths, weights, N, P, bool(mean), out)
    return out


# --- fused single-direction chamfer terms (functions/chamfer.py:135-185) --------------------
CHAMFER_MAX_FEATURES = 4
CHAMFER_MAX_CHANNELS = 16


class _HostPointers(ctypes.c_void_p * (1 + CHAMFER_MAX_FEATURES)):
    """HOST array of device pointers (one per feature tensor, or per output: 1 + F), as the chamfer entries take them;
    data_ptr() lets it stand where a tensor stands in a native call."""

    def data_ptr(self):
        return ctypes.addressof(self)


class _HostChannels(ctypes.c_int64 * CHAMFER_MAX_FEATURES):
    def data_ptr(self):
        return ctypes.addressof(self)


def _ptr_array(tensors):
    arr = _HostPointers()  # (null pointers)
    for i, t in enumerate(tensors):
        if t is not None:
            arr[i] = t.data_ptr()
    return arr


def _feature_args(x_feats, y_feats):
    """The `F, x_feats, y_feats, C` of every chamfer entry, from feature lists _check_chamfer_shapes has passed."""
    return len(x_feats), _ptr_array(x_feats), _ptr_array(y_feats), _HostChannels(*[t.shape[2] for t in x_feats])


def _f32c_list(tensors, name):
    return [_f32c(t, name) for t in tensors]


def _check_chamfer_shapes(N, P1, P2, idx, x_lengths, y_lengths, weights, x_feats, y_feats):
    """The shape check of all four chamfer wrappers (`idx`: the (N, P1) neighbour table, None where a call has none)."""
    if len(x_feats) != len(y_feats) or len(x_feats) > CHAMFER_MAX_FEATURES:
        raise RuntimeError(f"chamfer: at most {CHAMFER_MAX_FEATURES} feature pairs")
    if (idx is not None and idx.shape != (N, P1)) or x_lengths.shape != (N,) or y_lengths.shape != (N,):
        raise RuntimeError("chamfer: idx must be (N, P1) and the lengths (N,)")
    if weights is not None and weights.shape != (N,):
        raise RuntimeError("chamfer: weights must have shape (N,)")
    for a, b in zip(x_feats, y_feats):
        if a.dim() != 3 or b.dim() != 3 or a.shape[:2] != (N, P1) or b.shape[:2] != (N, P2) \
                or a.shape[2] != b.shape[2] or not 1 <= a.shape[2] <= CHAMFER_MAX_CHANNELS:
            raise RuntimeError("chamfer: features must be (N, P1, C) / (N, P2, C) with 1 <= C <= "
                               f"{CHAMFER_MAX_CHANNELS}")


def chamfer_forward(dists, idx, x_lengths, y_lengths, weights, x_feats, y_feats, abs_cosine: bool, mean: bool):
    """dists (N,P1) fp32 and idx (N,P1) int64 of the K=1 search -> out (1+F, N): row 0 the point term,
    row 1+f the cosine term of feature f, each already weighted and (for "mean") length-normalised."""
    dev = _require_gpu(dists, idx, x_lengths, y_lengths, weights, *x_feats, *y_feats)
    dists, idx, weights = _f32c(dists, "dists"), _i64c(idx, "idx"), _f32c(weights, "weights")
    x_lengths, y_lengths = _i64c(x_lengths, "x_lengths"), _i64c(y_lengths, "y_lengths")
    x_feats, y_feats = _f32c_list(x_feats, "x_feats"), _f32c_list(y_feats, "y_feats")
    N, P1 = dists.shape
    F = len(x_feats)
    P2 = y_feats[0].shape[1] if F else 0
    _check_chamfer_shapes(N, P1, P2, idx, x_lengths, y_lengths, weights, x_feats, y_feats)
    out = _out((1 + F, N), dtype=torch.float32, device=dev)
    _call.chamfer_forward("chamfer_forward", dev, dists, idx, x_lengths, y_lengths, weights, N, P1, P2,
                          *_feature_args(x_feats, y_feats), bool(abs_cosine), bool(mean), out,
                          *_scratch(dev, _lib.pointops_chamfer_workspace_bytes, N, P1))
    return out


def chamfer_backward(x, y, idx, x_lengths, y_lengths, weights, grad_out, norm: int, x_feats, y_feats,
                     abs_cosine: bool, mean: bool, into=None):
    """Closed-form gradients of chamfer_forward's outputs: returns (grad_x, grad_y, [grad_x_feat], [grad_y_feat]).
    `into` = (grad_x, grad_y, [grad_x_feat], [grad_y_feat]) buffers that already hold gradients (the other direction's,
    roles swapped): the gradients are ADDED to them (pointops_chamfer_backward_accumulate) and they are returned."""
    dev = _require_gpu(x, y, idx, grad_out, x_lengths, y_lengths, weights, *x_feats, *y_feats)
    x, y, grad_out, weights = _f32c(x, "x"), _f32c(y, "y"), _f32c(grad_out, "grad_out"), _f32c(weights, "weights")
    idx, x_lengths, y_lengths = _i64c(idx, "idx"), _i64c(x_lengths, "x_lengths"), _i64c(y_lengths, "y_lengths")
    x_feats, y_feats = _f32c_list(x_feats, "x_feats"), _f32c_list(y_feats, "y_feats")
    N, P1, D = x.shape
    P2 = y.shape[1]
    F = len(x_feats)
    if y.shape[0] != N or y.shape[2] != D or grad_out.shape != (1 + F, N):
        raise RuntimeError("chamfer_backward: inconsistent shapes")
    _check_chamfer_shapes(N, P1, P2, idx, x_lengths, y_lengths, weights, x_feats, y_feats)
    if into is None:
        grad_x, grad_y = _out_like(x), _out_like(y)
        gxf, gyf = [_out_like(t) for t in x_feats], [_out_like(t) for t in y_feats]
        entry = _call.chamfer_backward
    else:
        grad_x, grad_y, gxf, gyf = into
        gxf, gyf = list(gxf), list(gyf)
        for g, like in zip([grad_x, grad_y, *gxf, *gyf], [x, y, *x_feats, *y_feats]):
            if (g.shape != like.shape or g.dtype != torch.float32 or not g.is_contiguous()
                    or g.device != like.device):
                raise RuntimeError("chamfer_backward: `into` buffers must match the inputs (fp32, contiguous)")
        entry = _call.chamfer_backward_accumulate
    entry("chamfer_backward", dev, x, y, idx, x_lengths, y_lengths, weights, grad_out, N, P1, P2, D, int(norm),
          *_feature_args(x_feats, y_feats), bool(abs_cosine), bool(mean), grad_x, grad_y, _ptr_array(gxf),
          _ptr_array(gyf))
    return grad_x, grad_y, gxf, gyf


_BATCH_REDUCTION = {None: 0, "mean": 1, "sum": 2}


def chamfer_pair_forward(x, y, x_lengths, y_lengths, norm: int, x_feats, y_feats, abs_cosine: bool, mean: bool,
                         batch_reduction):
    """Both directions of an unweighted chamfer distance in ONE native call (pointops_chamfer_pair_forward):
    returns (outs, idx_xy (N,P1), idx_yx (N,P2)); outs = 1+F tensors, () after a batch reduction, (N,) without one."""
    dev = _require_gpu(x, y, x_lengths, y_lengths, *x_feats, *y_feats)
    x, y = _f32c(x, "x"), _f32c(y, "y")
    x_lengths, y_lengths = _i64c(x_lengths, "x_lengths"), _i64c(y_lengths, "y_lengths")
    x_feats, y_feats = _f32c_list(x_feats, "x_feats"), _f32c_list(y_feats, "y_feats")
    if norm not in (1, 2):
        raise ValueError("Support for 1 or 2 norm.")
    N, P1, D = x.shape
    P2 = y.shape[1]
    F = len(x_feats)
    if y.shape[0] != N or y.shape[2] != D:
        raise RuntimeError("chamfer_pair_forward: inconsistent shapes")
    _check_chamfer_shapes(N, P1, P2, None, x_lengths, y_lengths, None, x_feats, y_feats)
    red = _BATCH_REDUCTION[batch_reduction]
    idx_xy = _out((N, P1), dtype=torch.int64, device=dev)
    idx_yx = _out((N, P2), dtype=torch.int64, device=dev)
    outs = [_out(() if red else (N,), dtype=torch.float32, device=dev) for _ in range(1 + F)]
    _call.chamfer_pair_forward("chamfer_pair_forward", dev, x, y, x_lengths, y_lengths, N, P1, P2, D, int(norm),
                               *_feature_args(x_feats, y_feats), bool(abs_cosine), bool(mean), red, idx_xy, idx_yx,
                               _ptr_array(outs),
                               *_scratch(dev, _lib.pointops_chamfer_pair_workspace_bytes, N, P1, P2, D, F))
    return outs, idx_xy, idx_yx


def chamfer_pair_backward(x, y, idx_xy, idx_yx, x_lengths, y_lengths, grads, norm: int, x_feats, y_feats,
                          abs_cosine: bool, mean: bool, batch_reduction):
    """Gradients of chamfer_pair_forward's 1+F outputs (`grads`: one tensor or None per output) in ONE native call:
    returns (grad_x, grad_y, [grad_x_feat], [grad_y_feat])."""
    dev = _require_gpu(x, y, idx_xy, idx_yx, x_lengths, y_lengths, *grads, *x_feats, *y_feats)
    x, y, idx_xy, idx_yx = _f32c(x, "x"), _f32c(y, "y"), _i64c(idx_xy, "idx_xy"), _i64c(idx_yx, "idx_yx")
    x_lengths, y_lengths = _i64c(x_lengths, "x_lengths"), _i64c(y_lengths, "y_lengths")
    x_feats, y_feats, grads = _f32c_list(x_feats, "x_feats"), _f32c_list(y_feats, "y_feats"), _f32c_list(grads, "grad")
    N, P1, D = x.shape
    P2 = y.shape[1]
    F = len(x_feats)
    red = _BATCH_REDUCTION[batch_reduction]
    want = () if red else (N,)
    if len(grads) != 1 + F or any(g is not None and g.shape != want for g in grads):
        raise RuntimeError("chamfer_pair_backward: one gradient per output, () after a batch reduction, (N,) without")
    if y.shape[0] != N or y.shape[2] != D or idx_yx.shape != (N, P2):
        raise RuntimeError("chamfer_pair_backward: inconsistent shapes")
    _check_chamfer_shapes(N, P1, P2, idx_xy, x_lengths, y_lengths, None, x_feats, y_feats)
    grad_x, grad_y = _out_like(x), _out_like(y)
    gxf, gyf = [_out_like(t) for t in x_feats], [_out_like(t) for t in y_feats]
    _call.chamfer_pair_backward("chamfer_pair_backward", dev, x, y, idx_xy, idx_yx, x_lengths, y_lengths,
                                _ptr_array(grads), N, P1, P2, D, int(norm), *_feature_args(x_feats, y_feats),
                                bool(abs_cosine), bool(mean), red, grad_x, grad_y, _ptr_array(gxf), _ptr_array(gyf),
                                *_scratch(dev, _lib.pointops_chamfer_pair_backward_workspace_bytes, N, F))
    return grad_x, grad_y, gxf, gyf
