"""The template instances of the search kernels and the inputs that run each of them at its bucket edges, written once
for tests/test_search_instances_cpu.py (which certifies the inputs with the oracle alone) and
tests/test_search_instances_gpu.py (which runs the kernels on them).

csrc/dispatch.h maps a runtime K to the smallest listed capacity KC >= K (with_bucket) and D, the norm and the
workgroup size to a listed instance or a fallback (with_exact).  The value lists below are copies of the lists in the
source; the CPU test reads the source as text and compares.  The K lists hold every bucket's last value, the first value
of the next bucket and, where the bucket is wide enough, a value strictly inside: K < KC is where a list of KC slots of
which only K count, the K-th gate, the row write and the merge of partial lists can go wrong unnoticed.

A batch is ragged, 6 clouds and a seventh that starts the pattern again (the 256-lane geometries repeat it over 1024 and
2048 clouds):
    lengths2 = P2, KC + 1, K + 1, K, K - 1, 0   clamped to [0, P2]; a value that repeats becomes 1, then KC
    lengths1 = P1, 1, P1 - 1, 0, P1, 65
Rows past a length hold 9.0 (coordinates lie in [0, 1]): a kernel that reads them gets wrong neighbours, not silence.
The full cloud is a lattice, coordinates {0..4} * 0.25: the K-th and (K+1)-th candidates tie exactly for some queries
and a == b happens per coordinate; the other clouds are uniform, the seventh -- full on both sides -- among them, so
that lists of K out of KC slots also meet a long cloud without ties (every second full cloud of the big batches).  Ball-query batches draw the lattice coordinate with
weights (.05, .1, .7, .1, .05) -- the centre site alone then holds more than 100 of the 700 points at every D <= 5, so a
row with more than K points inside exists for every K of the list -- and run at the radii 0.26 and 0.5: 0.5 * 0.5 is the
squared distance of two lattice steps exactly (strict <), 0.26 leaves rows partly and all -1.

COUNTS (asserted by the CPU test against what the generators yield) -- instances: the distinct kernel template
instances the calls reach; calls: the (D, norm, K) or (D, K, radius) cases, each run under every knob of its family.

    family          instances  calls   what
    scan64                112    288   knn_reg_kernel<D, KC, NORM>, 64 lanes, S = 1
    sliced            112 + 7    288   the same with S = 4..8 slices, knn_merge_kernel<KC>
    scan256                16     16   the same kernel with 256 lanes: one K per (D, norm), rotating through the buckets
    small_q1              112    288   knn_small_kernel<D, KC, NORM, 1>
    small_q2               32     32   knn_small_kernel<D, KC, NORM, 4>: KC <= 2 only
    small_gated_q1        112    288   the same two on clouds long enough for the gates to be refreshed
    small_gated_q2         32     32
    wide64                 10     64   knn_wide_kernel<KC, NORM, 64>, S = 1, D = 9 and 33
    wide64_sliced      10 + 5     64   the same with S >= 2, knn_merge_kernel<KC>
    wide256                10     20   knn_wide_kernel<KC, NORM, 256>
    wide_long               2     12   knn_wide_kernel<64, NORM, 64>: K = 33, 48, 64
    wide_lds                2      8   knn_wide_kernel<0, NORM, 64>: K = 65, 100
    grid                   48    108   grid_search<D, .>(KC, NORM) for KC <= 64 and the wave sort above (6 instances)
    ball_scan               5    140   ball_query_kernel<1..4 | runtime D>, two radii per (D, K)
    ball_small              5    140   ball_small_kernel<1..4 | runtime D>
    ball_grid              12     72   ball_grid_lane_kernel<D, KC>, leftovers to the list or the scan kernel
    ball_list               3     72   ball_query_list_kernel<D> (K % 4 == 0) or the scan kernel over query lists
"""
import functools
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pytorch3d_pointops_amd", "csrc")


def source(name):
    return open(os.path.join(CSRC, name)).read()


def constant(text, name):
    """The value of `constexpr T name = a * b;` in the source text."""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9*\s]+);", text)
    assert m, f"no constant {name}"
    value = 1
    for f in m.group(1).split("*"):
        value *= int(f)
    return value

# ------------------------------------------------------------------ the lists of the source (see the CPU test)
SCAN_D = (1, 2, 3, 4, 5, 6, 7, 8)  # kScanD (knn_grid.h)
SCAN_KC = (1, 2, 4, 8, 16, 24, 32)  # kScanKC (knn_grid.h)
WIDE_KC = (4, 8, 16, 24, 32)  # launch_knn_wide (knn_wide.hip)
WIDE_WG = (64, 256)  # Ints<64> with the fallback 256
GRID_KC = (1, 2, 4, 8, 16, 32, 64)  # kGridKC (knn_grid_search.h)
GRID_D = (1, 2, 3)  # knn_grid.hip, knn_grid_wsort.hip
BALL_D = (1, 2, 3, 4)  # ball_query_kernel / ball_small_kernel; any other D takes the runtime-D instance <0>
BALL_LIST_D = (1, 2, 3)  # ball_query_list_kernel, ball_grid_lane_kernel, ball_order_kernel
BALL_GRID_KC = (8, 16, 32, 64)  # ball_grid_lane_kernel (ball_grid.hip)
NORMS = (1, 2)

# ------------------------------------------------------------------ the K values of the matrix
# (12, 20, 28 and the grid's 12, 24, 48: multiples of 4 below their capacity -- the only K < KC whose rows leave in
# 16-byte stores, write_row's vec16 path)
REG_K = (1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32)
GRID_K = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 24, 32, 33, 48, 64, 65, 100, 128)
BALL_K = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100)
WIDE_D = (9, 33)  # no register-scan instance: D = 9 is the first such D, 33 leaves a partial row of 4 per LDS line
WIDE_K = REG_K[2:]  # from 3 upwards: the first wide bucket is 4
LONG_K = (33, 48, 64)  # 64-slot register lists fed by an LDS queue
LDS_K = (65, 100)  # lists in LDS
ROTATING_K = (1, 2, 3, 5, 12, 21, 29)  # one K per bucket of SCAN_KC, below the capacity wherever the bucket allows (12: a
# row of 16-byte stores)
WIDE256_K = ROTATING_K[2:]
BALL_RADII = (0.26, 0.5)
PAD = np.float32(9.0)


def bucket(K, caps):
    """with_bucket of csrc/dispatch.h: the smallest listed capacity >= K, else the last one; K itself without a list."""
    return next((c for c in caps if K <= c), caps[-1]) if caps else K


def lengths2(K, KC, P2):
    raw = [min(max(v, 0), P2) for v in (P2, KC + 1, K + 1, K, K - 1, 0)]
    spare = [v for v in (1, KC) if v not in raw and v <= P2]
    out = []
    for v in raw:
        if v in out and spare:
            v = spare.pop(0)
        out.append(v)
    return out


def lengths1(P1):
    return [P1, 1, P1 - 1, 0, P1, min(65, P1)]


# geometry: (N, P1, P2(D, KC)) -- the smallest sizes that reach the path
#   few     N ceil(P1 / 64) = 21 waves: the wave-per-query kernels by default, 64-lane workgroups, P2 < 512: one slice
#   sliced  P2 in [512, 1024]: knn_split_count gives min(8, P2 / 128) = 4..8 slices; short clouds leave slices empty
#   many    N ceil(P1 / 256) = 2048: 256-lane workgroups (the second tile of a cloud holds one query); P2 just above KC
#   grid    one cloud of 3000 points per side, five short ones
#   long    the full cloud is longer than max(512, 128 K) candidates: knn_small_kernel refreshes its wave-uniform gates
#           (kth_head_bits<KC>(., K)) at least once, and on the lattice most later candidates tie with the gate
#   edge256 2048 clouds of two queries: 256-lane workgroups of knn_wide_kernel, so D * 256 * 4 bytes of LDS
GEOMETRY = {
    "few": (7, 131, lambda D, KC: 333),
    "sliced": (7, 131, lambda D, KC: 512 + 64 * (D % 9)),
    "many": (1024, 257, lambda D, KC: KC + 8),
    "grid": (7, 3000, lambda D, KC: 3000),
    "ball": (7, 131, lambda D, KC: 700),
    "long": (7, 131, lambda D, KC: max(128 * KC, 512) + 261),
    "edge256": (2048, 2, lambda D, KC: KC + 8),
}
_SEED = {name: i for i, name in enumerate(sorted(GEOMETRY))}


def _fill(rng, N, P, D, lengths, weights=None):
    pts = rng.random((N, P, D), dtype=np.float32)
    for n in range(0, N, 12):  # the full cloud of every second group of six: the lattice
        pts[n] = (rng.choice(5, size=(P, D), p=weights).astype(np.float32) * np.float32(0.25))
    for n in range(N):
        pts[n, lengths[n]:] = PAD
    return pts


@functools.lru_cache(maxsize=64)
def batch(geometry, D, K, caps):
    """dict(p1, p2, l1, l2, KC) of one (geometry, D, K); `caps`: the capacity list of the family (() = none).  Read-only
    and cached: the oracle's answer is computed once per batch and shared."""
    N, P1, p2_of = GEOMETRY[geometry]
    KC = bucket(K, caps)
    P2 = p2_of(D, KC)
    rng = np.random.default_rng([20240 + _SEED[geometry], D, K])
    l1 = np.array([lengths1(P1)[n % 6] for n in range(N)])  # (N > 6: the pattern repeats)
    l2 = np.array([lengths2(K, KC, P2)[n % 6] for n in range(N)])
    weights = (0.05, 0.1, 0.7, 0.1, 0.05) if geometry == "ball" else None
    out = dict(p1=_fill(rng, N, P1, D, l1, weights), p2=_fill(rng, N, P2, D, l2, weights), l1=l1, l2=l2, KC=KC)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def self_batch(D, K):
    """The grid batch as a self-query: the target cloud and its lengths on both sides."""
    b = batch("grid", D, K, GRID_KC)
    return dict(p1=b["p2"], p2=b["p2"], l1=b["l2"], l2=b["l2"], KC=b["KC"])


# ------------------------------------------------------------------ the KNN families
# name: (geometry, POINTOPS_DEBUG, version, family of the plan, slices: 1 | "many", D list, capacity list)
KNN = {
    "scan64": ("few", "knn_small=0", 2, "scan", 1, SCAN_D, SCAN_KC),
    "sliced": ("sliced", "knn_small=0", 2, "scan", "many", SCAN_D, SCAN_KC),
    "scan256": ("many", "knn_small=0", 2, "scan", 1, SCAN_D, SCAN_KC),
    "small_q1": ("few", "knn_small=1,knn_small_q=1", 2, "small", 1, SCAN_D, SCAN_KC),
    "small_q2": ("few", "knn_small=1,knn_small_q=2", 2, "small", 1, SCAN_D, SCAN_KC),
    "small_gated_q1": ("long", "knn_small=1,knn_small_q=1", 2, "small", 1, SCAN_D, SCAN_KC),
    "small_gated_q2": ("long", "knn_small=1,knn_small_q=2", 2, "small", 1, SCAN_D, SCAN_KC),
    "wide64": ("few", "", 0, "wide", 1, WIDE_D, WIDE_KC),
    "wide64_sliced": ("sliced", "", 0, "wide", "many", WIDE_D, WIDE_KC),
    "wide256": ("many", "", 0, "wide", 1, WIDE_D, WIDE_KC),
    "wide_long": ("few", "", 0, "wide", 1, WIDE_D, (64,)),
    "wide_lds": ("few", "", 0, "wide", 1, WIDE_D, ()),
    "grid": ("grid", "", 3, "grid", 1, GRID_D, GRID_KC),
}


def knn_ks(family, D, norm):
    """The K values one (family, D, norm) runs."""
    if family == "scan256":  # the oracle on 1024 clouds costs about a second: one K, every bucket for some D
        return (ROTATING_K[(2 * (D - 1) + norm - 1) % len(ROTATING_K)],)
    return {"small_q2": (1, 2), "small_gated_q2": (1, 2), "wide64": WIDE_K, "wide64_sliced": WIDE_K, "wide256": WIDE256_K, "wide_long": LONG_K,
            "wide_lds": LDS_K, "grid": GRID_K}.get(family, REG_K)


def knn_calls(family):
    """[(D, norm, K)] of a family."""
    return [(D, norm, K) for D in KNN[family][5] for norm in NORMS for K in knn_ks(family, D, norm)]


def knn_instances(family):
    """The distinct template instances the calls of a family reach, as (D or 0, KC, norm) (wide: D is a runtime value)."""
    caps = KNN[family][6]
    wide = family.startswith("wide")
    return {(0 if wide else D, 0 if family == "wide_lds" else bucket(K, caps), norm) for D, norm, K in knn_calls(family)}


def merge_instances(family):
    return {bucket(K, KNN[family][6]) for _, _, K in knn_calls(family)}


def grid_instances():
    """(D, KC, norm) of the list searches, KC = 0 for the wave sort above 64."""
    return {(D, 0 if K > 64 else bucket(K, GRID_KC), norm) for D, norm, K in knn_calls("grid")}


# (version asked for, D, K, family of the automatic choice it falls through to) on the few-queries geometry
FALL_THROUGH = ((1, 9, 8, "wide"), (2, 9, 8, "wide"), (1, 3, 33, "wide"), (2, 3, 33, "wide"), (3, 4, 8, "small"),
                (3, 3, 129, "wide"))


# ------------------------------------------------------------------ the ball-query families
# name: (knobs, D list, K list)
BALL = {
    "ball_scan": (("ball_small=0,ball_grid=0",), (1, 2, 3, 4, 5), BALL_K),
    "ball_small": (("ball_small=1,ball_grid=0",), (1, 2, 3, 4, 5), BALL_K),
    # factor 0: every cloud through its grid, leftovers to the list kernel (ball_stage=1, K % 4 == 0) or the scan
    "ball_grid": (tuple(f"ball_grid=1,ball_factor=0,ball_stage={s},ball_order={o}" for s in (0, 1) for o in (0, 1)),
                  BALL_LIST_D, tuple(K for K in BALL_K if K <= 64)),
    # factor 1e30: the device sends every cloud to the scan, every query through the lists
    "ball_list": (tuple(f"ball_grid=1,ball_factor=1e30,ball_stage={s},ball_order={o}" for s in (0, 1) for o in (0, 1)),
                  BALL_LIST_D, tuple(K for K in BALL_K if K <= 64)),
}


BALL_IDS = [(family, D) for family in sorted(BALL) for D in BALL[family][1]]


def ball_calls(family):
    """[(D, K, radius)]: each is run under every knob of the family and compared with the oracle once per distinct
    result (the knobs never change results)."""
    _, Ds, Ks = BALL[family]
    return [(D, K, r) for D in Ds for K in Ks for r in BALL_RADII]


def ball_batch(D, K):
    return batch("ball", D, K, BALL_GRID_KC if K <= 64 else ())


def ball_instances(family):
    _, Ds, Ks = BALL[family]
    if family == "ball_grid":
        return {(D, bucket(K, BALL_GRID_KC)) for D in Ds for K in Ks}
    return {D if D in (BALL_D if family in ("ball_scan", "ball_small") else BALL_LIST_D) else 0 for D in Ds}


# ------------------------------------------------------------------ the LDS budgets of knn_wide_supported
def wide_budget_edges(lds_max=None, long_kc=None, long_queue=None):
    """[(D, K, inside)] (by default from the constants as knn_wide.hip has them now): the last shape inside each LDS budget of knn_wide_supported and the first outside it, from the
    constants of knn_wide.hip (register lists: D * 256 * 4 bytes; long lists: (D * 4 + queue * 8) * 64; LDS lists:
    (D * 4 + K * 8) * 64; each at most lds_max - 1024)."""
    if lds_max is None:
        text = source("knn_wide.hip")
        lds_max, long_kc, long_queue = (constant(text, n) for n in ("kWideLdsMax", "kLongKC", "kLongQueue"))
    room = lds_max - 1024
    d_reg = room // (256 * 4)
    d_long = (room // 64 - long_queue * 8) // 4
    k_lds = (room // 64 - 3 * 4) // 8
    assert k_lds > long_kc
    return [(d_reg, 4, True), (d_reg + 1, 4, False), (d_long, 40, True), (d_long + 1, 40, False), (3, k_lds, True),
            (3, k_lds + 1, False)]


def edge_batch_of(K):
    """(geometry, capacity list) of the batch that runs a budget edge: register lists take the 256-lane workgroups,
    whose LDS the budget is written for."""
    return ("edge256", WIDE_KC) if K <= 32 else ("few", (64,) if K <= 64 else ())


COUNTS = {  # family: (instances, calls) -- the table of the docstring
    "scan64": (112, 288), "sliced": (112 + 7, 288), "scan256": (16, 16), "small_q1": (112, 288), "small_q2": (32, 32),
    "small_gated_q1": (112, 288), "small_gated_q2": (32, 32), "wide64": (10, 64), "wide64_sliced": (10 + 5, 64), "wide256": (10, 20), "wide_long": (2, 12), "wide_lds": (2, 8),
    "grid": (48, 108), "ball_scan": (5, 140), "ball_small": (5, 140), "ball_grid": (12, 72), "ball_list": (3, 72),
}
