"""Coordinate frames for the search kernels' tests (test_coordinate_frames_cpu.py, test_coordinate_frames_gpu.py and
the frame fuzz of test_fuzz_grid_gpu.py).  A frame maps a base cloud pair (p1, p2) to a transformed pair; the SAME map
goes over both clouds of a call.

EXACT frames change every a[d] - b[d] by an exact factor (+-1 or 2^k), so the reference's own arithmetic -- fp32
differences, products and sums, unfused -- gives the same neighbours and the same distances up to that exact factor:
  shift t      x -> x + t, accepted only when x + t is representable for every coordinate (`shift_exact`),
  negation     x -> -x on all or some axes (a lattice's 0.0 becomes -0.0 and is kept),
  scale 2^k    x -> x 2^k, accepted only when no squared difference leaves the normal range (`scale_exact`),
and compositions, applied as scale(negate(shift(x))).
INEXACT frames (offsets that round, per-axis scales, magnitudes 1e18 / 1e-18, a constant negative axis, clouds of
opposite sign, a far outlier) re-round the differences: their results are compared with the reference semantics on
the SAME transformed inputs, never with the untransformed call.  Every input stays finite and no squared distance
overflows (`assert_finite_frame`); NaN / inf stay unpinned."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)  # 2^-126
FLT_MAX = float(np.finfo(np.float32).max)


def quantise(x, bits=24):
    """Round to multiples of 2^-bits (values of order one stay fp32): bases whose values do not sit on a grid
    (powers of uniforms, gaussian blobs) are put on one before they are shifted."""
    s = float(2 ** bits)
    return (np.round(np.asarray(x, np.float64) * s) / s).astype(np.float32)


def quantum(*arrays):
    """Largest power of two that divides every coordinate of the arrays (float; 1.0 for all-zero input)."""
    e_min = None
    for x in arrays:
        v = np.asarray(x, np.float32).ravel()
        v = v[v != 0]
        if v.size == 0:
            continue
        m, e = np.frexp(v.astype(np.float64))  # v = m 2^e, 0.5 <= |m| < 1; m 2^53 is an integer
        mi = np.abs(m * float(2 ** 53)).astype(np.int64)
        tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
        lo = int((e.astype(np.int64) - 53 + tz).min())
        e_min = lo if e_min is None else min(e_min, lo)
    return 1.0 if e_min is None else float(2.0 ** e_min)


def shift_exact(x, t):
    """x + t as fp32, or ValueError when some coordinate of x + t is not representable (the shift would re-round
    differences and the frame would not be exact)."""
    y = np.asarray(x, np.float32).astype(np.float64) + np.asarray(t, np.float64)
    y32 = y.astype(np.float32)
    if not np.array_equal(y32.astype(np.float64), y):
        raise ValueError(f"shift by {t} is not exact for this cloud")
    return y32


def scale_exact(arrays, k):
    """[x 2^k for x in arrays], or ValueError unless, in float64, 4^k (smallest nonzero squared difference) >= FLT_MIN
    and 4^k (largest sum of squared differences) <= FLT_MAX: every fp32 difference, square, sum (and the L1 terms,
    which lie between) then scales by an exact power of two.  The smallest nonzero |difference| is bounded by the
    coordinates' common quantum, the largest by the joint extent."""
    arrays = [np.asarray(x, np.float32) for x in arrays]
    q = quantum(*arrays)
    D = arrays[0].shape[-1]
    lo = np.min([x.reshape(-1, D).min(0) for x in arrays if x.size], axis=0).astype(np.float64)
    hi = np.max([x.reshape(-1, D).max(0) for x in arrays if x.size], axis=0).astype(np.float64)
    amax = max(float(np.abs(x).max()) for x in arrays if x.size)
    f = 4.0 ** k
    if not (f * q * q >= FLT_MIN):
        raise ValueError(f"scale 2^{k}: squared differences of quantum {q} would leave the normal range")
    if not (f * float(((hi - lo) ** 2).sum()) <= FLT_MAX and (2.0 ** k) * amax <= FLT_MAX):
        raise ValueError(f"scale 2^{k}: squared distances would overflow")
    s = np.float32(2.0 ** k)
    out = [(x * s).astype(np.float32) for x in arrays]
    for x, y in zip(arrays, out):
        assert np.array_equal(y.astype(np.float64), x.astype(np.float64) * 2.0 ** k)
    return out


def assert_finite_frame(arrays):
    """Every coordinate finite and, in float64, the largest possible squared distance below FLT_MAX."""
    arrays = [np.asarray(x, np.float32) for x in arrays if np.asarray(x).size]
    D = arrays[0].shape[-1]
    assert all(np.isfinite(x).all() for x in arrays)
    lo = np.min([x.reshape(-1, D).min(0) for x in arrays], axis=0).astype(np.float64)
    hi = np.max([x.reshape(-1, D).max(0) for x in arrays], axis=0).astype(np.float64)
    assert float(((hi - lo) ** 2).sum()) < FLT_MAX, "a squared distance could overflow"


class Frame:
    """name, family ("shift" | "neg" | "scale" | "compose" | "inexact") and the map itself.
    Exact frames: x -> 2^k * sign * (x + t); `sign` (per axis, +-1), `k` and `t` describe what the results must do."""

    def __init__(self, name, family, t=0.0, neg=(), k=0, fn=None, needs_pair=False, lattice_only=False,
                 rscale=1.0):
        self.name, self.family, self.t, self.k, self.fn = name, family, t, k, fn
        self.neg = neg if neg == "all" else tuple(neg)  # "all" or the negated axes (clamped to the last axis)
        self.rscale = rscale  # inexact frames: what a ball_query radius is multiplied by to stay meaningful
        self.exact = fn is None
        self.needs_pair = needs_pair  # treats p1 and p2 differently: not for self-queries
        self.lattice_only = lattice_only

    def __repr__(self):
        return self.name

    def sign(self, D):
        s = np.ones(D, np.float32)
        for ax in (range(D) if self.neg == "all" else self.neg):
            s[min(ax, D - 1)] = -1.0
        return s

    def dist_factor(self, norm):
        return np.float32((4.0 if norm == 2 else 2.0) ** self.k)

    def grad_factor(self, norm, D):
        """grad_p1 / grad_p2 of the framed call = this (per axis) times the base call's: L2 gradients 2 g (a - b)
        follow the differences, L1 gradients g sign(a - b) only their signs."""
        return (self.sign(D) * np.float32(2.0 ** self.k if norm == 2 else 1.0)).astype(np.float32)

    def apply(self, p1, p2=None):
        """-> (p1', p2'); p2 None or `p2 is p1` (a self-query) gives the same array object twice."""
        same = p2 is None or p2 is p1
        arrays = [np.asarray(p1, np.float32)] + ([] if same else [np.asarray(p2, np.float32)])
        if not self.exact:
            assert not (same and self.needs_pair)
            out = self.fn(*(arrays if not same else [arrays[0], arrays[0]]))
            out = [np.ascontiguousarray(o, dtype=np.float32) for o in out][: len(arrays)]
            assert_finite_frame(out)
        else:
            D = arrays[0].shape[-1]
            out = [shift_exact(x, self.t) for x in arrays] if self.t != 0.0 else arrays
            if self.neg:
                out = [(x * self.sign(D)).astype(np.float32) for x in out]  # exact; 0.0 -> -0.0 on negated axes
            if self.k:
                out = scale_exact(out, self.k)
            out = [np.ascontiguousarray(o, dtype=np.float32) for o in out]
        return (out[0], out[0]) if same else (out[0], out[1])

    def radius(self, radius):
        """ball_query radius of the framed call: np.float32(radius) 2^k, so radius^2 scales exactly."""
        assert self.exact
        return float(np.float32(radius)) * 2.0 ** self.k


def _per_axis(v, D):
    return np.resize(np.asarray(v, np.float32), D)  # the three values repeat over wider points


def _affine(scale, offset):
    centre = any(c != 1.0 for c in scale)  # scaled frames are centred first: every axis mixes signs

    def fn(a, b):
        D = a.shape[-1]
        s, o = _per_axis(scale, D), _per_axis(offset, D)
        return [((x - np.float32(0.5)) * s + o).astype(np.float32) if centre else (x * s + o).astype(np.float32)
                for x in (a, b)]

    return fn


def _planar(a, b):
    out = []
    for x in (a, b):
        y = (x - np.float32(0.5)).astype(np.float32)
        y[..., -1] = np.float32(-0.25)
        out.append(y)
    return out


def _opposite(a, b):
    return [(-(a + np.float32(0.25))).astype(np.float32), (b + np.float32(0.25)).astype(np.float32)]


def _outlier(a, b):
    same = a is b
    b = b.copy()
    b[:, 0, :] = np.float32(-1e3)  # one point far below the unit cube: the box stretches in one direction
    return [b, b] if same else [a, b]


EXACT = [
    Frame("shift-0.5", "shift", t=-0.5),
    Frame("shift-1.0", "shift", t=-1.0),
    Frame("shift+2^20", "shift", t=float(2 ** 20), lattice_only=True),
    Frame("shift-(2^20-3)", "shift", t=-float(2 ** 20 - 3), lattice_only=True),
    Frame("neg_all", "neg", neg="all"),
    Frame("neg_y", "neg", neg=(1,)),
    Frame("scale2^-30", "scale", k=-30),
    Frame("scale2^+40", "scale", k=40),
    Frame("negy.shift-0.5.scale2^-30", "compose", t=-0.5, neg=(1,), k=-30),
    Frame("negall.shift-1.0.scale2^+40", "compose", t=-1.0, neg="all", k=40),
]

INEXACT = [
    Frame("offset-1e3", "inexact", fn=_affine((1.0, 1.0, 1.0), (-1e3, -1e3, -1e3))),
    Frame("offset(1e4,-37.25,0.1)", "inexact", fn=_affine((1.0, 1.0, 1.0), (1e4, -37.25, 0.1))),
    Frame("aniso(1,1e-3,1e3)", "inexact", fn=_affine((1.0, 1e-3, 1e3), (0.0, 0.0, 0.0))),
    Frame("aniso(7,0.3,1e-4)", "inexact", fn=_affine((7.0, 0.3, 1e-4), (0.0, 0.0, 0.0))),
    Frame("mag1e18", "inexact", fn=_affine((1e18, 1e18, 1e18), (0.0, 0.0, 0.0)), rscale=1e18),
    Frame("mag1e-18", "inexact", fn=_affine((1e-18, 1e-18, 1e-18), (0.0, 0.0, 0.0)),
          rscale=1e-18),  # squares subnormal or exactly 0
    Frame("planar_z-0.25", "inexact", fn=_planar),
    Frame("opposite_signs", "inexact", fn=_opposite, needs_pair=True),
    Frame("outlier-1e3", "inexact", fn=_outlier),
]

BY_NAME = {f.name: f for f in EXACT + INEXACT}


def frames_for(lattice=False, self_query=False, inexact=True):
    out = [f for f in EXACT if lattice or not f.lattice_only]
    if inexact:
        out += [f for f in INEXACT if not (self_query and f.needs_pair)]
    return out
