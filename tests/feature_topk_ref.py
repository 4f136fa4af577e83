"""numpy restatement of the certificate of csrc/feature_topk.h (the FEATURE TOP-K block of include/pointops_amd.h), on
the arithmetic of tests/match_ref.py: which rows the K <= 32 screen must send to its exact fallback.  Nothing here reads
the library."""
import numpy as np

import match_ref as ref

F32 = np.float32


def list_of(j, S):
    """t(j) = 2 ((j >> 5) mod S) + ((j >> 2) & 1): the wave that sees the target's block, the half of the accumulator."""
    return 2 * ((j >> 5) % S) + ((j >> 2) & 1)


def uncertified_rows(f1, f2, lengths1=None, lengths2=None, K=1, M=16, S=1):
    """(N, P1) bool.  Each of the 2 S lists of a row keeps the M smallest (s, j) of its targets; the collected targets
    of a row are all its lists; r_K is the K-th smallest exact distance among them (+inf if there are fewer); s_cut is
    the smallest M-th key over the lists (+inf for a list that never filled); the row is certified when the cloud has
    at most M targets or fl(r_K + E) < s_cut, and never when a norm is not finite or above 2^126."""
    lengths1, lengths2 = ref.full_lengths(f1, lengths1), ref.full_lengths(f2, lengths2)
    N, P1, D = f1.shape
    out = np.zeros((N, P1), bool)
    for n in range(N):
        l1, l2 = int(min(max(lengths1[n], 0), P1)), int(min(max(lengths2[n], 0), f2.shape[1]))
        if l1 == 0 or l2 == 0:
            continue
        n2 = ref.norms(f2[n, :l2])
        n2max = n2.max() if np.isfinite(n2).all() else F32(np.nan)
        lists = list_of(np.arange(l2), S)
        for lo in range(0, l1, 128):  # (blocks of rows: the float64 temporaries stay in cache)
            a, b = f1[n, lo:min(lo + 128, l1)], f2[n, :l2]
            s, n1, _ = ref.screen_values(a, b)
            fin = ref.row_finite(D, n1, n2max)
            if l2 <= M:
                out[n, lo:lo + len(a)] = ~fin
                continue
            r = ref.pair_distances(a, b)
            E = ref.screen_bound(D, n1, n2max)
            collected = np.zeros(s.shape, bool)
            s_cut = np.full(len(a), np.inf, F32)
            for t in range(2 * S):
                js = np.nonzero(lists == t)[0]
                if len(js) == 0:
                    continue
                order = np.argsort(s[:, js], axis=1, kind="stable")[:, :M]
                np.put_along_axis(collected, js[order], True, axis=1)
                if len(js) >= M:
                    s_cut = np.minimum(s_cut, np.take_along_axis(s[:, js], order[:, M - 1:M], axis=1)[:, 0])
            kept = np.sort(np.where(collected, r, F32(np.inf)), axis=1)
            rK = kept[:, K - 1] if K <= l2 else np.full(len(a), np.inf, F32)
            with np.errstate(all="ignore"):
                ok = fin & ((rK + E).astype(F32) < s_cut)
            out[n, lo:lo + len(a)] = ~ok
    return out
