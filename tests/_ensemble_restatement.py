"""numpy restatement of fh_ensemble_stats (include/fh_hip.h), word for word: float64, explicit loops over the members, no fused
multiply-add (numpy rounds every product before the sum it feeds).  Vectorised over the elements only.

Per element p of an ensemble of K samples x_k in the sampler's units:
    v_k     = min(max(127.5 * x_k + 127.5, 0), 255)
    m       = (((v_0 + v_1) + v_2) + ...) / K          summed in member order
    SS      = sum_k (v_k - m)^2                        summed in member order, second pass
    mean_u8 = (uint8) floor(m + 0.5)
    std     = (float32) sqrt(SS / (K - 1))
With the truth t as a double and d2 = (t - m)^2, p is covered at c sigma when  d2 * K * (K - 1) <= (c * c) * SS * (K + 1).
Per ensemble: spread2 = mean_p SS / (K - 1), skill2 = mean_p d2, cover_c = covered fraction; skill2 = cover_c = -1 without a truth."""
import numpy as np


def to_u8_units(x):
    x = np.asarray(x, dtype=np.float64)
    return np.minimum(np.maximum(127.5 * x + 127.5, 0.0), 255.0)


def stats_of_values(v, truth=None):
    """v: float64 [K, n] values in 8-bit units (already clipped); truth: [n] or None.  Returns a dict of per-element arrays
    (m, SS, mean_u8, std, and with a truth d2, lhs, rhs1, rhs2, covered1, covered2) and the per-ensemble numbers (spread2, skill2,
    count1, count2, cover1, cover2)."""
    v = np.asarray(v, dtype=np.float64)
    K, n = v.shape
    s = v[0].copy()
    for k in range(1, K):
        s = s + v[k]
    m = s / float(K)
    SS = np.zeros(n, dtype=np.float64)
    for k in range(K):
        d = v[k] - m
        SS = SS + d * d
    var = SS / float(K - 1)
    r = dict(m=m, SS=SS, mean_u8=np.floor(m + 0.5).astype(np.uint8), std=np.sqrt(var).astype(np.float32),
             spread2=float(np.sum(var) / float(n)), skill2=-1.0, count1=-1, count2=-1, cover1=-1.0, cover2=-1.0)
    if truth is not None:
        t = np.asarray(truth).astype(np.float64).reshape(n)
        d2 = (t - m) * (t - m)
        lhs = d2 * float(K) * float(K - 1)
        r.update(d2=d2, lhs=lhs, skill2=float(np.sum(d2) / float(n)))
        for c in (1, 2):
            rhs = float(c * c) * SS * float(K + 1)
            covered = lhs <= rhs
            r[f"rhs{c}"], r[f"covered{c}"] = rhs, covered
            r[f"count{c}"] = int(np.count_nonzero(covered))
            r[f"cover{c}"] = r[f"count{c}"] / float(n)
    return r


def ensemble_stats(x, truth=None):
    """x: float64 [K, n] samples of ONE ensemble in the sampler's units; truth uint8 [n] or None"""
    return stats_of_values(to_u8_units(x), truth)


def fair(r, rel=1e-9):
    """True when an exact comparison with another float64 implementation of the same formulas is fair: no element within `rel`
    (relative) of a coverage boundary - an element with lhs = rhs = 0 (all members on one clip, the truth there too) is exact on
    both sides and counts as off the boundary - and no m + 0.5 within `rel` of an integer."""
    h = r["m"] + 0.5
    ok = bool(np.all(np.abs(h - np.round(h)) > rel))
    if "lhs" in r:
        for c in (1, 2):
            big = np.maximum(r["lhs"], r[f"rhs{c}"])
            ok = ok and bool(np.all((np.abs(r["lhs"] - r[f"rhs{c}"]) > rel * big) | (big == 0.0)))
    return ok
