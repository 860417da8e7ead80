"""Shuffled AUC (code_for_Metrics/AUC_shuffled.m as eval_diem.m:64-71 calls it) in numpy: the statement the HIP kernels
(vinet_amd/csrc/metrics.hip: sauc_*) implement, and the model the CPU tests put in their place.

Per map S (float32 or float64), fixation map F, other map O:
  1. S <- (S - min) / (max - min) in the dtype of S.
  2. N = #{F > 0}; NaN if N == 0 (AUC_shuffled.m:33-36), if max == min or S holds a NaN (:46-49).
  3. other set = { p : O_p > 0 and not F_p > 0 } (eval_diem.m:65), M its size, K = min(N, M); M == 0 -> NaN (MATLAB's 0/0).
  4. thresholds t_k = k * step in float64 for k = 0, 1, ... while t_k <= 1 -- the element formula of np.arange.  MATLAB's colon
     operator may differ in the last bit for some k and MATLAB cannot be run here: this is the project's definition.
     AUC_shuffled.m:77 stops at max(Sth, curfix); the thresholds above give the point (0, 0) again and add zero area.
  5. per split: curfix = S at K distinct locations of the other set; tp_k = #{Sth >= t_k} / N, fp_k = #{curfix >= t_k} / K;
     (0,0) first, (1,1) last, thresholds descending in between; trapz(fp, tp) in float64; the score is the mean over splits.
  6. counts are integers; `v >= t_k` compares the identically rounded normalised value in float64, never floor(v / step).

The splits' locations are an INPUT here (`samples`: int `[n_splits, >= K]`, each row K pixel indices then -1): the metric is
pinned to its formula.  `draw` is the device's counter-based draw, so that a test can tell what the kernel must select.
"""
import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


def thresholds(step):
    """t_k = k * step (float64) for every k >= 0 with t_k <= 1"""
    k = np.arange(int(1.0 / step) + 3, dtype=np.float64)
    t = k * np.float64(step)
    return t[t <= 1.0]


def normalise(smap):
    s = np.asarray(smap).reshape(-1)
    assert s.dtype in (np.float32, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (s - s.min()) / (s.max() - s.min())


def other_set(fixmap, othermap):
    """-> (fixation mask, sorted pixel indices of the other set)"""
    f = np.asarray(fixmap).reshape(-1) > 0
    o = np.asarray(othermap).reshape(-1) > 0
    return f, np.flatnonzero(o & ~f)


def split_auc(sth, curfix, step):
    """AUC_shuffled.m:75-89 for one split, on normalised values"""
    t = thresholds(step)[::-1]                                   # descending, as fliplr(0:step:...)
    tp, fp = np.zeros(t.size + 2), np.zeros(t.size + 2)
    tp[-1] = fp[-1] = 1.0
    s64, c64 = sth.astype(np.float64), curfix.astype(np.float64)
    for i, th in enumerate(t):
        tp[i + 1] = float((s64 >= th).sum()) / sth.size
        fp[i + 1] = float((c64 >= th).sum()) / curfix.size
    return float(_trapz(tp, x=fp))                               # trapz(fp, tp) in MATLAB's (x, y) order


def auc_shuffled(smap, fixmap, othermap, samples, step=0.1):
    """-> (score, N, M).  `samples`: [n_splits, kmax] pixel indices, -1 padded; every row must hold exactly K = min(N, M)"""
    f, oth = other_set(fixmap, othermap)
    n, m = int(f.sum()), int(oth.size)
    nan = float("nan")
    if n == 0:
        return nan, n, m
    raw = np.asarray(smap).reshape(-1)
    if np.isnan(raw).any() or not raw.max() > raw.min() or m == 0:
        return nan, n, m
    s = normalise(smap)
    sth, k = s[f], min(n, m)
    aucs = []
    for row in np.asarray(samples):
        idx = row[row >= 0]
        assert idx.size == k and np.unique(idx).size == k, "a split holds K distinct locations"
        aucs.append(split_auc(sth, s[idx], step))
    return float(np.mean(np.array(aucs, dtype=np.float64))), n, m


# ---- the device draw (vinet_amd/csrc/metrics.hip: sauc_keys, sauc_key) ----------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def keys(pixels, seed, frame, split):
    """the 32-bit key of every pixel index for (seed, frame id, split): a bijection of the pixel index"""
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    u = lambda v: np.uint64(v & 0xFFFFFFFF)
    x = _mix32(u(seed) ^ np.uint64(0x9E3779B9))
    x = _mix32((x + u(seed >> 32)) & _M32)
    x = _mix32(x ^ u(frame))
    x = _mix32((x + u(frame >> 32)) & _M32)
    k0 = _mix32(x ^ u(split * 0x85EBCA6B))
    k1 = _mix32((k0 + np.uint64(0x9E3779B9)) & _M32) ^ x
    p = np.asarray(pixels, dtype=np.uint64)
    return _mix32((_mix32(p ^ k0) + k1) & _M32)


def draw(other_idx, k, seed, frame, n_splits):
    """-> int32 [n_splits, k]: per split the k locations of `other_idx` with the smallest keys, ascending by pixel index"""
    other_idx = np.asarray(other_idx, dtype=np.int64)
    out = np.empty((n_splits, k), dtype=np.int32)
    for j in range(n_splits):
        h = keys(other_idx, seed, frame, j)
        out[j] = np.sort(other_idx[np.argsort(h, kind="stable")[:k]])
    return out
