"""AUC-Borji (code_for_Metrics/AUC_Borji.m) and the information gain (InfoGain.m, IG.m) in numpy, float64: the statements the HIP
kernels (vinet_amd/csrc/metrics.hip: split_auc_kernel with BorjiDraw, info_gain_kernel) implement, and the models the CPU tests put in their
place.

AUC-Borji, per map S (float32 or float64) and fixation map F:
  1. N = #{F > 0}; NaN if N <= 1 (AUC_Borji.m:31), if max == min or S holds a NaN (:43-48).
  2. S <- (S - min) / (max - min) in the dtype of S; thresholds, `>=`, the end points and the trapezoid sum are the shuffled AUC's
     (tests/sauc_model.py: thresholds, normalise, split_auc), tp and fp both over N (:75-76).
  3. per split: curfix = S at N locations drawn from ALL pixels, uniformly, with replacement (:58 randi): a location may be a
     fixation and may repeat.  The score is the mean of the splits' areas.
The locations are an INPUT (`samples`: int `[n_splits, >= N]`, each row N pixel indices then -1); `draw` is the device's
counter-based draw.

Information gain, per map S, fixation map F, baseline map B (or None), everything in float64:
  v = (S - min) / (max - min), p = v / sum(v); the same for B -> pb;
  score = mean over { F > 0 } of log2(eps + p) - log2(eps + pb), eps = 2^-52 (InfoGain.m:17-27); without a baseline the second
  term is absent (IG.m:28-31).  NaN: no fixation, a constant S or B, a NaN in either.
"""
import numpy as np

from tests import sauc_model as SM

BORJI_DOMAIN = 0x426F726A69415543          # "BorjiAUC": folded into the seed, so that --sauc and --borji do not share a stream
EPS = 2.0 ** -52


def auc_borji(smap, fixmap, samples, step=0.1):
    """-> (score, N).  `samples`: [n_splits, kmax] pixel indices, -1 padded; every row must hold exactly N"""
    f = np.asarray(fixmap).reshape(-1) > 0
    n = int(f.sum())
    nan = float("nan")
    if n <= 1:
        return nan, n
    raw = np.asarray(smap).reshape(-1)
    if np.isnan(raw).any() or not raw.max() > raw.min():
        return nan, n
    s = SM.normalise(smap)
    sth = s[f]
    aucs = []
    for row in np.asarray(samples):
        idx = row[row >= 0]
        assert idx.size == n and (idx < s.size).all(), "a split holds N locations"
        aucs.append(SM.split_auc(sth, s[idx], step))
    return float(np.mean(np.array(aucs, dtype=np.float64))), n


def draw(n, N, seed, frame, n_splits):
    """-> int32 [n_splits, N]: sample j of split q is pixel (h * n) >> 32 with h the shuffled AUC's key of j under
    (seed ^ BORJI_DOMAIN, frame id, q); each row ascending (what loss.auc_borji_batch(return_samples=True) hands back)"""
    seed = (int(seed) & (2 ** 64 - 1)) ^ BORJI_DOMAIN
    out = np.empty((n_splits, N), dtype=np.int32)
    j = np.arange(N)
    for q in range(n_splits):
        h = SM.keys(j, seed, frame, q)
        out[q] = np.sort((h * np.uint64(n)) >> np.uint64(32))
    return out


def _dist(m):
    v = np.asarray(m, dtype=np.float64).reshape(-1)
    if np.isnan(v).any() or not v.max() > v.min():
        return None
    v = (v - v.min()) / (v.max() - v.min())
    return v / v.sum()


def info_gain(smap, fixmap, baseline=None):
    f = np.asarray(fixmap).reshape(-1) > 0
    p = _dist(smap)
    pb = _dist(baseline) if baseline is not None else None
    if not f.any() or p is None or (baseline is not None and pb is None):
        return float("nan")
    t = np.log2(EPS + p[f])
    if pb is not None:
        t = t - np.log2(EPS + pb[f])
    return float(np.mean(t))
