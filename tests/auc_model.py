"""AUC-Judd (loss.py:122-213) as a rank problem, in numpy: the statement the HIP kernel (vinet_amd/csrc/metrics.hip)
implements, and the model the CPU tests put in its place.

The reference sweeps one threshold per fixation over the whole map.  With t_0 >= ... >= t_{N-1} the normalised values at
the fixations, k_p = #{ i : t_i > S_p } and hist[k] = #{ p : k_p = k }:  above_i = #{ p : S_p >= t_i } = sum_{k <= i} hist[k].
Everything up to `above` is integers; tests/test_metrics_host.py shows that the score is the reference's to the last bit.
"""
import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


def score_from_above(above, npixels, fp_offset=0):
    """loss.py:179-192 given the counts: tp[i+1] = (i+1)/N, fp[i+1] = (above_i - i - fp_offset) / (P - N), np.trapz(tp, x=fp).
    fp_offset 0 is loss.py:189 (0-based i), 1 is AUC_Judd.m:72 (the 1-based index is subtracted)."""
    above = np.asarray(above, dtype=np.int64)
    n = above.size
    tp, fp = np.zeros(n + 2), np.zeros(n + 2)
    tp[-1] = fp[-1] = 1
    i = np.arange(n, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp[1:-1] = (i + 1).astype(np.float64) / n
        fp[1:-1] = (above - i - fp_offset).astype(np.float64) / (npixels - n)
    return float(_trapz(tp, x=fp))


def score_matlab(above, npixels):
    """AUC_Judd.m:68-75 transcribed line by line (1-based loop index kept), applied to given counts.  The MATLAB file cannot be
    run here: this pins the `mit` variant to its formula, not to MATLAB's output."""
    nfix = len(above)
    tp, fp = np.zeros(nfix + 2), np.zeros(nfix + 2)
    tp[0], tp[-1] = 0, 1
    fp[0], fp[-1] = 0, 1
    for i in range(1, nfix + 1):
        aboveth = int(above[i - 1])
        tp[i] = i / nfix
        fp[i] = (aboveth - i) / (npixels - nfix)
    return float(_trapz(tp, fp))           # trapz(fp, tp) in MATLAB's (x, y) order


def auc_judd_rank(smap, fixmap, fp_offset=0, noise=None):
    """-> (score, N, above [N] int64).  `smap` keeps its dtype through the normalisation (float32 maps are normalised in
    float32, loss.py:163-164); `noise` (float64, already divided by 1e7) is added first as loss.py:160 does."""
    s = np.asarray(smap)
    if noise is not None:
        s = s.astype(np.float64) + np.asarray(noise, dtype=np.float64)
    s = s.reshape(-1)
    f = np.asarray(fixmap).reshape(-1) > 0
    n = int(f.sum())
    none = np.zeros(0, dtype=np.int64)
    if n == 0:
        return float("nan"), 0, none
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (s - s.min()) / (s.max() - s.min())
    if np.isnan(s).all():
        return float("nan"), n, none
    t_asc = np.sort(s[f])
    k = n - np.searchsorted(t_asc, s, side="right")          # thresholds strictly above the pixel
    hist = np.bincount(k, minlength=n + 1)
    above = np.cumsum(hist)[:n]
    return score_from_above(above, s.size, fp_offset), n, above
