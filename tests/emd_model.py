"""The earth mover's distance of code_for_Metrics/EMD.m in plain numpy / Python, the statement the device kernels
(vinet_amd/csrc/emd.hip) are held to.

Three steps.  `resize_weights` / `resize` is MATLAB's default imresize (bicubic, antialiased when shrinking) written from its
definition; there is no MATLAB to compare with, so the tests check it against that definition and a row worked out by hand.
`quantise` is the double-precision wrapper of FastEMD (emd_hat_impl.hpp:27-59, 396-475): pre-flow of min(P, Q) per bin, then the
integers floor(x * 1e6 / max(sum P, sum Q) + 0.5) and floor(D * 1e6 / max D + 0.5).  `min_cost` is a plain successive-shortest-
path solver (Bellman-Ford on the residual graph, no potentials: nothing in common with the device's Dijkstra) for
the integer transportation problem: every unit of the lighter side is shipped, the heavier side's surplus is dropped free."""
import math

import numpy as np

MULT = 1e6


# ---- MATLAB imresize (bicubic, antialias) -----------------------------------------------------------------------------------------
def cubic(t):
    a = abs(t)
    if a <= 1.0:
        return 1.5 * a ** 3 - 2.5 * a ** 2 + 1.0
    if a <= 2.0:
        return -0.5 * a ** 3 + 2.5 * a ** 2 - 4.0 * a + 2.0
    return 0.0


def out_size(n_in, downsize):
    return int(math.ceil(n_in / downsize))


def resize_weights(n_in, n_out, scale):
    """imresize's `contributions` for one dimension as a dense float64 [n_out, n_in] matrix (indices clamped to the border,
    the weights of clamped taps added up)"""
    s = float(scale)
    width = 4.0 / s if s < 1.0 else 4.0
    W = np.zeros((n_out, n_in), dtype=np.float64)
    ntaps = int(math.ceil(width)) + 2
    for x in range(1, n_out + 1):
        u = x / s + 0.5 * (1.0 - 1.0 / s)
        left = int(math.floor(u - width / 2.0))
        idx = [left + k for k in range(ntaps)]
        if s < 1.0:
            w = [s * cubic(s * (u - i)) for i in idx]
        else:
            w = [cubic(u - i) for i in idx]
        tot = 0.0
        for v in w:
            tot += v
        for i, v in zip(idx, w):
            W[x - 1, min(max(i, 1), n_in) - 1] += v / tot
    return W


def resize(img, n_rows, n_cols, scale_r, scale_c):
    img = np.asarray(img, dtype=np.float64)
    return resize_weights(img.shape[0], n_rows, scale_r) @ img @ resize_weights(img.shape[1], n_cols, scale_c).T


def histograms(saliency, fixation, downsize=32):
    """EMD.m:33-41 -> (P from the fixation map, Q from the saliency map, R, C), each map divided by its own sum"""
    fixation, saliency = np.asarray(fixation, dtype=np.float64), np.asarray(saliency, dtype=np.float64)
    R, C = out_size(fixation.shape[0], downsize), out_size(fixation.shape[1], downsize)
    im1 = resize(fixation, R, C, 1.0 / downsize, 1.0 / downsize)
    im2 = resize(saliency, R, C, R / saliency.shape[0], C / saliency.shape[1])
    return im1.reshape(-1) / seq_sum(im1.reshape(-1)), im2.reshape(-1) / seq_sum(im2.reshape(-1)), R, C


# ---- FastEMD's wrapper --------------------------------------------------------------------------------------------------------------
def seq_sum(v):
    t = 0.0
    for x in v:
        t += float(x)
    return t


def ground_distance(R, C):
    rr, cc = np.divmod(np.arange(R * C), C)
    return np.sqrt(((rr[:, None] - rr[None, :]) ** 2 + (cc[:, None] - cc[None, :]) ** 2).astype(np.float64))


def quantise(P, Q, R, C):
    """-> None (the score is NaN), or (supply int64 [N], demand int64 [N], iC int64 [N, N], f, cf, swapped, margin); supply is the
    heavier side.  margin: the smallest distance of a p * f or q * f from a rounding boundary."""
    P, Q = np.asarray(P, dtype=np.float64).reshape(-1), np.asarray(Q, dtype=np.float64).reshape(-1)
    assert P.size == Q.size == R * C
    sp, sq = seq_sum(P), seq_sum(Q)
    D = ground_distance(R, C)
    big = max(sp, sq)
    if not (math.isfinite(sp) and math.isfinite(sq)) or not big > 0.0 or not D.max() > 0.0:
        return None
    m = np.where(P < Q, P, Q)
    p, q = P - m, Q - m
    f, cf = MULT / big, MULT / D.max()
    ip, iq = np.floor(p * f + 0.5).astype(np.int64), np.floor(q * f + 0.5).astype(np.int64)
    iC = np.floor(D * cf + 0.5).astype(np.int64)
    frac = np.concatenate([p * f, q * f]) + 0.5
    margin = float(np.abs(frac - np.round(frac)).min())
    swapped = int(iq.sum()) > int(ip.sum())
    if swapped:
        ip, iq = iq, ip
    return ip, iq, iC, f, cf, swapped, margin


def min_cost(supply, demand, cost):
    """the minimum of sum flow * cost that meets every demand (sum supply >= sum demand), exact in int64; -> (K, augmentations)"""
    supply, demand, cost = (np.asarray(x, dtype=np.int64) for x in (supply, demand, cost))
    src, snk = np.nonzero(supply > 0)[0], np.nonzero(demand > 0)[0]
    a, d = supply[src].copy(), demand[snk].copy()
    assert a.sum() >= d.sum()
    S, T = src.size, snk.size
    c = cost[np.ix_(src, snk)]
    flow = np.zeros((S, T), dtype=np.int64)
    INF = np.int64(1) << 60
    K = augs = 0
    while d.any():
        # Bellman-Ford from every source with supply left, one pass = every forward arc, then every reverse arc with flow
        ds, dt = np.where(a > 0, 0, INF), np.full(T, INF)
        ps, pt = np.full(S, -1), np.full(T, -1)
        for _ in range(S + T + 1):
            cand = ds[:, None] + c
            best = cand.argmin(axis=0)
            val = cand[best, np.arange(T)]
            up_t = val < dt
            dt, pt = np.where(up_t, val, dt), np.where(up_t, best, pt)
            cand = np.where(flow > 0, dt[None, :] - c, INF)
            best = cand.argmin(axis=1)
            val = cand[np.arange(S), best]
            up_s = val < ds
            ds, ps = np.where(up_s, val, ds), np.where(up_s, best, ps)
            if not up_t.any() and not up_s.any():
                break
        else:
            raise AssertionError("negative cycle: the flow was not optimal")
        t = int(np.where(d > 0, dt, INF).argmin())
        amt, j, path = int(d[t]), t, []
        while True:
            i = int(pt[j])
            path.append((i, j, 1))
            if ps[i] < 0:
                break
            j = int(ps[i])
            path.append((i, j, -1))
            amt = min(amt, int(flow[i, j]))
        amt = min(amt, int(a[i]))
        for u, w, sign in path:
            flow[u, w] += sign * amt
        a[i] -= amt
        d[t] -= amt
        K += amt * int(dt[t])
        augs += 1
    assert K == int((flow * c).sum()) and (flow >= 0).all()
    return K, augs


def emd_hist(P, Q, R, C, return_all=False):
    """emd_hat_gd_metric(P, Q, D, 0) for R x C bins in row-major order -> score, or (score, K, margin)"""
    qz = quantise(P, Q, R, C)
    if qz is None:
        return (float("nan"), 0, 0.0) if return_all else float("nan")
    ip, iq, iC, f, cf, _, margin = qz
    K, _ = min_cost(ip, iq, iC)
    score = float(K) / f / cf
    return (score, K, margin) if return_all else score


def emd(saliency, fixation, downsize=32, return_all=False):
    """EMD.m -> score, or (score, K, margin, P, Q)"""
    P, Q, R, C = histograms(saliency, fixation, downsize)
    if return_all:
        return emd_hist(P, Q, R, C, True) + (P, Q)
    return emd_hist(P, Q, R, C)


# ---- the end-to-end cases of tests/test_gpu_emd.py (the host test checks that every one of them qualifies for an exact K) ------------
E2E = {          # name: (ground truth H, W, prediction H, W, downsize, maps, dtype, seed)
    "2x3": (64, 96, 64, 96, 32, 2, np.float32, 1),
    "4x5_ragged": (100, 130, 100, 130, 32, 2, np.float64, 2),
    "7x12_half_size_prediction": (224, 384, 112, 192, 32, 1, np.float32, 3),
    "12x20": (360, 640, 360, 640, 32, 1, np.float32, 4),
}
MARGIN = 1e-6          # a p * f this far from a rounding boundary cannot cross it through 1e-12 of histogram error (times f = 1e6)
_E2E_CACHE = {}


def _blobs(rng, B, H, W, k):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W))
    for b in range(B):
        for _ in range(k):
            cy, cx, sg = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.04, 0.2) * W
            out[b] += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
        out[b] += 0.02 * rng.random((H, W))
    return out


def e2e_case(name):
    """-> (pred [B,Hs,Ws], gt [B,Hg,Wg], downsize, [(score, K, margin, P, Q) per map]); computed once per process"""
    if name not in _E2E_CACHE:
        Hg, Wg, Hs, Ws, ds, B, dtype, seed = E2E[name]
        rng = np.random.default_rng(seed)
        gt, pred = _blobs(rng, B, Hg, Wg, 4).astype(dtype), _blobs(rng, B, Hs, Ws, 5).astype(dtype)
        _E2E_CACHE[name] = (pred, gt, ds, [emd(pred[b], gt[b], ds, return_all=True) for b in range(B)])
    return _E2E_CACHE[name]
