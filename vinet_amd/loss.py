"""Saliency losses on MI355X -- drop-in for the reference's loss.py:13-99.

`kldiv(s_map, gt)`, `cc(s_map, gt)`, `similarity(s_map, gt)` keep the reference's
signatures ([B,H,W] maps -> scalar, batch mean) and are differentiable w.r.t.
`s_map`.  Forward and backward each run as one workgroup-per-sample HIP kernel
with fp64 accumulators (libvinet_hip.so: vinet_loss_fwd / vinet_loss_bwd).
Ground truth may be float32 or float64 (the DIEM loader hands over float64,
SURVEY.md F11); like the reference the result is then float64.

The validation metrics `nss` (loss.py:101-120) and `auc_judd` (loss.py:122-213) run on the device too, forward only;
`auc_judd_batch` scores a whole batch in one launch (libvinet_hip.so: vinet_auc_judd, one workgroup per map, exact
integer counts).  `auc_shuff` (loss.py:215-284) is left out on purpose: the reference raises TypeError on every input
(it calls the torch `normalize_map` on a numpy array), so there is nothing to reproduce.  The shuffled AUC that the
reference's evaluation does compute is the MATLAB one (code_for_Metrics/AUC_shuffled.m, called from eval_diem.m): that is
`auc_shuffled` / `auc_shuffled_batch` here (libvinet_hip.so: vinet_auc_shuffled), with `shuffle_map` for createShuffmap1.m.
The two other fixation metrics of that folder run on the device as well: `auc_borji` / `auc_borji_batch` (AUC_Borji.m;
vinet_auc_borji) and `info_gain` / `info_gain_batch` (InfoGain.m, IG.m; vinet_info_gain).  The distribution metric of that
folder that is not a loss, the earth mover's distance, is `emd` / `emd_batch` (EMD.m; vinet_emd), with `emd_hist_batch` for
histograms that are already downsampled (vinet_emd_hist).
"""
import torch

from . import _lib as L
from . import engine as E

_WHICH = {"kldiv": 0, "cc": 1, "similarity": 2, "nss": 3}
_NAME = {v: k for k, v in _WHICH.items()}
_F32_F64 = (torch.float32, torch.float64)


def _is64(t):
    """the C ABI's dtype flag of a float32 / float64 tensor"""
    return 1 if t.dtype == torch.float64 else 0


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _on_device(t, maps, name):
    """A tensor that goes to a kernel beside `maps` must live where they do: its pointer is handed over as it is, and a host pointer
    in a kernel is a device fault, not a Python error.  `name`: "<metric>: <argument>"."""
    if t.device != maps.device:
        raise ValueError("%s on %s, the maps on %s" % (name, t.device, maps.device))
    return t


def _canon(t, dtypes=_F32_F64, maps=None, name=None):
    """`t` as the kernels take it: detached, its dtype kept if it is one of `dtypes` and cast to the first of them if not,
    contiguous.  With `maps` (the saliency maps; `t` is a companion of theirs): on their device, or ValueError."""
    if maps is not None:
        _on_device(t, maps, name)
    t = t.detach()
    if t.dtype not in dtypes:
        t = t.to(dtypes[0])
    return t.contiguous()


def _first(m):
    """a 2-D map, or item 0 of a 3-D batch, as a batch of one"""
    return m[:1] if m.dim() == 3 else m.unsqueeze(0)


def _loss_fwd(which, s, g):
    """vinet_loss_fwd on maps that are float32 `[B,H,W]` and float32 / float64, both contiguous -> the batch value (float32
    scalar) and the per-sample statistics the backward kernel and `per_sample` read (float64 `[B * 8]`)"""
    B, n = s.shape[0], s.shape[1] * s.shape[2]
    saved = torch.empty(B * 8, dtype=torch.float64, device=s.device)
    out = torch.empty((), dtype=torch.float32, device=s.device)
    L.check(L.get().vinet_loss_fwd(which, s.data_ptr(), g.data_ptr(), _is64(g), B, n, saved.data_ptr(), out.data_ptr(),
                                   E._stream_for(s.device)), "vinet_loss_fwd")
    return out, saved


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s_map, gt, which):
        assert s_map.size() == gt.size()
        assert s_map.dim() == 3, "expected [B,H,W] maps"
        s = _canon(s_map, (torch.float32,))
        g = _canon(gt, maps=s, name=_NAME[which] + ": gt")
        loss, saved = _loss_fwd(which, s, g)
        ctx.save_for_backward(s, g, saved)
        ctx.which, ctx.shape = which, s_map.shape
        return loss.double() if g.dtype == torch.float64 else loss

    @staticmethod
    def backward(ctx, gout):
        s, g, saved = ctx.saved_tensors
        B, n = s.shape[0], s.shape[1] * s.shape[2]
        lib = L.get()
        stream = E._stream_for(s.device)
        gs = gout.detach().float().contiguous()
        ds = torch.empty_like(s)
        L.check(lib.vinet_loss_bwd(ctx.which, s.data_ptr(), g.data_ptr(), _is64(g), B, n,
                                   saved.data_ptr(), gs.data_ptr(), 1.0, 0, ds.data_ptr(), stream), "vinet_loss_bwd")
        return ds.view(ctx.shape), None, None


def kldiv(s_map, gt):
    """loss.py:13-38."""
    return _LossFn.apply(s_map, gt, 0)


def cc(s_map, gt):
    """loss.py:80-99."""
    return _LossFn.apply(s_map, gt, 1)


def similarity(s_map, gt):
    """loss.py:52-78 (with normalize_map, loss.py:41-50)."""
    return _LossFn.apply(s_map, gt, 2)


@torch.no_grad()
def nss(s_map, gt):
    """loss.py:101-120 for maps of equal size (the reference `cv2.resize`s s_map to gt's size first when they
    differ, which is host post-processing): z-score of the saliency map with the unbiased
    std (+2.2204e-16), mean over the fixation mask; batch mean.  A validation metric: no gradient."""
    assert s_map.size() == gt.size(), "nss: resize the saliency map to the fixation map first"
    assert s_map.dim() == 3, "expected [B,H,W] maps"
    s = _canon(s_map, (torch.float32,))
    g = _canon(gt, maps=s, name="nss: gt")
    out, _ = _loss_fwd(3, s, g)
    return out.double() if g.dtype == torch.float64 else out


@torch.no_grad()
def auc_judd_batch(s_maps, fix_maps, *, noise=None, mit=False, return_counts=False):
    """AUC-Judd of every map of a batch: `[B,H,W]` float32 or float64 saliency maps, fixation maps of the same size (a
    fixation is `> 0`) -> float64 `[B]` on the device, NaN where a map has no fixation or is constant.  `noise`: an optional
    float64 `[B,H,W]` tensor added as `s.double() + noise` first (that is what the reference's jitter is, loss.py:158-160).
    `mit=True` subtracts the 1-based threshold index as AUC_Judd.m:72 does; the default reproduces loss.py:189.
    `return_counts`: also the number of fixations `[B]` and the `above` counts `[B, H*W]` (int32, first N valid)."""
    assert s_maps.size() == fix_maps.size(), "auc_judd: resize the saliency map to the fixation map first"
    assert s_maps.dim() == 3, "expected [B,H,W] maps"
    s = s_maps.detach()
    if noise is not None:
        assert noise.size() == s.size() and noise.dtype == torch.float64, "noise: a float64 tensor of the maps' size"
        s = s.double() + _on_device(noise, s, "auc_judd: noise")
    s = _canon(s)
    g = _canon(fix_maps, maps=s, name="auc_judd: fix_maps")
    B, n = s.shape[0], s.shape[1] * s.shape[2]
    lib = L.get()
    ws = torch.empty(max(int(lib.vinet_auc_judd_workspace(B, n)), 8), dtype=torch.uint8, device=s.device)
    score = torch.empty(B, dtype=torch.float64, device=s.device)
    nfix = torch.empty(B, dtype=torch.int32, device=s.device)
    above = torch.empty((B, n), dtype=torch.int32, device=s.device) if return_counts else None
    L.check(lib.vinet_auc_judd(s.data_ptr(), _is64(s), g.data_ptr(), _is64(g), B, n, 1 if mit else 0, ws.data_ptr(), ws.numel(),
                               score.data_ptr(), nfix.data_ptr(), _ptr(above), E._stream_for(s.device)), "vinet_auc_judd")
    return (score, nfix, above) if return_counts else score


def auc_judd(saliencyMap, fixationMap, jitter=True, toPlot=False, normalize=False):
    """loss.py:122-213 for maps of equal size: a 2-D map or, of a 3-D batch, item 0 (loss.py:135-137) -> Python float.
    `jitter=True` adds `torch.rand(float64) / 1e7`, drawn on the maps' device.  Prints the reference's message and returns NaN
    when there is no fixation or the map is constant."""
    if toPlot:
        raise NotImplementedError("auc_judd(toPlot=True) draws with matplotlib on the host; plot the returned score's inputs yourself")
    if normalize:
        raise NotImplementedError("auc_judd(normalize=True) raises TypeError in the reference (torch normalize_map on a numpy array)")
    assert saliencyMap.size() == fixationMap.size(), "auc_judd: resize the saliency map to the fixation map first"
    assert saliencyMap.dim() in (2, 3), "expected a [H,W] map or a [B,H,W] batch"
    s, f = _first(saliencyMap), _first(fixationMap)
    noise = torch.rand(s.shape, dtype=torch.float64, device=s.device) / 1e7 if jitter else None
    score, nfix, _ = auc_judd_batch(s, f, noise=noise, return_counts=True)
    score, nfix = float(score[0]), int(nfix[0])
    if score != score:
        print('Error: no fixationMap' if nfix == 0 else 'NaN saliencyMap')
    return score


def shuffle_map(fix_maps):
    """createShuffmap1.m: the union of a video's fixation maps, `[T,H,W]` (a fixation is `> 0`) -> uint8 `[H,W]`.  The frame's
    own fixations (eval_diem.m:65) are taken out by the kernel, per map."""
    assert fix_maps.dim() == 3, "expected [T,H,W] fixation maps"
    return (fix_maps > 0).any(dim=0).to(torch.uint8)


@torch.no_grad()
def auc_shuffled_batch(s_maps, fix_maps, other_map, *, n_splits=100, step=0.1, seed=0, frame_ids=None, samples=None,
                       return_samples=False, return_counts=False):
    """Shuffled AUC (AUC_shuffled.m) of every map of a batch: `[B,H,W]` float32 or float64 saliency maps, fixation maps of the
    same size, `other_map` `[H,W]` (one for the batch) or `[B,H,W]`, uint8 / bool / float32 / float64 -> float64 `[B]` on the
    device.  A map's other set is `other > 0 and not fix > 0` (eval_diem.m:65), K = min(fixations, other set); NaN where a map
    has no fixation, is constant, holds a NaN or has an empty other set.
    The K locations of each of the `n_splits` splits are drawn on the device as a function of (`seed`, the map's frame id,
    split, pixel) -- `frame_ids`: int64 `[B]`, default 0 .. B-1; a map's score does not depend on the batch around it -- or
    taken from `samples`: int32 `[B, n_splits, kmax]`, each row K pixel indices then -1.
    `return_counts`: also the fixations `[B]` and the other set's size `[B]` (int32); `return_samples`: those and the drawn
    locations, int32 `[B, n_splits, max K]`, each row ascending and padded with -1."""
    score, nfix, nother, drawn = _split_auc("auc_shuffled", s_maps, fix_maps, other_map, n_splits, step, seed, frame_ids, samples,
                                            return_samples)
    if return_samples:
        return score, nfix, nother, drawn
    return (score, nfix, nother) if return_counts else score


def auc_shuffled(saliencyMap, fixationMap, otherMap, Nsplits=100, stepSize=0.1):
    """AUC_shuffled.m's signature for maps of equal size (2-D, or item 0 of a 3-D batch as `auc_judd` takes it) -> Python float.
    `otherMap` is used as eval_diem.m:64-71 hands it over: locations that are fixations of this map do not count.  Prints the
    MATLAB messages and returns NaN when there is no fixation or the map is constant; toPlot has no counterpart."""
    assert saliencyMap.size() == fixationMap.size(), "auc_shuffled: resize the saliency map to the fixation map first"
    assert saliencyMap.dim() in (2, 3), "expected a [H,W] map or a [B,H,W] batch"
    s, f = _first(saliencyMap), _first(fixationMap)
    o = otherMap[0] if otherMap.dim() == 3 else otherMap
    score, nfix, _ = auc_shuffled_batch(s, f, o, n_splits=Nsplits, step=stepSize, return_counts=True)
    score, nfix = float(score[0]), int(nfix[0])
    if score != score:
        print('no fixationMap' if nfix == 0 else 'NaN saliencyMap')
    return score


def _draw_args(g, n_splits, frame_ids, samples, return_samples):
    """what selects or returns the locations of a split metric, on the device of the fixation maps `g` (frame ids and samples are
    moved there): the frame ids (or None), the given samples (or None), the buffer for the drawn ones (or None), a row's length"""
    B, dev = g.shape[0], g.device
    fid = None
    if frame_ids is not None:
        fid = torch.as_tensor(frame_ids, dtype=torch.int64).to(dev).contiguous()
        assert tuple(fid.shape) == (B,), "frame_ids: one int64 per map"
    smp = out = None
    kmax = 0
    if samples is not None:
        assert samples.dim() == 3 and tuple(samples.shape[:2]) == (B, n_splits) and samples.shape[2] > 0, "samples: [B, n_splits, kmax]"
        smp = samples.detach().to(device=dev, dtype=torch.int32).contiguous()
        kmax = smp.shape[2]
    elif return_samples:
        kmax = max(int((g > 0).flatten(1).sum(1).max()), 1)          # a split has at most as many locations as the map has fixations
        out = torch.empty((B, n_splits, kmax), dtype=torch.int32, device=dev)
    return fid, smp, out, kmax


def _split_auc(who, s_maps, fix_maps, other_map, n_splits, step, seed, frame_ids, samples, return_samples):
    """`auc_shuffled_batch` (`who` "auc_shuffled") and `auc_borji_batch` ("auc_borji", `other_map` None): the checks, the marshalling
    and the call -> score, nfix, nother (None without an other map), the drawn samples (None unless `return_samples`)"""
    assert s_maps.size() == fix_maps.size(), "%s: resize the saliency map to the fixation map first" % who
    assert s_maps.dim() == 3, "expected [B,H,W] maps"
    if other_map is not None:
        assert other_map.dim() in (2, 3) and tuple(other_map.shape[-2:]) == tuple(s_maps.shape[1:]), "other_map: [H,W] or [B,H,W] of the maps' size"
        assert other_map.dim() == 2 or other_map.shape[0] == s_maps.shape[0], "other_map: one map, or one per saliency map"
    assert samples is None or not return_samples, "return_samples returns the device draw"
    s = _canon(s_maps)
    g = _canon(fix_maps, maps=s, name=who + ": fix_maps")
    o = None
    if other_map is not None:
        o = other_map.to(torch.uint8) if other_map.dtype == torch.bool else other_map
        o = _canon(o, (torch.float32, torch.uint8, torch.float64), maps=s, name=who + ": other_map")
    B, n, dev = s.shape[0], s.shape[1] * s.shape[2], s.device
    lib = L.get()
    n_splits, step = int(n_splits), float(step)
    fid, smp, out, kmax = _draw_args(g, n_splits, frame_ids, samples, return_samples)
    need = int(getattr(lib, "vinet_%s_workspace" % who)(B, n, n_splits, step))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    nfix = torch.empty(B, dtype=torch.int32, device=dev)
    nother = torch.empty(B, dtype=torch.int32, device=dev) if o is not None else None
    maps = (s.data_ptr(), _is64(s), g.data_ptr(), _is64(g))
    rest = (B, n, n_splits, step, int(seed), _ptr(fid), _ptr(smp), kmax, ws.data_ptr(), need, score.data_ptr(), nfix.data_ptr())
    if o is not None:
        rc = lib.vinet_auc_shuffled(*maps, o.data_ptr(), {torch.uint8: 0, torch.float32: 1, torch.float64: 2}[o.dtype],
                                    0 if o.dim() == 2 else n, *rest, nother.data_ptr(), _ptr(out), E._stream_for(dev))
    else:
        rc = lib.vinet_auc_borji(*maps, *rest, _ptr(out), E._stream_for(dev))
    L.check(rc, "vinet_" + who)
    if out is not None:
        # the kernel fills a row in no particular order: ascending, the -1 padding last
        big = torch.iinfo(torch.int32).max
        srt = torch.where(out < 0, torch.full_like(out, big), out).sort(dim=2).values
        out = torch.where(srt == big, torch.full_like(srt, -1), srt)
    return score, nfix, nother, out


@torch.no_grad()
def auc_borji_batch(s_maps, fix_maps, *, n_splits=100, step=0.1, seed=0, frame_ids=None, samples=None, return_samples=False,
                    return_counts=False):
    """AUC-Borji (AUC_Borji.m) of every map of a batch: `[B,H,W]` float32 or float64 saliency maps, fixation maps of the same
    size -> float64 `[B]` on the device.  Per split N = #fixations locations drawn from ALL pixels, uniformly and with
    replacement (MATLAB's randi); tp and fp over N; NaN where a map has at most one fixation (AUC_Borji.m:31), is constant or
    holds a NaN.
    The locations are drawn on the device as a function of (`seed`, the map's frame id, split, sample number) -- `frame_ids`:
    int64 `[B]`, default 0 .. B-1; a map's score does not depend on the batch around it; the stream is not the one
    `auc_shuffled_batch` draws from under the same seed -- or taken from `samples`: int32 `[B, n_splits, kmax]`, each row N
    pixel indices then -1.
    `return_counts`: also the fixations `[B]` (int32); `return_samples`: those and the drawn locations, int32
    `[B, n_splits, max N]`, each row ascending and padded with -1."""
    score, nfix, _, drawn = _split_auc("auc_borji", s_maps, fix_maps, None, n_splits, step, seed, frame_ids, samples, return_samples)
    if return_samples:
        return score, nfix, drawn
    return (score, nfix) if return_counts else score


def auc_borji(saliencyMap, fixationMap, Nsplits=100, stepSize=0.1):
    """AUC_Borji.m's signature for maps of equal size (2-D, or item 0 of a 3-D batch as `auc_judd` takes it) -> Python float.
    Prints the MATLAB messages and returns NaN when there is at most one fixation (AUC_Borji.m:31-35) or the map is constant
    (:45-48); toPlot has no counterpart."""
    assert saliencyMap.size() == fixationMap.size(), "auc_borji: resize the saliency map to the fixation map first"
    assert saliencyMap.dim() in (2, 3), "expected a [H,W] map or a [B,H,W] batch"
    s, f = _first(saliencyMap), _first(fixationMap)
    score, nfix = auc_borji_batch(s, f, n_splits=Nsplits, step=stepSize, return_counts=True)
    score, nfix = float(score[0]), int(nfix[0])
    if score != score:
        print('no fixationMap' if nfix <= 1 else 'NaN saliencyMap')
    return score


@torch.no_grad()
def info_gain_batch(s_maps, fix_maps, baseline=None, *, return_counts=False):
    """Information gain (InfoGain.m; IG.m without a baseline) of every map of a batch: `[B,H,W]` float32 or float64 saliency
    maps, fixation maps of the same size, `baseline` None, `[H,W]` (one for the batch) or `[B,H,W]`, float32 or float64 ->
    float64 `[B]` on the device: the mean over the fixations of log2(eps + p) - log2(eps + pb), p and pb the min-max normalised
    maps divided by their sums, all in float64.  NaN where a map has no fixation, the map or its baseline is constant, or
    either holds a NaN.  `return_counts`: also the fixations `[B]` (int32)."""
    assert s_maps.size() == fix_maps.size(), "info_gain: resize the saliency map to the fixation map first"
    assert s_maps.dim() == 3, "expected [B,H,W] maps"
    s = _canon(s_maps)
    g = _canon(fix_maps, maps=s, name="info_gain: fix_maps")
    B, n, dev = s.shape[0], s.shape[1] * s.shape[2], s.device
    bl = None
    if baseline is not None:
        assert baseline.dim() in (2, 3) and tuple(baseline.shape[-2:]) == tuple(s.shape[1:]), "baseline: [H,W] or [B,H,W] of the maps' size"
        assert baseline.dim() == 2 or baseline.shape[0] == B, "baseline: one map, or one per saliency map"
        bl = _canon(baseline, maps=s, name="info_gain: baseline")
    score = torch.empty(B, dtype=torch.float64, device=dev)
    nfix = torch.empty(B, dtype=torch.int32, device=dev)
    L.check(L.get().vinet_info_gain(s.data_ptr(), _is64(s), g.data_ptr(), _is64(g), _ptr(bl), _is64(bl) if bl is not None else 0,
                                    0 if bl is None or bl.dim() == 2 else n, B, n, score.data_ptr(), nfix.data_ptr(),
                                    E._stream_for(dev)), "vinet_info_gain")
    return (score, nfix) if return_counts else score


def info_gain(saliencyMap, fixationMap, baselineMap=None):
    """InfoGain.m's signature (IG.m's when `baselineMap` is None) for maps of equal size (2-D, or item 0 of a 3-D batch) ->
    Python float."""
    assert saliencyMap.size() == fixationMap.size(), "info_gain: resize the saliency map to the fixation map first"
    assert saliencyMap.dim() in (2, 3), "expected a [H,W] map or a [B,H,W] batch"
    s, f = _first(saliencyMap), _first(fixationMap)
    bl = None if baselineMap is None else (baselineMap[0] if baselineMap.dim() == 3 else baselineMap)
    return float(info_gain_batch(s, f, bl)[0])


_EMD_WEIGHTS = {}


def _emd_weights(n_in, n_out, scale, device):
    """utils.matlab_resize_weights on `device`, uploaded once per (n_in, n_out, scale, device)"""
    key = (n_in, n_out, float(scale), str(device))
    if key not in _EMD_WEIGHTS:
        from . import utils
        _EMD_WEIGHTS[key] = utils.matlab_resize_weights(n_in, n_out, float(scale)).to(device).contiguous()
    return _EMD_WEIGHTS[key]


def _emd_outputs(B, dev, return_cost, return_status):
    score = torch.empty(B, dtype=torch.float64, device=dev)
    cost = torch.empty(B, dtype=torch.int64, device=dev) if return_cost else None
    status = torch.empty(B, dtype=torch.int32, device=dev) if return_status else None
    return score, cost, status


def _emd_result(score, cost, status, more=()):
    out = (score,) + tuple(x for x in (cost, status) if x is not None) + tuple(more)
    return out[0] if len(out) == 1 else out


@torch.no_grad()
def emd_batch(s_maps, gt_maps, *, downsize=32, return_cost=False, return_status=False, return_hist=False):
    """Earth mover's distance (EMD.m) of every pair of a batch: `[B,Hs,Ws]` saliency maps and `[B,Hg,Wg]` ground-truth maps,
    float32 or float64, of any two sizes -> float64 `[B]` on the device.  The ground truth is resized by 1 / `downsize` to
    R x C = ceil(Hg / downsize) x ceil(Wg / downsize) bins and the saliency map to that size (MATLAB's imresize: bicubic,
    antialiased), each is divided by its sum, and FastEMD's emd_hat_gd_metric with the bins' Euclidean distance and no penalty
    for extra mass is solved exactly on integers (1e6 units of mass, 1e6 steps of distance).  NaN where a resized map sums to
    zero or holds a NaN, or the grid has a single bin.  At most 512 bins.
    `return_cost`: also the integer optimum K `[B]` (int64); `return_status`: also the solver's status `[B]` (int32, 0 = solved;
    include/vinet_hip.h); `return_hist`: also the two histograms, float64 `[B, 2, R*C]` (ground truth, saliency map)."""
    assert s_maps.dim() == 3 and gt_maps.dim() == 3 and s_maps.shape[0] == gt_maps.shape[0], "expected [B,Hs,Ws] and [B,Hg,Wg] maps"
    s = _canon(s_maps)
    g = _canon(gt_maps, maps=s, name="emd: gt_maps")
    dev = s.device
    downsize = int(downsize)
    B, (Hs, Ws), (Hg, Wg) = s.shape[0], s.shape[1:], g.shape[1:]
    R, C = (-(-Hg // downsize), -(-Wg // downsize)) if downsize >= 1 else (0, 0)
    lib = L.get()
    need = int(lib.vinet_emd_workspace(B, R, C))
    wts = [None] * 4
    if need:          # (else the library refuses the call below and says why)
        wts = [_emd_weights(Hg, R, 1.0 / downsize, dev), _emd_weights(Wg, C, 1.0 / downsize, dev),
               _emd_weights(Hs, R, R / Hs, dev), _emd_weights(Ws, C, C / Ws, dev)]
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    score, cost, status = _emd_outputs(B, dev, return_cost, return_status)
    hist = torch.empty((B, 2, R * C), dtype=torch.float64, device=dev) if return_hist else None
    L.check(lib.vinet_emd(s.data_ptr(), _is64(s), Hs, Ws, g.data_ptr(), _is64(g), Hg, Wg, B, downsize, R, C, _ptr(wts[0]), _ptr(wts[1]),
                          _ptr(wts[2]), _ptr(wts[3]), ws.data_ptr(), need, score.data_ptr(), _ptr(cost), _ptr(status), _ptr(hist),
                          E._stream_for(dev)), "vinet_emd")
    return _emd_result(score, cost, status, (hist,) if return_hist else ())


@torch.no_grad()
def emd_hist_batch(P, Q, R, C, *, return_cost=False, return_status=False):
    """The solver of `emd_batch` on ready histograms: `P`, `Q` `[B, R*C]` (or `[B,R,C]`), float32 or float64, the bins of an
    R x C grid in row-major order -> float64 `[B]` on the device.  The histograms are taken as they are (FastEMD scales by
    max(sum P, sum Q) itself); negative bins are allowed."""
    R, C = int(R), int(C)
    assert P.shape == Q.shape and P.dim() in (2, 3) and P[0].numel() == R * C, "expected P and Q as [B, R*C]"
    p = _canon(P, (torch.float64,))
    q = _canon(Q, (torch.float64,), maps=p, name="emd_hist: Q")
    B, dev = p.shape[0], p.device
    lib = L.get()
    need = int(lib.vinet_emd_workspace(B, R, C))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    score, cost, status = _emd_outputs(B, dev, return_cost, return_status)
    L.check(lib.vinet_emd_hist(p.data_ptr(), q.data_ptr(), B, R, C, ws.data_ptr(), need, score.data_ptr(), _ptr(cost), _ptr(status),
                               E._stream_for(dev)), "vinet_emd_hist")
    return _emd_result(score, cost, status)


def emd(saliencyMap, fixationMap, toPlot=False, downsize=32):
    """EMD.m's signature: a 2-D saliency map and a 2-D ground-truth map of any two sizes (or item 0 of 3-D batches, as `auc_judd`
    takes them) -> Python float."""
    if toPlot:
        raise NotImplementedError("emd(toPlot=True) draws with matplotlib on the host; plot the returned score's inputs yourself")
    assert saliencyMap.dim() in (2, 3) and fixationMap.dim() in (2, 3), "expected [H,W] maps or [B,H,W] batches"
    s, f = _first(saliencyMap), _first(fixationMap)
    return float(emd_batch(s, f, downsize=downsize)[0])


@torch.no_grad()
def per_sample(name, s_map, gt):
    """The value of `kldiv` / `cc` / `similarity` / `nss` for every map of the batch on its own: float64 `[B]`, what the batched
    functions average (the forward kernel writes it per sample).  The evaluator needs it to skip NaN frames (diem_val.py:116-129)."""
    assert s_map.size() == gt.size() and s_map.dim() == 3, "expected [B,H,W] maps of equal size"
    which = _WHICH[name]
    s = _canon(s_map, (torch.float32,))
    _, saved = _loss_fwd(which, s, _canon(gt, maps=s, name="per_sample: gt"))
    return saved.view(s.shape[0], 8)[:, 2 if which == 0 else 5].clone()
