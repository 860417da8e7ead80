"""Score saved saliency maps against ground truth -- the counterpart of the reference's validation loop
(diem_val.py:75-172) for maps that are already on disk (what generate_result*.py wrote).

    python -m vinet_amd.evaluate --pred_dir P --gt_dir G [--fix_dir F] [--batch 64] [--blur] [--json out.json]
                                 [--sauc [--other_map FILE] [--sauc_splits 100] [--sauc_step 0.1]]
                                 [--borji [--borji_splits 100] [--borji_step 0.1]] [--ig [--baseline FILE]]
                                 [--emd [--emd_downsize 32]]
    python -m vinet_amd.evaluate --synthetic N          (N generated frames, no directory)

    P/<video>/<frame>.png|jpg            predicted maps
    G/<video>/maps/<frame>               ground-truth maps          (DHF1K / Hollywood / UCF layout of dataloader.py)
    F/<video>/fixation/<frame>.png       fixations (or .npy; fixMap_*.mat where scipy.io imports); F defaults to G

Frames of a video are paired by the last `_`-separated token of the file stem (`eyeMap_0012.jpg` <-> `0012.png`,
diem_val.py:204); a frame without its partner is an error that names the file.  Files are decoded on the host (PIL), uploaded
as bytes per batch; the prediction is resized to the ground truth's size (and blurred with --blur) by the device
post-processing, then `similarity`, `cc`, `kldiv`, `nss` and `auc_judd_batch` run per batch.  Frames whose CC, SIM or NSS is
NaN are skipped and counted (diem_val.py:116-129).  Printed: the reference's eight lines (frame-weighted, then
video-averaged) plus a KLdiv line each.

`--sauc` adds the shuffled AUC of the reference's MATLAB evaluation (eval_diem.m:40,64-71 with code_for_Metrics/AUC_shuffled.m)
as the column `sAUC`: a first pass over a video's fixation files builds their union (createShuffmap1.m), or `--other_map`
supplies one dataset-level map; the frame's own fixations are taken out per frame (`loss.auc_shuffled_batch`).  The random
locations are a function of (`--seed`, the running frame number, split, pixel): the result does not depend on `--batch`.  A
frame whose sAUC alone is NaN (no other fixation left) stays in the other means and is left out of the sAUC means, counted
as `sauc_skipped` (eval_diem.m:85 drops NaNs per metric).

`--borji` adds AUC-Borji (code_for_Metrics/AUC_Borji.m, `loss.auc_borji_batch`) as the column `AUCB`; its random locations are
keyed like the sAUC's (`--seed`, the running frame number), on a stream of their own.  `--ig` adds the information gain
(InfoGain.m, `loss.info_gain_batch`) as the column `IG`.  Its baseline is `--baseline FILE` (an image or a .npy array, resized
to the ground truth's size on the device) or, by default, leave-one-video-out: a first pass sums every video's ground-truth
maps on the device, and video v is scored against the total minus its own sum (with a single video: against the total, and
the output says so).  That default needs ground-truth maps of one size.  NaN frames of either column are accounted for as
the sAUC's are: `borji_skipped`, `ig_skipped`.

`--emd` adds the earth mover's distance (code_for_Metrics/EMD.m, `loss.emd_batch`) as the column `EMD`, between the resized
prediction and the ground-truth map: both are brought to ceil(H / d) x ceil(W / d) bins with MATLAB's imresize, d =
`--emd_downsize` (32 as in EMD.m), divided by their sums, and FastEMD's transportation problem is solved exactly on the device.
Lower is better.  A frame whose EMD alone is NaN (a map that sums to zero) is counted as `emd_skipped`, beside `emd_frames` and
`emd_videos`, as the other optional columns are.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

METRICS = ("SIM", "CC", "NSS", "AUCJ", "KLdiv")          # the order of diem_val.py:163-172, KLdiv appended
EXTRA = (("sauc", "sAUC"), ("borji", "AUCB"), ("ig", "IG"), ("emd", "EMD"))          # optional columns (flag, name), each with NaN counts of its own
_IMG = (".png", ".jpg", ".jpeg")


def frame_key(filename):
    return os.path.splitext(os.path.basename(filename))[0].split('_')[-1]


def _files(d, exts):
    if not os.path.isdir(d):
        raise FileNotFoundError("evaluate: directory %s is missing" % d)
    return {frame_key(f): os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(exts)}


def collect(pred_dir, gt_dir, fix_dir=None):
    """-> [(video, [(key, pred_path, gt_path, fix_path)])], videos and frames sorted"""
    fix_dir = fix_dir or gt_dir
    fix_exts = _IMG + (".npy",)
    try:
        import scipy.io  # noqa: F401
        fix_exts += (".mat",)
    except ImportError:
        pass
    videos = []
    for v in sorted(d for d in os.listdir(pred_dir) if os.path.isdir(os.path.join(pred_dir, d))):
        pred = _files(os.path.join(pred_dir, v), _IMG)
        gt = _files(os.path.join(gt_dir, v, "maps"), _IMG)
        fix = _files(os.path.join(fix_dir, v, "fixation"), fix_exts)
        for k, p in pred.items():
            for what, table in (("ground-truth map", gt), ("fixation map", fix)):
                if k not in table:
                    raise FileNotFoundError("evaluate: no %s for %s" % (what, p))
        for what, table in (("ground-truth map", gt), ("fixation map", fix)):
            for k, p in table.items():
                if k not in pred:
                    raise FileNotFoundError("evaluate: no predicted map for %s %s" % (what, p))
        videos.append((v, [(k, pred[k], gt[k], fix[k]) for k in sorted(pred)]))
    return videos


def load_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('L'))


def load_fixation(path):
    """binary fixation map as uint8 [H,W]"""
    if path.endswith(".npy"):
        a = np.load(path)
    elif path.endswith(".mat"):
        import scipy.io as sio
        a = sio.loadmat(path)['eyeMap']          # diem_val.py:194-196
    else:
        a = load_gray(path)
    return (np.asarray(a) > 0).astype(np.uint8)


def synthetic_videos(n):
    """n generated frames in two videos, as in-memory (key, pred, gt, fix) arrays: 112x192 predictions, 224x384 ground truth"""
    from . import synth
    n = max(int(n), 2)
    videos, done = [], 0
    for vi, cnt in enumerate((n // 2, n - n // 2)):
        gt = (synth.saliency_maps("eval_gt%d" % vi, cnt, 224, 384, vi, noise=0.0) * 255).astype(np.uint8)
        pred = synth.saliency_maps("eval_pred%d" % vi, cnt, 112, 192, vi, levels=256).astype(np.uint8)
        idx = synth.fixations("eval_fix%d" % vi, gt, 60, vi)
        fix = synth.fixation_maps(idx, 224, 384, dtype=np.uint8)
        videos.append(("synthetic%d" % vi, [("%04d" % (i + 1), pred[i], gt[i], fix[i]) for i in range(cnt)]))
        done += cnt
    return videos


def frame_metrics(pred_u8, gt_u8, fix_u8, blur=False, noise=None, sauc=None, borji=None, ig=None, emd=None):
    """uint8 device tensors [B,h,w], [B,H,W], [B,H,W] -> {metric: float64 [B] tensor}: diem_val.py:198-221 process() after the
    model call, for a batch.  `noise`: float64 [B,H,W] jitter for AUC-Judd (loss.py:160) or None.  `sauc`: None, or the
    keywords of loss.auc_shuffled_batch (other_map, frame_ids, n_splits, step, seed), which adds "sAUC".  `borji`: None, or the
    keywords of loss.auc_borji_batch (frame_ids, n_splits, step, seed), which adds "AUCB".  `ig`: None, or a dict with the
    `baseline` of loss.info_gain_batch, which adds "IG".  `emd`: None, or a dict with the `downsize` of loss.emd_batch, which adds "EMD"."""
    from . import loss, preprocess, utils
    size = tuple(gt_u8.shape[1:])
    if blur:
        s = utils.resize_blur(pred_u8.float(), size)
    elif tuple(pred_u8.shape[1:]) != size:
        s = preprocess.gt_to_tensor(pred_u8.contiguous(), size)          # (/ 255: every metric here is scale-invariant)
    else:
        s = pred_u8.float()
    gt, fix = gt_u8.float(), fix_u8.float()
    res = {"SIM": loss.per_sample("similarity", s, gt), "CC": loss.per_sample("cc", s, gt), "NSS": loss.per_sample("nss", s, fix),
           "AUCJ": loss.auc_judd_batch(s, fix, noise=noise), "KLdiv": loss.per_sample("kldiv", s, gt)}
    if sauc is not None:
        res["sAUC"] = loss.auc_shuffled_batch(s, fix, **sauc)
    if borji is not None:
        res["AUCB"] = loss.auc_borji_batch(s, fix, **borji)
    if ig is not None:
        res["IG"] = loss.info_gain_batch(s, fix, ig["baseline"])
    if emd is not None:
        res["EMD"] = loss.emd_batch(s, gt, downsize=emd["downsize"])
    return res


class Scores:
    """the sums of diem_val.py:76-86 and :96-100; frames whose SIM, CC or NSS is NaN are skipped and counted.  `sauc=True`,
    `borji=True`, `ig=True` and `emd=True` keep the further columns "sAUC", "AUCB", "IG" and "EMD", each with counts of its own: a scored frame
    whose value in such a column is NaN is left out of that column only."""

    def __init__(self, sauc=False, borji=False, ig=False, emd=False):
        self.sauc, self.borji, self.ig, self.emd = sauc, borji, ig, emd
        self.extra = tuple((flag, col) for flag, col in EXTRA if getattr(self, flag))
        self.cols = METRICS + tuple(col for _, col in self.extra)
        self.frame_sum = dict.fromkeys(METRICS, 0.0)
        self.frame_cnt = self.skipped = 0
        self.video_avg_sum = dict.fromkeys(METRICS, 0.0)
        self.num_videos = 0
        self.videos = {}
        self.notes = {}          # remarks on how a column was computed, carried into the summary
        self.xsum, self.xvideo_avg_sum = dict.fromkeys(self.cols[len(METRICS):], 0.0), dict.fromkeys(self.cols[len(METRICS):], 0.0)
        self.xcnt, self.xskipped, self.xvideos = (dict.fromkeys(self.cols[len(METRICS):], 0) for _ in range(3))

    def add_video(self, name, keys, values, per_frame=False):
        """values: {metric: sequence of per-frame floats}"""
        vsum, cnt, skipped, frames = dict.fromkeys(METRICS, 0.0), 0, 0, {}
        xs = {col: [0.0, 0, 0] for _, col in self.extra}          # sum, scored, skipped
        for i, k in enumerate(keys):
            row = {m: float(values[m][i]) for m in self.cols}
            if per_frame:
                frames[k] = row
            if math.isnan(row["SIM"]) or math.isnan(row["CC"]) or math.isnan(row["NSS"]):
                print("1", name, k)
                print("No saliency")
                skipped += 1
                continue
            for m in METRICS:
                vsum[m] += row[m]
                self.frame_sum[m] += row[m]
            cnt += 1
            for _, col in self.extra:
                if math.isnan(row[col]):
                    xs[col][2] += 1
                else:
                    xs[col][0] += row[col]
                    xs[col][1] += 1
        self.frame_cnt += cnt
        self.skipped += skipped
        rec = {"frames": cnt, "skipped": skipped}
        for flag, col in self.extra:
            xsum, xcnt, xskipped = xs[col]
            self.xsum[col] += xsum
            self.xcnt[col] += xcnt
            self.xskipped[col] += xskipped
            rec.update({flag + "_frames": xcnt, flag + "_skipped": xskipped})
            if xcnt:
                rec[col] = xsum / xcnt
                self.xvideo_avg_sum[col] += rec[col]
                self.xvideos[col] += 1
        if cnt:
            self.num_videos += 1
            for m in METRICS:
                rec[m] = vsum[m] / cnt
                self.video_avg_sum[m] += rec[m]
        else:
            print(name, "has no scorable frame: left out of the video average")
        if per_frame:
            rec["per_frame"] = frames
        self.videos[name] = rec

    def summary(self):
        nan = float("nan")
        s = {"frames": self.frame_cnt, "skipped": self.skipped, "num_videos": self.num_videos,
             "frame_weighted": {m: self.frame_sum[m] / self.frame_cnt if self.frame_cnt else nan for m in METRICS},
             "video_averaged": {m: self.video_avg_sum[m] / self.num_videos if self.num_videos else nan for m in METRICS},
             "videos": self.videos}
        for flag, col in self.extra:
            s["frame_weighted"][col] = self.xsum[col] / self.xcnt[col] if self.xcnt[col] else nan
            s["video_averaged"][col] = self.xvideo_avg_sum[col] / self.xvideos[col] if self.xvideos[col] else nan
            s.update({flag + "_frames": self.xcnt[col], flag + "_skipped": self.xskipped[col], flag + "_videos": self.xvideos[col]})
        s.update(self.notes)
        return s

    def report(self, out=None):
        s = self.summary()
        for m in self.cols:
            print("%s:" % m, s["frame_weighted"][m], file=out)
        for m in self.cols:
            print("Avg Video %s:" % m, s["video_averaged"][m], file=out)
        for key in sorted(self.notes):
            print("%s: %s" % (key, self.notes[key]), file=out)
        for flag, col in self.extra:
            print("%s frames scored: %d, skipped (NaN %s only): %d, videos: %d" % (col, s[flag + "_frames"], col, s[flag + "_skipped"], s[flag + "_videos"]), file=out)
        print("frames scored: %d, skipped (NaN): %d, videos: %d" % (s["frames"], s["skipped"], s["num_videos"]), file=out)
        return s


def _batches(frames, batch):
    """consecutive frames of equal prediction / ground-truth size, at most `batch` of them"""
    cur, shape = [], None
    for f in frames:
        sh = (f[1].shape, f[2].shape)
        if cur and (sh != shape or len(cur) == batch):
            yield cur
            cur = []
        cur.append(f)
        shape = sh
    if cur:
        yield cur


def video_other_map(frames):
    """createShuffmap1.m: the union of a video's fixation maps, uint8 [H,W] -- one pass over the fixation files"""
    union = None
    for k, _, _, f in frames:
        a = f if isinstance(f, np.ndarray) else load_fixation(f)
        a = a > 0
        if union is not None and a.shape != union.shape:
            raise ValueError("evaluate --sauc: the fixation maps of one video differ in size (%s: %s, before %s)" % (k, a.shape, union.shape))
        union = a if union is None else (union | a)
    return union.astype(np.uint8)


def load_other_map(path):
    """--other_map: a .npy array or an image, other fixations where > 0"""
    return (np.asarray(np.load(path) if path.endswith(".npy") else load_gray(path)) > 0).astype(np.uint8)


def load_baseline(path):
    """--baseline: a .npy array or an image -> a 2-D array (uint8 for an image)"""
    a = np.asarray(np.load(path) if path.endswith(".npy") else load_gray(path))
    if a.ndim != 2:
        raise ValueError("evaluate --baseline: %s holds an array of shape %s, expected one [H,W] map" % (path, a.shape))
    return a


def _baseline_for(base, size, device):
    """the --baseline array as a device tensor of the ground truth's `size`: as it is where the sizes agree, else through the
    device resize that the predictions take"""
    if tuple(base.shape) == tuple(size):
        t = torch.from_numpy(np.array(base)).to(device)
        return t if t.dtype in (torch.float32, torch.float64) else t.double()
    if base.dtype != np.uint8:
        raise ValueError("evaluate --baseline: a %s array of size %s cannot be resized to the ground truth's %s; give a uint8 map or one of that size"
                         % (base.dtype, tuple(base.shape), tuple(size)))
    from . import preprocess
    return preprocess.gt_to_tensor(torch.from_numpy(np.array(base)).to(device), size)


def video_gt_sums(videos, device, batch=64):
    """the first pass of the leave-one-video-out baseline: every video's ground-truth maps summed on the device, float64 [H,W]
    each (sums of integers: exact, whatever the batch)"""
    sums, size = [], None
    for name, frames in videos:
        acc = None
        for i in range(0, len(frames), batch):
            maps = [g if isinstance(g, np.ndarray) else load_gray(g) for _, _, g, _ in frames[i:i + batch]]
            for (k, *_), g in zip(frames[i:i + batch], maps):
                size = size or g.shape
                if g.shape != size:
                    raise ValueError("evaluate --ig: the ground-truth maps differ in size (%s / %s: %s, before %s), so there is no "
                                     "leave-one-video-out baseline: give one with --baseline FILE" % (name, k, g.shape, size))
            part = torch.from_numpy(np.stack(maps)).to(device).double().sum(0)
            acc = part if acc is None else acc + part
        sums.append(acc)
    return sums


def evaluate(videos, device, batch=64, blur=False, jitter=True, per_frame=False, seed=0, sauc=None, borji=None, ig=None, emd=None):
    """videos: collect()'s paths or synthetic_videos()'s arrays -> Scores.  `sauc`: None, or a dict with `n_splits`, `step` and
    `other_map` (uint8 [H,W] array for every video, or None for each video's own union).  `borji`: None, or a dict with
    `n_splits` and `step`.  `ig`: None, or a dict with `baseline` (a [H,W] array for every video, or None for leave-one-video-out).
    `emd`: None, or a dict with `downsize`"""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    scores = Scores(sauc=sauc is not None, borji=borji is not None, ig=ig is not None, emd=emd is not None)
    cols = scores.cols
    frame_no = 0          # the running frame number of the run: the frame id of the sAUC and AUC-Borji draws
    base_file = base_sums = base_total = None
    if ig is not None:
        base_file = ig.get("baseline")
        if base_file is None:
            base_sums = video_gt_sums(videos, device, batch)
            filled = [x for x in base_sums if x is not None]          # (a video without frames has no sum and scores nothing)
            assert filled, "evaluate --ig: no ground-truth map to build the baseline from"
            base_total = sum(filled[1:], filled[0])
            scores.notes["ig_baseline"] = ("leave-one-video-out: all other videos' ground-truth maps" if len(videos) > 1 else
                                           "a single video, no other to take the baseline from: its own ground-truth maps")
        base_cache = {}
    for vi, (name, frames) in enumerate(videos):
        print("=" * 25)
        print('processing ' + name, flush=True)
        vals, keys = {m: [] for m in cols}, []
        if sauc is not None:
            other = sauc.get("other_map")
            other = video_other_map(frames) if other is None else other
            other_dev = torch.from_numpy(other).to(device)
        if base_sums is not None:
            base_dev = base_total - base_sums[vi] if len(videos) > 1 and base_sums[vi] is not None else base_total
        loaded = ((k, p if isinstance(p, np.ndarray) else load_gray(p), g if isinstance(g, np.ndarray) else load_gray(g),
                   f if isinstance(f, np.ndarray) else load_fixation(f)) for k, p, g, f in frames)
        for chunk in _batches(loaded, batch):
            for k, p, g, f in chunk:
                assert g.shape == f.shape, "evaluate: %s / %s: ground truth %s and fixation map %s differ in size" % (name, k, g.shape, f.shape)
            up = lambda j: torch.from_numpy(np.stack([c[j] for c in chunk])).to(device)
            gt_u8 = up(2)
            noise = torch.rand(gt_u8.shape, dtype=torch.float64, device=device, generator=gen) / 1e7 if jitter else None
            more = {}
            if sauc is not None or borji is not None:
                ids = torch.arange(frame_no, frame_no + len(chunk), dtype=torch.int64, device=device)
            if sauc is not None:
                assert tuple(other.shape) == tuple(gt_u8.shape[1:]), "evaluate --sauc: %s: other map %s, frames %s" % (name, other.shape, tuple(gt_u8.shape[1:]))
                more["sauc"] = dict(other_map=other_dev, frame_ids=ids, n_splits=sauc["n_splits"], step=sauc["step"], seed=seed)
            if borji is not None:
                more["borji"] = dict(frame_ids=ids, n_splits=borji["n_splits"], step=borji["step"], seed=seed)
            if ig is not None:
                if base_file is not None:
                    size = tuple(gt_u8.shape[1:])
                    if size not in base_cache:
                        base_cache[size] = _baseline_for(base_file, size, device)
                    base_dev = base_cache[size]
                more["ig"] = dict(baseline=base_dev)
            if emd is not None:
                more["emd"] = dict(downsize=emd["downsize"])
            res = frame_metrics(up(1), gt_u8, up(3), blur=blur, noise=noise, **more)
            frame_no += len(chunk)
            for m in cols:
                vals[m].extend(res[m].cpu().tolist())
            keys.extend(c[0] for c in chunk)
        scores.add_video(name, keys, vals, per_frame=per_frame)
    return scores


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument('--pred_dir', type=str)
    p.add_argument('--gt_dir', type=str)
    p.add_argument('--fix_dir', default=None, type=str, help="default: --gt_dir")
    p.add_argument('--batch', default=64, type=int)
    p.add_argument('--blur', action='store_true', help="cv2.GaussianBlur(11x11) after the resize, as diem_val.py:208")
    p.add_argument('--jitter', default=1, type=int, help="AUC-Judd jitter (loss.py:158-160); 0 = off, reproducible to the bit")
    p.add_argument('--seed', default=0, type=int, help="seed of the jitter noise and of the sAUC and AUC-Borji draws")
    p.add_argument('--sauc', action='store_true', help="add the shuffled AUC (AUC_shuffled.m as eval_diem.m calls it) as the column sAUC")
    p.add_argument('--other_map', default=None, type=str, help="--sauc: one .npy / .png other-fixation map for every video (default: each video's union)")
    p.add_argument('--sauc_splits', default=100, type=int, help="--sauc: random splits per frame (AUC_shuffled.m Nsplits)")
    p.add_argument('--sauc_step', default=0.1, type=float, help="--sauc: threshold step (AUC_shuffled.m stepSize)")
    p.add_argument('--borji', action='store_true', help="add AUC-Borji (AUC_Borji.m) as the column AUCB")
    p.add_argument('--borji_splits', default=100, type=int, help="--borji: random splits per frame (AUC_Borji.m Nsplits)")
    p.add_argument('--borji_step', default=0.1, type=float, help="--borji: threshold step (AUC_Borji.m stepSize)")
    p.add_argument('--ig', action='store_true', help="add the information gain (InfoGain.m) as the column IG")
    p.add_argument('--baseline', default=None, type=str, help="--ig: one .npy / image baseline map for every video (default: leave-one-video-out sum of the ground truth)")
    p.add_argument('--emd', action='store_true', help="add the earth mover's distance (EMD.m) as the column EMD")
    p.add_argument('--emd_downsize', default=32, type=int, help="--emd: the maps are resized by 1 / this before the transport problem (EMD.m downsize)")
    p.add_argument('--per_frame', action='store_true', help="keep every frame's values in the JSON")
    p.add_argument('--json', default=None, type=str)
    p.add_argument('--synthetic', default=0, type=int, help="score N generated frames, no directory needed")
    p.add_argument('--device', default="cuda", type=str)
    args = p.parse_args(argv)
    if args.synthetic > 0:
        videos = synthetic_videos(args.synthetic)
    else:
        if not (args.pred_dir and args.gt_dir):
            p.error("--pred_dir and --gt_dir (or --synthetic N)")
        videos = collect(args.pred_dir, args.gt_dir, args.fix_dir)
    sauc = None
    if args.sauc:
        sauc = dict(n_splits=args.sauc_splits, step=args.sauc_step, other_map=load_other_map(args.other_map) if args.other_map else None)
    elif args.other_map:
        p.error("--other_map needs --sauc")
    borji = dict(n_splits=args.borji_splits, step=args.borji_step) if args.borji else None
    ig = None
    if args.ig:
        ig = dict(baseline=load_baseline(args.baseline) if args.baseline else None)
    elif args.baseline:
        p.error("--baseline needs --ig")
    emd = dict(downsize=args.emd_downsize) if args.emd else None
    scores = evaluate(videos, torch.device(args.device), batch=args.batch, blur=args.blur, jitter=bool(args.jitter),
                      per_frame=args.per_frame, seed=args.seed, sauc=sauc, borji=borji, ig=ig, emd=emd)
    s = scores.report()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(s, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
