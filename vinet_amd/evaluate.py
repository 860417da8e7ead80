"""Score saved saliency maps against ground truth -- the counterpart of the reference's validation loop
(diem_val.py:75-172) for maps that are already on disk (what generate_result*.py wrote).

    python -m vinet_amd.evaluate --pred_dir P --gt_dir G [--fix_dir F] [--batch 64] [--blur] [--json out.json]
                                 [--sauc [--other_map FILE] [--sauc_splits 100] [--sauc_step 0.1]]
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
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

METRICS = ("SIM", "CC", "NSS", "AUCJ", "KLdiv")          # the order of diem_val.py:163-172, KLdiv appended
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


def frame_metrics(pred_u8, gt_u8, fix_u8, blur=False, noise=None, sauc=None):
    """uint8 device tensors [B,h,w], [B,H,W], [B,H,W] -> {metric: float64 [B] tensor}: diem_val.py:198-221 process() after the
    model call, for a batch.  `noise`: float64 [B,H,W] jitter for AUC-Judd (loss.py:160) or None.  `sauc`: None, or the
    keywords of loss.auc_shuffled_batch (other_map, frame_ids, n_splits, step, seed), which adds "sAUC"."""
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
    return res


class Scores:
    """the sums of diem_val.py:76-86 and :96-100; frames whose SIM, CC or NSS is NaN are skipped and counted.  `sauc=True`
    keeps a sixth column "sAUC" with counts of its own: a scored frame whose sAUC is NaN is left out of that column only."""

    def __init__(self, sauc=False):
        self.sauc = sauc
        self.frame_sum = dict.fromkeys(METRICS, 0.0)
        self.frame_cnt = self.skipped = 0
        self.video_avg_sum = dict.fromkeys(METRICS, 0.0)
        self.num_videos = 0
        self.videos = {}
        self.sauc_sum = self.sauc_video_avg_sum = 0.0
        self.sauc_cnt = self.sauc_skipped = self.sauc_videos = 0

    def add_video(self, name, keys, values, per_frame=False):
        """values: {metric: sequence of per-frame floats}"""
        vsum, cnt, skipped, frames = dict.fromkeys(METRICS, 0.0), 0, 0, {}
        ssum, scnt, sskipped = 0.0, 0, 0
        for i, k in enumerate(keys):
            row = {m: float(values[m][i]) for m in METRICS + (("sAUC",) if self.sauc else ())}
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
            if self.sauc:
                if math.isnan(row["sAUC"]):
                    sskipped += 1
                else:
                    ssum += row["sAUC"]
                    scnt += 1
        self.frame_cnt += cnt
        self.skipped += skipped
        rec = {"frames": cnt, "skipped": skipped}
        if self.sauc:
            self.sauc_sum += ssum
            self.sauc_cnt += scnt
            self.sauc_skipped += sskipped
            rec.update(sauc_frames=scnt, sauc_skipped=sskipped)
            if scnt:
                rec["sAUC"] = ssum / scnt
                self.sauc_video_avg_sum += rec["sAUC"]
                self.sauc_videos += 1
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
        if self.sauc:
            s["frame_weighted"]["sAUC"] = self.sauc_sum / self.sauc_cnt if self.sauc_cnt else nan
            s["video_averaged"]["sAUC"] = self.sauc_video_avg_sum / self.sauc_videos if self.sauc_videos else nan
            s.update(sauc_frames=self.sauc_cnt, sauc_skipped=self.sauc_skipped, sauc_videos=self.sauc_videos)
        return s

    def report(self, out=None):
        s = self.summary()
        cols = METRICS + (("sAUC",) if self.sauc else ())
        for m in cols:
            print("%s:" % m, s["frame_weighted"][m], file=out)
        for m in cols:
            print("Avg Video %s:" % m, s["video_averaged"][m], file=out)
        if self.sauc:
            print("sAUC frames scored: %d, skipped (NaN sAUC only): %d, videos: %d" % (s["sauc_frames"], s["sauc_skipped"], s["sauc_videos"]), file=out)
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


def evaluate(videos, device, batch=64, blur=False, jitter=True, per_frame=False, seed=0, sauc=None):
    """videos: collect()'s paths or synthetic_videos()'s arrays -> Scores.  `sauc`: None, or a dict with `n_splits`, `step` and
    `other_map` (uint8 [H,W] array for every video, or None for each video's own union)"""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    scores = Scores(sauc=sauc is not None)
    cols = METRICS + (("sAUC",) if sauc is not None else ())
    frame_no = 0          # the running frame number of the run: the frame id of the sAUC draw
    for name, frames in videos:
        print("=" * 25)
        print('processing ' + name, flush=True)
        vals, keys = {m: [] for m in cols}, []
        if sauc is not None:
            other = sauc.get("other_map")
            other = video_other_map(frames) if other is None else other
            other_dev = torch.from_numpy(other).to(device)
        loaded = ((k, p if isinstance(p, np.ndarray) else load_gray(p), g if isinstance(g, np.ndarray) else load_gray(g),
                   f if isinstance(f, np.ndarray) else load_fixation(f)) for k, p, g, f in frames)
        for chunk in _batches(loaded, batch):
            for k, p, g, f in chunk:
                assert g.shape == f.shape, "evaluate: %s / %s: ground truth %s and fixation map %s differ in size" % (name, k, g.shape, f.shape)
            up = lambda j: torch.from_numpy(np.stack([c[j] for c in chunk])).to(device)
            gt_u8 = up(2)
            noise = torch.rand(gt_u8.shape, dtype=torch.float64, device=device, generator=gen) / 1e7 if jitter else None
            if sauc is None:
                res = frame_metrics(up(1), gt_u8, up(3), blur=blur, noise=noise)
            else:
                assert tuple(other.shape) == tuple(gt_u8.shape[1:]), "evaluate --sauc: %s: other map %s, frames %s" % (name, other.shape, tuple(gt_u8.shape[1:]))
                ids = torch.arange(frame_no, frame_no + len(chunk), dtype=torch.int64, device=device)
                res = frame_metrics(up(1), gt_u8, up(3), blur=blur, noise=noise,
                                    sauc=dict(other_map=other_dev, frame_ids=ids, n_splits=sauc["n_splits"], step=sauc["step"], seed=seed))
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
    p.add_argument('--seed', default=0, type=int, help="seed of the jitter noise and of the sAUC draw")
    p.add_argument('--sauc', action='store_true', help="add the shuffled AUC (AUC_shuffled.m as eval_diem.m calls it) as the column sAUC")
    p.add_argument('--other_map', default=None, type=str, help="--sauc: one .npy / .png other-fixation map for every video (default: each video's union)")
    p.add_argument('--sauc_splits', default=100, type=int, help="--sauc: random splits per frame (AUC_shuffled.m Nsplits)")
    p.add_argument('--sauc_step', default=0.1, type=float, help="--sauc: threshold step (AUC_shuffled.m stepSize)")
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
    scores = evaluate(videos, torch.device(args.device), batch=args.batch, blur=args.blur, jitter=bool(args.jitter),
                      per_frame=args.per_frame, seed=args.seed, sauc=sauc)
    s = scores.report()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(s, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
