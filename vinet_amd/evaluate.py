"""Score saved saliency maps against ground truth -- the counterpart of the reference's validation loop
(diem_val.py:75-172) for maps that are already on disk (what generate_result*.py wrote).

    python -m vinet_amd.evaluate --pred_dir P --gt_dir G [--fix_dir F] [--batch 64] [--blur] [--json out.json]
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


def frame_metrics(pred_u8, gt_u8, fix_u8, blur=False, noise=None):
    """uint8 device tensors [B,h,w], [B,H,W], [B,H,W] -> {metric: float64 [B] tensor}: diem_val.py:198-221 process() after the
    model call, for a batch.  `noise`: float64 [B,H,W] jitter for AUC-Judd (loss.py:160) or None."""
    from . import loss, preprocess, utils
    size = tuple(gt_u8.shape[1:])
    if blur:
        s = utils.resize_blur(pred_u8.float(), size)
    elif tuple(pred_u8.shape[1:]) != size:
        s = preprocess.gt_to_tensor(pred_u8.contiguous(), size)          # (/ 255: every metric here is scale-invariant)
    else:
        s = pred_u8.float()
    gt, fix = gt_u8.float(), fix_u8.float()
    return {"SIM": loss.per_sample("similarity", s, gt), "CC": loss.per_sample("cc", s, gt), "NSS": loss.per_sample("nss", s, fix),
            "AUCJ": loss.auc_judd_batch(s, fix, noise=noise), "KLdiv": loss.per_sample("kldiv", s, gt)}


class Scores:
    """the sums of diem_val.py:76-86 and :96-100; frames whose SIM, CC or NSS is NaN are skipped and counted"""

    def __init__(self):
        self.frame_sum = dict.fromkeys(METRICS, 0.0)
        self.frame_cnt = self.skipped = 0
        self.video_avg_sum = dict.fromkeys(METRICS, 0.0)
        self.num_videos = 0
        self.videos = {}

    def add_video(self, name, keys, values, per_frame=False):
        """values: {metric: sequence of per-frame floats}"""
        vsum, cnt, skipped, frames = dict.fromkeys(METRICS, 0.0), 0, 0, {}
        for i, k in enumerate(keys):
            row = {m: float(values[m][i]) for m in METRICS}
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
        self.frame_cnt += cnt
        self.skipped += skipped
        rec = {"frames": cnt, "skipped": skipped}
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
        return {"frames": self.frame_cnt, "skipped": self.skipped, "num_videos": self.num_videos,
                "frame_weighted": {m: self.frame_sum[m] / self.frame_cnt if self.frame_cnt else nan for m in METRICS},
                "video_averaged": {m: self.video_avg_sum[m] / self.num_videos if self.num_videos else nan for m in METRICS},
                "videos": self.videos}

    def report(self, out=None):
        s = self.summary()
        for m in METRICS:
            print("%s:" % m, s["frame_weighted"][m], file=out)
        for m in METRICS:
            print("Avg Video %s:" % m, s["video_averaged"][m], file=out)
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


def evaluate(videos, device, batch=64, blur=False, jitter=True, per_frame=False, seed=0):
    """videos: collect()'s paths or synthetic_videos()'s arrays -> Scores"""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    scores = Scores()
    for name, frames in videos:
        print("=" * 25)
        print('processing ' + name, flush=True)
        vals, keys = {m: [] for m in METRICS}, []
        loaded = ((k, p if isinstance(p, np.ndarray) else load_gray(p), g if isinstance(g, np.ndarray) else load_gray(g),
                   f if isinstance(f, np.ndarray) else load_fixation(f)) for k, p, g, f in frames)
        for chunk in _batches(loaded, batch):
            for k, p, g, f in chunk:
                assert g.shape == f.shape, "evaluate: %s / %s: ground truth %s and fixation map %s differ in size" % (name, k, g.shape, f.shape)
            up = lambda j: torch.from_numpy(np.stack([c[j] for c in chunk])).to(device)
            gt_u8 = up(2)
            noise = torch.rand(gt_u8.shape, dtype=torch.float64, device=device, generator=gen) / 1e7 if jitter else None
            res = frame_metrics(up(1), gt_u8, up(3), blur=blur, noise=noise)
            for m in METRICS:
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
    p.add_argument('--seed', default=0, type=int, help="seed of the jitter noise")
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
    scores = evaluate(videos, torch.device(args.device), batch=args.batch, blur=args.blur, jitter=bool(args.jitter),
                      per_frame=args.per_frame, seed=args.seed)
    s = scores.report()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(s, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
