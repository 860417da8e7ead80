#!/usr/bin/env python3
"""maps/s of vinet_amd.loss.auc_judd_batch, auc_shuffled_batch, auc_borji_batch and info_gain_batch on the device, beside their
numpy models (tests/auc_model.py, tests/sauc_model.py, tests/borji_ig_model.py) on the host.

    python tools/metrics_bench.py [--reps 20] [--json out.json] [--forward 1] [--dump out.npz]

Shapes: 224x384 / 60 fixations, 360x640 / 900, 1080x1920 / 20 000 (above the kernel's LDS switch point: workspace route),
each at B = 1 and 64.  s-AUC rows (`--sauc 0` leaves them out): the same shapes with an other set of 600 / 20 000 / 100 000
locations (a frame against its video's union map), 100 splits, step 0.1, the device draw; the host column is the model fed the
model of that draw.  AUC-Borji and information-gain rows (`--borji 0` / `--ig 0` leave them out): the same shapes; AUC-Borji with
100 splits, step 0.1, the device draw; the information gain with one baseline map for the batch.  Every shape is warmed up; a timing is a host clock around `reps` calls that end in a device
synchronise.  `--forward 1` also times the ViNet-32 forward (bf16, 224x384) that produces 64 maps, the yardstick the metric
should stay below.  EMD rows (`--emd 0` leaves them out): `loss.emd_batch` end to end and `loss.emd_hist_batch` (the solver alone)
at 7x12 bins (224x384 maps) and 12x20 bins (360x640) at downsize 32, B = 64 and 256, eight different map pairs repeated over the
batch; the host column is not a model but the CPU time of the reference's own solver on a dense histogram of that grid, as
tests/golden/make_emd_goldens.py recorded it (one core).  `--judd 0` leaves the AUC-Judd rows out.  No GPU: the device columns
fail, nothing falls back.  `--dump FILE.npz` also stores what every row computed, for comparing two builds of the library bit for
bit (VINET_LIB selects one): per row, under "<row>/<name>", the scores of the calls it timed and, for the two drawn metrics, the
samples of one `return_samples` call; the jitter noise is seeded then.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests import auc_model as M
from tests import borji_ig_model as BM
from tests import sauc_model as SM
from vinet_amd import loss, synth

SHAPES = ((224, 384, 60), (360, 640, 900), (1080, 1920, 20000))
SAUC_OTHERS = (600, 20000, 100000)


def _inputs(H, W, nfix, B):
    s1 = synth.saliency_maps("mb", 1, H, W, 1)
    f1 = synth.fixation_maps(synth.fixations("mbf", s1, nfix, 1), H, W)
    return np.repeat(s1, B, 0), np.repeat(f1, B, 0)


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def _keep(dump, row, **results):
    """device results of one row -> dump["<row>/<name>"] (numpy); `row` from the row's own fields"""
    key = "_".join(str(row[k]) for k in ("metric", "H", "W", "B"))
    dump.update({"%s/%s" % (key, name): r.cpu().numpy() for name, r in results.items()})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", default=20, type=int)
    p.add_argument("--json", default=None)
    p.add_argument("--forward", default=0, type=int)
    p.add_argument("--sauc", default=1, type=int)
    p.add_argument("--borji", default=1, type=int)
    p.add_argument("--ig", default=1, type=int)
    p.add_argument("--emd", default=1, type=int)
    p.add_argument("--judd", default=1, type=int)
    p.add_argument("--dump", default=None, help="FILE.npz: the device results of every row")
    args = p.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs the GPU"
    dev = torch.device("cuda:0")
    rows = []
    dump = None
    if args.dump:
        dump = {}
        torch.manual_seed(0)
    for H, W, nfix in (SHAPES if args.judd else ()):
        s1, f1 = _inputs(H, W, nfix, 1)
        t0 = time.perf_counter()
        M.auc_judd_rank(s1[0], f1[0])
        host = time.perf_counter() - t0
        for B in (1, 64):
            s, f = (torch.from_numpy(np.repeat(a, B, 0)).to(dev) for a in (s1, f1))
            noise = torch.rand(s.shape, dtype=torch.float64, device=dev) / 1e7
            reps = max(3, args.reps // (4 if H >= 1080 else 1))
            t32 = _time(lambda: loss.auc_judd_batch(s, f), reps)
            t64 = _time(lambda: loss.auc_judd_batch(s, f, noise=noise), reps)
            rows.append(dict(H=H, W=W, nfix=nfix, B=B, ms_fp32=t32 * 1e3, maps_per_s_fp32=B / t32, ms_jitter_fp64=t64 * 1e3,
                             maps_per_s_jitter_fp64=B / t64, numpy_model_ms_per_map_one_core=host * 1e3))
            print(json.dumps(rows[-1]), flush=True)
            if dump is not None:
                _keep(dump, dict(rows[-1], metric="AUCJ"), fp32=loss.auc_judd_batch(s, f), jitter_fp64=loss.auc_judd_batch(s, f, noise=noise))
    for (H, W, nfix), nother in zip(SHAPES, SAUC_OTHERS if args.sauc else ()):
        s1, f1 = _inputs(H, W, nfix, 1)
        so = synth.saliency_maps("mbo", 1, H, W, 12)
        o1 = synth.fixation_maps(synth.fixations("mbof", so, nother, 12), H, W, dtype=np.uint8)[0]
        fm, oth = SM.other_set(f1[0], o1)
        t0 = time.perf_counter()
        SM.auc_shuffled(s1[0], f1[0], o1, SM.draw(oth, min(int(fm.sum()), oth.size), 0, 0, 100))
        host = time.perf_counter() - t0
        o = torch.from_numpy(o1).to(dev)
        for B in (1, 64):
            s, f = (torch.from_numpy(np.repeat(a, B, 0)).to(dev) for a in (s1, f1))
            reps = max(3, args.reps // (4 if H >= 1080 else 1))
            t32 = _time(lambda: loss.auc_shuffled_batch(s, f, o), reps)
            rows.append(dict(metric="sAUC", H=H, W=W, nfix=nfix, nother=int(oth.size), splits=100, B=B, ms_fp32=t32 * 1e3, maps_per_s_fp32=B / t32,
                             numpy_model_ms_per_map_one_core=host * 1e3))
            print(json.dumps(rows[-1]), flush=True)
            if dump is not None:
                _keep(dump, rows[-1], score=loss.auc_shuffled_batch(s, f, o), samples=loss.auc_shuffled_batch(s, f, o, return_samples=True)[3])
    for H, W, nfix in (SHAPES if args.borji else ()):
        s1, f1 = _inputs(H, W, nfix, 1)
        t0 = time.perf_counter()
        BM.auc_borji(s1[0], f1[0], BM.draw(H * W, nfix, 0, 0, 100))
        host = time.perf_counter() - t0
        for B in (1, 64):
            s, f = (torch.from_numpy(np.repeat(a, B, 0)).to(dev) for a in (s1, f1))
            reps = max(3, args.reps // (4 if H >= 1080 else 1))
            t32 = _time(lambda: loss.auc_borji_batch(s, f), reps)
            rows.append(dict(metric="AUCB", H=H, W=W, nfix=nfix, splits=100, B=B, ms_fp32=t32 * 1e3, maps_per_s_fp32=B / t32,
                             numpy_model_ms_per_map_one_core=host * 1e3))
            print(json.dumps(rows[-1]), flush=True)
            if dump is not None:
                _keep(dump, rows[-1], score=loss.auc_borji_batch(s, f), samples=loss.auc_borji_batch(s, f, return_samples=True)[2])
    for H, W, nfix in (SHAPES if args.ig else ()):
        s1, f1 = _inputs(H, W, nfix, 1)
        b1 = synth.saliency_maps("mbb", 1, H, W, 9, noise=0.0)[0]
        t0 = time.perf_counter()
        BM.info_gain(s1[0], f1[0], b1)
        host = time.perf_counter() - t0
        base = torch.from_numpy(b1).to(dev)
        for B in (1, 64):
            s, f = (torch.from_numpy(np.repeat(a, B, 0)).to(dev) for a in (s1, f1))
            reps = max(3, args.reps // (4 if H >= 1080 else 1))
            t32 = _time(lambda: loss.info_gain_batch(s, f, base), reps)
            rows.append(dict(metric="IG", H=H, W=W, nfix=nfix, B=B, ms_fp32=t32 * 1e3, maps_per_s_fp32=B / t32,
                             numpy_model_ms_per_map_one_core=host * 1e3))
            print(json.dumps(rows[-1]), flush=True)
            if dump is not None:
                _keep(dump, rows[-1], score=loss.info_gain_batch(s, f, base))
    if args.emd:
        z = np.load(os.path.join(ROOT, "tests", "golden", "emd_fastemd.npz"))
        ref = {(m["R"], m["C"]): m["cpu_seconds"] for m in json.loads(str(z["meta"])) if m["name"].startswith("dense_")}
        for H, W in ((224, 384), (360, 640)):
            R, C = -(-H // 32), -(-W // 32)
            g8 = synth.saliency_maps("mbeg", 8, H, W, 3, noise=0.0)
            p8 = synth.saliency_maps("mbep", 8, H, W, 4)
            for B in (64, 256):
                s, g = (torch.from_numpy(np.tile(a, (B // 8, 1, 1))).to(dev) for a in (p8, g8))
                score, status, hist = loss.emd_batch(s, g, return_status=True, return_hist=True)
                assert int(status.abs().sum()) == 0 and bool(torch.isfinite(score).all())
                P, Q = hist[:, 0].contiguous(), hist[:, 1].contiguous()
                reps = max(3, args.reps // 4)
                t_all = _time(lambda: loss.emd_batch(s, g), reps)
                t_solve = _time(lambda: loss.emd_hist_batch(P, Q, R, C), reps)
                rows.append(dict(metric="EMD", H=H, W=W, bins="%dx%d" % (R, C), B=B, ms=t_all * 1e3, maps_per_s=B / t_all,
                                 solver_only_ms=t_solve * 1e3, solver_only_maps_per_s=B / t_solve,
                                 fastemd_cpu_ms_per_map_one_core=ref[(R, C)] * 1e3))
                print(json.dumps(rows[-1]), flush=True)
                if dump is not None:
                    _keep(dump, rows[-1], score=loss.emd_batch(s, g), solver_only=loss.emd_hist_batch(P, Q, R, C))
    if args.forward:
        from vinet_amd import engine, model
        engine.set_default_dtype("bf16")
        m = model.VideoSaliencyModel(num_clips=32)
        m.load_state_dict(synth.synth_state_dict(m.state_dict(), 7))
        m = m.to(dev).eval()
        x = synth.clip(1, 32, 224, 384, 0).permute(0, 2, 1, 3, 4).expand(64, -1, -1, -1, -1).contiguous().to(dev)
        with torch.no_grad():
            t = _time(lambda: m(x), 3)
        rows.append(dict(forward_vinet32_bf16_B64_ms=t * 1e3))
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    if dump is not None:
        np.savez(args.dump, **dump)


if __name__ == "__main__":
    main()
