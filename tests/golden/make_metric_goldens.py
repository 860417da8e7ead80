#!/usr/bin/env python3
"""Generate tests/golden/auc_judd.npz FROM THE REAL REFERENCE (loss.py:122-213, imported unmodified).

Runs only where the reference tree exists (never on the GPU machine).  Same stub trick as make_goldens.py: empty cv2 /
torchvision packages ahead of the reference on sys.path.  For every case of tests/metric_cases.py it
  1. builds the maps from vinet_amd/synth.py and draws the fixations;
  2. scores every map with the reference's auc_judd (jitter=False; for the jitter case `np.random.random` is replaced by a
     function that returns the recorded synth noise, so the reference and the device see the same noise);
  3. computes `above_i = #{S >= t_i}` from the same normalised map by sorting, and REFUSES to write unless the reference's
     score is reproduced from those counts to the last bit;
  4. for the cases with `jitter_runs`: runs the reference that many times with seeded np.random noise and stores the minimum
     and maximum score per map.
Stored: fixation indices, `above`, scores (data only).

Usage:  python tests/golden/make_metric_goldens.py [/path/to/reference]
"""
import contextlib
import io
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests import auc_model as M
from tests import metric_cases as MC
from tests.golden import make_goldens as MG


def _reference(RL, s, f, noise=None):
    """loss.auc_judd on one [H,W] pair, its prints swallowed; `noise`: what np.random.random returns (else jitter=False)"""
    real = np.random.random
    if noise is not None:
        np.random.random = lambda shape: noise.reshape(shape)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return float(RL.auc_judd(torch.from_numpy(s), torch.from_numpy(f), jitter=noise is not None))
    finally:
        np.random.random = real


def _above(s, f, noise):
    """#{S >= t_i} for the descending thresholds, by sorting the reference's own normalised map (loss.py:160-164, 171-178)"""
    S = s if noise is None else s + noise / 10 ** 7
    S = ((S - S.min()) / (S.max() - S.min())).flatten()
    t = np.array(sorted(S[f.flatten() > 0], reverse=True))
    return S.size - np.searchsorted(np.sort(S), t, side="left")


def main():
    if len(sys.argv) > 1:
        MG.REF = sys.argv[1]
    MG._install_stubs()
    import loss as RL
    res, meta = {}, {"numpy": np.__version__, "cases": {}}
    for name, c in MC.CASES.items():
        t0 = time.time()
        s = MC.maps(name)
        idx = MC.draw_fixations(name, s)
        fix = MC.synth.fixation_maps(idx, c["H"], c["W"], dtype=np.dtype(c.get("fix_dtype", "float32")))
        raw = MC.synth.jitter_noise("auc_" + name, c["B"], c["H"], c["W"], c["seed"]) if c.get("jitter") else None
        scores, above = [], []
        for b in range(c["B"]):
            r = _reference(RL, s[b], fix[b], None if raw is None else raw[b])
            scores.append(r)
            if r != r:
                above.append(np.zeros(0, dtype=np.int64))
                continue
            a = _above(s[b], fix[b], None if raw is None else raw[b])
            mine = M.score_from_above(a, s[b].size)
            if mine != r:
                raise SystemExit("%s[%d]: the counts do not reproduce the reference: %.17g vs %.17g" % (name, b, mine, r))
            above.append(a)
        extra = {}
        if c.get("jitter_runs"):
            runs = np.empty((c["jitter_runs"], c["B"]))
            for k in range(c["jitter_runs"]):
                np.random.seed(1000 + k)
                for b in range(c["B"]):
                    with contextlib.redirect_stdout(io.StringIO()):
                        runs[k, b] = float(RL.auc_judd(torch.from_numpy(s[b]), torch.from_numpy(fix[b]), jitter=True))
            extra = {"jitter_min": runs.min(0), "jitter_max": runs.max(0)}
            nojit = [_reference(RL, s[b], fix[b]) for b in range(c["B"])]
            extra["score_nojitter"] = np.array(nojit)
        res.update(MC.pack(name, idx, above, scores, extra))
        meta["cases"][name] = dict(c, scores=[None if v != v else v for v in scores], seconds=round(time.time() - t0, 1))
        print(name, scores, {k: v.tolist() for k, v in extra.items()}, "%.1f s" % (time.time() - t0), flush=True)
    res["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(MC.FIXTURE, **res)
    print("wrote", MC.FIXTURE, os.path.getsize(MC.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
