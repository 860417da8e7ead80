"""The AUC-Judd fixture cases (tests/golden/auc_judd.npz): recipes shared by the generator (tests/golden/make_metric_goldens.py),
the CPU tests and the GPU tests.  Maps come from vinet_amd/synth.py by name and seed; the fixture holds the fixation indices,
N, the `above` counts and the reference's scores."""
import json
import os

import numpy as np

from vinet_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "auc_judd.npz")
LDS_CAP = 4096          # vinet_amd/csrc/metrics.hip: AUC_LDS_CAP (more fixations than this run over the workspace)

# name -> recipe.  `nfix`: fixations per map (a list: per map); `levels`: quantisation; `jitter`: recorded noise is added (fp64 path);
# `special`: per-map construction other than synth.fixations; `fix_dtype`: dtype of the fixation map
CASES = {
    "smooth60":  dict(B=2, H=224, W=384, seed=11, levels=0, nfix=[60, 60]),                       # no ties
    "quant400":  dict(B=2, H=224, W=384, seed=12, levels=256, nfix=[400, 400], jitter_runs=32),   # a saved PNG: heavy ties
    "dhf900":    dict(B=2, H=360, W=640, seed=13, levels=0, nfix=[900, 900]),                     # DHF1K native size
    "jit30":     dict(B=2, H=40, W=56, seed=14, levels=16, nfix=[30, 30], jitter=True, jitter_runs=32),   # fp64 path
    "ends":      dict(B=3, H=40, W=56, seed=15, levels=0, nfix=[1, 5, 5], special=["", "argmax", "argmin"]),
    "large":     dict(B=2, H=1080, W=1920, seed=16, levels=0, nfix=[20000, 6000]),                # above LDS_CAP: workspace path
    "nan":       dict(B=3, H=40, W=56, seed=17, levels=0, nfix=[0, 30, 30], special=["", "constant", ""]),
    "fix64":     dict(B=2, H=40, W=56, seed=18, levels=0, nfix=[30, 30], fix_dtype="float64"),    # DIEM path
}


def maps(name):
    """the case's saliency maps [B,H,W] float32 (numpy)"""
    c = CASES[name]
    s = synth.saliency_maps("auc_" + name, c["B"], c["H"], c["W"], c["seed"], levels=c["levels"])
    for b, sp in enumerate(c.get("special", [])):
        if sp == "constant":
            s[b] = 0.5
    return s


def draw_fixations(name, s):
    """generator side: the fixation indices of a case (the fixture stores them)"""
    c = CASES[name]
    out = []
    for b in range(c["B"]):
        n, sp = c["nfix"][b], (c.get("special") or [""] * c["B"])[b]
        idx = synth.fixations("auc_%s_%d" % (name, b), s[b:b + 1], n, c["seed"])[0] if n else np.zeros(0, dtype=np.int64)
        if sp in ("argmax", "argmin"):
            ext = int(s[b].argmax() if sp == "argmax" else s[b].argmin())
            idx = np.unique(np.concatenate([idx[idx != ext][:n - 1], [ext]]))
        out.append(idx.astype(np.int64))
    return out


def noise(name):
    """recorded jitter of a case, already divided by 1e7 (loss.py:160), or None"""
    c = CASES[name]
    if not c.get("jitter"):
        return None
    return synth.jitter_noise("auc_" + name, c["B"], c["H"], c["W"], c["seed"]) / 10 ** 7


def _enc(a):
    """sorted / monotone int arrays as first differences (they compress to a fraction)"""
    a = np.asarray(a, dtype=np.int64)
    return np.diff(a, prepend=0).astype(np.int32)


def _dec(d):
    return np.cumsum(np.asarray(d, dtype=np.int64))


def pack(name, idx, above, scores, extra=None):
    """generator side: the npz entries of one case"""
    res = {}
    for b in range(CASES[name]["B"]):
        res["%s/fix%d" % (name, b)] = _enc(idx[b])
        res["%s/above%d" % (name, b)] = _enc(above[b])
    res["%s/score" % name] = np.asarray(scores, dtype=np.float64)
    for k, v in (extra or {}).items():
        res["%s/%s" % (name, k)] = np.asarray(v)
    return res


class Case:
    """one fixture case with its inputs rebuilt: s [B,H,W] float32, fix [B,H,W], noise (float64 or None), and the expected
    nfix [B], above (list of int64 arrays), score [B] (float64, NaN where the reference returns NaN)"""

    def __init__(self, name, z):
        c = CASES[name]
        self.name, self.B, self.H, self.W = name, c["B"], c["H"], c["W"]
        self.s = maps(name)
        self.idx = [_dec(z["%s/fix%d" % (name, b)]) for b in range(self.B)]
        self.fix = synth.fixation_maps(self.idx, self.H, self.W, dtype=np.dtype(c.get("fix_dtype", "float32")))
        self.noise = noise(name)
        self.above = [_dec(z["%s/above%d" % (name, b)]) for b in range(self.B)]
        self.score = np.asarray(z["%s/score" % name], dtype=np.float64)
        self.nfix = np.array([len(i) for i in self.idx])
        self.jitter_minmax = (np.asarray(z[name + "/jitter_min"]), np.asarray(z[name + "/jitter_max"])) if (name + "/jitter_min") in z else None


def load(names=None):
    z = np.load(FIXTURE)
    return [Case(n, z) for n in (names or CASES)]


def meta():
    return json.loads(str(np.load(FIXTURE)["meta"]))
