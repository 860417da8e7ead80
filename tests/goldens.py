"""Helpers to read tests/golden/*.npz and rebuild the exact weights/inputs the
fixtures were generated with (recipes live in vinet_amd/synth.py)."""
import json
import os

import numpy as np
import torch

from vinet_amd import synth

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# a committed file stays under 1 MiB: a fixture whose compressed arrays exceed PART_BYTES is stored as <name>.npz plus
# <name>.part2.npz, <name>.part3.npz, ... (whole arrays per part); load() merges them back
PART_BYTES = 960 * 1024


class Fixture(dict):
    """the merged arrays of one fixture, read like numpy's NpzFile (z[key], z.files)"""

    @property
    def files(self):
        return list(self)


def _parts(path):
    import glob
    import re
    base = path[:-len(".npz")]
    extra = sorted(glob.glob(glob.escape(base) + ".part*.npz"), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    return [path] + extra


def load(name):
    z = Fixture()
    for p in _parts(os.path.join(GOLDEN_DIR, name + ".npz")):
        with np.load(p) as part:
            for k in part.files:
                assert k not in z, "%s: key %s stored twice" % (p, k)
                z[k] = part[k]
    meta = json.loads(str(z["meta"]))
    return z, meta


def save(path, **arrays):
    """np.savez_compressed, split into parts of at most PART_BYTES compressed (an array larger than that gets a part of its own)"""
    import io
    import zlib
    for p in _parts(path)[1:]:
        os.remove(p)
    groups, cur, size = [], {}, 0
    for k, v in arrays.items():
        b = io.BytesIO()
        np.save(b, np.asanyarray(v))
        n = len(zlib.compress(b.getvalue(), 6))
        if cur and size + n > PART_BYTES:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    groups.append(cur)
    base = path[:-len(".npz")]
    for i, g in enumerate(groups):
        np.savez_compressed(path if i == 0 else "%s.part%d.npz" % (base, i + 1), **g)


def t(arr):
    return torch.from_numpy(np.asarray(arr))


def state_dict_for(model, weight_seed, z=None, meta=None):
    """procedural weights (+ the calibrated head stored in the fixture)."""
    sd = synth.synth_state_dict(model.state_dict(), weight_seed)
    if z is not None and "head_w" in z.files:
        wk = meta.get("head_w_key")
        bk = meta.get("head_b_key")
        if wk is None:  # decoder-only fixture
            wk, bk = "convtsp4.6.weight", "convtsp4.6.bias"
        sd[wk] = t(z["head_w"])
        sd[bk] = t(z["head_b"])
    return sd
