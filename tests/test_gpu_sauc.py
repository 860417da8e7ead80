"""Shuffled AUC on the device (vinet_amd/csrc/metrics.hip: sauc_*) against its numpy statement (tests/sauc_model.py).

Bounds.  `nfix`, `nother` and every count are integers: exact.  tp and fp are quotients of exact integers and every term of a
split's trapezoid sum is rounded identically on both sides; the only freedom is the order of the fp64 sums: <= 13 terms in
[0, 1] per split (step 0.1), <= 100 splits: error < 100 * 13 * 2^-53 < 2e-13 -> 1e-12 absolute for every case.  (step 0.01
has 103 terms per split, summed by both sides in trees / pairs: still far below 1e-12.)
The device draw is compared with its model (tests/sauc_model.draw) location by location: exact."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sauc_model as SM
from vinet_amd import _lib as L
from vinet_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_CAP = 8192          # SAUC_LDS_CAP of metrics.hip


def _dev():
    return torch.device("cuda:0")


def _maps(name, B, H, W, nfix, nother, seed=0, levels=0):
    """-> float32 maps [B,H,W], fixation maps (float32), one other map (uint8) drawn where ANOTHER synthetic map is high"""
    s = synth.saliency_maps(name, B, H, W, seed, levels=levels).astype(np.float32)
    f = synth.fixation_maps(synth.fixations(name + "f", s, nfix, seed), H, W)
    so = synth.saliency_maps(name + "o", 1, H, W, seed + 11)
    o = synth.fixation_maps(synth.fixations(name + "of", so, nother, seed + 11), H, W, dtype=np.uint8)[0]
    return s, f, o


def _samples(f, o, n_splits, seed):
    """a host-drawn table [B, n_splits, kmax] for per-map fixation maps `f` and other maps `o` ([H,W] or [B,H,W])"""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(f.shape[0]):
        fm, oth = SM.other_set(f[b], o if o.ndim == 2 else o[b])
        k = min(int(fm.sum()), oth.size)
        rows.append([rng.choice(oth, k, replace=False) for _ in range(n_splits)] if k else [np.zeros(0, np.int64)] * n_splits)
    kmax = max(1, max(r.size for rr in rows for r in rr))
    t = np.full((f.shape[0], n_splits, kmax), -1, dtype=np.int32)
    for b, rr in enumerate(rows):
        for j, r in enumerate(rr):
            t[b, j, :r.size] = r
    return t


def _check_given(s, f, o, n_splits=100, step=0.1, seed=1):
    """the given-samples route on numpy inputs against the model; -> the device scores"""
    from vinet_amd import loss
    dev = _dev()
    smp = _samples(f, o, n_splits, seed)
    got, nfix, noth = loss.auc_shuffled_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(o).to(dev),
                                              n_splits=n_splits, step=step, samples=torch.from_numpy(smp).to(dev), return_counts=True)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (s.shape[0],)
    got, nfix, noth = got.cpu().numpy(), nfix.cpu().numpy(), noth.cpu().numpy()
    for b in range(s.shape[0]):
        want, n, m = SM.auc_shuffled(s[b], f[b], o if o.ndim == 2 else o[b], smp[b], step)
        print("[%d] N %d M %d device %.17g model %.17g diff %.3g" % (b, nfix[b], noth[b], got[b], want, got[b] - want))
        assert (nfix[b], noth[b]) == (n, m)
        assert (math.isnan(want) and math.isnan(got[b])) or abs(got[b] - want) <= TOL
    return got


def test_given_samples_smooth_map():
    s, f, o = _maps("sg_smooth", 3, 90, 160, 60, 600)
    got = _check_given(s, f, o)
    assert (got > 0.5).all() and (got < 1.0).all()                   # fixations were drawn where the map is high
    _check_given(s, f, o, n_splits=7, step=0.01)                     # 101 thresholds: the per-location atomics instead of the ballots
    _check_given(s, f, o, n_splits=3, step=0.3)                      # 1 / step is no integer: thresholds 0, .3, .6, .9


def test_given_samples_quantised_map_with_values_on_the_thresholds():
    """251 levels: range 250, so every multiple of 25 normalises onto a threshold of step 0.1, in float32 and in float64, which
    fall on different sides of k * 0.1 for some k (tests/test_sauc_host.py pins which)"""
    s, f, o = _maps("sg_quant", 2, 48, 64, 60, 600)
    lo, hi = s.min(axis=(1, 2), keepdims=True), s.max(axis=(1, 2), keepdims=True)
    s = np.floor((s - lo) / (hi - lo) * 250 + 0.5).astype(np.float32)
    assert all(m.max() == 250 and m.min() == 0 for m in s) and (s % 25 == 0).sum() > 100
    a32 = _check_given(s, f, o)
    a64 = _check_given(s.astype(np.float64), f, o)
    print("float32 maps", a32, "float64 maps", a64)


def test_given_samples_small_other_set_single_fixation_and_float64_inputs():
    s, f, o = _maps("sg_small", 2, 48, 64, 60, 20)
    _check_given(s, f, o)                                            # K = M < N
    s1, f1, o1 = _maps("sg_one", 2, 48, 64, 1, 300)
    _check_given(s1, f1, o1)                                         # N = 1
    _check_given(s.astype(np.float64), f.astype(np.float64), o.astype(np.float64))
    _check_given(s, f, o.astype(np.float32))


def test_shared_other_map_equals_a_copy_per_map_bit_for_bit():
    s, f, o = _maps("sg_shared", 3, 48, 64, 40, 300)
    a = _check_given(s, f, o)
    b = _check_given(s, f, np.repeat(o[None], 3, 0))
    assert a.tobytes() == b.tobytes()


def test_nan_rows():
    s, f, o = _maps("sg_nan", 4, 48, 64, 40, 300)
    f[0] = 0                                 # no fixation
    s[1] = 0.25                              # constant map
    o3 = np.repeat(o[None], 4, 0)
    o3[2] = (f[2] > 0)                       # the other set is the map's own fixations: empty once they are removed
    got = _check_given(s, f, o3)
    assert np.isnan(got[:3]).all() and not math.isnan(got[3])
    from vinet_amd import loss
    dev = _dev()
    drawn, nfix, noth, smp = loss.auc_shuffled_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(o3).to(dev),
                                                     n_splits=5, return_samples=True)
    drawn = drawn.cpu().numpy()
    assert np.isnan(drawn[:3]).all() and not math.isnan(drawn[3]) and (smp[:3] == -1).all() and noth.tolist()[2] == 0
    snan = s.copy()
    snan[3, 5, 5] = np.nan
    assert torch.isnan(loss.auc_shuffled_batch(torch.from_numpy(snan).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(o3).to(dev), n_splits=5)).all()


@pytest.fixture(scope="module")
def large():
    """360x640, 9000 fixations, an other set of about 20 000: K and M above the LDS capacity of the list"""
    s, f, o = _maps("sg_large", 1, 360, 640, 9000, 22000)
    fm, oth = SM.other_set(f[0], o)
    assert fm.sum() > LDS_CAP and oth.size > LDS_CAP
    return s, f, o


def test_given_samples_large_case(large):
    _check_given(*large, n_splits=10)


def _draw(s, f, o, **kw):
    from vinet_amd import loss
    dev = _dev()
    fid = kw.pop("frame_ids", None)
    if fid is not None:
        fid = torch.tensor(fid, dtype=torch.int64, device=dev)
    score, nfix, noth, smp = loss.auc_shuffled_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(o).to(dev),
                                                     frame_ids=fid, return_samples=True, **kw)
    return score.cpu().numpy(), nfix.cpu().numpy(), noth.cpu().numpy(), smp.cpu().numpy()


def _check_draw(s, f, o, n_splits, step=0.1, seed=0, frame_ids=None):
    score, nfix, noth, smp = _draw(s, f, o, n_splits=n_splits, step=step, seed=seed, frame_ids=frame_ids)
    for b in range(s.shape[0]):
        fm, oth = SM.other_set(f[b], o)
        k = min(int(fm.sum()), oth.size)
        assert (nfix[b], noth[b]) == (int(fm.sum()), oth.size)
        rows = smp[b][:, :k]
        assert (smp[b][:, k:] == -1).all() and (rows >= 0).all()
        assert all(np.unique(r).size == k for r in rows)                           # K distinct locations in every split
        assert np.isin(rows, oth).all() and not fm[rows].any()                     # of the other set, none on a fixation
        assert len({r.tobytes() for r in rows}) == n_splits or k == oth.size       # the splits differ
        fid = b if frame_ids is None else frame_ids[b]
        assert np.array_equal(rows, SM.draw(oth, k, seed, fid, n_splits))          # the draw is the documented function
        want = SM.auc_shuffled(s[b], f[b], o, smp[b], step)[0]
        print("[%d] N %d M %d K %d device %.17g model %.17g diff %.3g" % (b, nfix[b], noth[b], k, score[b], want, score[b] - want))
        assert abs(score[b] - want) <= TOL
    return score, smp


def test_device_draw_selects_k_distinct_other_locations_and_the_model_reproduces_the_score():
    s, f, o = _maps("sd_a", 3, 90, 160, 60, 600)
    a, sa = _check_draw(s, f, o, 100)
    again, sagain = _draw(s, f, o, n_splits=100)[::3]
    assert a.tobytes() == again.tobytes() and np.array_equal(sa, sagain)           # the same seed: the same bits
    b, sb = _check_draw(s, f, o, 100, seed=123456789012345)
    assert not np.array_equal(sa, sb)                                              # another seed: other locations
    _check_draw(s, f, o, 9, step=0.01, frame_ids=[7, 2 ** 40 + 3, -5])
    s2, f2, o2 = _maps("sd_b", 2, 48, 64, 60, 20)
    _check_draw(s2, f2, o2, 5)                                                     # K = M: the whole other set in every split


def test_batch_item_equals_the_map_alone_with_its_frame_id():
    s, f, o = _maps("sd_alone", 4, 48, 64, 50, 500)
    ids = [11, 3, 3, 900]
    whole = _draw(s, f, o, n_splits=20, seed=5, frame_ids=ids)
    for b in range(4):
        one = _draw(s[b:b + 1], f[b:b + 1], o, n_splits=20, seed=5, frame_ids=ids[b:b + 1])
        assert one[0].tobytes() == whole[0][b:b + 1].tobytes() and np.array_equal(one[3][0], whole[3][b])
    # the default frame ids are 0 .. B-1: position matters only through them
    d = _draw(s, f, o, n_splits=20, seed=5)
    assert np.array_equal(d[3][1], _draw(s[1:2], f[1:2], o, n_splits=20, seed=5, frame_ids=[1])[3][0])


def test_lds_route_and_workspace_route_agree_bit_for_bit():
    s, f, o = _maps("sd_routes", 2, 90, 160, 60, 600)
    a = _draw(s, f, o, n_splits=30)
    L.set_option("sauc_ws", 1)
    try:
        w = _draw(s, f, o, n_splits=30)
    finally:
        L.set_option("sauc_ws", 0)
    assert a[0].tobytes() == w[0].tobytes() and np.array_equal(a[3], w[3])


def test_device_draw_large_case_reads_the_list_from_the_workspace(large):
    _check_draw(*large, n_splits=4)


def test_draw_is_uniform_over_the_other_set():
    """8 maps share one other set of M = 600 (none of it on a fixation of any map), K = 60, 100 splits: each location's
    inclusion count over the 800 draws is Binomial(800, 0.1), mean 80, sigma = sqrt(800 * 0.1 * 0.9) = 8.49; every count within
    6 sigma (a correct sampler fails about once in 10^6 runs; one that favours low indices or low key bits fails at once)"""
    H, W = 48, 64
    s = synth.saliency_maps("su", 8, H, W, 2).astype(np.float32)
    f = synth.fixation_maps(synth.fixations("suf", s, 60, 2), H, W)
    free = np.flatnonzero(~(f.reshape(8, -1) > 0).any(0))
    oth = np.sort(np.random.default_rng(7).choice(free, 600, replace=False))
    o = np.zeros(H * W, dtype=np.uint8)
    o[oth] = 1
    score, nfix, noth, smp = _draw(s, f, o.reshape(H, W), n_splits=100)
    assert (nfix == 60).all() and (noth == 600).all() and smp.shape == (8, 100, 60) and (smp >= 0).all()
    counts = np.bincount(smp.reshape(-1), minlength=H * W)
    assert counts.sum() == counts[oth].sum() == 800 * 60
    sigma = math.sqrt(800 * 0.1 * 0.9)
    c = counts[oth]
    print("inclusion counts: min %d max %d mean %.2f std %.2f (binomial sigma %.2f)" % (c.min(), c.max(), c.mean(), c.std(), sigma))
    assert np.abs(c - 80).max() <= 6 * sigma
    # by position in the (sorted) other set: the low and the high half are taken equally often within 6 sigma of their sum
    half = c[:300].sum()
    assert abs(half - 24000) <= 6 * math.sqrt(48000 * 0.25)


def test_matlab_signature_and_messages(capsys):
    from vinet_amd import loss
    dev = _dev()
    s, f, o = _maps("sm", 2, 48, 64, 30, 300)
    st, ft, ot = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(o).to(dev)
    v = loss.auc_shuffled(st[0], ft[0], ot)
    assert isinstance(v, float) and v == float(loss.auc_shuffled_batch(st[:1], ft[:1], ot)[0])
    assert v == loss.auc_shuffled(st, ft, ot, 100, 0.1)                          # item 0 of a batch, positional Nsplits / stepSize
    assert math.isnan(loss.auc_shuffled(st[0], torch.zeros_like(ft[0]), ot))
    assert capsys.readouterr().out.strip() == "no fixationMap"
    assert math.isnan(loss.auc_shuffled(torch.ones_like(st[0]), ft[0], ot))
    assert capsys.readouterr().out.strip() == "NaN saliencyMap"
    u = loss.shuffle_map(ft)
    assert u.dtype == torch.uint8 and np.array_equal(u.cpu().numpy(), (f > 0).any(0).astype(np.uint8))


def test_torch_op_and_opcheck():
    from vinet_amd import loss, ops  # noqa: F401
    dev = _dev()
    s, f, o = _maps("sop", 2, 48, 64, 30, 300)
    st, ft, ot = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(o).to(dev)
    ids = torch.tensor([4, 9], dtype=torch.int64, device=dev)
    got = torch.ops.vinet.auc_shuffled(st, ft, ot, 20, 0.1, 3, ids)
    assert got.cpu().numpy().tobytes() == loss.auc_shuffled_batch(st, ft, ot, n_splits=20, seed=3, frame_ids=ids).cpu().numpy().tobytes()
    torch.library.opcheck(torch.ops.vinet.auc_shuffled.default, (st, ft, ot, 20, 0.1, 3, ids), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.vinet.auc_shuffled.default, (st.double(), ft.double(), ot, 5, 0.05, 0, None), test_utils=("test_schema", "test_faketensor"))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.vinet.auc_shuffled(torch.empty(5, 8, 8), torch.empty(5, 8, 8), torch.empty(8, 8, dtype=torch.uint8), 100, 0.1, 0, None)
        assert tuple(out.shape) == (5,) and out.dtype == torch.float64


def test_evaluator_command_with_sauc_on_a_synthetic_tree(tmp_path):
    """the sAUC lines are printed, the per-frame values are loss.auc_shuffled_batch's on the same maps with the running frame
    number as frame id, and --batch 2 / --batch 5 give the same bits"""
    from tests.test_gpu_metrics import _write_tree
    from vinet_amd import loss, preprocess
    P, G, arrays = _write_tree(str(tmp_path))
    runs = []
    for batch in ("2", "5"):
        out = os.path.join(str(tmp_path), "scores%s.json" % batch)
        cmd = [sys.executable, "-m", "vinet_amd.evaluate", "--pred_dir", P, "--gt_dir", G, "--batch", batch, "--jitter", "0", "--per_frame",
               "--json", out, "--sauc", "--sauc_splits", "20", "--seed", "3"]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        heads = [l.split(":")[0] for l in r.stdout.strip().splitlines()[-14:]]
        assert heads == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "sAUC", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ",
                         "Avg Video KLdiv", "Avg Video sAUC", "sAUC frames scored", "frames scored"]
        runs.append(json.load(open(out)))
    a, b = runs
    assert a["sauc_frames"] == 5 and a["sauc_skipped"] == 0 and a["frames"] == 5 and a["skipped"] == 1
    assert a["frame_weighted"]["sAUC"] == b["frame_weighted"]["sAUC"] and a["video_averaged"]["sAUC"] == b["video_averaged"]["sAUC"]
    dev = _dev()
    names = sorted({n for n, _ in arrays})
    fid = 0
    for name in names:
        keys = sorted(k for n, k in arrays if n == name)
        union = torch.from_numpy(np.stack([arrays[(name, k)][2] for k in keys])).to(dev)
        other = loss.shuffle_map(union)
        for k in keys:
            p, g, f = (torch.from_numpy(x[None]).to(dev) for x in arrays[(name, k)])
            sm = preprocess.gt_to_tensor(p, g.shape[1:])
            want = float(loss.auc_shuffled_batch(sm, f.float(), other, n_splits=20, seed=3, frame_ids=[fid])[0])
            va, vb = a["videos"][name]["per_frame"][k]["sAUC"], b["videos"][name]["per_frame"][k]["sAUC"]
            print(name, k, fid, want, va, vb)
            assert va == want and vb == want and 0.0 <= want <= 1.0
            fid += 1
