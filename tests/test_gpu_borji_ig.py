"""AUC-Borji and the information gain on the device (vinet_amd/csrc/metrics.hip: split_auc_kernel with BorjiDraw, info_gain_kernel) against
their numpy statements (tests/borji_ig_model.py).

Bounds.  AUC-Borji: `nfix` and every count are integers: exact.  tp and fp are quotients of exact integers and every term of a
split's trapezoid sum is rounded identically on both sides; the only freedom is the order of the fp64 sums: <= 13 terms in [0, 1]
per split (step 0.1; 103 at step 0.01, summed in trees / pairs by both sides), <= 100 splits: error < 100 * 13 * 2^-53 < 2e-13
-> 1e-12 absolute, the tolerance of tests/test_gpu_sauc.py.  The device draw is compared with its model location by location:
exact.
Information gain: an fp64 sum of n <= 86 016 non-negative terms is off by at most n * 2^-53 ~ 1e-11, relative; that enters log2
as about 1.4e-11 absolute; the logarithm's own few ulps on |values| <= 52 add about 1e-14: 1e-9 absolute is two orders above.

Shapes: 3x4 / 2x2 (the hand cases), 24x40 (n = 960 < the 1024 lanes: lanes without a pixel), 36x64 (n = 2304, no multiple of
1024), 224x384 once (the long loops)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import borji_ig_model as BM
from vinet_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
IG_TOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _maps(name, B, H, W, nfix, seed=0, levels=0):
    s = synth.saliency_maps(name, B, H, W, seed, levels=levels).astype(np.float32)
    f = synth.fixation_maps(synth.fixations(name + "f", s, nfix, seed), H, W)
    return s, f


def _samples(f, n_splits, seed):
    """a host-drawn table [B, n_splits, kmax]: per row N locations from all pixels, with replacement, then -1"""
    rng = np.random.default_rng(seed)
    ns = [int((m > 0).sum()) for m in f]
    t = np.full((f.shape[0], n_splits, max(1, max(ns))), -1, dtype=np.int32)
    for b, N in enumerate(ns):
        t[b, :, :N] = rng.integers(0, f[b].size, (n_splits, N))
    return t


def _check_given(s, f, n_splits=100, step=0.1, seed=1, smp=None):
    """the given-samples route on numpy inputs against the model; -> the device scores"""
    from vinet_amd import loss
    dev = _dev()
    smp = _samples(f, n_splits, seed) if smp is None else smp
    got, nfix = loss.auc_borji_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), n_splits=n_splits, step=step,
                                     samples=torch.from_numpy(smp).to(dev), return_counts=True)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (s.shape[0],)
    got, nfix = got.cpu().numpy(), nfix.cpu().numpy()
    for b in range(s.shape[0]):
        want, n = BM.auc_borji(s[b], f[b], smp[b], step)
        print("[%d] N %d step %g device %.17g model %.17g diff %.3g" % (b, nfix[b], step, got[b], want, got[b] - want))
        assert nfix[b] == n
        assert (math.isnan(want) and math.isnan(got[b])) or abs(got[b] - want) <= TOL
    return got


def test_borji_hand_case_on_the_device():
    """tests/test_borji_ig_host.py works it out: areas 8/9, 7/9 and 1/2, their mean 13/18"""
    s = np.array([[[0, 1, 2, 3], [4, 5, 6, 7], [8, 2, 6, 4]]], dtype=np.float32)
    f = np.zeros((1, 12), dtype=np.float32)
    f[0, [8, 6, 2]] = 1
    f = f.reshape(1, 3, 4)
    for rows, want in (([[0, 1, 4]], 8 / 9), ([[4, 4, 0]], 7 / 9), ([[6, 6, 6]], 1 / 2), ([[0, 1, 4], [4, 4, 0], [6, 6, 6]], 13 / 18)):
        smp = np.array([rows], dtype=np.int32)
        for ss in (s, s.astype(np.float64)):
            got = _check_given(ss, f, n_splits=len(rows), step=0.25, smp=smp)
            assert abs(got[0] - want) <= TOL
    top = np.full((1, 4, 6), 3.0, dtype=np.float32)
    top[0, 0, :3], top[0, 3, :3] = 9.0, 1.0
    ft = np.zeros((1, 4, 6), dtype=np.float32)
    ft[0, 0, :3] = 1
    assert _check_given(top, ft, n_splits=2, smp=np.array([[[18, 19, 20], [18, 18, 18]]], dtype=np.int32))[0] == 1.0


def test_borji_given_samples_smooth_maps():
    s, f = _maps("bg_smooth", 3, 36, 64, 70)
    got = _check_given(s, f)
    assert (got > 0.5).all() and (got < 1.0).all()                   # fixations were drawn where the map is high
    _check_given(s, f, n_splits=7, step=0.01)                        # 101 thresholds: the per-lane atomics instead of the ballots
    _check_given(s, f, n_splits=3, step=0.3)                         # 1 / step is no integer: thresholds 0, .3, .6, .9
    s2, f2 = _maps("bg_small", 2, 24, 40, 70)
    _check_given(s2, f2)
    _check_given(s2, f2, n_splits=5, step=0.01)


def test_borji_given_samples_quantised_map_with_values_on_the_thresholds():
    """256 levels: range 255, so every multiple of 51 normalises onto a threshold of step 0.1 (k / 5), 0 and 255 onto thresholds of
    step 0.25, in float32 and in float64, which fall on different sides of k * 0.1 for some k"""
    s, f = _maps("bg_quant", 2, 36, 64, 70)
    lo, hi = s.min(axis=(1, 2), keepdims=True), s.max(axis=(1, 2), keepdims=True)
    s = np.floor((s - lo) / (hi - lo) * 255 + 0.5).astype(np.float32)
    assert all(m.max() == 255 and m.min() == 0 for m in s) and (s % 51 == 0).sum() > 20
    for step in (0.25, 0.1):
        a32 = _check_given(s, f, step=step)
        a64 = _check_given(s.astype(np.float64), f, step=step)
        print("step", step, "float32 maps", a32, "float64 maps", a64)


@pytest.mark.parametrize("nfix", [2, 70, 600])
def test_borji_given_samples_by_number_of_fixations(nfix):
    """2: the smallest N that scores; 70: more than one wave, no multiple of 64; 600: not far below one pass of the 1024 lanes"""
    s, f = _maps("bg_n%d" % nfix, 2, 36, 64, nfix)
    _check_given(s, f, n_splits=20)
    _check_given(s.astype(np.float64), f.astype(np.float64), n_splits=20)
    _check_given(s, f, n_splits=4, step=0.01)


def test_borji_given_samples_large_map():
    s, f = _maps("bg_large", 1, 224, 384, 1500)                       # N > 1024: a second pass over the samples
    _check_given(s, f, n_splits=10)


def _nan_batch():
    s, f = _maps("bg_nan", 5, 24, 40, 40)
    f[0] = 0                                     # no fixation
    keep = np.flatnonzero(f[1])[0]
    f[1] = 0
    f[1].reshape(-1)[keep] = 1                   # one fixation: NaN here (AUC_Borji.m:31), unlike s-AUC
    s[2] = 0.25                                  # constant map
    s[3, 5, 5] = np.nan
    return s, f


def test_borji_nan_rows_beside_valid_rows():
    from vinet_amd import loss
    s, f = _nan_batch()
    got = _check_given(s, f, n_splits=5)
    assert np.isnan(got[:4]).all() and not math.isnan(got[4])
    dev = _dev()
    drawn, nfix, smp = loss.auc_borji_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), n_splits=5, return_samples=True)
    drawn, smp = drawn.cpu().numpy(), smp.cpu().numpy()
    assert nfix.tolist() == [0, 1, 40, 40, 40] and tuple(smp.shape) == (5, 5, 40)
    assert np.isnan(drawn[:4]).all() and (smp[:4] == -1).all() and (smp[4] >= 0).all()
    alone = loss.auc_borji_batch(torch.from_numpy(s[4:]).to(dev), torch.from_numpy(f[4:]).to(dev), n_splits=5, frame_ids=[4])
    assert alone.cpu().numpy().tobytes() == drawn[4:].tobytes()


def _draw(s, f, **kw):
    from vinet_amd import loss
    dev = _dev()
    fid = kw.pop("frame_ids", None)
    if fid is not None:
        fid = torch.tensor(fid, dtype=torch.int64, device=dev)
    score, nfix, smp = loss.auc_borji_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), frame_ids=fid, return_samples=True, **kw)
    return score.cpu().numpy(), nfix.cpu().numpy(), smp.cpu().numpy()


def _check_draw(s, f, n_splits, step=0.1, seed=0, frame_ids=None):
    score, nfix, smp = _draw(s, f, n_splits=n_splits, step=step, seed=seed, frame_ids=frame_ids)
    n = s[0].size
    for b in range(s.shape[0]):
        N = int((f[b] > 0).sum())
        assert nfix[b] == N
        rows = smp[b][:, :N]
        assert (smp[b][:, N:] == -1).all() and (rows >= 0).all() and (rows < n).all()          # every index in [0, n)
        fid = b if frame_ids is None else frame_ids[b]
        assert np.array_equal(rows, BM.draw(n, N, seed, fid, n_splits))                         # the draw is the documented function
        want = BM.auc_borji(s[b], f[b], smp[b], step)[0]
        print("[%d] N %d device %.17g model %.17g diff %.3g" % (b, N, score[b], want, score[b] - want))
        assert abs(score[b] - want) <= TOL
    return score, smp


def test_borji_device_draw_is_the_documented_function_and_the_model_reproduces_the_score():
    from vinet_amd import loss
    s, f = _maps("bd_a", 3, 36, 64, 70)
    a, sa = _check_draw(s, f, 100)
    again, _, sagain = _draw(s, f, n_splits=100)
    assert a.tobytes() == again.tobytes() and np.array_equal(sa, sagain)           # two launches: the same bits
    b, sb = _check_draw(s, f, 100, seed=123456789012345)
    assert not np.array_equal(sa, sb)                                              # another seed: other locations
    _check_draw(s, f, 9, step=0.01, frame_ids=[7, 2 ** 40 + 3, -5])
    s2, f2 = _maps("bd_b", 2, 24, 40, 600)
    _, s600 = _check_draw(s2, f2, 5)
    assert all(np.unique(r).size < 600 for r in s600[0])                           # with replacement: 600 of 960 pixels repeat
    s3, f3 = _maps("bd_c", 1, 224, 384, 1500)
    _check_draw(s3, f3, 4)
    # the same seed does not give the shuffled AUC's locations: every pixel as the other set, K = N = 70
    dev = _dev()
    other = torch.ones(36, 64, dtype=torch.uint8, device=dev)
    ssmp = loss.auc_shuffled_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), other, return_samples=True)[3].cpu().numpy()
    assert ssmp.shape == sa.shape and not np.array_equal(ssmp, sa) and not any(np.array_equal(x, y) for x, y in zip(ssmp[0], sa[0]))


def test_borji_batch_item_equals_the_map_alone_with_its_frame_id():
    s, f = _maps("bd_alone", 4, 24, 40, 50)
    ids = [11, 3, 3, 900]
    whole = _draw(s, f, n_splits=30, seed=5, frame_ids=ids)
    for b in range(4):
        one = _draw(s[b:b + 1], f[b:b + 1], n_splits=30, seed=5, frame_ids=ids[b:b + 1])
        assert one[0].tobytes() == whole[0][b:b + 1].tobytes() and np.array_equal(one[2][0], whole[2][b])
    # the default frame ids are 0 .. B-1: position matters only through them
    d = _draw(s, f, n_splits=30, seed=5)
    assert np.array_equal(d[2][1], _draw(s[1:2], f[1:2], n_splits=30, seed=5, frame_ids=[1])[2][0])
    # 100 copies of map 0 in one launch run 20 split groups per map instead of 30: not a bit moves
    many = _draw(np.repeat(s[:1], 100, 0), np.repeat(f[:1], 100, 0), n_splits=30, seed=5, frame_ids=[11] * 100)
    assert many[0].tobytes() == np.repeat(whole[0][:1], 100).tobytes() and all(np.array_equal(m, whole[2][0]) for m in many[2][::33])


def test_borji_draw_is_uniform_over_all_pixels():
    """8 maps of 24x40 with N = 60, 100 splits: 48 000 draws over n = 960 pixels, 50 expected each.  Pearson's chi-square of the
    pixel counts has 959 degrees of freedom; the bound is that distribution's 1 - 1e-6 quantile, 1181.75 (a correct sampler fails
    once in 10^6 runs; one that favours low indices or never reaches some pixels fails at once).  Fixation pixels are drawn like
    any other."""
    H, W = 24, 40
    s = synth.saliency_maps("bu", 8, H, W, 2).astype(np.float32)
    f = synth.fixation_maps(synth.fixations("buf", s, 60, 2), H, W)
    score, nfix, smp = _draw(s, f, n_splits=100)
    assert (nfix == 60).all() and smp.shape == (8, 100, 60) and (smp >= 0).all() and (smp < H * W).all()
    counts = np.bincount(smp.reshape(-1), minlength=H * W)
    e = 48000 / 960
    chi2 = float(((counts - e) ** 2 / e).sum())
    on_fix = int(sum(np.isin(smp[b], np.flatnonzero(f[b])).sum() for b in range(8)))
    print("pixel counts: min %d max %d chi-square %.1f (959 dof: mean 959, bound 1181.75); draws on fixation pixels %d (expected 3000)"
          % (counts.min(), counts.max(), chi2, on_fix))
    assert counts.sum() == 48000 and chi2 < 1181.75
    # a draw lands on one of the map's 60 fixation pixels with probability 1/16: Binomial(48000, 1/16), sigma 53; 6 sigma
    assert abs(on_fix - 3000) <= 6 * math.sqrt(48000 * (1 / 16) * (15 / 16))


# ---- information gain -------------------------------------------------------------------------------------------------------------
def _check_ig(s, f, base=None):
    from vinet_amd import loss
    dev = _dev()
    bt = None if base is None else torch.from_numpy(base).to(dev)
    got, nfix = loss.info_gain_batch(torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev), bt, return_counts=True)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (s.shape[0],)
    got, nfix = got.cpu().numpy(), nfix.cpu().numpy()
    for b in range(s.shape[0]):
        want = BM.info_gain(s[b], f[b], None if base is None else (base if base.ndim == 2 else base[b]))
        print("[%d] N %d device %.17g model %.17g diff %.3g" % (b, nfix[b], got[b], want, got[b] - want))
        assert nfix[b] == int((f[b] > 0).sum())
        assert (math.isnan(want) and math.isnan(got[b])) or abs(got[b] - want) <= IG_TOL
    return got


def test_info_gain_hand_case_on_the_device():
    s = np.array([[[0, 1], [2, 5]]], dtype=np.float32)
    f = np.array([[[0, 1], [1, 0]]], dtype=np.float32)
    b = np.array([[1, 1], [1, 3]], dtype=np.float32)
    for cast in (np.float32, np.float64):
        assert abs(_check_ig(s.astype(cast), f.astype(cast))[0] + 2.5) <= IG_TOL
        assert abs(_check_ig(s.astype(cast), f, b.astype(cast))[0] - 49.5) <= IG_TOL


@pytest.mark.parametrize("H,W,nfix", [(24, 40, 30), (36, 64, 70), (224, 384, 60)])
def test_info_gain_against_the_model(H, W, nfix):
    B = 3 if H < 224 else 2
    s, f = _maps("ig_%d" % H, B, H, W, nfix)
    base = synth.saliency_maps("ig_base%d" % H, 1, H, W, 9, noise=0.0)[0]          # float32, a centre-prior stand-in
    none = _check_ig(s, f)
    shared = _check_ig(s, f, base)
    assert np.isfinite(none).all() and np.isfinite(shared).all() and not np.array_equal(none, shared)
    per_map = _check_ig(s, f, np.repeat(base[None], B, 0))
    assert shared.tobytes() == per_map.tobytes()                                   # [H,W] for the batch == a copy per map
    assert _check_ig(s, f, base).tobytes() == shared.tobytes()                     # two launches: the same bits
    if H < 224:
        _check_ig(s.astype(np.float64), f.astype(np.float64), base.astype(np.float64))
        _check_ig(s, f.astype(np.float64), base.astype(np.float64))
        own = np.stack([synth.saliency_maps("ig_own%d" % H, B, H, W, 3)[b] for b in range(B)]).astype(np.float64)
        each = _check_ig(s, f, own)                                                # a baseline of its own per map
        assert _check_ig(s[1:2], f[1:2], own[1:2]).tobytes() == each[1:2].tobytes()          # the map alone: the same bits


def test_info_gain_nan_rows_for_each_rule():
    s, f = _maps("ig_nan", 6, 24, 40, 30)
    base = np.repeat(synth.saliency_maps("ig_nanb", 1, 24, 40, 4), 6, 0)
    f[0] = 0                                     # no fixation
    s[1] = 0.5                                   # constant map
    base[2] = 2.0                                # constant baseline
    s[3, 2, 2] = np.nan
    base[4, 7, 7] = np.nan
    got = _check_ig(s, f, base)
    assert np.isnan(got[:5]).all() and np.isfinite(got[5])
    plain = _check_ig(s, f)                      # without a baseline only the map's own rules apply
    assert np.isnan(plain[[0, 1, 3]]).all() and np.isfinite(plain[[2, 4, 5]]).all()


# ---- entry points -----------------------------------------------------------------------------------------------------------------
def test_matlab_signatures_and_messages(capsys):
    from vinet_amd import loss
    dev = _dev()
    s, f = _maps("bm", 2, 24, 40, 30)
    st, ft = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev)
    v = loss.auc_borji(st[0], ft[0])
    assert isinstance(v, float) and v == float(loss.auc_borji_batch(st[:1], ft[:1])[0]) and 0.5 < v < 1.0
    assert v == loss.auc_borji(st, ft, 100, 0.1)                                 # item 0 of a batch, positional Nsplits / stepSize
    assert capsys.readouterr().out == ""
    assert math.isnan(loss.auc_borji(st[0], torch.zeros_like(ft[0])))
    assert capsys.readouterr().out.strip() == "no fixationMap"
    one = torch.zeros_like(ft[0])
    one[3, 3] = 1
    assert math.isnan(loss.auc_borji(st[0], one))                                # AUC_Borji.m:31: `<= 1`
    assert capsys.readouterr().out.strip() == "no fixationMap"
    assert math.isnan(loss.auc_borji(torch.ones_like(st[0]), ft[0]))
    assert capsys.readouterr().out.strip() == "NaN saliencyMap"
    base = torch.from_numpy(synth.saliency_maps("bmb", 1, 24, 40, 4)[0]).to(dev)
    g = loss.info_gain(st[0], ft[0], base)
    assert isinstance(g, float) and g == float(loss.info_gain_batch(st[:1], ft[:1], base)[0]) == loss.info_gain(st, ft, base[None])
    assert loss.info_gain(st[0], ft[0]) == float(loss.info_gain_batch(st[:1], ft[:1])[0]) != g
    with pytest.raises(ValueError, match="baseline on cpu"):
        loss.info_gain_batch(st, ft, base.cpu())
    with pytest.raises(ValueError, match="fix_maps on cpu"):
        loss.auc_borji_batch(st, ft.cpu())


def test_torch_ops_and_opcheck():
    from vinet_amd import loss, ops  # noqa: F401
    dev = _dev()
    s, f = _maps("bop", 2, 24, 40, 30)
    st, ft = torch.from_numpy(s).to(dev), torch.from_numpy(f).to(dev)
    base = torch.from_numpy(synth.saliency_maps("bopb", 1, 24, 40, 4)[0]).to(dev)
    ids = torch.tensor([4, 9], dtype=torch.int64, device=dev)
    got = torch.ops.vinet.auc_borji(st, ft, 20, 0.1, 3, ids)
    assert got.cpu().numpy().tobytes() == loss.auc_borji_batch(st, ft, n_splits=20, seed=3, frame_ids=ids).cpu().numpy().tobytes()
    ig = torch.ops.vinet.info_gain(st, ft, base)
    assert ig.cpu().numpy().tobytes() == loss.info_gain_batch(st, ft, base).cpu().numpy().tobytes()
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.vinet.auc_borji.default, (st, ft, 20, 0.1, 3, ids), test_utils=utils)
    torch.library.opcheck(torch.ops.vinet.auc_borji.default, (st.double(), ft.double(), 5, 0.05, 0, None), test_utils=utils)
    torch.library.opcheck(torch.ops.vinet.info_gain.default, (st, ft, base), test_utils=utils)
    torch.library.opcheck(torch.ops.vinet.info_gain.default, (st.double(), ft, None), test_utils=utils)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.vinet.auc_borji(torch.empty(5, 8, 8), torch.empty(5, 8, 8), 100, 0.1, 0, None)
        assert tuple(out.shape) == (5,) and out.dtype == torch.float64
        out = torch.ops.vinet.info_gain(torch.empty(5, 8, 8), torch.empty(5, 8, 8), torch.empty(8, 8))
        assert tuple(out.shape) == (5,) and out.dtype == torch.float64


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------
def _run(args, timeout=300):
    r = subprocess.run([sys.executable, "-m", "vinet_amd.evaluate"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_evaluator_command_with_borji_ig_and_sauc_on_a_synthetic_tree(tmp_path):
    """the new columns are the models' values on the same files (the prediction resized as the evaluator resizes it, the running
    frame number as frame id, the other video's ground-truth sum as baseline), and --batch 3 / --batch 64 write the same JSON"""
    from tests.test_gpu_metrics import _write_tree
    from vinet_amd import preprocess
    P, G, arrays = _write_tree(str(tmp_path))
    texts = []
    for batch in ("3", "64"):
        out = os.path.join(str(tmp_path), "scores%s.json" % batch)
        stdout = _run(["--pred_dir", P, "--gt_dir", G, "--batch", batch, "--jitter", "0", "--per_frame", "--json", out, "--sauc", "--sauc_splits", "20",
                       "--borji", "--borji_splits", "20", "--ig", "--seed", "3"])
        heads = [l.split(":")[0] for l in stdout.strip().splitlines()[-21:]]
        assert heads == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "sAUC", "AUCB", "IG", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ",
                         "Avg Video KLdiv", "Avg Video sAUC", "Avg Video AUCB", "Avg Video IG", "ig_baseline", "sAUC frames scored",
                         "AUCB frames scored", "IG frames scored", "frames scored"]
        texts.append(open(out).read())
    assert texts[0] == texts[1]
    a = json.loads(texts[0])
    assert a["frames"] == 5 and a["skipped"] == 1 and a["borji_frames"] == 5 and a["borji_skipped"] == 0 and a["ig_frames"] == 5 and a["ig_skipped"] == 0
    assert "leave-one-video-out" in a["ig_baseline"]
    dev = _dev()
    names = sorted({n for n, _ in arrays})
    sums = {name: np.sum([arrays[k][1].astype(np.float64) for k in arrays if k[0] == name], axis=0) for name in names}
    fid = 0
    for name in names:
        base = sums[[n for n in names if n != name][0]]
        for k in sorted(k for n, k in arrays if n == name):
            p, g, f = arrays[(name, k)]
            sm = preprocess.gt_to_tensor(torch.from_numpy(p[None]).to(dev), g.shape)[0].cpu().numpy()
            N = int((f > 0).sum())
            wb = BM.auc_borji(sm, f, BM.draw(f.size, N, 3, fid, 20), 0.1)[0]
            wi = BM.info_gain(sm, f, base)
            row = a["videos"][name]["per_frame"][k]
            print(name, k, fid, "AUCB", row["AUCB"], wb, "IG", row["IG"], wi)
            assert abs(row["AUCB"] - wb) <= TOL and abs(row["IG"] - wi) <= IG_TOL and 0.0 <= wb <= 1.0
            fid += 1


def test_evaluator_synthetic_with_and_without_the_new_flags(tmp_path):
    """--synthetic works with both flags, and without them prints and writes exactly the lines and keys it always did, with the
    values the flagged run has in those columns"""
    o0, o1 = os.path.join(str(tmp_path), "plain.json"), os.path.join(str(tmp_path), "more.json")
    plain = _run(["--synthetic", "4", "--jitter", "0", "--json", o0])
    more = _run(["--synthetic", "4", "--jitter", "0", "--json", o1, "--borji", "--borji_splits", "10", "--ig"])
    s0, s1 = json.load(open(o0)), json.load(open(o1))
    cols = ["SIM", "CC", "NSS", "AUCJ", "KLdiv"]
    want = ["%s: %s" % (m, s0["frame_weighted"][m]) for m in cols] + ["Avg Video %s: %s" % (m, s0["video_averaged"][m]) for m in cols]
    want.append("frames scored: %d, skipped (NaN): %d, videos: %d" % (s0["frames"], s0["skipped"], s0["num_videos"]))
    lines = plain.splitlines()
    assert lines[-11:] == want and [l for l in lines[:-11] if l.startswith("processing")] == ["processing synthetic0", "processing synthetic1"]
    assert list(s0) == ["frames", "skipped", "num_videos", "frame_weighted", "video_averaged", "videos"] and list(s0["frame_weighted"]) == cols
    assert list(s0["videos"]["synthetic0"]) == ["frames", "skipped"] + cols
    assert not any(w in plain for w in ("AUCB", "IG", "baseline"))
    assert all(s1["frame_weighted"][m] == s0["frame_weighted"][m] and s1["video_averaged"][m] == s0["video_averaged"][m] for m in cols)
    assert s1["borji_frames"] == 4 and s1["ig_frames"] == 4 and 0.0 <= s1["frame_weighted"]["AUCB"] <= 1.0 and math.isfinite(s1["frame_weighted"]["IG"])
    assert "AUCB frames scored: 4" in more and "IG frames scored: 4" in more
