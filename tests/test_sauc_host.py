"""Shuffled AUC without a GPU: the numpy statement of the definition (tests/sauc_model.py) on cases worked out by hand, the
`>=` semantics on values that sit on a threshold, the C ABI's argument checks, and the evaluator's --sauc path (the per-video
union, --other_map, the NaN accounting, the unchanged default output) with the metric functions replaced by the model."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import sauc_model as SM
from tests import test_metrics_host as TH
from vinet_amd import _lib as L


def _all(idx, n_splits=3):
    """a sample table that takes the whole of `idx` in every split"""
    return np.tile(np.asarray(idx, dtype=np.int32), (n_splits, 1))


def test_fixations_at_the_maximum_and_others_at_the_minimum_score_exactly_one():
    s = np.full((4, 6), 3.0, dtype=np.float32)
    s[0, :3] = 9.0                       # the maximum: the fixations
    s[3, :3] = 1.0                       # the minimum: the whole other set
    f = np.zeros((4, 6)); f[0, :3] = 1
    o = np.zeros((4, 6)); o[3, :3] = 1
    _, oth = SM.other_set(f, o)
    score, n, m = SM.auc_shuffled(s, f, o, _all(oth))
    assert (n, m) == (3, 3) and score == 1.0


def test_other_set_with_the_fixations_values_scores_exactly_one_half():
    """a left-right symmetric map, fixations on the left, the other set at the mirrored pixels: tp == fp at every threshold,
    and with N = 4 every coordinate is a multiple of 1/4, so the trapezoid sum is exact"""
    left = np.array([[0, 10, 40, 20], [90, 30, 0, 70], [55, 100, 5, 0]], dtype=np.float32)
    s = np.concatenate([left, left[:, ::-1]], axis=1)
    f = np.zeros(s.shape); o = np.zeros(s.shape)
    for r, c in ((0, 1), (1, 0), (1, 3), (2, 1)):
        f[r, c] = 1
        o[r, 7 - c] = 1
    _, oth = SM.other_set(f, o)
    for step in (0.1, 0.25, 0.01):
        score, n, m = SM.auc_shuffled(s, f, o, _all(oth), step=step)
        assert (n, m) == (4, 4) and score == 0.5, (step, score)


def test_three_by_four_map_worked_out_by_hand():
    """S / 8 is exact in binary and so are the thresholds of step 0.25 = 1, .75, .5, .25, 0:

        S = 0 1 2 3      normalised  0    .125 .25  .375     pixel index  0 1 2  3
            4 5 6 7                  .5   .625 .75  .875                  4 5 6  7
            8 2 6 4                  1    .25  .75  .5                    8 9 10 11

    fixations at pixels 8, 6, 2: Sth = {1, .75, .25}, N = 3; tp by descending threshold = 1/3, 2/3, 2/3, 1, 1.
    other map at pixels 0, 1, 4, 5, 6; pixel 6 is a fixation of this map and leaves (eval_diem.m:65): other set {0, 1, 4, 5},
    M = 4, K = 3.
    split A = {0, 1, 4}: curfix {0, .125, .5}, fp = 0, 0, 1/3, 1/3, 1: the curve (0,0) (0,1/3) (0,2/3) (1/3,2/3) (1/3,1) (1,1) (1,1)
        has area 1/3 * 2/3 + 2/3 * 1 = 8/9.
    split B = {1, 4, 5}: curfix {.125, .5, .625}, fp = 0, 0, 2/3, 2/3, 1: (0,0) (0,1/3) (0,2/3) (2/3,2/3) (2/3,1) (1,1) (1,1)
        has area 2/3 * 2/3 + 1/3 * 1 = 7/9.
    score = (8/9 + 7/9) / 2 = 5/6."""
    s = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [8, 2, 6, 4]], dtype=np.float64)
    f = np.zeros(12); f[[8, 6, 2]] = 1
    o = np.zeros(12); o[[0, 1, 4, 5, 6]] = 1
    fm, oth = SM.other_set(f, o)
    assert oth.tolist() == [0, 1, 4, 5]
    sn = SM.normalise(s)
    assert SM.split_auc(sn[fm], sn[[0, 1, 4]], 0.25) == pytest.approx(8 / 9, abs=1e-15)
    assert SM.split_auc(sn[fm], sn[[1, 4, 5]], 0.25) == pytest.approx(7 / 9, abs=1e-15)
    for dtype in (np.float32, np.float64):
        score, n, m = SM.auc_shuffled(s.astype(dtype), f.reshape(3, 4), o.reshape(3, 4), np.array([[0, 1, 4, -1], [1, 4, 5, -1]]), step=0.25)
        assert (n, m) == (3, 4) and score == pytest.approx(5 / 6, abs=1e-15)


def test_values_on_a_threshold_fall_on_the_side_their_rounding_puts_them():
    """uint8-derived maps of range 250: 25 -> 0.1 and 75 -> 0.3.  t_3 = 3 * 0.1 = 0.30000000000000004 in float64.  A float64
    map gives 75 / 250 = 0.3 (0.29999999999999998...) < t_3; a float32 map gives float32(0.3) = 0.30000001192... >= t_3.
    t_1 = 0.1 is exactly the double 25 / 250: equal, so `>=` holds in both dtypes."""
    t = SM.thresholds(0.1)
    assert t.size == 11 and t[3] == 0.30000000000000004 and t[1] == 0.1 and t[10] == 1.0
    vals = np.array([0, 25, 75, 250, 125, 200], dtype=np.float64)
    v64, v32 = SM.normalise(vals), SM.normalise(vals.astype(np.float32)).astype(np.float64)
    assert v64[1] == t[1] and v64[1] >= t[1] and v32[1] > t[1]
    assert v64[2] < t[3] and v32[2] >= t[3]
    # one fixation at the value 75, the other set {0, 25}: only tp at t_3 differs between the dtypes
    s = np.array([[0, 25, 75], [250, 125, 200]], dtype=np.float64)
    f = np.zeros((2, 3)); f[0, 2] = 1
    o = np.zeros((2, 3)); o[0, :2] = 1
    a64 = SM.auc_shuffled(s, f, o, [[0], [1]])[0]
    a32 = SM.auc_shuffled(s.astype(np.float32), f, o, [[0], [1]])[0]
    # N = K = 1.  split {0} (value 0): fp = 0 down to t_0 in both; tp = 1 from t_3 (float32) or from t_2 (float64) on: area 1 both.
    # split {1} (value 0.1 >= t_1): fp = 1 from t_1 on, tp = 1 before that in both: area 1.
    assert a64 == 1.0 and a32 == 1.0
    # with the other location at the value 75 itself and the fixation at 25 the side shows in the score
    f2 = np.zeros((2, 3)); f2[0, 1] = 1
    o2 = np.zeros((2, 3)); o2[0, 2] = 1
    # fixation 0.1: tp = 1 from t_1.  other 0.3: fp = 1 from t_3 (float32) / t_2 (float64) -- before tp rises: area 0 both ways
    assert SM.auc_shuffled(s, f2, o2, [[2]])[0] == 0.0 and SM.auc_shuffled(s.astype(np.float32), f2, o2, [[2]])[0] == 0.0
    sth32, sth64 = np.array([v32[2]]), np.array([v64[2]])
    cur = np.array([t[3]])                                    # a location that sits exactly on t_3
    assert SM.split_auc(sth32, cur, 0.1) == 0.5               # tp and fp rise together: the diagonal
    assert SM.split_auc(sth64, cur, 0.1) == 0.0               # tp rises one threshold later: under the diagonal


def test_nan_rules_and_the_removal_of_own_fixations():
    s = np.arange(12, dtype=np.float32).reshape(3, 4)
    f = np.zeros((3, 4)); f[1, 1] = 1
    o = np.zeros((3, 4)); o[1, 1] = 1; o[2, 2] = 1
    assert SM.auc_shuffled(s, f, o, [[10]])[1:] == (1, 1)                              # the own fixation is not an other location
    assert math.isnan(SM.auc_shuffled(s, np.zeros((3, 4)), o, [[10]])[0])              # no fixation
    assert math.isnan(SM.auc_shuffled(np.ones((3, 4), np.float32), f, o, [[10]])[0])   # constant map
    assert math.isnan(SM.auc_shuffled(s, f, f, [[-1]])[0])                             # empty other set
    bad = s.copy(); bad[0, 0] = np.nan
    assert math.isnan(SM.auc_shuffled(bad, f, o, [[10]])[0])


def test_draw_model_is_a_uniform_choice_without_replacement():
    """the key is a bijection of the pixel index (no ties), every split takes K distinct locations of the other set, and over
    8 frames x 100 splits each of 600 locations is taken Binomial(800, 0.1) times: mean 80, sigma 8.49; all within 6 sigma"""
    p = np.arange(100000)
    assert np.unique(SM.keys(p, 3, 5, 7)).size == p.size
    oth = np.sort(np.random.default_rng(1).choice(48 * 64, 600, replace=False))
    counts = np.zeros(48 * 64, dtype=np.int64)
    for frame in range(8):
        d = SM.draw(oth, 60, seed=0, frame=frame, n_splits=100)
        assert all(np.unique(r).size == 60 for r in d) and np.isin(d, oth).all()
        assert len({r.tobytes() for r in d}) == 100
        np.add.at(counts, d.reshape(-1), 1)
    c = counts[oth]
    sigma = math.sqrt(800 * 0.1 * 0.9)
    assert c.sum() == 800 * 60 and abs(c - 80).max() <= 6 * sigma, (c.min(), c.max())
    assert not np.array_equal(SM.draw(oth, 60, 0, 0, 2), SM.draw(oth, 60, 1, 0, 2))


def test_library_exports_and_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "vinet_auc_shuffled") and hasattr(raw, "vinet_auc_shuffled_workspace")
    assert lib.vinet_abi_version() == 16
    need = lib.vinet_auc_shuffled_workspace(2, 1000, 100, 0.1)
    assert need >= 2 * (100 * 8 + 1000 * 4 + 12 * 4)
    for bad in ((0, 1000, 100, 0.1), (2, 0, 100, 0.1), (2, 1000, 0, 0.1), (2, 1000, 100, 0.0), (2, 1000, 100, 1.5), (2, 1000, 100, 1e-5)):
        assert lib.vinet_auc_shuffled_workspace(*bad) == 0, bad
    p = 4096          # never dereferenced: every call below is rejected before a launch
    ok = dict(s=p, s64=0, fix=p, f64=0, oth=p, okind=0, ostride=0, B=2, n=1000, nsplits=100, step=0.1, seed=0, fid=None, smp=None, kmax=0,
              ws=p, wsb=need, score=p, nfix=p, nother=p, out=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vinet_auc_shuffled(a["s"], a["s64"], a["fix"], a["f64"], a["oth"], a["okind"], a["ostride"], a["B"], a["n"], a["nsplits"],
                                      a["step"], a["seed"], a["fid"], a["smp"], a["kmax"], a["ws"], a["wsb"], a["score"], a["nfix"],
                                      a["nother"], a["out"], a["stream"])

    for bad, word in ((dict(s=None), b"null"), (dict(fix=None), b"null"), (dict(oth=None), b"null"), (dict(score=None), b"null"),
                      (dict(nother=None), b"null"), (dict(B=0), b"positive"), (dict(n=0), b"positive"), (dict(n=-3), b"positive"),
                      (dict(nsplits=0), b"positive"), (dict(step=0.0), b"step"), (dict(step=-0.1), b"step"), (dict(step=1.01), b"step"),
                      (dict(step=float("nan")), b"step"), (dict(step=1e-5), b"thresholds"), (dict(okind=3), b"other_kind"),
                      (dict(ostride=999), b"other_stride"), (dict(smp=p, kmax=0), b"kmax"), (dict(out=p, kmax=0), b"kmax"),
                      (dict(smp=p, out=p, kmax=4), b"samples_out"), (dict(wsb=need - 1), b"workspace"), (dict(ws=None), b"workspace"),
                      (dict(ws=p + 4), b"workspace")):
        assert call(**bad) < 0, bad
        assert word in lib.vinet_last_error(), (bad, lib.vinet_last_error())


def test_python_surface_has_no_cpu_fallback():
    import torch
    from vinet_amd import loss
    assert not L.is_test_double()
    s, f, o = torch.rand(2, 8, 8), (torch.rand(2, 8, 8) > 0.8).float(), (torch.rand(8, 8) > 0.5).to(torch.uint8)
    with pytest.raises(Exception):
        loss.auc_shuffled_batch(s, f, o)
    with pytest.raises(Exception):
        loss.auc_shuffled(s[0], f[0], o)
    with pytest.raises(AssertionError, match="resize the saliency map"):
        loss.auc_shuffled_batch(torch.rand(2, 4, 8), f, o)
    with pytest.raises(AssertionError, match="other_map"):
        loss.auc_shuffled_batch(s, f, o[:4])
    assert not hasattr(loss, "auc_shuff")
    u = loss.shuffle_map(torch.tensor([[[0, 1], [0, 0]], [[0, 0], [2, 0]], [[0, 1], [0, 0]]]))
    assert u.dtype == torch.uint8 and u.tolist() == [[0, 1], [1, 0]]


# ---- the evaluator, metric functions replaced by numpy -----------------------------------------------------------------------------
SEEN = []


def _model_metrics_sauc(pred_u8, gt_u8, fix_u8, blur=False, noise=None, sauc=None):
    """tests/test_metrics_host.py's stand-in plus the sAUC column: the model on the model of the device draw"""
    import torch
    out = TH._model_metrics(pred_u8, gt_u8, fix_u8, blur=blur, noise=noise)
    if sauc is not None:
        other, ids = sauc["other_map"].numpy(), sauc["frame_ids"].tolist()
        SEEN.append((other.copy(), ids, sauc["n_splits"], sauc["step"], sauc["seed"]))
        vals = []
        for p, f, fid in zip(pred_u8.numpy().astype(np.float32), fix_u8.numpy(), ids):
            fm, oth = SM.other_set(f, other)
            k = min(int(fm.sum()), oth.size)
            smp = SM.draw(oth, k, sauc["seed"], fid, sauc["n_splits"]) if k else np.full((sauc["n_splits"], 1), -1)
            vals.append(SM.auc_shuffled(p, f, other, smp, sauc["step"])[0])
        out["sAUC"] = torch.tensor(vals, dtype=torch.float64)
    return out


def _videos_for_sauc():
    """the tiny tree of test_metrics_host, with vidB's second frame fixated on a subset of the first frame's pixels: frame 0001 of
    vidB then has an empty other set (NaN sAUC, every other metric fine), frame 0002 a non-empty one"""
    vids = TH._tiny_videos()
    k1, p1, g1, f1 = vids["vidB"][0]
    k2, p2, g2, f2 = vids["vidB"][1]
    sub = np.zeros_like(f1)
    idx = np.flatnonzero(f1)
    sub.reshape(-1)[idx[:5]] = 1
    vids["vidB"][1] = (k2, p2, g2, sub)
    return vids


def test_evaluator_builds_the_union_per_video_and_accounts_for_nan_sauc(tmp_path, monkeypatch, capsys):
    import torch
    from vinet_amd import evaluate as EV
    vids = _videos_for_sauc()
    P, G = TH._write_tree(str(tmp_path), vids)
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_sauc)
    del SEEN[:]
    collected = EV.collect(P, G)
    scores = EV.evaluate(collected, torch.device("cpu"), batch=2, jitter=False, per_frame=True, seed=4, sauc=dict(n_splits=7, step=0.1, other_map=None))
    s = scores.report()
    text = capsys.readouterr().out
    heads = [l.split(":")[0] for l in text.strip().splitlines()[-14:]]
    assert heads == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "sAUC", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ",
                     "Avg Video KLdiv", "Avg Video sAUC", "sAUC frames scored", "frames scored"]
    # the other map of a batch is the union of ALL fixation maps of its video (the frame's own included: the metric removes them)
    unions = {name: np.max(np.stack([f for _, _, _, f in frames]), axis=0) for name, frames in vids.items()}
    assert [ids for _, ids, *_ in SEEN] == [[0, 1], [2], [3, 4]]                      # running frame numbers, batch = 2
    assert np.array_equal(SEEN[0][0], unions["vidA"]) and np.array_equal(SEEN[1][0], unions["vidA"]) and np.array_equal(SEEN[2][0], unions["vidB"])
    assert all(x[2:] == (7, 0.1, 4) for x in SEEN)
    # vidA 0002 has an empty ground truth: skipped for every column.  vidB 0001: NaN sAUC only.
    assert s["frames"] == 4 and s["skipped"] == 1 and s["sauc_frames"] == 3 and s["sauc_skipped"] == 1 and s["sauc_videos"] == 2
    pf = {name: s["videos"][name]["per_frame"] for name in vids}
    assert math.isnan(pf["vidB"]["0001"]["sAUC"]) and not math.isnan(pf["vidB"]["0001"]["SIM"])
    assert s["videos"]["vidB"]["sauc_skipped"] == 1 and s["videos"]["vidB"]["frames"] == 2
    va = (pf["vidA"]["0001"]["sAUC"] + pf["vidA"]["0003"]["sAUC"]) / 2
    vb = pf["vidB"]["0002"]["sAUC"]
    assert s["videos"]["vidA"]["sAUC"] == pytest.approx(va, rel=1e-12) and s["videos"]["vidB"]["sAUC"] == pytest.approx(vb, rel=1e-12)
    assert s["video_averaged"]["sAUC"] == pytest.approx((va + vb) / 2, rel=1e-12)
    assert s["frame_weighted"]["sAUC"] == pytest.approx((2 * va + vb) / 3, rel=1e-12)
    assert 0.0 <= vb <= 1.0 and 0.0 <= va <= 1.0
    # the five other columns are what they are without --sauc
    monkeypatch.setattr(EV, "frame_metrics", TH._model_metrics)
    plain = EV.evaluate(collected, torch.device("cpu"), batch=2, jitter=False, per_frame=True).summary()
    for m in EV.METRICS:
        assert plain["frame_weighted"][m] == s["frame_weighted"][m] and plain["video_averaged"][m] == s["video_averaged"][m]
    # another batch size: the same frame ids, the same values
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_sauc)
    del SEEN[:]
    s5 = EV.evaluate(collected, torch.device("cpu"), batch=5, jitter=False, per_frame=True, seed=4, sauc=dict(n_splits=7, step=0.1, other_map=None)).summary()
    assert [ids for _, ids, *_ in SEEN] == [[0, 1, 2], [3, 4]]
    assert s5["frame_weighted"]["sAUC"] == s["frame_weighted"]["sAUC"] and all(s5["videos"]["vidA"]["per_frame"][k] == pf["vidA"][k] for k in ("0001", "0003"))


def test_evaluator_other_map_file_replaces_the_union(tmp_path, monkeypatch):
    import json
    from PIL import Image
    from vinet_amd import evaluate as EV
    vids = _videos_for_sauc()
    P, G = TH._write_tree(str(tmp_path), vids)
    other = (np.random.default_rng(3).random((24, 40)) > 0.7).astype(np.uint8)
    npy, png = os.path.join(str(tmp_path), "other.npy"), os.path.join(str(tmp_path), "other.png")
    np.save(npy, other * 3)
    Image.fromarray(other * 255).save(png)
    assert np.array_equal(EV.load_other_map(npy), other) and np.array_equal(EV.load_other_map(png), other)
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_sauc)
    del SEEN[:]
    out = os.path.join(str(tmp_path), "s.json")
    assert EV.main(["--pred_dir", P, "--gt_dir", G, "--batch", "4", "--jitter", "0", "--sauc", "--other_map", npy, "--sauc_splits", "5",
                    "--sauc_step", "0.05", "--seed", "9", "--device", "cpu", "--json", out]) == 0
    assert len(SEEN) == 2 and all(np.array_equal(x[0], other) and x[2:] == (5, 0.05, 9) for x in SEEN)
    s = json.load(open(out))
    assert s["sauc_frames"] == 4 and s["sauc_skipped"] == 0 and "sAUC" in s["frame_weighted"]      # vidB 0001 has other locations now
    with pytest.raises(SystemExit):
        EV.main(["--pred_dir", P, "--gt_dir", G, "--other_map", npy, "--device", "cpu"])


def test_default_output_is_unchanged_without_sauc(tmp_path, monkeypatch, capsys):
    import torch
    from vinet_amd import evaluate as EV
    assert EV.METRICS == ("SIM", "CC", "NSS", "AUCJ", "KLdiv")
    P, G = TH._write_tree(str(tmp_path), TH._tiny_videos())
    monkeypatch.setattr(EV, "frame_metrics", TH._model_metrics)          # the five-argument stand-in: no `sauc` keyword may reach it
    s = EV.evaluate(EV.collect(P, G), torch.device("cpu"), batch=2, jitter=False, per_frame=True).report()
    lines = capsys.readouterr().out.strip().splitlines()
    assert [l.split(":")[0] for l in lines[-11:]] == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "Avg Video SIM", "Avg Video CC", "Avg Video NSS",
                                                     "Avg Video AUCJ", "Avg Video KLdiv", "frames scored"]
    assert not any("sAUC" in l for l in lines)
    assert sorted(s) == ["frame_weighted", "frames", "num_videos", "skipped", "video_averaged", "videos"]
    assert sorted(s["frame_weighted"]) == sorted(EV.METRICS) and sorted(s["video_averaged"]) == sorted(EV.METRICS)
    assert sorted(s["videos"]["vidB"]) == sorted(("frames", "skipped", "per_frame") + EV.METRICS)
    assert sorted(s["videos"]["vidB"]["per_frame"]["0001"]) == sorted(EV.METRICS)
