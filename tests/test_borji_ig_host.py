"""AUC-Borji and the information gain without a GPU: the numpy statements of the definitions (tests/borji_ig_model.py) on cases
worked out by hand, the C ABI's argument checks, and the evaluator's --borji / --ig paths (the leave-one-video-out baseline,
--baseline, the unequal-size error, the NaN accounting per column, the unchanged default output) with the metric functions
replaced by the models."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from tests import borji_ig_model as BM
from tests import sauc_model as SM
from tests import test_metrics_host as TH
from tests import test_sauc_host as TS
from vinet_amd import _lib as L

S34 = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [8, 2, 6, 4]], dtype=np.float64)


def _fix34():
    f = np.zeros(12)
    f[[8, 6, 2]] = 1
    return f.reshape(3, 4)


# ---- AUC-Borji --------------------------------------------------------------------------------------------------------------------
def test_borji_three_by_four_map_worked_out_by_hand():
    """The 3x4 map of tests/test_sauc_host.py, step 0.25 (S / 8 and the thresholds 1, .75, .5, .25, 0 are exact in binary):

        normalised  0    .125 .25  .375     pixel index  0 1 2  3
                    .5   .625 .75  .875                  4 5 6  7
                    1    .25  .75  .5                    8 9 10 11

    fixations at pixels 8, 6, 2: Sth = {1, .75, .25}, N = 3; tp by descending threshold = 1/3, 2/3, 2/3, 1, 1.
    split {0, 1, 4}: curfix {0, .125, .5}, fp = 0, 0, 1/3, 1/3, 1: area 1/3 * 2/3 + 2/3 * 1 = 8/9.
    split {4, 4, 0} (a location twice): curfix {.5, .5, 0}, fp = 0, 0, 2/3, 2/3, 1: area 2/3 * 2/3 + 1/3 * 1 = 7/9.
    split {6, 6, 6} (a fixation pixel, three times): curfix {.75, .75, .75}, fp = 0, 1, 1, 1, 1: the curve (0,0) (0,1/3) (1,2/3)
        (1,2/3) (1,1) (1,1) (1,1) has area 1 * (1/3 + 2/3) / 2 = 1/2.
    The score of the three splits is their mean, (8/9 + 7/9 + 1/2) / 3 = (16 + 14 + 9) / 54 = 39/54 = 13/18.  (The issue that
    asked for this test lists the same three areas and gives 47/54 for their mean: a slip of addition, 16 + 14 + 9 is 39.  The
    three areas determine the mean, so they are asserted as listed and the mean as what they add up to.)"""
    f = _fix34()
    sn = SM.normalise(S34)
    fm = f.reshape(-1) > 0
    for idx, area in (([0, 1, 4], 8 / 9), ([4, 4, 0], 7 / 9), ([6, 6, 6], 1 / 2)):
        assert SM.split_auc(sn[fm], sn[idx], 0.25) == pytest.approx(area, abs=1e-15), idx
        assert BM.auc_borji(S34, f, [idx], 0.25) == (pytest.approx(area, abs=1e-15), 3)
    smp = np.array([[0, 1, 4, -1], [4, 4, 0, -1], [6, 6, 6, -1]])
    for dtype in (np.float32, np.float64):
        score, n = BM.auc_borji(S34.astype(dtype), f, smp, 0.25)
        assert n == 3 and score == pytest.approx((8 / 9 + 7 / 9 + 1 / 2) / 3, abs=1e-15) and score == pytest.approx(13 / 18, abs=1e-15)


def test_borji_fixations_at_the_maximum_and_samples_at_the_minimum_score_exactly_one():
    s = np.full((4, 6), 3.0, dtype=np.float32)
    s[0, :3] = 9.0
    s[3, :3] = 1.0
    f = np.zeros((4, 6)); f[0, :3] = 1
    for step in (0.1, 0.25, 0.01):
        assert BM.auc_borji(s, f, [[18, 19, 20], [18, 18, 18], [20, 19, 19]], step) == (1.0, 3)


def test_borji_nan_rules():
    f1 = np.zeros((3, 4)); f1[2, 0] = 1
    score, n = BM.auc_borji(S34, f1, [[0]], 0.25)
    assert math.isnan(score) and n == 1                                   # AUC_Borji.m:31: one fixation is NaN here, unlike s-AUC
    assert math.isnan(BM.auc_borji(S34, np.zeros((3, 4)), [[-1]], 0.25)[0])
    assert math.isnan(BM.auc_borji(np.ones((3, 4), np.float32), _fix34(), [[0, 1, 2]], 0.25)[0])
    bad = S34.copy(); bad[0, 0] = np.nan
    assert math.isnan(BM.auc_borji(bad, _fix34(), [[0, 1, 2]], 0.25)[0])


def test_borji_draw_model_is_uniform_with_replacement_and_a_stream_of_its_own():
    """indices in [0, n); repeats occur (N = 600 draws from n = 960: a draw without a repeat has probability < 1e-90); over 8 frames x
    100 splits x 60 samples each pixel is hit Binomial(48000, 1/960) times: a chi-square over the 960 pixels with 959 degrees of
    freedom, bound = its 1 - 1e-6 quantile, 1181.75 (Wilson-Hilferty, 959 * (1 - 2/(9*959) + 4.7534 * sqrt(2/(9*959)))^3, gives 1181.84)"""
    d = BM.draw(960, 600, seed=0, frame=0, n_splits=3)
    assert d.dtype == np.int32 and d.shape == (3, 600) and d.min() >= 0 and d.max() < 960
    assert all(np.unique(r).size < 600 for r in d) and (np.diff(d, axis=1) >= 0).all()
    counts = np.zeros(960, dtype=np.int64)
    for frame in range(8):
        np.add.at(counts, BM.draw(960, 60, 0, frame, 100).reshape(-1), 1)
    e = 48000 / 960
    chi2 = float(((counts - e) ** 2 / e).sum())
    assert counts.sum() == 48000 and chi2 < 1181.75, chi2
    assert not np.array_equal(BM.draw(960, 60, 0, 0, 2), BM.draw(960, 60, 1, 0, 2))
    assert not np.array_equal(BM.draw(960, 60, 0, 0, 2), BM.draw(960, 60, 0, 1, 2))
    # not the shuffled AUC's stream: the same keys without the domain constant give other pixels
    plain = np.sort((SM.keys(np.arange(60), 0, 0, 0) * np.uint64(960)) >> np.uint64(32))
    assert not np.array_equal(BM.draw(960, 60, 0, 0, 1)[0], plain)


# ---- information gain -------------------------------------------------------------------------------------------------------------
def test_info_gain_two_by_two_map_worked_out_by_hand():
    """S = [[0,1],[2,5]]: v = 0, .2, .4, 1, sum 1.6, p = 0, 1/8, 1/4, 5/8; fixations at pixels 1 and 2: log2 = -3 and -2: -2.5.
    Baseline [[1,1],[1,3]]: vb = 0, 0, 0, 1 = pb: no mass at the fixations, the term is log2(eps) = -52 each: -2.5 + 52 = 49.5.
    The only deviation is the eps inside the logarithms, of order 1e-15."""
    s = np.array([[0, 1], [2, 5]])
    f = np.array([[0, 1], [1, 0]])
    b = np.array([[1, 1], [1, 3]])
    for dtype in (np.float32, np.float64):
        assert BM.info_gain(s.astype(dtype), f) == pytest.approx(-2.5, abs=1e-12)
        assert BM.info_gain(s.astype(dtype), f, b.astype(dtype)) == pytest.approx(49.5, abs=1e-12)
    assert BM.info_gain(s.astype(np.float64), f, s.astype(np.float64) * 3 + 7) == 0.0          # the map as its own baseline, rescaled


def test_info_gain_nan_rules():
    s = np.array([[0, 1], [2, 5]], dtype=np.float64)
    f = np.array([[0, 1], [1, 0]])
    assert math.isnan(BM.info_gain(s, np.zeros((2, 2))))
    assert math.isnan(BM.info_gain(np.ones((2, 2)), f))
    assert math.isnan(BM.info_gain(s, f, np.full((2, 2), 4.0)))
    bad = s.copy(); bad[1, 1] = np.nan
    assert math.isnan(BM.info_gain(bad, f)) and math.isnan(BM.info_gain(s, f, bad))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_rejects_bad_borji_arguments_without_a_gpu():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(raw, n) for n in ("vinet_auc_borji", "vinet_auc_borji_workspace", "vinet_info_gain"))
    assert lib.vinet_abi_version() == 16
    need = lib.vinet_auc_borji_workspace(2, 1000, 100, 0.1)
    assert 2 * (100 * 8 + 12 * 4) <= need < lib.vinet_auc_shuffled_workspace(2, 1000, 100, 0.1)          # no location list
    for bad in ((0, 1000, 100, 0.1), (2, 0, 100, 0.1), (2, 1000, 0, 0.1), (2, 1000, 100, 0.0), (2, 1000, 100, 1.5), (2, 1000, 100, 1e-5)):
        assert lib.vinet_auc_borji_workspace(*bad) == 0, bad
    p = 4096          # never dereferenced: every call below is rejected before a launch
    ok = dict(s=p, s64=0, fix=p, f64=0, B=2, n=1000, nsplits=100, step=0.1, seed=0, fid=None, smp=None, kmax=0, ws=p, wsb=need, score=p,
              nfix=p, out=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vinet_auc_borji(a["s"], a["s64"], a["fix"], a["f64"], a["B"], a["n"], a["nsplits"], a["step"], a["seed"], a["fid"],
                                   a["smp"], a["kmax"], a["ws"], a["wsb"], a["score"], a["nfix"], a["out"], a["stream"])

    for bad, word in ((dict(s=None), b"null"), (dict(fix=None), b"null"), (dict(score=None), b"null"), (dict(nfix=None), b"null"),
                      (dict(B=0), b"positive"), (dict(n=0), b"positive"), (dict(n=-3), b"positive"), (dict(nsplits=0), b"nsplits"),
                      (dict(nsplits=-1), b"nsplits"), (dict(step=0.0), b"step"), (dict(step=-0.1), b"step"), (dict(step=1.01), b"step"),
                      (dict(step=float("nan")), b"step"), (dict(step=1e-5), b"thresholds"), (dict(smp=p, kmax=0), b"kmax"),
                      (dict(out=p, kmax=0), b"kmax"), (dict(smp=p, out=p, kmax=4), b"samples_out"), (dict(wsb=need - 1), b"workspace"),
                      (dict(ws=None), b"workspace"), (dict(ws=p + 4), b"workspace")):
        assert call(**bad) < 0, bad
        assert word in lib.vinet_last_error() and b"auc_borji" in lib.vinet_last_error(), (bad, lib.vinet_last_error())


def test_library_rejects_bad_info_gain_arguments_without_a_gpu():
    lib = L.load()
    p = 4096
    ok = dict(s=p, s64=0, fix=p, f64=0, base=p, b64=1, bstride=0, B=2, n=1000, score=p, nfix=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vinet_info_gain(a["s"], a["s64"], a["fix"], a["f64"], a["base"], a["b64"], a["bstride"], a["B"], a["n"], a["score"],
                                   a["nfix"], a["stream"])

    for bad, word in ((dict(s=None), b"null"), (dict(fix=None), b"null"), (dict(score=None), b"null"), (dict(nfix=None), b"null"),
                      (dict(B=0), b"positive"), (dict(n=0), b"positive"), (dict(n=-7), b"positive"), (dict(bstride=999), b"baseline_stride"),
                      (dict(bstride=-1), b"baseline_stride")):
        assert call(**bad) < 0, bad
        assert word in lib.vinet_last_error() and b"info_gain" in lib.vinet_last_error(), (bad, lib.vinet_last_error())


def test_python_surface_has_no_cpu_fallback():
    import torch
    from vinet_amd import loss, ops  # noqa: F401
    assert not L.is_test_double()
    s, f = torch.rand(2, 8, 8), (torch.rand(2, 8, 8) > 0.8).float()
    for fn in (lambda: loss.auc_borji_batch(s, f), lambda: loss.auc_borji(s[0], f[0]), lambda: loss.info_gain_batch(s, f),
               lambda: loss.info_gain(s[0], f[0], torch.rand(8, 8)), lambda: torch.ops.vinet.auc_borji(s, f, 10, 0.1, 0, None),
               lambda: torch.ops.vinet.info_gain(s, f, None)):
        with pytest.raises(Exception):
            fn()
    with pytest.raises(AssertionError, match="resize the saliency map"):
        loss.auc_borji_batch(torch.rand(2, 4, 8), f)
    with pytest.raises(AssertionError, match="resize the saliency map"):
        loss.info_gain_batch(torch.rand(2, 4, 8), f)
    with pytest.raises(AssertionError, match="baseline"):
        loss.info_gain_batch(s, f, torch.rand(4, 8))


# ---- the evaluator, metric functions replaced by numpy -----------------------------------------------------------------------------
SEEN = []


def _model_metrics_all(pred_u8, gt_u8, fix_u8, blur=False, noise=None, sauc=None, borji=None, ig=None):
    """tests/test_sauc_host.py's stand-in plus the AUCB and IG columns: the models, AUC-Borji on the model of the device draw"""
    import torch
    out = TS._model_metrics_sauc(pred_u8, gt_u8, fix_u8, blur=blur, noise=noise, sauc=sauc)
    preds, fixes = pred_u8.numpy().astype(np.float32), fix_u8.numpy()
    if borji is not None:
        ids = borji["frame_ids"].tolist()
        SEEN.append(("borji", ids, borji["n_splits"], borji["step"], borji["seed"]))
        vals = []
        for p, f, fid in zip(preds, fixes, ids):
            N = int((f > 0).sum())
            vals.append(BM.auc_borji(p, f, BM.draw(p.size, N, borji["seed"], fid, borji["n_splits"]), borji["step"])[0])
        out["AUCB"] = torch.tensor(vals, dtype=torch.float64)
    if ig is not None:
        base = ig["baseline"].numpy()
        SEEN.append(("ig", base.copy(), str(ig["baseline"].dtype)))
        out["IG"] = torch.tensor([BM.info_gain(p, f, base) for p, f in zip(preds, fixes)], dtype=torch.float64)
    return out


def _three_videos():
    """three in-memory videos of 24x40 frames (2, 3 and 2 of them), as synthetic_videos() hands them over"""
    from vinet_amd import synth
    vids = []
    for vi, cnt in enumerate((2, 3, 2)):
        gt = (synth.saliency_maps("bi_gt%d" % vi, cnt, 24, 40, vi, noise=0.0) * 255).astype(np.uint8)
        pred = synth.saliency_maps("bi_pred%d" % vi, cnt, 24, 40, vi + 5, levels=256).astype(np.uint8)
        fix = synth.fixation_maps(synth.fixations("bi_fix%d" % vi, gt, 12, vi), 24, 40, dtype=np.uint8)
        vids.append(("vid%d" % vi, [("%04d" % (i + 1), pred[i], gt[i], fix[i]) for i in range(cnt)]))
    return vids


def test_evaluator_leave_one_video_out_baseline(monkeypatch, capsys):
    import torch
    from vinet_amd import evaluate as EV
    vids = _three_videos()
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_all)
    del SEEN[:]
    s = EV.evaluate(vids, torch.device("cpu"), batch=2, jitter=False, per_frame=True, ig=dict(baseline=None)).report()
    text = capsys.readouterr().out
    sums = [np.sum([g.astype(np.float64) for _, _, g, _ in frames], axis=0) for _, frames in vids]
    want = [sums[1] + sums[2], sums[0] + sums[2], sums[0] + sums[1]]
    seen = [x for x in SEEN if x[0] == "ig"]
    assert len(seen) == 4 and all(x[2] == "torch.float64" for x in seen)           # batches of 2: 1 + 2 + 1
    for x, v in zip(seen, (0, 1, 1, 2)):
        assert np.array_equal(x[1], want[v]), v                                   # the total minus the video's own sum, exactly
    for (name, frames), base in zip(vids, want):
        for k, p, g, f in frames:
            assert s["videos"][name]["per_frame"][k]["IG"] == BM.info_gain(p.astype(np.float32), f, base)
    assert s["ig_frames"] == 7 and s["ig_skipped"] == 0 and s["ig_videos"] == 3 and "leave-one-video-out" in s["ig_baseline"]
    heads = [l.split(":")[0] for l in text.strip().splitlines()[-15:]]
    assert heads == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "IG", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ",
                     "Avg Video KLdiv", "Avg Video IG", "ig_baseline", "IG frames scored", "frames scored"]
    per = [s["videos"][n]["IG"] for n, _ in vids]
    assert s["video_averaged"]["IG"] == pytest.approx(sum(per) / 3, rel=1e-12)
    assert s["frame_weighted"]["IG"] == pytest.approx((2 * per[0] + 3 * per[1] + 2 * per[2]) / 7, rel=1e-12)
    # another batch size: the same baselines, the same values
    s5 = EV.evaluate(vids, torch.device("cpu"), batch=5, jitter=False, per_frame=True, ig=dict(baseline=None)).summary()
    assert s5["frame_weighted"]["IG"] == s["frame_weighted"]["IG"] and s5["videos"]["vid1"]["per_frame"] == s["videos"]["vid1"]["per_frame"]
    # a single video has no other video: the total, and the output says so
    del SEEN[:]
    one = EV.evaluate(vids[1:2], torch.device("cpu"), batch=8, jitter=False, ig=dict(baseline=None))
    assert np.array_equal(SEEN[0][1], sums[1]) and "single video" in one.summary()["ig_baseline"]
    one.report()
    assert "ig_baseline: a single video" in capsys.readouterr().out


def test_evaluator_unequal_ground_truth_sizes_ask_for_a_baseline_file(monkeypatch):
    import torch
    from vinet_amd import evaluate as EV
    vids = _three_videos()
    k, p, g, f = vids[2][1][1]
    vids[2][1][1] = (k, p[:20], g[:20], f[:20])
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_all)
    with pytest.raises(ValueError, match=r"differ in size.*--baseline"):
        EV.evaluate(vids, torch.device("cpu"), batch=2, jitter=False, ig=dict(baseline=None))
    # with a baseline of that size for every frame there is nothing to sum: the same videos, cut to one size, run
    vids[2] = (vids[2][0], vids[2][1][:1])
    base = np.arange(24 * 40, dtype=np.float32).reshape(24, 40)
    del SEEN[:]
    s = EV.evaluate(vids, torch.device("cpu"), batch=2, jitter=False, ig=dict(baseline=base)).summary()
    assert s["ig_frames"] == 6 and "ig_baseline" not in s and all(np.array_equal(x[1], base) and x[2] == "torch.float32" for x in SEEN)
    with pytest.raises(ValueError, match="cannot be resized"):
        EV.evaluate(vids, torch.device("cpu"), batch=2, jitter=False, ig=dict(baseline=base[:12]))


def test_evaluator_baseline_file_and_flags(tmp_path, monkeypatch):
    from PIL import Image
    from vinet_amd import evaluate as EV
    vids = TS._videos_for_sauc()
    P, G = TH._write_tree(str(tmp_path), vids)
    base = np.random.default_rng(5).integers(0, 256, (24, 40)).astype(np.uint8)
    npy, png = os.path.join(str(tmp_path), "base.npy"), os.path.join(str(tmp_path), "base.png")
    np.save(npy, base.astype(np.float64) / 7)
    Image.fromarray(base).save(png)
    assert np.array_equal(EV.load_baseline(png), base) and EV.load_baseline(npy).dtype == np.float64
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_all)
    out = os.path.join(str(tmp_path), "s.json")
    for path, want, dtype in ((npy, base.astype(np.float64) / 7, "torch.float64"), (png, base.astype(np.float64), "torch.float64")):
        del SEEN[:]
        assert EV.main(["--pred_dir", P, "--gt_dir", G, "--batch", "4", "--jitter", "0", "--ig", "--baseline", path, "--borji", "--borji_splits", "5",
                        "--borji_step", "0.05", "--seed", "9", "--device", "cpu", "--json", out, "--per_frame"]) == 0
        igs, bos = [x for x in SEEN if x[0] == "ig"], [x for x in SEEN if x[0] == "borji"]
        assert len(igs) == 2 and all(np.array_equal(x[1], want) and x[2] == dtype for x in igs)
        assert [x[1:] for x in bos] == [([0, 1, 2], 5, 0.05, 9), ([3, 4], 5, 0.05, 9)]          # running frame numbers
        s = json.load(open(out))
        assert s["ig_frames"] == 4 and s["ig_skipped"] == 0 and s["borji_frames"] == 4 and "ig_baseline" not in s and "sauc_frames" not in s
        assert list(s["frame_weighted"]) == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "AUCB", "IG"]
    with pytest.raises(SystemExit):
        EV.main(["--pred_dir", P, "--gt_dir", G, "--baseline", npy, "--device", "cpu"])


def test_evaluator_counts_nan_frames_per_column(tmp_path, monkeypatch, capsys):
    """tests/test_sauc_host.py's tree (vidA 0002: empty ground truth, skipped for every column; vidB 0001: NaN sAUC only) with
    vidB 0002 cut to ONE fixation: NaN AUC-Borji (AUC_Borji.m:31), every other column fine.  A constant --baseline makes every
    IG NaN."""
    import torch
    from vinet_amd import evaluate as EV
    vids = TS._videos_for_sauc()
    k, p, g, f = vids["vidB"][1]
    one = np.zeros_like(f)
    one.reshape(-1)[np.flatnonzero(f)[0]] = 1
    vids["vidB"][1] = (k, p, g, one)
    P, G = TH._write_tree(str(tmp_path), vids)
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_all)
    collected = EV.collect(P, G)
    kw = dict(batch=2, jitter=False, per_frame=True, seed=4, sauc=dict(n_splits=7, step=0.1, other_map=None), borji=dict(n_splits=7, step=0.1))
    s = EV.evaluate(collected, torch.device("cpu"), ig=dict(baseline=None), **kw).report()
    text = capsys.readouterr().out
    heads = [l.split(":")[0] for l in text.strip().splitlines()[-21:]]
    assert heads == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "sAUC", "AUCB", "IG", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ",
                     "Avg Video KLdiv", "Avg Video sAUC", "Avg Video AUCB", "Avg Video IG", "ig_baseline", "sAUC frames scored",
                     "AUCB frames scored", "IG frames scored", "frames scored"]
    assert "AUCB frames scored: 3, skipped (NaN AUCB only): 1, videos: 2" in text
    assert (s["frames"], s["skipped"]) == (4, 1)
    assert (s["sauc_frames"], s["sauc_skipped"]) == (3, 1) and (s["borji_frames"], s["borji_skipped"], s["borji_videos"]) == (3, 1, 2)
    assert (s["ig_frames"], s["ig_skipped"], s["ig_videos"]) == (4, 0, 2)
    pf = {name: s["videos"][name]["per_frame"] for name in vids}
    assert math.isnan(pf["vidB"]["0002"]["AUCB"]) and not any(math.isnan(pf["vidB"]["0002"][m]) for m in EV.METRICS + ("sAUC", "IG"))
    assert math.isnan(pf["vidB"]["0001"]["sAUC"]) and not math.isnan(pf["vidB"]["0001"]["AUCB"])
    assert s["videos"]["vidB"]["borji_skipped"] == 1 and s["videos"]["vidB"]["borji_frames"] == 1 and s["videos"]["vidB"]["frames"] == 2
    va = (pf["vidA"]["0001"]["AUCB"] + pf["vidA"]["0003"]["AUCB"]) / 2
    vb = pf["vidB"]["0001"]["AUCB"]
    assert s["videos"]["vidA"]["AUCB"] == pytest.approx(va, rel=1e-12) and s["videos"]["vidB"]["AUCB"] == pytest.approx(vb, rel=1e-12)
    assert s["video_averaged"]["AUCB"] == pytest.approx((va + vb) / 2, rel=1e-12)
    assert s["frame_weighted"]["AUCB"] == pytest.approx((2 * va + vb) / 3, rel=1e-12)
    assert 0.0 <= va <= 1.0 and 0.0 <= vb <= 1.0
    # the other columns are what they are without the new flags
    only = EV.evaluate(collected, torch.device("cpu"), batch=2, jitter=False, per_frame=True, seed=4, sauc=kw["sauc"]).summary()
    for m in EV.METRICS + ("sAUC",):
        assert only["frame_weighted"][m] == s["frame_weighted"][m] and only["video_averaged"][m] == s["video_averaged"][m]
    # another batch size: the same frame ids, the same AUCB
    s5 = EV.evaluate(collected, torch.device("cpu"), ig=dict(baseline=None), **dict(kw, batch=5)).summary()
    assert s5["frame_weighted"]["AUCB"] == s["frame_weighted"]["AUCB"] and s5["frame_weighted"]["IG"] == s["frame_weighted"]["IG"]
    # a constant baseline: every scored frame has a NaN IG and stays in the other means
    c = EV.evaluate(collected, torch.device("cpu"), ig=dict(baseline=np.full((24, 40), 3, np.uint8)), **kw).summary()
    assert (c["ig_frames"], c["ig_skipped"], c["ig_videos"]) == (0, 4, 0) and math.isnan(c["frame_weighted"]["IG"]) and math.isnan(c["video_averaged"]["IG"])
    assert c["frames"] == 4 and c["frame_weighted"]["AUCB"] == s["frame_weighted"]["AUCB"] and "IG" not in c["videos"]["vidA"]


def test_default_output_is_unchanged_without_the_new_flags(tmp_path, monkeypatch, capsys):
    import torch
    from vinet_amd import evaluate as EV
    assert EV.METRICS == ("SIM", "CC", "NSS", "AUCJ", "KLdiv")
    P, G = TH._write_tree(str(tmp_path), TH._tiny_videos())
    monkeypatch.setattr(EV, "frame_metrics", TH._model_metrics)          # the five-argument stand-in: no new keyword may reach it
    scores = EV.evaluate(EV.collect(P, G), torch.device("cpu"), batch=2, jitter=False, per_frame=True)
    capsys.readouterr()
    s = scores.report()
    lines = capsys.readouterr().out.splitlines()
    # the report, line for line, as the evaluator has always printed it
    want = ["%s: %s" % (m, s["frame_weighted"][m]) for m in EV.METRICS] + ["Avg Video %s: %s" % (m, s["video_averaged"][m]) for m in EV.METRICS]
    want.append("frames scored: %d, skipped (NaN): %d, videos: %d" % (s["frames"], s["skipped"], s["num_videos"]))
    assert lines == want
    assert list(s) == ["frames", "skipped", "num_videos", "frame_weighted", "video_averaged", "videos"]
    assert list(s["frame_weighted"]) == list(EV.METRICS) and list(s["video_averaged"]) == list(EV.METRICS)
    assert list(s["videos"]["vidB"]) == ["frames", "skipped"] + list(EV.METRICS) + ["per_frame"]
    assert list(s["videos"]["vidB"]["per_frame"]["0001"]) == list(EV.METRICS)
    # Scores(sauc=...) and the sAUC-only report keep their shape: the keys, in their order
    sc = EV.Scores(sauc=True)
    sc.add_video("v", ["1", "2"], {m: [0.5, 0.25] for m in EV.METRICS + ("sAUC",)})
    t = sc.summary()
    assert list(t) == ["frames", "skipped", "num_videos", "frame_weighted", "video_averaged", "videos", "sauc_frames", "sauc_skipped", "sauc_videos"]
    assert list(t["videos"]["v"]) == ["frames", "skipped", "sauc_frames", "sauc_skipped", "sAUC"] + list(EV.METRICS)
    sc.report()
    assert capsys.readouterr().out.splitlines()[-2] == "sAUC frames scored: 2, skipped (NaN sAUC only): 0, videos: 1"
