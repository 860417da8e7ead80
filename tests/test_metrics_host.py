"""AUC-Judd and the evaluator without a GPU: the numpy rank model (tests/auc_model.py) against the reference's recorded
results (tests/golden/auc_judd.npz, written by tests/golden/make_metric_goldens.py from the unmodified reference), the C ABI's
argument checks, and the evaluator's pairing / averaging / NaN skipping with the metric functions replaced by the model."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import auc_model as M
from tests import metric_cases as MC
from vinet_amd import _lib as L

CASES = MC.load()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_rank_model_reproduces_the_reference(case):
    """scores to the last bit, `above` exactly, NaN where the reference returns NaN"""
    for b in range(case.B):
        score, n, above = M.auc_judd_rank(case.s[b], case.fix[b], noise=None if case.noise is None else case.noise[b])
        assert n == case.nfix[b]
        if math.isnan(case.score[b]):
            assert math.isnan(score)
            continue
        assert np.array_equal(above, case.above[b])
        assert score == case.score[b], (score, case.score[b])


def test_fixture_covers_what_it_claims():
    by = {c.name: c for c in CASES}
    assert by["large"].nfix.max() > MC.LDS_CAP and by["large"].nfix[0] == 20000        # workspace path
    assert math.isnan(by["nan"].score[0]) and math.isnan(by["nan"].score[1]) and not math.isnan(by["nan"].score[2])
    assert by["fix64"].fix.dtype == np.float64 and by["jit30"].noise is not None
    q = by["quant400"]
    assert (np.diff(q.above[0]) == 0).sum() > 100                                      # heavy ties: runs of equal counts
    assert by["ends"].nfix[0] == 1
    s = by["ends"].s
    assert int(s[1].argmax()) in by["ends"].idx[1] and int(s[2].argmin()) in by["ends"].idx[2]
    assert os.path.getsize(MC.FIXTURE) < 300 * 1024


@pytest.mark.parametrize("case", [c for c in CASES if c.name != "nan"], ids=lambda c: c.name)
def test_mit_variant_is_the_matlab_formula(case):
    """fp_offset = 1 against AUC_Judd.m:68-75 transcribed (the MATLAB file cannot be run here: the variant is pinned to its formula
    only), on the fixture's counts; and it differs from the Python port's result"""
    for b in range(case.B):
        npix = case.H * case.W
        assert M.score_from_above(case.above[b], npix, 1) == M.score_matlab(case.above[b], npix)
        assert M.score_from_above(case.above[b], npix, 1) != case.score[b]
        assert abs(M.score_from_above(case.above[b], npix, 1) - case.score[b]) < 1e-3


def test_library_exports_and_rejects_bad_arguments_without_a_gpu():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "vinet_auc_judd") and hasattr(raw, "vinet_auc_judd_workspace")
    need = lib.vinet_auc_judd_workspace(2, 1000)
    assert need >= 2 * (1024 * 8 + 1001 * 4)
    assert lib.vinet_auc_judd_workspace(0, 1000) == 0
    p = 4096          # never dereferenced: every call below is rejected before a launch
    ok = dict(s=p, s64=0, fix=p, f64=0, B=2, n=1000, off=0, ws=p, wsb=need, score=p, nfix=p, above=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.vinet_auc_judd(a["s"], a["s64"], a["fix"], a["f64"], a["B"], a["n"], a["off"], a["ws"], a["wsb"], a["score"], a["nfix"],
                                  a["above"], a["stream"])

    for bad, word in ((dict(score=None), b"score"), (dict(n=0), b"positive"), (dict(n=-5), b"positive"), (dict(B=0), b"positive"),
                      (dict(wsb=need - 1), b"workspace"), (dict(ws=None), b"workspace"), (dict(off=2), b"fp_offset"), (dict(s=None), b"null")):
        assert call(**bad) < 0, bad
        assert word in lib.vinet_last_error(), (bad, lib.vinet_last_error())


def test_python_surface_has_no_cpu_fallback():
    import torch
    from vinet_amd import loss
    assert not L.is_test_double()
    s, f = torch.rand(1, 8, 8), (torch.rand(1, 8, 8) > 0.8).float()
    with pytest.raises(Exception):
        loss.auc_judd_batch(s, f)
    with pytest.raises(Exception):
        loss.auc_judd(s, f, jitter=False)
    with pytest.raises(NotImplementedError):
        loss.auc_judd(s, f, toPlot=True)
    with pytest.raises(NotImplementedError):
        loss.auc_judd(s, f, normalize=True)
    with pytest.raises(AssertionError, match="resize the saliency map"):
        loss.auc_judd_batch(torch.rand(1, 4, 8), f)
    assert not hasattr(loss, "auc_shuff")


def test_companion_tensor_on_another_device_is_refused_before_the_library(monkeypatch):
    """Maps on the meta device, one companion tensor on the CPU: every metric raises a ValueError that names itself and the argument,
    and none of them reaches the library on the way (a host pointer handed to a kernel is a device fault, not a Python error)."""
    import torch
    from vinet_amd import loss

    def reached():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "get", reached)
    meta = torch.device("meta")
    s, cpu = torch.empty(2, 8, 8, device=meta), torch.ones(2, 8, 8)
    hist, hist_cpu = torch.empty(2, 6, device=meta), torch.ones(2, 6)
    with pytest.raises(AssertionError, match="the library was reached"):          # (with everything in one place the call goes on)
        loss.auc_judd_batch(s, s)
    for metric, arg, call in (
            ("auc_judd", "fix_maps", lambda: loss.auc_judd_batch(s, cpu)),
            ("auc_judd", "noise", lambda: loss.auc_judd_batch(s, s, noise=cpu.double())),
            ("auc_shuffled", "fix_maps", lambda: loss.auc_shuffled_batch(s, cpu, s[0])),
            ("auc_shuffled", "other_map", lambda: loss.auc_shuffled_batch(s, s, cpu[0])),
            ("auc_borji", "fix_maps", lambda: loss.auc_borji_batch(s, cpu)),
            ("info_gain", "fix_maps", lambda: loss.info_gain_batch(s, cpu)),
            ("info_gain", "baseline", lambda: loss.info_gain_batch(s, s, cpu[0])),
            ("emd", "gt_maps", lambda: loss.emd_batch(s, cpu)),
            ("emd_hist", "Q", lambda: loss.emd_hist_batch(hist, hist_cpu, 2, 3)),
            ("nss", "gt", lambda: loss.nss(s, cpu)),
            ("per_sample", "gt", lambda: loss.per_sample("cc", s, cpu)),
            ("kldiv", "gt", lambda: loss.kldiv(s, cpu))):
        with pytest.raises(ValueError, match=r"^%s: %s on cpu, the maps on meta$" % (metric, arg)):
            call()


# ---- the evaluator on a tiny tree, metric functions replaced by numpy ------------------------------------------------------------
def _model_metrics(pred_u8, gt_u8, fix_u8, blur=False, noise=None):
    """numpy stand-in for evaluate.frame_metrics on equal-size maps: SIM / CC / NSS / KLdiv by their definitions (loss.py), AUC-J by
    the rank model.  An all-zero ground truth gives NaN SIM / CC, no fixation gives NaN NSS, as in the reference."""
    import torch
    out = {m: [] for m in ("SIM", "CC", "NSS", "AUCJ", "KLdiv")}
    with np.errstate(all="ignore"):
        for p, g, f in zip(pred_u8.numpy().astype(np.float64), gt_u8.numpy().astype(np.float64), fix_u8.numpy().astype(np.float64)):
            pn, gn = (p - p.min()) / (p.max() - p.min()), (g - g.min()) / (g.max() - g.min())
            out["SIM"].append(np.minimum(pn / pn.sum(), gn / gn.sum()).sum())
            out["CC"].append(np.corrcoef(p.ravel(), g.ravel())[0, 1])
            out["NSS"].append((((p - p.mean()) / (p.std(ddof=1) + 2.2204e-16)) * f).sum() / f.sum())
            out["AUCJ"].append(M.auc_judd_rank(p.astype(np.float32), f)[0])
            pp, gg = p / p.sum(), g / g.sum()
            out["KLdiv"].append((gg * np.log(2.2204e-16 + gg / (pp + 2.2204e-16))).sum())
    return {k: torch.tensor(v, dtype=torch.float64) for k, v in out.items()}


def _write_tree(root, videos):
    """videos: {name: [(key, pred, gt, fix)]} -> P / G trees in the DHF1K layout (fixations as .png, one video as .npy)"""
    from PIL import Image
    P, G = os.path.join(root, "pred"), os.path.join(root, "gt")
    for vi, (name, frames) in enumerate(videos.items()):
        for d in (os.path.join(P, name), os.path.join(G, name, "maps"), os.path.join(G, name, "fixation")):
            os.makedirs(d)
        for key, pred, gt, fix in frames:
            Image.fromarray(pred).save(os.path.join(P, name, "%s.png" % key))
            Image.fromarray(gt).save(os.path.join(G, name, "maps", "eyeMap_%s.png" % key))
            if vi == 0:
                Image.fromarray(fix * 255).save(os.path.join(G, name, "fixation", "%s.png" % key))
            else:
                np.save(os.path.join(G, name, "fixation", "fixMap_%s.npy" % key), fix)
    return P, G


def _tiny_videos():
    from vinet_amd import synth
    vids = {}
    for vi, (name, cnt) in enumerate((("vidA", 3), ("vidB", 2))):
        gt = (synth.saliency_maps("ev_gt%d" % vi, cnt, 24, 40, vi, noise=0.0) * 255).astype(np.uint8)
        pred = synth.saliency_maps("ev_pred%d" % vi, cnt, 24, 40, vi, levels=256).astype(np.uint8)
        fix = synth.fixation_maps(synth.fixations("ev_fix%d" % vi, gt, 12, vi), 24, 40, dtype=np.uint8)
        vids[name] = [("%04d" % (i + 1), pred[i], gt[i], fix[i]) for i in range(cnt)]
    vids["vidA"][1] = (vids["vidA"][1][0], vids["vidA"][1][1], np.zeros((24, 40), np.uint8), vids["vidA"][1][3])     # empty ground truth: NaN SIM / CC
    return vids


def test_evaluator_pairs_averages_and_skips_nan_frames(tmp_path, monkeypatch, capsys):
    import torch
    from vinet_amd import evaluate as EV
    vids = _tiny_videos()
    P, G = _write_tree(str(tmp_path), vids)
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics)
    collected = EV.collect(P, G)
    assert [v for v, _ in collected] == ["vidA", "vidB"]
    assert [k for k, *_ in collected[0][1]] == ["0001", "0002", "0003"]
    assert collected[1][1][0][3].endswith("fixMap_0001.npy") and collected[0][1][0][2].endswith("eyeMap_0001.png")
    scores = EV.evaluate(collected, torch.device("cpu"), batch=2, jitter=False, per_frame=True)
    s = scores.report()
    text = capsys.readouterr().out
    tail = [l.split(":")[0] for l in text.strip().splitlines()[-11:-1]]
    assert tail == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ", "Avg Video KLdiv"]
    assert "No saliency" in text and "1 vidA 0002" in text
    assert s["frames"] == 4 and s["skipped"] == 1 and s["num_videos"] == 2
    # expected values: the model per frame, from the arrays, skipping the frame with the empty ground truth
    per = {}
    for name, frames in vids.items():
        for key, p, g, f in frames:
            r = _model_metrics(torch.from_numpy(p[None]), torch.from_numpy(g[None]), torch.from_numpy(f[None]))
            per[(name, key)] = {m: float(v[0]) for m, v in r.items()}
    kept = {k: v for k, v in per.items() if k != ("vidA", "0002")}
    assert math.isnan(per[("vidA", "0002")]["CC"])
    for m in EV.METRICS:
        assert s["frame_weighted"][m] == pytest.approx(sum(v[m] for v in kept.values()) / 4, rel=1e-12)
        va = (per[("vidA", "0001")][m] + per[("vidA", "0003")][m]) / 2
        vb = (per[("vidB", "0001")][m] + per[("vidB", "0002")][m]) / 2
        assert s["videos"]["vidA"][m] == pytest.approx(va, rel=1e-12) and s["videos"]["vidA"]["skipped"] == 1
        assert s["video_averaged"][m] == pytest.approx((va + vb) / 2, rel=1e-12)
        assert s["videos"]["vidB"]["per_frame"]["0002"][m] == pytest.approx(per[("vidB", "0002")][m], rel=1e-12)


def test_evaluator_names_the_file_without_a_partner(tmp_path):
    from vinet_amd import evaluate as EV
    P, G = _write_tree(str(tmp_path), _tiny_videos())
    os.remove(os.path.join(G, "vidA", "maps", "eyeMap_0003.png"))
    with pytest.raises(FileNotFoundError, match=r"ground-truth map for .*vidA.0003\.png"):
        EV.collect(P, G)
    os.remove(os.path.join(P, "vidA", "0003.png"))
    with pytest.raises(FileNotFoundError, match=r"no predicted map for fixation map .*0003\.png"):
        EV.collect(P, G)
