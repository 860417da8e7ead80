"""The earth mover's distance without a GPU: the numpy model (tests/emd_model.py) against the values of the reference's own
solver (tests/golden/emd_fastemd.npz, written by tests/golden/make_emd_goldens.py), against networkx where it is installed
and against cases worked out by hand; MATLAB's imresize weights against their definition (there is no MATLAB to compare
with); the C ABI's refusals; the evaluator's EMD column with the metric functions replaced by the model.

Bound against the goldens: the integer optimum K is the same number on both sides, what remains are the two fp64 divisions
K / f / cf on values below about 25: a few ulps, 1e-12 absolute."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

from tests import emd_model as EM
from vinet_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12


def goldens():
    z = np.load(os.path.join(HERE, "golden", "emd_fastemd.npz"))
    return [(m, z[m["name"] + "_P"], z[m["name"] + "_Q"]) for m in json.loads(str(z["meta"]))]


def test_golden_file_holds_the_cases_it_should():
    g = goldens()
    assert len(g) >= 16
    assert {(m["R"], m["C"]) for m, _, _ in g} >= {(1, 2), (1, 3), (2, 2), (2, 3), (5, 13), (7, 12), (12, 20)}
    names = " ".join(m["name"] for m, _, _ in g)
    for word in ("dense", "empty30", "empty90", "one_source", "one_sink", "equal", "permutation", "negative", "unequal_sums"):
        assert word in names
    assert sum(1 for m, P, Q in g if (P < 0).any() or (Q < 0).any()) >= 2
    assert any(abs(P.sum() - Q.sum()) > 0.05 for _, P, Q in g)
    assert all(m["cpu_seconds"] >= 0 for m, _, _ in g)


@pytest.mark.parametrize("case", goldens(), ids=lambda c: c[0]["name"])
def test_model_against_the_reference_solver(case):
    m, P, Q = case
    got = EM.emd_hist(P, Q, m["R"], m["C"])
    print(m["name"], "model %.17g reference %s diff %.3g" % (got, m["score"], got - float(m["score"])))
    assert abs(got - float(m["score"])) <= TOL


def test_goldens_swap_roles_both_ways():
    sw = [EM.quantise(P, Q, m["R"], m["C"])[5] for m, P, Q in goldens()]
    assert any(sw) and not all(sw)


def test_model_against_network_simplex():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(5)
    for R, C in ((2, 3), (5, 13), (7, 12)):
        P, Q = rng.random(R * C) * (rng.random(R * C) > 0.3), rng.random(R * C) * (rng.random(R * C) > 0.3)
        P, Q = P / P.sum(), 0.95 * Q / Q.sum()
        ip, iq, iC, f, cf, _, _ = EM.quantise(P, Q, R, C)
        G = nx.DiGraph()
        extra = int(ip.sum() - iq.sum())
        for i in np.nonzero(ip)[0]:
            G.add_node("s%d" % i, demand=-int(ip[i]))
            G.add_edge("s%d" % i, "drop", weight=0)
            for j in np.nonzero(iq)[0]:
                G.add_edge("s%d" % i, "t%d" % j, weight=int(iC[i, j]))
        for j in np.nonzero(iq)[0]:
            G.add_node("t%d" % j, demand=int(iq[j]))
        G.add_node("drop", demand=extra)
        K, _ = nx.network_simplex(G)
        assert K == EM.min_cost(ip, iq, iC)[0]


def test_hand_cases():
    assert EM.emd_hist([1, 0], [0, 1], 1, 2) == 1.0
    assert EM.emd_hist([1, 0, 0], [0, 0, 1], 1, 3) == 2.0
    assert EM.emd_hist([.5, .5, 0], [0, .5, .5], 1, 3) == 1.0
    assert EM.emd_hist([.2, .5, .3, 0, 0, 0], [.2, .5, .3, 0, 0, 0], 2, 3) == 0.0
    # the pre-flow rule on a negative bin: P = [1.5, -0.5], Q = [0, 1]: m = [0, -0.5], p = [1.5, 0], q = [0, 1.5]: 1.5 over distance 1
    assert EM.emd_hist([1.5, -0.5], [0, 1], 1, 2) == pytest.approx(1.5, abs=TOL)
    # the free surplus: P = [1, 0], Q = [0, 0.5] ships half a unit
    assert EM.emd_hist([1, 0], [0, .5], 1, 2) == pytest.approx(0.5, abs=TOL)
    for P, Q, R, C in (([0, 0], [0, 0], 1, 2), ([1, float("nan")], [0, 1], 1, 2), ([1], [1], 1, 1)):
        assert math.isnan(EM.emd_hist(P, Q, R, C))


# ---- imresize -----------------------------------------------------------------------------------------------------------------------
def test_resize_weights_of_the_product_are_the_models():
    from vinet_amd import utils
    for n_in, n_out, s in ((224, 7, 1 / 32), (130, 5, 1 / 32), (112, 7, 7 / 112), (8, 4, 0.5), (5, 5, 1.0), (4, 8, 2.0)):
        assert np.array_equal(utils.matlab_resize_weights(n_in, n_out, s).numpy(), EM.resize_weights(n_in, n_out, s))


def test_resize_weights_properties():
    for n_in, n_out, s in ((224, 7, 1 / 32), (384, 12, 1 / 32), (100, 4, 1 / 32), (130, 5, 1 / 32), (192, 12, 12 / 192), (8, 4, 0.5), (6, 6, 1.0)):
        W = EM.resize_weights(n_in, n_out, s)
        assert W.shape == (n_out, n_in) and np.abs(W.sum(1) - 1).max() <= 1e-15
        assert np.abs(W @ np.full(n_in, 3.25) - 3.25).max() <= 1e-14
        if abs(n_out / s - n_in) < 1e-9:          # the output grid is centred on the input: mirror symmetry
            assert np.abs(W - W[::-1, ::-1]).max() <= 1e-15
    assert np.array_equal(EM.resize_weights(6, 6, 1.0), np.eye(6))
    for (H, W), (R, C) in (((224, 384), (7, 12)), ((360, 640), (12, 20)), ((100, 130), (4, 5))):
        assert (EM.out_size(H, 32), EM.out_size(W, 32)) == (R, C)
    const = EM.resize(np.full((100, 130), 0.7), 4, 5, 1 / 32, 1 / 32)
    assert const.shape == (4, 5) and np.abs(const - 0.7).max() <= 1e-14


def test_resize_row_worked_out_by_hand():
    """n_in = 8, s = 1/2, output x = 2: u = 2 / s + 0.5 (1 - 1 / s) = 3.5, width 8, left = floor(3.5 - 4) = -1, taps -1 .. 8.
    h(t) = cubic(t / 2) / 2 at t = u - index = 4.5, 3.5, 2.5, 1.5, 0.5, -0.5, ..., -4.5, that is cubic at 2.25, 1.75, 1.25, .75, .25:
        cubic(2.25) = 0
        cubic(1.75) = -0.5 * 5.359375 + 2.5 * 3.0625 - 7 + 2 = -0.0234375
        cubic(1.25) = -0.5 * 1.953125 + 2.5 * 1.5625 - 5 + 2 = -0.0703125
        cubic(0.75) = 1.5 * 0.421875 - 2.5 * 0.5625 + 1      =  0.2265625
        cubic(0.25) = 1.5 * 0.015625 - 2.5 * 0.0625 + 1      =  0.8671875
    The halves of these sum to 1 over the ten taps already.  Tap -1 and tap 0 are clamped onto pixel 1: it gets
    (0 - 0.0234375 - 0.0703125) / 2 = -0.046875 (tap 1 is pixel 1 itself); pixel 8 is tap 8 alone (weight 0)... in full:"""
    want = [(-0.0234375 - 0.0703125) / 2, 0.2265625 / 2, 0.8671875 / 2, 0.8671875 / 2, 0.2265625 / 2, -0.0703125 / 2, -0.0234375 / 2, 0.0]
    assert np.allclose(EM.resize_weights(8, 4, 0.5)[1], want, rtol=0, atol=1e-16)


# ---- the cases of the device test qualify ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EM.E2E))
def test_end_to_end_cases_qualify_for_an_exact_cost(name):
    """tests/test_gpu_emd.py asserts the integer optimum exactly where no p * f lies within MARGIN of a rounding boundary: every
    listed case must, so that none is skipped in silence"""
    pred, gt, ds, res = EM.e2e_case(name)
    Hg, Wg = EM.E2E[name][:2]
    for score, K, margin, P, Q in res:
        print(name, "score %.6f K %d margin %.3g" % (score, K, margin))
        assert margin > EM.MARGIN and K > 0 and math.isfinite(score)
        assert P.size == EM.out_size(Hg, ds) * EM.out_size(Wg, ds) and abs(P.sum() - 1) < 1e-12 and abs(Q.sum() - 1) < 1e-12


# ---- the library and the Python surface ---------------------------------------------------------------------------------------------
def test_library_refuses_before_any_launch():
    lib = L.load()
    assert lib.vinet_emd_workspace(4, 12, 20) > 0 and lib.vinet_emd_workspace(4, 16, 32) > 0
    for B, R, C in ((0, 2, 3), (1, 0, 3), (1, 2, 0), (1, 16, 33), (1, 1, 513)):
        assert lib.vinet_emd_workspace(B, R, C) == 0
    p = 4096
    ok = dict(s=p, s64=0, Hs=64, Ws=96, gt=p, g64=0, Hg=64, Wg=96, B=1, ds=32, R=2, C=3, ws=p, wsb=1 << 20)

    def emd(**kw):
        a = dict(ok, **kw)
        return lib.vinet_emd(a["s"], a["s64"], a["Hs"], a["Ws"], a["gt"], a["g64"], a["Hg"], a["Wg"], a["B"], a["ds"], a["R"], a["C"], p, p, p, p,
                             a["ws"], a["wsb"], p, None, None, None, None)

    for bad, word in ((dict(ds=0), b"downsize"), (dict(ds=-3), b"downsize"), (dict(Hg=1024, Wg=1024, R=32, C=32), b"bins"),
                      (dict(R=0), b"at least one bin"), (dict(R=3), b"bins"), (dict(B=0), b"positive"), (dict(s=None), b"null"),
                      (dict(ws=None), b"workspace"), (dict(wsb=8), b"workspace")):
        assert emd(**bad) < 0, bad
        assert word in lib.vinet_last_error() and b"emd" in lib.vinet_last_error(), (bad, lib.vinet_last_error())
    for bad, word in ((dict(R=23, C=23), b"bins"), (dict(R=0, C=4), b"at least one bin"), (dict(P=None), b"null"), (dict(wsb=8), b"workspace")):
        a = dict(dict(P=p, R=2, C=3, wsb=1 << 20), **bad)
        assert lib.vinet_emd_hist(a["P"], p, 1, a["R"], a["C"], p, a["wsb"], p, None, None, None) < 0, bad
        assert word in lib.vinet_last_error() and b"emd_hist" in lib.vinet_last_error(), (bad, lib.vinet_last_error())


def test_python_surface_has_no_cpu_fallback():
    import torch
    from vinet_amd import loss, ops  # noqa: F401
    assert not L.is_test_double()
    s, g = torch.rand(2, 64, 96), torch.rand(2, 64, 96)
    for fn in (lambda: loss.emd_batch(s, g), lambda: loss.emd(s[0], g[0]), lambda: loss.emd_hist_batch(torch.rand(2, 6), torch.rand(2, 6), 2, 3),
               lambda: torch.ops.vinet.emd(s, g, 32)):
        with pytest.raises(Exception):
            fn()
    with pytest.raises(NotImplementedError):
        loss.emd(s[0], g[0], toPlot=True)


# ---- the evaluator, metric functions replaced by numpy ---------------------------------------------------------------------------------
def _model_metrics_emd(pred_u8, gt_u8, fix_u8, blur=False, noise=None, emd=None):
    import torch
    from tests import test_metrics_host as TH
    out = TH._model_metrics(pred_u8, gt_u8, fix_u8, blur=blur, noise=noise)
    if emd is not None:
        out["EMD"] = torch.tensor([EM.emd(p.astype(np.float32), g.astype(np.float32), emd["downsize"]) for p, g in zip(pred_u8.numpy(), gt_u8.numpy())],
                                  dtype=torch.float64)
    return out


def _videos():
    from vinet_amd import synth
    vids = []
    for vi, cnt in enumerate((2, 3)):
        gt = (synth.saliency_maps("emd_gt%d" % vi, cnt, 24, 40, vi, noise=0.0) * 255).astype(np.uint8)
        pred = synth.saliency_maps("emd_pred%d" % vi, cnt, 24, 40, vi + 5, levels=256).astype(np.uint8)
        fix = synth.fixation_maps(synth.fixations("emd_fix%d" % vi, gt, 12, vi), 24, 40, dtype=np.uint8)
        vids.append(("vid%d" % vi, [("%04d" % (i + 1), pred[i], gt[i], fix[i]) for i in range(cnt)]))
    return vids


def test_evaluator_emd_column_and_its_nan_accounting(monkeypatch, capsys):
    import torch
    from tests import test_metrics_host as TH
    from vinet_amd import evaluate as EV
    assert EV.EXTRA[-1] == ("emd", "EMD")
    vids = _videos()
    monkeypatch.setattr(EV, "frame_metrics", _model_metrics_emd)
    s = EV.evaluate(vids, torch.device("cpu"), batch=2, jitter=False, per_frame=True, emd=dict(downsize=8)).report()
    text = capsys.readouterr().out
    assert s["emd_frames"] == s["frames"] == 5 and s["emd_skipped"] == 0 and s["emd_videos"] == 2
    for name, frames in vids:
        for k, p, g, f in frames:
            assert s["videos"][name]["per_frame"][k]["EMD"] == EM.emd(p.astype(np.float32), g.astype(np.float32), 8)
    per = [s["videos"][n]["EMD"] for n, _ in vids]
    assert s["video_averaged"]["EMD"] == pytest.approx(sum(per) / 2, rel=1e-12)
    assert s["frame_weighted"]["EMD"] == pytest.approx((2 * per[0] + 3 * per[1]) / 5, rel=1e-12)
    assert "EMD frames scored: 5, skipped (NaN EMD only): 0, videos: 2" in text
    # a NaN EMD leaves the frame in the other means
    sc = EV.Scores(emd=True)
    sc.add_video("v", ["a", "b"], {"SIM": [.5, .5], "CC": [.5, .5], "NSS": [1, 1], "AUCJ": [.7, .7], "KLdiv": [1, 1], "EMD": [float("nan"), 2.0]})
    assert sc.summary()["frames"] == 2 and sc.summary()["emd_frames"] == 1 and sc.summary()["emd_skipped"] == 1 and sc.summary()["frame_weighted"]["EMD"] == 2.0
    # without the flag: the five-argument stand-in (no new keyword may reach it) and the keys of before
    monkeypatch.setattr(EV, "frame_metrics", TH._model_metrics)
    s0 = EV.evaluate(vids, torch.device("cpu"), batch=2, jitter=False).summary()
    assert sorted(s0) == ["frame_weighted", "frames", "num_videos", "skipped", "video_averaged", "videos"]
    assert sorted(s0["frame_weighted"]) == sorted(EV.METRICS) and sorted(s0["videos"]["vid0"]) == sorted(EV.METRICS + ("frames", "skipped"))
    assert "--emd" in EV.__doc__ and "--emd_downsize" in EV.__doc__
