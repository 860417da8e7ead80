"""The earth mover's distance on the device (vinet_amd/csrc/emd.hip: emd_prepare_kernel, emd_hist_kernel, emd_solve_kernel)
against the values of the reference's own solver (tests/golden/emd_fastemd.npz) and the numpy model (tests/emd_model.py).

Bounds.  The integer optimum K is an exactly defined number: `cost` is compared with `==`.  The score is K / f / cf, two fp64
divisions on values below about 25 on both sides: 1e-12 absolute against the golden's %.17g.  End to end, a bin of a resized
map is an fp64 sum of at most 130 x 130 products of weights below 1 and map values below 6, divided by a sum of order 1: the two
sides differ by the order of their additions only, a few 1e-14 relative; 1e-12 absolute on bins that are at most 1.  K is
exact there as long as no p * f lies within 1e-6 of a rounding boundary (1e-12 of histogram error times f = 1e6), which
tests/test_emd_host.py asserts for every case listed in emd_model.E2E: none is skipped.

Shapes: the goldens' grids (1x2 ... 12x20; 5x13 = 65 bins is one over a wave), 64x96 / 100x130 (ragged last bin) / 224x384 with
a 112x192 prediction / 360x640 once each, an 8x8 grid of ties."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import emd_model as EM
from tests.test_emd_host import goldens

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODEL_K = {}


def _dev():
    return torch.device("cuda:0")


def _hist(P, Q, R, C, dtype=np.float64):
    from vinet_amd import loss
    P, Q = np.atleast_2d(np.asarray(P, dtype=dtype)), np.atleast_2d(np.asarray(Q, dtype=dtype))
    score, cost, status = loss.emd_hist_batch(torch.from_numpy(P).to(_dev()), torch.from_numpy(Q).to(_dev()), R, C, return_cost=True,
                                              return_status=True)
    assert score.dtype == torch.float64 and score.device.type == "cuda" and tuple(score.shape) == (P.shape[0],)
    assert cost.dtype == torch.int64 and status.dtype == torch.int32
    return score.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy()


def _model_k(m, P, Q):
    if m["name"] not in _MODEL_K:
        _MODEL_K[m["name"]] = EM.emd_hist(P, Q, m["R"], m["C"], return_all=True)[1]
    return _MODEL_K[m["name"]]


@pytest.mark.parametrize("grid", sorted({(m["R"], m["C"]) for m, _, _ in goldens()}), ids=lambda g: "%dx%d" % g)
def test_every_golden_of_a_grid_in_one_batch(grid):
    cases = [c for c in goldens() if (c[0]["R"], c[0]["C"]) == grid]
    score, cost, status = _hist([P for _, P, _ in cases], [Q for _, _, Q in cases], *grid)
    for (m, P, Q), s, k, st in zip(cases, score, cost, status):
        want_k = _model_k(m, P, Q)
        print("%s device %.17g reference %s diff %.3g K %d model %d status %d" % (m["name"], s, m["score"], s - float(m["score"]), k, want_k, st))
        assert st == 0 and k == want_k
        assert abs(s - float(m["score"])) <= TOL


def test_hand_cases_fp32_and_fp64():
    for dtype in (np.float32, np.float64):
        assert _hist([1, 0], [0, 1], 1, 2, dtype)[0][0] == 1.0
        assert _hist([1, 0, 0], [0, 0, 1], 1, 3, dtype)[0][0] == 2.0
        assert _hist([.5, .5, 0], [0, .5, .5], 1, 3, dtype)[0][0] == 1.0
        s, k, st = _hist([.25, .5, .25, 0, 0, 0], [.25, .5, .25, 0, 0, 0], 2, 3, dtype)
        assert s[0] == 0.0 and k[0] == 0 and st[0] == 0
        assert abs(_hist([1.5, -0.5], [0, 1], 1, 2, dtype)[0][0] - 1.5) <= TOL          # a negative bin becomes demand on the other side
        assert abs(_hist([1, 0], [0, .5], 1, 2, dtype)[0][0] - 0.5) <= TOL              # the surplus is dropped free


def test_degenerate_grids():
    """8x8, two point masses on a diagonal: every monotone staircase is a shortest path, the integers make the value unique;
    and all mass in one bin on either side, in different bins: S = T = 1"""
    P, Q = np.zeros((3, 64)), np.zeros((3, 64))
    P[0, [0, 9]] = 0.5; Q[0, [54, 63]] = 0.5          # (0,0) (1,1) -> (6,6) (7,7)
    P[1, 3] = 1.0; Q[1, 60] = 1.0                     # (0,3) -> (7,4)
    P[2, :] = 1 / 64; Q[2, 27] = 1.0                  # uniform -> one bin
    score, cost, status = _hist(P, Q, 8, 8)
    for b in range(3):
        want, K, _ = EM.emd_hist(P[b], Q[b], 8, 8, return_all=True)
        print("[%d] device %.17g model %.17g K %d / %d" % (b, score[b], want, cost[b], K))
        assert status[b] == 0 and cost[b] == K and abs(score[b] - want) <= TOL
    assert abs(score[0] - 6 * math.sqrt(2)) <= 1e-5 and abs(score[1] - math.sqrt(50)) <= 1e-5          # (the 1e-6 grid of distances)


def test_nan_rules_leave_the_neighbours_alone():
    rng = np.random.default_rng(3)
    P, Q = rng.random((5, 6)), rng.random((5, 6))
    P /= P.sum(1, keepdims=True); Q /= Q.sum(1, keepdims=True)
    P[1] = 0; Q[1] = 0
    P[3, 2] = np.nan
    score, cost, status = _hist(P, Q, 2, 3)
    assert math.isnan(score[1]) and math.isnan(score[3]) and (status == 0).all()
    for b in (0, 2, 4):
        alone = _hist(P[b], Q[b], 2, 3)
        assert score[b] == alone[0][0] and cost[b] == alone[1][0] and abs(score[b] - EM.emd_hist(P[b], Q[b], 2, 3)) <= TOL
    s, k, st = _hist(np.ones((2, 1)), np.ones((2, 1)), 1, 1)
    assert np.isnan(s).all() and (st == 0).all()


def test_a_map_scores_the_same_bits_alone_and_inside_a_batch():
    cases = [c for c in goldens() if (c[0]["R"], c[0]["C"]) == (7, 12)]
    assert len(cases) >= 5
    P, Q = np.stack([c[1] for c in cases[:5]]), np.stack([c[2] for c in cases[:5]])
    batch = _hist(P, Q, 7, 12)
    alone = _hist(P[3], Q[3], 7, 12)
    assert batch[0][3] == alone[0][0] and batch[1][3] == alone[1][0] and batch[2][3] == alone[2][0] == 0


@pytest.mark.parametrize("name", sorted(EM.E2E))
def test_end_to_end_against_the_model(name):
    from vinet_amd import loss
    pred, gt, ds, res = EM.e2e_case(name)
    score, cost, status, hist = loss.emd_batch(torch.from_numpy(pred).to(_dev()), torch.from_numpy(gt).to(_dev()), downsize=ds, return_cost=True,
                                               return_status=True, return_hist=True)
    assert score.dtype == torch.float64 and tuple(score.shape) == (pred.shape[0],)
    score, cost, status, hist = (x.cpu().numpy() for x in (score, cost, status, hist))
    for b, (want, K, margin, P, Q) in enumerate(res):
        dp, dq = np.abs(hist[b, 0] - P).max(), np.abs(hist[b, 1] - Q).max()
        print("%s[%d] device %.17g model %.17g K %d / %d margin %.3g hist diff %.3g %.3g" % (name, b, score[b], want, cost[b], K, margin, dp, dq))
        assert status[b] == 0
        assert dp <= TOL and dq <= TOL
        assert margin > EM.MARGIN          # (tests/test_emd_host.py keeps it so)
        assert cost[b] == K
        assert abs(score[b] - want) <= TOL


def test_a_map_against_itself_is_exactly_zero_and_the_python_surface():
    from vinet_amd import loss, ops  # noqa: F401
    pred, gt, ds, _ = EM.e2e_case("4x5_ragged")
    g = torch.from_numpy(EM.e2e_case("2x3")[1][0]).to(_dev())          # 64 x 96: both resizes use the scale 1 / 32, P == Q bit for bit
    assert loss.emd(g, g) == 0.0 and loss.emd(g.double(), g) == 0.0
    p = torch.from_numpy(pred).to(_dev())
    one = loss.emd(p[1], torch.from_numpy(gt[1]).to(_dev()))
    both = loss.emd_batch(p, torch.from_numpy(gt).to(_dev()))
    assert isinstance(one, float) and one == float(both[1]) and one == float(torch.ops.vinet.emd(p, torch.from_numpy(gt).to(_dev()), 32)[1])
    with pytest.raises(NotImplementedError):
        loss.emd(g, g, toPlot=True)
    with pytest.raises(RuntimeError, match="downsize"):
        loss.emd_batch(p, p, downsize=0)
    with pytest.raises(RuntimeError, match="bins"):
        loss.emd_batch(p, p, downsize=4)          # 25 x 33 bins
    z = torch.zeros_like(p)
    assert torch.isnan(loss.emd_batch(z, p)).all() and torch.isnan(loss.emd_batch(p, z)).all()


def test_evaluator_emd_column():
    """`evaluate --synthetic 4 --emd --json` in a fresh process: the column is there and finite, every scored frame has one;
    without the flag the keys are the ones of before"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        outs = []
        for flags in (["--emd"], []):
            path = os.path.join(tmp, "out%d.json" % len(outs))
            r = subprocess.run([sys.executable, "-m", "vinet_amd.evaluate", "--synthetic", "4", "--jitter", "0", "--json", path] + flags, cwd=ROOT,
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            outs.append((json.load(open(path)), r.stdout))
    (s, text), (s0, text0) = outs
    assert math.isfinite(s["frame_weighted"]["EMD"]) and math.isfinite(s["video_averaged"]["EMD"]) and s["frame_weighted"]["EMD"] > 0
    assert s["emd_frames"] == s["frames"] == 4 and s["emd_skipped"] == 0 and s["emd_videos"] == 2
    assert "EMD:" in text and "Avg Video EMD:" in text
    assert sorted(s0) == ["frame_weighted", "frames", "num_videos", "skipped", "video_averaged", "videos"] and "EMD" not in text0
    assert sorted(s0["frame_weighted"]) == sorted(["SIM", "CC", "NSS", "AUCJ", "KLdiv"])
    for m in s0["frame_weighted"]:
        assert s0["frame_weighted"][m] == s["frame_weighted"][m]
