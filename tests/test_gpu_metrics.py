"""AUC-Judd on the device (vinet_amd/csrc/metrics.hip) and the evaluator, against the reference's recorded results
(tests/golden/auc_judd.npz: written from the unmodified reference by tests/golden/make_metric_goldens.py).

Bounds.  `nfix` and `above` are integers: exact.  `score`: tp and fp are quotients of exact integers, every term of the
trapezoid sum is rounded identically on both sides, the only freedom is the order of an fp64 sum of N + 1 <= 2.1e4 terms in
[0, 1]: error < (N + 1) * 2^-53 < 3e-12 in the worst case, far less for the tree sums both sides use -> 1e-12 absolute
for every case, the large-N one included."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import auc_model as M
from tests import metric_cases as MC
from vinet_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL = 1e-12
CASES = MC.load()
BY = {c.name: c for c in CASES}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _inputs(case):
    s = torch.from_numpy(case.s).to(_dev())
    if case.noise is not None:
        s = s.double() + torch.from_numpy(case.noise).to(_dev())
    return s.contiguous(), torch.from_numpy(case.fix).to(_dev())


def _raw(s, fix, fp_offset=0, want_above=True):
    """vinet_auc_judd itself: -> (score [B] f64, nfix [B], above [B,n] or None) as numpy"""
    lib = L.load()
    B, n = s.shape[0], s.shape[1] * s.shape[2]
    ws = torch.empty(int(lib.vinet_auc_judd_workspace(B, n)), dtype=torch.uint8, device=s.device)
    score = torch.full((B,), -7.0, dtype=torch.float64, device=s.device)
    nfix = torch.full((B,), -7, dtype=torch.int32, device=s.device)
    above = torch.full((B, n), -7, dtype=torch.int32, device=s.device) if want_above else None
    rc = lib.vinet_auc_judd(s.data_ptr(), int(s.dtype == torch.float64), fix.data_ptr(), int(fix.dtype == torch.float64), B, n, fp_offset,
                            ws.data_ptr(), ws.numel(), score.data_ptr(), nfix.data_ptr(), above.data_ptr() if want_above else None,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    return score.cpu().numpy(), nfix.cpu().numpy(), (above.cpu().numpy() if want_above else None)


def _check(case, score, nfix, above, expect=None):
    expect = case.score if expect is None else expect
    assert np.array_equal(nfix, case.nfix)
    for b in range(case.B):
        print("%s[%d]: N %d device %.17g reference %.17g diff %.3g" % (case.name, b, nfix[b], score[b], expect[b], score[b] - expect[b]))
        if math.isnan(expect[b]):
            assert math.isnan(score[b])
            continue
        if above is not None:
            assert np.array_equal(above[b, :nfix[b]], case.above[b])
            assert (above[b, nfix[b]:] == -7).all()                      # nothing written past the N counts
        assert abs(score[b] - expect[b]) <= TOL


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_entry_point_reproduces_the_reference(case):
    s, fix = _inputs(case)
    _check(case, *_raw(s, fix))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_python_surface_and_mit_variant(case):
    from vinet_amd import loss
    dev = _dev()
    s32, fix = torch.from_numpy(case.s).to(dev), torch.from_numpy(case.fix).to(dev)
    noise = None if case.noise is None else torch.from_numpy(case.noise).to(dev)
    got = loss.auc_judd_batch(s32, fix, noise=noise)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (case.B,)
    _check(case, got.cpu().numpy(), case.nfix, None)
    sc, nf, ab = loss.auc_judd_batch(s32, fix, noise=noise, return_counts=True)
    assert np.array_equal(nf.cpu().numpy(), case.nfix)
    mit = loss.auc_judd_batch(s32, fix, noise=noise, mit=True).cpu().numpy()
    want = np.array([M.auc_judd_rank(case.s[b], case.fix[b], 1, None if case.noise is None else case.noise[b])[0] for b in range(case.B)])
    _check(case, mit, case.nfix, None, expect=want)
    # the drop-in: item 0 of a 3-D input, a 2-D input; jitter off (recorded noise has no way in: cases with noise are skipped here)
    if case.noise is None:
        for args in ((s32, fix), (s32[0], fix[0])):
            v = loss.auc_judd(*args, jitter=False)
            assert isinstance(v, float)
            assert (math.isnan(v) and math.isnan(case.score[0])) or abs(v - case.score[0]) <= TOL


def test_drop_in_messages_and_errors(capsys):
    from vinet_amd import loss
    case = BY["nan"]
    s, fix = torch.from_numpy(case.s).to(_dev()), torch.from_numpy(case.fix).to(_dev())
    assert math.isnan(loss.auc_judd(s[0], fix[0], jitter=False))
    assert capsys.readouterr().out.strip() == "Error: no fixationMap"
    assert math.isnan(loss.auc_judd(s[1], fix[1], jitter=False))
    assert capsys.readouterr().out.strip() == "NaN saliencyMap"
    with pytest.raises(NotImplementedError):
        loss.auc_judd(s, fix, toPlot=True)
    with pytest.raises(NotImplementedError):
        loss.auc_judd(s, fix, normalize=True)
    with pytest.raises(AssertionError, match="resize the saliency map to the fixation map first"):
        loss.auc_judd(s[:, :20], fix)
    with pytest.raises(Exception):
        loss.auc_judd_batch(s.cpu(), fix.cpu())


def test_torch_op_and_opcheck():
    from vinet_amd import ops  # noqa: F401
    case = BY["smooth60"]
    s, fix = _inputs(case)
    got = torch.ops.vinet.auc_judd(s, fix, False)
    _check(case, got.cpu().numpy(), case.nfix, None)
    torch.library.opcheck(torch.ops.vinet.auc_judd.default, (s, fix, False), test_utils=("test_schema", "test_faketensor"))
    c64 = BY["jit30"]
    s64, f64 = _inputs(c64)
    torch.library.opcheck(torch.ops.vinet.auc_judd.default, (s64, f64, True), test_utils=("test_schema", "test_faketensor"))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = torch.ops.vinet.auc_judd(torch.empty(5, 8, 8), torch.empty(5, 8, 8), False)
        assert tuple(out.shape) == (5,) and out.dtype == torch.float64


@pytest.mark.parametrize("name", ["quant400", "dhf900", "nan", "large"])
def test_batch_item_equals_the_map_alone_and_runs_repeat(name):
    case = BY[name]
    s, fix = _inputs(case)
    first, nf, ab = _raw(s, fix)
    again, _, ab2 = _raw(s, fix)
    assert first.tobytes() == again.tobytes() and np.array_equal(ab, ab2)            # bit-identical, NaN included
    for b in range(case.B):
        alone, _, _ = _raw(s[b:b + 1].contiguous(), fix[b:b + 1].contiguous(), want_above=False)
        assert alone.tobytes() == first[b:b + 1].tobytes()


@pytest.mark.parametrize("name", ["smooth60", "quant400", "dhf900", "jit30", "ends", "nan", "fix64"])
def test_lds_route_and_workspace_route_agree_bit_for_bit(name):
    case = BY[name]
    assert case.nfix.max() <= MC.LDS_CAP
    s, fix = _inputs(case)
    a = _raw(s, fix)
    L.set_option("auc_ws", 1)
    try:
        w = _raw(s, fix)
    finally:
        L.set_option("auc_ws", 0)
    assert a[0].tobytes() == w[0].tobytes() and np.array_equal(a[1], w[1]) and np.array_equal(a[2], w[2])
    _check(case, *w)


@pytest.mark.parametrize("name", ["quant400", "jit30"])
def test_jitter_without_given_noise_lies_in_the_references_spread(name):
    """the two tie-heavy cases, where jitter has a real effect: between the minimum and maximum of the reference's 32 recorded runs
    with seeded noise, widened by that spread once"""
    from vinet_amd import loss
    case = BY[name]
    lo, hi = case.jitter_minmax
    s, fix = torch.from_numpy(case.s).to(_dev()), torch.from_numpy(case.fix).to(_dev())
    torch.manual_seed(5)
    for b in range(case.B):
        v = loss.auc_judd(s[b], fix[b])                      # jitter=True is the default
        spread = hi[b] - lo[b]
        print("%s[%d]: jittered %.6f, reference runs [%.6f, %.6f]" % (name, b, v, lo[b], hi[b]))
        assert spread > 0 and lo[b] - spread <= v <= hi[b] + spread


def _write_tree(root, n_videos=2, n_frames=3):
    """P / G trees in the DHF1K layout: 45x80 predictions, 90x160 ground truth and fixations, one frame with an empty ground truth"""
    from PIL import Image
    from vinet_amd import synth
    P, G = os.path.join(root, "pred"), os.path.join(root, "gt")
    arrays = {}
    for vi in range(n_videos):
        name = "video%d" % vi
        for d in (os.path.join(P, name), os.path.join(G, name, "maps"), os.path.join(G, name, "fixation")):
            os.makedirs(d)
        gt = (synth.saliency_maps("gev_gt%d" % vi, n_frames, 90, 160, vi, noise=0.0) * 255).astype(np.uint8)
        pred = synth.saliency_maps("gev_pred%d" % vi, n_frames, 45, 80, vi, levels=256).astype(np.uint8)
        fix = synth.fixation_maps(synth.fixations("gev_fix%d" % vi, gt, 40, vi), 90, 160, dtype=np.uint8)
        if vi == 1:
            gt[1] = 0
        for i in range(n_frames):
            key = "%04d" % (i + 1)
            Image.fromarray(pred[i]).save(os.path.join(P, name, key + ".png"))
            Image.fromarray(gt[i]).save(os.path.join(G, name, "maps", key + ".png"))
            Image.fromarray(fix[i] * 255).save(os.path.join(G, name, "fixation", key + ".png"))
            arrays[(name, key)] = (pred[i], gt[i], fix[i])
    return P, G, arrays


@pytest.mark.parametrize("blur", [False, True])
def test_evaluator_command_on_a_synthetic_tree(tmp_path, blur):
    from vinet_amd import loss, preprocess, utils
    P, G, arrays = _write_tree(str(tmp_path))
    out = os.path.join(str(tmp_path), "scores.json")
    cmd = [sys.executable, "-m", "vinet_amd.evaluate", "--pred_dir", P, "--gt_dir", G, "--batch", "2", "--jitter", "0", "--per_frame", "--json", out]
    r = subprocess.run(cmd + (["--blur"] if blur else []), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    heads = [l.split(":")[0] for l in lines[-11:-1]]
    assert heads == ["SIM", "CC", "NSS", "AUCJ", "KLdiv", "Avg Video SIM", "Avg Video CC", "Avg Video NSS", "Avg Video AUCJ", "Avg Video KLdiv"]
    assert "processing video0" in r.stdout and "No saliency" in r.stdout
    s = json.load(open(out))
    assert s["frames"] == 5 and s["skipped"] == 1 and s["num_videos"] == 2
    dev = _dev()
    tot = dict.fromkeys(("SIM", "CC", "NSS", "AUCJ"), 0.0)
    for (name, key), (p, g, f) in arrays.items():
        pt, gt, ft = (torch.from_numpy(a[None]).to(dev) for a in (p, g, f))
        sm = utils.resize_blur(pt.float(), gt.shape[1:]) if blur else preprocess.gt_to_tensor(pt, gt.shape[1:])
        one = {"SIM": float(loss.similarity(sm, gt.float())), "CC": float(loss.cc(sm, gt.float())), "NSS": float(loss.nss(sm, ft.float())),
               "AUCJ": loss.auc_judd(sm, ft.float(), jitter=False)}
        row = s["videos"][name]["per_frame"][key]
        for m, v in one.items():
            if math.isnan(v):
                assert math.isnan(row[m])
            elif m == "AUCJ":
                assert row[m] == v                                     # same kernel, same map: the same bits
            else:
                assert row[m] == pytest.approx(v, rel=2e-6)            # the per-map functions return float32
        if not math.isnan(one["CC"]):
            for m in tot:
                tot[m] += one[m]
    for m in tot:
        assert s["frame_weighted"][m] == pytest.approx(tot[m] / 5, rel=2e-6)


def test_evaluator_synthetic_mode():
    r = subprocess.run([sys.executable, "-m", "vinet_amd.evaluate", "--synthetic", "6", "--batch", "4"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AUCJ:" in r.stdout and "Avg Video KLdiv:" in r.stdout and "frames scored: 6" in r.stdout
