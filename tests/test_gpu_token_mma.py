"""The arithmetic modes of the token encoder's linear products on the MI355X (csrc/tk_gemm_bf16.h, VINET_TK_MMA_*).

One product (vinet_token_gemm), bit for bit: operands whose split is known by construction and whose sums fp32 adds exactly in any
order (tests/token_mma_cases.py), so F32 must give sum a b, BF16X3 sum a b - sum lo lo and BF16 sum hi hi, each EXACTLY, and the three
differ: the mode is applied, no term is missing and none is counted twice.  Every form x every epilogue, at every tile edge of both
tile heights, with row strides above the widths (NaN in the gaps), a sentinel tail and bias / res at an offset between NaNs.

One product on random data: against the float64 sum of the mode's own terms (numpy statement of the split), gate
(K + 4) 2^-24 sum |term| per element; the distance from the unrounded product goes to the parity report.

The whole encoder: against tests/token_mma_cases.torch_run_mode (tests/transformer_model.py's stages around mode-arithmetic linears).
Upper bound, per tensor: max |device - fp64 model| <= 2 x max |fp32 emulation - fp64 model| (both relative to the tensor's largest
element; the fp64 model is the unrounded one).  Lower bound: in bf16 mode the device differs from its own F32-mode result by at
least a quarter of the emulation's error -- on the output, the input gradient and the weight matrices' gradients, the tensors that
come out of a mode product (a LayerNorm's bias gradient in the last layer is a column sum no product feeds: it cannot differ).

The model: the avfusion32 golden through the public class under token_mma = "match", and the default option against a run that
calls the entry points without a mode."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_fusion as FU
from tests import test_gpu_transformer as T0
from tests import token_mma_cases as TC
from tests import transformer_model as TM
from tests.gpu_report import note as _note
from tests.test_gpu_fusion import _real_library  # noqa: F401  (autouse: the real library, fp32 context)
from vinet_amd import _lib as L
from vinet_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = FU.DEV
SENT = -12345.0
NAN = float("nan")


@pytest.fixture(autouse=True)
def _option_restored():
    yield
    E.configure(token_mma="fp32")


# ---- one product ---------------------------------------------------------------------------------------------------------------
def _padded(arr, ld, fill=NAN, lead=0, tail=8):
    """[rows][width] numpy -> (device buffer, byte offset of element [0][0]): rows `ld` apart, `fill` in the gaps, before and behind"""
    rows, width = arr.shape
    buf = torch.full((lead + rows * ld + tail,), fill, dtype=torch.float32)
    torch.as_strided(buf, (rows, width), (ld, 1), lead).copy_(torch.from_numpy(arr))
    return buf.to(DEV), 4 * lead


def _gemm(mma, form, epi, ops, M, N, K):
    """vinet_token_gemm on padded operands; returns (C [M][N] numpy, every other element of C's buffer)"""
    A, B = ops["A"], ops["B"]
    lda, ldb, ldc = A.shape[1] + 4, B.shape[1] + 8, N + 3
    a, _ = _padded(A, lda)
    b, _ = _padded(B, ldb)
    c0 = ops["c0"] if epi == 4 else np.full((M, N), SENT, dtype=np.float32)
    c, _ = _padded(c0, ldc, fill=SENT, tail=37)
    bias, boff = _padded(ops["bias"][None, :], N, lead=3)
    res, roff = _padded(ops["res"], ldc, lead=5)
    rc = L.load().vinet_token_gemm(mma, form, epi, a.data_ptr(), lda, b.data_ptr(), ldb, c.data_ptr(), ldc, M, N, K,
                                   bias.data_ptr() + boff if epi in (1, 2) else None, res.data_ptr() + roff if epi == 3 else None,
                                   torch.cuda.current_stream().cuda_stream)
    L.check(rc, "vinet_token_gemm")
    flat = c.cpu()
    inside = torch.zeros(flat.numel(), dtype=torch.bool)
    torch.as_strided(inside, (M, N), (ldc, 1)).fill_(True)
    return torch.as_strided(flat, (M, N), (ldc, 1)).numpy().copy(), flat[~inside]


@pytest.mark.parametrize("epi", TC.EPIS)
@pytest.mark.parametrize("form", TC.FORMS)
def test_one_product_is_exact_in_every_mode_and_the_modes_differ(form, epi):
    shapes = TC.SHAPES + ([TC.SLICED_SHAPE] if form == 2 else [])
    for M, N, K in shapes:
        ops = TC.exact_operands(form, epi, M, N, K, seed=1000 * form + K + M)
        got = {}
        for mode, mma in TC.MODES.items():
            c, outside = _gemm(mma, form, epi, ops, M, N, K)
            want = TC.epilogue_np(epi, ops["want"][mode], ops["bias"].astype(np.int64), ops["res"].astype(np.int64), ops["c0"].astype(np.int64))
            bad = int((c.astype(np.float64) != want.astype(np.float64)).sum())
            print("form %d epi %d %4d x %3d x %3d %-6s wrong elements: %d" % (form, epi, M, N, K, mode, bad))
            assert bad == 0, (form, epi, M, N, K, mode, bad)
            assert bool((outside == SENT).all()), "gaps or tail of C written: form %d epi %d %s %s" % (form, epi, (M, N, K), mode)
            got[mode] = c
        if epi != 2:      # (a ReLU may clip the few elements that differ)
            assert not np.array_equal(got["fp32"], got["bf16x3"]) and not np.array_equal(got["bf16x3"], got["bf16"]) \
                and not np.array_equal(got["fp32"], got["bf16"]), (form, epi, M, N, K)


RANDOM_SHAPES = [(4, 4, 16), (68, 132, 80), (132, 68, 256), (TC.TALL_FROM + 4, 68, 48)]


@pytest.mark.parametrize("form", TC.FORMS)
def test_one_product_on_random_data_sums_its_modes_own_terms(form):
    shapes = RANDOM_SHAPES + ([TC.SLICED_SHAPE] if form == 2 else [])
    for M, N, K in shapes:
        rng = np.random.default_rng(77 + form + M + K)
        a = rng.standard_normal((M, K)).astype(np.float32)
        b = rng.standard_normal((K, N)).astype(np.float32)
        ops = dict(A=np.ascontiguousarray(a.T if form == 2 else a), B=np.ascontiguousarray(b.T if form == 0 else b),
                   bias=rng.standard_normal(N).astype(np.float32), res=np.zeros((M, N), np.float32), c0=np.zeros((M, N), np.float32))
        unrounded = a.astype(np.float64) @ b.astype(np.float64)
        for mode, mma in TC.MODES.items():
            terms = TC.terms_np(mode, a, b)
            ref = sum(x.astype(np.float64) @ y.astype(np.float64) for x, y in terms) + ops["bias"].astype(np.float64)[None, :]
            mag = sum(np.abs(x).astype(np.float64) @ np.abs(y).astype(np.float64) for x, y in terms) + np.abs(ops["bias"]).astype(np.float64)[None, :]
            c, outside = _gemm(mma, form, 1, ops, M, N, K)
            gate = (K + 4) * 2.0 ** -24 * mag
            err = np.abs(c.astype(np.float64) - ref)
            worst = float((err / gate).max())
            dist = float(np.abs(c.astype(np.float64) - unrounded - ops["bias"][None, :]).max() / np.abs(unrounded).max())
            print("form %d %4d x %3d x %3d %-6s err / gate %.3f, distance from the unrounded product %.3e" % (form, M, N, K, mode, worst, dist))
            _note("token_mma_product_f%d_%dx%dx%d_%s" % (form, M, N, K, mode), dict(worst_err_over_gate=worst, rel_distance_from_unrounded=dist))
            assert worst <= 1.0, (form, M, N, K, mode, worst)
            assert bool((outside == SENT).all())


# ---- the whole encoder ---------------------------------------------------------------------------------------------------------
class ModeEncoder(FU.Encoder):
    """tests.test_gpu_fusion.Encoder through the entry points that take the mode"""

    def __init__(self, case, mode, **kw):
        super().__init__(case, **kw)
        self.mma = TC.MODES[mode]
        assert self.lib.vinet_token_encoder_workspace_mma(C.byref(self.d), self.mma) == self.ws.numel()

    def forward(self, xview, yview, masks=None):
        self.d.masks = masks.data_ptr() if masks is not None else None
        L.check(self.lib.vinet_token_encoder_fwd_mma(C.byref(self.d), self.mma, C.byref(xview), C.byref(yview), self.stream), "vinet_token_encoder_fwd_mma")

    def backward(self, dyview, dxview, grads):
        self.garr = (C.c_void_p * len(grads))(*[g.data_ptr() if g is not None else None for g in grads])
        self.d.grads, self.d.masks = self.garr, None
        L.check(self.lib.vinet_token_encoder_bwd_mma(C.byref(self.d), self.mma, C.byref(dyview), C.byref(dxview) if dxview is not None else None,
                                                     self.stream), "vinet_token_encoder_bwd_mma")


UPPER, LOWER = 2.0, 0.25
_EMU = {}


def _emulation(case, mode):
    """the fp32 emulation of `mode` on the case's shared inputs; computed once, never modified"""
    if (case, mode) not in _EMU:
        S, Ef, F, H, NL, B = case
        x, proj = FU._inputs(case)
        sd = {k: v.clone() for k, v in FU._state_dict(case).items()}
        _EMU[(case, mode)] = TC.torch_run_mode(sd, x, proj, mode, torch.float32, nhead=H, n_layers=NL)
    return _EMU[(case, mode)]


def _rel(a, r):
    return float((a.double().cpu() - r).abs().max()) / float(r.abs().max())


def _upper(name, mode, got, emu, r64, keys=None):
    """per tensor: device error against the unrounded fp64 model <= UPPER x the emulation's; all measured and printed first"""
    bad, worst, worst_k = [], 0.0, None
    for k in (r64 if keys is None else keys):
        assert got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all()), k
        dev, em = _rel(got[k], r64[k]), _rel(emu[k], r64[k])
        ratio = dev / em if em > 0 else (0.0 if dev == 0 else float("inf"))
        print("%-20s %-6s %-62s device %.3e emulation %.3e ratio %.2f" % (name, mode, k, dev, em, ratio))
        if ratio > worst:
            worst, worst_k = ratio, k
        if ratio > UPPER:
            bad.append((k, dev, em, ratio))
    _note("token_mma_%s_%s" % (name, mode), dict(worst_device_over_emulation_error=worst, worst_tensor=worst_k, gate=UPPER))
    assert not bad, bad


def _product_fed(k):
    return k in ("train_y", "train_gx") or k.endswith(("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight"))


ENCODER_CASES = {
    "s1": (1, 32, 48, 2, 2, 3), "s17": (17, 32, 48, 2, 2, 3), "s65": FU.MODE_CASE, "s21_e512": (21, 512, 512, 4, 1, 2),
    "f16": (21, 32, 16, 2, 1, 2), "real_b1_l1": FU.REAL_B1,
}


@pytest.mark.parametrize("name", list(ENCODER_CASES))
def test_encoder_in_each_mode_against_its_emulation(name):
    case = ENCODER_CASES[name]
    x, proj = FU._inputs(case)
    r64, _ = FU._reference(case)
    got = {mode: ModeEncoder(case, mode).run(x, proj) for mode in TC.MODES}
    old = FU.Encoder(case).run(x, proj)
    for k in old:
        assert torch.equal(old[k], got["fp32"][k]), "F32 mode is not the entry point without a mode: %s" % k
    for mode in ("bf16x3", "bf16"):
        assert set(got[mode]) == set(r64)
        _upper(name, mode, got[mode], _emulation(case, mode), r64)
    emu = _emulation(case, "bf16")
    short = []
    for k in filter(_product_fed, r64):
        moved, em = float((got["bf16"][k].double() - got["fp32"][k].double()).abs().max()) / float(r64[k].abs().max()), _rel(emu[k], r64[k])
        print("%-20s bf16 vs F32 on the device %-56s moved %.3e emulation error %.3e" % (name, k, moved, em))
        if moved < LOWER * em:
            short.append((k, moved, em))
    assert not short, "bf16 mode is closer to F32 mode than its arithmetic allows: %s" % short


def test_eval_mode_in_each_mode():
    case = FU.MODE_CASE
    x, proj = FU._inputs(case)
    r64, _ = FU._reference(case)
    for mode in ("bf16x3", "bf16"):
        got = ModeEncoder(case, mode, train=0).run(x, proj)
        _upper("eval_s65", mode, got, _emulation(case, mode), r64, keys=["train_y"])


def test_dropout_masks_do_not_depend_on_the_mode_and_the_modes_hold_under_them():
    case = FU.MODE_CASE
    S, Ef, F, H, NL, B = case
    p = 0.1
    x, proj = FU._inputs(case)
    nbytes = NL * (B * H * S * S + B * S * (2 * Ef + F))
    runs, masks = {}, {}
    for mode in TC.MODES:
        enc = ModeEncoder(case, mode, p=p, seed=4321)
        masks[mode] = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        runs[mode] = enc.run(x, proj, masks[mode])
        assert int(enc.step) == 1
    flat = masks["fp32"].cpu()
    assert 0.85 < float(flat.float().mean()) < 0.95
    for mode in ("bf16x3", "bf16"):
        assert torch.equal(masks[mode].cpu(), flat), "the keep masks of %s differ from F32 mode's" % mode
    mk = TM.split_masks(flat, NL, B, S, Ef, F, H)
    sd = {k: v.clone() for k, v in FU._state_dict(case).items()}
    r64 = T0._torch_run(sd, x, proj, torch.float64, p, mk, nhead=H, n_layers=NL)
    for mode in ("bf16x3", "bf16"):
        emu = TC.torch_run_mode(sd, x, proj, mode, torch.float32, p, mk, nhead=H, n_layers=NL)
        _upper("dropout_s65", mode, runs[mode], emu, r64)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_two_clips_equal_two_single_clips_and_two_runs_agree_bit_for_bit(mode):
    """the real shape, B = 2: 704 workspace rows, so the weight gradients run in two slices (512 + 192 rows) and a clip boundary
    lies inside a GEMM tile"""
    case = (339, 512, 512, 4, 1, 2)
    x, proj = FU._inputs(case)
    enc = ModeEncoder(case, mode)
    a, b = enc.run(x, proj), enc.run(x, proj)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between two runs" % k
    r64, _ = FU._reference(case)
    _upper("real_b2_l1", mode, a, _emulation(case, mode), r64)
    for i in range(2):
        one = ModeEncoder(case[:5] + (1,), mode, sd=FU._state_dict(case)).run(x[:, i:i + 1].contiguous(), proj[:, i:i + 1].contiguous())
        assert torch.equal(a["train_y"][:, i], one["train_y"][:, 0]), i
        assert torch.equal(a["train_gx"][:, i], one["train_gx"][:, 0]), i


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_null_gradients_are_skipped_and_a_second_backward_accumulates(mode):
    case = FU.MODE_CASE
    x, proj = FU._inputs(case)
    enc = ModeEncoder(case, mode)
    full = enc.run(x, proj)
    xb, pb = enc.dense(x), enc.dense(proj)
    y, gx = torch.empty_like(xb), torch.full_like(xb, 7.0)
    enc.forward(enc.view(xb), enc.view(y))
    grads = enc.zero_grads()
    skipped = [i % 3 == 1 for i in range(len(grads))]
    enc.backward(enc.view(pb), None, [None if s else g for g, s in zip(grads, skipped)])
    torch.cuda.synchronize()
    assert bool((gx == 7.0).all())
    for n, g, s in zip(enc.names, grads, skipped):
        if s:
            assert not bool(g.any()), n
        else:
            assert torch.equal(g.cpu(), full["train_g:" + n]), n
    grads = enc.zero_grads()
    enc.backward(enc.view(pb), enc.view(gx), grads)
    enc.backward(enc.view(pb), enc.view(gx), grads)
    torch.cuda.synchronize()
    assert torch.equal(gx.permute(1, 0, 2).cpu(), full["train_gx"])
    for n, g in zip(enc.names, grads):
        assert torch.equal(g.cpu(), 2 * full["train_g:" + n]), n


def test_backward_uses_the_mode_its_forward_resolved():
    """fusion.token_encoder_forward resolves the option once: changing it between forward and backward changes nothing"""
    from vinet_amd import fusion
    from vinet_amd import model as VM
    case = FU.MODE_CASE
    S, Ef, F, H, NL, B = case
    tf = VM._TransformerParams(Ef, hidden_size=F, nhead=H, num_encoder_layers=NL, max_len=S, max_head_width=VM.TOKEN_ENCODER_MAX_HEAD_WIDTH)
    tf.load_state_dict(FU._state_dict(case))
    for l in tf.transformer_encoder.layers:
        l.dropout.p = l.dropout1.p = l.dropout2.p = 0.0
        l.self_attn.dropout = 0.0
    tf = tf.to(DEV).train()
    x, proj = FU._inputs(case)
    xn = x.permute(1, 2, 0).reshape(B, Ef, S, 1, 1).contiguous().to(DEV)
    gn = proj.permute(1, 2, 0).reshape(B, Ef, S, 1, 1).contiguous().to(DEV)

    def run(fwd_mode, bwd_mode):
        for q in tf.parameters():
            q.grad = None
        xr = xn.detach().requires_grad_(True)
        E.configure(token_mma=fwd_mode)
        y = fusion.token_encoder_tokens(tf, xr)
        E.configure(token_mma=bwd_mode)
        (y * gn).sum().backward()
        return [y.detach().clone(), xr.grad.clone()] + [q.grad.clone() for q in tf.parameters() if q.grad is not None]

    same, switched, plain = run("bf16", "bf16"), run("bf16", "fp32"), run("fp32", "fp32")
    assert len(same) == len(switched) == len(plain) > 10
    for a, b in zip(same, switched):
        assert torch.equal(a, b)
    assert not torch.equal(same[0], plain[0]) and not torch.equal(same[1], plain[1])


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_avfusion_map_fp32s_with_matching_token_arithmetic():
    E.configure(token_mma="match")
    y, z, meta = FU._avfusion("fp32s")
    d = float((y.cpu().double() - torch.from_numpy(z["y"]).double()).abs().max())
    _note("token_mma_avfusion_fp32s_match", dict(max_abs=d, top2_gap=meta["top2_gap"]))
    print("avfusion fp32s + match: max abs", d)
    assert d <= 1e-3, d
    assert int(y.reshape(-1).argmax()) == meta["argmax"]


def test_avfusion_map_bf16_with_matching_token_arithmetic():
    E.configure(token_mma="match")
    y, z, meta = FU._avfusion("bf16")
    ref = torch.from_numpy(z["y"]).double().reshape(-1)
    mine = y.cpu().double().reshape(-1)
    d = float((mine - ref).abs().max())
    cc = float(np.corrcoef(mine.numpy(), ref.numpy())[0, 1])
    top5 = torch.topk(ref, 5).indices.tolist()
    _note("token_mma_avfusion_bf16_match", dict(max_abs=d, cc=cc, argmax_matches=int(mine.argmax()) == meta["argmax"]))
    print("avfusion bf16 + match: max abs", d, "cc", cc)
    assert d <= 2.5e-2 and cc >= 0.999 and int(mine.argmax()) in top5


def test_the_default_option_is_the_entry_points_without_a_mode_bit_for_bit(monkeypatch):
    assert E.TOKEN_MMA == "fp32"
    y_default, _, _ = FU._avfusion("fp32s")
    lib, seen = L.load(), []

    def ws(d, mma):
        seen.append(("ws", mma))
        return lib.vinet_token_encoder_workspace(d)

    def fwd(d, mma, x, y, s):
        seen.append(("fwd", mma))
        return lib.vinet_token_encoder_fwd(d, x, y, s)

    monkeypatch.setattr(lib, "vinet_token_encoder_workspace_mma", ws)
    monkeypatch.setattr(lib, "vinet_token_encoder_fwd_mma", fwd)
    y_old, _, _ = FU._avfusion("fp32s")
    assert seen == [("ws", L.TK_MMA_F32), ("fwd", L.TK_MMA_F32)], seen
    assert torch.equal(y_default, y_old)
    monkeypatch.undo()
    # and "match" hands the fp32s context's own arithmetic to the same call (the map itself may round to the same floats)
    real, modes = lib.vinet_token_encoder_fwd_mma, []

    def spy(d, mma, x, y, s):
        modes.append(mma)
        return real(d, mma, x, y, s)

    monkeypatch.setattr(lib, "vinet_token_encoder_fwd_mma", spy)
    E.configure(token_mma="match")
    y_match, _, _ = FU._avfusion("fp32s")
    assert modes == [L.TK_MMA_BF16X3], modes
    _note("token_mma_avfusion_fp32s_match_vs_default", dict(max_abs=float((y_match - y_default).abs().max())))


def test_training_step_fp32s_with_matching_token_arithmetic_moves_every_parameter_and_the_loss_falls():
    from vinet_amd import loss as VL
    from vinet_amd import optim as VO
    from vinet_amd import parallel
    E.configure(token_mma="match")
    m, x, a, gt = FU._train_setup("fp32s")
    names = {id(p): k for k, p in m.named_parameters()}
    params = parallel.trainable_parameters(m)
    before = {names[id(p)]: p.detach().clone() for p in params}
    assert len([k for k in before if k.startswith(("transformer.", "conv_in_1x1.", "audio_conv_1x1."))]) == 40
    opt = VO.Adam(params, lr=1e-4)
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = VL.kldiv(m(x, a), gt)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if step == 0:
            now = dict(m.named_parameters())
            for k, v in before.items():
                assert not torch.equal(now[k].detach(), v), "%s did not move" % k
    _note("token_mma_avfusion_train_fp32s_match", dict(losses=losses))
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses
