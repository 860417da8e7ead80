"""The arithmetic modes of the token encoder's attention on the MI355X (csrc/tk_attn_bf16.h; the `attn` argument of the _attn entry
points, VINET_TK_MMA_* values).

One stage through vinet_token_attn_fwd / _bwd, bit for bit in all three modes, on the exact cases of tests/token_attn_cases.py:
operands whose split is known by construction and whose sums fp32 adds exactly in any order, so each mode must give the sum of ITS
terms exactly, and the modes differ.  Outputs go into NaN-filled buffers with a sentinel tail: padding rows must come back zero,
the tail must survive; qkv's padding rows are NaN (no kernel may read them).

The whole encoder on random data against tests/token_attn_cases.torch_run_modes.  Upper bound per tensor, the project's own
(tests/test_gpu_token_mma.py): max |device - fp64 model| <= 2 x max |fp32 emulation - fp64 model|.  Lower bound: with fp32 linears
and bf16 attention the device is away from the all-fp32 device result by at least a quarter of the emulation's error on the
attention-fed tensors (output, input gradient, in_proj gradients).

The model: the avfusion32 golden and one training step under token_mma = token_attn = "match"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_fusion as FU
from tests import test_gpu_token_mma as GM
from tests import test_gpu_transformer as T0
from tests import token_attn_cases as AC
from tests import token_mma_cases as TC
from tests import transformer_model as TM
from tests.gpu_report import note as _note
from tests.test_gpu_fusion import _real_library  # noqa: F401  (autouse: the real library, fp32 context)
from vinet_amd import _lib as L
from vinet_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = FU.DEV
SENT = -12345.0
TAIL = 37
UPPER, LOWER = GM.UPPER, GM.LOWER


@pytest.fixture(autouse=True)
def _options_restored():
    yield
    E.configure(token_mma="fp32")
    E.set_token_attn("fp32")


# ---- one stage through the handle ------------------------------------------------------------------------------------------------
def _dev(arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(DEV)


def _out(n):
    """NaN-filled output of n floats with a sentinel tail"""
    t = torch.full((n + TAIL,), float("nan"), dtype=torch.float32)
    t[n:] = SENT
    return t.to(DEV)


def _tail_ok(t, n):
    return bool((t[n:].cpu() == SENT).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward(attn, c):
    """vinet_token_attn_fwd on a case: (P [B, H, S, S], ao [B, H, S, D]) numpy; checks padding rows and tails"""
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    Ef, Sp = H * D, AC.sp_of(S)
    qkv = _dev(AC.pack_qkv(c["q"], c["k"], c["v"]))
    P, ao = _out(B * H * S * S), _out(B * Sp * Ef)
    L.check(L.load().vinet_token_attn_fwd(attn, qkv.data_ptr(), B, S, Ef, H, P.data_ptr(), ao.data_ptr(), _stream()), "vinet_token_attn_fwd")
    torch.cuda.synchronize()
    assert _tail_ok(P, B * H * S * S) and _tail_ok(ao, B * Sp * Ef), "a tail was written"
    rows, pad = AC.unpack_rows(ao[:B * Sp * Ef].cpu().numpy(), B, H, S, D)
    assert not pad.any(), "ao's padding rows are not zero"
    return P[:B * H * S * S].cpu().numpy().reshape(B, H, S, S), rows


def _backward(attn, c):
    """vinet_token_attn_bwd on a case with caller-supplied P and ao: dict(dot [B, H, S], dq, dk, dv [B, H, S, D]) numpy"""
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    Ef, Sp = H * D, AC.sp_of(S)
    qkv, P = _dev(AC.pack_qkv(c["q"], c["k"], c["v"])), _dev(c["P"])
    dao, ao = _dev(AC.pack_rows(c["dao"], 0.0)), _dev(AC.pack_rows(c["ao"], 0.0))
    dot, dqkv = _out(B * Sp * H), _out(B * Sp * 3 * Ef)
    L.check(L.load().vinet_token_attn_bwd(attn, qkv.data_ptr(), P.data_ptr(), dao.data_ptr(), ao.data_ptr(), B, S, Ef, H, dot.data_ptr(),
                                          dqkv.data_ptr(), _stream()), "vinet_token_attn_bwd")
    torch.cuda.synchronize()
    assert _tail_ok(dot, B * Sp * H) and _tail_ok(dqkv, B * Sp * 3 * Ef), "a tail was written"
    g = dqkv[:B * Sp * 3 * Ef].cpu().numpy().reshape(B * Sp, 3 * Ef)
    out = {}
    for i, name in enumerate(("dq", "dk", "dv")):
        out[name], pad = AC.unpack_rows(np.ascontiguousarray(g[:, i * Ef:(i + 1) * Ef]), B, H, S, D)
        assert not pad.any(), "%s's padding rows are not zero" % name
    d = dot[:B * Sp * H].cpu().numpy().reshape(B, Sp, H)
    assert not d[:, S:].any()
    out["dot"] = np.transpose(d[:, :S], (0, 2, 1))
    return out


def _exact(kind, S, D, mode, name, got, want):
    bad = int((got.astype(np.float64) != np.asarray(want, np.float64)).sum())
    print("%-6s S %3d D %3d %-6s %-3s wrong elements: %d" % (kind, S, D, mode, name, bad))
    assert bad == 0, (kind, S, D, mode, name, bad)


def _modes_differ(kind, S, D, got, names):
    for n in names:
        a, b, c = (got[m][n] for m in ("fp32", "bf16x3", "bf16"))
        assert not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c), (kind, S, D, n)


@pytest.mark.parametrize("D", AC.POW2_D)
def test_scores_and_ao_are_exact_in_every_mode_and_the_modes_differ(D):
    for S in [s for s, d in AC.SCORES_CASES if d == D]:
        c = AC.exact_scores_case(S, D, AC.case_seed(1, S, D))
        got = {}
        for mode, attn in AC.MODES.items():
            P, ao = _forward(attn, c)
            _exact("scores", S, D, mode, "P", P, c["want"][mode]["P"])
            _exact("scores", S, D, mode, "ao", ao, c["want"][mode]["ao"])
            got[mode] = dict(P=P, ao=ao)
        _modes_differ("scores", S, D, got, ("P", "ao"))


@pytest.mark.parametrize("D", sorted(set(d for _, d in AC.FLAT_CASES)))
def test_equal_scores_at_every_head_width_and_sequence_edge(D):
    for S in [s for s, d in AC.FLAT_CASES if d == D]:
        c = AC.exact_flat_case(S, D, AC.case_seed(2, S, D))
        got = {}
        for mode, attn in AC.MODES.items():
            P, ao = _forward(attn, c)
            _exact("flat", S, D, mode, "P", P, c["want"][mode]["P"])
            _exact("flat", S, D, mode, "ao", ao, c["want"][mode]["ao"])
            got[mode] = ao
        assert not np.array_equal(got["fp32"], got["bf16"]), (S, D)


@pytest.mark.parametrize("D", AC.POW2_D)
def test_dq_dk_dv_from_a_known_ds_are_exact_in_every_mode_and_the_modes_differ(D):
    for S in [s for s, d in AC.DS_CASES if d == D]:
        c = AC.exact_ds_case(S, D, AC.case_seed(3, S, D))
        got = {}
        for mode, attn in AC.MODES.items():
            got[mode] = _backward(attn, c)
            for n in ("dot", "dq", "dk", "dv"):
                _exact("ds", S, D, mode, n, got[mode][n], c["want"][mode][n])
        _modes_differ("ds", S, D, got, ("dq", "dk", "dv"))


@pytest.mark.parametrize("D", sorted(set(d for _, d in AC.DP_CASES)))
def test_dp_shows_through_the_split_of_ds_at_every_head_width(D):
    for S in [s for s, d in AC.DP_CASES if d == D]:
        c = AC.exact_dp_case(S, D, AC.case_seed(4, S, D))
        got = {}
        for mode, attn in AC.MODES.items():
            got[mode] = _backward(attn, c)
            for n in ("dot", "dq", "dk", "dv"):
                _exact("dp", S, D, mode, n, got[mode][n], c["want"][mode][n])
        _modes_differ("dp", S, D, got, ("dq", "dk"))


# ---- the whole encoder -----------------------------------------------------------------------------------------------------------
class AttnEncoder(FU.Encoder):
    """tests.test_gpu_fusion.Encoder through the entry points that take both modes"""

    def __init__(self, case, mma, attn, **kw):
        super().__init__(case, **kw)
        self.mma, self.attn = TC.MODES[mma], TC.MODES[attn]
        assert self.lib.vinet_token_encoder_workspace_attn(C.byref(self.d), self.mma, self.attn) == self.ws.numel()

    def forward(self, xview, yview, masks=None):
        self.d.masks = masks.data_ptr() if masks is not None else None
        L.check(self.lib.vinet_token_encoder_fwd_attn(C.byref(self.d), self.mma, self.attn, C.byref(xview), C.byref(yview), self.stream),
                "vinet_token_encoder_fwd_attn")

    def backward(self, dyview, dxview, grads):
        self.garr = (C.c_void_p * len(grads))(*[g.data_ptr() if g is not None else None for g in grads])
        self.d.grads, self.d.masks = self.garr, None
        L.check(self.lib.vinet_token_encoder_bwd_attn(C.byref(self.d), self.mma, self.attn, C.byref(dyview),
                                                      C.byref(dxview) if dxview is not None else None, self.stream), "vinet_token_encoder_bwd_attn")


PAIRS = (("bf16x3", "bf16x3"), ("bf16", "bf16"), ("fp32", "bf16"))
_EMU = {}


def _emulation(case, mma, attn):
    """the fp32 emulation of (mma, attn) on the case's shared inputs; computed once, never modified"""
    if (case, mma, attn) not in _EMU:
        S, Ef, F, H, NL, B = case
        x, proj = FU._inputs(case)
        sd = {k: v.clone() for k, v in FU._state_dict(case).items()}
        _EMU[(case, mma, attn)] = AC.torch_run_modes(sd, x, proj, mma, attn, torch.float32, nhead=H, n_layers=NL)
    return _EMU[(case, mma, attn)]


def _upper(name, pair, got, emu, r64, keys=None):
    """per tensor: device error against the unrounded fp64 model <= UPPER x the emulation's; all measured and printed first"""
    bad, worst, worst_k = [], 0.0, None
    for k in (r64 if keys is None else keys):
        assert got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all()), k
        dev, em = GM._rel(got[k], r64[k]), GM._rel(emu[k], r64[k])
        ratio = dev / em if em > 0 else (0.0 if dev == 0 else float("inf"))
        print("%-14s %-6s/%-6s %-62s device %.3e emulation %.3e ratio %.2f" % (name, pair[0], pair[1], k, dev, em, ratio))
        if ratio > worst:
            worst, worst_k = ratio, k
        if ratio > UPPER:
            bad.append((k, dev, em, ratio))
    _note("token_attn_%s_%s_%s" % (name, pair[0], pair[1]), dict(worst_device_over_emulation_error=worst, worst_tensor=worst_k, gate=UPPER))
    assert not bad, bad


def _attention_fed(k):
    return k in ("train_y", "train_gx") or k.endswith(("in_proj_weight", "in_proj_bias"))


@pytest.mark.parametrize("name", list(GM.ENCODER_CASES))
def test_encoder_in_each_pair_of_modes_against_its_emulation(name):
    case = GM.ENCODER_CASES[name]
    x, proj = FU._inputs(case)
    r64, _ = FU._reference(case)
    plain = GM.ModeEncoder(case, "fp32").run(x, proj)
    same = AttnEncoder(case, "fp32", "fp32").run(x, proj)
    for k in plain:
        assert torch.equal(plain[k], same[k]), "attn = F32 is not the _mma entry point: %s" % k
    got = {}
    for pair in PAIRS:
        got[pair] = AttnEncoder(case, *pair).run(x, proj)
        assert set(got[pair]) == set(r64)
        _upper(name, pair, got[pair], _emulation(case, *pair), r64)
    emu, short = _emulation(case, "fp32", "bf16"), []
    for k in filter(_attention_fed, r64):
        moved = float((got[("fp32", "bf16")][k].double() - plain[k].double()).abs().max()) / float(r64[k].abs().max())
        em = GM._rel(emu[k], r64[k])
        print("%-14s fp32/bf16 vs fp32/fp32 on the device %-56s moved %.3e emulation error %.3e" % (name, k, moved, em))
        if moved < LOWER * em:
            short.append((k, moved, em))
    assert not short, "bf16 attention is closer to fp32 attention than its arithmetic allows: %s" % short


def test_eval_mode_in_each_pair_of_modes():
    case = FU.MODE_CASE
    x, proj = FU._inputs(case)
    r64, _ = FU._reference(case)
    for pair in PAIRS:
        got = AttnEncoder(case, *pair, train=0).run(x, proj)
        _upper("eval_s65", pair, got, _emulation(case, *pair), r64, keys=["train_y"])


def test_dropout_masks_do_not_depend_on_the_mode_and_the_modes_hold_under_them():
    case = FU.MODE_CASE
    S, Ef, F, H, NL, B = case
    p = 0.1
    x, proj = FU._inputs(case)
    nbytes = NL * (B * H * S * S + B * S * (2 * Ef + F))
    runs, masks = {}, {}
    for pair in (("fp32", "fp32"),) + PAIRS:
        enc = AttnEncoder(case, *pair, p=p, seed=4321)
        masks[pair] = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        runs[pair] = enc.run(x, proj, masks[pair])
        assert int(enc.step) == 1
    flat = masks[("fp32", "fp32")].cpu()
    assert 0.85 < float(flat.float().mean()) < 0.95
    for pair in PAIRS:
        assert torch.equal(masks[pair].cpu(), flat), "the keep masks of %s / %s differ from F32 mode's" % pair
    mk = TM.split_masks(flat, NL, B, S, Ef, F, H)
    sd = {k: v.clone() for k, v in FU._state_dict(case).items()}
    r64 = T0._torch_run(sd, x, proj, torch.float64, p, mk, nhead=H, n_layers=NL)
    for pair in PAIRS:
        emu = AC.torch_run_modes(sd, x, proj, pair[0], pair[1], torch.float32, p, mk, nhead=H, n_layers=NL)
        _upper("dropout_s65", pair, runs[pair], emu, r64)


@pytest.mark.parametrize("pair", [("bf16x3", "bf16x3"), ("bf16", "bf16")])
def test_two_clips_equal_two_single_clips_and_two_runs_agree_bit_for_bit(pair):
    """the real shape, B = 2: six query tiles of 64 per clip and head, head width 128"""
    case = (339, 512, 512, 4, 1, 2)
    x, proj = FU._inputs(case)
    enc = AttnEncoder(case, *pair)
    a, b = enc.run(x, proj), enc.run(x, proj)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between two runs" % k
    r64, _ = FU._reference(case)
    _upper("real_b2_l1", pair, a, _emulation(case, *pair), r64)
    for i in range(2):
        one = AttnEncoder(case[:5] + (1,), *pair, sd=FU._state_dict(case)).run(x[:, i:i + 1].contiguous(), proj[:, i:i + 1].contiguous())
        assert torch.equal(a["train_y"][:, i], one["train_y"][:, 0]), i
        assert torch.equal(a["train_gx"][:, i], one["train_gx"][:, 0]), i


@pytest.mark.parametrize("pair", [("bf16x3", "bf16x3"), ("fp32", "bf16")])
def test_null_gradients_are_skipped_and_a_second_backward_accumulates(pair):
    case = FU.MODE_CASE
    x, proj = FU._inputs(case)
    enc = AttnEncoder(case, *pair)
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
    """fusion.token_encoder_forward resolves the selector once: changing it between forward and backward changes nothing"""
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
        E.set_token_attn(fwd_mode)
        y = fusion.token_encoder_tokens(tf, xr)
        E.set_token_attn(bwd_mode)
        (y * gn).sum().backward()
        return [y.detach().clone(), xr.grad.clone()] + [q.grad.clone() for q in tf.parameters() if q.grad is not None]

    same, switched, plain = run("bf16", "bf16"), run("bf16", "fp32"), run("fp32", "fp32")
    assert len(same) == len(switched) == len(plain) > 10
    for a, b in zip(same, switched):
        assert torch.equal(a, b)
    assert not torch.equal(same[0], plain[0]) and not torch.equal(same[1], plain[1])
    # and the result is the C entry points' own: the same forward through AttnEncoder
    enc = AttnEncoder(case, "fp32", "bf16").run(x, proj)
    assert torch.equal(same[0].reshape(B, Ef, S).permute(2, 0, 1).cpu(), enc["train_y"])


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _both_match():
    E.configure(token_mma="match")
    E.set_token_attn("match")


def test_the_selector_reaches_the_attn_entry_points_only_when_it_is_not_fp32(monkeypatch):
    lib, seen = L.load(), []
    for n in ("vinet_token_encoder_fwd_mma", "vinet_token_encoder_fwd_attn"):
        real = getattr(lib, n)
        monkeypatch.setattr(lib, n, lambda *a, _n=n, _r=real: (seen.append((_n,) + tuple(a[1:3 if _n.endswith("attn") else 2])), _r(*a))[1])
    y_default, _, _ = FU._avfusion("fp32s")
    assert seen == [("vinet_token_encoder_fwd_mma", L.TK_MMA_F32)], seen
    del seen[:]
    _both_match()
    y_match, _, _ = FU._avfusion("fp32s")
    assert seen == [("vinet_token_encoder_fwd_attn", L.TK_MMA_BF16X3, L.TK_MMA_BF16X3)], seen
    _note("token_attn_avfusion_fp32s_match_vs_default", dict(max_abs=float((y_match - y_default).abs().max())))


def test_avfusion_map_fp32s_with_matching_token_arithmetic():
    _both_match()
    y, z, meta = FU._avfusion("fp32s")
    d = float((y.cpu().double() - torch.from_numpy(z["y"]).double()).abs().max())
    _note("token_attn_avfusion_fp32s_match", dict(max_abs=d, top2_gap=meta["top2_gap"], argmax_matches=int(y.reshape(-1).argmax()) == meta["argmax"]))
    print("avfusion fp32s + match / match: max abs", d)
    assert d <= 1e-3, d
    assert int(y.reshape(-1).argmax()) == meta["argmax"]


def test_avfusion_map_bf16_with_matching_token_arithmetic():
    _both_match()
    y, z, meta = FU._avfusion("bf16")
    ref = torch.from_numpy(z["y"]).double().reshape(-1)
    mine = y.cpu().double().reshape(-1)
    d = float((mine - ref).abs().max())
    cc = float(np.corrcoef(mine.numpy(), ref.numpy())[0, 1])
    top5 = torch.topk(ref, 5).indices.tolist()
    _note("token_attn_avfusion_bf16_match", dict(max_abs=d, cc=cc, argmax_matches=int(mine.argmax()) == meta["argmax"]))
    print("avfusion bf16 + match / match: max abs", d, "cc", cc)
    assert d <= 2.5e-2 and cc >= 0.999 and int(mine.argmax()) in top5


def test_training_step_fp32s_with_both_options_matching_moves_every_parameter_and_the_loss_falls():
    from vinet_amd import loss as VL
    from vinet_amd import optim as VO
    from vinet_amd import parallel
    _both_match()
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
    _note("token_attn_avfusion_train_fp32s_match", dict(losses=losses))
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses
