"""Token-wise fusion on the MI355X (csrc/token_encoder.hip): the token encoder through the C ABI at the model's shape, at every
tile edge of the attention kernels and at the descriptor's feature edges; eval mode, dropout under the exported masks, bf16 token
I/O, null gradients, accumulation, strided views; the split / mean / broadcast pair; the reference's recordings; training and
the two drivers (graph capture of this model is refused: DESIGN.md "Token-wise fusion", tests/test_fusion_host.py).

Bound of every comparison with tests/transformer_model.py in fp64, per tensor and on every element: max |gpu - ref64| <= 4 x e32,
e32 = the torch model's own fp32-vs-fp64 error on that tensor for the same inputs (measured here, never taken from the kernels),
floored at 2^-22 max |ref64|.

Tile sizes of the kernels as built (csrc/token_encoder.hip): a workgroup owns TK_BQ = 64 queries (keys in the dK / dV kernel), a
wave 16 of them; forward streams keys in tiles of TK_BK = 64, backward in tiles of TK_BB = 32; workspace rows per clip are S rounded
up to 16; weight gradients are sliced above TF_WGRAD_CHUNK = 512 (padded) rows."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import goldens as G
from tests import model_cases as MC
from tests import test_fusion_host as FH
from tests import test_gpu_transformer as T0
from tests import transformer_model as TM
from tests.gpu_report import note as _note
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import synth

pytestmark = pytest.mark.gpu
DEV = T0.DEV
GATE = 4.0
WAVE_ROWS, QUERY_TILE, KEY_TILE_FWD, TILE_BWD = 16, 64, 64, 32


@pytest.fixture(autouse=True)
def _real_library():
    assert not L.is_test_double()
    L.load()
    E.set_default_dtype("fp32")
    yield
    E.set_default_dtype("bf16")


# ---- cases: (S, E, F, H, L, B) -------------------------------------------------------------------------------------------------
REAL_B1 = (339, 512, 512, 4, 1, 1)
REAL_B2 = (339, 512, 512, 4, 2, 2)
_SEQ = sorted({1, WAVE_ROWS - 1, WAVE_ROWS, WAVE_ROWS + 1, TILE_BWD - 1, TILE_BWD, TILE_BWD + 1, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1,
               KEY_TILE_FWD - 1, KEY_TILE_FWD, KEY_TILE_FWD + 1, 2 * QUERY_TILE + 1})
SEQ_CASES = {"s%d" % s: (s, 32, 48, 2, 2, 3) for s in _SEQ}
FEATURE_CASES = {
    "e400_h5_width80_above_the_old_cap": (21, 400, 400, 5, 1, 2),
    "e512_h8_width64": (21, 512, 512, 8, 1, 2),
    "e512_h4_width128": (21, 512, 512, 4, 1, 2),
    "e16_h1_width16": (21, 16, 16, 1, 1, 2),
    "e48_h4_width12_not_a_multiple_of_8": (21, 48, 48, 4, 1, 2),
    "e32_f16_f_below_e": (21, 32, 16, 2, 1, 2),
    "e32_f1024_f_above_e": (21, 32, 1024, 2, 1, 2),
}
MODE_CASE = (65, 32, 48, 2, 2, 3)          # 65 tokens in 80 workspace rows: two query tiles, padded rows between the clips

_STATE, _INPUTS, _REFS = {}, {}, {}


def _state_dict(case):
    """parameters of `_TransformerParams` under a fixed seed, the constant vectors (biases at 0, LayerNorm at 1 / 0) perturbed by
    N(0, 0.1) and every matrix element by a factor 1 + 0.25 N(0, 1), so that a wrong bias / gamma index or a swapped layer shows"""
    S, Ef, F, H, NL, B = case
    key = (S, Ef, F, H, NL)
    if key not in _STATE:
        from vinet_amd import model as VM
        torch.manual_seed(3390 + S + Ef + F + H + NL)
        tf = VM._TransformerParams(Ef, hidden_size=F, nhead=H, num_encoder_layers=NL, max_len=S, max_head_width=VM.TOKEN_ENCODER_MAX_HEAD_WIDTH)
        sd = {k: v.clone() for k, v in tf.state_dict().items()}
        for k, v in sd.items():
            if k == "pos_encoder.pe":
                continue
            n = synth.normal("fusion_shapes|" + k, tuple(v.shape), 17)
            sd[k] = (v * (1 + 0.25 * n) if v.dim() == 2 else v + 0.1 * n).contiguous()
        _STATE[key] = sd
    return _STATE[key]


def _inputs(case, bf16=False):
    key = (case, bf16)
    if key not in _INPUTS:
        S, Ef, F, H, NL, B = case
        x = synth.normal("fusion_x_%d_%d_%d" % (S, Ef, B), (S, B, Ef), 31)
        proj = synth.normal("fusion_proj_%d_%d_%d" % (S, Ef, B), (S, B, Ef), 32)
        if bf16:
            x, proj = x.bfloat16().float(), proj.bfloat16().float()
        _INPUTS[key] = (x, proj)
    return _INPUTS[key]


def _reference(case, bf16=False, p=0.0, masks=None):
    """(fp64 run, fp32 run) of the torch model; computed once per case and shared (never modified)"""
    S, Ef, F, H, NL, B = case
    key = (case, bf16)
    if masks is None and key in _REFS:
        return _REFS[key]
    sd = {k: v.clone() for k, v in _state_dict(case).items()}
    x, proj = _inputs(case, bf16)
    r = tuple(T0._torch_run(sd, x, proj, dt, p, masks, nhead=H, n_layers=NL) for dt in (torch.float64, torch.float32))
    if masks is None:
        _REFS[key] = r
    return r


PARAM_KEYS = TM.LAYER_KEYS


class Encoder:
    """the C ABI called directly: device parameters, one descriptor, forward and backward on views the test lays out itself"""

    def __init__(self, case, sd=None, p=0.0, train=1, seed=1234, dtype=L.F32):
        S, Ef, F, H, NL, B = case
        self.case, self.dtype = case, dtype
        sd = _state_dict(case) if sd is None else sd
        self.names = ["transformer_encoder.layers.%d.%s" % (i, k) for i in range(NL) for k in PARAM_KEYS]
        self.params = [sd[n].to(DEV).float().contiguous() for n in self.names]
        self.pe = sd["pos_encoder.pe"].reshape(S, Ef).to(DEV).float().contiguous()
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
        d = self.d = L.CTokenEncoderDesc()
        d.dtype, d.B, d.S, d.E, d.H, d.F, d.L, d.train, d.p, d.eps, d.seed = dtype, B, S, Ef, H, F, NL, train, p, 1e-5, seed
        d.step, d.pe = self.step.data_ptr(), self.pe.data_ptr()
        self.parr = (C.c_void_p * len(self.params))(*[q.data_ptr() for q in self.params])
        d.params = self.parr
        self.lib = L.load()
        n = self.lib.vinet_token_encoder_workspace(C.byref(d))
        assert n > 0, self.lib.vinet_last_error()
        self.ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        d.ws, d.ws_bytes = self.ws.data_ptr(), n
        self.tdt = torch.bfloat16 if dtype == L.BF16 else torch.float32
        self.stream = torch.cuda.current_stream().cuda_stream

    def view(self, t, ld=None, sB=None, off=0):
        """CTensor over the torch buffer `t` (elements of the activation dtype): [B][S][1][1][E] at `off`, row stride ld, clip stride sB"""
        S, Ef, F, H, NL, B = self.case
        ld = Ef if ld is None else ld
        sB = S * ld if sB is None else sB
        return L.CTensor(t.data_ptr() + off * t.element_size(), B, S, 1, 1, Ef, ld, sB)

    def dense(self, tokens):
        """[S, B, E] -> device buffer [B, S, E] in the activation dtype"""
        return tokens.permute(1, 0, 2).contiguous().to(DEV).to(self.tdt)

    def forward(self, xview, yview, masks=None):
        self.d.masks = masks.data_ptr() if masks is not None else None
        rc = self.lib.vinet_token_encoder_fwd(C.byref(self.d), C.byref(xview), C.byref(yview), self.stream)
        L.check(rc, "vinet_token_encoder_fwd")

    def backward(self, dyview, dxview, grads):
        self.garr = (C.c_void_p * len(grads))(*[g.data_ptr() if g is not None else None for g in grads])
        self.d.grads, self.d.masks = self.garr, None
        rc = self.lib.vinet_token_encoder_bwd(C.byref(self.d), C.byref(dyview), C.byref(dxview) if dxview is not None else None, self.stream)
        L.check(rc, "vinet_token_encoder_bwd")

    def zero_grads(self):
        return [torch.zeros_like(q) for q in self.params]

    def run(self, x, proj, masks=None):
        """dense forward + backward on tokens [S, B, E]; tensors keyed like tests.test_gpu_transformer._torch_run"""
        xb, pb = self.dense(x), self.dense(proj)
        y, gx = torch.empty_like(xb), torch.empty_like(xb)
        self.forward(self.view(xb), self.view(y), masks)
        got = {"train_y": y.float().permute(1, 0, 2).cpu()}
        if self.d.train:
            grads = self.zero_grads()
            self.backward(self.view(pb), self.view(gx), grads)
            got["train_gx"] = gx.float().permute(1, 0, 2).cpu()
            for n, g in zip(self.names, grads):
                got["train_g:" + n] = g.cpu()
        torch.cuda.synchronize()
        return got


def _bound(r64, r32, k):
    r = r64[k]
    return max(float((r32[k].double() - r).abs().max()), 2.0 ** -22 * float(r.abs().max()))


def _check(name, got, r64, r32, keys=None, rel=0.0):
    """every tensor: |got - r64| <= rel |r64| + GATE e32 on every element; all tensors are measured and printed before the
    assertion, the worst ratio goes to the parity report"""
    worst, worst_k, bad = 0.0, None, []
    for k in (r64 if keys is None else keys):
        r = r64[k]
        mine = got[k].double().cpu()
        assert mine.shape == r.shape, (k, mine.shape, r.shape)
        assert bool(torch.isfinite(mine).all()), k
        e32 = _bound(r64, r32, k)
        err = (mine - r).abs()
        relk = rel if k in ("train_y", "train_gx") else 0.0
        allow = relk * r.abs() + GATE * e32
        ratio = GATE * float((err / allow).max()) if e32 > 0 else (0.0 if float(err.max()) == 0 else float("inf"))
        print("%-24s %-62s err %.3e torch-fp32 %.3e ratio %.2f" % (name, k, float(err.max()), e32, ratio))
        if ratio > worst:
            worst, worst_k = ratio, k
        if ratio > GATE:
            bad.append((k, float(err.max()), e32, ratio))
    _note("fusion_encoder_" + name, dict(worst_ratio_to_torch_fp32_error=worst, worst_tensor=worst_k, gate=GATE))
    assert not bad, bad
    return worst


def _case_run(name, case):
    x, proj = _inputs(case)
    got = Encoder(case).run(x, proj)
    r64, r32 = _reference(case)
    assert set(got) == set(r64)
    _check(name, got, r64, r32)
    return got


# ---- real shape ------------------------------------------------------------------------------------------------------------------

def test_real_shape_one_clip():
    """S = 339, E = 512, H = 4, F = 512, L = 1, B = 1: an odd token count, a ragged last query and key tile (339 = 5 x 64 + 19),
    heads 128 wide, a weight-gradient reduction over 352 rows of which 13 are padding"""
    _case_run("real_b1", REAL_B1)


def test_real_shape_two_clips_two_layers_equal_single_clips_bit_for_bit():
    """B = 2, L = 2: 704 workspace rows (a sliced weight gradient, slices of 512 and 192 rows) and a clip boundary inside GEMM tiles;
    output and input gradient of each clip equal that clip run alone, bit for bit; two runs agree bit for bit, gradients included"""
    case = REAL_B2
    x, proj = _inputs(case)
    enc = Encoder(case)
    a, b = enc.run(x, proj), enc.run(x, proj)
    r64, r32 = _reference(case)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between two runs" % k
    _check("real_b2_l2", a, r64, r32)
    single_case = case[:5] + (1,)
    for i in range(2):
        one = Encoder(single_case, sd=_state_dict(case)).run(x[:, i:i + 1].contiguous(), proj[:, i:i + 1].contiguous())
        assert torch.equal(a["train_y"][:, i], one["train_y"][:, 0]), i
        assert torch.equal(a["train_gx"][:, i], one["train_gx"][:, 0]), i


# ---- edges -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SEQ_CASES))
def test_sequence_edges(name):
    """E = 32, H = 2, F = 48, L = 2, B = 3 at S = 1 and one below, at and one above the wave's 16 rows, the backward tile (32), the
    query tile and the forward key tile (64), and 129 (three query tiles, the last with one row)"""
    _case_run("seq_" + name, SEQ_CASES[name])


@pytest.mark.parametrize("name", list(FEATURE_CASES))
def test_feature_edges(name):
    _case_run("feat_" + name, FEATURE_CASES[name])


# ---- modes -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [MODE_CASE, REAL_B1[:4] + (2, 1)], ids=["s65_l2_b3", "real_l2_b1"])
def test_eval_mode(case):
    """train = 0: one saved slot, every layer after the first reads its input from `out`"""
    x, proj = _inputs(case)
    got = Encoder(case, train=0).run(x, proj)
    r64, r32 = _reference(case)
    _check("eval_s%d" % case[0], got, r64, r32, keys=["train_y"])


def test_dropout_under_the_exported_masks():
    """p = 0.1: forward and every gradient equal the torch model given the kernels' own keep masks (layout [B][H][S][S] | [B S][E] |
    [B S][F] | [B S][E] per layer, although the kernels index sites 1..3 by the padded row); kept share per site within 5 binomial
    standard deviations of 0.9; the same (seed, counter) repeats the masks, the next step draws others; eval draws none"""
    case = MODE_CASE
    S, Ef, F, H, NL, B = case
    p = 0.1
    x, proj = _inputs(case)
    enc = Encoder(case, p=p, seed=4321)
    nbytes = NL * (B * H * S * S + B * S * (2 * Ef + F))
    masks = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    got = enc.run(x, proj, masks)
    assert int(enc.step) == 1
    flat = masks.cpu()
    mk = TM.split_masks(flat, NL, B, S, Ef, F, H)
    for li, ms in enumerate(mk):
        for si, m in enumerate(ms):
            n, frac = m.numel(), float(m.float().mean())
            assert set(m.unique().tolist()) <= {0, 1}
            print("layer %d site %d keeps %.5f of %d" % (li, si, frac, n))
            assert abs(frac - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, "layer %d site %d keeps %.5f of %d" % (li, si, frac, n)
    sd = {k: v.clone() for k, v in _state_dict(case).items()}
    r64, r32 = (T0._torch_run(sd, x, proj, dt, p, mk, nhead=H, n_layers=NL) for dt in (torch.float64, torch.float32))
    _check("dropout_s65", got, r64, r32)
    enc.step.zero_()
    again = torch.zeros_like(masks)
    got2 = enc.run(x, proj, again)
    assert torch.equal(again, masks)
    for k in got:
        assert torch.equal(got[k], got2[k]), k
    nxt = torch.zeros_like(masks)
    enc.run(x, proj, nxt)
    assert int(enc.step) == 2
    same, q = float((nxt.cpu() == flat).float().mean()), (1 - p) ** 2 + p ** 2
    assert abs(same - q) <= 5 * (q * (1 - q) / flat.numel()) ** 0.5, same


@pytest.mark.parametrize("case", [MODE_CASE, (21, 512, 512, 4, 1, 2)], ids=["s65_e32", "s21_e512"])
def test_bf16_token_io(case):
    """bf16 views around fp32 arithmetic.  Input and projection are bf16 values, so the only roundings are those of the output and
    the input gradient: |gpu - ref64| <= 2^-8 |ref64| + 4 e32 elementwise (the most a correct rounding to bf16's 8 significant bits
    moves a value, plus room for a value the fp32 error moves across a rounding boundary); parameter gradients keep the plain bound"""
    x, proj = _inputs(case, bf16=True)
    got = Encoder(case, dtype=L.BF16).run(x, proj)
    r64, r32 = _reference(case, bf16=True)
    assert set(got) == set(r64)
    _check("bf16_s%d_e%d" % case[:2], got, r64, r32, rel=2.0 ** -8)


def test_null_gradients_are_skipped_and_a_second_backward_accumulates():
    case = MODE_CASE
    x, proj = _inputs(case)
    enc = Encoder(case)
    full = enc.run(x, proj)
    xb, pb = enc.dense(x), enc.dense(proj)
    y, gx = torch.empty_like(xb), torch.full_like(xb, 7.0)
    enc.forward(enc.view(xb), enc.view(y))
    # dx = NULL, every third gradient NULL: the others equal the full run bit for bit, nothing else is written
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
    # a second backward into the same buffers adds: g + g, and dx is stored (not added)
    grads = enc.zero_grads()
    enc.backward(enc.view(pb), enc.view(gx), grads)
    enc.backward(enc.view(pb), enc.view(gx), grads)
    torch.cuda.synchronize()
    assert torch.equal(gx.permute(1, 0, 2).cpu(), full["train_gx"])
    for n, g in zip(enc.names, grads):
        assert torch.equal(g.cpu(), 2 * full["train_g:" + n]), n


def test_strided_input_and_channel_sub_view_output_leave_their_surroundings_alone():
    """input rows `ld = E + 16` apart in clips `sB = S ld + 48` apart; the output (and the input gradient) into channels [0, E) of a
    sentinel-filled [B][S][2E] tensor: results equal the dense run bit for bit and every sentinel survives"""
    case = (21, 32, 48, 2, 1, 2)
    S, Ef, F, H, NL, B = case
    x, proj = _inputs(case)
    enc = Encoder(case)
    full = enc.run(x, proj)
    ld, sB = Ef + 16, S * (Ef + 16) + 48
    xbuf = torch.full((B * sB,), float("nan"), device=DEV)
    xs = torch.as_strided(xbuf, (B, S, Ef), (sB, ld, 1))
    xs.copy_(enc.dense(x))
    SENT = -12345.0
    ywide = torch.full((B, S, 2 * Ef), SENT, device=DEV)
    gwide = torch.full((B, S, 2 * Ef), SENT, device=DEV)
    pwide = torch.full((B, S, 2 * Ef), float("nan"), device=DEV)
    pwide[:, :, :Ef] = enc.dense(proj)
    enc.forward(enc.view(xbuf, ld=ld, sB=sB), enc.view(ywide, ld=2 * Ef))
    grads = enc.zero_grads()
    enc.backward(enc.view(pwide, ld=2 * Ef), enc.view(gwide, ld=2 * Ef), grads)
    torch.cuda.synchronize()
    assert torch.equal(ywide[:, :, :Ef].permute(1, 0, 2).cpu(), full["train_y"])
    assert torch.equal(gwide[:, :, :Ef].permute(1, 0, 2).cpu(), full["train_gx"])
    assert bool((ywide[:, :, Ef:] == SENT).all()) and bool((gwide[:, :, Ef:] == SENT).all())
    assert bool(torch.isnan(xbuf).sum() == B * sB - B * S * Ef)
    for n, g in zip(enc.names, grads):
        assert torch.equal(g.cpu(), full["train_g:" + n]), n


def test_the_two_pointwise_convs_write_and_differentiate_through_the_token_rows():
    """fusion.token_buffer: two 1x1 convs write their row ranges of one token matrix in place and read their output gradients
    from the same rows of its gradient (dy views with a clip stride larger than their extent).  Behind them only the split /
    mean / broadcast, so torch states the whole in three lines: outputs, input gradients, weight and bias gradients against fp64
    (bound: 4 x torch's own fp32 error per tensor, floored at 2^-22 of its largest element)"""
    from vinet_amd import fusion
    from vinet_amd.model_utils import ConvParams
    B, Cin, Cout, thw, Sa = 2, 16, 32, (2, 3, 4), 3
    Sv = thw[0] * thw[1] * thw[2]

    class Pair(torch.nn.Module):
        compute_dtype = None

        def __init__(self):
            super().__init__()
            self.cv = ConvParams(Cin, Cout, kernel_size=1, stride=1, bias=True)
            self.ca = ConvParams(Cin, Cout, kernel_size=1, stride=1, bias=True)

    m = Pair()
    sd = {k: synth.normal("pair|" + k, tuple(v.shape), 51) * (0.2 if v.dim() > 1 else 1.0) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    xv = synth.normal("pair_xv", (B, Cin) + thw, 52)
    xa = synth.normal("pair_xa", (B, Cin, Sa, 1, 1), 53)
    gy = synth.normal("pair_gy", (B, 2 * Cout) + thw, 54)

    def fwd(ctx, v, a):
        tokens, (tv, ta) = fusion.token_buffer(ctx, v.v.B, [thw, (Sa, 1, 1)], Cout)
        E.conv_forward(ctx, m.cv.plan(), v, dst=tv)
        E.conv_forward(ctx, m.ca.plan(), a, dst=ta)
        return fusion.token_split_forward(ctx, tokens, Sa, thw)

    xvd, xad = xv.to(DEV).requires_grad_(True), xa.to(DEV).requires_grad_(True)
    y = E.run_root(E.BlockBody(m, fwd), [xvd, xad], list(m.parameters()))[0]
    (y * gy.to(DEV)).sum().backward()
    got = {"y": y.detach(), "gxv": xvd.grad, "gxa": xad.grad}
    got.update({"g:" + k: q.grad for k, q in m.named_parameters()})

    def ref(dt):
        P = {k: v.to(dt).requires_grad_(True) for k, v in sd.items()}
        v, a = xv.to(dt).requires_grad_(True), xa.to(dt).requires_grad_(True)
        tv = torch.nn.functional.conv3d(v, P["cv.weight"], P["cv.bias"])
        ta = torch.nn.functional.conv3d(a, P["ca.weight"], P["ca.bias"])
        out = torch.cat((tv, ta.mean(dim=(2, 3, 4), keepdim=True).expand_as(tv)), dim=1)
        (out * gy.to(dt)).sum().backward()
        r = {"y": out.detach(), "gxv": v.grad, "gxa": a.grad}
        r.update({"g:" + k: q.grad for k, q in P.items()})
        return r

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert set(got) == set(r64)
    _check("token_rows_convs", got, r64, r32)


# ---- split / mean / broadcast ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Sv, Sa, Ef", [(5, 1, 16), (336, 3, 512), (65, 3, 48)], ids=["5+1_e16", "336+3_e512", "65+3_e48"])
def test_split_mean_broadcast(Sv, Sa, Ef):
    """forward and backward against fp64 (bound: 4 x torch's own fp32 error on the tensor, floored at 2^-22 of its largest element);
    the video half is a copy, bit for bit; two runs agree bit for bit"""
    lib, B = L.load(), 2
    x = synth.normal("split_x_%d_%d" % (Sv, Ef), (B, Sv + Sa, Ef), 41)
    gy = synth.normal("split_gy_%d_%d" % (Sv, Ef), (B, Sv, 2 * Ef), 42)

    def ref(dt):
        xr = x.to(dt).requires_grad_(True)
        y = torch.cat((xr[:, :Sv], xr[:, Sv:].mean(dim=1, keepdim=True).expand(B, Sv, Ef)), dim=2)
        (y * gy.to(dt)).sum().backward()
        return {"y": y.detach(), "gx": xr.grad}

    r64, r32 = ref(torch.float64), ref(torch.float32)
    xd, gyd = x.to(DEV), gy.to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    tx = lambda t: L.CTensor(t.data_ptr(), B, Sv + Sa, 1, 1, Ef, Ef, (Sv + Sa) * Ef)
    ty = lambda t: L.CTensor(t.data_ptr(), B, Sv, 1, 1, 2 * Ef, 2 * Ef, Sv * 2 * Ef)
    runs = []
    for _ in range(2):
        y, gx = torch.full((B, Sv, 2 * Ef), float("nan"), device=DEV), torch.full((B, Sv + Sa, Ef), float("nan"), device=DEV)
        L.check(lib.vinet_token_split_fwd(C.byref(tx(xd)), L.F32, Sa, C.byref(ty(y)), stream), "vinet_token_split_fwd")
        L.check(lib.vinet_token_split_bwd(C.byref(ty(gyd)), L.F32, Sa, C.byref(tx(gx)), stream), "vinet_token_split_bwd")
        torch.cuda.synchronize()
        runs.append({"y": y.cpu(), "gx": gx.cpu()})
    for k in ("y", "gx"):
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert torch.equal(runs[0]["y"][:, :, :Ef], x[:, :Sv]) and torch.equal(runs[0]["gx"][:, :Sv], gy[:, :, :Ef])
    for k in ("y", "gx"):
        e32 = _bound(r64, r32, k)
        err = float((runs[0][k].double() - r64[k]).abs().max())
        print("split %s err %.3e torch-fp32 %.3e" % (k, err, e32))
        assert err <= GATE * e32, (k, err, e32)


# ---- the reference's recordings ----------------------------------------------------------------------------------------------------

def test_block_against_the_reference_recording_fp32():
    """fusion_block.npz: eval output, train output, input gradient and every parameter gradient on the stored samples: error against
    the reference's fp64 recording <= 4 x the reference's own fp32 error of that tensor"""
    z, meta, sd, x, proj = FH.block_inputs(torch.float32)
    case = (FH.S_TOKENS, FH.FEATURES, FH.FEATURES, FH.HEADS, FH.LAYERS, 2)
    got = Encoder(case, sd=sd).run(x, proj)
    got["eval_y"] = Encoder(case, sd=sd, train=0).run(x, proj)["train_y"]
    ratios = {}
    try:
        ratios = FH.against_block_golden(z, meta, got, lambda k: GATE * meta["fp32_err"][k])
    finally:
        if ratios:
            _note("fusion_block_fp32", dict(worst_ratio_to_reference_fp32_error=GATE * max(ratios.values()), gate=GATE,
                                            worst_tensor=max(ratios, key=ratios.get)))


def _avfusion(dtype):
    from vinet_amd import model as VM
    E.set_default_dtype(dtype)
    z, meta = G.load("avfusion32")
    m = VM.VideoAudioSaliencyFusionModel().eval()
    sd = G.state_dict_for(m, meta["seed"], z, meta)
    sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
    m.load_state_dict(sd)
    m = m.to(DEV)
    x = synth.clip(1, 32, 224, 384, meta["seed"]).to(DEV).permute(0, 2, 1, 3, 4)
    a = synth.audio(1, 70560, meta["seed"]).to(DEV)
    with torch.no_grad():
        y = m(x, a)
    return y, z, meta


@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
def test_avfusion_map(dtype):
    y, z, meta = _avfusion(dtype)
    d = float((y.cpu().double() - torch.from_numpy(z["y"]).double()).abs().max())
    _note("avfusion_" + dtype, dict(max_abs=d, top2_gap=meta["top2_gap"]))
    print("avfusion", dtype, "max abs", d)
    assert d <= 1e-3, d
    assert int(y.reshape(-1).argmax()) == meta["argmax"]


def test_avfusion_map_bf16():
    y, z, meta = _avfusion("bf16")
    ref = torch.from_numpy(z["y"]).double().reshape(-1)
    mine = y.cpu().double().reshape(-1)
    d = float((mine - ref).abs().max())
    cc = float(np.corrcoef(mine.numpy(), ref.numpy())[0, 1])
    top5 = torch.topk(ref, 5).indices.tolist()
    _note("avfusion_bf16", dict(max_abs=d, cc=cc, argmax_matches=int(mine.argmax()) == meta["argmax"]))
    print("avfusion bf16 max abs", d, "cc", cc)
    assert d <= 2.5e-2 and cc >= 0.999 and int(mine.argmax()) in top5


def test_avfusion_tokens_entering_the_encoder(monkeypatch):
    """the token matrix the two 1x1 convs write (fp32 context) against the reference's recording of the tensor entering its
    Transformer, [339, 1, 512]: a failure of the map test above is then the convs' (or the backbone's) or the encoder's.
    Bound: 1e-3 of the tensor's largest element -- the project's fp32 contract for the map (1e-3 absolute on values in [0, 1])
    restated for a tensor of another scale"""
    from vinet_amd import fusion
    box, real = {}, fusion.token_encoder_forward

    def spy(ctx, tf, tokens, *a, **k):
        box["tokens"] = tokens.v.torch5().float().clone()
        return real(ctx, tf, tokens, *a, **k)

    monkeypatch.setattr(fusion, "token_encoder_forward", spy)
    y, z, meta = _avfusion("fp32")
    ref = torch.from_numpy(z["tokens"]).double()                       # [S, B = 1, E]
    mine = box["tokens"].reshape(1, 339, 512).permute(1, 0, 2).double().cpu()
    assert mine.shape == ref.shape
    err, scale = float((mine - ref).abs().max()), float(ref.abs().max())
    print("avfusion tokens: max abs %.3e, largest element %.3e" % (err, scale))
    _note("avfusion_tokens_fp32", dict(max_abs=err, largest=scale))
    assert err <= 1e-3 * scale, (err, scale)


def test_refused_in_forward_a_clip_that_is_not_224x384():
    from vinet_amd import model as VM
    m = VM.VideoAudioSaliencyFusionModel().eval().to(DEV)
    x = synth.clip(1, 32, 128, 192, 3).to(DEV).permute(0, 2, 1, 3, 4)
    with pytest.raises(ValueError, match="224 x 384"), torch.no_grad():
        m(x, synth.audio(1, 70560, 3).to(DEV))


# ---- training and drivers ------------------------------------------------------------------------------------------------------------

def _train_setup(dtype="fp32"):
    from vinet_amd import model as VM
    E.set_default_dtype(dtype)
    m = VM.VideoAudioSaliencyFusionModel()
    sd = synth.synth_state_dict(m.state_dict(), 3)
    sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    x = synth.clip(1, 32, 224, 384, 5).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    a = synth.audio(1, 70560, 5).to(DEV)
    gt = synth.gt_map(1, 224, 384, 5).to(DEV)
    return m, x, a, gt


def test_training_step_moves_every_trainable_parameter_and_the_loss_falls():
    from vinet_amd import loss as VL
    from vinet_amd import optim as VO
    from vinet_amd import parallel
    m, x, a, gt = _train_setup()
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
            assert m.bilinear.weight.grad is None
    _note("avfusion_train_fp32", dict(losses=losses))
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses
    assert int(m.transformer.step_counter(DEV)) == 3


def test_trainer_runs_an_epoch_with_the_fusion_model(tmp_path, monkeypatch):
    """python -m vinet_amd.train --dataset synthetic --use_sound True --token_fusion True: one epoch (train, validate, save)"""
    from vinet_amd import train
    monkeypatch.chdir(tmp_path)
    train.main(["--dataset", "synthetic", "--use_sound", "True", "--token_fusion", "True", "--no_epochs", "1",
                "--synthetic_steps", "4", "--batch_size", "2", "--no_workers", "0", "--model_val_path", str(tmp_path / "tk.pt")])
    sd = torch.load(tmp_path / "tk.pt", map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    assert any(k.endswith("audio_conv_1x1.weight") for k in sd) and any(k.endswith("transformer.pos_encoder.pe") for k in sd)


def test_audio_visual_inference_with_the_fusion_model(tmp_path):
    """generate_result_audio_visual's flow with --token_fusion on a synthetic DIEM-like tree: one map per frame"""
    import wave
    from PIL import Image
    from vinet_amd import generate_result_audio_visual as AV
    E.set_default_dtype("bf16")
    args = AV.build_parser().parse_args(["--use_sound", "True", "--token_fusion", "True", "--batch", "2"])
    m = AV.build_token_fusion_model(args).eval()
    sd = synth.synth_state_dict(m.state_dict(), 5)
    sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
    m.load_state_dict(sd)
    m = m.to(DEV)
    rng = np.random.default_rng(8)
    N, h, w, fps, Fs = 63, 45, 80, 25, 22050
    root = tmp_path / "data"
    for d in ("fold_lists", "video_frames/DIEM/v1", "video_audio/DIEM/v1", "annotations/DIEM/v1/maps"):
        os.makedirs(root / d)
    (root / "fold_lists" / "DIEM_list_test_fps.txt").write_text("v1 %d %d\n" % (N, fps))
    u8 = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    for i in range(N):
        Image.fromarray(u8[i]).save(root / "video_frames" / "DIEM" / "v1" / ("%04d.png" % (i + 1)))
        Image.fromarray(u8[i, :, :, 0]).save(root / "annotations" / "DIEM" / "v1" / "maps" / ("%04d.png" % (i + 1)))
    pcm = rng.integers(-20000, 20000, int(Fs * N / fps), dtype=np.int16)
    with wave.open(str(root / "video_audio" / "DIEM" / "v1" / "v1.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(Fs); f.writeframes(pcm.tobytes())
    args.path_indata, args.save_path = str(root), str(tmp_path / "out")
    assert AV.validate(args, m, DEV) == N
    files = sorted(os.listdir(tmp_path / "out" / "v1"))
    assert len(files) == N
    img = np.asarray(Image.open(tmp_path / "out" / "v1" / files[-1]))
    assert img.shape[:2] == (h, w) and img.max() > img.min()
