"""The transformer kernels (csrc/transformer.hip) at every GEMM tile height, weight-gradient slicing and descriptor edge that
`check_desc` accepts: output, input gradient and all twelve parameter gradients of every layer against tests/transformer_model.py
in fp64 on every element; eval mode, dropout under the exported masks, bf16 token I/O; and what the descriptor must refuse.

Bound, per tensor: max|gpu - ref64| <= 4 x e32, with e32 the torch model's own fp32-vs-fp64 error on that tensor for the same
inputs (measured here, never taken from the kernels), floored at 2^-22 max|ref64|: four fp32 half-ulps of the tensor's largest
element, nearer than which no fp32 result can be expected.

Parameters come from `_TransformerParams` under a fixed seed.  Its initialisation leaves in_proj_bias / out_proj.bias at 0, the
LayerNorm weights at 1 and biases at 0 and gives every layer the same weights, under which a wrong bias / gamma index or a
swapped layer would not show; so the constant vectors get a deterministic N(0, 0.1) added and every weight matrix a
layer-specific factor 1 + 0.25 N(0, 1) per element (`synth.normal`), which keeps the initialisation's scale."""
import ctypes as C

import pytest
import torch

from tests import test_gpu_transformer as T0
from tests import transformer_model as TM
from tests.gpu_report import note as _note
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import synth

pytestmark = pytest.mark.gpu
DEV = T0.DEV
S = 32
GATE = 4.0

# (E, F, H, L): the small shape of the tile and slicing cases (3E = 144 and F = 80 leave partial 64-column tiles), and the model's own
SMALL = (48, 80, 4, 2)
HEADLINE = (336, 336, 4, 3)

# id -> (E, F, H, L, B)
TILE_CASES = {
    "b16_512tok_last_single_launch_wgrad": SMALL + (16,),
    "b17_544tok_two_slices_last_of_32": SMALL + (17,),
    "b31_992tok_two_slices_last_of_480": SMALL + (31,),
    "b33_1056tok_three_slices_last_of_32": SMALL + (33,),
    "b128_4096tok_first_64row_tiles": SMALL + (128,),
    "b129_4128tok_back_to_32row_tiles": SMALL + (129,),
    "b130_4160tok_65_tiles_of_64rows": SMALL + (130,),
    "b256_8192tok_first_128row_tiles": SMALL + (256,),
    "b258_8256tok_back_to_64row_tiles": SMALL + (258,),
    "headline_b192_e336_6144tok_12_slices": HEADLINE + (192,),
}
EDGE_CASES = {
    "e16_f16_h4_d4": (16, 16, 4, 1, 3),
    "e16_f16_h1_d16": (16, 16, 1, 1, 3),
    "e48_f80_h4_d12_not_a_multiple_of_8": SMALL + (3,),
    "e96_f16_h1_d96_one_head_f_below_e": (96, 16, 1, 2, 3),
    "e320_f64_h4_layernorm_row_5x64": (320, 64, 4, 1, 3),
    "e336_f336_h7_d48": (336, 336, 7, 1, 3),
    "e384_f1024_h4_d96_largest_e": (384, 1024, 4, 1, 3),
    "e64_f4096_h2_b1_wgrad_4096_rows_transposed_loader": (64, 4096, 2, 1, 1),
}
EVAL_CASES = {
    "e96_f16_h1_l2_b3": EDGE_CASES["e96_f16_h1_d96_one_head_f_below_e"],
    "e48_f80_h4_l2_b130_64row_tiles": TILE_CASES["b130_4160tok_65_tiles_of_64rows"],
    "headline_b192_e336_l3": TILE_CASES["headline_b192_e336_6144tok_12_slices"],
}
DROPOUT_CASES = {"b3": SMALL + (3,), "b130_64row_tiles": SMALL + (130,)}
BF16_CASES = {"e48_f80_h4_l2_b3": SMALL + (3,), "e336_f336_h4_l1_b2": (336, 336, 4, 1, 2)}


@pytest.fixture(autouse=True)
def _real_library():
    assert not L.is_test_double()
    L.load()
    E.set_default_dtype("fp32")
    yield
    E.set_default_dtype("bf16")


_STATE, _INPUTS, _REFS = {}, {}, {}


def _state_dict(Ef, F, H, NL):
    key = (Ef, F, H, NL)
    if key not in _STATE:
        from vinet_amd import model as VM
        torch.manual_seed(20240 + Ef + F + H + NL)
        sd = {k: v.clone() for k, v in VM._TransformerParams(Ef, hidden_size=F, nhead=H, num_encoder_layers=NL, max_len=S).state_dict().items()}
        for k, v in sd.items():
            if k == "pos_encoder.pe":
                continue
            n = synth.normal("tf_shapes|" + k, tuple(v.shape), 11)
            sd[k] = (v * (1 + 0.25 * n) if v.dim() == 2 else v + 0.1 * n).contiguous()
        _STATE[key] = sd
    return _STATE[key]


def _encoder(case, p=0.0, train=True, seed=1234):
    from vinet_amd import model as VM
    Ef, F, H, NL, B = case
    tf = VM._TransformerParams(Ef, hidden_size=F, nhead=H, num_encoder_layers=NL, max_len=S)
    tf.load_state_dict(_state_dict(Ef, F, H, NL))
    tf.dropout_seed = seed
    for l in tf.transformer_encoder.layers:
        l.dropout.p = l.dropout1.p = l.dropout2.p = p
        l.self_attn.dropout = p
    return tf.to(DEV).train(train)


def _inputs(case, bf16=False):
    key = (case, bf16)
    if key not in _INPUTS:
        Ef, F, H, NL, B = case
        x = synth.normal("tf_shapes_x_%d_%d" % (Ef, B), (S, B, Ef), 21)
        proj = synth.normal("tf_shapes_proj_%d_%d" % (Ef, B), (S, B, Ef), 22)
        if bf16:
            x, proj = x.bfloat16().float(), proj.bfloat16().float()
        _INPUTS[key] = (x, proj)
    return _INPUTS[key]


def _reference(case, bf16=False, p=0.0, masks=None):
    """(fp64 run, fp32 run) of the torch model; computed once per case and shared (never modified)"""
    Ef, F, H, NL, B = case
    key = (case, bf16)
    if masks is None and key in _REFS:
        return _REFS[key]
    sd = {k: v.clone() for k, v in _state_dict(Ef, F, H, NL).items()}      # (the torch run turns its fp32 tensors into leaves)
    x, proj = _inputs(case, bf16)
    r = tuple(T0._torch_run(sd, x, proj, dt, p, masks, nhead=H, n_layers=NL) for dt in (torch.float64, torch.float32))
    if masks is None:
        _REFS[key] = r
    return r


def _run(tf, case, bf16=False, masks=None):
    x, proj = _inputs(case, bf16)
    return T0._run(tf, x, proj, masks, thw=(1, 1, case[0]))


def _bound(r64, r32, k):
    r = r64[k]
    return max(float((r32[k].double() - r).abs().max()), 2.0 ** -22 * float(r.abs().max()))


def _check(name, got, r64, r32, keys=None, rel=0.0):
    """every tensor: |got - r64| <= rel |r64| + GATE e32 on every element; all tensors are measured and printed before the
    assertion, the worst ratio of error to allowance x GATE goes to the parity report"""
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
        print("%-28s %-62s err %.3e torch-fp32 %.3e ratio %.2f" % (name, k, float(err.max()), e32, ratio))
        if ratio > worst:
            worst, worst_k = ratio, k
        if ratio > GATE:
            bad.append((k, float(err.max()), e32, ratio))
    _note("transformer_shapes_" + name, dict(worst_ratio_to_torch_fp32_error=worst, worst_tensor=worst_k, gate=GATE))
    assert not bad, bad
    return worst


@pytest.mark.parametrize("name", list(TILE_CASES))
def test_tile_heights_and_weight_gradient_slices(name):
    """fp32, p = 0: every tensor within the bound, and two runs agree bit for bit.  (B = 31 was the longest weight-gradient sum of
    one launch, 992 tokens, while slicing began at 1024 tokens: layer 0's linear1.weight gradient then stood at 4.07 x the torch
    model's fp32 error, 4.28e-5 against 1.05e-5.  Slicing now begins above 512 tokens, so B = 16 is the longest single sum.)"""
    case = TILE_CASES[name]
    tf = _encoder(case)
    a, b = _run(tf, case), _run(tf, case)
    r64, r32 = _reference(case)
    assert set(a) == set(r64)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between two runs" % k
    _check(name, a, r64, r32)


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_descriptor_edges(name):
    case = EDGE_CASES[name]
    got = _run(_encoder(case), case)
    r64, r32 = _reference(case)
    assert set(got) == set(r64)
    _check(name, got, r64, r32)


@pytest.mark.parametrize("name", list(EVAL_CASES))
def test_eval_mode(name):
    """train(False) under no_grad: one saved slot, every layer after the first reads its input from `out`"""
    from vinet_amd import fusion
    case = EVAL_CASES[name]
    tf = _encoder(case, train=False)
    x, _ = _inputs(case)
    with torch.no_grad():
        y = fusion.transformer_tokens(tf, T0._to_ncdhw(x, (1, 1, case[0])).to(DEV))
    r64, r32 = _reference(case)
    _check("eval_" + name, {"train_y": T0._to_tokens(y)}, r64, r32, keys=["train_y"])


@pytest.mark.parametrize("name", list(DROPOUT_CASES))
def test_dropout_under_the_exported_masks(name):
    """p = 0.25, E != F: forward and every gradient equal the torch model given the kernels' own keep masks (mask layout and the
    counter index m N + n with N = 48, 80, 144); kept share per site within 5 binomial standard deviations of 0.75; a second
    forward draws other masks, which agree with the first on 0.75^2 + 0.25^2 of the elements, as independent draws do (5 sigma)"""
    case = DROPOUT_CASES[name]
    Ef, F, H, NL, B = case
    p = 0.25
    tf = _encoder(case, p=p, seed=4321)
    masks = torch.zeros(tf.mask_bytes(B), dtype=torch.uint8, device=DEV)
    got = _run(tf, case, masks=masks)
    assert int(tf.step_counter(DEV)) == 1
    flat = masks.cpu()
    mk = TM.split_masks(flat, NL, B, S, Ef, F, H)
    for li, ms in enumerate(mk):
        for si, m in enumerate(ms):
            n, frac = m.numel(), float(m.float().mean())
            assert set(m.unique().tolist()) <= {0, 1}
            print("layer %d site %d keeps %.5f of %d" % (li, si, frac, n))
            assert abs(frac - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, "layer %d site %d keeps %.5f of %d" % (li, si, frac, n)
    r64, r32 = _reference(case, p=p, masks=mk)
    _check("dropout_" + name, got, r64, r32)
    nxt = torch.zeros_like(masks)
    _run(tf, case, masks=nxt)
    assert int(tf.step_counter(DEV)) == 2
    same, q = float((nxt.cpu() == flat).float().mean()), (1 - p) ** 2 + p ** 2
    print("second forward agrees on %.5f of %d" % (same, flat.numel()))
    assert abs(same - q) <= 5 * (q * (1 - q) / flat.numel()) ** 0.5, same


@pytest.mark.parametrize("name", list(BF16_CASES))
def test_bf16_token_io(name):
    """bf16 activations: tf_load_tokens<bf16> / tf_store_tokens<bf16> around fp32 arithmetic.  Input and projection are bf16 values,
    so the only roundings are those of the output and the input gradient: |gpu - ref64| <= 2^-8 |ref64| + 4 e32 elementwise
    (2^-8 |ref64|: the most a correct rounding to bf16's 8 significant bits can move a value; 4 e32: room for a value the fp32
    error moves across a rounding boundary.  Measured: 0.99 of that allowance, as a correct rounding gives);
    parameter gradients are fp32 and keep the plain bound"""
    case = BF16_CASES[name]
    E.set_default_dtype("bf16")
    got = _run(_encoder(case), case, bf16=True)
    r64, r32 = _reference(case, bf16=True)
    assert set(got) == set(r64)
    for k in ("train_y", "train_gx"):
        assert torch.equal(got[k].cpu(), got[k].cpu().bfloat16().float()), "%s is not made of bf16 values" % k
    _check("bf16_" + name, got, r64, r32, rel=2.0 ** -8)


# ---- what the descriptor must refuse: error returns before any launch ---------------------------------------------------------

def _desc(**kw):
    d = L.CTransformerDesc()
    d.dtype, d.B, d.S, d.E, d.H, d.F, d.L, d.train, d.p, d.eps, d.seed = E.F32, 3, S, 48, 4, 80, 2, 1, 0.0, 1e-5, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _workspace(**kw):
    lib = L.load()
    n = lib.vinet_transformer_workspace(C.byref(_desc(**kw)))
    return n, (lib.vinet_last_error() or b"").decode()


@pytest.mark.parametrize("fields, named", [
    (dict(E=40, H=4), "E = 40"),
    (dict(E=400, H=4), "E = 400"),
    (dict(F=40), "F = 40"),
    (dict(E=384, H=2), "E / H = 384 / 2"),
    (dict(S=16), "16 tokens per clip"),
    (dict(p=1.0), "p = 1.0"),
], ids=["e40", "e400", "f40", "e384_h2_d192", "s16", "p1"])
def test_descriptors_that_must_be_refused(fields, named):
    assert _workspace()[0] > 0
    n, msg = _workspace(**fields)
    print(n, msg)
    assert n == -1 and named in msg, (n, msg)


def test_head_width_limit_is_the_librarys():
    from vinet_amd import model as VM
    assert VM.TRANSFORMER_MAX_HEAD_WIDTH == 96
    assert _workspace(E=96, H=1)[0] > 0
    n, msg = _workspace(E=112, H=1)
    assert n == -1 and "E / H = 112 / 1" in msg and "<= 96" in msg, (n, msg)
    VM._TransformerParams(96, nhead=1, num_encoder_layers=1, max_len=S)
    with pytest.raises(NotImplementedError, match="width"):
        VM._TransformerParams(112, nhead=1, num_encoder_layers=1, max_len=S)
    with pytest.raises(NotImplementedError, match="width"):
        VM._TransformerParams(384, nhead=2)
