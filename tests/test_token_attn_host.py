"""The arithmetic modes of the token encoder's attention (include/vinet_hip.h: the `attn` argument, VINET_TK_MMA_* values), everything
that needs no GPU: the five entry points exist and are bound, bad arguments are refused before anything touches a device, the engine
selector and the drivers' flag, and the numpy / torch statement of the seven products that the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import token_attn_cases as AC
from tests import token_mma_cases as TC
from vinet_amd import _lib as L
from vinet_amd import engine as E

NEW = ("vinet_token_encoder_workspace_attn", "vinet_token_encoder_fwd_attn", "vinet_token_encoder_bwd_attn", "vinet_token_attn_fwd",
       "vinet_token_attn_bwd")


def _desc(**kw):
    d = L.CTokenEncoderDesc()
    d.dtype, d.B, d.S, d.E, d.H, d.F, d.L, d.train, d.p, d.eps = L.F32, 2, 339, 512, 4, 512, 3, 1, 0.1, 1e-5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_five_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    raw = C.CDLL(L.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in L.SIGNATURES and getattr(lib, n).argtypes == L.SIGNATURES[n], n
    assert lib.vinet_token_encoder_workspace_attn.restype is C.c_int64
    assert lib.vinet_abi_version() == 16 == L.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(), dict(B=1, S=1, L=1), dict(train=0), dict(B=192), dict(E=32, H=2, F=48, S=65)])
def test_workspace_is_the_old_entry_points_for_every_attn(kw):
    lib = L.load()
    old = lib.vinet_token_encoder_workspace(C.byref(_desc(**kw)))
    assert old > 0
    for mma in (0, 1, 2):
        for attn in (0, 1, 2):
            assert lib.vinet_token_encoder_workspace_attn(C.byref(_desc(**kw)), mma, attn) == old


@pytest.mark.parametrize("attn", [-1, 3, 16])
def test_an_unknown_attn_is_refused_with_its_value(attn):
    lib = L.load()
    x = L.CTensor(0, 2, 339, 1, 1, 512, 512, 339 * 512)
    why = b"attn = %d" % attn
    assert lib.vinet_token_encoder_workspace_attn(C.byref(_desc()), 0, attn) == -1
    assert why in lib.vinet_last_error()
    assert lib.vinet_token_encoder_fwd_attn(C.byref(_desc()), 1, attn, C.byref(x), C.byref(x), None) == -1
    assert b"token_encoder_fwd" in lib.vinet_last_error() and why in lib.vinet_last_error()
    assert lib.vinet_token_encoder_bwd_attn(C.byref(_desc()), 2, attn, C.byref(x), C.byref(x), None) == -1
    assert b"token_encoder_bwd" in lib.vinet_last_error() and why in lib.vinet_last_error()
    assert lib.vinet_token_attn_fwd(attn, 64, 1, 16, 32, 2, 64, 64, None) == -1
    assert b"token_attn_fwd" in lib.vinet_last_error() and why in lib.vinet_last_error()
    assert lib.vinet_token_attn_bwd(attn, 64, 64, 64, 64, 1, 16, 32, 2, 64, 64, None) == -1
    assert b"token_attn_bwd" in lib.vinet_last_error() and why in lib.vinet_last_error()
    # (an unknown mma is still refused by the new entry points, with its own name)
    assert lib.vinet_token_encoder_fwd_attn(C.byref(_desc()), 7, 0, C.byref(x), C.byref(x), None) == -1
    assert b"mma = 7" in lib.vinet_last_error()


def _fwd(lib, attn=1, qkv=64, B=1, S=16, E=32, H=2, P=64, ao=64):
    return lib.vinet_token_attn_fwd(attn, qkv, B, S, E, H, P, ao, None)


def _bwd(lib, attn=1, qkv=64, P=64, dao=64, ao=64, B=1, S=16, E=32, H=2, dot=64, dqkv=64):
    return lib.vinet_token_attn_bwd(attn, qkv, P, dao, ao, B, S, E, H, dot, dqkv, None)


SHAPE_REFUSALS = [
    (dict(S=0), b"S = 0"), (dict(S=1025), b"S = 1025"), (dict(B=0), b"B = 0"), (dict(H=0), b"H = 0"),
    (dict(E=24), b"E = 24"), (dict(E=528, H=8), b"E = 528"), (dict(E=48, H=5), b"E / H = 48 / 5"), (dict(E=32, H=16), b"E / H = 32 / 16"),
    (dict(E=512, H=2), b"E / H = 512 / 2"), (dict(B=4096, S=1024, E=512, H=4), b"32-bit"),
]


@pytest.mark.parametrize("kw, reason", SHAPE_REFUSALS + [
    (dict(qkv=0), b"null matrix"), (dict(P=0), b"null matrix"), (dict(ao=0), b"null matrix"),
    (dict(qkv=68), b"16-byte aligned"), (dict(ao=72), b"16-byte aligned"), (dict(P=66), b"4-byte aligned"),
])
def test_a_forward_stage_off_the_grid_is_refused_with_the_reason(kw, reason):
    """(the pointers are small integers no kernel may ever see: the refusal comes first, in every mode)"""
    lib = L.load()
    for attn in (0, 1, 2):
        assert _fwd(lib, attn=attn, **kw) == -1
        assert b"token_attn_fwd" in lib.vinet_last_error() and reason in lib.vinet_last_error(), lib.vinet_last_error()


@pytest.mark.parametrize("kw, reason", SHAPE_REFUSALS + [
    (dict(qkv=0), b"null matrix"), (dict(P=0), b"null matrix"), (dict(dao=0), b"null matrix"), (dict(ao=0), b"null matrix"),
    (dict(dot=0), b"null matrix"), (dict(dqkv=0), b"null matrix"),
    (dict(qkv=68), b"16-byte aligned"), (dict(dao=72), b"16-byte aligned"), (dict(ao=68), b"16-byte aligned"), (dict(dqkv=72), b"16-byte aligned"),
    (dict(P=66), b"4-byte aligned"), (dict(dot=65), b"4-byte aligned"),
])
def test_a_backward_stage_off_the_grid_is_refused_with_the_reason(kw, reason):
    lib = L.load()
    for attn in (0, 1, 2):
        assert _bwd(lib, attn=attn, **kw) == -1
        assert b"token_attn_bwd" in lib.vinet_last_error() and reason in lib.vinet_last_error(), lib.vinet_last_error()


def test_the_setter_accepts_the_four_values_refuses_a_fifth_and_restores():
    assert E.TOKEN_ATTN == "fp32" and E.TOKEN_ATTN_VALUES == ("fp32", "bf16x3", "bf16", "match")
    assert "TOKEN_ATTN" not in E._CONFIG and "TOKEN_ATTN" not in E.config()
    for v in E.TOKEN_ATTN_VALUES:
        old = E.set_token_attn(v)
        assert old == "fp32" and E.TOKEN_ATTN == v
        assert E.set_token_attn(old) == v and E.TOKEN_ATTN == "fp32"
    for bad in ("fp16", "", "BF16", 1, None):
        with pytest.raises(ValueError, match="fp32, bf16x3, bf16, match"):
            E.set_token_attn(bad)
        assert E.TOKEN_ATTN == "fp32"
    with pytest.raises(KeyError):
        E.configure(token_attn="bf16")


def test_match_follows_the_context_and_a_named_mode_does_not():
    try:
        E.set_token_attn("match")
        assert [E.token_attn_mode(dt) for dt in (L.F32, L.F32S, L.BF16)] == [L.TK_MMA_F32, L.TK_MMA_BF16X3, L.TK_MMA_BF16]
        for name, want in (("fp32", L.TK_MMA_F32), ("bf16x3", L.TK_MMA_BF16X3), ("bf16", L.TK_MMA_BF16)):
            E.set_token_attn(name)
            assert [E.token_attn_mode(dt) for dt in (L.F32, L.F32S, L.BF16)] == [want] * 3
        # (the two selectors are independent)
        E.set_token_attn("bf16")
        assert E.token_mma_mode(L.BF16) == L.TK_MMA_F32
    finally:
        E.set_token_attn("fp32")


def test_both_drivers_default_to_fp32_and_take_the_four_values():
    from vinet_amd import generate_result_audio_visual as AV
    from vinet_amd import train
    for mod in (train, AV):
        assert mod.build_parser().parse_args([]).token_attn == "fp32"
        for v in E.TOKEN_ATTN_VALUES:
            assert mod.build_parser().parse_args(["--token_attn", v]).token_attn == v
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--token_attn", "fp16"])


def _small_state(S, Ef, F, NL, dtype=torch.float64):
    sd = {"pos_encoder.pe": torch.randn(S, 1, Ef, dtype=dtype)}
    shapes = dict(zip(TC.TM.LAYER_KEYS, [(3 * Ef, Ef), (3 * Ef,), (Ef, Ef), (Ef,), (F, Ef), (F,), (Ef, F), (Ef,), (Ef,), (Ef,), (Ef,), (Ef,)]))
    for i in range(NL):
        for k, sh in shapes.items():
            sd["transformer_encoder.layers.%d.%s" % (i, k)] = torch.randn(sh, dtype=dtype) * 0.3
    return sd


def test_the_emulation_with_fp32_attention_is_the_linear_modes_model():
    torch.manual_seed(11)
    S, B, Ef, F, H, NL = 5, 2, 16, 32, 2, 2
    sd = _small_state(S, Ef, F, NL)
    x, proj = torch.randn(S, B, Ef, dtype=torch.float64), torch.randn(S, B, Ef, dtype=torch.float64)
    keep = [tuple((torch.rand(sh) < 0.8).to(torch.uint8) for sh in ((B, H, S, S), (B, S, Ef), (B, S, F), (B, S, Ef))) for _ in range(NL)]
    for mma in ("fp32", "bf16"):
        for p, mk in ((0.0, None), (0.2, keep)):
            a = TC.torch_run_mode(sd, x, proj, mma, torch.float64, p, mk, nhead=H, n_layers=NL)
            b = AC.torch_run_modes(sd, x, proj, mma, "fp32", torch.float64, p, mk, nhead=H, n_layers=NL)
            assert set(a) == set(b)
            for k in a:
                assert torch.equal(a[k], b[k]), (mma, p, k)


def test_the_attention_function_in_float64_without_rounding_is_autograd_of_the_plain_attention():
    """_ModeAttention's hand-written backward (the kernels' formulas, rowsum(dAO AO) included) against autograd, in a mode that
    rounds nothing: monkey-free, by calling its forward / backward pieces on float64 with mode fp32, with and without keep masks"""
    torch.manual_seed(12)
    B, H, S, D = 2, 2, 7, 4
    for keep in (None, (torch.rand(B, H, S, S) < 0.7).double() / 0.7):
        q, k, v = (torch.randn(B, H, S, D, dtype=torch.float64, requires_grad=True) for _ in range(3))
        g = torch.randn(B, H, S, D, dtype=torch.float64)
        att = torch.softmax((q * 0.5) @ k.transpose(-1, -2), dim=-1)
        ((att if keep is None else att * keep) @ v * g).sum().backward()
        want = [t.grad.clone() for t in (q, k, v)]
        q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        (AC._ModeAttention.apply(q2, k2, v2, keep, "fp32", 0.5) * g).sum().backward()
        for a, b in zip(want, (q2.grad, k2.grad, v2.grad)):
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    c = AC.torch_run_modes(_small_state(5, 16, 32, 1), torch.randn(5, 2, 16).double(), torch.randn(5, 2, 16).double(), "fp32", "bf16", torch.float64,
                           nhead=2, n_layers=1)
    assert all(bool(torch.isfinite(t).all()) for t in c.values())


def _pairwise(want, key):
    a, b, c = (np.asarray(want[m][key], np.float64) for m in ("fp32", "bf16x3", "bf16"))
    return not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c)


def test_the_exact_builders_meet_their_conditions_and_the_modes_differ_in_each_of_the_seven_products():
    """every case the GPU test runs goes through its builder's own assertions (splits as constructed, every partial sum inside fp32's
    exact integers in any order, exp of every gap exactly 0); and for each of the seven products the three modes' expected values are
    pairwise different in at least one case: scores through P, dP through dQ and dK of the one-product case"""
    seen = dict.fromkeys(("scores", "ao", "dp", "dq", "dk", "dv"), False)
    for S, D in AC.SCORES_CASES:
        w = AC.exact_scores_case(S, D, AC.case_seed(1, S, D))["want"]
        seen["scores"] |= _pairwise(w, "P")
        seen["ao"] |= _pairwise(w, "ao")
    for S, D in AC.FLAT_CASES:
        w = AC.exact_flat_case(S, D, AC.case_seed(2, S, D))["want"]
        assert not np.array_equal(w["fp32"]["ao"], w["bf16"]["ao"])
    for S, D in AC.DS_CASES:
        w = AC.exact_ds_case(S, D, AC.case_seed(3, S, D))["want"]
        for k in ("dq", "dk", "dv"):
            seen[k] |= _pairwise(w, k)
    for S, D in AC.DP_CASES:
        w = AC.exact_dp_case(S, D, AC.case_seed(4, S, D))["want"]
        seen["dp"] |= _pairwise(w, "dp") and _pairwise(w, "dk") and _pairwise(w, "dq")
    assert all(seen.values()), seen


def test_the_row_layout_helpers_round_trip():
    rng = np.random.default_rng(3)
    B, H, S, D = 2, 3, 17, 4
    x = rng.standard_normal((B, H, S, D)).astype(np.float32)
    m = AC.pack_rows(x, np.nan)
    assert m.shape == (B * 32, H * D)
    back, pad = AC.unpack_rows(m, B, H, S, D)
    assert np.array_equal(back, x) and pad.shape == (B, 15, H * D) and np.isnan(pad).all()
    assert m[32 + 5, 2 * D + 1] == x[1, 2, 5, 1]
