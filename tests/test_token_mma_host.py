"""The arithmetic modes of the token encoder's linear products (VINET_TK_MMA_*), everything that needs no GPU: the four entry
points exist and are bound, bad arguments are refused before anything touches a device, the engine option and the drivers' flag,
and the numpy / torch statement of the split that the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import token_mma_cases as TC
from vinet_amd import _lib as L
from vinet_amd import engine as E

NEW = ("vinet_token_encoder_workspace_mma", "vinet_token_encoder_fwd_mma", "vinet_token_encoder_bwd_mma", "vinet_token_gemm")


def _desc(**kw):
    d = L.CTokenEncoderDesc()
    d.dtype, d.B, d.S, d.E, d.H, d.F, d.L, d.train, d.p, d.eps = L.F32, 2, 339, 512, 4, 512, 3, 1, 0.1, 1e-5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_four_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = L.load()
    raw = C.CDLL(L.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
        assert n in L.SIGNATURES and getattr(lib, n).argtypes == L.SIGNATURES[n], n
    assert lib.vinet_token_encoder_workspace_mma.restype is C.c_int64
    assert lib.vinet_abi_version() == 16 == L.ABI_VERSION
    assert (L.TK_MMA_F32, L.TK_MMA_BF16X3, L.TK_MMA_BF16) == (0, 1, 2) == tuple(TC.MODES[k] for k in ("fp32", "bf16x3", "bf16"))


@pytest.mark.parametrize("kw", [dict(), dict(B=1, S=1, L=1), dict(train=0), dict(B=192), dict(E=32, H=2, F=48, S=65)])
def test_workspace_is_the_old_entry_points_in_every_mode(kw):
    lib = L.load()
    old = lib.vinet_token_encoder_workspace(C.byref(_desc(**kw)))
    assert old > 0
    for mma in (0, 1, 2):
        assert lib.vinet_token_encoder_workspace_mma(C.byref(_desc(**kw)), mma) == old


@pytest.mark.parametrize("mma", [-1, 3, 16])
def test_an_unknown_mode_is_refused_with_its_value(mma):
    lib = L.load()
    x = L.CTensor(0, 2, 339, 1, 1, 512, 512, 339 * 512)
    assert lib.vinet_token_encoder_workspace_mma(C.byref(_desc()), mma) == -1
    assert b"mma = %d" % mma in lib.vinet_last_error()
    assert lib.vinet_token_encoder_fwd_mma(C.byref(_desc()), mma, C.byref(x), C.byref(x), None) == -1
    assert b"token_encoder_fwd" in lib.vinet_last_error() and b"mma = %d" % mma in lib.vinet_last_error()
    assert lib.vinet_token_encoder_bwd_mma(C.byref(_desc()), mma, C.byref(x), C.byref(x), None) == -1
    assert b"token_encoder_bwd" in lib.vinet_last_error() and b"mma = %d" % mma in lib.vinet_last_error()
    assert lib.vinet_token_gemm(mma, 0, 0, 16, 16, 16, 16, 16, 16, 4, 4, 16, None, None, None) == -1
    assert b"token_gemm" in lib.vinet_last_error() and b"mma = %d" % mma in lib.vinet_last_error()


def _gemm(lib, mma=1, form=0, epi=0, A=64, lda=16, B=64, ldb=16, Cp=64, ldc=16, M=4, N=4, K=16, bias=None, res=None):
    return lib.vinet_token_gemm(mma, form, epi, A, lda, B, ldb, Cp, ldc, M, N, K, bias, res, None)


@pytest.mark.parametrize("kw, reason", [
    (dict(form=3), b"form = 3"), (dict(form=-1), b"form = -1"), (dict(epi=5), b"epi = 5"), (dict(epi=-2), b"epi = -2"),
    (dict(M=6), b"M = 6"), (dict(M=0), b"M = 0"), (dict(N=10), b"N = 10"), (dict(K=24), b"K = 24"), (dict(K=8), b"K = 8"),
    (dict(A=0), b"null matrix"), (dict(Cp=0), b"null matrix"),
    (dict(K=32), b"lda = 16"), (dict(form=1, N=32), b"ldb = 16"), (dict(form=2, M=32), b"lda = 16"), (dict(N=32, ldb=32), b"ldc = 16"),
    (dict(lda=18), b"16-byte aligned"), (dict(A=68), b"16-byte aligned"), (dict(B=72), b"16-byte aligned"),
    (dict(epi=1), b"epi = 1 needs bias"), (dict(epi=2), b"epi = 2 needs bias"), (dict(epi=3), b"epi = 3 needs res"),
])
def test_a_product_off_the_grid_is_refused_with_the_reason(kw, reason):
    """(the pointers are small integers no kernel may ever see: the refusal comes first, in every mode)"""
    lib = L.load()
    for mma in (0, 1, 2):
        assert _gemm(lib, mma=mma, **kw) == -1
        assert reason in lib.vinet_last_error(), lib.vinet_last_error()


def test_configure_accepts_the_four_values_refuses_a_fifth_and_restores():
    assert E._CONFIG["TOKEN_MMA"] == "fp32" and E.TOKEN_MMA == "fp32"
    for v in ("fp32", "bf16x3", "bf16", "match"):
        old = E.configure(token_mma=v)
        assert old == {"TOKEN_MMA": "fp32"} and E.TOKEN_MMA == v and E.config()["TOKEN_MMA"] == v
        E.configure(**old)
        assert E.TOKEN_MMA == "fp32"
    for bad in ("fp16", "", "BF16", 1):
        with pytest.raises(ValueError, match="token_mma"):
            E.configure(token_mma=bad)
        assert E.TOKEN_MMA == "fp32"
    old = E.configure_from_string("token_mma=match")
    assert E.TOKEN_MMA == "match"
    E.configure(**old)
    assert E.config(changed_only=True).get("TOKEN_MMA") is None


def test_match_follows_the_context_and_a_named_mode_does_not():
    try:
        E.configure(token_mma="match")
        assert [E.token_mma_mode(dt) for dt in (L.F32, L.F32S, L.BF16)] == [L.TK_MMA_F32, L.TK_MMA_BF16X3, L.TK_MMA_BF16]
        for name, want in (("fp32", L.TK_MMA_F32), ("bf16x3", L.TK_MMA_BF16X3), ("bf16", L.TK_MMA_BF16)):
            E.configure(token_mma=name)
            assert [E.token_mma_mode(dt) for dt in (L.F32, L.F32S, L.BF16)] == [want] * 3
    finally:
        E.configure(token_mma="fp32")


def test_both_drivers_default_to_fp32_and_take_the_four_values():
    from vinet_amd import generate_result_audio_visual as AV
    from vinet_amd import train
    for mod in (train, AV):
        assert mod.build_parser().parse_args([]).token_mma == "fp32"
        for v in E.TOKEN_MMA_VALUES:
            assert mod.build_parser().parse_args(["--token_mma", v]).token_mma == v
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--token_mma", "fp16"])


def test_the_split_carries_sixteen_significant_bits():
    """hi + lo == a to 16 significant bits on random fp32 data: |a - hi| <= 2^(e-8) for |a| in [2^e, 2^(e+1)), so the remainder lies
    in a binade where bf16 steps by at most 2^(e-16) and |a - hi - lo| <= 2^(e-17) <= 2^-17 |a| (a remainder of exactly 2^(e-8) is
    a bf16 value).  hi and lo are bf16 values, hi is the nearest one with ties to even, and torch's bfloat16 cast states the same split"""
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(1 << 16) * np.exp2(rng.integers(-20, 20, 1 << 16))).astype(np.float32)
    hi, lo = TC.split_np(a)
    for part in (hi, lo):
        assert not np.any(part.view(np.uint32) & 0xFFFF)
    a64, hi64, lo64 = a.astype(np.float64), hi.astype(np.float64), lo.astype(np.float64)
    assert np.all(np.abs(a64 - hi64) <= 2.0 ** -8 * np.abs(a64))          # half a unit of bf16's 8th bit
    assert np.all(np.abs(a64 - hi64 - lo64) <= 2.0 ** -17 * np.abs(a64))
    assert np.any(lo != 0)
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], dtype=np.float32)      # halfway: down to even, up to even
    assert TC.hi_np(ties).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]
    th, tl = TC.split_t(torch.from_numpy(a))
    assert np.array_equal(th.numpy(), hi) and np.array_equal(tl.numpy(), lo)


def test_the_exact_operands_meet_their_condition_for_every_case():
    """the int64 assertion of the generator (every partial sum below 2^24, in any order) on every case the GPU test runs, and the
    three expected results pairwise different in each"""
    cases = [(f, s) for f in TC.FORMS for s in TC.SHAPES] + [(2, TC.SLICED_SHAPE)]
    for form, (M, N, K) in cases:
        ops = TC.exact_operands(form, 3, M, N, K, seed=1000 * form + K + M)
        w = ops["want"]
        assert not np.array_equal(w["fp32"], w["bf16x3"]) and not np.array_equal(w["bf16x3"], w["bf16"]) and not np.array_equal(w["fp32"], w["bf16"])
        A, B = TC.logical(form, ops["A"], ops["B"])
        assert A.shape == (M, K) and B.shape == (K, N)
        for mode in TC.MODES:
            got = sum(a.astype(np.float64) @ b.astype(np.float64) for a, b in TC.terms_np(mode, A, B))
            assert np.array_equal(got, w[mode].astype(np.float64)), (form, M, N, K, mode)


def test_the_mode_model_in_fp32_mode_is_the_plain_model():
    """tests/token_mma_cases.torch_run_mode with mode fp32 equals tests/transformer_model.py's encoder (same stages, plain products)"""
    from tests import test_gpu_transformer as T0
    torch.manual_seed(7)
    S, B, Ef, F, H, NL = 5, 2, 16, 32, 2, 2
    sd = {"pos_encoder.pe": torch.randn(S, 1, Ef, dtype=torch.float64)}
    shapes = dict(zip(TC.TM.LAYER_KEYS, [(3 * Ef, Ef), (3 * Ef,), (Ef, Ef), (Ef,), (F, Ef), (F,), (Ef, F), (Ef,), (Ef,), (Ef,), (Ef,), (Ef,)]))
    for i in range(NL):
        for k, sh in shapes.items():
            sd["transformer_encoder.layers.%d.%s" % (i, k)] = torch.randn(sh, dtype=torch.float64) * 0.3
    x, proj = torch.randn(S, B, Ef, dtype=torch.float64), torch.randn(S, B, Ef, dtype=torch.float64)
    a = T0._torch_run(sd, x, proj, torch.float64, nhead=H, n_layers=NL)
    b = TC.torch_run_mode(sd, x, proj, "fp32", torch.float64, nhead=H, n_layers=NL)
    assert set(a) == set(b)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * max(1.0, float(a[k].abs().max())), k
    c = TC.torch_run_mode(sd, x, proj, "bf16", torch.float64, nhead=H, n_layers=NL)
    assert float((c["train_y"] - a["train_y"]).abs().max()) > 1e-4
