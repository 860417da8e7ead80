"""tests/tail_cases.py without a GPU: every case runs through the CPU model of the ABI (tests/abi_emulator.py) against the float64
reference, at the gate the GPU test applies to the library.  That shows each case is well posed (finite, a unique minimum, at
least one fixation per NSS sample, the gate reachable at all) and checks the model against a second, independent statement of
each operation.  The argument checks of the entry points run on the real library: they return before any launch."""
import pytest
import torch

from tests import tail_cases as TC
from tests.abi_emulator import AbiEmulator
from vinet_amd import _lib as L


def _side():
    return TC.Side(AbiEmulator())


def _ids(cases):
    return [c[0] for c in cases]


# ---- losses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TC.LOSS_SHAPES, ids=lambda s: "B%d_n%d" % s)
@pytest.mark.parametrize("g64", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=TC.LOSS_NAMES)
def test_loss_cases_are_well_posed_and_the_model_meets_the_gate(which, g64, shape):
    s, g = TC.loss_inputs(which, g64, *shape)
    assert g.dtype == (torch.float64 if g64 else torch.float32) and s.shape == g.shape == shape
    assert float(s.min()) >= 0.01 and float(s.max()) <= 0.99
    TC.loss_well_posed(which, s, g)
    assert bool(torch.isfinite(TC.loss_per_sample(which, s.double(), g.double())).all())
    if which < 3:
        assert bool(torch.isfinite(TC.loss_grad_ref(which, s, g)).all())
    TC.check_loss_fwd(_side(), which, g64, *shape)


@pytest.mark.parametrize("args", TC.LOSS_BWD_ARGS, ids=_ids(TC.LOSS_BWD_ARGS))
@pytest.mark.parametrize("shape", TC.LOSS_BWD_SHAPES, ids=lambda s: "B%d_n%d" % s)
@pytest.mark.parametrize("g64", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2], ids=TC.LOSS_NAMES[:3])
def test_loss_gradient_cases(which, g64, shape, args):
    TC.check_loss_bwd(_side(), which, g64, *shape, *args[1:])


def test_loss_tables_cover_the_edges():
    ns = [n for _, n in TC.LOSS_SHAPES]
    assert min(ns) == 2 and any(n < 64 for n in ns) and 1023 in ns and 1024 in ns and 1025 in ns and 65 in ns
    assert any(B == 1 for B, _ in TC.LOSS_SHAPES) and all(h * w == n for n, (h, w) in TC.LOSS_HW.items())
    assert all(s in TC.LOSS_SHAPES for s in TC.LOSS_BWD_SHAPES)
    bn = sorted(n for _, n in TC.LOSS_BWD_SHAPES)
    assert bn[0] < 64 < bn[1] < 1024 < bn[2]
    assert [a[1:] for a in TC.LOSS_BWD_ARGS] == [(0.7, -1.0, 0), (None, 0.25, 0), (0.7, 1.0, 1)]


# ---- Adam, fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TC.ADAM_CASES, ids=_ids(TC.ADAM_CASES))
def test_adam_cases(case):
    name, n, gs, steps, t0 = case
    p, g, m, v = TC.adam_inputs(case)
    assert p.numel() % 4 == 0 and 0 <= p.numel() - n < 4 and len(g) == steps
    assert bool((v >= 0).all()) and (t0 == 0) == (not bool(m[:n].any()))
    TC.check_adam(_side(), case)


def test_adam_reference_is_torch_adam():
    """the written-out recurrence against torch.optim.Adam in float64 (grad_scale folded into the gradient)"""
    case = ("vs_torch", 1027, 0.125, 3, 0)
    p, g, m, v = TC.adam_inputs(case)
    tp = torch.nn.Parameter(p[:1027].double().clone())
    opt = torch.optim.Adam([tp], lr=TC.f32(1e-4), betas=(0.9, 0.999), eps=TC.f32(1e-8))
    for k in range(3):
        tp.grad = g[k][:1027].double() * 0.125
        opt.step()
    # (the entry point receives beta2 as a float and forms 1 - beta2 from it: 1 - float(0.999) is 1.3e-5 below 0.001, the
    #  square root halves that, so each step of 1e-4 is 6.5e-10 off torch's; the bias corrections come from the exact betas on
    #  both sides.  Three steps: 2e-9.)
    assert float((TC.adam_ref(case)[0] - tp.detach()).abs().max()) < 4e-9


@pytest.mark.parametrize("n", TC.FILL_NS)
def test_fill_cases(n):
    TC.check_fill(_side(), n)


# ---- bilinear ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [1, 0], ids=["bias", "nobias"])
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.BIL_CASES + [("i48_j4_forward_only", TC.BIL_FWD_ONLY)], ids=_ids(TC.BIL_CASES) + ["i48_j4_forward_only"])
def test_bilinear_forward_cases(case, dt, with_bias):
    TC.check_bilinear_fwd(_side(), case[1], dt, with_bias)


@pytest.mark.parametrize("mode", TC.BIL_BWD_MODES, ids=_ids(TC.BIL_BWD_MODES))
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.BIL_CASES, ids=_ids(TC.BIL_CASES))
def test_bilinear_backward_cases(case, dt, mode):
    TC.check_bilinear_bwd(_side(), case[1], dt, mode[1])


def test_bilinear_tables_reach_their_branches():
    by = dict(TC.BIL_CASES)
    assert TC.bil_w_roundings(*by["b33_pairs"][:2])[2] == 33 and TC.bil_w_roundings(*by["c704_pairs"][:2])[2] == 33
    assert all(TC.bil_w_roundings(*s[:2])[2] <= 32 for n, s in TC.BIL_CASES if not n.endswith("_pairs"))
    assert sorted({s[3] for _, s in TC.BIL_CASES}) == [1, 2, 3, 4]
    assert any(s[1] % 64 for _, s in TC.BIL_CASES) and any(s[4] % 16 for _, s in TC.BIL_CASES) and any(s[2] < 4 for _, s in TC.BIL_CASES)
    assert all(16 * (s[2] * s[3] + 1) <= 8 * 256 for _, s in TC.BIL_CASES)          # the backward's limit
    B, Cc, I, J, O = TC.BIL_FWD_ONLY
    assert I <= 48 and J <= 4 and 16 * (I * J + 1) > 8 * 256
    # the derived bound is far below the table's gate times the largest result only through the sum of |terms|: it is not a wider gate
    for name in ("b33_pairs", "c704_pairs"):
        ref = TC.bil_ref(by[name], TC.F32)
        k = TC.bil_w_roundings(*by[name][:2])[0]
        assert float((k * TC.U32 * ref["abs_dw"]).max()) < TC.BIL_BWD_TOL[TC.F32] * float(ref["dw"].abs().max())


# ---- upsample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.UP_CASES, ids=_ids(TC.UP_CASES))
def test_upsample_cases(case, dt):
    side = _side()
    TC.check_upsample_fwd(side, case[1], dt)
    for acc in (0, 1):
        TC.check_upsample_bwd(side, case[1], dt, acc)
    TC.check_upsample_bwd_relu(side, case[1], dt)


def test_upsample_reference_clamps_at_extent_one():
    """H == 1 and W == 1: every output is the one input, the transpose is the sum of its four outputs"""
    x = torch.arange(8, dtype=torch.float64).view(1, 1, 1, 1, 8)
    assert torch.equal(TC._interp(x), x.expand(1, 1, 2, 2, 8))
    dy = torch.arange(32, dtype=torch.float64).view(1, 1, 2, 2, 8)
    assert torch.equal(TC._interp_t((1, 1, 1, 1, 8), dy), dy.sum((2, 3), keepdim=True))


# ---- act_bwd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(TC.ACT_LAYOUTS))
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("combo", TC.ACT_COMBOS, ids=lambda c: "-".join(TC.DTN[d] for d in c))
def test_act_bwd_cases(combo, act, layout):
    TC.check_act_bwd(_side(), combo, act, layout)


# ---- unfold1d ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.UNFOLD_CASES, ids=lambda c: "B%d_L%d_C%d_k%d_s%d_p%d" % c)
def test_unfold1d_cases(case, dt):
    TC.check_unfold1d(_side(), case, dt)


# ---- argument checks of the real entry points (no launch happens) ----------------------------------------------------------------
def test_entry_points_refuse_what_the_cases_say_they_refuse():
    lib = L.load()
    assert not L.is_test_double()
    TC.check_bilinear_rejects(lib, lambda t: t.clone())
    TC.check_other_rejects(lib, lambda t: t.clone())
