"""The small kernels around the network on a real MI355X, at the edges their one-shape tests in tests/test_gpu_kernels.py do not
reach: the losses below, at and just past a wave and the 1024-lane workgroup with every backward argument form, Adam's tail
loop, gradient scale and grid cap, fill's empty and capped launches, the bilinear fusion's lane / output tails, NULL outputs,
`+=` contract and repeated pair loop, the upsample's extent-one clamps, quad fall-back and sliced views, every dtype combination
and view form of vinet_act_bwd, and vinet_unfold1d's other strides, pads and windows.  Cases, float64 references and gates live in
tests/tail_cases.py; tests/test_tail_cases_host.py runs the same cases through the CPU model of the ABI."""
import pytest

from tests import gpu_report
from tests import tail_cases as TC
from tests.test_gpu_kernels import _dev, _lib, _stream

pytestmark = pytest.mark.gpu

# family -> {measured quantity: worst value over the cases run}; written beside the gates when the module is done, never asserted on
_WORST = {}
_GATES = {
    "loss": "value and per-sample slot 1e-6 * max(1, |ref|); gradient 1e-6 * max|g| + 1e-12; accumulate: 2 * 2^-24 * max(|d0| + |g|) + 1e-12",
    "adam": "p, m, v 1e-6 * max(1, max|ref|)",
    "bilinear": "forward 2e-5 / 2e-2 (fp32 / bf16), backward 5e-5 / 3e-2, x max(1, max|ref|); more than 32 pairs: k * 2^-24 * (|initial| + sum|terms|)",
    "upsample": "forward 1e-6 / 1e-2, backward 1e-5 / 2e-2, x max(1, max|ref|)",
    "act_bwd": "1e-6 / 1e-2 x max(1, max|ref|)",
}


def _side():
    return TC.Side(_lib(), _dev(), _stream())


def _ids(cases):
    return [c[0] for c in cases]


def _worst(family, tag, errs):
    w = _WORST.setdefault(family, {})
    for k, v in errs.items():
        w[tag + k] = max(w.get(tag + k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for family, w in _WORST.items():
        gpu_report.note("tail_kernels/" + family, dict(gate=_GATES[family], worst=w))


# ---- losses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TC.LOSS_SHAPES, ids=lambda s: "B%d_n%d" % s)
@pytest.mark.parametrize("g64", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=TC.LOSS_NAMES)
def test_loss_forward(which, g64, shape):
    _worst("loss", TC.LOSS_NAMES[which] + "/", TC.check_loss_fwd(_side(), which, g64, *shape))


@pytest.mark.parametrize("args", TC.LOSS_BWD_ARGS, ids=_ids(TC.LOSS_BWD_ARGS))
@pytest.mark.parametrize("shape", TC.LOSS_BWD_SHAPES, ids=lambda s: "B%d_n%d" % s)
@pytest.mark.parametrize("g64", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2], ids=TC.LOSS_NAMES[:3])
def test_loss_gradient(which, g64, shape, args):
    """gscale given / NULL, coeff -1 / 0.25 / 1, store / accumulate onto a filled buffer"""
    _worst("loss", TC.LOSS_NAMES[which] + "/", TC.check_loss_bwd(_side(), which, g64, *shape, *args[1:]))


# ---- Adam, fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TC.ADAM_CASES, ids=_ids(TC.ADAM_CASES))
def test_adam(case):
    """n below, at and past one float4, a tail of 1..3 elements behind it, grad_scale != 1, a resumed run, the capped grid"""
    _worst("adam", "", TC.check_adam(_side(), case))


@pytest.mark.parametrize("n", TC.FILL_NS)
def test_fill(n):
    TC.check_fill(_side(), n)


# ---- bilinear ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [1, 0], ids=["bias", "nobias"])
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.BIL_CASES + [("i48_j4_forward_only", TC.BIL_FWD_ONLY)], ids=_ids(TC.BIL_CASES) + ["i48_j4_forward_only"])
def test_bilinear_forward(case, dt, with_bias):
    _worst("bilinear", TC.DTN[dt] + "/", TC.check_bilinear_fwd(_side(), case[1], dt, with_bias))


@pytest.mark.parametrize("mode", TC.BIL_BWD_MODES, ids=_ids(TC.BIL_BWD_MODES))
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.BIL_CASES, ids=_ids(TC.BIL_CASES))
def test_bilinear_backward(case, dt, mode):
    """every output asked for, and each NULL form with the remaining outputs still right; dw / dbias add to non-zero buffers"""
    _worst("bilinear", TC.DTN[dt] + "/", TC.check_bilinear_bwd(_side(), case[1], dt, mode[1]))


# ---- upsample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [1, 0], ids=["up_blk1", "up_blk0"])
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.UP_CASES, ids=_ids(TC.UP_CASES))
def test_upsample(case, dt, blk):
    """forward, plain backward storing and accumulating, backward with the ReLU gate; up_blk = 1 takes the 8-channel kernels
    where C % 8 == 0 and falls back to the quad kernels by itself elsewhere, up_blk = 0 forces the quad kernels"""
    lib, side = _lib(), _side()
    assert lib.vinet_set_option(b"up_blk", blk) == 0
    try:
        errs = dict(TC.check_upsample_fwd(side, case[1], dt))
        for acc in (0, 1):
            errs["dx_acc%d" % acc] = TC.check_upsample_bwd(side, case[1], dt, acc)["dx"]
        errs["dx_relu"] = TC.check_upsample_bwd_relu(side, case[1], dt)["dx"]
    finally:
        lib.vinet_set_option(b"up_blk", 1)
    _worst("upsample", TC.DTN[dt] + "/", errs)


# ---- act_bwd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(TC.ACT_LAYOUTS))
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "sigmoid"])
@pytest.mark.parametrize("combo", TC.ACT_COMBOS, ids=lambda c: "-".join(TC.DTN[d] for d in c))
def test_act_bwd(combo, act, layout):
    _worst("act_bwd", "-".join(TC.DTN[d] for d in combo) + "/", TC.check_act_bwd(_side(), combo, act, layout))


# ---- unfold1d ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", TC.DTS, ids=TC.DTN.get)
@pytest.mark.parametrize("case", TC.UNFOLD_CASES, ids=lambda c: "B%d_L%d_C%d_k%d_s%d_p%d" % c)
def test_unfold1d(case, dt):
    TC.check_unfold1d(_side(), case, dt)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_bilinear_backward_refuses_what_the_forward_accepts():
    """I = 48, J = 4: vinet_bilinear_fwd runs it (test_bilinear_forward[i48_j4_forward_only]), vinet_bilinear_bwd answers
    "I*J too large" (its weight-gradient kernel holds at most I*J = 127): negative, vinet_last_error set, dw untouched.
    The two entry points disagree about their limits; this pins the disagreement down as it is."""
    TC.check_bilinear_rejects(_lib(), lambda t: t.clone().to(_dev()))


def test_misaligned_adam_nss_backward_and_a_sixth_act_combination_are_refused():
    TC.check_other_rejects(_lib(), lambda t: t.clone().to(_dev()))
