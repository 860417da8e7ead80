"""Every kernel of csrc/bn.hip on a real MI355X against the float64 references of tests/bn_cases.py (gates and their derivations: that
module's docstring).  tests/test_bn_cases_host.py runs the same cases through the CPU model of the ABI.

Which case reaches which kernel (case ids start with the tag; the route of each case is worked out in bn_cases.RCase / ACase and
asserted cell by cell in the host test):

  channel_reduce_small_kernel<T, MODE>     sweep at 1, 63, 64 voxels; views-v30; fwd-v30; small with reduce_small = 1; channel_sum small
  channel_reduce8_kernel<T, MODE>          sweep (C = 24), rowcap (rows == bn_rows == 1024), chan (C = 8 ... 4096: R = 256, 85, 51, 10, 2, 1
                                           and two group passes), rounds (bn_rows 2 / 3, reduce_il 0 / 1: many rounds, the last ragged),
                                           views, fwd, small with reduce_small = 0; in mode 1 with bf16 only under bn_lean = 0
  bn_bwd_reduce8_bf16_kernel<4, 4>         the same cases in mode 1 with bf16 at the default bn_lean = 1
  channel_reduce_kernel<T, MODE>           sweep and chan with C = 4, 12; rounds with C = 12; ptr8mod16, ld_c_plus4, sB4mod8,
                                           x_oct_dz_quad (each view off the 8-channel grid for one reason alone); views with C = 12;
                                           channel_sum quad.  Never launched by a kernel test before.
  bn_finalize_kernel, bn_bwd_finalize_kernel   test_finalize, test_bwd_finalize (rows 1 ... 1030, ld 0 and C + 12, NULL outputs, count = 1, a
                                           variance that rounds negative, |mean| = 1e3 std, train = 0, momentum 0 and 1), the chain
  bn_partials_fold_kernel                  test_partials_fold (chunks around the 8-deep unrolled trip, a ragged last chunk)
  bn_fold_kernel                           test_bn_fold (C = 1, 255, 256, 257, each optional pointer NULL)
  channel_sum_finalize_kernel              test_channel_sum (Cout 1, C / 4, C; store and accumulate)
  bn_bwd_apply8_kernel<T, false>           seam (1, vb - 1, vb, vb + 1, 2 vb + 4 R + 1 voxels for C = 8, 24, 200, 1024, 2048; in place and
                                           apart), views; bf16 under bn_lean = 0
  bn_bwd_apply8_bf16_kernel<4, 4>          the same cases with bf16 at the default bn_lean = 1
  bn_bwd_apply8_kernel<float, true>        the fp32 seam and views cases marked -split (dx against vinet_bn_bwd_apply's, hi / lo planes)
  bn_bwd_apply_kernel<T>                   elementwise (C = 4, 12: 255 ... 258 quads), dx_off_grid, views with C = 12.  Never launched by
                                           a kernel test before.
  (act_bwd_kernel: tests/test_gpu_tail_kernels.py.  <4, 4> is the only instantiation of the two bf16 kernels the library launches.)

NOT COVERED: the doubling of the apply kernels' voxels per block past 16 384 blocks, which needs about 1 GB of tensors.  The refused
forms (a scale without a shift, ragged group loops) are asked for their return value only, never launched."""
import pytest

from tests import bn_cases as BC
from tests import gpu_report
from tests.test_gpu_kernels import _dev, _lib, _stream

pytestmark = pytest.mark.gpu

_WORST = {}      # family -> {measure: (worst value, case)}
_RUN = {}        # kernel -> cases that reached it and passed their gates


def _side():
    return BC.Side(_lib(), _dev(), _stream())


def _note(family, case, errs, kernels=()):
    for k in kernels:
        _RUN[k] = _RUN.get(k, 0) + 1
    slot = _WORST.setdefault(family, {})
    for k, v in errs.items():
        if isinstance(v, float) and v >= slot.get(k, (-1.0, None))[0]:
            slot[k] = (v, repr(case))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    gpu_report.note("bn_kernels", dict(
        gate="reductions: exact data bit-equal, random within 1.01 (nvox + 4) u sum|term|; apply: exact data bit-equal, random within 8u "
             "|scale| (|g| + |c1| + (|x| + |mean|) |invstd c2|) (+ 2^-9 |ref| bf16); small kernels within 4u max(1, |ref|) of the float64 fold "
             "of the same partials; *_over_bound and the small kernels' figures are error / bound (<= 1 passes)",
        worst={f: {k: dict(value=v, case=c) for k, (v, c) in slot.items()} for f, slot in sorted(_WORST.items())}, cases=dict(sorted(_RUN.items()))))


@pytest.mark.parametrize("case", BC.REDUCE_CASES, ids=[c.id for c in BC.REDUCE_CASES])
def test_reduce(case):
    _note("reduce", case, BC.check_reduce(_side(), case), [case.kernel])


@pytest.mark.parametrize("case", BC.APPLY_CASES, ids=[c.id for c in BC.APPLY_CASES])
def test_apply(case):
    _note("apply", case, BC.check_apply(_side(), case), case.kernels)


@pytest.mark.parametrize("case", BC.FIN_CASES, ids=[c.id for c in BC.FIN_CASES])
def test_finalize(case):
    _note("finalize", case, BC.check_finalize(_side(), case), ["bn_finalize_kernel"])


@pytest.mark.parametrize("case", BC.BFIN_CASES, ids=[c.id for c in BC.BFIN_CASES])
def test_bwd_finalize(case):
    _note("bwd_finalize", case, BC.check_bwd_finalize(_side(), case), ["bn_bwd_finalize_kernel"])


@pytest.mark.parametrize("per,Cc,out_rows", BC.PFOLD_CASES)
def test_partials_fold(per, Cc, out_rows):
    _note("partials_fold", (per, Cc, out_rows), BC.check_partials_fold(_side(), per, Cc, out_rows), ["bn_partials_fold_kernel"])


@pytest.mark.parametrize("null", BC.BNFOLD_NULLS)
@pytest.mark.parametrize("Cc", BC.BNFOLD_CS)
def test_bn_fold(Cc, null):
    _note("bn_fold", (Cc, null), BC.check_bn_fold(_side(), Cc, null), ["bn_fold_kernel"])


@pytest.mark.parametrize("case", BC.CSUM_CASES, ids=["%s-v%d-c%d-%s-cout%d-acc%d" % ((c[0], c[1], c[2], BC.DTN[c[3]]) + c[4:]) for c in BC.CSUM_CASES])
def test_channel_sum(case):
    _note("channel_sum", case, BC.check_channel_sum(_side(), *case), ["channel_sum_finalize_kernel"])


def test_chain_against_autograd():
    """stats -> finalize -> bwd_reduce -> bwd_finalize -> apply against float64 autograd of F.batch_norm(training=True); the error of
    torch's own fp32 CPU run stands beside the library's in the parity report"""
    _note("chain", "2x3x5x7x24-f32", BC.check_chain(_side()))


def test_refusals():
    BC.check_refusals(_side())
