"""bn_bwd_reduce_pool_kernel / bn_bwd_apply_pool_kernel (BatchNorm backward with the 1x3x3 / s(1,2,2) / p(0,1,1) max-pool backward
folded in) on a real MI355X against vinet_maxpool3d_bwd -> vinet_bn_bwd_reduce / vinet_bn_bwd_apply: gates and their derivations in
tests/bn_pool_cases.py.

Shapes: (1,1,1,1) and (1,1,2,2) -- one block, one partial; (2,3,5,7) -- odd H and W: partial blocks, windows past the edge, B > 1 for
the batch stride of a T slice; (1,2,6,4); (2,2,9,16) -- more lanes than one round of a workgroup.  C = 8, 24 (a group count that is
no power of two: R = 85 and idle lanes), 64 and 192 (the two real widths), 520 (65 groups: R = 3).  Each case runs exact and random
data, ReLU on and off, four argmax planes (the forward pool's own on random and on constant input, the maximum fan-in, blocks no
window points into) and the gradient as a dense tensor and as a T slice of a larger buffer, the apply pass in place and out of place.
The launches of the benchmarked step itself (C64 x 66 M voxels, C192 x 16.5 M accumulating into a T slice) are replayed by
tests/test_gpu_headline_step.py through tests/headline_bn_pool.py."""
import pytest

from tests import bn_pool_cases as PC
from tests import gpu_report
from tests import headline_bn_pool      # noqa: F401 (registers the full-shape replays of both entry points with the headline step's gate)
from tests.tail_cases import Side
from tests.test_gpu_kernels import _dev, _lib, _stream

pytestmark = pytest.mark.gpu

_WORST = {}


def _side():
    return Side(_lib(), _dev(), _stream())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    gpu_report.note("bn_pool_kernels", dict(
        gate="apply: bit-identical to pool backward -> bn_bwd_apply; reduce: exact data bit-equal column totals, random data error / bound of "
             "bn_cases.check_reduce (<= 1 passes)", worst_reduce_err_over_bound=dict(sorted(_WORST.items()))))


@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("Cc", PC.CS)
@pytest.mark.parametrize("dims", PC.DIMS, ids=["x".join(map(str, d)) for d in PC.DIMS])
def test_fused_against_composition(dims, Cc, acc, monkeypatch):
    _WORST["%s-c%d-acc%d" % ("x".join(map(str, dims)), Cc, acc)] = PC.check_case(_side(), monkeypatch, dims, Cc, acc)


def test_refusals():
    PC.check_refusals(_side())
