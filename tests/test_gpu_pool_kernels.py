"""Every instantiation of csrc/pool.hip on a real MI355X, bit for bit against the float64 window scan of tests/pool_cases.py: the
12 forward instantiations under all four pre forms (negative values, ties, exact affine arithmetic), with and without an argmax,
over +inf and NaN data; the 13 backward instantiations storing and accumulating through a forward's argmax and through random
taps; x / dx and y / dy dense, channel-sliced and T-sliced inside sentinel-filled buffers, the argmax between guards.  No gate takes
a tolerance.  tests/test_pool_cases_host.py runs the same cases through the CPU model of the ABI."""
import pytest

from tests import gpu_report
from tests import pool_cases as PC
from tests.test_gpu_kernels import _dev, _lib, _stream

pytestmark = pytest.mark.gpu

_RUN = {}      # instantiation -> cases that reached it and passed their gates


def _side():
    return PC.Side(_lib(), _dev(), _stream())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    gpu_report.note("pool_kernels", dict(gate="y, argmax and dx equal the float64 window scan bit for bit (NaNs by position); every element outside a "
                                              "view and every guard byte unchanged; y without an argmax equals y with one", cases=dict(sorted(_RUN.items()))))


@pytest.mark.parametrize("case", PC.FWD_CASES, ids=[c.id for c in PC.FWD_CASES])
def test_forward(case):
    PC.check_forward(_side(), _lib(), case)
    _RUN[case.kernel] = _RUN.get(case.kernel, 0) + 1


@pytest.mark.parametrize("case", PC.BWD_CASES, ids=[c.id for c in PC.BWD_CASES])
def test_backward(case):
    PC.check_backward(_side(), _lib(), case)
    _RUN[case.kernel] = _RUN.get(case.kernel, 0) + 1
