"""vinet_maxpool3d_keep on a real MI355X: the cases of tests/pool_keep_cases.py on libvinet_hip.so -- y and argmax bit-identical to
vinet_maxpool3d, keep equal to vinet_copy_affine up to the sign of a zero (counted and printed, run with -s), every element of
keep written, nothing else touched, the refusals refused.  Importing tests/headline_pool_keep registers the full-shape replay of
the entry point for tests/test_gpu_headline_step.py."""
import pytest

from tests import headline_pool_keep  # noqa: F401  (registers vinet_maxpool3d_keep in headline_step.NONCONV)
from tests import pool_keep_cases as PC
from vinet_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pool", PC.SERVED, ids=[PC.POOL_NAMES[p] for p in PC.SERVED])
def test_cases_on_the_library(pool):
    side, rep = PC.LibSide(L.load(), "cuda:0"), PC.Report()
    for c in PC.SERVED_CASES:
        if c.pool == pool:
            PC.run_case(side, c, rep)
    assert rep.cases == len([c for c in PC.SERVED_CASES if c.pool == pool])
    print("%s: %d cases, %d of %d keep elements differ from vinet_copy_affine in the sign of a zero" % (
        PC.POOL_NAMES[pool], rep.cases, rep.zero_sign, rep.elements))


def test_refused_forms_launch_nothing():
    side = PC.LibSide(L.load(), "cuda:0")
    for c in PC.REFUSED_CASES:
        PC.run_case(side, c)
