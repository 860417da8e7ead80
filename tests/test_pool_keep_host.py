"""tests/pool_keep_cases.py without a GPU: the case table's coverage claims, the ownership partition behind vinet_maxpool3d_keep, the
cases on the CPU model of the kernel, four wrong models that named cases must catch, and the real library's refusals (its
argument checks run on host memory, before any launch)."""
import pytest

from tests import pool_keep_cases as PC
from vinet_amd import _lib as L


def test_every_served_window_meets_every_pre_form_and_view_kind():
    for pool in PC.SERVED:
        cs = [c for c in PC.SERVED_CASES if c.pool == pool]
        assert {c.pre for c in cs} == set(PC.PRE_FORMS), pool
        assert {c.xf for c in cs} == set(PC.X_FORMS) and {c.kf for c in cs} == set(PC.KEEP_FORMS) and {c.yf for c in cs} == set(PC.Y_FORMS), pool
        assert {c.am for c in cs} == {True, False}, pool
        for pre in PC.PRE_FORMS:            # each pre form with and without an argmax, on a sliced keep
            assert {c.am for c in cs if c.pre == pre} == {True, False}, (pool, pre)
            assert any(c.kf != "dense" for c in cs if c.pre == pre), (pool, pre)
        assert {c.dims[0] for c in cs} == {1, 2} and {c.dims[4] for c in cs} == {8, 24, 40}, pool
        assert {c.dims[1] for c in cs} == ({2, 4} if pool == PC.T2 else {1, 2, 4}), pool
        assert all(c.dims[1:4] == (4, 9, 10) or max(c.dims[2:4]) <= 5 for c in cs), pool
        assert {(c.dims[2], c.dims[3]) for c in cs} >= {(h, w) for h in range(1, 6) for w in range(1, 6)}, pool
        assert any(c.odims[0] * c.odims[1] * c.odims[2] * c.odims[3] * c.odims[4] // 8 > 256 for c in cs), "more than one workgroup"
    assert len({c.id for c in PC.CASES}) == len(PC.CASES)
    assert len(PC.REFUSED_CASES) >= 3 and {"lds", "oddT", "fp32"} <= {c.why for c in PC.REFUSED_CASES}


def test_owned_taps_partition_the_input_exactly_when_the_predicate_says_so():
    """per dimension, for every extent 1 .. 9: each input index has exactly one (output, tap in [p, p + s)) iff k >= p + s and
    out * s >= in -- the two conditions of vinet_maxpool3d_keep_ok"""
    for pool in PC.SERVED + (PC.K3, PC.S2):
        for k, s, p in zip(*pool):
            for n in range(1, 10):
                cnt, out = PC.owners(n, k, s, p)
                if out < 1:
                    continue
                assert (cnt == [1] * n) == (k >= p + s and out * s >= n), (pool, k, s, p, n, cnt)
    for pool in (PC.P0, PC.P1):             # the two overlapping windows: served at every extent
        for k, s, p in zip(*pool):
            assert all(PC.owners(n, k, s, p)[0] == [1] * n for n in range(1, 10))
    assert PC.owners(3, 2, 2, 0)[0] == [1, 1, 0]            # (2,1,1)/s2 at T = 3: the last frame has no owner


@pytest.mark.parametrize("pool", PC.SERVED, ids=[PC.POOL_NAMES[p] for p in PC.SERVED])
def test_cases_on_the_model(pool):
    side, rep = PC.HostSide(PC.Model()), PC.Report()
    for c in PC.SERVED_CASES:
        if c.pool == pool:
            PC.run_case(side, c, rep)
    assert rep.cases == len([c for c in PC.SERVED_CASES if c.pool == pool])
    print("%s: %d cases, %d of %d keep elements differ from the copy in the sign of a zero" % (PC.POOL_NAMES[pool], rep.cases, rep.zero_sign, rep.elements))


def test_refusals_on_the_model_and_on_the_library():
    for c in PC.REFUSED_CASES:
        PC.run_case(PC.HostSide(PC.Model()), c)
        PC.run_case(PC.LibSide(L.load(), "cpu"), c)


def _named(pred):
    return next(c for c in PC.SERVED_CASES if pred(c))


WRONG = {
    # the wrong model -> the case that must catch it
    "owner_shift": _named(lambda c: c.pool == PC.P0 and c.dims[2] >= 3 and c.dims[3] >= 3),
    "unrounded": _named(lambda c: c.pool == PC.P1 and c.pre == "general"),
    "drop_partial": _named(lambda c: c.pool == PC.P1 and c.dims[1] == 1 and c.dims[2] == 3),
    "x_strides": _named(lambda c: c.pool == PC.T2 and c.kf == "tslice" and c.xf == "dense" and c.dims[0] == 2),
}


def test_the_named_cases():
    assert WRONG["owner_shift"].id == "ok_k133s2_B1T1H3W3C8_none_xdense_kdense_ychan_null"
    assert WRONG["unrounded"].id == "ok_k333s2_B2T1H2W1C40_general_xdense_ktslice_ydense_am"
    assert WRONG["drop_partial"].id == "ok_k333s2_B1T1H3W1C40_neg_scales_xchan_ktslice_chan_ychan_am"
    assert WRONG["x_strides"].id == "ok_k211s2_B2T2H2W1C40_general_xdense_ktslice_ydense_am"


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_a_wrong_model_fails_its_named_case(wrong):
    PC.run_case(PC.HostSide(PC.Model()), WRONG[wrong])
    with pytest.raises(AssertionError):
        PC.run_case(PC.HostSide(PC.Model(wrong)), WRONG[wrong])
