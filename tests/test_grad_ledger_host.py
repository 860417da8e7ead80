"""The engine's gradient ledger (vinet_amd/engine.py, the section below Act), exercised directly on the CPU model of the ABI:
who has written a gradient, who still will, and whether what somebody remembered about it is still true.  Counts, object identity
and launch lists only: nothing here takes a tolerance."""
import pytest
import torch

from tests.abi_emulator import AbiEmulator
from vinet_amd import _lib as L
from vinet_amd import engine as E

B, T, H, W, CC = 2, 2, 7, 10, 16
CPU = torch.device("cpu")


@pytest.fixture
def ctx():
    L._install_test_double(AbiEmulator())
    log = E.LAUNCH_LOG = []
    try:
        c = E.Ctx(CPU, E.BF16, training=True, record=True)
        c.log = log
        yield c
    finally:
        E.LAUNCH_LOG = None
        L._install_test_double(None)


def _act(pending=False, t=T, cc=CC, dt=E.BF16):
    v = E.View.alloc(B, t, H, W, cc, dt, CPU, zero=True)
    if pending:         # relu(bn(z)) waiting for its consumer
        return E.Act(v, torch.ones(cc), torch.zeros(cc), relu=True, needs_grad=True, mean=torch.zeros(cc), invstd=torch.ones(cc))
    return E.Act(v, needs_grad=True)


def _count_down(ctx, readers, writers):
    """note one reader through each of `readers`, then let `writers` write in order: the count is the same seen through every one of
    them, and it is 1 exactly inside the backward of the last"""
    for x in readers:
        E.note_reader(ctx, x)
    n = len(writers)
    assert n == len(readers)
    for i, x in enumerate(writers):
        assert {E.writers_left(y) for y in readers} == {n - i}
        assert (E.writers_left(x) == 1) == (i == n - 1)
        x.mark_grad_ready()
    assert {E.writers_left(y) for y in readers} == {0}


# ---- writers_left ------------------------------------------------------------------------------------------------------------
def test_writers_left_of_an_activation_that_owns_its_storage(ctx):
    x = _act(True)
    assert E.writers_left(x) == 0
    _count_down(ctx, [x, x, x], [x, x, x])


def test_writers_left_counts_the_readers_of_a_materialised_alias_and_of_its_source_together(ctx):
    a = _act(True)
    d = E.materialize(ctx, a)
    assert d.alias_of is a and [n for n, _, _ in ctx.log] == ["vinet_copy_affine"] and not ctx.tape
    assert E.writers_left(a) == 0, "the materialisation itself never writes"
    _count_down(ctx, [d, a, d], [d, d, a])


def test_a_neighbouring_region_or_the_whole_tensor_does_not_move_the_count_of_a_region(ctx):
    p = _act()
    r0, r1 = p.region(0, 8), p.region(8, 16)
    for x in (r0, r0, r1, p):
        E.note_reader(ctx, x)
    assert (E.writers_left(r0), E.writers_left(r1), E.writers_left(p)) == (2, 1, 1)
    r1.mark_grad_ready()
    p.mark_grad_ready()
    assert (E.writers_left(r0), E.writers_left(r1), E.writers_left(p)) == (2, 0, 0)
    r0.mark_grad_ready()
    assert E.writers_left(r0) == 1
    r0.mark_grad_ready()
    # ... and a slice of a region counts on the region
    _count_down(ctx, [r0.sub_chan(0, 4), r0], [r0.sub_chan(4, 8), r0.sub_chan(0, 4)])
    assert (E.writers_left(r1), E.writers_left(p)) == (0, 0)


def test_writers_left_of_a_concat_member_is_the_concats(ctx):
    p = _act()
    m0, m1 = p.sub_chan(0, 8), p.sub_chan(8, 16)
    _count_down(ctx, [m0, p, m1], [p, m1, m0])


@pytest.mark.parametrize("last", ["skip", "concat"])
def test_a_rehomed_skip_brings_its_earlier_readers_along(ctx, last):
    """a decoder skip re-homed into a T slice of a concat, with one reader noted before the re-homing (the conv that reads the skip
    in the encoder) and one after: both, and the concat's own consumer, count in ONE place, whoever asks"""
    skip, cat = _act(True), _act(t=2 * T)
    E.note_reader(ctx, skip)
    dst = E.materialize(ctx, skip, cat.sub_t(T, 2 * T), share_grad=True)
    assert not ctx.tape and skip.storage()[0] is cat, "not re-homed"
    assert E.writers_left(skip) == E.writers_left(cat) == E.writers_left(dst) == 1, "the materialisation itself never writes"
    E.note_reader(ctx, skip)
    E.note_reader(ctx, cat)
    for i, x in enumerate([cat, skip, skip] if last == "skip" else [skip, skip, cat]):
        assert E.writers_left(skip) == E.writers_left(cat) == E.writers_left(dst) == 3 - i
        x.mark_grad_ready()
    assert E.writers_left(skip) == E.writers_left(cat) == 0


# ---- storage() ---------------------------------------------------------------------------------------------------------------
def _same_storage(x):
    """x.storage() names the Act whose grad_view() allocated what x.grad_view() resolves into, at that channel offset"""
    owner, off = x.storage()
    assert owner.parent is None
    g, go = x.grad_view(), owner.grad_view()
    assert g.buf is go.buf and go is owner.grad_view()
    if off is not None:
        assert (g.off - go.off) % go.ld == off and g.C == x.v.C
    return owner, off


def test_storage_sums_the_channel_offsets_through_members_regions_and_the_alias(ctx):
    p = _act(True)
    assert _same_storage(p) == (p, 0)
    m = p.sub_chan(4, 16)
    r = m.region(2, 10)
    mm = r.sub_chan(1, 5)
    assert _same_storage(m) == (p, 4) and _same_storage(r) == (p, 6) and _same_storage(mm) == (p, 7)
    d = E.materialize(ctx, mm)
    assert d.alias_of is mm and _same_storage(d) == (p, 7)
    assert r.root() is r and mm.root() is r and d.root() is r and m.root() is p      # (root() answers another question)


def test_storage_has_no_channel_offset_through_a_t_slice_or_a_row_range(ctx):
    p = _act(t=2 * T)
    assert _same_storage(p.sub_t(T, 2 * T)) == (p, None)
    assert _same_storage(p.sub_t(0, T).sub_chan(8, 16)) == (p, None)
    assert _same_storage(p.sub_chan(8, 16).sub_t(0, T)) == (p, None)
    assert _same_storage(p.sub_rows(3, (1, 2, 5))) == (p, None)
    assert _same_storage(p.sub_rows(3, (1, 2, 5)).sub_chan(0, 8)) == (p, None)
    skip = _act(True)
    E.materialize(ctx, skip, p.sub_t(T, 2 * T), share_grad=True)
    assert _same_storage(skip) == (p, None) and _same_storage(skip.sub_chan(8, 16)) == (p, None)


# ---- the deferred writer -----------------------------------------------------------------------------------------------------
VIEWS = {
    "itself": lambda c, x: x,
    "sub_chan": lambda c, x: x.sub_chan(8, 16),
    "region": lambda c, x: x.region(0, 8),
    "sub_t": lambda c, x: x.sub_t(1, 2),
    "sub_rows": lambda c, x: x.sub_rows(3, (1, 2, 5)),
    "nested": lambda c, x: x.sub_chan(4, 16).region(0, 8).sub_chan(0, 4),
    "alias": lambda c, x: E.materialize(c, x),
}


def _deferred(x, acc):
    calls = []

    def launch(a):
        calls.append(a)
        x.grad_view()           # (as the pool backward does: it must find the record gone)
    rec = E._PoolRec(x, None, None, None, acc, launch)
    E._defer_pool(rec)
    return rec, calls


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("how", sorted(VIEWS))
def test_a_deferred_writer_runs_once_in_front_of_whoever_asks_for_the_gradient(ctx, how, acc):
    x = _act(how == "alias")        # (sub_rows wants a plain parent, the alias a pending one)
    asker = VIEWS[how](ctx, x)
    E.note_reader(ctx, x)
    rec, calls = _deferred(x, acc)
    assert x.is_grad_ready() and E.writers_left(x) == 0 and calls == [], "deferring counts as the write, and launches nothing"
    asker.grad_view()
    assert calls == [acc], "the accumulate flag of the moment it was deferred"
    asker.grad_view()
    x.grad_view()
    assert calls == [acc]


def test_a_deferred_writer_taken_by_its_batchnorm_backward_never_runs(ctx):
    x, inp = _act(True), _act()
    rec, calls = _deferred(x, 1)
    bn = object()
    # not this layer's: asked through another activation, no BatchNorm, a joint one, eval mode, an input without a gradient
    other = x.sub_chan(0, 8)
    no_grad = E.Act(inp.v)
    joint = E.JointBN.__new__(E.JointBN)
    for args in ((other, bn, True, inp), (x, None, True, inp), (x, joint, True, inp), (x, bn, False, inp), (x, bn, True, no_grad)):
        assert E._take_pool_rec(*args) is None
    assert calls == []
    assert E._take_pool_rec(x, bn, True, inp) is rec and E._take_pool_rec(x, bn, True, inp) is None
    x.grad_view()
    other.grad_view()
    assert calls == []


def test_a_record_left_in_place_still_runs_for_the_next_one_who_asks(ctx):
    x = _act(True)
    rec, calls = _deferred(x, 0)
    assert E._take_pool_rec(x.sub_chan(0, 8), object(), True, _act()) is None
    x.sub_chan(0, 8).grad_view()
    assert calls == [0]


# ---- stamps ------------------------------------------------------------------------------------------------------------------
def test_a_stamp_goes_invalid_with_the_next_writer_whichever_slice_it_arrives_through(ctx):
    p = _act()
    m0, m1 = p.sub_chan(0, 8), p.sub_chan(8, 16)
    m0.mark_grad_ready()
    s = E.grad_stamp(m0)
    assert E.unwritten_since(m0, s) and E.unwritten_since(p, s) and E.unwritten_since(m1, s)
    p.grad_view()
    assert E.unwritten_since(m0, s), "asking for the gradient is not writing it"
    m1.mark_grad_ready()
    assert not E.unwritten_since(m0, s) and not E.unwritten_since(p, s)
    assert E.unwritten_since(m0, E.grad_stamp(p))


def test_a_stamp_on_a_region_outlives_writers_of_its_neighbours(ctx):
    p = _act()
    r0, r1 = p.region(0, 8), p.region(8, 16)
    s = E.grad_stamp(r0)
    r1.mark_grad_ready()
    p.mark_grad_ready()
    assert E.unwritten_since(r0, s) and E.unwritten_since(r0.sub_chan(0, 4), s)
    r0.sub_chan(4, 8).mark_grad_ready()
    assert not E.unwritten_since(r0, s)


def test_partial_sums_are_found_until_a_later_writer_and_never_through_a_t_slice(ctx):
    p = _act(True)
    m = p.sub_chan(4, 16)
    ws = object()
    m.mark_grad_ready()
    E._register_bnb(ctx, m, ws, 3)
    assert E._find_bnb(ctx, m, 0, 12) == (ws, 3, 0, 12)
    assert E._find_bnb(ctx, p, 6, 4) == (ws, 3, 2, 12) and E._find_bnb(ctx, m.sub_chan(2, 6), 0, 4) == (ws, 3, 2, 12)
    assert E._find_bnb(ctx, p, 0, 8) is None, "not covered"
    p.sub_chan(0, 4).mark_grad_ready()          # a sibling slice: the same root
    assert E._find_bnb(ctx, m, 0, 12) is None
    q = _act(True, t=2 * T)
    qs = q.sub_t(0, T)
    qs.mark_grad_ready()
    E._register_bnb(ctx, qs, ws, 3)
    assert E._find_bnb(ctx, qs, 0, CC) is None and not any(v for k, v in ctx._bnb.items() if k == id(q))


def test_the_mask_of_a_gradient_holds_until_its_next_writer(ctx):
    x = _act()
    assert not E.grad_is_masked(x), "a fresh activation"
    x.mark_grad_ready()
    E.mask_grad(x)
    assert E.grad_is_masked(x)
    x.grad_view()
    assert E.grad_is_masked(x)
    x.mark_grad_ready()
    assert not E.grad_is_masked(x)


# ---- re-homing ---------------------------------------------------------------------------------------------------------------
def _refused(ctx, skip, cat):
    """the re-homing did not happen, and the copy-in-backward fallback recorded instead: it runs, and counts as a writer"""
    before = E.writers_left(skip)
    dst = E.materialize(ctx, skip, cat.sub_t(T, 2 * T), share_grad=True)
    assert skip.storage()[0] is not cat and len(ctx.tape) == 1
    assert E.writers_left(skip) == before + 1 and E.writers_left(cat) == 0
    assert [n for n, _, _ in ctx.log] == ["vinet_copy_affine"]
    E.note_reader(ctx, cat)
    cat.grad_view(zero=True)
    dst.mark_grad_ready()
    ctx.tape[0]()
    assert [n for n, _, _ in ctx.log] == ["vinet_copy_affine"] * 2 and E.writers_left(skip) == before
    assert skip.is_grad_ready() and skip.grad_view().buf is not cat.grad_view().buf


def test_an_activation_that_has_gradient_storage_is_not_rehomed(ctx):
    skip = _act(True)
    skip.grad_view()
    _refused(ctx, skip, _act(t=2 * T))


def test_a_concat_member_is_not_rehomed(ctx):
    _refused(ctx, _act(True, cc=2 * CC).sub_chan(CC, 2 * CC), _act(t=2 * T))


def test_a_skip_of_another_dtype_is_not_rehomed(ctx):
    _refused(ctx, _act(True), _act(t=2 * T, dt=E.F32))
