"""tests/pool_cases.py without a GPU: every case runs through the CPU model of the ABI (tests/abi_emulator.py) at the gates the GPU
test applies to the library, with each case's kernel names asked of the real library (the routes are host code).  The module also
asserts what the exactness of the cases rests on, that the table holds the cells it claims, and that the gates have teeth: four
wrong variants of the model must each fail at least one case."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import abi_emulator as A
from tests import pool_cases as PC
from tests import route_cases as R
from vinet_amd import _lib as L

F32, BF16, TDT = PC.F32, PC.BF16, PC.TDT


def _side(model=None):
    return PC.Side(model or A.AbiEmulator())


def _lib():
    lib = L.load()
    assert not L.is_test_double()
    return lib


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", PC.FWD_CASES, ids=_ids(PC.FWD_CASES))
def test_forward_case(case):
    PC.check_forward(_side(), _lib(), case)


@pytest.mark.parametrize("case", PC.BWD_CASES, ids=_ids(PC.BWD_CASES))
def test_backward_case(case):
    PC.check_backward(_side(), _lib(), case)


# ---- what the exactness rests on -------------------------------------------------------------------------------------------------
def _windows_with(mask, pool):
    """how many taps of each window hold a marked position"""
    count =torch.zeros((mask.shape[0],) + PC.out_dims(pool, mask.shape) + (mask.shape[4],), dtype=torch.int64)
    (kT, kH, kW) = pool[0]
    for tap in range(kT * kH * kW):
        am = torch.full(count.shape, tap, dtype=torch.uint8)
        t, h, w, inside = PC.tap_positions(pool, mask.shape, am)
        b, c = torch.arange(mask.shape[0]).view(-1, 1, 1, 1, 1), torch.arange(mask.shape[4]).view(1, 1, 1, 1, -1)
        hit = mask[b, t.clamp(0, mask.shape[1] - 1), h.clamp(0, mask.shape[2] - 1), w.clamp(0, mask.shape[3] - 1), c] & inside
        count += hit
    return count


def test_forward_data_is_exact_in_its_storage_type():
    keys = {(c.pool, c.dims, c.dt, c.pre, c.family) for c in PC.FWD_CASES}
    negative_wins = {PC.K3: 0, PC.P0: 0, PC.P1: 0}
    for pool, dims, dt, pre, family in sorted(keys, key=repr):
        x, scale, shift = PC.fwd_inputs(pool, dims, dt, pre, family)
        assert x.dtype == TDT[dt] and tuple(x.shape) == dims
        v = PC.pre64(x, scale, shift, pre.endswith("relu"))
        nan = torch.isnan(v)
        # pre(x) is representable in the storage type, and what the fp32 fma of the kernels gives is that very value
        assert torch.equal(v.to(TDT[dt]).double()[~nan], v[~nan]), (pool, dims, dt, pre)
        if scale is not None:
            assert float(v.abs().max()) <= 9 and torch.equal((v * 8).round(), v * 8)
            assert bool((x.double().abs() <= 4).all()) and torch.equal((x.double() * 4).round(), x.double() * 4)
            assert {float(s) for s in scale} <= set(PC.SCALES) and (len(scale) < 6 or {float(s) for s in scale} == set(PC.SCALES))
            assert bool((shift.abs() <= 1).all()) and torch.equal((shift * 4).round(), shift * 4)
            f = np.float32(x.float().numpy()) * scale.numpy() + shift.numpy()          # fp32, unfused: the products are exact
            assert np.array_equal(f.astype(np.float64), PC.pre64(x, scale, shift, False).numpy())
        # no -0.0 and no -inf, before and after the pre
        for t in (x.double(), v):
            assert not bool(((t == 0) & torch.signbit(t)).any()) and not bool((t == float("-inf")).any())
        if not pre.endswith("relu"):
            assert bool((v[~nan] < 0).any())
            if pool in negative_wins:
                padded = _windows_with(torch.ones(dims, dtype=torch.bool), pool) < pool[0][0] * pool[0][1] * pool[0][2]
                negative_wins[pool] += int(((PC.fwd_ref(pool, dims, dt, pre, family)[0] < 0) & padded).sum())
        if family == "nan":
            assert pre == "none" and pool in PC.NAN_GEOMETRIES
            assert bool(nan.any()) and not bool(torch.signbit(x[torch.isnan(x)].float()).any()) and bool((v == float("inf")).any())
            per_window = _windows_with(nan, pool)
            assert int(per_window.max()) == 1                                              # at most one NaN per window, and some window has one
            out = PC.fwd_ref(pool, dims, dt, pre, family)[0]
            assert torch.equal(torch.isnan(out), per_window == 1)
            # +inf beside the -inf halo (the sum test of the LDS kernel): a border window that holds one
            padded = _windows_with(torch.ones(dims, dtype=torch.bool), pool) < pool[0][0] * pool[0][1] * pool[0][2]
            assert bool(((_windows_with(v == float("inf"), pool) > 0) & padded & ~torch.isnan(out)).any())
        else:
            assert not bool(nan.any()) and bool(torch.isfinite(v).all())
    # windows that hang over an edge and hold negative values only: padding that counted as 0 (or as code 0x8000) would win them
    assert all(n >= 8 for n in negative_wins.values()), negative_wins


def test_backward_sums_are_exact_and_the_argmaxes_are_what_a_forward_produces():
    codes = {}
    for pool, dims, dt, src in sorted({(c.pool, c.dims, c.dt, c.src) for c in PC.BWD_CASES}, key=repr):
        dy, old, am = PC.bwd_inputs(pool, dims, dt, src)
        for t in (dy, old):
            assert t.dtype == TDT[dt] and bool((t.double().abs() <= 2).all()) and torch.equal(t.double().round(), t.double())
        assert tuple(am.shape) == tuple(dy.shape) and am.dtype == torch.uint8
        assert bool(PC.tap_positions(pool, dims, am)[3].all())
        ref = PC.bwd_ref(pool, dims, dt, src)
        assert float((ref.abs() + old.double().abs()).max()) <= 27 * 2 + 2
        assert torch.equal((ref + old.double()).to(TDT[dt]).double(), ref + old.double())
        assert float(ref.sum()) == float(dy.double().sum())                                  # every window routed exactly once
        if src == "rand":
            codes.setdefault(pool, set()).update(int(a) for a in am.unique())
            if pool == PC.K3 and min(dims[1:4]) >= 3:          # (stride 1: 27 windows hold each inner voxel)
                assert int(torch.bincount(_flat_targets(pool, dims, am)).max()) >= 4      # many windows route to one voxel
    for pool, seen in codes.items():
        assert seen == set(range(pool[0][0] * pool[0][1] * pool[0][2])), PC.POOL_NAMES[pool]     # every tap code occurs


def _flat_targets(pool, dims, am):
    B, T, H, W, Cc = dims
    t, h, w, _ = PC.tap_positions(pool, dims, am)
    b, c = torch.arange(B).view(-1, 1, 1, 1, 1), torch.arange(Cc).view(1, 1, 1, 1, -1)
    return ((((b * T + t) * H + h) * W + w) * Cc + c).reshape(-1)


def test_uncovered_trailing_positions_exist_and_stay_zero_in_the_reference():
    for pool in PC.NON_OVERLAPPING:
        for dims in PC.GEOMETRIES[pool]:
            covered = torch.zeros(dims, dtype=torch.bool)
            k = pool[0][0] * pool[0][1] * pool[0][2]
            odims = (dims[0],) + PC.out_dims(pool, dims) + (dims[4],)
            for tap in range(k):
                am = torch.full(odims, tap, dtype=torch.uint8)
                covered.view(-1)[_flat_targets(pool, dims, am)] = True
            assert bool((~covered).any()), PC.POOL_NAMES[pool]
            for src in ("fwd", "rand"):
                assert not bool(PC.bwd_ref(pool, dims, BF16, src)[~covered].any())


# ---- coverage claims -------------------------------------------------------------------------------------------------------------
def test_the_table_holds_the_cells_it_claims():
    ids = [c.id for c in PC.FWD_CASES + PC.BWD_CASES]
    assert len(ids) == len(set(ids))
    exact = [c for c in PC.FWD_CASES if c.family == "exact"]
    cells = {(c.kernel, c.pre) for c in exact}
    assert len(PC.FWD_INSTANTIATIONS) == 12 and cells == {(k, p) for k in PC.FWD_INSTANTIATIONS for p in PC.PRE_FORMS} and len(cells) == 48
    # a NULL-argmax twin of every cell, and every instantiation meets the NaN family
    assert {(c.kernel, c.pre) for c in exact if c.null_twin} == cells
    assert {c.kernel for c in PC.FWD_CASES if c.family == "nan"} == set(PC.FWD_INSTANTIATIONS)
    assert all(c.pre == "none" and c.pool in (PC.K3, PC.P0) for c in PC.FWD_CASES if c.family == "nan")
    bcells = {(c.kernel, c.acc, c.src) for c in PC.BWD_CASES}
    assert len(PC.BWD_INSTANTIATIONS) == 13 and bcells == {(k, a, s) for k in PC.BWD_INSTANTIATIONS for a in (0, 1) for s in ("fwd", "rand")}
    assert len({(k, a) for k, a, s in bcells}) == 26
    for k in PC.FWD_INSTANTIATIONS:
        mine = [c for c in PC.FWD_CASES if c.kernel == k]
        assert {c.xform for c in mine} == {c.yform for c in mine} == set(PC.VIEW_FORMS), k
    for k in PC.BWD_INSTANTIATIONS:
        mine = [c for c in PC.BWD_CASES if c.kernel == k]
        assert {c.xform for c in mine} == {c.yform for c in mine} == set(PC.VIEW_FORMS), k          # a channel-sliced and a T-sliced dy
    for k in PC.FWD_INSTANTIATIONS + PC.BWD_INSTANTIATIONS:          # ... with two batch items: a T slice only shows in the batch stride
        two = [c for c in PC.FWD_CASES + PC.BWD_CASES if c.kernel == k and c.dims[0] >= 2]
        assert {c.xform for c in two} == {c.yform for c in two} == set(PC.VIEW_FORMS), k
    geos = {(c.pool, c.dims) for c in PC.FWD_CASES} & {(c.pool, c.dims) for c in PC.BWD_CASES}
    for pool, dims in [(PC.K3, (1, 2, 1, 3, 8)), (PC.K3, (2, 3, 9, 10, 24)), (PC.K3, (2, 1, 9, 10, 24)), (PC.K3, (1, 4, 8, 17, 72)), (PC.K3, (1, 5, 2, 2, 8)),
                       (PC.P0, (2, 1, 1, 1, 8)), (PC.P0, (1, 2, 1, 6, 8)), (PC.P0, (1, 3, 7, 9, 24)), (PC.P0, (2, 2, 8, 10, 16)),
                       (PC.P1, (1, 1, 1, 1, 8)), (PC.P1, (1, 2, 2, 2, 8)), (PC.P1, (2, 5, 7, 9, 24)), (PC.P1, (1, 4, 8, 10, 16))]:
        assert (pool, dims) in geos
    assert any(p == PC.K3 and d[4] == 12 for p, d in geos) and any(p == PC.P0 and d[4] == 12 for p, d in geos)
    assert any(p == PC.T2 and d[1] == 5 for p, d in geos) and any(p == PC.S2 and d[2:4] == (5, 7) for p, d in geos)
    assert any(p == PC.T4 and (d[1], d[3]) == (7, 5) for p, d in geos) and any(p == PC.T8 and d[1] == 17 for p, d in geos)
    # C = 12 lies inside rows of 32 wherever it is a channel slice
    assert PC.view_geo("chan", (2, 3, 9, 10, 12), 16) == dict(ld=32, c_off=8) and PC.view_geo("chan", (2, 3, 9, 10, 24), 16) == dict(ld=40, c_off=8)
    assert PC.view_geo("tslice", (2, 3, 9, 10, 24), 8) == dict(t_total=5, t_off=1)
    assert not any("scale_only" in c.id for c in PC.FWD_CASES)


# ---- a scale without a shift -----------------------------------------------------------------------------------------------------
def test_a_scale_without_a_shift_is_rejected_by_the_name_query_and_the_model():
    lib = _lib()
    d, x, pre, y, am = R.pool_args(PC.K3, BF16, (2, 8, 9, 10), (24, 40, 8), "scale_only")
    buf = C.create_string_buffer(128)
    assert lib.vinet_maxpool3d_kernel_name(C.byref(d), C.byref(x), pre, C.byref(y), am, buf, 128) == -1
    assert b"scale needs a shift" in lib.vinet_last_error()
    for form in ("none", "relu", "affine_relu"):
        d, x, pre, y, am = R.pool_args(PC.K3, BF16, (2, 8, 9, 10), (24, 40, 8), form)
        assert lib.vinet_maxpool3d_kernel_name(C.byref(d), C.byref(x), pre, C.byref(y), am, buf, 128) == 0
    model = A.AbiEmulator()
    assert model.vinet_maxpool3d(None, None, L.CAffine(0x10000, None, 1), None, None, 0) == -1 and b"scale needs a shift" in model.vinet_last_error()


# ---- the gates have teeth --------------------------------------------------------------------------------------------------------
class WrongPool(A.AbiEmulator):
    """the model with one thing wrong in its forward.  last_tie: the last maximum of a window wins; pad_zero: padding counts as 0;
    abs_compare: the comparison is on |x|; past_view: y is written one channel past its view"""

    def __init__(self, wrong):
        super().__init__()
        self.wrong = wrong

    def vinet_maxpool3d(self, d, x, pre, y, argmax, stream):
        d_, x_, y_ = A._deref(d), A._deref(x), A._deref(y)
        if self.wrong == "past_view":
            rc = super().vinet_maxpool3d(d, x, pre, y, argmax, stream)
            raw = A._raw(y_.ptr, A._span(y_), d_.dtype)          # (the view's span: never past the buffer)
            v = A._strided(y_, d_.dtype)
            for b in range(y_.B):
                rows = v[b].reshape(-1, y_.C)
                off = b * y_.sB + np.arange(rows.shape[0]) * y_.ld + y_.C
                ok = off < raw.shape[0]
                raw[off[ok]] = rows[ok, -1]
            return rc
        xa = A.affine(A.rd(x_, d_.dtype), pre, x_.C).astype(np.float64)
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = (d_.kT, d_.kH, d_.kW), (d_.sT, d_.sH, d_.sW), (d_.pT, d_.pH, d_.pW)
        best = np.zeros((y_.B, y_.T, y_.H, y_.W, y_.C))
        arg, have = np.zeros(best.shape, np.uint8), np.zeros(best.shape, bool)
        key = np.abs if self.wrong == "abs_compare" else (lambda a: a)
        taps = [(kt, kh, kw) for kt in range(kT) for kh in range(kH) for kw in range(kW)]
        with np.errstate(invalid="ignore"):
            for tap, (kt, kh, kw) in enumerate(taps):
                t, h, w = np.arange(y_.T) * sT - pT + kt, np.arange(y_.H) * sH - pH + kh, np.arange(y_.W) * sW - pW + kw
                ok = ((t >= 0) & (t < x_.T))[:, None, None] & ((h >= 0) & (h < x_.H))[None, :, None] & ((w >= 0) & (w < x_.W))[None, None, :]
                g = xa[:, t.clip(0, x_.T - 1)][:, :, h.clip(0, x_.H - 1)][:, :, :, w.clip(0, x_.W - 1)]
                ok = np.broadcast_to(ok[None, :, :, :, None], g.shape)
                g = np.where(ok, g, 0.0)                         # a padded tap is a candidate of value 0 (pad_zero) or none at all
                valid = np.ones_like(ok) if self.wrong == "pad_zero" else ok
                better = key(g) >= key(best) if self.wrong == "last_tie" else key(g) > key(best)
                take = valid & (~have | better | (np.isnan(g) & ~np.isnan(best)))
                best, arg, have = np.where(take, g, best), np.where(take, np.uint8(tap), arg), have | take
        A.wr(y_, d_.dtype, best.astype(np.float32))
        if argmax:
            np.ctypeslib.as_array((C.c_uint8 * arg.size).from_address(argmax))[:] = arg.reshape(-1)
        return 0


@pytest.mark.parametrize("wrong", ["last_tie", "pad_zero", "abs_compare", "past_view"])
def test_a_wrong_model_fails_a_case(wrong):
    lib, failed = _lib(), []
    for case in PC.FWD_CASES:
        try:
            PC.check_forward(_side(WrongPool(wrong)), lib, case)
        except AssertionError:
            failed.append(case)
    assert failed, wrong
    if wrong == "abs_compare":                        # invisible to data that is >= 0 wherever it is compared
        assert not any(c.pre.endswith("relu") for c in failed)
    if wrong in ("pad_zero", "abs_compare"):
        assert {c.pre for c in failed} >= {"none", "affine"}
    if wrong == "past_view":
        assert {c.yform for c in failed} == set(PC.VIEW_FORMS)
