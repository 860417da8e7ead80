"""tests/bn_cases.py without a GPU: every case runs through the CPU model of the ABI (tests/abi_emulator.py) at the gates the GPU test
applies to the library.  The module also asserts what the exact cases rest on, that the tables hold the cells they claim (every
kernel of csrc/bn.hip, every edge the routes turn on), that the refusals hold in the library itself (they are host code: nothing is
launched), and that the gates have teeth: wrong variants of the model must each fail a case."""
import numpy as np
import pytest
import torch

from tests import abi_emulator as A
from tests import bn_cases as BC
from vinet_amd import _lib as L

F32, BF16 = BC.F32, BC.BF16


def _side(model=None):
    return BC.Side(model or A.AbiEmulator())


def _ids(cases):
    return [repr(c) for c in cases]


@pytest.mark.parametrize("case", BC.REDUCE_CASES, ids=_ids(BC.REDUCE_CASES))
def test_reduce_case(case):
    BC.check_reduce(_side(), case)


@pytest.mark.parametrize("case", BC.APPLY_CASES, ids=_ids(BC.APPLY_CASES))
def test_apply_case(case):
    BC.check_apply(_side(), case)


@pytest.mark.parametrize("case", BC.FIN_CASES, ids=_ids(BC.FIN_CASES))
def test_finalize_case(case):
    BC.check_finalize(_side(), case)


@pytest.mark.parametrize("case", BC.BFIN_CASES, ids=_ids(BC.BFIN_CASES))
def test_bwd_finalize_case(case):
    BC.check_bwd_finalize(_side(), case)


@pytest.mark.parametrize("per,Cc,out_rows", BC.PFOLD_CASES)
def test_partials_fold_case(per, Cc, out_rows):
    BC.check_partials_fold(_side(), per, Cc, out_rows)


@pytest.mark.parametrize("null", BC.BNFOLD_NULLS)
@pytest.mark.parametrize("Cc", BC.BNFOLD_CS)
def test_bn_fold_case(Cc, null):
    BC.check_bn_fold(_side(), Cc, null)


@pytest.mark.parametrize("case", BC.CSUM_CASES, ids=["%s-v%d-c%d-%s-cout%d-acc%d" % ((c[0], c[1], c[2], BC.DTN[c[3]]) + c[4:]) for c in BC.CSUM_CASES])
def test_channel_sum_case(case):
    BC.check_channel_sum(_side(), *case)


def test_chain_against_autograd():
    BC.check_chain(_side())


def test_refusals_of_the_model():
    BC.check_refusals(_side())


def test_refusals_of_the_library():
    """the argument checks run before any launch: the real library answers them on host memory, without a device"""
    lib = L.load()
    assert not L.is_test_double()
    BC.check_refusals(BC.Side(lib))


# ---- what the exact cases rest on ------------------------------------------------------------------------------------------------
def test_exact_reduce_data_sums_exactly_in_fp32():
    for dims, dt in sorted({(c.dims, c.dt) for c in BC.REDUCE_CASES if c.data == "exact"}):
        x, dz, mean, invstd, scale, shift = BC._reduce_data(dims, dt, "exact")
        assert x.dtype == BC.TDT[dt] and torch.equal(x.double().round(), x.double()) and float(x.double().abs().max()) <= 3
        assert torch.equal(dz.double().round(), dz.double()) and float(dz.double().abs().max()) <= 2
        assert torch.equal((mean * 2).round(), mean * 2) and set(invstd.tolist()) <= {0.5, 1.0, 2.0} and torch.equal(shift.round(), shift)
        assert set(scale.abs().tolist()) <= {0.5, 1.0, 2.0}
        nvox = dims[0] * dims[1] * dims[2] * dims[3]
        for mode, fwd in ((0, "none"), (1, "none"), (1, "affine"), (1, "relu")):
            ref, mag = BC._reduce_ref(dims, dt, "exact", mode, fwd)
            # every term a multiple of 1/4, every conceivable partial sum below 2^24 quarter units: exact in any order
            assert torch.equal((ref * 4).round(), ref * 4) and float(mag.max()) * 4 < 2 ** 24 and nvox * 16 * 4 < 2 ** 24
            if mode and fwd != "none" and nvox >= 63:
                open_ = BC.relu_gate(x.double(), fwd, scale, shift)
                assert bool(open_.any()) and not bool(open_.all())
                if fwd == "affine":      # the gate's edge itself: x * scale + shift == 0 is closed
                    assert bool((x.double() * scale.double() + shift.double() == 0).any())


def test_exact_apply_data_is_representable_and_never_zero():
    for dims, dt in sorted({(c.dims, c.dt) for c in BC.APPLY_CASES if c.data == "exact"}):
        for relu in (0, 1):
            ref, _ = BC._apply_ref(dims, dt, "exact", relu)          # (asserts representability and the absence of zeros itself)
            assert torch.equal((ref * 8).round(), ref * 8)
        p = BC._apply_data(dims, dt, "exact")[2]
        assert torch.equal((p["c1"] * 4).round() % 2, torch.ones(dims[4])) and set(p["invstd"].tolist()) <= {1.0, 2.0}


def test_the_constant_channel_rounds_to_a_negative_variance():
    part, count, _ = BC._fin_inputs(257, 64, "const")
    P = part.double()
    mean = P[:, 0, 0].sum() / count
    assert float(P[:, 1, 0].sum() / count - mean * mean) < 0
    part, count, _ = BC._fin_inputs(63, 5, "bigmean")
    P = part.double()
    mean, var = P[:, 0].sum(0) / count, P[:, 1].sum(0) / count - (P[:, 0].sum(0) / count) ** 2
    assert bool((mean.abs() > 500 * var.clamp_min(0).sqrt()).all())


# ---- coverage claims -------------------------------------------------------------------------------------------------------------
def _r(**want):
    return [c for c in BC.REDUCE_CASES if all(getattr(c, k) == v for k, v in want.items())]


def test_the_reduce_table_holds_the_cells_it_claims():
    ids = [c.id for c in BC.REDUCE_CASES]
    assert len(ids) == len(set(ids))
    # every kernel in both modes (the lean one: mode 1, bf16), both types, exact and random
    for k in BC.REDUCE_KERNELS:
        cells = {(c.mode, c.dt, c.data) for c in _r(kernel=k)}
        want = {(1, BF16, d) for d in ("exact", "rand")} if k == "bn_bwd_reduce8_bf16_kernel" else {(m, t, d) for m in (0, 1) for t in BC.DTS for d in ("exact", "rand")}
        assert cells >= want, k
        if k != "bn_bwd_reduce8_bf16_kernel":
            assert {c.dt for c in _r(kernel=k, mode=1)} == set(BC.DTS)
        assert {c.fwd for c in _r(kernel=k, mode=1)} == set(BC.FWD_FORMS), k
        assert {c.r0 for c in _r(kernel=k, mode=1)} >= {4, 12}, k
    assert {c.nvox for c in _r(tag="sweep")} == {1, 63, 64, 65, 127, 129, 4100}
    assert {c.kernel for c in _r(tag="sweep", nvox=64)} == {"channel_reduce_small_kernel"} and "channel_reduce_small_kernel" not in {c.kernel for c in _r(nvox=65)}
    assert _r(tag="rowcap", nvox=65600, C=8, opts={}) and BC.OPT_DEFAULTS["bn_rows"] == 1024 < 65600 // 64
    assert {c.C for c in _r(tag="chan", nvox=130)} == {4, 12, 8, 24, 40, 200, 1024, 2048, 4096}
    assert {c.kernel for c in _r(tag="chan") if c.C in (4, 12)} == {"channel_reduce_kernel"}
    for rows in (2, 3):
        for il in (0, 1):
            for Cc in (8, 24, 12):
                mine = [c for c in _r(tag="rounds", nvox=5000, C=Cc) if c.opts.get("bn_rows") == rows and c.opts.get("reduce_il") == il]
                assert {(c.mode, c.dt, c.data) for c in mine} == {(m, t, d) for m in (0, 1) for t in BC.DTS for d in ("exact", "rand")}
    # the last round is ragged: 2500 and 1667 voxels per block are no multiple of 4 * R for R = 256, 85 (and 4 * 85 for the quad route)
    assert all(-(-5000 // rows) % (4 * r) for rows in (2, 3) for r in (256, 85))
    # the alignment routes: each reaches the 4-channel kernel for one reason alone
    for tag in ("ptr8mod16", "ld_c_plus4", "sB4mod8", "x_oct_dz_quad"):
        assert _r(tag=tag) and {c.kernel for c in _r(tag=tag)} == {"channel_reduce_kernel"}, tag
    c = _r(tag="ptr8mod16")[0]
    x, _ = c.slabs_geo()
    assert c.dt == BF16 and (x.off * 2) % 16 == 8 and x.ld % 8 == 0 and x.sB % 8 == 0
    x, _ = _r(tag="ld_c_plus4")[0].slabs_geo()
    assert x.ld == x.dims[4] + 4 and x.off == 0
    assert all(c.slabs_geo()[0].sB % 8 == 4 for c in _r(tag="sB4mod8"))
    for c in _r(tag="x_oct_dz_quad"):
        x, g = c.slabs_geo()
        assert BC.oct_ok(x) and not BC.oct_ok(g) and BC.quad_ok(g)
    # views: all four forms on either tensor, with two batch items, on every kernel
    for k in BC.REDUCE_KERNELS:
        mine = [c for c in _r(kernel=k) if c.dims[0] == 2]
        assert {c.xform for c in mine} >= {"dense", "chan", "tslice", "both"}, k
        assert {c.gform for c in mine if c.mode} >= {"dense", "chan", "tslice", "both"}, k
    # both values of bn_lean on bf16 mode 1, of reduce_small at <= 64 voxels
    assert {c.opts.get("bn_lean", 1) for c in _r(mode=1, dt=BF16) if c.C % 8 == 0 and c.nvox > 64} == {0, 1}
    assert {(c.nvox, c.opts["reduce_small"]) for c in _r(tag="small")} == {(n, v) for n in (1, 63, 64) for v in (0, 1)}
    assert "channel_reduce_small_kernel" not in {c.kernel for c in _r(tag="small") if c.opts["reduce_small"] == 0}
    # no case is one the library refuses
    assert all(c.C // 8 <= 256 or (c.C // 8) % 256 == 0 for c in BC.REDUCE_CASES)


def _a(**want):
    return [c for c in BC.APPLY_CASES if all(getattr(c, k) == v for k, v in want.items())]


def test_the_apply_table_holds_the_cells_it_claims():
    ids = [c.id for c in BC.APPLY_CASES]
    assert len(ids) == len(set(ids))
    reached = {k for c in BC.APPLY_CASES for k in c.kernels}
    assert reached == set(BC.APPLY_KERNELS)
    for Cc in (8, 24, 200, 1024, 2048):
        vb = BC.apply_vb(Cc)
        want = {1, vb - 1, vb, vb + 1, 2 * vb + vb // 4 + 1}
        assert {c.nvox for c in _a(tag="seam", C=Cc, dxform="inplace")} == want
        for k in ("bn_bwd_apply8_kernel", "bn_bwd_apply8_bf16_kernel", "bn_bwd_apply8_kernel<split>"):
            assert {c.nvox for c in _a(tag="seam", C=Cc) if k in c.kernels} >= want, (Cc, k)
        assert {c.dt for c in _a(tag="seam", C=Cc) if "bn_bwd_apply8_kernel" in c.kernels} == {F32, BF16}
    assert (BC.apply_vb(8), BC.apply_vb(24), BC.apply_vb(200), BC.apply_vb(1024), BC.apply_vb(2048)) == (4096, 1360, 160, 32, 16)
    ew = [c for c in BC.APPLY_CASES if c.kernels == ["bn_bwd_apply_kernel"]]
    assert {c.nvox * c.C // 4 for c in ew} >= {254, 255, 256, 257, 258}
    assert {c.dt for c in ew} == {F32, BF16} and {c.C for c in ew} == {4, 8, 12}
    for c in _a(tag="dx_off_grid"):          # dz and x on the 8-channel grid, dx alone off it
        slabs = [BC.Slab(c.dims, c.dt, fill=0.0, **c.geo(w)) for w in ("dz", "x", "dx")]
        assert BC.oct_ok(slabs[0]) and BC.oct_ok(slabs[1]) and not BC.oct_ok(slabs[2]) and BC.quad_ok(slabs[2])
    for k in BC.APPLY_KERNELS:
        mine = [c for c in BC.APPLY_CASES if k in c.kernels]
        assert {c.relu for c in mine} == {0, 1} and {c.data for c in mine} == {"exact", "rand"}, k
        assert {c.r0 for c in mine} == {0, 4, 12}, k
        assert "inplace" in {c.dxform for c in mine}, k
        two = {c.dxform for c in mine if c.dims[0] == 2}
        assert two >= {"inplace", "chan", "tslice", "both"}, (k, two)
        assert {c.inform for c in mine if c.dims[0] == 2} >= {"dense", "chan", "tslice", "both"}, k


def test_the_small_tables_hold_the_cells_they_claim():
    assert {c.rows for c in BC.FIN_CASES} == {1, 63, 255, 256, 257, 1030} and {c.C for c in BC.FIN_CASES} == {1, 5, 64}
    assert {c.ld for c in BC.FIN_CASES if c.C == 5} == {0, 17}
    assert {c.flavour for c in BC.FIN_CASES} == {"normal", "const", "bigmean", "count1"}
    assert {c.null for c in BC.FIN_CASES} == set(BC.FIN_NULLS) | {None} and {c.momentum for c in BC.FIN_CASES} >= {0.0, 1.0}
    assert {c.null for c in BC.BFIN_CASES} == set(BC.BFIN_NULLS) | {None} and {c.flavour for c in BC.BFIN_CASES} == {"train0", "train1"}
    assert {p for p, _, _ in BC.PFOLD_CASES} >= set(BC.FOLD_PERS) and {c for _, c, _ in BC.PFOLD_CASES} == set(BC.FOLD_CS)
    assert all(BC.pfold_rows(p, o) % p for p, _, o in BC.PFOLD_CASES if p >= 3 and o > 1)          # the last chunk is ragged
    assert {(t, co == 1, co == c, a) for t, _, c, _, co, a in BC.CSUM_CASES} >= {(t, x, y, a) for t in ("small", "oct", "quad") for x, y in ((True, False), (False, True)) for a in (0, 1)}
    assert any(co == c // 4 and co > 1 for _, _, c, _, co, _ in BC.CSUM_CASES)


# ---- the gates have teeth --------------------------------------------------------------------------------------------------------
class WrongBn(A.AbiEmulator):
    """the model with one thing wrong.  drop_last: the reductions lose the view's last voxel; twice: they count the first voxel twice;
    gate_ge: the ReLU gate is z >= 0; no_shift: the gate ignores the shift; past_view: the apply writes one channel past dx's view;
    split_trunc: the hi plane is truncated, not rounded; biased: running_var takes the biased variance; fold_off: partials_fold
    reads one row too few in its last chunk"""

    def __init__(self, wrong):
        super().__init__()
        self.wrong = wrong

    def _tamper(self, x, dtype, partials, dz=None):
        x = A._deref(x)
        v = A.rd(x, dtype).reshape(-1, x.C).astype(np.float64)
        g = None if dz is None else A.rd(A._deref(dz), dtype).reshape(-1, x.C).astype(np.float64)
        return v, g, A._f32(partials, 2 * x.C).reshape(2, x.C)

    def vinet_channel_stats(self, x, dtype, partials, stream):
        rc = super().vinet_channel_stats(x, dtype, partials, stream)
        if self.wrong in ("drop_last", "twice"):
            v, _, P = self._tamper(x, dtype, partials)
            at, sign = (-1, -1.0) if self.wrong == "drop_last" else (0, 1.0)
            P[0] += sign * v[at]
            P[1] += sign * v[at] * v[at]
        return rc

    def _bn_bwd_terms(self, dz, x_raw, dtype, fwd, mean, invstd):
        if self.wrong in ("gate_ge", "no_shift") and fwd.relu:
            Cc = x_raw.C
            xv, g = A.rd(x_raw, dtype), A.rd(dz, dtype)
            z = xv.astype(np.float64) * (A._f32(fwd.scale, Cc) if fwd.scale else 1.0) + (A._f32(fwd.shift, Cc) if fwd.shift and self.wrong == "gate_ge" else 0.0)
            g = g * ((z >= 0) if self.wrong == "gate_ge" else (z > 0))
            return g, (xv - A._f32(mean, Cc)) * A._f32(invstd, Cc)
        return super()._bn_bwd_terms(dz, x_raw, dtype, fwd, mean, invstd)

    def vinet_bn_bwd_apply(self, dz, x_raw, dtype, fwd, mean, invstd, c1, c2, dx, stream):
        rc = super().vinet_bn_bwd_apply(dz, x_raw, dtype, fwd, mean, invstd, c1, c2, dx, stream)
        if self.wrong == "past_view":
            d = A._deref(dx)
            raw = A._raw(d.ptr, A._span(d), dtype)
            v = A._strided(d, dtype)
            for b in range(d.B):
                rows = v[b].reshape(-1, d.C)
                off = b * d.sB + np.arange(rows.shape[0]) * d.ld + d.C
                ok = off < raw.shape[0]
                raw[off[ok]] = rows[ok, -1]
        return rc

    def vinet_split_bf16(self, src, pre, hi, lo, stream):
        rc = super().vinet_split_bf16(src, pre, hi, lo, stream)
        if self.wrong == "split_trunc":
            v = A.rd(A._deref(src), F32)
            u = np.ascontiguousarray(v).view(np.uint32) & 0xFFFF0000
            A.wr(A._deref(hi), BF16, u.view(np.float32))
        return rc

    def vinet_bn_finalize(self, partials, rows, Cc, ld, count, gamma, beta, eps, momentum, rm, rv, mean, invstd, scale, shift, stream):
        if self.wrong == "biased" and rv:
            keep = A._f32(rv, Cc).copy()
            rc = super().vinet_bn_finalize(partials, rows, Cc, ld, count, gamma, beta, eps, momentum, rm, rv, mean, invstd, scale, shift, stream)
            new = A._f32(rv, Cc)
            m = np.float32(momentum)
            if count > 1 and m > 0:
                new[:] = (1 - m) * keep + (new - (1 - m) * keep) * np.float32((count - 1) / count)
            return rc
        return super().vinet_bn_finalize(partials, rows, Cc, ld, count, gamma, beta, eps, momentum, rm, rv, mean, invstd, scale, shift, stream)

    def vinet_bn_partials_fold(self, partials, rows, Cc, out, out_rows, stream):
        rc = super().vinet_bn_partials_fold(partials, rows, Cc, out, out_rows, stream)
        if self.wrong == "fold_off" and rc == 0:
            P = A._f32(partials, rows * 2 * Cc).reshape(rows, 2, Cc)
            A._f32(out, out_rows * 2 * Cc).reshape(out_rows, 2, Cc)[-1] -= P[-1]
        return rc


def _failed(check, cases, wrong):
    out = []
    for case in cases:
        try:
            check(_side(WrongBn(wrong)), *(case if isinstance(case, tuple) else (case,)))
        except AssertionError:
            out.append(case)
    return out


@pytest.mark.parametrize("wrong", ["drop_last", "twice"])
def test_a_model_that_miscounts_a_voxel_fails_the_stats_cases(wrong):
    cases = [c for c in BC.REDUCE_CASES if c.mode == 0 and c.nvox <= 260]
    failed = _failed(BC.check_reduce, cases, wrong)
    # exact data: every case whose miscounted voxel is not all zeros fails; random data: the bound is far below one term
    assert {c.data for c in failed} == {"exact", "rand"} and len(failed) >= len(cases) * 3 // 4, (wrong, len(failed), len(cases))


@pytest.mark.parametrize("wrong", ["gate_ge", "no_shift"])
def test_a_model_with_a_wrong_gate_fails_the_affine_cases(wrong):
    cases = [c for c in BC.REDUCE_CASES if c.mode == 1 and c.nvox in (130, 260)]
    failed = _failed(BC.check_reduce, cases, wrong)
    assert failed and {c.fwd for c in failed} == ({"affine", "relu"} if wrong == "gate_ge" else {"affine"})
    assert "exact" in {c.data for c in failed}
    assert _failed(BC.check_apply, [c for c in BC.APPLY_CASES if c.relu and c.nvox == 260 and c.data == "exact"], wrong)


@pytest.mark.parametrize("wrong,fn,cases", [
    ("past_view", BC.check_apply, [c for c in BC.APPLY_CASES if c.nvox == 260]),
    ("split_trunc", BC.check_apply, [c for c in BC.APPLY_CASES if c.split and c.nvox == 260 and c.data == "rand"]),
    ("biased", BC.check_finalize, BC.FIN_CASES),
    ("fold_off", BC.check_partials_fold, BC.PFOLD_CASES)], ids=["past_view", "split_trunc", "biased", "fold_off"])
def test_a_wrong_model_fails_a_case(wrong, fn, cases):
    failed = _failed(fn, cases, wrong)
    assert failed, wrong
    if wrong == "past_view":          # wherever something lies behind a row of the view: every form but the dense one
        assert {c.dxform if c.dxform != "inplace" else c.inform for c in failed} >= {"chan", "tslice", "both"}
    if wrong == "fold_off":
        assert len(failed) == len(cases)
