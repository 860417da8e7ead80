"""tests/layout_cases.py without a GPU: every case runs through the CPU model of the ABI (tests/abi_emulator.py) at the gates the GPU
test applies to the library.  The model stores the split format VINET_F32S as plain fp32 by design, so an F32S pack case does two
things here: its reference is checked against its own definition (de-permuted hi + lo within 2^-16 |v| of v, zero padding, every
position written once), and the model runs the same jobs as F32 against the F32 reference.  The module also asserts, from the Python
mirrors of pt_shape, the prefix split and the copy route, that the tables reach the edges they claim, and holds the argument
refusals on the real library (host code: they return before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import abi_emulator as A
from tests import layout_cases as LC
from vinet_amd import _lib as L

F32, BF16, F32S = LC.F32, LC.BF16, LC.F32S


def _side(model=None):
    return LC.Side(model or A.AbiEmulator())


@pytest.mark.parametrize("dt", LC.PDTS, ids=[LC.PDTN[d] for d in LC.PDTS])
@pytest.mark.parametrize("case", LC.PACK_CASES, ids=[repr(c) for c in LC.PACK_CASES])
def test_pack_case(case, dt):
    if dt == F32S:
        LC.check_f32s_reference(case)
        dt = F32
    LC.check_pack(_side(), case, dt)


@pytest.mark.parametrize("case,flags", LC.UNPACK_CASES, ids=["%r-flags%d" % cf for cf in LC.UNPACK_CASES])
def test_unpack_case(case, flags):
    LC.check_unpack(_side(), case, flags)


@pytest.mark.parametrize("case", LC.IMPORT_CASES, ids=[c.id for c in LC.IMPORT_CASES])
def test_import_case(case):
    LC.check_import(_side(), case)


@pytest.mark.parametrize("case", LC.EXPORT_CASES, ids=[c.id for c in LC.EXPORT_CASES])
def test_export_case(case):
    LC.check_export(_side(), case)


@pytest.mark.parametrize("case", LC.COPY_CASES, ids=[c.id for c in LC.COPY_CASES])
def test_copy_case(case):
    LC.check_copy(_side(), case)


@pytest.mark.parametrize("case", LC.SPLIT_CASES, ids=["q%d-hi_%s-lo_%s-%s-%s-src_%s" % (c[0], c[1], c[2], c[5], c[6], c[7]) for c in LC.SPLIT_CASES])
def test_split_case(case):
    LC.check_split(_side(), *case)


def test_refusals_of_the_library():
    """the argument checks run before any launch: the real library answers them on host memory, without a device"""
    lib = L.load()
    assert not L.is_test_double()
    LC.check_refusals(LC.Side(lib))


# ---- the mirrors and what the tables reach -----------------------------------------------------------------------------------------
def test_the_split_position_table_is_the_formats_permutation():
    assert sorted(LC.F32S_POS) == list(range(32))
    for q in range(4):          # lane group q: K positions 8q .. 8q+7 hold channels {4q .. 4q+3, 16+4q .. 16+4q+3}
        assert sorted(c for c in range(32) if LC.F32S_POS[c] // 8 == q) == list(range(4 * q, 4 * q + 4)) + list(range(16 + 4 * q, 20 + 4 * q))
        assert [LC.F32S_POS[4 * q + e] for e in range(4)] == [8 * q + e for e in range(4)]            # a 16-byte piece stays in order
        assert [LC.F32S_POS[16 + 4 * q + e] for e in range(4)] == [8 * q + 4 + e for e in range(4)]


def test_the_pack_tables_cover_the_edges():
    # both sides of every tap boundary, in the class the mirror says
    assert set(LC.TAPS) == {1, 27, 32, 33, 64, 65, 128, 129, 256, 257}
    assert [LC.pt_pairs(t) for t in (32, 33, 64, 65, 128, 129, 256)] == [256, 128, 128, 64, 64, 32, 32]
    by_tag = {c.tag: c for c in LC.PACK_CASES}
    for nt in LC.TAPS:
        jobs = by_tag["taps%d" % nt].jobs
        fwd, trn = [j for j in jobs if not j.tr], [j for j in jobs if j.tr]
        if nt > 256:          # the in-kernel element-wise branch of a tiled launch
            assert all(j.shape["TRn"] == 0 and j.shape["units"] == -(-j.numel // 256) for j in jobs)
            continue
        pairs = LC.pt_pairs(nt)
        assert all((j.shape["TRn"], j.shape["TCc"]) == (pairs // 32, 32) for j in fwd) and all((j.shape["TRn"], j.shape["TCc"]) == (pairs // 8, 8) for j in trn)
        TRn = pairs // 32
        assert {(j.N, j.Cin) for j in fwd} >= {(n, c) for n in (TRn - 1, TRn + 1) if n > 0 for c in (31, 33)}
        assert {(j.N, j.Cin) for j in trn} >= {(n, c) for n in (31, 33) for c in (7, 9)}
        # ragged tiles on both axes: rows past N, columns past Cin
        assert (TRn == 1 or any(j.N % TRn for j in fwd)) and any(j.Cin % 32 for j in fwd) and any(j.Cin % 8 for j in trn) and any(j.N % j.shape["TRn"] for j in trn)
        for j in jobs:
            assert j.shape["TRn"] * j.shape["rs"] <= LC.PT_LDS_FLOATS, j
        if nt in LC.CLASS_TOP:
            assert {(j.N, j.Cin, j.tr) for j in jobs} >= {(1, 1, 0), (1, 1, 1), (TRn, 32, 0), (pairs // 8, 32, 1)}
            # whole tiles at the largest tap count of the class: the most LDS a tile of this class ever takes
            full = [j for j in jobs if j.N >= j.shape["TRn"] and j.N % j.shape["TRn"] == 0 and j.Cin % j.shape["TCc"] == 0]
            assert {j.tr for j in full} == {0, 1}
            assert all(j.shape["TRn"] * j.shape["rs"] == pairs * nt + j.shape["TRn"] <= LC.PT_LDS_FLOATS for j in full)
    # the 64- and 32-pair classes: forward 2 x 32 and 1 x 32, transposed 8 x 8 and 4 x 8
    shapes = {(j.shape["TRn"], j.shape["TCc"], j.tr) for c in LC.PACK_CASES for j in c.jobs}
    assert shapes >= {(8, 32, 0), (4, 32, 0), (2, 32, 0), (1, 32, 0), (32, 8, 1), (16, 8, 1), (8, 8, 1), (4, 8, 1)}
    # the stem, a stem of 4 channels and one row; side-by-side jobs at col = 32 and at the columns of a joint conv
    misc = by_tag["misc"].jobs
    assert {(j.N, j.Cin) for j in misc if j.stem} == {(64, 3), (1, 4)}
    ld = [j for j in misc if j.ld]
    assert all(j.ld % 32 == 0 and j.tr for j in ld) and {j.col for j in ld} >= {0, 32, 160, 272} and any(j.col % 32 for j in ld) and any(j.ntaps > 1 for j in ld)
    members = (160, 112, 24)          # Mixed_4c's entry convs (engine.JointConvPlan.offs: running sums of the members' N)
    assert [sum(members[:i]) for i in range(3)] == sorted(j.col for j in ld if j.dest == "c")
    # the prefix table: per = 1, 2, 4, a ragged last thread, the cap and the fall-back past it
    assert tuple(len(by_tag["njobs%d" % n].jobs) for n in LC.JOB_COUNTS) == LC.JOB_COUNTS == (1, 255, 256, 257, 1024, 1025)
    assert {LC.prefix_per(n) for n in LC.JOB_COUNTS if n <= LC.PT_MAXJOBS} == {1, 2, 4}
    assert LC.prefix_per(257) == 2 and 257 % 2 == 1 and LC.PT_MAXJOBS in LC.JOB_COUNTS
    assert LC.pack_kernel("tiled", F32, 1024) == "pack_weights_tiled_kernel<f32>" and LC.pack_kernel("tiled", F32, 1025) == "pack_weights_multi_kernel<f32>"
    assert LC.pack_kernel("tiled", F32, 1025, True) == "unpack_wgrad_multi_kernel"
    cyc = by_tag["njobs257"].jobs[:5]
    assert any(j.stem for j in cyc) and any(j.tr for j in cyc) and len({(j.N, j.Cin, j.ntaps) for j in cyc}) == 5
    # two-unit workgroups: some of the 2048 take two units, some one
    assert LC.PT_GRID < by_tag["units"].units < 2 * LC.PT_GRID and LC.pt_shape(520, 1024, 1)["units"] == 65 * 32
    ucases = {c.tag: c for c, _ in LC.UNPACK_CASES}
    assert LC.PT_GRID < ucases["units"].units < 2 * LC.PT_GRID
    assert {f for c, f in LC.UNPACK_CASES if c.tag == "taps129"} == {0, 1, 2, 3}
    assert all(j.unpack_ok() for c, _ in LC.UNPACK_CASES for j in c.jobs)
    assert {len(c.jobs) for c, _ in LC.UNPACK_CASES if c.tag.startswith("njobs")} == set(LC.JOB_COUNTS)


def test_the_io_tables_cover_the_edges():
    ids = [c.id for c in LC.IO_CASES]
    assert len(ids) == len(set(ids))
    for kind in ("import", "export"):
        mine = [c for c in LC.IO_CASES if c.kind == kind]
        assert {c.dims[0] * c.dims[1] * c.dims[2] * c.dims[3] for c in mine} >= {1, 255, 256, 257}
        for axis in (1, 2, 3):
            assert any(c.dims[axis] == 1 and c.dims[0] == 2 for c in mine), (kind, axis)
        assert {c.form for c in mine} == set(LC.FORMS) and {c.dt for c in mine} == {F32, BF16}
    imp = [c for c in LC.IO_CASES if c.kind == "import"]
    assert {(c.C, c.dstC) for c in imp} >= {(1, 4), (3, 4), (4, 4), (5, 8), (4, 8)} and {c.src for c in imp} == {"perm", "bcast"}
    pad = [c for c in LC.IO_CASES if c.kind == "import_pad"]
    assert {c.pad[2:] for c in pad} >= {(0, 0), (3, 3), (0, 5)} and {c.src for c in pad} == {"perm", "bcast"} and {c.form for c in pad} == set(LC.FORMS)
    assert any(c.pad[2] + c.pad[0] == c.dims[2] and c.pad[3] + c.pad[1] == c.dims[3] for c in pad)
    assert any(c.pad[2] + c.pad[0] < c.dims[2] and c.pad[3] + c.pad[1] < c.dims[3] for c in pad)
    assert any(c.pad[:2] == (1, 1) for c in pad) and any(c.dims[3] > LC.BLOCK for c in pad)
    for Hs, Ws in ((3, 5), (4, 6), (1, 1)):          # the folded stem: H + 6 by W + 8 + (W & 1), pads 3 and 3
        assert any(c.pad == (Hs, Ws, 3, 3) and c.dims[2:] == (Hs + 6, Ws + 8 + (Ws & 1)) and c.C == 3 and c.dstC == 4 for c in pad)
    exp = [c for c in LC.IO_CASES if c.kind == "export"]
    assert {(c.acc, c.aff, c.data) for c in exp} == {(a, f, d) for a in (0, 1) for f in LC.AFFS for d in ("exact", "rand")}
    assert {c.perm for c in exp} == {False, True}


def test_the_copy_table_covers_the_edges():
    ids = [c.id for c in LC.COPY_CASES]
    assert len(ids) == len(set(ids))
    assert {c.kernel for c in LC.COPY_CASES} == set(LC.COPY_KERNELS)
    quad = [c for c in LC.COPY_CASES if c.tag == "quad"]
    assert {(c.sdt, c.ddt, c.acc, c.aff) for c in quad} == {(s, d, a, f) for s in LC.DTS for d in LC.DTS for a in (0, 1) for f in LC.AFFS}
    assert {c.nvox * c.C // 4 for c in quad} >= {1, 255, 256, 257} and {c.C for c in quad} == {4, 12}
    assert {c.data for c in quad} == {"exact", "rand"} and {c.sform for c in quad} == set(LC.FORMS) and {c.dform for c in quad} >= set(LC.FORMS) | {"inplace"}
    # off the 8-channel grid for one reason alone, where the 8-channel kernel would otherwise run
    for tag, why in (("ptr8mod16", ["ptr"]), ("ld_c_plus4", ["ld"]), ("sB_alone", ["sB"]), ("sB4mod8", ["ld", "ptr"])):
        mine = [c for c in LC.COPY_CASES if c.tag == tag]
        assert mine and all(c.kernel == "copy_affine_kernel<bf16,bf16>" and c.nvox >= LC.OCT_MIN and c.C == 8 and c.sdt == c.ddt == BF16 for c in mine)
        assert {("src" if c.sform != "dense" else "dst", c.dform == "inplace") for c in mine} == {("src", False), ("dst", False), ("src", True)}
        for c in mine:          # the source's view, the destination's, or the one view of an in-place copy: off the grid for `why` alone
            s_ = LC.make_slab(c.dims, c.sdt, c.sform, c.schan, LC.Geo)
            d_ = s_ if c.dform == "inplace" else LC.make_slab(c.dims, c.ddt, c.dform, c.dchan, LC.Geo)
            assert sorted([LC.oct_failures(s_), LC.oct_failures(d_)]) in ([[], why], [why, why]), (c, LC.oct_failures(s_), LC.oct_failures(d_))
            assert LC.quad_ok(s_) and LC.quad_ok(d_)
    # both routes on both sides of 65 536 voxels, the block seam, idle threads
    seam = [c for c in LC.COPY_CASES if c.tag == "seam"]
    assert (LC.copy_vb(8), LC.copy_vb(24), LC.copy_vb(200), LC.copy_vb(512)) == (4096, 1360, 160, 64) and 256 % (24 // 8) and 256 % (200 // 8)
    for Cc in (8, 24, 200):
        vb = LC.copy_vb(Cc)
        assert {c.nvox for c in seam if c.C == Cc} == {65535, 65536, 65537, 65536 + vb - 1, 65536 + vb + 1}
        assert {c.kernel for c in seam if c.C == Cc and c.nvox == 65535} == {"copy_affine_kernel<bf16,bf16>"}
        assert {c.kernel for c in seam if c.C == Cc and c.nvox >= 65536} == {"copy_affine8_kernel"}
        assert {c.dform == "inplace" for c in seam if c.C == Cc and c.nvox >= 65536} == {False, True}
    assert any(c.C == 512 and c.kernel == "copy_affine8_kernel" for c in seam)
    assert {c.data for c in seam if c.C <= 24} == {"exact", "rand"} and {c.data for c in seam if c.C > 24} == {"exact"}
    oct_ = [c for c in LC.COPY_CASES if c.kernel == "copy_affine8_kernel"]
    assert {c.acc for c in oct_} == {0, 1} and {c.aff for c in oct_} == set(LC.AFFS) and {c.sform for c in oct_} >= {"dense", "chan", "tslice"}
    # the other type pairs stay on the quad kernel past the threshold
    assert {c.kernel for c in LC.COPY_CASES if c.tag == "pairs"} == set(LC.COPY_KERNELS) - {"copy_affine8_kernel", "copy_affine_kernel<bf16,bf16>"}
    # split_bf16: 1, 255, 257 quads, planes with different ld, one of them a T slice, with and without the affine
    assert {c[0] for c in LC.SPLIT_CASES} == {1, 255, 257} and {c[5] for c in LC.SPLIT_CASES} == set(LC.AFFS)
    assert all(("tslice" in (c[1], c[2])) or ("both" in (c[1], c[2])) for c in LC.SPLIT_CASES)


# ---- the gates have teeth ------------------------------------------------------------------------------------------------------------
class WrongLayout(A.AbiEmulator):
    """the model with one thing wrong.  pad_dirty: a pack leaves its last padding column unwritten; ld_spill: a side-by-side job also
    writes the column behind its own; keep_pad: the clear flag leaves the padding columns; pad_shift: import_pad is one column
    off; drop_last: copy_affine leaves the view's last voxel as it was; no_acc: export ignores `accumulate`"""

    def __init__(self, wrong):
        super().__init__()
        self.wrong = wrong

    def vinet_pack_weights(self, w, N, Cin, ntaps, transpose, stem, dtype, out, stream):
        if self.wrong == "pad_dirty" and not stem and (N if transpose else Cin) % 32:
            rows, kp = (Cin if transpose else N), ((N if transpose else Cin) + 31) // 32 * 32
            raw = A._raw(out, ntaps * rows * kp, dtype)
            keep = raw[kp - 1]
            rc = super().vinet_pack_weights(w, N, Cin, ntaps, transpose, stem, dtype, out, stream)
            raw[kp - 1] = keep
            return rc
        return super().vinet_pack_weights(w, N, Cin, ntaps, transpose, stem, dtype, out, stream)

    def vinet_pack_weights_multi(self, table, njobs, total, dtype, stream):
        rc = super().vinet_pack_weights_multi(table, njobs, total, dtype, stream)
        if self.wrong == "ld_spill":
            tab = np.ctypeslib.as_array((C.c_int64 * (8 * (njobs + 1))).from_address(table)).reshape(njobs + 1, 8)
            for j in range(njobs):
                ld, col = int(tab[j, 7]) & 0xffffffff, int(tab[j, 7]) >> 32
                if ld and col + int(tab[j, 2]) < ld:
                    A._raw(int(tab[j, 1]), ld, dtype)[col + int(tab[j, 2])] = 0
        return rc

    def vinet_unpack_wgrad(self, dw, N, Cin, ntaps, stem, accumulate, grad, stream):
        if self.wrong == "keep_pad" and accumulate & 2 and not stem and Cin % 32:
            kp = (Cin + 31) // 32 * 32
            raw = A._f32(dw, ntaps * N * kp)
            keep = float(raw[kp - 1])
            rc = super().vinet_unpack_wgrad(dw, N, Cin, ntaps, stem, accumulate, grad, stream)
            raw[kp - 1] = keep
            return rc
        return super().vinet_unpack_wgrad(dw, N, Cin, ntaps, stem, accumulate, grad, stream)

    def vinet_import_ncdhw_pad(self, src, sb, sc, st, sh, sw, Cc, Hs, Ws, pad_top, pad_left, dst, dst_dtype, stream):
        d = A._deref(dst)
        if self.wrong == "pad_shift" and pad_left + Ws < d.W:
            pad_left += 1
        return super().vinet_import_ncdhw_pad(src, sb, sc, st, sh, sw, Cc, Hs, Ws, pad_top, pad_left, dst, dst_dtype, stream)


    def vinet_copy_affine(self, src, src_dtype, pre, dst, dst_dtype, accumulate, stream):
        if self.wrong != "drop_last":
            return super().vinet_copy_affine(src, src_dtype, pre, dst, dst_dtype, accumulate, stream)
        last = A._strided(A._deref(dst), dst_dtype)[-1, -1, -1, -1]
        keep = last.copy()
        rc = super().vinet_copy_affine(src, src_dtype, pre, dst, dst_dtype, accumulate, stream)
        last[:] = keep
        return rc

    def vinet_export_ncdhw(self, src, src_dtype, pre, dst, sb, sc, st, sh, sw, accumulate, stream):
        return super().vinet_export_ncdhw(src, src_dtype, pre, dst, sb, sc, st, sh, sw, 0 if self.wrong == "no_acc" else accumulate, stream)


def _failed(check, cases, wrong):
    out = []
    for args in cases:
        try:
            check(_side(WrongLayout(wrong)), *args)
        except AssertionError:
            out.append(args)
    return out


def test_a_wrong_model_fails_the_cases():
    packs = [(c, dt) for c in LC.PACK_CASES if c.tag in ("taps27", "taps129", "misc") for dt in (F32, BF16)]
    assert len(_failed(LC.check_pack, [p for p in packs if p[0].tag != "misc"], "pad_dirty")) == 4
    assert _failed(LC.check_pack, [p for p in packs if p[0].tag == "misc"], "ld_spill")
    assert not _failed(LC.check_pack, [p for p in packs if p[0].tag != "misc"], "ld_spill")
    unp = [(c, f) for c, f in LC.UNPACK_CASES if c.tag == "taps33"]
    assert {f for _, f in _failed(LC.check_unpack, unp, "keep_pad")} == {2, 3}
    pads = [(c,) for c in LC.IMPORT_CASES if c.kind == "import_pad"]
    failed = _failed(LC.check_import, pads, "pad_shift")
    assert failed and all(c.pad[3] + c.pad[1] < c.dims[3] for c, in failed)


def test_a_wrong_copy_or_export_fails_the_cases():
    small = [(c,) for c in LC.COPY_CASES if c.tag == "quad" and c.nvox >= 85 and c.sdt == F32]
    failed = _failed(LC.check_copy, small, "drop_last")
    # a voxel left as it was shows wherever the copy changes it: every store into the sentinel, every accumulate of a non-zero value
    assert {c.data for c, in failed} == {"exact", "rand"} and len(failed) >= len(small) * 3 // 4 and {c.dform for c, in failed} >= set(LC.FORMS) | {"inplace"}
    exps = [(c,) for c in LC.EXPORT_CASES if c.dims == (1, 3, 5, 17)]
    assert {c.acc for c, in _failed(LC.check_export, exps, "no_acc")} == {1} and len(_failed(LC.check_export, exps, "no_acc")) == len(exps) // 2


def test_a_tampered_split_reference_is_caught():
    """the F32S self-check reads the reference through the position table: a table with two channels swapped no longer de-permutes"""
    case = next(c for c in LC.PACK_CASES if c.tag == "taps27")
    keep = list(LC.F32S_POS)
    want, _ = LC.pack_expected(case, F32S)
    try:
        LC.F32S_POS[3], LC.F32S_POS[16] = LC.F32S_POS[16], LC.F32S_POS[3]
        assert not torch.equal(LC._bits(LC.pack_expected(case, F32S)[0]), LC._bits(want))
    finally:
        LC.F32S_POS[:] = keep
    LC.check_f32s_reference(case)
