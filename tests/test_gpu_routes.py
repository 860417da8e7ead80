"""Every conv / weight-gradient instantiation the launch tables name, and every value of the library options (options.h), on its
own: the exact kernel name (vinet_conv3d_kernel_name / vinet_conv3d_wgrad_kernel_name -- equality, not a prefix), then the case
bit for bit against the ABI model on exact-arithmetic inputs and under the suite's tolerance on random ones.  The exact comparison
of every ledger entry must also REJECT three deliberately wrong references (altered on the CPU side only).

The ledgers and the option table are plain data: tests/test_route_tables.py checks them against the launch tables, options.h and
the library's host-side routing without a GPU."""
import contextlib
import ctypes as C
import os

import pytest
import torch

from tests import route_cases as R
from tests import test_gpu_kernels as K
from tests.abi_emulator import AbiEmulator
from vinet_amd import _lib as L
from vinet_amd import engine as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS_H = os.path.join(ROOT, "vinet_amd", "csrc", "options.h")
OPT_DEFAULTS = R.option_defaults(OPTIONS_H)
BF16, F32, F32S = E.BF16, E.F32, L.F32S


@pytest.fixture(autouse=True)
def _options_back_to_the_header_defaults():
    yield
    lib = L.load()
    for k, v in OPT_DEFAULTS.items():
        lib.vinet_set_option(k.encode(), v)


def _opts(o):
    return R.options(L.load(), o, OPT_DEFAULTS)


def _case(table, name, **more):
    c = next(c for c in table if c[0] == name)
    return c[:7] + (dict(c[7], **more),) if more else c


def _wcase(table, name, **more):
    c = next(c for c in table if c[0] == name)
    return c[:8] + (dict(c[8] if len(c) > 8 else {}, **more),)


# ====================================================================================================================
# 1. the convolution ledger
# ====================================================================================================================
PW1, SP3, T3 = ((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((1, 3, 3), (1, 1, 1), (0, 1, 1)), ((3, 1, 1), (1, 1, 1), (1, 0, 0))
LADDER = dict(pp=0, ht=0, pw=0)      # the ladder reaches CONV_DMA (CONV_IGEMM with dma = 0)

# conv_dma / conv_igemm tiles: (tile, options beyond LADDER, plain case, pre case).  The plain cases have whole column tiles, the pre
# cases a ragged N (56, 120, 88, ...) where the picker still lands on the tile; every M leaves a ragged last row tile except the
# natural 131072-row case of the two large tiles (M = 131043 = 511 x 256 + 227 beside it)
BIG, BIG_RAGGED = (2, 4, 128, 128), (1, 1, 361, 363)
DMA_TILES = [
    ((4, 1, 4, 1), {}, ("t_n16", (1, 2, 9, 15), 64, 16) + SP3 + ({},), ("t_n8_pre", (1, 2, 9, 15), 64, 8) + SP3 + (dict(pre=True, stats=True),)),
    ((4, 2, 4, 1), {}, ("t_n32", (1, 2, 9, 15), 96, 32) + T3 + (dict(stats=True),), ("t_n24_pre", (2, 2, 9, 15), 64, 24) + SP3 + (dict(pre=True, act=1),)),
    ((4, 3, 4, 1), {}, ("t_n48", (1, 2, 9, 15), 64, 48) + SP3 + (dict(epi=True, act=1),), ("t_n40_pre", (1, 2, 9, 15), 40, 40) + PW1 + (dict(pre=True, stats=True),)),
    ((2, 2, 2, 2), {}, ("t_n64", (1, 2, 9, 15), 64, 64) + SP3 + (dict(stats=True),), ("t_n56_pre", (1, 2, 9, 15), 96, 56) + T3 + (dict(pre=True),)),
    ((2, 4, 2, 2), {}, ("t_n128", (1, 2, 9, 15), 64, 128) + SP3 + ({},), ("t_n120_pre", (1, 2, 9, 15), 64, 120) + SP3 + (dict(pre=True, stats=True, act=1),)),
    ((4, 2, 2, 2), dict(n64_tile=1), ("t_n64_128r", (1, 2, 9, 15), 64, 64) + SP3 + (dict(stats=True),), ("t_n56_128r_pre", (1, 2, 9, 15), 96, 56) + T3 + (dict(pre=True),)),
    ((4, 4, 2, 2), dict(n128_tile=1), ("t_n128_128r", (1, 2, 9, 15), 64, 128) + SP3 + ({},), ("t_n120_128r_pre", (1, 2, 9, 15), 64, 120) + SP3 + (dict(pre=True, stats=True),)),
    ((4, 6, 2, 2), dict(n192_tile=2), ("t_n192", (1, 2, 9, 15), 64, 192) + SP3 + (dict(stats=True),), ("t_n192_pre", (1, 3, 9, 15), 96, 192) + T3 + (dict(pre=True, act=1),)),
    ((4, 6, 4, 1), {}, ("t_n96_m16380", (1, 2, 91, 90), 32, 96) + PW1 + (dict(stats=True),), ("t_n88_m16380_pre", (1, 2, 91, 90), 32, 88) + PW1 + (dict(pre=True),)),
    ((4, 4, 4, 1), {}, ("t_n64_m131072", BIG, 32, 64) + PW1 + (dict(stats=True),), ("t_n56_m131043_pre", BIG_RAGGED, 32, 56) + PW1 + (dict(pre=True),)),
    ((4, 8, 4, 1), dict(n128_kmax=0), ("t_n128_m131072", BIG, 32, 128) + PW1 + ({},), ("t_n120_m131043_pre", BIG_RAGGED, 32, 120) + PW1 + (dict(pre=True, stats=True),)),
]


def _bnb_of(case):      # the same plain case as a data gradient that also leaves the BatchNorm-backward sums (conv_bnb.hip)
    return (case[0] + "_bnb",) + case[1:7] + (dict(bnb=dict()),)


class Entry:
    def __init__(self, key, case, opts=None, dt=BF16, cdt=None, tol=None, runner="conv"):
        self.key, self.case, self.opts, self.dt, self.cdt, self.tol, self.runner = key, case, dict(opts or {}), dt, cdt, tol, runner
        self.name = key.split(" [")[0]      # " [bnb]" / " [natural]" ...: instantiations and routes the name does not tell apart

    def __repr__(self):
        return self.key


def _conv_ledger():
    out = []
    for (mt, nt, wm, wn), o, plain, pre in DMA_TILES:
        t = "%d,%d,%d,%d" % (mt, nt, wm, wn)
        out.append(Entry("conv_dma_kernel<%s,3,plain>" % t, plain, dict(LADDER, **o)))
        out.append(Entry("conv_dma_kernel<%s,3,pre>" % t, pre, dict(LADDER, **o)))
        out.append(Entry("conv_dma_kernel<%s,3,plain> [bnb]" % t, _bnb_of(plain), dict(LADDER, **o)))
        out.append(Entry("conv_igemm_kernel<bf16,%s,0>" % t, pre, dict(LADDER, dma=0, **o)))
        out.append(Entry("conv_igemm_kernel<bf16,%s,0> [plain]" % t, plain, dict(LADDER, dma=0, **o)))
    # the large tiles that split-K makes affordable: one sk_tile bit each, scratch lent
    sk64 = ("sk_n64_m4096", (1, 1, 64, 64), 352, 64) + SP3 + (dict(act=1, splitk=True),)
    out += [Entry("conv_dma_kernel<4,6,2,2,3,plain> [sk_tile=1]", _case(K.SPLITK_CASES, "sk_tile192", splitk=True), dict(LADDER, sk_tile=1)),
            Entry("conv_dma_kernel<4,4,2,2,3,plain> [sk_tile=2]", _case(K.SPLITK_CASES, "sk_tile128", splitk=True), dict(LADDER, sk_tile=2)),
            Entry("conv_dma_kernel<4,2,2,2,3,plain> [sk_tile=4]", sk64, dict(LADDER, sk_tile=4)),
            Entry("conv_dma_kernel<4,4,4,1,3,plain> [sk_tile=8]", sk64, dict(LADDER, sk_tile=8))]
    # the register-staged kernel on its natural route: a pending affine without ReLU, ReLU alone -- no option set
    for cname, pre in (("pw_pre_stats", "affine"), ("sp_3x3", "relu"), ("cin24", "affine"), ("concat_slice_out", "relu"), ("xslice_pre", "affine")):
        c = _case(K.CONV_CASES, cname, pre=pre)
        out.append(Entry("%s [natural, %s, %s]" % (R.NATURAL_IGEMM[cname], cname, pre), c))
    # fp32 tensors: exact fp32 MFMA and the split-bf16 form, the six widths the fp32 picker returns; conv_dma3
    for i, (nt, n) in enumerate(((8, 128), (6, 96), (4, 64), (3, 48), (2, 32), (1, 16))):
        c = ("f_n%d" % n, (1, 2, 9, 11), 32 + 32 * (i % 2), n) + (SP3 if i % 2 else T3) + (dict(pre=bool(i & 2), stats=bool(i & 1)),)
        out.append(Entry("conv_igemm_kernel<float,2,%d,4,1,0>" % nt, c, dt=F32))
        out.append(Entry("conv_igemm_kernel<float/split,2,%d,4,1,0>" % nt, c, dict(dma3=0), dt=F32, cdt=F32S, tol=1e-4))
    for n, pre in ((32, False), (32, True), (64, False), (64, True)):
        c = ("d3_n%d" % n, (1, 2, 9, 11), 64, n - 8 * pre) + SP3 + (dict(pre=pre, stats=not pre),)
        out.append(Entry("conv_dma3_kernel<%d,3,%s>" % (n, "pre" if pre else "plain"), c, dt=F32, cdt=F32S, tol=1e-4))
    # the stem form of the register-staged kernel.  tests.test_gpu_kernels.test_conv3d_stem_mode is the runner: it has no hook, so these
    # two entries run exact and random but WITHOUT the three wrong-reference rejections of the other entries
    out += [Entry("conv_igemm_kernel<bf16,4,4,4,1,1>", None, dt=BF16, runner="stem"), Entry("conv_igemm_kernel<float,2,4,4,1,1>", None, dt=F32, runner="stem")]
    # halo tiles: bf16 (14), split-bf16 (12), BatchNorm-backward (8)
    new = {
        "r_pw_32_pre": ("r_pw_32_pre", (2, 1, 8, 12), 32, 32) + PW1 + (dict(pre=True, stats=True),),
        "r_ht_32_16": ("r_ht_32_16", (1, 2, 18, 16), 64, 32) + SP3 + (dict(stats=True),),
        "r_ht_pre_64_32": ("r_ht_pre_64_32", (1, 2, 9, 32), 64, 64) + SP3 + (dict(pre=True, stats=True),),
        "r_ht_pre_96_16": ("r_ht_pre_96_16", (1, 2, 18, 16), 64, 96) + SP3 + (dict(pre=True, act=1),),
        "r_ht_pre_32_16": ("r_ht_pre_32_16", (1, 2, 18, 16), 64, 32) + SP3 + (dict(pre=True),),
        "r_htt_64": ("r_htt_64", (1, 5, 14, 24), 128, 64) + T3 + (dict(tline=True, stats=True),),
        "r_bnb_ht_64_16": ("r_bnb_ht_64_16", (1, 2, 18, 16), 64, 64) + SP3 + (dict(bnb=dict()),),
        "r_bnb_ht_32_16": ("r_bnb_ht_32_16", (1, 2, 18, 16), 64, 32) + SP3 + (dict(bnb=dict(relu=False)),),
    }

    def ht_case(n):
        c = new[n] if n in new else next(c for c in K.HT_CASES + K.BNB_CASES if c[0] == n)
        ex = dict(c[7])
        ex.setdefault("tline", 5)
        return c[:7] + (ex,)
    for name, cn in R.HT_BF16.items():
        out.append(Entry(name, ht_case(cn), dict(ht=2, ht_pre=1)))
    for name, cn in R.HT_F32S.items():
        out.append(Entry(name, ht_case(cn), dict(ht=2), dt=F32, cdt=F32S, tol=1e-4))
    for name, cn in R.HT_BNB.items():
        out.append(Entry(name + " [bnb]", ht_case(cn), dict(ht=2, pw=0, pp=0)))
    # pointwise streaming kernel (6), ping-pong kernel (2)
    for name, cn in R.PW.items():
        out.append(Entry(name, _case(K.PW_CASES + [new["r_pw_32_pre"]], cn, tline=6), dict(pw=2)))
    out += [Entry("conv_pp_kernel<256>", _case(K.PP_CASES, "pp_kp96_odd"), dict(pp=3)), Entry("conv_pp_kernel<192>", _case(K.PP_CASES, "pp_45taps"), dict(pp=4))]
    return out


CONV_LEDGER = _conv_ledger()


def _last_tile_rows(ns, bm):
    """index tensors (b, t, h, w) into y of the last `bm`-row M tile of the launch (linear m order; the halo tiles cut M by image
    rows instead: for them this is simply a tile-sized piece of the output that the reference loses)"""
    B, oT, oH, oW = ns["dims"]
    omT, ooT = ns["om"]
    M = ns["M"]
    m = torch.arange((M - 1) // bm * bm, M)
    return m // (oT * oH * oW), (m // (oH * oW)) % oT * omT + ooT, (m // oW) % oH, m % oW


def _conv_wrong_references(ns, bm):
    """the comparison that just passed must reject: a reference without one K chunk of 32, without the last M tile, shifted by a voxel"""
    emu = AbiEmulator()
    yp, wp, taps = ns["yp"], ns["wp"], ns["taps"]
    got, ref = yp.get("gpu"), yp.cpu.clone()

    def rerun():
        yp.cpu.copy_(ns["y_init"])
        assert emu.vinet_conv3d(*ns["mk"]("cpu")) == 0
        return yp.cpu.clone()

    wrong = {}
    keep = wp.cpu.clone()
    wp.cpu.view(ns["ntaps"], -1, ns["Kp"])[ns["ntaps"] // 2, :, 0:32] = 0
    wrong["one K chunk of 32 dropped"] = rerun()
    wp.cpu.copy_(keep)
    keep = taps.cpu.clone()
    taps.cpu[:, 2] += 1
    wrong["shifted by one voxel"] = rerun()
    taps.cpu.copy_(keep)
    yv = ns["ymk"]("cpu")
    w = ref.clone()
    idx = _last_tile_rows(ns, bm)
    w5 = E.View(w, yv.off, yv.B, yv.T, yv.H, yv.W, yv.C, yv.ld, yv.sB, ns["odt"]).torch5()
    i5 = E.View(ns["y_init"], yv.off, yv.B, yv.T, yv.H, yv.W, yv.C, yv.ld, yv.sB, ns["odt"]).torch5()
    w5[idx] = i5[idx]
    wrong["last M tile dropped"] = w
    yp.cpu.copy_(ref)
    for what, w in wrong.items():
        try:
            K._cmp(got, w, ns["tol"], what)
        except AssertionError:
            continue
        raise AssertionError("conv %s: the comparison ACCEPTED a wrong reference (%s)" % (ns["name"], what))


def _conv_info(lib, d):
    return dict(name=R.conv_name(lib, d), tile_m=lib.vinet_conv3d_tile_m(C.byref(d)), stats_rows=lib.vinet_conv3d_stats_rows(C.byref(d)),
                splitk_bytes=lib.vinet_conv3d_splitk_bytes(C.byref(d)), bnb_rows=lib.vinet_conv3d_bn_bwd_stats_rows(C.byref(d)))


def _probe_conv(case, opts, dt=BF16, cdt=None, tol=None, exact=True, selftest=False, more=None):
    """the case under `opts`: checked by the case runner against the ABI model; returns (y, float64 fold of the statistics rows,
    routing answers) of the GPU launch"""
    lib = L.load()
    out = {}

    def hook(ns):
        d = ns["mk"]("gpu")[0]._obj
        out["info"] = _conv_info(lib, d)
        out["y"] = ns["yp"].get("gpu").clone()
        r = out["info"]["stats_rows"]
        out["stats"] = ns["stats"].get("gpu")[:r * 2 * ns["N"]].view(r, 2, ns["N"]).double().sum(0) if case[7].get("stats") else None
        if ns["bpart"] is not None:
            br = out["info"]["bnb_rows"]
            out["bnb"] = ns["bpart"].get("gpu")[:br * 2 * ns["N"]].view(br, 2, ns["N"]).double().sum(0)
        if selftest:
            _conv_wrong_references(ns, out["info"]["tile_m"])
        if more:
            more(ns, out)
    with _opts(opts):
        with (K.exact_mode() if exact else contextlib.nullcontext()):
            # (forced: the ABI model's tile_m / statistics rows know neither the options nor the pointwise kernel's one row per workgroup)
            K._run_conv_case(case, dt, forced=bool(opts) or case[7].get("tline") == 6, cdt=cdt, tol=tol, hook=hook)
    return out


@pytest.mark.parametrize("e", CONV_LEDGER, ids=[e.key for e in CONV_LEDGER])
def test_conv_ledger(e):
    lib = L.load()
    if e.runner == "stem":
        d = R.stem_desc(e.dt)
        assert R.conv_name(lib, d) == e.name
        with K.exact_mode():
            K.test_conv3d_stem_mode(e.dt)
        K.test_conv3d_stem_mode(e.dt)
        return
    with _opts(e.opts):
        assert R.conv_name(lib, R.conv_desc(e.case, e.dt, e.cdt)) == e.name
    out = _probe_conv(e.case, e.opts, e.dt, e.cdt, e.tol, exact=True, selftest=True)
    assert out["info"]["name"] == e.name, (out["info"], e.name)
    if "[bnb]" in e.key:
        assert out["info"]["bnb_rows"] > 0
    if "[sk_tile" in e.key:
        assert out["info"]["splitk_bytes"] >= 2 * out["y"].numel() * 4
    out = _probe_conv(e.case, e.opts, e.dt, e.cdt, e.tol, exact=False)
    assert out["info"]["name"] == e.name


# ====================================================================================================================
# 2. the weight-gradient ledger
# ====================================================================================================================
RS_48 = ["rs_w32_k5", "rs_w64_k2", "rs_w96_k1", "rs_slices", "rs_n192", "rs_n128_k2", "rs_partial_chunks", "rs_w48", "rs_w24", "rs_w24_h3"]
RS_8 = ["rs_w192_n32", "rs_w128", "rs_w160"]


def _wgrad_ledger():
    out = []
    for cn in RS_48 + RS_8:
        c = _wcase(K.WGRAD_RS_CASES, cn, tline=4)
        W = c[1][3]
        if cn in RS_48:
            out.append(Entry("conv_wgrad_rs_kernel<W%d,4w> [%s]" % (W, cn), c, dict(wgrad_rs=2)))
        out.append(Entry("conv_wgrad_rs_kernel<W%d,8w> [%s]" % (W, cn), c, dict(wgrad_rs=2, wgrad_rs4=0)))
    for c in K.WGRAD_CASES:
        for tr in (1, 0):
            out.append(Entry("conv_wgrad_kernel<bf16,0> [%s, wgrad_tr=%d]" % (c[0], tr), c, dict(wgrad_dma=0, wgrad_tr=tr)))
    for cn in ("sp3", "cin24_n208"):
        c = _wcase(K.WGRAD_CASES, cn)
        for tr in (1, 0):
            out.append(Entry("conv_wgrad_kernel<float/split,0> [%s, wgrad_tr=%d]" % (cn, tr), c, dict(wgrad_dma=0, wgrad_tr=tr), dt=F32, cdt=F32S))
        out.append(Entry("conv_wgrad_kernel<float,0> [%s]" % cn, c, dict(wgrad_dma=0), dt=F32))      # (the exact-fp32 form reads LDS with ds_read_b32: no wgrad_tr)
    # the register-staged kernel on its natural route: a pending ReLU alone, an affine without ReLU -- no option set
    for cn, pre in (("sp3", "relu"), ("cin24_n208", "relu"), ("dec", "affine"), ("pw_slices", "affine")):
        c = _wcase(K.WGRAD_CASES, cn)
        out.append(Entry("conv_wgrad_kernel<bf16,0> [natural, %s, %s]" % (cn, pre), c[:7] + (pre,) + c[8:]))
    # conv_wgrad_dma_kernel<tn,tc,tg,.>: wgrad_dma.hip:383-387 -- (64,32,7) plain; (64,64,tg) for tg = 1, 2, 3, 7, 9, plain and pre.
    # (128,128,1) is instantiated (WG(128, 1, 3)) but wg_pick never returns tn = 128: unreachable, listed as such in route_cases.py
    t7 = ("dma_t7_c64", (1, 9, 5, 6), 64, 64, (7, 1, 1), (2, 1, 1), (3, 0, 0))
    t7n = ("dma_t7_c32", (1, 9, 5, 6), 32, 64, (7, 1, 1), (2, 1, 1), (3, 0, 0))
    t2 = ("dma_t2", (1, 4, 6, 7), 96, 80, (2, 1, 1), (2, 1, 1), (0, 0, 0))
    for key, c, o in [("64,64,1,plain", _wcase(K.WGRAD_CASES, "pw"), {}), ("64,64,1,pre", _wcase(K.WGRAD_CASES, "sp3"), {}),
                      ("64,64,2,plain", t2 + (False,), dict(wgrad_tg=2)), ("64,64,2,pre", t2 + (True,), dict(wgrad_tg=2)),
                      ("64,64,3,plain", _wcase(K.WGRAD_CASES, "cin24_n208"), dict(wgrad_tg=3)), ("64,64,3,pre", _wcase(K.WGRAD_CASES, "dec"), dict(wgrad_tg=3)),
                      ("64,64,7,plain", t7 + (False,), dict(wgrad_tg=7)), ("64,64,7,pre", t7n + (True,), dict(wgrad_tg=7)),
                      ("64,32,7,plain", t7n + (False,), dict(wgrad_tg=7)),
                      ("64,64,9,plain", _wcase(K.WGRAD_CASES, "cin24_n208"), dict(wgrad_tg=9)), ("64,64,9,pre", _wcase(K.WGRAD_CASES, "sp3_xslice"), dict(wgrad_tg=9))]:
        out.append(Entry("conv_wgrad_dma_kernel<%s>" % key, c, dict(o, wgrad_pp=0)))
    return out


WGRAD_LEDGER = _wgrad_ledger()


def _wgrad_wrong_references(ns):
    emu = AbiEmulator()
    dw, dp, taps = ns["dw"], ns["dp"], ns["taps"]
    got, ref = dw.get("gpu"), dw.cpu.clone()

    def rerun():
        dw.cpu.zero_()
        assert emu.vinet_conv3d_wgrad(*ns["mk"]("cpu")) == 0
        return dw.cpu.clone()

    wrong = {}
    ld = dp.cpu.numel() // ns["M"]
    keep = dp.cpu.clone()
    dp.cpu[:32 * ld] = 0                      # (the reduction axis of a weight gradient is the voxel index: its chunks are 32 voxels)
    wrong["one K chunk of 32 dropped"] = rerun()
    dp.cpu.copy_(keep)
    keep = taps.cpu.clone()
    taps.cpu[:, 2] += 1
    wrong["shifted by one voxel"] = rerun()
    taps.cpu.copy_(keep)
    w = ref.clone()
    w.view(-1, ns["N"], ns["Kp"])[:, (ns["N"] - 1) // 64 * 64:, :] = 0       # (M of this GEMM = the output channels: its last 64-row tile)
    wrong["last M tile dropped"] = w
    dw.cpu.copy_(ref)
    for what, w in wrong.items():
        try:
            K._cmp(got, w, ns["tol"], what)
        except AssertionError:
            continue
        raise AssertionError("wgrad %s: the comparison ACCEPTED a wrong reference (%s)" % (ns["name"], what))


def _probe_wgrad(case, opts, dt=BF16, cdt=None, exact=True, selftest=False):
    lib = L.load()
    out = {}

    def hook(ns):
        out["name"] = R.wgrad_name(lib, ns["mk"]("gpu")[0]._obj)
        out["dw"] = ns["dw"].get("gpu").clone()
        if selftest:
            _wgrad_wrong_references(ns)
    with _opts(opts):
        with (K.exact_mode() if exact else contextlib.nullcontext()):
            K._run_wgrad_case(case, dt, cdt=cdt, hook=hook)
    return out


@pytest.mark.parametrize("e", WGRAD_LEDGER, ids=[e.key for e in WGRAD_LEDGER])
def test_wgrad_ledger(e):
    lib = L.load()
    with _opts(e.opts):
        assert R.wgrad_name(lib, R.wgrad_desc(e.case, e.dt, e.cdt)) == e.name
    out = _probe_wgrad(e.case, e.opts, e.dt, e.cdt, exact=True, selftest=True)
    assert out["name"] == e.name
    assert _probe_wgrad(e.case, e.opts, e.dt, e.cdt, exact=False)["name"] == e.name


# ====================================================================================================================
# 3. the option sweep: one row per option of options.h (tests/test_route_tables.py fails on an option without a row)
# ====================================================================================================================
def _is_wgrad(case):      # (weight-gradient cases carry their pending affine as element 7, conv cases their extras dict)
    return not isinstance(case[7], dict)


def _sweep(option, values, cases, base=None, claim=None, note=""):
    """cases: [(case, dt, cdt)] or [(case, dt, cdt, options of this case beside `base`)], conv and weight-gradient cases alike; claim: the routing answer that must differ from the default's ("name", "tile_m", "stats_rows",
    "splitk_bytes"), None where the option changes the grid or the order only"""
    return dict(kind="sweep", option=option, values=values, cases=cases, base=dict(base or {}), claim=claim, note=note)


def _exempt(reason, test=None):
    return dict(kind="exempt", reason=reason, test=test)


def _bf(*cases):
    return [(c, BF16, None) for c in cases]


_HT_BIG = ("o_ht_16x32", (4, 24, 16, 32), 64, 192) + SP3 + (dict(tline=5, stats=True),)           # 384 halo tiles at H x W = 512 < ht_minhw
_HT_BIG_PRE = ("o_ht_16x32_pre", (4, 24, 16, 32), 64, 192) + SP3 + (dict(tline=5, pre=True),)
_HTT_BIG = ("o_htt_8x8", (48, 16, 8, 8), 64, 192) + T3 + (dict(tline=True, stats=True),)          # 384 temporal tiles at H x W = 64 < ht_t_minhw
_PW_BIG = ("o_pw_m131072", BIG, 96, 192) + PW1 + (dict(tline=6, stats=True),)                     # two 96-column tiles of the pointwise kernel
_PP_PW = ("o_pp_pw", (1, 4, 64, 64), 64, 480) + PW1 + ({},)                                       # one K tile of 64, 128 tiles of 256 x 256
_N64_MID = ("o_n64_m65536", (1, 4, 128, 128), 32, 64) + PW1 + (dict(stats=True),)
_N128_MID = ("o_n128_m65536", (1, 4, 128, 128), 32, 128) + PW1 + (dict(stats=True),)
_TPERM = [("o_tperm_n32", (3, 3, 16, 16), 64, 32) + T3 + (dict(stats=True),), ("o_tperm_n48", (2, 3, 16, 32), 32, 48) + SP3 + (dict(pre=True),),
          ("o_tperm_n48_b1", (1, 3, 16, 16), 64, 48) + T3 + ({},)]
_TS_SEGS = [_case(K.CONV_TS_CASES, "ts_segs_k7s2", tline=True), _case(K.CONV_TS_CASES, "ts_segs_acc", tline=True),
            ("o_ts_segs_min", (1, 8, 8, 8), 64, 64) + T3 + (dict(tline=True, stats=True),)]
_DMA_SMALL = [DMA_TILES[2][2], DMA_TILES[3][3], DMA_TILES[4][3]]

OPTION_ROWS = {
    "dma": _sweep("dma", [0], _bf(*_DMA_SMALL), LADDER, "name"),
    "dma3": _sweep("dma3", [0], [(_case(K.CONV_CASES, "sp_3x3"), F32, F32S), (_case(K.CONV_CASES, "tm_3x1"), F32, F32S)], {}, "name"),
    "pp": _exempt("swept", "test_conv3d_pingpong"),
    "pp_pw_kt": _sweep("pp_pw_kt", [1, 2], _bf(_PP_PW), {}, "name@1", note="threshold lowered to the case's one K tile: 1 takes conv_pp, 2 (and the default 8) does not"),
    "pw": _exempt("swept", "test_conv3d_pointwise_stream"),
    "pw_maxtn": _sweep("pw_maxtn", [1, 2], _bf(_PW_BIG), {}, "name@1", note="the heuristic's M >= 131072 is no option: the case has two column tiles, 1 refuses them, 2 (and the default 4) takes them"),
    "ht": _exempt("swept", "test_conv3d_halo_tile"),
    "ht3": _exempt("swept", "test_conv3d_halo_tile_split_bf16"),
    "ht_minhw": _sweep("ht_minhw", [512, 513], _bf(_HT_BIG), {}, "name@512", note="threshold lowered to the case's 16 x 32: 512 takes the halo tiles, 513 (and the default) does not"),
    "ht_t": _sweep("ht_t", [0], _bf(_HTT_BIG), dict(ht_t_minhw=64), "name"),
    "ht_t_minhw": _sweep("ht_t_minhw", [64, 65], _bf(_HTT_BIG), {}, "name@64", note="threshold lowered to the case's 8 x 8"),
    "ht_pre": _sweep("ht_pre", [1], _bf(_HT_BIG_PRE), dict(ht_minhw=512), "name"),
    "conv_hs": _exempt("swept", "test_stem_folded"),
    "conv_hs_segs": dict(kind="custom", test="test_option_conv_hs_segs"),
    "conv_ts": _exempt("swept", "test_conv3d_tstream"),
    "conv_ts_segs": _sweep("conv_ts_segs", [0], _bf(*_TS_SEGS), dict(conv_ts=2), "stats_rows"),
    "splitk": _exempt("swept", "test_conv3d_splitk"),
    "sk_tile": _sweep("sk_tile", [0, 1, 2, 4, 8], _bf(_case(K.SPLITK_CASES, "sk_tile192", splitk=True), _case(K.SPLITK_CASES, "sk_tile128", splitk=True),
                                                      ("sk_n64_m4096", (1, 1, 64, 64), 352, 64) + SP3 + (dict(act=1, splitk=True),)), LADDER, "any",
                      note="every case changes its tile for at least one value (which value: the ledger's sk_tile entries)"),
    "n64_tile": _sweep("n64_tile", [1, 2], _bf(DMA_TILES[3][2], _N64_MID), LADDER, "any", note="1 moves the small case off 64 x 64, 2 the 65536-row case off 128 x 64"),
    "n64_kmax": _exempt("gated by M >= 2^20 rows, which no option lowers: a launch would need a tensor eight times the largest of this suite.  The route "
                        "flips on either side of the threshold in tests/test_route_tables.py::test_n64_kmax_flips_the_tile_on_the_host (no launch); "
                        "the tile it selects runs as conv_dma_kernel<4,2,2,2,3,*> in the ledger"),
    "n128_tile": _sweep("n128_tile", [1, 2], _bf(DMA_TILES[4][2], _N128_MID), LADDER, "any"),
    "n128_kmax": _sweep("n128_kmax", [0, 1], _bf(DMA_TILES[10][2]), LADDER, "name@0", note="1 K step: 1 (and the default 64) takes 128 x 128, 0 takes 256 x 128"),
    "n192_tile": _exempt("swept", "test_conv3d_n192_tile"),
    # conv: fill_args (256-row tiles, oT > 1, oH x oW % 256 == 0); weight gradients: the K-tile order of the ping-pong kernel (wgrad_pp.hip:436,
    # To > 1, Ho x Wo % 64 == 0; both row tiles) and of the LDS-DMA kernel (wgrad_dma.hip:374, Ho x Wo % 32 == 0; one and three taps per group)
    "tperm": _sweep("tperm", [1], _bf(*_TPERM) + [(_wcase(K.WGRAD_PP_CASES, "pp_bigm"), BF16, None, dict(wgrad_pp=3)), (_wcase(K.WGRAD_PP_CASES, "pp_bigm"), BF16, None, dict(wgrad_pp=4)),
                                                 (("o_tperm_wpp_3t", (2, 5, 8, 8), 96, 128) + T3 + (True, {}), BF16, None, dict(wgrad_pp=3)),
                                                 (_wcase(K.WGRAD_PP_CASES, "pp_bigm"), BF16, None, dict(wgrad_pp=0)), (_wcase(K.WGRAD_CASES, "splitk"), BF16, None, dict(wgrad_pp=0))],
                    LADDER, None),
    "bnb_epi": dict(kind="custom", test="test_option_bnb_epi_off_refuses_the_launch"),
    "wgrad_dma": _sweep("wgrad_dma", [0], _bf(*K.WGRAD_CASES), {}, "name"),
    "wgrad_tg": _exempt("swept: every (tile, taps per group) of the launch table", "test_wgrad_ledger"),
    "wgrad_tr": _sweep("wgrad_tr", [0], _bf(*K.WGRAD_CASES[:4]), dict(wgrad_dma=0), None),
    "wgrad_pp": _exempt("swept", "test_conv3d_wgrad_pingpong"),
    "wgrad_pp_cap": _sweep("wgrad_pp_cap", [0], _bf(_wcase(K.WGRAD_PP_CASES, "pp_bigm", max_cus=8), _wcase(K.WGRAD_PP_CASES, "pp_bigm", max_cus=0)), dict(wgrad_pp=3), None),
    "wgrad_ts": _exempt("swept", "test_conv3d_wgrad_tstream"),
    "wgrad_ts_cap": _sweep("wgrad_ts_cap", [1], _bf(_wcase(K.WGRAD_TS_CASES, "ts_k7s2_long", tline=True, max_cus=8), _wcase(K.WGRAD_TS_CASES, "ts_k7s2_long", tline=True, max_cus=0)),
                           dict(wgrad_ts=2), None),
    "wgrad_hs": _exempt("swept", "test_stem_folded"),
    "wgrad_rs": _exempt("swept", "test_conv3d_wgrad_rowstream"),
    "wgrad_rs4": _sweep("wgrad_rs4", [0], _bf(*[_wcase(K.WGRAD_RS_CASES, n, tline=4) for n in RS_48]), dict(wgrad_rs=2), "name"),
    "wgrad_tf": _exempt("swept", "test_conv3d_wgrad_tframes"),
    "wgrad_skinny": _exempt("swept", "test_conv3d_wgrad_skinny"),
    "bn_lean": dict(kind="custom", test="test_option_bn_reductions", values=[0]),
    "bn_rows": dict(kind="custom", test="test_option_bn_reductions", values=[1, 7]),
    "reduce_il": dict(kind="custom", test="test_option_bn_reductions", values=[0]),
    "reduce_small": dict(kind="custom", test="test_option_bn_reductions", values=[0]),
    "pack_tiled": _exempt("swept", "test_pack_weights_multi_matches_single_packs"),
    "pool_lds": _exempt("swept, the kernel asserted by name; every value's route: tests/route_cases.py POOL_TABLE", "test_maxpool_k3s1_lds_forward"),
    "pool_pk": _exempt("swept, the kernel asserted by name; every value's route: tests/route_cases.py POOL_TABLE", "test_maxpool_k3s1_lds_forward_bf16_fp32_compare"),
    "pool_twalk": _exempt("swept, the kernel asserted by name; every value's route: tests/route_cases.py POOL_TABLE", "test_maxpool_k3s1_twalk_backward"),
    "pool_blk": _exempt("swept, the kernel asserted by name; every value's route: tests/route_cases.py POOL_TABLE", "test_maxpool_133s2_generic_backward"),
    "up_blk": _exempt("swept", "test_upsample_quad_kernels"),
    "auc_ws": _exempt("swept", "test_lds_route_and_workspace_route_agree_bit_for_bit"),
    "sauc_ws": _exempt("swept", "test_lds_route_and_workspace_route_agree_bit_for_bit"),
}
SWEEPS = [(n, i) for n, r in OPTION_ROWS.items() if r["kind"] == "sweep" for i in range(len(r["cases"]))]


def _same(a, b, what):
    assert a.dtype == b.dtype and torch.equal(a, b), "%s: results differ between option values (%d elements)" % (what, int((a.float() != b.float()).sum()))


def _sweep_id(n, i):
    c = OPTION_ROWS[n]["cases"][i]
    more = "".join("-%s%d" % kv for kv in sorted(c[3].items())) if len(c) > 3 else ""
    return "%s-%s%s%s" % (n, c[0][0], "-cus%d" % c[0][8]["max_cus"] if _is_wgrad(c[0]) and len(c[0]) > 8 and "max_cus" in c[0][8] else "", more)


@pytest.mark.parametrize("option,i", SWEEPS, ids=[_sweep_id(n, i) for n, i in SWEEPS])
def test_option_sweep(option, i):
    """exact-arithmetic inputs at the default and at every value: each equals the ABI model (the case runner) and they equal each other
    bit for bit; statistics agree after folding their rows in float64; the route changes where the row says so"""
    row = OPTION_ROWS[option]
    case, dt, cdt = row["cases"][i][:3]
    base_opts = dict(row["base"], **(row["cases"][i][3] if len(row["cases"][i]) > 3 else {}))
    tol = 1e-4 if cdt == F32S else None
    wgrad = _is_wgrad(case)
    if wgrad:
        run = lambda o: _probe_wgrad(case, o, dt, cdt)
    else:
        run = lambda o: _probe_conv(case, o, dt, cdt, tol)
    base = run(base_opts)
    changed = []
    for v in row["values"]:
        got = run(dict(base_opts, **{option: v}))
        what = "%s=%d on %s" % (option, v, case[0])
        if wgrad:
            _same(got["dw"], base["dw"], what)
            changed.append(got["name"] != base["name"])
            continue
        _same(got["y"], base["y"], what)
        if base["stats"] is not None:
            K._cmp(got["stats"], base["stats"], 1e-4 if dt == F32 else 2e-2, "conv stats " + what)
        gi, bi = got["info"], base["info"]
        changed.append(any(gi[k] != bi[k] for k in ("name", "tile_m", "stats_rows", "splitk_bytes")) if row["claim"] in ("any", None)
                       else gi[row["claim"].split("@")[0]] != bi[row["claim"].split("@")[0]])
    claim = row["claim"]
    if claim is None:
        return
    if claim == "any":
        assert any(changed), "%s: no value changed the route of %s" % (option, case[0])
    elif "@" in claim:      # a threshold: the named value flips the route, the value on the other side of the threshold does not
        flip = row["values"].index(int(claim.split("@")[1]))
        assert changed[flip] and not any(c for j, c in enumerate(changed) if j != flip), "%s: route changes %s for values %s" % (option, changed, row["values"])
    else:
        assert all(changed), "%s: %s did not change for %s (values %s: %s)" % (option, claim, case[0], row["values"], changed)


def test_option_bnb_epi_off_refuses_the_launch():
    """bnb_epi = 0: the rows query answers 0 and a conv with bnb_partials set is refused with a message -- not launched"""
    lib = L.load()
    seen = []

    def refuse(ns, out):
        assert lib.vinet_set_option(b"bnb_epi", 0) == 0
        try:
            args = ns["mk"]("gpu")
            assert lib.vinet_conv3d_bn_bwd_stats_rows(args[0]) == 0
            before = ns["yp"].get("gpu").clone()
            rc = lib.vinet_conv3d(*args)
            torch.cuda.synchronize()
            assert rc != 0 and b"bnb" in lib.vinet_last_error(), (rc, lib.vinet_last_error())
            assert torch.equal(ns["yp"].get("gpu"), before), "the refused launch wrote y"
            seen.append(out["info"]["name"])
        finally:
            lib.vinet_set_option(b"bnb_epi", 1)
    for cn in ("bnb_ht_64_64", "bnb_pw_64_48"):
        c = _case(K.BNB_CASES, cn)
        ht = cn.startswith("bnb_ht")
        if ht:
            c = c[:7] + (dict(c[7], tline=5),)
        out = _probe_conv(c, dict(ht=2 if ht else 0, pw=0, pp=0), more=refuse)
        assert out["info"]["bnb_rows"] > 0
    assert len(seen) == 2 and seen[0].startswith("conv_ht_kernel<") and seen[1].startswith("conv_dma_kernel<")


def test_option_conv_hs_segs():
    """conv_hs_segs = 0: whole strips only -- fewer statistics rows, the same folded-stem results (tests.test_gpu_kernels.test_stem_folded
    on exact-arithmetic inputs, on the smallest image with two row segments and on the one with a ragged fourth)"""
    lib = L.load()
    for hw in ((28, 128), (60, 128)):
        d = R.folded_stem_desc(2, 3, hw)
        with _opts(dict(conv_hs=2)):
            assert R.conv_name(lib, d) == "conv_hs_kernel"
            rows = lib.vinet_conv3d_stats_rows(C.byref(d))
            with _opts(dict(conv_hs_segs=0)):
                rows0 = lib.vinet_conv3d_stats_rows(C.byref(d))
        assert rows0 == 2 * 3 * (hw[1] // 2 // 64) and rows == rows0 * (2 if hw[0] == 28 else 4), (rows0, rows)
        for v in (1, 0):
            with _opts(dict(conv_hs_segs=v)):
                with K.exact_mode():
                    K.test_stem_folded(BF16, hw)


BN_CHANNELS = [16, 24, 64, 208, 528, 1024]
BN_OPTION_VALUES = [(n, v) for n in ("bn_lean", "bn_rows", "reduce_il", "reduce_small") for v in OPTION_ROWS[n]["values"]]


def _bn_reduce_case(dt, Cc, shape, exact):
    """vinet_channel_stats and vinet_bn_bwd_reduce with the rows the library answers under the current options, against the ABI
    model's float64 sums after folding the rows in float64 (the tolerances of test_bn_kernels; equality on exact-arithmetic inputs)"""
    lib = L.load()
    B, T, H, W = shape
    with (K.exact_mode() if exact else contextlib.nullcontext()):
        xp, xmk = K.view_pair(B, T, H, W, Cc, dt, "rbx", 1, ld=Cc + 8, c_off=8)
        gp, gmk = K.view_pair(B, T, H, W, Cc, dt, "rbg", 2)
        sc, sh = K.fvec("rbs", Cc, 3, 0.5, 1.5), K.fvec("rbh", Cc, 4)
        mean, istd = K.fvec("rbm", Cc, 5), K.fvec("rbi", Cc, 6, 0.5, 2.0)
    rows = lib.vinet_stats_rows(C.byref(xmk("gpu").ct()))
    rmax = max(rows, AbiEmulator().vinet_stats_rows(xmk("cpu").ct()))
    outs = []
    for fn, mk, tol in (("vinet_channel_stats", lambda s, p: [C.byref(xmk(s).ct()), dt, p.ptr(s), K._stream() if s == "gpu" else 0], 1e-5),
                        ("vinet_bn_bwd_reduce", lambda s, p: [C.byref(gmk(s).ct()), C.byref(xmk(s).ct()), dt, L.CAffine(sc.ptr(s), sh.ptr(s), 1), mean.ptr(s), istd.ptr(s),
                                                              p.ptr(s), K._stream() if s == "gpu" else 0], 2e-5)):
        part = K.Pair(torch.full((rmax * 2 * Cc,), float("nan")))
        K.run_both(fn, lambda s: mk(s, part))
        got = part.get("gpu")[:rows * 2 * Cc].view(rows, 2, Cc).double().sum(0)
        ref = part.get("cpu").view(rmax, 2, Cc)[:1].double().sum(0)      # (the model writes its float64 sums into row 0)
        assert torch.isfinite(got).all(), "%s: unwritten rows" % fn
        if exact:
            assert torch.equal(got, ref), "%s: sums of exact-arithmetic inputs differ by %g" % (fn, float((got - ref).abs().max()))
        else:
            K._cmp(got, ref, tol, fn)
        outs.append(got)
    return rows, outs


@pytest.mark.parametrize("option,value", BN_OPTION_VALUES, ids=["%s=%d" % nv for nv in BN_OPTION_VALUES])
def test_option_bn_reductions(option, value):
    """bn_lean = 0 (the generic BatchNorm-backward forms), reduce_il = 0 (contiguous windows), reduce_small = 0, bn_rows = 1 / 7: the
    channel counts of test_bn_kernels, bf16 and fp32, on its 210-voxel tensor and on a 35-voxel one (channel_reduce_small_kernel's),
    then test_bn_kernels and test_bn_partials_fold themselves under the option"""
    lib = L.load()
    for shape in ((2, 3, 5, 7), (1, 1, 5, 7)):
        x = L.CTensor(R._P, shape[0], shape[1], shape[2], shape[3], 16, 16, shape[1] * shape[2] * shape[3] * 16)
        rows_default = lib.vinet_stats_rows(C.byref(x))
        for dt in K.DTS:
            for Cc in BN_CHANNELS:
                for exact in (True, False):
                    r0, base = _bn_reduce_case(dt, Cc, shape, exact)
                    assert r0 == rows_default
                    with _opts({option: value}):
                        r1, got = _bn_reduce_case(dt, Cc, shape, exact)
                    if option == "bn_rows":
                        assert r1 == min(rows_default, value), "bn_rows = %d: %d rows" % (value, r1)
                    for a, b in zip(got, base):
                        if exact:
                            assert torch.equal(a, b)
    if option != "bn_rows":      # (test_bn_kernels sizes its tables by the model's row count: the header's bn_rows)
        with _opts({option: value}):
            for dt in K.DTS:
                for Cc in BN_CHANNELS:
                    K.test_bn_kernels(dt, Cc)
    with _opts({option: value}):
        for rows, Cc, out_rows in [(5000, 64, 256), (4097, 176, 256), (300, 24, 7), (64, 832, 64)]:
            K.test_bn_partials_fold(rows, Cc, out_rows)
