"""Descriptors of the kernel-suite cases WITHOUT tensors: the routing queries of libvinet_hip.so (kernel name, tile_m, stats rows,
split-K bytes) are pure host code, so the ledgers of tests/test_gpu_routes.py can be checked against the library on a machine
without a GPU (tests/test_route_tables.py) before the same cases run on one."""
import ctypes as C
import re

from vinet_amd import _lib as L
from vinet_amd import engine as E

_P = 0x10000      # a 16-byte aligned stand-in for every pointer the route only tests for null / alignment


def _ct(B, T, H, W, Cc, ld, t_total, es, c_off=0, t_off=0):
    ld = Cc if ld is None else ld
    tt = T if t_total is None else t_total
    return L.CTensor(_P + (t_off * H * W * ld + c_off) * es, B, T, H, W, Cc, ld, tt * H * W * ld)


def conv_desc(case, dt, cdt=None):
    """the VinetConvDesc tests.test_gpu_kernels._run_conv_case builds for `case`, shape fields only (a mirror of that runner's mk():
    change them together -- tests/test_gpu_routes.py asserts the kernel name from both)"""
    name, (B, T, H, W), Cin, N, k, s, p, ex = case
    oT, oH, oW = [(d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip((T, H, W), k, s, p)]
    head = ex.get("head", False)
    Ny = E.EG[dt] if head else N
    odt = E.F32 if ex.get("out_f32") else dt
    omT, ooT = ex.get("om", (1, 0))
    d = L.CConvDesc()
    d.dtype, d.out_dtype, d.mode = (dt if cdt is None else cdt), odt, 0
    d.x = _ct(B, T, H, W, Cin, ex.get("in_ld"), ex.get("in_ttotal"), E.ESIZE[dt], ex.get("in_coff", 0), ex.get("in_toff", 0))
    d.y = _ct(B, oT * omT, oH, oW, Ny, ex.get("out_ld"), ex.get("out_ttotal"), E.ESIZE[odt], ex.get("out_coff", 0), ex.get("out_toff", 0))
    d.oT, d.oH, d.oW = oT, oH, oW
    d.sT, d.sH, d.sW = s
    d.omT = d.omH = d.omW = 1
    d.ntaps, d.taps, d.w, d.Kp = k[0] * k[1] * k[2], _P, _P, E.rup(Cin, 32)
    pre = ex.get("pre")
    d.pre = L.CAffine(None, None, 1) if pre == "relu" else (L.CAffine(_P, _P, 0 if pre == "affine" else 1) if pre else L.CAffine(None, None, 0))
    d.out_scale = _P if ex.get("epi") else None
    d.out_shift = _P if (ex.get("epi") or ex.get("epi_shift")) else None
    d.act = ex.get("act", 0)
    d.accumulate = 1 if ex.get("accumulate") else 0
    d.stats = _P if ex.get("stats") else None
    d.n_valid = N if head else 0
    if ex.get("tline"):
        d.tline, d.tpad = (1 if ex["tline"] is True else ex["tline"]), p[0]
    if ex.get("om"):
        d.omT, d.ooT = ex["om"]
    bnb = ex.get("bnb")
    if bnb is not None:
        z = _ct(B, oT, oH, oW, Ny, bnb.get("ld"), None, E.ESIZE[odt], bnb.get("coff", 0))
        d.bnb_z, d.bnb_ld, d.bnb_sB = z.ptr, z.ld, z.sB
        d.bnb_fwd = L.CAffine(_P, _P, 1 if bnb.get("relu", True) else 0)
        d.bnb_mean, d.bnb_invstd, d.bnb_partials = _P, _P, _P
    if ex.get("splitk"):
        d.splitk_ws, d.splitk_ws_bytes = _P, 1 << 40
    return d


def wgrad_desc(case, dt, cdt=None):
    """the VinetWgradDesc of tests.test_gpu_kernels._run_wgrad_case, shape fields only (a mirror of that runner's mk(): change them together)"""
    name, (B, T, H, W), Cin, N, k, s, p, pre = case[:8]
    ex = case[8] if len(case) > 8 else {}
    oT, oH, oW = [(d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip((T, H, W), k, s, p)]
    d = L.CWgradDesc()
    d.dtype, d.mode = (dt if cdt is None else cdt), 0
    d.x = _ct(B, T, H, W, Cin, ex.get("x_ld"), None, E.ESIZE[dt], ex.get("x_coff", 0))
    d.dy = _ct(B, oT, oH, oW, N, ex.get("dy_ld"), None, E.ESIZE[dt], ex.get("dy_coff", 0))
    d.sT, d.sH, d.sW = s
    d.ntaps, d.taps, d.dw, d.Kp = k[0] * k[1] * k[2], _P, _P, E.rup(Cin, 32)
    d.pre = L.CAffine(None, None, 1) if pre == "relu" else (L.CAffine(_P, _P, 0 if pre == "affine" else 1) if pre else L.CAffine(None, None, 0))
    if ex.get("tline"):
        d.tline, d.tpad = (1 if ex["tline"] is True else ex["tline"]), p[0]
    d.max_cus = ex.get("max_cus", 0)
    return d


def conv_name(lib, d):
    buf = C.create_string_buffer(128)
    assert lib.vinet_conv3d_kernel_name(C.byref(d), buf, 128) == 0
    return buf.value.decode()


def wgrad_name(lib, d):
    buf = C.create_string_buffer(128)
    assert lib.vinet_conv3d_wgrad_kernel_name(C.byref(d), buf, 128) == 0
    return buf.value.decode()


def pool_args(ksp, dt, dims, chan, pre="affine_relu", am="ok"):
    """(descriptor, x, pre, y, argmax) as tests.test_gpu_kernels.test_maxpool builds them, without tensors: x (and dx) a channel slice
    (C, ld, c_off) of a wider buffer, y (and dy) dense unless a fourth element of `chan` gives its ld"""
    k, s, p = ksp
    B, T, H, W = dims
    Cc, ld, c_off, y_ld = (tuple(chan) + (None,))[:4]
    oT, oH, oW = [(d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip((T, H, W), k, s, p)]
    x = _ct(B, T, H, W, Cc, ld, None, E.ESIZE[dt], c_off)
    y = _ct(B, oT, oH, oW, Cc, y_ld, None, E.ESIZE[dt])
    aff = {"none": L.CAffine(None, None, 0), "relu": L.CAffine(None, None, 1), "affine_relu": L.CAffine(_P, _P, 1), "scale_only": L.CAffine(_P, None, 1)}[pre]
    return L.CPoolDesc(dt, *(k + s + p)), x, aff, y, {"ok": _P, "null": None, "+4": _P + 4}[am]


def pool_names(lib, d, x, pre, y, argmax):
    """(forward, backward) kernel of vinet_maxpool3d(d, x, pre, y, argmax) and vinet_maxpool3d_bwd(d, dy = y's view, argmax, dx = x's view);
    None where the library rejects the arguments (the backward without an argmax)"""
    buf = C.create_string_buffer(128)
    fwd = buf.value.decode() if lib.vinet_maxpool3d_kernel_name(C.byref(d), C.byref(x), pre, C.byref(y), argmax, buf, 128) == 0 else None
    bwd = buf.value.decode() if lib.vinet_maxpool3d_bwd_kernel_name(C.byref(d), C.byref(y), argmax, C.byref(x), buf, 128) == 0 else None
    return fwd, bwd


def option_defaults(path):
    """{name: default} out of options.h (the defaults are integer expressions: `28 * 48`)"""
    out = {}
    for m in re.finditer(r"VN_OPT\(\s*(\w+)\s*,\s*([^,]+?)\s*,\s*\"", open(path).read()):
        if m.group(1) != "name":
            v = 1
            for f in m.group(2).split("*"):
                v *= int(f)
            out[m.group(1)] = v
    return out


class options:
    """`with options(lib, dict)`: set, then back to the header's defaults whatever happens"""

    def __init__(self, lib, opts, defaults):
        self.lib, self.opts, self.defaults = lib, opts, defaults

    def __enter__(self):
        for k, v in self.opts.items():
            assert self.lib.vinet_set_option(k.encode(), v) == 0, (k, v, self.lib.vinet_last_error())
        return self

    def __exit__(self, *a):
        for k in self.opts:
            self.lib.vinet_set_option(k.encode(), self.defaults[k])
        return False


def stem_desc(dt):
    """the stem-mode descriptor of tests.test_gpu_kernels.test_conv3d_stem_mode"""
    d = L.CConvDesc()
    d.dtype, d.out_dtype, d.mode = dt, dt, 1
    d.x = _ct(2, 3, 18, 22, 4, None, None, E.ESIZE[dt])
    d.y = _ct(2, 3, 9, 11, 64, None, None, E.ESIZE[dt])
    d.oT, d.oH, d.oW = 3, 9, 11
    d.sT, d.sH, d.sW = 1, 2, 2
    d.omT = d.omH = d.omW = 1
    d.ntaps, d.taps, d.w, d.Kp = 7, _P, _P, 32
    return d


def folded_stem_desc(B, T, hw, dt=None):
    """the folded stem of tests.test_gpu_kernels.test_stem_folded as the strip kernel sees it (tline = 2)"""
    dt = E.BF16 if dt is None else dt
    H, W = hw
    Hp, Wp = H + 6, W + 8 + (W & 1)
    oH, oW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = L.CConvDesc()
    d.dtype, d.out_dtype, d.mode = dt, dt, 0
    d.x = L.CTensor(_P, B, T, Hp, Wp // 2, 32, 8, T * Hp * Wp * 4)
    d.y = _ct(B, T, oH, oW, 64, None, None, E.ESIZE[dt])
    d.oT, d.oH, d.oW = T, oH, oW
    d.sT, d.sH, d.sW = 1, 2, 1
    d.omT = d.omH = d.omW = 1
    d.ntaps, d.taps, d.w, d.Kp, d.tline = 7, _P, _P, 32, 2
    d.stats = _P
    return d


# ---- which case reaches which instantiation (checked against the library's routing by tests/test_route_tables.py) ----
NATURAL_IGEMM = {"pw_pre_stats": "conv_igemm_kernel<bf16,4,3,4,1,0>", "sp_3x3": "conv_igemm_kernel<bf16,2,4,2,2,0>", "cin24": "conv_igemm_kernel<bf16,2,2,2,2,0>",
                 "concat_slice_out": "conv_igemm_kernel<bf16,4,2,4,1,0>", "xslice_pre": "conv_igemm_kernel<bf16,2,4,2,2,0>"}
HT_BF16 = {      # vinet_launch_conv_ht_bf16, conv_bf16.hip:39-56
    "conv_ht_kernel<64,t,plain>": "r_htt_64", "conv_ht_kernel<64,t,pre>": "htt_pre_128", "conv_ht_kernel<96,t,plain>": "htt_192", "conv_ht_kernel<96,t,pre>": "htt_pre_cin160",
    "conv_ht_kernel<64,32,pre>": "r_ht_pre_64_32", "conv_ht_kernel<96,32,pre>": "ht_pre_64_96", "conv_ht_kernel<64,16,pre>": "ht_pre_tw16_cin96", "conv_ht_kernel<96,16,pre>": "r_ht_pre_96_16",
    "conv_ht_kernel<32,32>": "ht_cin24_n32", "conv_ht_kernel<64,32>": "ht_192_64_5t", "conv_ht_kernel<96,32>": "ht_64_192",
    "conv_ht_kernel<32,16>": "r_ht_32_16", "conv_ht_kernel<64,16>": "ht_tw16_rows20", "conv_ht_kernel<96,16>": "ht_tw16_w48"}
HT_F32S = {      # vinet_launch_conv_ht_f32s, conv_f32.hip:27-42
    "conv_ht3_kernel<64,t,plain>": "htt_192", "conv_ht3_kernel<64,t,pre>": "htt_pre_128", "conv_ht3_kernel<32,t,plain>": "htt_acc_slices", "conv_ht3_kernel<32,t,pre>": "htt_pre_cin160",
    "conv_ht3_kernel<64,32,pre>": "ht_pre_slices", "conv_ht3_kernel<32,32,pre>": "ht_pre_64_96", "conv_ht3_kernel<64,16,pre>": "ht_pre_tw16_cin96", "conv_ht3_kernel<32,16,pre>": "r_ht_pre_32_16",
    "conv_ht3_kernel<32,32>": "ht_cin24_n32", "conv_ht3_kernel<64,32>": "ht_64_192", "conv_ht3_kernel<32,16>": "r_ht_32_16", "conv_ht3_kernel<64,16>": "ht_tw16_rows20"}
HT_BNB = {       # vinet_launch_conv_ht_bnb, conv_bnb.hip:20-32
    "conv_ht_kernel<64,t,plain>": "bnb_htt_64", "conv_ht_kernel<96,t,plain>": "bnb_htt_192", "conv_ht_kernel<32,32>": "bnb_ht_64_32", "conv_ht_kernel<64,32>": "bnb_ht_64_64",
    "conv_ht_kernel<96,32>": "bnb_ht_acc_192", "conv_ht_kernel<32,16>": "r_bnb_ht_32_16", "conv_ht_kernel<64,16>": "r_bnb_ht_64_16", "conv_ht_kernel<96,16>": "bnb_ht_128_96_tw16"}
PW = {           # vinet_launch_conv_pw_bf16, conv_bf16.hip:62-66
    "conv_pw_kernel<32,plain>": "pw_32_32", "conv_pw_kernel<32,pre>": "r_pw_32_pre", "conv_pw_kernel<64,plain>": "pw_64_64_relu", "conv_pw_kernel<64,pre>": "pw_cin40_n40_pre",
    "conv_pw_kernel<96,plain>": "pw_cin176_relu", "conv_pw_kernel<96,pre>": "pw_192_176_slices"}

_TILES = ["4,8,4,1", "4,6,4,1", "4,4,4,1", "4,3,4,1", "4,2,4,1", "4,1,4,1", "4,4,2,2", "4,2,2,2", "2,4,2,2", "2,2,2,2", "4,6,2,2"]
# Every conv instantiation of the launch tables, counted by hand (tests/test_route_tables.py counts the sources again):
#   conv_bf16.hip  56 = 1 stem (:12) + 11 CASE (:13-14) + 11 DMA_CASE x plain / pre (:26-27) + 2 conv_pp (:34) + 14 conv_ht (:41-55) + 6 conv_pw (:64-66)
#   conv_f32.hip   32 = 2 stem (:13) + 7 CASE x float / split (:14-15) + 4 conv_dma3 (:22-23) + 12 conv_ht3 (:29-41)
#   conv_bnb.hip   19 = 11 DMA_BNB_CASE (:14-15) + 8 conv_ht (:22-31)
CONV_INSTANTIATION_COUNTS = {"conv_bf16.hip": 56, "conv_f32.hip": 32, "conv_bnb.hip": 19}
CONV_INSTANTIATIONS_RUN = (
    ["conv_igemm_kernel<bf16,4,4,4,1,1>", "conv_igemm_kernel<float,2,4,4,1,1>", "conv_pp_kernel<256>", "conv_pp_kernel<192>"] +
    ["conv_igemm_kernel<bf16,%s,0>" % t for t in _TILES] +
    ["conv_dma_kernel<%s,3,%s>%s" % (t, f, b) for t in _TILES for f, b in (("plain", ""), ("pre", ""), ("plain", " [bnb]"))] +
    ["conv_igemm_kernel<%s,2,%d,4,1,0>" % (a, nt) for a in ("float", "float/split") for nt in (8, 6, 4, 3, 2, 1)] +
    ["conv_dma3_kernel<%d,3,%s>" % (n, f) for n in (32, 64) for f in ("plain", "pre")] +
    list(HT_BF16) + list(HT_F32S) + [n + " [bnb]" for n in HT_BNB] + list(PW))
CONV_INSTANTIATIONS_NOT_RUN = {
    "conv_igemm_kernel<float/split,2,4,4,1,1>": "conv_f32.hip:13, the stem form of the split-bf16 arithmetic: the case runners have no hi / lo stem pack (the engine folds the stem "
                                                "into a generic conv for this arithmetic; tests.test_gpu_kernels.test_stem_folded runs that)",
    "conv_igemm_kernel<float,2,2,2,2,0>": "conv_f32.hip:15, unreachable: vinet_pick_conv_tile returns {2, nt, 4, 1} for fp32 tensors",
    "conv_igemm_kernel<float/split,2,2,2,2,0>": "conv_f32.hip:15, unreachable for the same reason",
}
# wgrad_dma.hip:383-387: (64,32,7) plain + WG(64, tg) x plain / pre for tg = 1, 2, 3, 7, 9 = 11 reachable; WG(128, 1, 3) (two more) is
# unreachable -- wg_pick (wgrad_dma.hip:342) only ever answers tn = 64
WGRAD_NAMES_RUN = (["conv_wgrad_rs_kernel<W%d,4w>" % w for w in (24, 48, 32, 64, 96)] + ["conv_wgrad_rs_kernel<W%d,8w>" % w for w in (24, 48, 32, 64, 96, 128, 160, 192)] +
                   ["conv_wgrad_kernel<bf16,0>", "conv_wgrad_kernel<float/split,0>", "conv_wgrad_kernel<float,0>", "conv_wgrad_dma_kernel<64,32,7,plain>"] +
                   ["conv_wgrad_dma_kernel<64,64,%d,%s>" % (tg, f) for tg in (1, 2, 3, 7, 9) for f in ("plain", "pre")])
WGRAD_NAMES_NOT_RUN = {"conv_wgrad_dma_kernel<128,128,1,plain>": "wgrad_dma.hip:387, unreachable: wg_pick never answers a 128-row tile",
                       "conv_wgrad_dma_kernel<128,128,1,pre>": "wgrad_dma.hip:387, unreachable for the same reason"}


# ---- max-pool routes (pool.hip: pool_fwd_route / pool_bwd_route) ----
# (key, pool, dtype, (B, T, H, W), (C, ld, c_off[, ld of y]), pre, argmax, options) -> forward kernel, backward kernel (None: rejected, the
# backward needs an argmax).  The names were recorded from the if-chains the two entry points had before the routes existed (each branch
# made to answer its kernel's name); the routes must reproduce every row.  Shapes too big to launch are here by descriptor alone.
F32, BF16 = E.F32, E.BF16
P0, P1, K3 = ((1, 3, 3), (1, 2, 2), (0, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (1, 1, 1), (1, 1, 1))
P3, T3 = ((2, 1, 1), (2, 1, 1), (0, 0, 0)), ((3, 1, 1), (1, 1, 1), (1, 0, 0))
SM, OCT, QUAD = (2, 8, 9, 10), (24, 40, 8), (12, 28, 8)      # the kernel suite's small clip; 8- and 4-channel slices of a wider buffer
C65536, C65535, ONE = (1, 2, 256, 256), (1, 2, 255, 257), (8, 8, 0)      # one channel octet: H x W 8-channel columns
POOL_TABLE = [
    ('natural_k133s2_f32', P0, F32, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd_k133s2_kernel<f32>'),
    ('natural_k333s2_f32', P1, F32, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd_k3s2_kernel<f32>'),
    ('natural_k333s1_f32', K3, F32, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd_k3s1_kernel<f32>'),
    ('natural_k211s2_f32', P3, F32, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd8_kernel<f32>'),
    ('c12_k133s2_f32', P0, F32, SM, QUAD, 'affine_relu', 'ok', dict(), 'maxpool_fwd_kernel<f32>', 'maxpool_bwd_kernel<f32>'),
    ('c12_k333s1_f32', K3, F32, SM, QUAD, 'affine_relu', 'ok', dict(), 'maxpool_tslide_kernel<f32>', 'maxpool_bwd_kernel<f32>'),
    ('lds2_f32', K3, F32, SM, OCT, 'affine_relu', 'ok', dict(pool_lds=2), 'maxpool_k3s1_lds_kernel<f32>', 'maxpool_bwd_k3s1_kernel<f32>'),
    ('twalk2_f32', K3, F32, SM, OCT, 'affine_relu', 'ok', dict(pool_twalk=2), 'maxpool_tslide8_kernel<f32>', 'maxpool_bwd_k3s1_twalk_kernel<f32>'),
    ('twalk2_lds0_f32', K3, F32, SM, OCT, 'affine_relu', 'ok', dict(pool_twalk=2, pool_lds=0), 'maxpool_tslide8_kernel<f32>', 'maxpool_bwd_k3s1_twalk_kernel<f32>'),
    ('twalk3_f32', K3, F32, SM, OCT, 'affine_relu', 'ok', dict(pool_twalk=3, pool_lds=0), 'maxpool_tslide8_kernel<f32>', 'maxpool_bwd_k3s1_twalk_kernel<f32>'),
    ('blk0_k133s2_f32', P0, F32, SM, OCT, 'affine_relu', 'ok', dict(pool_blk=0), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd8_kernel<f32>'),
    ('blk0_k333s2_f32', P1, F32, SM, OCT, 'affine_relu', 'ok', dict(pool_blk=0), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd8_kernel<f32>'),
    ('cols65536_f32', K3, F32, C65536, ONE, 'affine_relu', 'ok', dict(), 'maxpool_k3s1_lds_kernel<f32>', 'maxpool_bwd_k3s1_twalk_kernel<f32>'),
    ('cols65535_f32', K3, F32, C65535, ONE, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd_k3s1_kernel<f32>'),
    ('cols65536_lds0_f32', K3, F32, C65536, ONE, 'affine_relu', 'ok', dict(pool_lds=0), 'maxpool_tslide8_kernel<f32>', 'maxpool_bwd_k3s1_twalk_kernel<f32>'),
    ('cols65535_lds0_f32', K3, F32, C65535, ONE, 'affine_relu', 'ok', dict(pool_lds=0), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd_k3s1_kernel<f32>'),
    ('cols65536_k311_f32', T3, F32, C65536, ONE, 'affine_relu', 'ok', dict(), 'maxpool_tslide8_kernel<f32>', 'maxpool_bwd8_kernel<f32>'),
    ('cols65535_k311_f32', T3, F32, C65535, ONE, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_kernel<f32>', 'maxpool_bwd8_kernel<f32>'),
    ('natural_k133s2_bf16', P0, BF16, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k133s2_kernel<bf16>'),
    ('natural_k333s2_bf16', P1, BF16, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k3s2_kernel<bf16>'),
    ('natural_k333s1_bf16', K3, BF16, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('natural_k211s2_bf16', P3, BF16, SM, OCT, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd8_kernel<bf16>'),
    ('c12_k133s2_bf16', P0, BF16, SM, QUAD, 'affine_relu', 'ok', dict(), 'maxpool_fwd_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('c12_k333s1_bf16', K3, BF16, SM, QUAD, 'affine_relu', 'ok', dict(), 'maxpool_tslide_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('lds2_bf16', K3, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_lds=2), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('twalk2_bf16', K3, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_twalk=2), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('twalk2_lds0_bf16', K3, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_twalk=2, pool_lds=0), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('twalk3_bf16', K3, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_twalk=3, pool_lds=0), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd_k3s1_twalk_kernel<bf16>'),
    ('blk0_k133s2_bf16', P0, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_blk=0), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd8_kernel<bf16>'),
    ('blk0_k333s2_bf16', P1, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_blk=0), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd8_kernel<bf16>'),
    ('cols65536_bf16', K3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('cols65535_bf16', K3, BF16, C65535, ONE, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('cols65536_lds0_bf16', K3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(pool_lds=0), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('cols65535_lds0_bf16', K3, BF16, C65535, ONE, 'affine_relu', 'ok', dict(pool_lds=0), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('cols65536_k311_bf16', T3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd8_kernel<bf16>'),
    ('cols65535_k311_bf16', T3, BF16, C65535, ONE, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd8_kernel<bf16>'),
    ('pk0_lds2', K3, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_pk=0, pool_lds=2), 'maxpool_k3s1_lds_kernel<bf16>', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('pk0_k133s2', P0, BF16, SM, OCT, 'affine_relu', 'ok', dict(pool_pk=0), 'maxpool_fwd8_kernel<bf16>', 'maxpool_bwd_k133s2_kernel<bf16>'),
    # a scale without a shift: every kernel would read shift[c] through the null pointer, so the forward is rejected (None); the backward has no pre
    ('scale_only_lds2', K3, BF16, SM, OCT, 'scale_only', 'ok', dict(pool_lds=2), None, 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('scale_only_k133s2', P0, BF16, SM, OCT, 'scale_only', 'ok', dict(), None, 'maxpool_bwd_k133s2_kernel<bf16>'),
    ('no_pre_lds2', K3, BF16, SM, OCT, 'none', 'ok', dict(pool_lds=2), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('relu_only_k133s2', P0, BF16, SM, OCT, 'relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k133s2_kernel<bf16>'),
    ('t1_lds2', K3, BF16, (2, 1, 9, 10), OCT, 'affine_relu', 'ok', dict(pool_lds=2, pool_twalk=2), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('t2_lds2', K3, BF16, (2, 2, 9, 10), OCT, 'affine_relu', 'ok', dict(pool_lds=2, pool_twalk=2), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('t1_c12', K3, BF16, (2, 1, 9, 10), QUAD, 'affine_relu', 'ok', dict(), 'maxpool_fwd_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('t2_c12', K3, BF16, (2, 2, 9, 10), QUAD, 'affine_relu', 'ok', dict(), 'maxpool_tslide_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('t1_cols65536', K3, BF16, (1, 1, 256, 256), ONE, 'affine_relu', 'ok', dict(), 'maxpool_fwd8_pk_kernel', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('argmax_plus4_k333s1', K3, BF16, SM, OCT, 'affine_relu', '+4', dict(), 'maxpool_fwd_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('argmax_plus4_lds2_twalk2', K3, BF16, SM, OCT, 'affine_relu', '+4', dict(pool_lds=2, pool_twalk=2), 'maxpool_fwd_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('argmax_plus4_k133s2', P0, BF16, SM, OCT, 'affine_relu', '+4', dict(), 'maxpool_fwd_kernel<bf16>', 'maxpool_bwd_kernel<bf16>'),
    ('argmax_plus4_c12', K3, F32, SM, QUAD, 'affine_relu', '+4', dict(), 'maxpool_tslide_kernel<f32>', 'maxpool_bwd_kernel<f32>'),
    ('argmax_null_k333s1', K3, BF16, SM, OCT, 'affine_relu', 'null', dict(), 'maxpool_fwd8_pk_kernel', None),
    ('argmax_null_cols65536', K3, BF16, C65536, ONE, 'affine_relu', 'null', dict(), 'maxpool_k3s1_pk_kernel', None),
    ('argmax_null_c12', P0, F32, SM, QUAD, 'affine_relu', 'null', dict(), 'maxpool_fwd_kernel<f32>', None),
    ('twalk0_cols65536', K3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(pool_twalk=0), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('twalk0_lds0_cols65536', K3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(pool_twalk=0, pool_lds=0), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd_k3s1_kernel<bf16>'),
    ('twalk3_cols65536', K3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(pool_twalk=3), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_twalk_kernel<bf16>'),
    ('lds0_pk0_cols65536', K3, BF16, C65536, ONE, 'affine_relu', 'ok', dict(pool_lds=0, pool_pk=0), 'maxpool_tslide8_kernel<bf16>', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('plane_2p30', K3, BF16, (1, 2, 4096, 4096), (64, 64, 0), 'affine_relu', 'ok', dict(), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_twalk_kernel<bf16>'),
    ('plane_2p30_f32', K3, F32, (1, 2, 4096, 4096), (64, 64, 0), 'affine_relu', 'ok', dict(), 'maxpool_k3s1_lds_kernel<f32>', 'maxpool_bwd_k3s1_twalk_kernel<f32>'),
    ('plane_2p27', K3, BF16, (1, 2, 4096, 4096), ONE, 'affine_relu', 'ok', dict(), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_tw3_kernel'),
    ('plane_2p30_dy_ld', K3, BF16, (1, 2, 4096, 4096), (8, 8, 0, 64), 'affine_relu', 'ok', dict(), 'maxpool_k3s1_pk_kernel', 'maxpool_bwd_k3s1_twalk_kernel<bf16>'),
]
