"""The max-pool kernels of csrc/pool.hip, bit for bit: case tables, a float64 window-scan reference and the runners that the host
test (tests/test_pool_cases_host.py, CPU model of the ABI) and the GPU test (tests/test_gpu_pool_kernels.py, libvinet_hip.so) share.

A pool is a selection, so nothing here takes a tolerance.  The reference (pool_ref) scans the window taps in (t, h, w) order over
float64 copies of the inputs with -inf padding and takes a tap when `v > best or (isnan(v) and not isnan(best))`: the first maximum
wins, padding never wins, the first NaN of a window propagates.  It shares no code with tests/abi_emulator.py and never calls
torch.max_pool3d.  The backward reference is an index_add of dy at the argmax positions in float64 (+ the old dx under accumulate).

Data, chosen so that every expectation is exact in fp32 AND in bf16:
  affine, affine_relu   x a multiple of 1/4 in [-4, 4], scale from {-2, -1, -0.5, 0.5, 1, 2} cycling over the channels, shift a multiple
                        of 1/4 in [-1, 1]: x * scale + shift is a multiple of 1/8 of magnitude <= 9 (8 significant bits), so the fma,
                        the rounding to bf16 and every comparison have one right answer -- ties (there are many) included
  none, relu            normal random data over 13 binades, rounded to the storage type: no arithmetic happens, and the data walks
                        the 16-bit order codes of the packed-key kernels across exponents and both signs
  NaN family (none)     the same with +inf at ~5 % of the positions and a positive quiet NaN at [:, 1::4, 1::4, 1::4, ::3]: no window
                        of the 3x3x3/s1 and 1x3x3/s2 pools holds two, so first-NaN-wins (the kernels) and last-NaN-wins (aten on
                        the CPU, inside the model) agree
  backward              dy and the old dx are integers in [-2, 2]: every sum has magnitude <= 27 * 2 + 2, exact in bf16.  Each case
                        runs with the reference's argmax of a forward case, or with a random in-range tap per output (every tap code
                        occurs, many windows route to one voxel)
OUTSIDE THE CONTRACT, and in no case: -0.0 (packed keys order -0 < +0, float compares do not), -inf (a window of nothing but -inf
has no in-range winner), a NaN through a ReLU (fmaxf(NaN, 0) and the integer max disagree by design).

Views: x / dx and y / dy are each dense, a channel slice (c_off 8 of a wider row) or a T slice (frames 1 .. T of T + 2) inside
buffers filled with a sentinel; the argmax lies between two 16-byte guards of 0xA5.  Every case names the kernel it is meant to
reach, and the runner asks the library's name query with the launch's own arguments before it launches."""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import torch

from tests import route_cases as R
from tests.tail_cases import BF16, BITS, DTN, F32, TDT, Side, Slab      # noqa: F401 (Side: for the two test modules)
from vinet_amd import _lib as L

OPT_DEFAULTS = R.option_defaults(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vinet_amd", "csrc", "options.h"))

# ---- pools: (kernel, stride, padding) ----
K3 = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
P0 = ((1, 3, 3), (1, 2, 2), (0, 1, 1))
P1 = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
T2 = ((2, 1, 1), (2, 1, 1), (0, 0, 0))
S2 = ((1, 2, 2), (1, 2, 2), (0, 0, 0))
T4 = ((4, 1, 1), (2, 1, 2), (0, 0, 0))
T8 = ((8, 1, 1), (8, 1, 1), (0, 0, 0))
POOL_NAMES = {K3: "k333s1", P0: "k133s2", P1: "k333s2", T2: "k211s2", S2: "k122s2", T4: "k411s212", T8: "k811s8"}
NON_OVERLAPPING = (T2, S2, T4, T8)

# (B, T, H, W, C) per pool: the smallest shapes at which each kernel can still go wrong
GEOMETRIES = {
    K3: [(1, 2, 1, 3, 8),           # T = 2: both temporal edges of the T-walk (to >= 1, to + 1 < T) meet in one window; H = 1
         (2, 3, 9, 10, 24),         # 2 x 2 partial 8 x 8 tiles, a partial channel group, two batch items
         (2, 1, 9, 10, 24),         # T = 1 leaves the T-walk
         (1, 4, 8, 17, 72),         # two channel groups of 64, the second one octet wide; H exactly one tile, three W tiles
         (1, 5, 2, 2, 8),           # every window hangs over every H / W edge
         (2, 3, 9, 10, 12),         # C = 12: the 4-channel kernels (tslide)
         (1, 2, 3, 5, 12),          # ... at T = 2
         (2, 1, 9, 10, 12)],        # ... at T = 1: the generic 4-channel kernel with 27 taps
    P0: [(2, 1, 1, 1, 8), (1, 2, 1, 6, 8), (1, 3, 7, 9, 24), (2, 2, 8, 10, 16), (2, 3, 7, 9, 12)],
    P1: [(1, 1, 1, 1, 8), (1, 2, 2, 2, 8), (2, 5, 7, 9, 24), (1, 4, 8, 10, 16), (1, 3, 5, 6, 12)],
    # extents that are no multiple of the stride: trailing frames / rows / columns that no window covers
    T2: [(2, 5, 3, 4, 8)],
    S2: [(1, 2, 5, 7, 16)],
    T4: [(2, 7, 3, 5, 16)],
    T8: [(1, 17, 2, 3, 8)],
}
NAN_GEOMETRIES = {K3: [(2, 3, 9, 10, 24), (1, 4, 8, 17, 72), (2, 3, 9, 10, 12)], P0: [(1, 3, 7, 9, 24), (2, 2, 8, 10, 16), (2, 3, 7, 9, 12)]}

PRE_FORMS = ["none", "relu", "affine", "affine_relu"]
VIEW_FORMS = ["dense", "chan", "tslice"]
# (x / dx form, y / dy form) by the running number of a kernel's cases: the first three already hold every form on either side
VIEW_PAIRS = [("dense", "chan"), ("chan", "tslice"), ("tslice", "dense"), ("dense", "dense"), ("chan", "chan"), ("tslice", "tslice"),
              ("dense", "tslice"), ("chan", "dense"), ("tslice", "chan")]
SCALES = [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]
X_OUTSIDE = 3e38        # around x: wins every comparison it is wrongly part of (where the channel's scale is positive)
Y_FILL = -77.0          # y, dx and the buffers around them before the launch: no expectation holds it
DY_OUTSIDE = 1000.0     # around dy: one wrongly gathered element puts a sum far off
GUARD = 0xA5
FWD_INSTANTIATIONS = (["maxpool_%s_kernel<%s>" % (k, t) for k in ("fwd", "tslide", "fwd8", "tslide8", "k3s1_lds") for t in ("f32", "bf16")] +
                      ["maxpool_fwd8_pk_kernel", "maxpool_k3s1_pk_kernel"])
BWD_INSTANTIATIONS = (["maxpool_%s_kernel<%s>" % (k, t) for k in ("bwd", "bwd8", "bwd_k133s2", "bwd_k3s2", "bwd_k3s1", "bwd_k3s1_twalk")
                       for t in ("f32", "bf16")] + ["maxpool_bwd_k3s1_tw3_kernel"])


def out_dims(pool, dims):
    k, s, p = pool
    return tuple((d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip(dims[1:4], k, s, p))


def fwd_routes(pool, dims, dt):
    """[(route, options, kernel)]: the forward kernels a geometry is run through, each forced by its options"""
    tn, T, Cc = DTN[dt], dims[1], dims[4]
    walk = pool == K3 and T >= 2
    if Cc % 8:
        return [("quad", {}, "maxpool_%s_kernel<%s>" % ("tslide" if walk else "fwd", tn))]
    out = [("default", {}, "maxpool_fwd8_kernel<f32>" if dt == F32 else "maxpool_fwd8_pk_kernel")]
    if dt == BF16:
        out.append(("pk0", dict(pool_pk=0), "maxpool_fwd8_kernel<bf16>"))
    if walk:
        out.append(("twalk2", dict(pool_twalk=2), "maxpool_tslide8_kernel<%s>" % tn))
        out.append(("lds2", dict(pool_lds=2), "maxpool_k3s1_lds_kernel<f32>" if dt == F32 else "maxpool_k3s1_pk_kernel"))
        if dt == BF16:
            out.append(("lds2_pk0", dict(pool_lds=2, pool_pk=0), "maxpool_k3s1_lds_kernel<bf16>"))
    return out


def bwd_routes(pool, dims, dt):
    tn = DTN[dt]
    if dims[4] % 8:
        return [("quad", {}, "maxpool_bwd_kernel<%s>" % tn)]
    if pool == K3:
        out = [("default", {}, "maxpool_bwd_k3s1_kernel<%s>" % tn),
               ("twalk2", dict(pool_twalk=2), "maxpool_bwd_k3s1_twalk_kernel<f32>" if dt == F32 else "maxpool_bwd_k3s1_tw3_kernel")]
        if dt == BF16:
            out.append(("twalk3", dict(pool_twalk=3), "maxpool_bwd_k3s1_twalk_kernel<bf16>"))
        return out
    if pool in (P0, P1):
        return [("default", {}, "maxpool_bwd_%s_kernel<%s>" % ("k133s2" if pool == P0 else "k3s2", tn)),
                ("blk0", dict(pool_blk=0), "maxpool_bwd8_kernel<%s>" % tn)]
    return [("default", {}, "maxpool_bwd8_kernel<%s>" % tn)]


class Case:
    """one launch (the forward: and its NULL-argmax twin).  kind: 'fwd' | 'bwd'; family: 'exact' | 'nan' (forward only);
    acc, src ('fwd': the reference's argmax of the affine_relu forward case of the geometry, 'rand': random in-range taps): backward"""

    def __init__(self, kind, pool, dims, dt, route, opts, kernel, views, pre=None, family="exact", acc=0, src=None):
        self.kind, self.pool, self.dims, self.dt, self.route, self.opts, self.kernel = kind, pool, dims, dt, route, opts, kernel
        self.xform, self.yform = views
        self.pre, self.family, self.acc, self.src = pre, family, acc, src
        self.null_twin = kind == "fwd"          # the same launch again with a NULL argmax (what inference passes)
        tail = (pre + ("-nan" if family == "nan" else "")) if kind == "fwd" else "%s-am_%s" % ("acc" if acc else "store", src)
        self.id = "%s-%s-%s-%s-%s-x_%s-y_%s-%s" % (kind, POOL_NAMES[pool], "x".join(str(d) for d in dims), DTN[dt], route, self.xform, self.yform, tail)

    def __repr__(self):
        return self.id


def _build():
    fwd, bwd, seen = [], [], {}

    def views(kernel):
        n = seen[kernel] = seen.get(kernel, -1) + 1
        return VIEW_PAIRS[n % len(VIEW_PAIRS)]

    for pool, geos in GEOMETRIES.items():
        for dims in geos:
            for dt in (F32, BF16):
                for route, opts, kernel in fwd_routes(pool, dims, dt):
                    for pre in PRE_FORMS:
                        fwd.append(Case("fwd", pool, dims, dt, route, opts, kernel, views(kernel), pre=pre))
                for route, opts, kernel in bwd_routes(pool, dims, dt):
                    for acc in (0, 1):
                        for src in ("fwd", "rand"):
                            bwd.append(Case("bwd", pool, dims, dt, route, opts, kernel, views(kernel), acc=acc, src=src))
    for pool, geos in NAN_GEOMETRIES.items():
        for dims in geos:
            for dt in (F32, BF16):
                for route, opts, kernel in fwd_routes(pool, dims, dt):
                    fwd.append(Case("fwd", pool, dims, dt, route, opts, kernel, views(kernel), pre="none", family="nan"))
    return fwd, bwd


FWD_CASES, BWD_CASES = _build()


# =====================================================================================================================
# data
# =====================================================================================================================
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


@functools.lru_cache(maxsize=None)
def fwd_inputs(pool, dims, dt, pre, family):
    """(x [B,T,H,W,C] in the storage type, scale, shift (fp32 [C], or None)); shared by every route of the geometry, never changed"""
    g = _gen("x", POOL_NAMES[pool], dims, dt, pre, family)
    Cc = dims[4]
    if pre.startswith("affine"):
        x = torch.randint(-16, 17, dims, generator=g).float() / 4
        scale = torch.tensor([SCALES[c % len(SCALES)] for c in range(Cc)])
        shift = torch.randint(-4, 5, (Cc,), generator=g).float() / 4
        return x.to(TDT[dt]), scale, shift
    x = torch.randn(dims, generator=g) * torch.exp2(torch.randint(-6, 7, dims, generator=g).float())
    x = x.to(TDT[dt])
    if family == "nan":
        x[torch.rand(dims, generator=g) < 0.05] = float("inf")
        x[:, 1::4, 1::4, 1::4, ::3] = float("nan")
    return x, None, None


def pre64(x, scale, shift, relu):
    """what the pool compares, in float64 (exact for the data above: no rounding to model)"""
    v = x.double()
    if scale is not None:
        v = v * scale.double() + shift.double()
    return v.clamp_min(0) if relu else v


def pool_ref(v, pool):
    """v: float64 [B,T,H,W,C] -> (max [B,oT,oH,oW,C] float64, argmax tap uint8): -inf padding, taps in (t, h, w) order, a tap is taken
    when it is greater than the best so far, or a NaN while the best is none"""
    (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = pool
    v = v.numpy()
    B, T, H, W, Cc = v.shape
    oT, oH, oW = out_dims(pool, v.shape)
    best = np.full((B, oT, oH, oW, Cc), -np.inf)
    arg = np.zeros(best.shape, np.uint8)
    taps = [(kt, kh, kw) for kt in range(kT) for kh in range(kH) for kw in range(kW)]
    with np.errstate(invalid="ignore"):
        for tap, (kt, kh, kw) in enumerate(taps):
            t, h, w = np.arange(oT) * sT - pT + kt, np.arange(oH) * sH - pH + kh, np.arange(oW) * sW - pW + kw
            ok = ((t >= 0) & (t < T))[:, None, None] & ((h >= 0) & (h < H))[None, :, None] & ((w >= 0) & (w < W))[None, None, :]
            g = v[:, t.clip(0, T - 1)][:, :, h.clip(0, H - 1)][:, :, :, w.clip(0, W - 1)]
            g = np.where(ok[None, :, :, :, None], g, -np.inf)
            take = (g > best) | (np.isnan(g) & ~np.isnan(best))
            best, arg = np.where(take, g, best), np.where(take, np.uint8(tap), arg)
    return torch.from_numpy(best), torch.from_numpy(arg)


@functools.lru_cache(maxsize=None)
def fwd_ref(pool, dims, dt, pre, family):
    x, scale, shift = fwd_inputs(pool, dims, dt, pre, family)
    return pool_ref(pre64(x, scale, shift, pre.endswith("relu")), pool)


def tap_positions(pool, dims, am):
    """input (t, h, w) of tap code am [B,oT,oH,oW,C] of every window, and whether it lies inside the input"""
    (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = pool
    oT, oH, oW = am.shape[1:4]
    am = am.long()
    t = torch.arange(oT).view(1, -1, 1, 1, 1) * sT - pT + am // (kH * kW)
    h = torch.arange(oH).view(1, 1, -1, 1, 1) * sH - pH + (am // kW) % kH
    w = torch.arange(oW).view(1, 1, 1, -1, 1) * sW - pW + am % kW
    return t, h, w, (t >= 0) & (t < dims[1]) & (h >= 0) & (h < dims[2]) & (w >= 0) & (w < dims[3])


@functools.lru_cache(maxsize=None)
def bwd_inputs(pool, dims, dt, src):
    """(dy [B,oT,oH,oW,C], old dx [B,T,H,W,C], argmax uint8 [B,oT,oH,oW,C]); dy and old dx integers in [-2, 2]"""
    g = _gen("dy", POOL_NAMES[pool], dims, dt, src)
    odims = (dims[0],) + out_dims(pool, dims) + (dims[4],)
    dy = torch.randint(-2, 3, odims, generator=g).float().to(TDT[dt])
    old = torch.randint(-2, 3, dims, generator=g).float().to(TDT[dt])
    if src == "fwd":
        am = fwd_ref(pool, dims, dt, "affine_relu", "exact")[1]
    else:
        (kT, kH, kW), _, (pT, pH, pW) = pool
        am = torch.randint(0, kT * kH * kW, odims, generator=g).to(torch.uint8)
        inside = tap_positions(pool, dims, am)[3]
        # a tap outside the input is no argmax a forward pass can produce: the window's tap (pT, pH, pW) is always inside
        am = torch.where(inside, am, torch.full_like(am, (pT * kH + pH) * kW + pW))
    return dy, old, am


@functools.lru_cache(maxsize=None)
def bwd_ref(pool, dims, dt, src):
    """the gather of dy through the argmax, float64, without the old dx"""
    dy, _, am = bwd_inputs(pool, dims, dt, src)
    B, T, H, W, Cc = dims
    t, h, w, inside = tap_positions(pool, dims, am)
    assert bool(inside.all())
    b, c = torch.arange(B).view(-1, 1, 1, 1, 1), torch.arange(Cc).view(1, 1, 1, 1, -1)
    flat = ((((b * T + t) * H + h) * W + w) * Cc + c).reshape(-1)
    return torch.zeros(B * T * H * W * Cc, dtype=torch.float64).index_add_(0, flat, dy.double().reshape(-1)).view(dims)


# =====================================================================================================================
# runners
# =====================================================================================================================
def view_geo(form, dims, wide):
    """Slab geometry of a view form; wide: the channels beside a channel slice (C = 12 always sits in rows of 32)"""
    B, T, H, W, Cc = dims
    if form == "chan":
        return dict(ld=32 if Cc == 12 else Cc + wide, c_off=8)
    if form == "tslice":
        return dict(t_total=T + 2, t_off=1)
    return {}


def kernel_name(lib, query, *args):
    buf = C.create_string_buffer(128)
    assert getattr(lib, query)(*args, buf, 128) == 0, lib.vinet_last_error()
    return buf.value.decode()


def _desc(case):
    k, s, p = case.pool
    return L.CPoolDesc(case.dt, *(k + s + p))


def assert_bits(got, ref64, dt, what):
    """got (storage type) equals the float64 expectation bit for bit; NaNs are compared by position"""
    want = ref64.to(TDT[dt])
    nan = torch.isnan(ref64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.equal(torch.isnan(got), nan), "%s: NaNs at other positions than expected" % what
    bad = (got.contiguous().view(BITS[dt]) != want.contiguous().view(BITS[dt])) & ~nan
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %r: %r against %r" % (what, int(bad.sum()), bad.numel(), at, float(got[at]), float(ref64[at])))


def _guarded(side, body):
    """a byte array between two 16-byte guards -> (buffer, pointer of the body)"""
    g = torch.full((16,), GUARD, dtype=torch.uint8)
    buf = side.put(torch.cat([g, body.reshape(-1), g]))
    return buf, buf.data_ptr() + 16


def _unguarded(buf, what):
    got = buf.cpu()
    assert bool((got[:16] == GUARD).all()) and bool((got[-16:] == GUARD).all()), what + ": a guard byte of the argmax changed"
    return got[16:-16]


def _same_bits(after, before, dt, what):
    assert torch.equal(after.cpu().view(BITS[dt]), before.view(BITS[dt])), what + " changed"


def check_forward(side, names, case):
    """`names`: the library that answers the name queries and holds the options (the host test: the real library beside the model).
    Gates: y and the argmax equal the reference everywhere; x, everything outside y's view and the guards are unchanged; the run
    with a NULL argmax reaches the same kernel and writes the same bits."""
    x0, scale, shift = fwd_inputs(case.pool, case.dims, case.dt, case.pre, case.family)
    ref_y, ref_am = fwd_ref(case.pool, case.dims, case.dt, case.pre, case.family)
    ydims = tuple(ref_y.shape)
    x = Slab(case.dims, case.dt, fill=X_OUTSIDE, values=x0, **view_geo(case.xform, case.dims, 16))
    y = Slab(ydims, case.dt, fill=Y_FILL, **view_geo(case.yform, ydims, 8))
    xb, yb, y2b = side.put(x.base), side.put(y.base), side.put(y.base)
    sc, sh = (None, None) if scale is None else (side.put(scale), side.put(shift))
    aff = L.CAffine(None if sc is None else sc.data_ptr(), None if sh is None else sh.data_ptr(), 1 if case.pre.endswith("relu") else 0)
    amb, amp = _guarded(side, torch.full((ref_am.numel(),), 255, dtype=torch.uint8))
    d = _desc(case)
    with R.options(names, case.opts, OPT_DEFAULTS):
        for buf, ptr in ((yb, amp), (y2b, None))[:2 if case.null_twin else 1]:
            args = (C.byref(d), x.ct(xb), aff, y.ct(buf), ptr)
            assert kernel_name(names, "vinet_maxpool3d_kernel_name", *args) == case.kernel, case
            side.call("vinet_maxpool3d", *args)
    assert_bits(y.inner(yb.cpu()), ref_y, case.dt, "%r: y" % case)
    y.assert_outside_untouched(yb, "%r: y" % case)
    got_am = _unguarded(amb, repr(case)).view(ref_am.shape)
    bad = got_am != ref_am
    assert not bool(bad.any()), "%r: argmax differs at %d of %d positions, first %r: %d against %d" % (
        case, int(bad.sum()), bad.numel(), tuple(int(i) for i in bad.nonzero()[0]), int(got_am[bad][0]), int(ref_am[bad][0]))
    _same_bits(xb, x.base, case.dt, "%r: x" % case)
    if case.null_twin:
        _same_bits(y2b, yb.cpu(), case.dt, "%r: y of the run without an argmax" % case)


def check_backward(side, names, case):
    """Gates: dx equals the reference bit for bit (positions no window covers: 0, or the old value under accumulate); everything
    outside dx's view, dy's buffer, the argmax and its guards are unchanged."""
    dy0, old, am = bwd_inputs(case.pool, case.dims, case.dt, case.src)
    ref = bwd_ref(case.pool, case.dims, case.dt, case.src) + (old.double() if case.acc else 0.0)
    ydims = tuple(dy0.shape)
    dy = Slab(ydims, case.dt, fill=DY_OUTSIDE, values=dy0, **view_geo(case.yform, ydims, 8))
    dx = Slab(case.dims, case.dt, fill=Y_FILL, values=old if case.acc else None, **view_geo(case.xform, case.dims, 16))
    dyb, dxb = side.put(dy.base), side.put(dx.base)
    amb, amp = _guarded(side, am)
    d = _desc(case)
    with R.options(names, case.opts, OPT_DEFAULTS):
        args = (C.byref(d), dy.ct(dyb), amp, dx.ct(dxb))
        assert kernel_name(names, "vinet_maxpool3d_bwd_kernel_name", *args) == case.kernel, case
        side.call("vinet_maxpool3d_bwd", *args, case.acc)
    assert_bits(dx.inner(dxb.cpu()), ref, case.dt, "%r: dx" % case)
    dx.assert_outside_untouched(dxb, "%r: dx" % case)
    _same_bits(dyb, dy.base, case.dt, "%r: dy" % case)
    assert torch.equal(_unguarded(amb, repr(case)), am.reshape(-1)), "%r: the argmax changed" % case
