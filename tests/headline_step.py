"""Census and float64 replay of the library launches of one real training step (tests/test_gpu_headline_step.py).

census(cfg) builds the step the way bench.measure does (ViNet-32, synthetic weights, 224 x 384, kldiv, fused Adam, the
weight-gradient side stream on), runs it once and records every Ctx.call: the entry point, a copy of every descriptor /
tensor struct among its arguments, the library's kernel name (conv and weight gradient) and a site string.  Device tap
tables are resolved through the engine's own tensors (ConvPlan._dev_taps), never by reading raw device memory.

replay_conv / replay_wgrad re-launch one census entry with the captured geometry and modes on fresh seeded buffers of the
same extents and compare the result with a float64 reference of the documented contract (the C ABI header, include/vinet_hip.h at the repository root).  With
integer data (activations, gradients and weights in [-2, 2], scales in {1, 2}, shifts in {-1, 0, 1}) every product and
every fp32 partial sum below 2^24 is exact in any order, so the stored value must equal the reference rounded to the output
dtype BIT FOR BIT.  Each comparison is also run against deliberately wrong references (a dropped 32-channel K chunk of one
tap, the last M tile dropped, a one-voxel shift), which it must reject.

A new model leg (AViNet, 64 x 256 x 448) is one more entry of CONFIGS."""
import ctypes as C
import gc

import torch

from vinet_amd import _lib as L
from vinet_amd import engine as E

F32, BF16, F32S = L.F32, L.BF16, L.F32S
TDT = {F32: torch.float32, BF16: torch.bfloat16, F32S: torch.float32}
EXACT = 1 << 24          # fp32 integers below this are exact; every exact check asserts its worst-case |sum| stays below it
SENTINEL = -0.28125      # not an integer and negative: no conv output (integers, or sigmoid values in (0, 1)) can equal it

# name -> (dtype, clips per GPU, T, H, W, model)
CONFIGS = {
    "bf16": dict(dtype="bf16", batch=192, clip=32, height=224, width=384, model="vinet"),      # the bench headline
    "fp32s": dict(dtype="fp32s", batch=64, clip=32, height=224, width=384, model="vinet"),     # bench --full's parity_path
}

CONV_ENTRIES = ("vinet_conv3d",)
WGRAD_ENTRIES = ("vinet_conv3d_wgrad",)
TENSOR_TYPES = (L.CTensor, L.CConvDesc, L.CWgradDesc, L.CPoolDesc, L.CAffine)


# ---- census -----------------------------------------------------------------------------------------------------------
class Entry:
    """one distinct launch of the step: entry point, struct copies, kernel name, site, how often it ran"""

    def __init__(self, name, args, kname, site, taps):
        self.name, self.args, self.kname, self.site, self.taps, self.count = name, args, kname, site, taps, 1

    @property
    def desc(self):
        return self.args[0]

    def __repr__(self):
        return "%s[%s] %s" % (self.name, self.kname, self.site)


def _copy_arg(a):
    obj = getattr(a, "_obj", a)           # C.byref(struct) -> the struct
    if isinstance(obj, TENSOR_TYPES):
        return type(obj).from_buffer_copy(obj)
    if isinstance(obj, (C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double)):
        return obj.value
    return obj


def _struct_key(s):
    """every integer field of a struct (pointers reduced to set / unset), recursively"""
    out = []
    for f, _ in s._fields_:
        v = getattr(s, f)
        if isinstance(v, C.Structure):
            out.append(_struct_key(v))
        elif f in ("ptr", "taps", "w", "scale", "shift", "out_scale", "out_shift", "stats", "splitk_ws", "dw", "bnb_z",
                   "bnb_mean", "bnb_invstd", "bnb_partials", "bnb_c1", "bnb_c2"):
            out.append(bool(v))
        else:
            out.append(v)
    return tuple(out)


def kernel_name(entry_name, d):
    buf = C.create_string_buffer(96)
    fn = L.get().vinet_conv3d_kernel_name if entry_name == "vinet_conv3d" else L.get().vinet_conv3d_wgrad_kernel_name
    fn(C.byref(d), buf, 96)
    return buf.value.decode()


def _site(name, args):
    def t(ct):
        return "%dx%dx%dx%dx%d" % (ct.B, ct.T, ct.H, ct.W, ct.C)
    a0 = args[0]
    if isinstance(a0, L.CConvDesc):
        return "conv x%s -> y%s taps%d s%d%d%d tline%d" % (t(a0.x), t(a0.y), a0.ntaps, a0.sT, a0.sH, a0.sW, a0.tline)
    if isinstance(a0, L.CWgradDesc):
        return "wgrad x%s dy%s taps%d s%d%d%d tline%d" % (t(a0.x), t(a0.dy), a0.ntaps, a0.sT, a0.sH, a0.sW, a0.tline)
    return " ".join(t(a) for a in args if isinstance(a, L.CTensor)) or name


def census(cfg_name, seed=0):
    """run one training step of CONFIGS[cfg_name] on cuda:0 and return its distinct launches [Entry] and the peak HBM (GB)
    of the step.  The model, optimizer and activations are freed before this returns."""
    from vinet_amd import loss, model, optim, synth
    cfg = CONFIGS[cfg_name]
    dev = torch.device("cuda:0")
    old_dt = E.default_dtype()
    old_cfg = E.configure(WGRAD_SIDE_STREAM=True)
    E.set_default_dtype(cfg["dtype"])
    taps = {}
    orig_dev_taps, orig_call = E.ConvPlan._dev_taps, E.Ctx.call
    entries, index = [], {}

    def dev_taps(self, key, rows, device):
        t = orig_dev_taps(self, key, rows, device)
        taps[t.data_ptr()] = t
        return t

    def call(self, name, *args, **kw):
        cargs = [_copy_arg(a) for a in args]
        kname, tp = "", None
        if name in CONV_ENTRIES + WGRAD_ENTRIES:
            d = cargs[0]
            kname = kernel_name(name, d)
            tp = None
            if not (name == "vinet_conv3d" and d.tline == 3):
                tp = taps[d.taps]       # KeyError: a tap table the engine did not make through ConvPlan._dev_taps
                tp = tuple(tuple(r) for r in tp.cpu().tolist())
        key = (name, tuple(_struct_key(a) if isinstance(a, C.Structure) else a for a in cargs if not isinstance(a, int)
                           or name not in CONV_ENTRIES + WGRAD_ENTRIES), kname, tp)
        if name not in CONV_ENTRIES + WGRAD_ENTRIES:
            # (non-conv entries: the pointer / stream arguments differ per launch; their extents live in the structs)
            key = (name, tuple(_struct_key(a) for a in cargs if isinstance(a, C.Structure)),
                   tuple(a for a in cargs if isinstance(a, int) and abs(a) < (1 << 20)))
        e = index.get(key)
        if e is None:
            e = index[key] = Entry(name, cargs, kname, _site(name, cargs), tp)
            entries.append(e)
        else:
            e.count += 1
        return orig_call(self, name, *args, **kw)

    E.ConvPlan._dev_taps, E.Ctx.call = dev_taps, call
    try:
        torch.zeros(1, device=dev)          # (initialises the device before the allocator statistics are touched)
        torch.cuda.reset_peak_memory_stats(dev)
        B, T, H, W = cfg["batch"], cfg["clip"], cfg["height"], cfg["width"]
        m = model.VideoSaliencyModel(num_clips=T)
        m.load_state_dict(synth.synth_state_dict(m.state_dict(), seed))
        m = m.to(dev).train()
        opt = optim.Adam(m.parameters(), lr=1e-4)
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        x = torch.randn((B, T, 3, H, W), generator=g, device=dev).permute(0, 2, 1, 3, 4)
        gt = synth.gt_map(B, H, W, seed).to(dev)
        opt.zero_grad()
        lo = loss.kldiv(m(x), gt)
        lo.backward()
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(lo).item()
        peak = torch.cuda.max_memory_allocated(dev) / 1e9
        del m, opt, x, gt, lo
    finally:
        E.ConvPlan._dev_taps, E.Ctx.call = orig_dev_taps, orig_call
        E.set_default_dtype({F32: "fp32", BF16: "bf16", F32S: "fp32s"}[old_dt])
        E.configure(**old_cfg)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return entries, peak


# ---- buffers ----------------------------------------------------------------------------------------------------------
def span(B, T, H, W, Cc, ld, sB):
    return (B - 1) * sB + ((T - 1) * H * W + (H - 1) * W + (W - 1)) * ld + Cc


class Buf:
    """fresh device buffer behind a view of a census descriptor: the view's span plus the original pointer's offset inside a
    512-byte granule (so every alignment property a kernel selector could look at is kept), filled with `fill`"""

    def __init__(self, orig_ptr, nelem, tdt, dev):
        es = torch.tensor([], dtype=tdt).element_size()
        self.lead = (int(orig_ptr or 0) % 512) // es
        self.t = torch.empty(self.lead + nelem + 64, dtype=tdt, device=dev)
        self.tdt, self.es = tdt, es

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead * self.es

    def view5(self, B, T, H, W, Cc, ld, sB, off=0):
        return torch.as_strided(self.t, (B, T, H, W, Cc), (sB, H * W * ld, W * ld, ld, 1), self.lead + off)


def tensor_buf(ct, tdt, dev):
    return Buf(ct.ptr, span(ct.B, ct.T, ct.H, ct.W, ct.C, ct.ld, ct.sB), tdt, dev)


def view_of(buf, ct):
    return buf.view5(ct.B, ct.T, ct.H, ct.W, ct.C, ct.ld, ct.sB)


def fill_ints(t, lo, hi, gen):
    """integers in [lo, hi] (the fill runs in fp32 / bf16 directly: random_ draws exact integers)"""
    t.random_(lo, hi + 1, generator=gen)
    return t


def fill_normal(t, std, gen):
    t.normal_(0.0, std, generator=gen)
    return t


def vec(n, kind, gen, dev, exact):
    """per-channel fp32 vector: kind 'scale' ({1, 2} / U(0.5, 1.5)), 'shift' ({-1, 0, 1} / N(0, 0.1))"""
    t = torch.empty(n + 4, dtype=torch.float32, device=dev)
    if kind == "scale":
        return fill_ints(t, 1, 2, gen) if exact else t.uniform_(0.5, 1.5, generator=gen)
    return fill_ints(t, -1, 1, gen) if exact else fill_normal(t, 0.1, gen)


def items_to_check(B, views):
    """batch items 0, 1, B-2, B-1 and every item holding an element at offset 2^31 - 1, 2^31, 2^32 - 1 or 2^32 of any of
    `views` ((span, sB) pairs): M tiles span item boundaries, and the 32-bit edges are where a truncated offset shows"""
    out = {0, min(1, B - 1), max(B - 2, 0), B - 1}
    for n, sB in views:
        for edge in ((1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32):
            if edge < n and sB > 0:
                out.add(min(edge // sB, B - 1))
    return sorted(out)


def to_dtype_exact(v64, tdt):
    """float64 reference -> the stored dtype (RNE; the float32 step is exact for |v| < 2^24)"""
    return v64.to(torch.float32).to(tdt)


# ---- weights ----------------------------------------------------------------------------------------------------------
def _split_perm():
    # VINET_F32S packs: positions 8q .. 8q+7 of a 32-wide chunk hold channels {4q .. 4q+3, 16+4q .. 16+4q+3}
    return [4 * (p // 8) + (p % 8) if p % 8 < 4 else 16 + 4 * (p // 8) + (p % 8 - 4) for p in range(32)]


def pack_weights(wl, cdt):
    """logical packed weights [nsl][N][Kp] (fp32) -> the bytes a descriptor of arithmetic dtype cdt reads"""
    if cdt == BF16:
        return wl.to(torch.bfloat16).contiguous()
    if cdt == F32:
        return wl.contiguous()
    rows = wl.reshape(-1, wl.shape[-1] // 32, 32)
    hi = rows.to(torch.bfloat16)
    lo = (rows - hi.float()).to(torch.bfloat16)
    perm = torch.tensor(_split_perm(), device=wl.device)
    return torch.cat([hi[..., perm], lo[..., perm]], -1).contiguous()


def weight_values(wl, cdt):
    """the weights the arithmetic sees (bf16: rounded; F32S: hi + lo)"""
    if cdt == BF16:
        return wl.to(torch.bfloat16).double()
    if cdt == F32S:
        hi = wl.to(torch.bfloat16)
        return hi.double() + (wl - hi.float()).to(torch.bfloat16).double()
    return wl.double()


# ---- float64 references -----------------------------------------------------------------------------------------------
def _gather_axis(x, idx, axis):
    n = x.shape[axis]
    ok = (idx >= 0) & (idx < n)
    g = x.index_select(axis, idx.clamp(0, n - 1))
    shape = [1] * x.ndim
    shape[axis] = -1
    return g * ok.reshape(shape).to(g.dtype)


def gathered(x, sT, sH, sW, dt_, dh_, dw_, oT, oH, oW):
    """x[t*sT+dt, h*sH+dh, w*sW+dw, :] with zero fill, x = one item [T][H][W][C] -> [oT][oH][oW][C]"""
    dev = x.device
    g = _gather_axis(x, torch.arange(oT, device=dev) * sT + dt_, 0)
    g = _gather_axis(g, torch.arange(oH, device=dev) * sH + dh_, 1)
    return _gather_axis(g, torch.arange(oW, device=dev) * sW + dw_, 2)


def affine64(x, scale, shift, relu, Cc, round_bf16=False):
    if scale is not None:
        x = x * scale[:Cc].double() + shift[:Cc].double()
        if round_bf16:
            x = x.to(torch.float32).to(torch.bfloat16).double()
    if relu:
        x = x.clamp_min(0)
    return x


def conv_ref_item(d, xi, w64, taps, drop=None):
    """sum over taps of one item (xi: [T][H][W][C] float64 with the pending affine applied) -> [oT][oH][oW][Nw] float64, and
    the same sum over |terms|.  drop = (tap index, 32-channel chunk) leaves that K chunk out (a self-test reference)."""
    Nw = w64.shape[1]
    acc = torch.zeros((d.oT, d.oH, d.oW, Nw), dtype=torch.float64, device=xi.device)
    mag = torch.zeros_like(acc)
    for k, (dt_, dh_, dw_, sl) in enumerate(taps):
        if d.mode == 0:
            g = gathered(xi, d.sT, d.sH, d.sW, dt_, dh_, dw_, d.oT, d.oH, d.oW).reshape(-1, xi.shape[-1])
            w = w64[sl, :, :xi.shape[-1]]
            if drop is not None and drop[0] == k:
                w = w.clone()
                w[:, 32 * drop[1]:32 * drop[1] + 32] = 0
            acc += (g @ w.T).reshape(acc.shape)
            mag += (g.abs() @ w.abs().T).reshape(acc.shape)
        else:       # VINET_CONV_STEM: each K chunk is 8 consecutive W positions x 4 channels
            for p in range(8):
                g = gathered(xi, d.sT, d.sH, d.sW, dt_, dh_, dw_ + p, d.oT, d.oH, d.oW).reshape(-1, 4)
                w = w64[sl, :, 4 * p:4 * p + 4]
                if drop is not None and drop[0] == k and drop[1] == 0:
                    w = w * 0
                acc += (g @ w.T).reshape(acc.shape)
                mag += (g.abs() @ w.abs().T).reshape(acc.shape)
    return acc, mag


def conv_tsd_ref_item(d, dyi, w64, drop=None):
    """tline 3: dx[ti] = sum_{kt: (ti + p - kt) % s == 0} dy[(ti + p - kt) / s] @ w[kt]^T (one item)"""
    k, s, p = d.ntaps, d.sT, d.tpad
    N = dyi.shape[-1]
    Cc = d.y.C
    acc = torch.zeros((d.y.T, d.y.H, d.y.W, Cc), dtype=torch.float64, device=dyi.device)
    mag = torch.zeros_like(acc)
    for ti in range(d.y.T):
        for kt in range(k):
            num = ti + p - kt
            if num % s == 0 and 0 <= num // s < dyi.shape[0]:
                w = w64[kt, :, :N]
                if drop is not None and drop[0] == kt:
                    w = w.clone()
                    w[:, 32 * drop[1]:32 * drop[1] + 32] = 0
                g = dyi[num // s].reshape(-1, N)
                acc[ti] += (g @ w.T).reshape(acc.shape[1:])
                mag[ti] += (g.abs() @ w.abs().T).reshape(acc.shape[1:])
    return acc, mag


def act64(v, act):
    if act == L.ACT_RELU:
        return v.clamp_min(0)
    if act == L.ACT_SIGMOID:
        return torch.sigmoid(v)
    return v


# ---- conv replay ------------------------------------------------------------------------------------------------------
class Result:
    def __init__(self, entry, mode):
        self.entry, self.mode, self.errors, self.checked, self.selftest = entry, mode, [], 0, []
        self.exact = mode == "exact"
        self.notes = []

    def fail(self, msg):
        self.errors.append("%r [%s]: %s" % (self.entry, self.mode, msg))


def compare(got, ref, mag, exact, tdt, tol=None):
    """None if `got` (stored dtype) matches the float64 reference, else a description.  exact: bit for bit after rounding
    ref to the stored dtype.  Otherwise |got - ref| <= tol(ref, mag) elementwise."""
    if exact:
        exp = to_dtype_exact(ref, tdt)
        if torch.equal(got, exp):
            return None
        bad = (got != exp).nonzero()
        i = tuple(bad[0].tolist())
        return "%d of %d elements differ, first at %s (got %r, expected %r)" % (bad.shape[0], got.numel(), list(i),
                                                                              got[i].item(), exp[i].item())
    err = (got.double() - ref).abs()
    lim = tol(ref, mag)
    bad = err > lim
    if not bool(bad.any()):
        return None
    i = tuple(bad.nonzero()[0].tolist())
    return "%d of %d elements beyond the bound, first at %s (got %r, ref %r, bound %r)" % (
        int(bad.sum()), got.numel(), list(i), got[i].item(), ref[i].item(), lim[i].item())


def _out_round(tdt):
    return 2.0 ** -8 if tdt == torch.bfloat16 else 2.0 ** -23


def conv_tolerance(d, tdt_out):
    """realistic-data bound for a forward / data-gradient launch: output rounding (half an ulp of the stored dtype, taken as a
    full ulp: 2^-8 bf16, 2^-23 fp32) plus the arithmetic: bf16 operands with a pending affine are rounded to bf16 after the
    affine (2^-8 per term); VINET_F32S splits each operand into hi + lo with ~2^-17 left out (2^-15 per term, both operands and
    slack); fp32 accumulation of the K terms in any tiled order (2^-16 of sum |terms|, i.e. 256 ulp of the largest partial)"""
    per_term = 2.0 ** -16
    if d.dtype == BF16 and d.pre.scale:
        per_term += 2.0 ** -8
    if d.dtype == F32S:
        per_term += 2.0 ** -15
    r = _out_round(tdt_out)
    return lambda ref, mag: r * ref.abs() + per_term * mag * (d.out_scale and 2.0 or 1.0) + 1e-30


def replay_conv(e, exact, seed, selftest=True, only_items=None):
    """re-launch conv census entry `e` on fresh data; returns a Result.  only_items: check these batch items instead of
    items_to_check (the realistic-data pass)"""
    lib = L.get()
    dev = torch.device("cuda:0")
    d0 = e.desc
    res = Result(e, "exact" if exact else "realistic")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    d = L.CConvDesc.from_buffer_copy(d0)
    xdt = TDT[d.dtype]
    ydt = TDT[d.out_dtype] if d.out_dtype != F32S else torch.float32
    keep = []

    # input
    xb = tensor_buf(d.x, xdt, dev)
    fill_ints(xb.t, -2, 2, gen) if exact else fill_normal(xb.t, 1.0, gen)
    d.x.ptr = xb.ptr
    Cx = d.x.C
    pre = None
    if d.pre.scale:
        ps, pb = vec(Cx, "scale", gen, dev, exact), vec(Cx, "shift", gen, dev, exact)
        d.pre.scale, d.pre.shift = ps.data_ptr(), pb.data_ptr()
        keep += [ps, pb]
        pre = (ps, pb)
    # weights
    N = d.y.C
    Nw = d.n_valid if d.n_valid > 0 else N
    if d.tline == 3:
        nsl = d.ntaps
        Nw = d.y.C
    else:
        nsl = max(r[3] for r in e.taps) + 1
        tt = torch.tensor(e.taps, dtype=torch.int32, device=dev).reshape(-1)
        keep.append(tt)
        d.taps = tt.data_ptr()
    Kin = d.x.C if d.mode == 0 else 32
    wl = torch.zeros((nsl, Nw, d.Kp), dtype=torch.float32, device=dev)
    if exact:
        fill_ints(wl[:, :, :Kin], -2, 2, gen)
    else:
        fill_normal(wl[:, :, :Kin], 1.0 / max(1.0, (Kin * max(len(e.taps or ()), d.ntaps)) ** 0.5), gen)
    wp = pack_weights(wl, d.dtype)
    keep.append(wp)
    d.w = wp.data_ptr()
    w64 = weight_values(wl, d.dtype)
    osc = osh = None
    if d.out_scale:
        osc = vec(N, "scale", gen, dev, exact)
        d.out_scale = osc.data_ptr()
    if d.out_shift:
        osh = vec(N, "shift", gen, dev, exact)
        d.out_shift = osh.data_ptr()
    # output: sentinel everywhere, integers at the written positions when accumulating
    yb = tensor_buf(d.y, ydt, dev)
    yb.t.fill_(SENTINEL)
    yfull = torch.as_strided(yb.t, (d.y.B, d.oT, d.oH, d.oW, N),
                             (d.y.sB, d.omT * d.y.H * d.y.W * d.y.ld, d.omH * d.y.W * d.y.ld, d.omW * d.y.ld, 1),
                             yb.lead + (d.ooT * d.y.H * d.y.W + d.ooH * d.y.W + d.ooW) * d.y.ld)
    if d.tline == 3:
        yfull = view_of(yb, d.y)
    if d.accumulate:
        old = torch.empty(yfull.shape, dtype=ydt, device=dev)
        fill_ints(old, -2, 2, gen) if exact else fill_normal(old, 1.0, gen)
        yfull.copy_(old)
        del old
    d.y.ptr = yb.ptr
    stats = None
    if d.stats:
        rows = lib.vinet_conv3d_stats_rows(C.byref(d))
        stats = torch.full((rows * 2 * N,), float("nan"), dtype=torch.float32, device=dev)
        d.stats = stats.data_ptr()
    ws = None
    if d.splitk_ws:
        nb = lib.vinet_conv3d_splitk_bytes(C.byref(d))
        ws = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=dev)
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), nb
    bnb = None
    if d.bnb_z:
        zb = Buf(d.bnb_z, span(d.y.B, d.y.T, d.y.H, d.y.W, d.y.C, d.bnb_ld, d.bnb_sB), ydt, dev)
        fill_ints(zb.t, -2, 2, gen) if exact else fill_normal(zb.t, 1.0, gen)
        fs = vec(N, "scale", gen, dev, exact) if d.bnb_fwd.scale else None
        fb = vec(N, "shift", gen, dev, exact) if d.bnb_fwd.shift else None
        mean = vec(N, "shift", gen, dev, exact)
        inv = vec(N, "scale", gen, dev, exact)
        d.bnb_z = zb.ptr
        d.bnb_fwd.scale = fs.data_ptr() if fs is not None else None
        d.bnb_fwd.shift = fb.data_ptr() if fb is not None else None
        d.bnb_mean, d.bnb_invstd = mean.data_ptr(), inv.data_ptr()
        part = None
        if d.bnb_partials:
            rows = lib.vinet_conv3d_bn_bwd_stats_rows(C.byref(d))
            assert rows > 0
            part = torch.full((rows * 2 * N,), float("nan"), dtype=torch.float32, device=dev)
            d.bnb_partials = part.data_ptr()
        bnb = (zb, fs, fb, mean, inv, part)

    # the route must be the census's
    kn = kernel_name("vinet_conv3d", d)
    if kn != e.kname:
        res.fail("replayed descriptor routes to %s, the step used %s" % (kn, e.kname))
        return res
    old_vals = yfull.clone() if d.accumulate else None
    rc = lib.vinet_conv3d(C.byref(d), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        res.fail("rc=%d: %s" % (rc, lib.vinet_last_error().decode()))
        return res
    torch.cuda.synchronize()

    # reference per checked item
    xall = view_of(xb, d.x)
    B = d.x.B
    items = items_to_check(B, [(span(d.x.B, d.x.T, d.x.H, d.x.W, d.x.C, d.x.ld, d.x.sB), d.x.sB),
                               (span(d.y.B, d.y.T, d.y.H, d.y.W, d.y.C, d.y.ld, d.y.sB), d.y.sB)])
    if only_items is not None:
        items = sorted(set(min(max(i if i >= 0 else B + i, 0), B - 1) for i in only_items))
    bm = lib.vinet_conv3d_tile_m(C.byref(d))
    M = B * d.oT * d.oH * d.oW
    last_tile0 = ((M - 1) // max(bm, 1)) * max(bm, 1)
    per_item = d.oT * d.oH * d.oW
    tol = None if exact else conv_tolerance(d, ydt)
    for b in items:
        xi = xall[b].double()
        if pre is not None:
            xi = affine64(xi, pre[0], pre[1], d.pre.relu, Cx, round_bf16=False)
        elif d.pre.relu:
            xi = xi.clamp_min(0)

        def full_ref(drop=None, zero_rows=None, shift=False):
            if d.tline == 3:
                acc, mag = conv_tsd_ref_item(d, xi, w64, drop)
            else:
                acc, mag = conv_ref_item(d, xi, w64, e.taps, drop)
            if Nw < N:
                acc = torch.cat([acc, acc.new_zeros(acc.shape[:-1] + (N - Nw,))], -1)
                mag = torch.cat([mag, mag.new_zeros(mag.shape[:-1] + (N - Nw,))], -1)
            if osc is not None:
                acc[..., :Nw] *= osc[:Nw].double()
                mag[..., :Nw] *= osc[:Nw].double()
            if osh is not None:
                acc[..., :Nw] += osh[:Nw].double()
                mag[..., :Nw] += osh[:Nw].double().abs()
            if zero_rows is not None:
                acc.reshape(-1, N)[zero_rows] = 0
            if shift:
                acc = acc.reshape(-1, N).roll(1, 0).reshape(acc.shape)
            acc = act64(acc, d.act)
            if d.accumulate:
                acc = acc + old_vals[b].double()
            return acc, mag

        ref, mag = full_ref()
        if exact:
            assert float(mag.max()) < EXACT, "exactness bound: sum |terms| = %g reaches 2^24" % float(mag.max())
            if d.act == L.ACT_SIGMOID:
                res.exact = False
        got = yfull[b]
        exact_here = exact and d.act != L.ACT_SIGMOID
        tol_here = tol if tol is not None else (lambda r, m_: 2.0 ** -8 * r.abs() + 2.0 ** -20)
        msg = compare(got, ref, mag, exact_here, ydt, tol_here)
        res.checked += 1
        if msg:
            res.fail("item %d: %s" % (b, msg))
            continue
        if selftest and b in (items[-1],):
            # the comparison must reject deliberately wrong references
            lo_m = b * per_item
            rows = [r - lo_m for r in range(max(last_tile0, lo_m), min(M, lo_m + per_item))]
            muts = [("dropped K chunk", dict(drop=(len(e.taps or [0] * d.ntaps) // 2, 0))),
                    ("one-voxel shift", dict(shift=True))]
            if rows:
                muts.append(("last M tile dropped", dict(zero_rows=torch.tensor(rows, device=dev))))
            else:
                res.notes.append("last M tile not in item %d" % b)
            for what, kw in muts:
                r2, _ = full_ref(**kw)
                if compare(got, r2, mag, exact_here, ydt, tol_here) is None:
                    res.selftest.append("%r: the check accepted a reference with %s" % (e, what))
    # untouched storage: padding channels, other channels of a concat buffer, frames outside the om / oo phase
    written = yfull.clone()
    yfull.fill_(SENTINEL)
    stray = (yb.t != SENTINEL)
    if bool(stray.any()):
        res.fail("%d elements outside the output view changed, first at flat %d" % (int(stray.sum()), int(stray.nonzero()[0, 0])))
    yfull.copy_(written)
    del stray
    # statistics of the pre-activation output, against float64 sums over the stored values
    if stats is not None:
        assert d.act == L.ACT_NONE and not d.accumulate, "stats with an activation / accumulate: the stored values are not the summed ones"
        st = stats.view(-1, 2, N).double().sum(0)
        s1 = torch.zeros(N, dtype=torch.float64, device=dev)
        s2 = torch.zeros_like(s1)
        sa = torch.zeros_like(s1)
        for b in range(B):
            v = written[b].reshape(-1, N).double()
            s1 += v.sum(0)
            s2 += (v * v).sum(0)
            sa += v.abs().sum(0)
        # the kernel sums fp32 values before the output rounding: one rounding of the stored dtype per element (2^-8 / 2^-23,
        # on sum |y| and on 2 * sum y^2) plus fp32 accumulation inside a tile (2^-16 of the magnitude)
        r = _out_round(ydt) + 2.0 ** -16
        if not bool(((st[0] - s1).abs() <= r * sa + 1e-6).all()) or not bool(((st[1] - s2).abs() <= 2.5 * r * s2 + 1e-6).all()):
            res.fail("stats: sums %s / %s vs %s / %s" % (st[0][:4].tolist(), st[1][:4].tolist(), s1[:4].tolist(), s2[:4].tolist()))
        res.exact = False
    if bnb is not None and bnb[5] is not None:
        zb, fs, fb, mean, inv, part = bnb
        P = part.view(-1, 2, N).double().sum(0)
        zall = zb.view5(d.y.B, d.y.T, d.y.H, d.y.W, N, d.bnb_ld, d.bnb_sB)
        s1 = torch.zeros(N, dtype=torch.float64, device=dev)
        s2, a1, a2 = torch.zeros_like(s1), torch.zeros_like(s1), torch.zeros_like(s1)
        for b in range(B):
            gq = written[b].reshape(-1, N).double() if d.tline != 3 else view_of(yb, d.y)[b].reshape(-1, N).double()
            z = zall[b].reshape(-1, N).double()
            if d.bnb_fwd.relu:
                zz = z * fs.double()[:N] + fb.double()[:N] if fs is not None else z
                gq = gq * (zz > 0)
            xh = (z - mean.double()[:N]) * inv.double()[:N]
            s1 += gq.sum(0)
            s2 += (gq * xh).sum(0)
            a1 += gq.abs().sum(0)
            a2 += (gq * xh).abs().sum(0)
        # fp32 products (z - mean) * invstd and tile sums: 2^-16 of the magnitudes
        if not bool(((P[0] - s1).abs() <= 2.0 ** -16 * a1 + 1e-6).all()) or not bool(((P[1] - s2).abs() <= 2.0 ** -16 * a2 + 1e-6).all()):
            res.fail("bnb_partials: %s / %s vs %s / %s" % (P[0][:4].tolist(), P[1][:4].tolist(), s1[:4].tolist(), s2[:4].tolist()))
        res.exact = False
    del keep
    return res


# ---- weight-gradient replay -------------------------------------------------------------------------------------------
def wgrad_tile_rows(kname, oH, oW):
    """M rows of the last tile of a weight-gradient route (by its kernel name): one frame for the frame-streaming kernels
    (conv_wgrad_ts / _tf), one image row for the row-streaming ones (conv_wgrad_rs / _hs), 32 voxels -- the M step of
    the tiled kernels (conv_wgrad_dma / _pp, wgrad_skinny, the generic one) -- otherwise.  Every one of them ends at M - 1."""
    if kname.startswith(("conv_wgrad_ts_kernel", "conv_wgrad_tf_kernel")):
        return oH * oW
    if kname.startswith(("conv_wgrad_rs_kernel", "conv_wgrad_hs_kernel")):
        return oW
    return 32


def sparse_rows(M, oW, gen, dev):
    """rows of dy that carry values: the first and last row of every 32-row block (so of every M tile whose height is a
    multiple of 32: 32, 64, 192, 256), the first and last position of every image row (the row- and frame-streaming kernels'
    tiles: frames are whole image rows), a seeded 1/512 of the rest, and row M-1"""
    m = torch.arange(M, device=dev)
    sel = (m % 32 == 0) | (m % 32 == 31) | (m == M - 1)
    w = m % oW
    sel |= (w == 0) | (w == oW - 1)
    sel |= torch.rand(M, generator=gen, device=dev) < (1.0 / 512)
    return sel.nonzero().squeeze(1)


def _sparse_pm1(shape, q, gen, dev):
    """{-1, 0, 1} with P(nonzero) = q"""
    u = torch.rand(shape, generator=gen, device=dev)
    return torch.where(u < q / 2, -1.0, torch.where(u < q, 1.0, 0.0))


def replay_wgrad(e, seed, selftest=True):
    """re-launch weight-gradient census entry `e` on a sparse integer dy; returns a Result"""
    lib = L.get()
    dev = torch.device("cuda:0")
    d = L.CWgradDesc.from_buffer_copy(e.desc)
    res = Result(e, "exact")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    xdt = TDT[d.dtype]
    keep = []
    xb = tensor_buf(d.x, xdt, dev)
    fill_ints(xb.t, -2, 2, gen)
    d.x.ptr = xb.ptr
    Cx = d.x.C
    pre = None
    if d.pre.scale:
        ps, pb = vec(Cx, "scale", gen, dev, True), vec(Cx, "shift", gen, dev, True)
        d.pre.scale, d.pre.shift = ps.data_ptr(), pb.data_ptr()
        pre = (ps, pb)
        keep += [ps, pb]
    B, oT, oH, oW, N = d.dy.B, d.dy.T, d.dy.H, d.dy.W, d.dy.C
    M = B * oT * oH * oW
    rows = sparse_rows(M, oW, gen, dev)
    nnz = rows.numel()
    # values: {-1, 0, 1} per channel, nonzero with probability q (about 2^20 values per channel at most, so that every sum
    # stays far below 2^24); the first channel of every selected row is +-1
    q = min(2.0 / 3.0, float(1 << 20) / nnz)
    vals = _sparse_pm1((nnz, N), q, gen, dev)
    vals[:, 0] = torch.where(torch.rand(nnz, generator=gen, device=dev) < 0.5, -1.0, 1.0)
    b_ = rows // (oT * oH * oW)
    r_ = rows % (oT * oH * oW)
    t_, h_, w_ = r_ // (oH * oW), (r_ // oW) % oH, r_ % oW
    dyb = tensor_buf(d.dy, xdt, dev)
    dyb.t.zero_()
    off = dyb.lead + b_ * d.dy.sB + ((t_ * oH + h_) * oW + w_) * d.dy.ld
    dz = vals.double()
    if d.bnb_z:
        # fused BatchNorm backward: dz = scale * (dy * mask - c1 - (z - mean) * invstd * c2), rounded to the activation dtype.
        # mean in {-1, 0, 1}, invstd in {1, 2}, c2 in {-1, 0, 1}, c1 in {-1, 0, 1} (0 where c2 = 0).  Every voxel's z is
        # z0 = mean - c1 / (invstd * c2) (mean where c2 = 0; a multiple of 1/2, exact in bf16), for which the c1 and the
        # (z - mean) terms cancel exactly, plus a sparse +-1 on the selected rows: the rows without dy values stay exactly 0
        # (so every sum stays exact) only if the kernel applies mean, invstd, c1 and c2 as the contract says -- one that
        # ignored any of them would add a dense term over all M rows.
        zb = Buf(d.bnb_z, span(B, oT, oH, oW, N, d.bnb_ld, d.bnb_sB), xdt, dev)
        fs = vec(N, "scale", gen, dev, True)
        fb = vec(N, "shift", gen, dev, True)
        mean = vec(N, "shift", gen, dev, True)
        inv = vec(N, "scale", gen, dev, True)
        c2 = vec(N, "shift", gen, dev, True)
        c1 = vec(N, "shift", gen, dev, True) * (c2 != 0)
        z0 = mean[:N].double() - torch.where(c2[:N] != 0, c1[:N].double() / (inv[:N].double() * c2[:N].double()),
                                             torch.zeros_like(c1[:N].double()))
        zb.t.fill_(SENTINEL)
        zb.view5(B, oT, oH, oW, N, d.bnb_ld, d.bnb_sB).copy_(z0.to(xdt).expand(B, oT, oH, oW, N))
        delta = _sparse_pm1((nnz, N), q, gen, dev).double()
        z64 = z0[None, :] + delta
        zoff = zb.lead + b_ * d.bnb_sB + ((t_ * oH + h_) * oW + w_) * d.bnb_ld
        zb.t[(zoff[:, None] + torch.arange(N, device=dev)[None, :]).reshape(-1)] = z64.reshape(-1).to(xdt)
        keep += [zb, fs, fb, mean, inv, c1, c2]
        d.bnb_z = zb.ptr
        d.bnb_fwd.scale, d.bnb_fwd.shift = fs.data_ptr(), fb.data_ptr()
        d.bnb_mean, d.bnb_invstd, d.bnb_c1, d.bnb_c2 = mean.data_ptr(), inv.data_ptr(), c1.data_ptr(), c2.data_ptr()
        g = dz
        if d.bnb_fwd.relu:
            g = g * ((z64 * fs[:N].double() + fb[:N].double()) > 0)
        dz = fs[:N].double() * (g - c1[:N].double() - (z64 - mean[:N].double()) * inv[:N].double() * c2[:N].double())
        assert float(dz.abs().max()) <= 16 and bool((dz == dz.round()).all()), "fused BN backward: dz must be a small integer"
    dyb.t[(off[:, None] + torch.arange(N, device=dev)[None, :]).reshape(-1)] = vals.reshape(-1).to(xdt)
    d.dy.ptr = dyb.ptr
    nsl = max(r[3] for r in e.taps) + 1
    tt = torch.tensor(e.taps, dtype=torch.int32, device=dev).reshape(-1)
    keep.append(tt)
    d.taps = tt.data_ptr()
    dw = torch.zeros(nsl * N * d.Kp, dtype=torch.float32, device=dev)
    d.dw = dw.data_ptr()
    kn = kernel_name("vinet_conv3d_wgrad", d)
    if kn != e.kname:
        res.fail("replayed descriptor routes to %s, the step used %s" % (kn, e.kname))
        return res
    rc = lib.vinet_conv3d_wgrad(C.byref(d), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        res.fail("rc=%d: %s" % (rc, lib.vinet_last_error().decode()))
        return res
    torch.cuda.synchronize()
    got = dw.view(nsl, N, d.Kp)

    # float64 reference over the rows that carry values
    x5 = view_of(xb, d.x)

    def xg_at(dt_, dh_, dw_, extra_w=0):
        ti, hi, wi = t_ * d.sT + dt_, h_ * d.sH + dh_, w_ * d.sW + dw_ + extra_w
        ok = (ti >= 0) & (ti < d.x.T) & (hi >= 0) & (hi < d.x.H) & (wi >= 0) & (wi < d.x.W)
        v = x5[b_, ti.clamp(0, d.x.T - 1), hi.clamp(0, d.x.H - 1), wi.clamp(0, d.x.W - 1)].double()
        if pre is not None:
            v = affine64(v, pre[0], pre[1], d.pre.relu, Cx)
        elif d.pre.relu:
            v = v.clamp_min(0)
        return v * ok[:, None]

    def reference(drop=None, last_tile=False, shift=0):
        ref = torch.zeros((nsl, N, d.Kp), dtype=torch.float64, device=dev)
        mag = torch.zeros_like(ref)
        tile = wgrad_tile_rows(e.kname, oH, oW)
        keep_rows = rows < ((M - 1) // tile) * tile if last_tile else None
        dzz = dz if keep_rows is None else dz * keep_rows[:, None]
        for k, (dt_, dh_, dw_, sl) in enumerate(e.taps):
            if d.mode == 0:
                xg = xg_at(dt_, dh_, dw_ + shift)
                part = dzz.T @ xg
                if drop is not None and drop[0] == k:
                    part[:, 32 * drop[1]:32 * drop[1] + 32] = 0
                ref[sl, :, :Cx] += part
                mag[sl, :, :Cx] += dzz.abs().T @ xg.abs()
            else:
                if drop is not None and drop[0] == k:
                    continue        # (a stem-mode K chunk is the tap's whole 8 positions x 4 channels)
                for p in range(8):
                    xg = xg_at(dt_, dh_, dw_ + shift, p)
                    ref[sl, :, 4 * p:4 * p + 4] += dzz.T @ xg[:, :4]
                    mag[sl, :, 4 * p:4 * p + 4] += dzz.abs().T @ xg[:, :4].abs()
        return ref, mag

    ref, mag = reference()
    worst = float(mag.max())
    assert worst < EXACT, "%r: exactness bound: sum |terms| = %g reaches 2^24" % (e, worst)
    res.notes.append("%d of %d rows carry dy; max sum |terms| %g" % (nnz, M, worst))
    res.checked = 1
    # (columns past x.C of a K chunk are padding: vinet_unpack_wgrad never reads them)
    got = got[:, :, :Cx] if d.mode == 0 else got
    ref, mag = (ref[:, :, :Cx], mag[:, :, :Cx]) if d.mode == 0 else (ref, mag)
    exp = ref.to(torch.float32)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i = tuple(bad[0].tolist())
        res.fail("dw: %d of %d entries differ, first at (slice, n, c) %s (got %r, expected %r)"
                 % (bad.shape[0], got.numel(), list(i), got[i].item(), exp[i].item()))
        return res
    if selftest:
        muts = [("dropped K chunk", dict(drop=(len(e.taps) // 2, 0))), ("last M tile dropped", dict(last_tile=True)),
                ("one-voxel shift", dict(shift=1))]
        for what, kw in muts:
            r2, _ = reference(**kw)
            r2 = r2[:, :, :Cx] if d.mode == 0 else r2
            if torch.equal(got, r2.to(torch.float32)):
                res.selftest.append("%r: the check accepted a reference with %s" % (e, what))
    del keep
    return res


# ---- the large non-conv launches --------------------------------------------------------------------------------------
def largest(entries, name):
    """the census entry of `name` with the most elements in its largest tensor argument"""
    cands = [e for e in entries if e.name == name]
    if not cands:
        return None

    def size(e):
        return max(span(t.B, t.T, t.H, t.W, t.C, t.ld, t.sB) for t in e.args if isinstance(t, L.CTensor))
    return max(cands, key=size)


def _fresh(ct, tdt, gen, dev, lo=-2, hi=2, fill=None):
    b = tensor_buf(ct, tdt, dev)
    if fill is None:
        fill_ints(b.t, lo, hi, gen)
    else:
        b.t.fill_(fill)
    c = L.CTensor.from_buffer_copy(ct)
    c.ptr = b.ptr
    return b, c


def _items(*cts):
    B = cts[0].B
    return items_to_check(B, [(span(t.B, t.T, t.H, t.W, t.C, t.ld, t.sB), t.sB) for t in cts])


def _eq(got, ref64, what, errs):
    msg = compare(got, ref64, None, True, got.dtype)
    if msg:
        errs.append("%s: %s" % (what, msg))


def _bn_terms(g, z, fs, fb, relu, mean, inv, Cc):
    if relu:
        zz = z * fs[:Cc].double() + fb[:Cc].double() if fs is not None else z
        g = g * (zz > 0)
    return g, (z - mean[:Cc].double()) * inv[:Cc].double()


def replay_bn_bwd(e, seed):
    """vinet_bn_bwd_apply (elementwise: exact on the checked items) or vinet_bn_bwd_reduce (per-channel sums over the whole
    tensor against float64, bound 2^-16 of sum |terms|: fp32 products (z - mean) * invstd and fp32 sums inside a row)"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    dzc, xc = e.args[0], e.args[1]
    dt, fwd = e.args[2], e.args[3]
    tdt = TDT[dt]
    Cc = xc.C
    dzb, dzc = _fresh(dzc, tdt, gen, dev)
    xb, xc = _fresh(xc, tdt, gen, dev)
    fs = vec(Cc, "scale", gen, dev, True) if fwd.scale else None
    fb = vec(Cc, "shift", gen, dev, True) if fwd.shift else None
    f = L.CAffine(fs.data_ptr() if fs is not None else None, fb.data_ptr() if fb is not None else None, fwd.relu)
    mean, inv = vec(Cc, "shift", gen, dev, True), vec(Cc, "scale", gen, dev, True)
    errs = []
    st = torch.cuda.current_stream().cuda_stream
    if e.name == "vinet_bn_bwd_apply":
        c1, c2 = vec(Cc, "shift", gen, dev, True), vec(Cc, "shift", gen, dev, True)
        dxb, dxc = _fresh(e.args[8], tdt, gen, dev, fill=SENTINEL)
        rc = lib.vinet_bn_bwd_apply(C.byref(dzc), C.byref(xc), dt, f, mean.data_ptr(), inv.data_ptr(), c1.data_ptr(),
                                    c2.data_ptr(), C.byref(dxc), st)
        assert rc == 0, lib.vinet_last_error()
        torch.cuda.synchronize()
        for b in _items(dzc, xc, dxc):
            g, xh = _bn_terms(view_of(dzb, dzc)[b].double(), view_of(xb, xc)[b].double(), fs, fb, fwd.relu, mean, inv, Cc)
            ref = (fs[:Cc].double() if fs is not None else 1.0) * (g - c1[:Cc].double() - xh * c2[:Cc].double())
            _eq(view_of(dxb, dxc)[b], ref, "%r item %d" % (e, b), errs)
        return errs
    rows = lib.vinet_stats_rows(C.byref(xc))
    P = torch.full((rows * 2 * Cc,), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.vinet_bn_bwd_reduce(C.byref(dzc), C.byref(xc), dt, f, mean.data_ptr(), inv.data_ptr(), P.data_ptr(), st)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    s = torch.zeros((4, Cc), dtype=torch.float64, device=dev)
    for b in range(xc.B):
        g, xh = _bn_terms(view_of(dzb, dzc)[b].reshape(-1, Cc).double(), view_of(xb, xc)[b].reshape(-1, Cc).double(),
                          fs, fb, fwd.relu, mean, inv, Cc)
        s[0] += g.sum(0)
        s[1] += (g * xh).sum(0)
        s[2] += g.abs().sum(0)
        s[3] += (g * xh).abs().sum(0)
    got = P.view(rows, 2, Cc).double().sum(0)
    for k in range(2):
        if not bool(((got[k] - s[k]).abs() <= 2.0 ** -16 * s[k + 2] + 1e-6).all()):
            errs.append("%r: sum %d: %s vs %s" % (e, k, got[k][:4].tolist(), s[k][:4].tolist()))
    return errs


def _untouched(b, ct, what, errs):
    """everything of b outside the view ct still holds SENTINEL (call after the view's own check: it is overwritten)"""
    view_of(b, ct).fill_(SENTINEL)
    if bool((b.t != SENTINEL).any()):
        errs.append("%s: elements outside the view changed" % what)


def _dyadic(t, bits, gen):
    """multiples of 2^-bits in [-2, 2]: values whose bf16 split leaves a nonzero lo plane, every step of the contract's
    arithmetic still exact (at most 2 + bits + a few significant bits)"""
    fill_ints(t, -(2 << bits), 2 << bits, gen)
    return t.mul_(2.0 ** -bits)


def _split_ref(v):
    """hi = bf16(v), lo = bf16(v - hi) in float64 (exact for the dyadic data above)"""
    hi = to_dtype_exact(v, torch.bfloat16).double()
    return hi, v - hi


def replay_bn_bwd_apply_split(e, seed):
    """vinet_bn_bwd_apply_split (fp32: the fp32s step's BatchNorm-backward apply): dx = scale * (dz * mask - c1 - (z - mean)
    * invstd * c2) and its planes hi = bf16(dx), lo = bf16(dx - hi).  dz in multiples of 2^-8, z and the coefficients
    integers: dx has at most 13 significant bits, so dx, hi and lo are exact and must match bit for bit on the checked items"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    dzc, xc, fwd = e.args[0], e.args[1], e.args[2]
    Cc = xc.C
    dzb, dzc = _fresh(dzc, torch.float32, gen, dev)
    _dyadic(dzb.t, 8, gen)
    xb, xc = _fresh(xc, torch.float32, gen, dev)
    fs = vec(Cc, "scale", gen, dev, True)
    fb = vec(Cc, "shift", gen, dev, True) if fwd.shift else None
    f = L.CAffine(fs.data_ptr(), fb.data_ptr() if fb is not None else None, fwd.relu)
    mean, inv = vec(Cc, "shift", gen, dev, True), vec(Cc, "scale", gen, dev, True)
    c1, c2 = vec(Cc, "shift", gen, dev, True), vec(Cc, "shift", gen, dev, True)
    dxb, dxc = _fresh(e.args[7], torch.float32, gen, dev, fill=SENTINEL)
    hib, hic = _fresh(e.args[8], torch.bfloat16, gen, dev, fill=SENTINEL)
    lob, loc = _fresh(e.args[9], torch.bfloat16, gen, dev, fill=SENTINEL)
    rc = lib.vinet_bn_bwd_apply_split(C.byref(dzc), C.byref(xc), f, mean.data_ptr(), inv.data_ptr(), c1.data_ptr(),
                                      c2.data_ptr(), C.byref(dxc), C.byref(hic), C.byref(loc), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    errs = []
    for b in _items(dzc, xc, dxc):
        g, xh = _bn_terms(view_of(dzb, dzc)[b].double(), view_of(xb, xc)[b].double(), fs, fb, fwd.relu, mean, inv, Cc)
        ref = fs[:Cc].double() * (g - c1[:Cc].double() - xh * c2[:Cc].double())
        hi, lo = _split_ref(ref)
        _eq(view_of(dxb, dxc)[b], ref, "%r dx item %d" % (e, b), errs)
        _eq(view_of(hib, hic)[b], hi, "%r hi item %d" % (e, b), errs)
        _eq(view_of(lob, loc)[b], lo, "%r lo item %d" % (e, b), errs)
    if not bool((view_of(lob, loc)[-1] != 0).any()):
        errs.append("%r: the data left the lo plane empty (the test would not see it)" % e)
    for b_, c_, w_ in ((dxb, dxc, "dx"), (hib, hic, "hi"), (lob, loc, "lo")):
        _untouched(b_, c_, "%r %s" % (e, w_), errs)
    return errs


def replay_split_bf16(e, seed):
    """vinet_split_bf16 (the fp32s step's hi / lo operand planes of x, with its pending affine, and of dy): v = pre(src),
    hi = bf16(v), lo = bf16(v - hi).  src in multiples of 2^-12, scale / shift integers: v has at most 15 significant bits,
    hi and lo are exact and must match bit for bit on the checked items (the items past element 2^31 included)"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    src, pre = e.args[0], e.args[1]
    sb, sc = _fresh(src, torch.float32, gen, dev)
    _dyadic(sb.t, 12, gen)
    Cc = src.C
    ps = vec(Cc, "scale", gen, dev, True) if pre.scale else None
    pb = vec(Cc, "shift", gen, dev, True) if pre.shift else None
    a = L.CAffine(ps.data_ptr() if ps is not None else None, pb.data_ptr() if pb is not None else None, pre.relu)
    hib, hic = _fresh(e.args[2], torch.bfloat16, gen, dev, fill=SENTINEL)
    lob, loc = _fresh(e.args[3], torch.bfloat16, gen, dev, fill=SENTINEL)
    rc = lib.vinet_split_bf16(C.byref(sc), a, C.byref(hic), C.byref(loc), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    errs = []
    for b in _items(sc, hic, loc):
        v = view_of(sb, sc)[b].double()
        v = affine64(v, ps, pb, pre.relu, Cc) if ps is not None else (v.clamp_min(0) if pre.relu else v)
        hi, lo = _split_ref(v)
        _eq(view_of(hib, hic)[b], hi, "%r hi item %d" % (e, b), errs)
        _eq(view_of(lob, loc)[b], lo, "%r lo item %d" % (e, b), errs)
    if not bool((view_of(lob, loc)[-1] != 0).any()):
        errs.append("%r: the data left the lo plane empty (the test would not see it)" % e)
    for b_, c_, w_ in ((hib, hic, "hi"), (lob, loc, "lo")):
        _untouched(b_, c_, "%r %s" % (e, w_), errs)
    return errs


def replay_channel_stats(e, seed):
    """vinet_channel_stats: (sum, sum of squares) per channel over the whole tensor vs float64 (integer data: the fp32 row
    sums are exact below 2^24; the bound 2^-20 of the magnitude covers longer rows)"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    dt = e.args[1]
    xb, xc = _fresh(e.args[0], TDT[dt], gen, dev)
    Cc = xc.C
    rows = lib.vinet_stats_rows(C.byref(xc))
    P = torch.full((rows * 2 * Cc,), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.vinet_channel_stats(C.byref(xc), dt, P.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    s = torch.zeros((2, Cc), dtype=torch.float64, device=dev)
    for b in range(xc.B):
        v = view_of(xb, xc)[b].reshape(-1, Cc).double()
        s[0] += v.sum(0)
        s[1] += (v * v).sum(0)
    got = P.view(rows, 2, Cc).double().sum(0)
    errs = []
    mag = torch.stack([s[1], s[1]])     # sum |x| <= sum x^2 for integers
    if not bool(((got - s).abs() <= 2.0 ** -20 * mag + 1e-6).all()):
        errs.append("%r: %s vs %s" % (e, got[:, :4].tolist(), s[:, :4].tolist()))
    return errs


def replay_copy_affine(e, seed):
    """vinet_copy_affine: dst (+)= pre(src), exact on integers, checked items + everything outside dst untouched"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    src, sdt, pre, dst, ddt, acc = e.args[:6]
    sb, sc = _fresh(src, TDT[sdt], gen, dev)
    db, dc = _fresh(dst, TDT[ddt], gen, dev, fill=SENTINEL)
    old = None
    if acc:
        old = torch.empty(view_of(db, dc).shape, dtype=TDT[ddt], device=dev)
        fill_ints(old, -2, 2, gen)
        view_of(db, dc).copy_(old)
    Cc = src.C
    ps = vec(Cc, "scale", gen, dev, True) if pre.scale else None
    pb = vec(Cc, "shift", gen, dev, True) if pre.shift else None
    a = L.CAffine(ps.data_ptr() if ps is not None else None, pb.data_ptr() if pb is not None else None, pre.relu)
    rc = lib.vinet_copy_affine(C.byref(sc), sdt, a, C.byref(dc), ddt, acc, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    errs = []
    for b in _items(sc, dc):
        ref = affine64(view_of(sb, sc)[b].double(), ps, pb, pre.relu, Cc) if ps is not None else view_of(sb, sc)[b].double()
        if ps is None and pre.relu:
            ref = ref.clamp_min(0)
        if old is not None:
            ref = ref + old[b].double()
        _eq(view_of(db, dc)[b], ref, "%r item %d" % (e, b), errs)
    v = view_of(db, dc)
    v.fill_(SENTINEL)
    if bool((db.t != SENTINEL).any()):
        errs.append("%r: elements outside dst changed" % e)
    return errs


def _pool_windows(xi, pd, oT, oH, oW):
    """(max, first argmax in (t, h, w) scan order) of one item, -inf padding"""
    dev = xi.device
    best = torch.full((oT, oH, oW, xi.shape[-1]), float("-inf"), dtype=torch.float64, device=dev)
    arg = torch.zeros(best.shape, dtype=torch.int64, device=dev)
    k = 0
    for kt in range(pd.kT):
        for kh in range(pd.kH):
            for kw in range(pd.kW):
                g = gathered(xi, pd.sT, pd.sH, pd.sW, kt - pd.pT, kh - pd.pH, kw - pd.pW, oT, oH, oW)
                ok = gathered(torch.ones_like(xi[..., :1]), pd.sT, pd.sH, pd.sW, kt - pd.pT, kh - pd.pH, kw - pd.pW, oT, oH, oW) > 0
                g = torch.where(ok, g, torch.full_like(g, float("-inf")))
                better = g > best
                best = torch.where(better, g, best)
                arg = torch.where(better, torch.full_like(arg, k), arg)
                k += 1
    return best, arg


def replay_maxpool(e, seed):
    """vinet_maxpool3d: max and argmax (first maximum wins: integer data has many ties) exact on the checked items;
    vinet_maxpool3d_bwd: dx (+)= the gather of dy through a fresh argmax, exact on the checked items"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    pd = e.args[0]
    tdt = TDT[pd.dtype]
    st = torch.cuda.current_stream().cuda_stream
    errs = []
    if e.name == "vinet_maxpool3d":
        xc0, pre, yc0 = e.args[1], e.args[2], e.args[3]
        xb, xc = _fresh(xc0, tdt, gen, dev)
        yb, yc = _fresh(yc0, tdt, gen, dev, fill=SENTINEL)
        Cc = xc.C
        ps = vec(Cc, "scale", gen, dev, True) if pre.scale else None
        pb = vec(Cc, "shift", gen, dev, True) if pre.shift else None
        a = L.CAffine(ps.data_ptr() if ps is not None else None, pb.data_ptr() if pb is not None else None, pre.relu)
        am = torch.full((yc.B * yc.T * yc.H * yc.W * yc.C,), 255, dtype=torch.uint8, device=dev) if e.args[4] else None
        rc = lib.vinet_maxpool3d(C.byref(pd), C.byref(xc), a, C.byref(yc), am.data_ptr() if am is not None else None, st)
        assert rc == 0, lib.vinet_last_error()
        torch.cuda.synchronize()
        for b in _items(xc, yc):
            xi = view_of(xb, xc)[b].double()
            if ps is not None:
                xi = affine64(xi, ps, pb, pre.relu, Cc)
            elif pre.relu:
                xi = xi.clamp_min(0)
            best, arg = _pool_windows(xi, pd, yc.T, yc.H, yc.W)
            _eq(view_of(yb, yc)[b], best, "%r item %d" % (e, b), errs)
            if am is not None:
                n = yc.T * yc.H * yc.W * yc.C
                got = am[b * n:(b + 1) * n].view(arg.shape).long()
                if not torch.equal(got, arg):
                    errs.append("%r item %d: argmax differs at %d positions" % (e, b, int((got != arg).sum())))
        return errs
    dyc0, dxc0, acc = e.args[1], e.args[3], e.args[4]
    dyb, dyc = _fresh(dyc0, tdt, gen, dev)
    dxb, dxc = _fresh(dxc0, tdt, gen, dev, fill=SENTINEL)
    old = None
    if acc:
        old = torch.empty(view_of(dxb, dxc).shape, dtype=tdt, device=dev)
        fill_ints(old, -2, 2, gen)
        view_of(dxb, dxc).copy_(old)
    # a fresh argmax: a window tap whose input position lies inside dx (what a forward pass can produce)
    k = pd.kT * pd.kH * pd.kW
    n = dyc.B * dyc.T * dyc.H * dyc.W * dyc.C
    am = torch.empty(n, dtype=torch.uint8, device=dev)
    shp = (dyc.B, dyc.T, dyc.H, dyc.W, dyc.C)
    r = torch.randint(0, k, shp, generator=gen, device=dev)
    ot = torch.arange(dyc.T, device=dev).view(1, -1, 1, 1, 1)
    oh = torch.arange(dyc.H, device=dev).view(1, 1, -1, 1, 1)
    ow = torch.arange(dyc.W, device=dev).view(1, 1, 1, -1, 1)

    def pos(tap):
        kt, kh, kw = tap // (pd.kH * pd.kW), (tap // pd.kW) % pd.kH, tap % pd.kW
        return ot * pd.sT - pd.pT + kt, oh * pd.sH - pd.pH + kh, ow * pd.sW - pd.pW + kw

    ti, hi, wi = pos(r)
    bad = (ti < 0) | (ti >= dxc.T) | (hi < 0) | (hi >= dxc.H) | (wi < 0) | (wi >= dxc.W)
    # (replace out-of-range taps by the window's centre-most in-range tap: the centre (pT, pH, pW) is always inside)
    centre = (pd.pT * pd.kH + pd.pH) * pd.kW + pd.pW
    r = torch.where(bad, torch.full_like(r, centre), r)
    am.copy_(r.reshape(-1).to(torch.uint8))
    del bad
    rc = lib.vinet_maxpool3d_bwd(C.byref(pd), C.byref(dyc), am.data_ptr(), C.byref(dxc), acc, st)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    for b in _items(dyc, dxc):
        rb = r[b]
        ti, hi, wi = pos(rb)
        ti, hi, wi = ti[0], hi[0], wi[0]
        ref = torch.zeros((dxc.T, dxc.H, dxc.W, dxc.C), dtype=torch.float64, device=dev)
        cc = torch.arange(dxc.C, device=dev).view(1, 1, 1, -1)
        flat = ((ti * dxc.H + hi) * dxc.W + wi) * dxc.C + cc
        ref.view(-1).index_add_(0, flat.reshape(-1), view_of(dyb, dyc)[b].double().reshape(-1))
        if old is not None:
            ref = ref + old[b].double()
        _eq(view_of(dxb, dxc)[b], ref, "%r item %d" % (e, b), errs)
    return errs


def _up64(xi):
    """nn.Upsample((1, 2, 2), trilinear, align_corners=False) of one item [T][H][W][C] in float64"""
    v = xi.permute(3, 0, 1, 2).unsqueeze(0)
    return torch.nn.functional.interpolate(v, scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)[0].permute(1, 2, 3, 0)


def replay_upsample(e, seed):
    """vinet_upsample2x / vinet_upsample2x_bwd_relu: integer data, weights 1/4 and 3/4 -> every value a multiple of 1/16
    below 64 in magnitude: exact in float64 and in bf16, so the checked items must match bit for bit"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    st = torch.cuda.current_stream().cuda_stream
    errs = []
    if e.name == "vinet_upsample2x":
        xc0, yc0, dt = e.args[:3]
        xb, xc = _fresh(xc0, TDT[dt], gen, dev)
        yb, yc = _fresh(yc0, TDT[dt], gen, dev, fill=SENTINEL)
        rc = lib.vinet_upsample2x(C.byref(xc), C.byref(yc), dt, st)
        assert rc == 0, lib.vinet_last_error()
        torch.cuda.synchronize()
        for b in _items(xc, yc):
            _eq(view_of(yb, yc)[b], _up64(view_of(xb, xc)[b].double()), "%r item %d" % (e, b), errs)
        return errs
    dyc0, dxc0, xfc0, dt = e.args[:4]
    dyb, dyc = _fresh(dyc0, TDT[dt], gen, dev)
    dxb, dxc = _fresh(dxc0, TDT[dt], gen, dev, fill=SENTINEL)
    xfb, xfc = _fresh(xfc0, TDT[dt], gen, dev)
    rc = lib.vinet_upsample2x_bwd_relu(C.byref(dyc), C.byref(dxc), C.byref(xfc), dt, st)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    for b in _items(dyc, dxc):
        xi = torch.zeros((dxc.T, dxc.H, dxc.W, dxc.C), dtype=torch.float64, device=dev, requires_grad=True)
        gx, = torch.autograd.grad(_up64(xi), xi, view_of(dyb, dyc)[b].double())
        ref = gx * (view_of(xfb, xfc)[b].double() > 0)
        _eq(view_of(dxb, dxc)[b], ref, "%r item %d" % (e, b), errs)
    return errs


def replay_import_pad(e, seed):
    """vinet_import_ncdhw_pad: strided fp32 NCDHW source -> zero-padded channels-last dst, exact on the checked items"""
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    _, sb_, sc_, st_, sh_, sw_, Cc, Hs, Ws, pt, pl, dst, ddt = e.args[:13]
    n = (dst.B - 1) * sb_ + (Cc - 1) * sc_ + (dst.T - 1) * st_ + (Hs - 1) * sh_ + (Ws - 1) * sw_ + 1
    src = fill_ints(torch.empty(n, dtype=torch.float32, device=dev), -2, 2, gen)
    db, dc = _fresh(dst, TDT[ddt], gen, dev, fill=SENTINEL)
    rc = lib.vinet_import_ncdhw_pad(src.data_ptr(), sb_, sc_, st_, sh_, sw_, Cc, Hs, Ws, pt, pl, C.byref(dc), ddt,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    errs = []
    for b in _items(dc):
        s5 = torch.as_strided(src, (dc.T, Hs, Ws, Cc), (st_, sh_, sw_, sc_), b * sb_).double()
        ref = torch.zeros((dc.T, dc.H, dc.W, dc.C), dtype=torch.float64, device=dev)
        ref[:, pt:pt + Hs, pl:pl + Ws, :Cc] = s5
        _eq(view_of(db, dc)[b], ref, "%r item %d" % (e, b), errs)
    return errs


NONCONV = {
    "vinet_bn_bwd_reduce": replay_bn_bwd,
    "vinet_bn_bwd_apply": replay_bn_bwd,
    "vinet_channel_stats": replay_channel_stats,
    "vinet_copy_affine": replay_copy_affine,
    "vinet_maxpool3d": replay_maxpool,
    "vinet_maxpool3d_bwd": replay_maxpool,
    "vinet_upsample2x": replay_upsample,
    "vinet_upsample2x_bwd_relu": replay_upsample,
    "vinet_import_ncdhw_pad": replay_import_pad,
    "vinet_bn_bwd_apply_split": replay_bn_bwd_apply_split,
    "vinet_split_bf16": replay_split_bf16,
}
