"""The BatchNorm kernels of csrc/bn.hip against float64 at their route, size and view edges: case tables, references, gates and the
runners that the host test (tests/test_bn_cases_host.py, CPU model of the ABI) and the GPU test (tests/test_gpu_bn_kernels.py,
libvinet_hip.so) share.  Nothing here shares code with tests/abi_emulator.py.

References read their inputs AFTER rounding to the storage type, and the fp32 parameter vectors as they are passed.  u = 2^-24.

  ReLU gate            x * scale + shift > 0 in float64: the product of two fp32 values is exact there and the rounded sum keeps its
                       sign, so this IS the kernels' fmaf(x, scale, shift) > 0 -- no exclusion zone around zero
  reductions, random   the float64 column totals over the rows the side reports (vinet_stats_rows) against the float64 sum of the
                       terms x, x^2, g, g * (x - mean) * invstd: |difference| <= 1.01 * (nvox + 4) * u * sum |term| per channel.  A term
                       takes at most 3 roundings (x - mean, * g, * invstd), a sum of nvox terms at most nvox - 1 more in ANY order,
                       the float64 total of the fp32 rows none; 1.01 covers the second-order terms ((1 + u)^65604 - 1 = 1.002 * 65604 u)
  reductions, exact    x integers in [-3, 3], dz in [-2, 2], mean in halves, invstd and scale powers of two, shift integers: every
                       term is a multiple of 1/4 and every partial sum stays below 2^24 quarter units, so the totals equal the reference
                       bit for bit -- no voxel dropped, none counted twice
  partials table       prefilled with NaN, a sentinel behind it: all rows * 2 * C floats finite afterwards (a block that owns no voxel
                       still writes its zeros), the sentinel's bits unchanged
  apply, random        |dx - ref| <= b = 8u * |scale| * (|g| + |c1| + (|x| + |mean|) * |invstd * c2|), g the gated gradient; bf16 output adds
                       half a bf16 ulp at |ref| + b, i.e. 2^(floor(log2(|ref| + b)) - 8).  (A flat 2^-9 |ref| is below what rounding to
                       8 significant bits costs: the exactly computed 2.7424 rounds to 2.75, 2^-8.5 away.  Half an ulp is between 2^-9
                       and 2^-8 of the value and is the least any correct kernel can be held to.)  Folded form A*g + B*x + D: B = -fl(fl(scale*invstd)*c2) (2 roundings), D = fma(k, mean,
                       -fl(scale*c1)), two fused multiply-adds -- 1u on |scale g|, 4u on |k x|, 5u on |k mean|, 4u on |scale c1|.
                       Element-wise form scale * (g - c1 - (x - mean) * invstd * c2): 3u, 3u, 5u.  Both below 8u.
  apply, exact         x, g, mean as above, invstd in {1, 2}, c2 integers, c1 an ODD multiple of 1/4: g - c1 - xhat * c2 is an odd
                       multiple of 1/4 of magnitude <= 18.75 (7 bits, never zero -- the sign of a zero is the one thing the two
                       forms disagree about), times a power of two: representable in bf16 (asserted), so dx is bit-equal
  apply_split          dx bit-equal to vinet_bn_bwd_apply's on the same inputs; hi == bf16(dx), lo == bf16(dx - hi) bit for bit
  finalize, bwd_finalize, partials_fold, fold, channel_sum
                       the reference starts from the same fp32 partials (channel_sum: the workspace the call leaves behind) widened
                       to float64, so a gate measures that kernel alone: outputs within 4u * max(1, |ref|); running statistics and
                       accumulated outputs within 4u * (|old| + |update|)

Every view passes quad_ok (C, ld, sB multiples of 4, the pointer aligned to 4 elements); nothing else is ever launched.  The refusals
(a scale without a shift and the reverse, channel counts whose group loop is ragged, C % Cout != 0, empty fold chunks) are only ever
asked for their return value and message: a refused call launches nothing.

NOT COVERED: the doubling of the apply kernels' voxels per block past 16 384 blocks (about 1 GB of tensors at C = 8)."""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import torch

from tests import route_cases as R
from tests.tail_cases import BF16, BITS, DTN, F32, TDT, U32, Side, Slab, f32, gate_bound      # noqa: F401 (Side: for the test modules)
from vinet_amd import _lib as L

OPT_DEFAULTS = R.option_defaults(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vinet_amd", "csrc", "options.h"))
DTS = (F32, BF16)
ES = {F32: 4, BF16: 2}
SENTINEL = -77.0         # around a written view and behind every written vector
NAN = float("nan")

# voxel count -> (B, T, H, W); B = 2 wherever a T slice has to show in the batch stride
DIMS = {1: (1, 1, 1, 1), 15: (1, 1, 3, 5), 16: (1, 2, 2, 4), 17: (1, 1, 1, 17), 30: (2, 1, 3, 5), 31: (1, 1, 1, 31), 32: (1, 2, 4, 4), 33: (1, 1, 3, 11),
        37: (1, 1, 1, 37), 63: (1, 3, 3, 7), 64: (1, 2, 4, 8), 65: (1, 1, 5, 13), 73: (1, 1, 1, 73), 85: (1, 1, 5, 17), 86: (1, 1, 2, 43),
        127: (1, 1, 1, 127), 128: (2, 2, 4, 8), 129: (1, 3, 1, 43), 130: (2, 1, 5, 13), 159: (1, 1, 3, 53), 160: (2, 2, 5, 8), 161: (1, 1, 7, 23),
        255: (1, 3, 5, 17), 256: (2, 2, 8, 8), 257: (1, 1, 1, 257), 260: (2, 2, 5, 13), 361: (1, 1, 19, 19), 1359: (1, 3, 3, 151), 1360: (2, 2, 17, 20),
        1361: (1, 1, 1, 1361), 3061: (1, 1, 1, 3061), 4095: (1, 3, 15, 91), 4096: (2, 2, 32, 32), 4097: (1, 1, 17, 241), 4100: (2, 2, 25, 41),
        5000: (2, 4, 25, 25), 9217: (1, 1, 13, 709), 65600: (2, 4, 100, 82)}
assert all(b * t * h * w == n for n, (b, t, h, w) in DIMS.items())


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _pick(values, n, g):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def view_geo(form, dims, Cc, chan=None):
    """Slab geometry of a view form.  chan: (ld, c_off) of a channel slice (default: 8 channels before and 8 behind)"""
    ld, off = chan or (Cc + 16, 8)
    geo = {}
    if form in ("chan", "both"):
        geo.update(ld=ld, c_off=off)
    if form in ("tslice", "both"):
        geo.update(t_total=dims[1] + 2, t_off=1)
    return geo


def oct_ok(slab):
    """csrc/elementwise.h oct_ok for a Slab over a 64-byte aligned allocation"""
    return slab.dims[4] % 8 == 0 and slab.ld % 8 == 0 and slab.sB % 8 == 0 and (slab.off * ES[slab.dt]) % 16 == 0


def quad_ok(slab):
    return slab.dims[4] % 4 == 0 and slab.ld % 4 == 0 and slab.sB % 4 == 0 and slab.off % 4 == 0


class Vec:
    """an fp32 parameter vector passed at offset r0 into a longer array (what engine.py does with `mean + r0`): NaN in front of
    and behind the C values an input may read, the sentinel around the C values an output may write"""

    def __init__(self, side, values, r0=0, out=False):
        self.n, self.r0, self.out = values.numel(), r0, out
        self.host = torch.full((r0 + self.n + 4,), SENTINEL if out else NAN)
        self.host[r0:r0 + self.n] = values.float()
        self.dev = side.put(self.host)

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * self.r0

    def get(self, what):
        got = self.dev.cpu()
        keep = torch.ones(got.numel(), dtype=torch.bool)
        keep[self.r0:self.r0 + self.n] = False
        assert torch.equal(got.view(torch.int32)[keep], self.host.view(torch.int32)[keep]), what + ": wrote outside its C values"
        return got[self.r0:self.r0 + self.n]


def _vp(v):
    return None if v is None else v.ptr


def put_tailed(side, slab, over, fill):
    """the slab's buffer with a tail behind it: NaN behind what is read, the sentinel behind what is written.  A block that ran
    `over` voxels past the view's last one (a lost `v1 > nvox` clamp) would land in the tail -- through the linear addressing
    (voxel * ld) and through the decoded one (voxel -> batch item, past B) alike -- where it poisons a sum or breaks the sentinel,
    instead of touching memory the case does not own."""
    B, T, H, W, _ = slab.dims
    last = B * T * H * W + over                               # one past the furthest voxel such a block could reach
    end = max(slab.off + last * slab.ld, (-(-last // (T * H * W)) + 1) * slab.sB)
    tail = torch.full((max(end - slab.base.numel(), 0) + slab.ld,), fill).to(TDT[slab.dt])
    return side.put(torch.cat([slab.base, tail]))


def untailed(buf, slab, fill, what):
    """the slab's part of a tailed buffer (on the host), after the check that the tail kept its bits"""
    got, n = buf.cpu(), slab.base.numel()
    want = torch.full((got.numel() - n,), fill).to(TDT[slab.dt])
    assert torch.equal(got[n:].view(BITS[slab.dt]), want.view(BITS[slab.dt])), what + ": wrote behind the end of its buffer"
    return got[:n]


# =====================================================================================================================
# reductions: vinet_channel_stats (mode 0), vinet_bn_bwd_reduce (mode 1)
# =====================================================================================================================
FWD_FORMS = ("none", "affine", "relu")      # relu = 0 / relu = 1 with scale and shift / relu = 1 with neither


class RCase:
    def __init__(self, tag, mode, dt, nvox, Cc, data, xform="dense", gform=None, xchan=None, gchan=None, fwd="affine", r0=0, opts=None):
        self.tag, self.mode, self.dt, self.nvox, self.C, self.data = tag, mode, dt, nvox, Cc, data
        self.dims = DIMS[nvox] + (Cc,)
        self.xform, self.gform, self.xchan, self.gchan = xform, gform or xform, xchan, gchan
        self.fwd, self.r0, self.opts = (fwd if mode else "none"), (r0 if mode else 0), dict(opts or {})
        self.kernel = self._kernel()
        self.id = "%s-%s-%s-v%d-c%d-%s-x_%s%s-g_%s%s-%s-r%d-%s" % (
            tag, "bwd" if mode else "stats", DTN[dt], nvox, Cc, data, self.xform, "" if xchan is None else "%d.%d" % xchan, self.gform,
            "" if gchan is None else "%d.%d" % gchan, self.fwd, self.r0, "_".join("%s%d" % kv for kv in sorted(self.opts.items())) or "default")

    def slabs(self):
        """(x, dz) over fresh buffers; dz is None in mode 0"""
        x = Slab(self.dims, self.dt, fill=NAN, values=reduce_inputs(self)[0], **view_geo(self.xform, self.dims, self.C, self.xchan))
        g = Slab(self.dims, self.dt, fill=NAN, values=reduce_inputs(self)[1], **view_geo(self.gform, self.dims, self.C, self.gchan)) if self.mode else None
        assert quad_ok(x) and (g is None or quad_ok(g)), self.id
        return x, g

    def _kernel(self):
        """the route of launch_channel_reduce (csrc/bn.hip) for this case"""
        o = dict(OPT_DEFAULTS, **self.opts)
        x, g = self.slabs_geo()
        rows = max(1, min(o["bn_rows"], (self.nvox + 63) // 64))
        if o["reduce_small"] and self.nvox <= 64 and rows == 1:
            return "channel_reduce_small_kernel"
        oct_ = oct_ok(x) and (g is None or oct_ok(g))
        if self.mode and o["bn_lean"] and self.dt == BF16 and oct_:
            return "bn_bwd_reduce8_bf16_kernel"
        return "channel_reduce8_kernel" if oct_ else "channel_reduce_kernel"

    def slabs_geo(self):
        x = Slab(self.dims, self.dt, fill=0.0, **view_geo(self.xform, self.dims, self.C, self.xchan))
        g = Slab(self.dims, self.dt, fill=0.0, **view_geo(self.gform, self.dims, self.C, self.gchan)) if self.mode else None
        return x, g

    def __repr__(self):
        return self.id


def _build_reduce():
    out, seen = [], set()

    def add(tag, nvox, Cc, modes=(0, 1), dts=DTS, datas=("exact", "rand"), **kw):
        for mode in modes:
            for dt in dts:
                for data in datas:
                    k = dict(kw)
                    k.setdefault("r0", (0, 4, 12)[len(out) % 3])
                    k.setdefault("fwd", "affine")            # the production form; the others: the "fwd" cases below
                    c = RCase(tag, mode, dt, nvox, Cc, data, **k)
                    if c.id not in seen:
                        seen.add(c.id)
                        out.append(c)

    # rows 1 -> 2 -> 3 and the hand-over from the small kernel at 64 voxels; R = 85 with one idle lane, and the quad route
    for nvox in (1, 63, 64, 65, 127, 129, 4100):
        for Cc in (24, 12):
            add("sweep", nvox, Cc)
    add("rowcap", 65600, 8)                                   # rows == bn_rows == 1024 < ceil(nvox / 64)
    for Cc in (4, 12, 8, 24, 40, 200, 1024, 2048, 4096):    # quad route; R = 256, 85, 51, 10, 2, 1; two uniform group passes
        add("chan", 130, Cc)
    add("chan", 130, 2048, opts=dict(bn_lean=0), modes=(1,), dts=(BF16,))
    add("chan", 130, 4096, opts=dict(bn_lean=0), modes=(1,), dts=(BF16,))
    # several rounds per lane, the last one ragged
    for rows in (2, 3):
        for il in (0, 1):
            for Cc in (8, 24, 12):
                add("rounds", 5000, Cc, opts=dict(bn_rows=rows, reduce_il=il))
                if Cc % 8 == 0:
                    add("rounds", 5000, Cc, opts=dict(bn_rows=rows, reduce_il=il, bn_lean=0), modes=(1,), dts=(BF16,))
    # route by alignment
    add("ptr8mod16", 130, 8, dts=(BF16,), xform="chan", xchan=(16, 4))                       # bf16 pointer 8 mod 16
    add("ld_c_plus4", 130, 8, xform="chan", xchan=(12, 0))                                   # ld % 8 == 4
    add("sB4mod8", 130, 12, xform="tslice")                                                  # sB = 3 * 65 * 12 = 4 mod 8
    add("sB4mod8", 130, 8, xform="both", xchan=(12, 4))
    add("x_oct_dz_quad", 130, 8, modes=(1,), xform="dense", gform="chan", gchan=(12, 0))
    add("x_oct_dz_quad", 5000, 24, modes=(1,), xform="dense", gform="chan", gchan=(28, 4))
    # views; the T slice has B = 2 (the non-linear vox_lin path and the batch stride)
    forms = ("dense", "chan", "tslice", "both")
    for i, form in enumerate(forms):
        for Cc, chan in ((24, None), (12, (24, 4))):
            add("views", 260, Cc, xform=form, gform=forms[(i + 1) % 4], xchan=chan, gchan=chan)
            add("views", 260, Cc, xform=form, gform=form, xchan=chan, gchan=chan)
        add("views", 30, 24, xform=form, gform=forms[(i + 1) % 4])                           # the small kernel over views
    # forward forms on every kernel; bn_lean and reduce_small at both values
    for fwd in FWD_FORMS:
        for r0 in (4, 12):
            for Cc in (8, 12):
                for nvox in (30, 130):
                    add("fwd", nvox, Cc, modes=(1,), fwd=fwd, r0=r0)
                add("fwd", 130, Cc, modes=(1,), dts=(BF16,), fwd=fwd, r0=r0, opts=dict(bn_lean=0))
    for nvox in (1, 63, 64):
        for Cc in (8, 12, 24):
            add("small", nvox, Cc, opts=dict(reduce_small=1))
            add("small", nvox, Cc, opts=dict(reduce_small=0))
    return out


def _exact_params(Cc, g, half_means=True):
    mean = _pick([-1.0, -0.5, 0.0, 0.5, 1.0] if half_means else [-1.0, 0.0, 1.0], Cc, g)
    scale = _pick([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], Cc, g)
    shift = torch.randint(-2, 3, (Cc,), generator=g).float()
    return mean, scale, shift


@functools.lru_cache(maxsize=None)
def _reduce_data(dims, dt, data):
    """(x, dz [B,T,H,W,C] in the storage type, mean, invstd, scale, shift fp32 [C]); shared by every case of the shape, never changed"""
    g = _gen("reduce", dims, dt, data)
    Cc = dims[4]
    if data == "exact":
        x = torch.randint(-3, 4, dims, generator=g).float()
        dz = torch.randint(-2, 3, dims, generator=g).float()
        mean, scale, shift = _exact_params(Cc, g)
        invstd = _pick([0.5, 1.0, 2.0], Cc, g)
    else:
        x = torch.randn(dims, generator=g) + 0.5 * torch.randn((Cc,), generator=g)
        dz = torch.randn(dims, generator=g)
        mean, invstd = 0.5 * torch.randn((Cc,), generator=g), 0.5 + 1.5 * torch.rand((Cc,), generator=g)
        scale = (0.5 + torch.rand((Cc,), generator=g)) * _pick([-1.0, 1.0], Cc, g)
        shift = 0.5 * torch.randn((Cc,), generator=g)
    return x.to(TDT[dt]), dz.to(TDT[dt]), mean, invstd, scale, shift


def reduce_inputs(case):
    return _reduce_data(case.dims, case.dt, case.data)


def relu_gate(x64, fwd, scale, shift):
    if fwd == "none":
        return torch.ones_like(x64, dtype=torch.bool)
    return (x64 * scale.double() + shift.double() > 0) if fwd == "affine" else (x64 > 0)


@functools.lru_cache(maxsize=None)
def _reduce_ref(dims, dt, data, mode, fwd):
    """(float64 sums [2, C], sums of |terms| [2, C])"""
    x, dz, mean, invstd, scale, shift = _reduce_data(dims, dt, data)
    xw = x.double()
    if mode == 0:
        t0, t1 = xw, xw * xw
    else:
        t0 = dz.double() * relu_gate(xw, fwd, scale, shift)
        t1 = t0 * (xw - mean.double()) * invstd.double()
    flat = lambda t: t.reshape(-1, dims[4])
    return torch.stack([flat(t0).sum(0), flat(t1).sum(0)]), torch.stack([flat(t0).abs().sum(0), flat(t1).abs().sum(0)])


def reduce_ref(case):
    return _reduce_ref(case.dims, case.dt, case.data, case.mode, case.fwd)


def affine_of(fwd, scale, shift):
    if fwd == "affine":
        return L.CAffine(scale.ptr, shift.ptr, 1)
    return L.CAffine(None, None, 1 if fwd == "relu" else 0)


SLACK = 64           # floats behind a partials table


def run_reduce(side, case, x, g, xb, gb):
    """launch one reduction over the given buffers -> (rows, table [rows, 2, C] on the host)"""
    _, _, mean, invstd, scale, shift = reduce_inputs(case)
    Cc = case.C
    with R.options(side.api, case.opts, OPT_DEFAULTS):
        rows = side.api.vinet_stats_rows(x.ct(xb))
        assert rows == max(1, min(dict(OPT_DEFAULTS, **case.opts)["bn_rows"] if side.dev.type != "cpu" else 1024, (case.nvox + 63) // 64)), (case, rows)
        n = rows * 2 * Cc
        part = side.put(torch.cat([torch.full((n,), NAN), torch.full((SLACK,), SENTINEL)]))
        if case.mode == 0:
            side.call("vinet_channel_stats", x.ct(xb), case.dt, part.data_ptr())
        else:
            vm, vi, vs, vh = (Vec(side, v, case.r0) for v in (mean, invstd, scale, shift))
            side.call("vinet_bn_bwd_reduce", g.ct(gb), x.ct(xb), case.dt, affine_of(case.fwd, vs, vh), vm.ptr, vi.ptr, part.data_ptr())
    got = part.cpu()
    assert bool((got[n:] == SENTINEL).all()), "%r: wrote behind the partials table" % case
    table = got[:n].view(rows, 2, Cc)
    assert bool(torch.isfinite(table).all()), "%r: %d of the table's floats were not written" % (case, int((~torch.isfinite(table)).sum()))
    return rows, table


def check_reduce(side, case):
    x, g = case.slabs()
    over = -(-case.nvox // max(1, min(dict(OPT_DEFAULTS, **case.opts)["bn_rows"], (case.nvox + 63) // 64)))      # a block's voxels
    xb, gb = put_tailed(side, x, over, NAN), None if g is None else put_tailed(side, g, over, NAN)
    rows, table = run_reduce(side, case, x, g, xb, gb)
    total = table.double().sum(0)
    ref, mag = reduce_ref(case)
    if case.data == "exact":
        bad = total != ref
        assert not bool(bad.any()), "%r: %d totals differ, first %r: %r against %r" % (
            case, int(bad.sum()), tuple(int(i) for i in bad.nonzero()[0]), float(total[bad][0]), float(ref[bad][0]))
        return dict(rows=rows)
    return dict(rows=rows, err_over_bound=gate_bound(total, ref, 1.01 * (case.nvox + 4) * U32 * mag, repr(case)))


# =====================================================================================================================
# vinet_bn_bwd_apply, vinet_bn_bwd_apply_split
# =====================================================================================================================
def apply_vb(Cc):
    """voxels per block of the 8-channel apply kernels below 16 384 blocks: 4 rounds of 4 voxels per lane"""
    return 16 * (256 // min(Cc // 8, 256))


class ACase:
    """dxform: 'inplace' (dx is dz's view: the production form) or a view form inside a sentinel-filled buffer; split: also through
    vinet_bn_bwd_apply_split (fp32, 8-channel views), hi / lo taking dx's form"""

    def __init__(self, tag, dt, nvox, Cc, data, dxform="inplace", inform="dense", dxchan=None, relu=1, opts=None, split=False, r0=0):
        self.tag, self.dt, self.nvox, self.C, self.data, self.dxform, self.inform, self.dxchan = tag, dt, nvox, Cc, data, dxform, inform, dxchan
        self.relu, self.opts, self.split, self.r0 = relu, dict(opts or {}), split, r0
        self.dims = DIMS[nvox] + (Cc,)
        self.kernels = self._kernels()
        self.id = "%s-%s-v%d-c%d-%s-in_%s-dx_%s%s-relu%d-r%d-%s%s" % (
            tag, DTN[dt], nvox, Cc, data, inform, dxform, "" if dxchan is None else "%d.%d" % dxchan, relu, r0,
            "_".join("%s%d" % kv for kv in sorted(self.opts.items())) or "default", "-split" if split else "")

    def geo(self, which):
        if which == "dx" and self.dxform != "inplace":
            return view_geo(self.dxform, self.dims, self.C, self.dxchan)
        return view_geo(self.inform, self.dims, self.C)

    def _kernels(self):
        o = dict(OPT_DEFAULTS, **self.opts)
        slabs = [Slab(self.dims, self.dt, fill=0.0, **self.geo(w)) for w in ("dz", "x", "dx")]
        assert all(quad_ok(s) for s in slabs), self.tag
        if not all(oct_ok(s) for s in slabs):
            assert not self.split
            return ["bn_bwd_apply_kernel"]
        first = "bn_bwd_apply8_bf16_kernel" if o["bn_lean"] and self.dt == BF16 else "bn_bwd_apply8_kernel"
        return [first] + (["bn_bwd_apply8_kernel<split>"] if self.split else [])

    def __repr__(self):
        return self.id


def _build_apply():
    out, seen = [], set()

    def add(tag, nvox, Cc, dts=DTS, datas=("exact", "rand"), **kw):
        for dt in dts:
            for data in datas:
                k = dict(kw)
                k.setdefault("r0", (0, 4, 12)[len(out) % 3])
                k.setdefault("relu", 1 - (len(out) // 3) % 2)
                if k.get("split") and dt != F32:
                    k["split"] = False
                c = ACase(tag, dt, nvox, Cc, data, **k)
                if c.id not in seen:
                    seen.add(c.id)
                    out.append(c)

    # the block seam: one voxel, one short of a block, a whole block, one more, two blocks and a ragged round of the third
    for Cc in (8, 24, 200, 1024, 2048):
        vb, R_ = apply_vb(Cc), apply_vb(Cc) // 16
        for nvox in (1, vb - 1, vb, vb + 1, 2 * vb + 4 * R_ + 1):
            add("seam", nvox, Cc, split=True)                                                      # in place
            add("seam", nvox, Cc, dts=(BF16,), opts=dict(bn_lean=0))
    for Cc in (8, 24):
        vb = apply_vb(Cc)
        add("seam", vb + 1, Cc, dxform="chan", split=True)                                         # the seam again, dx apart
    # the element-wise kernel: 255, 256, 257 quads (C = 4), 255 and 258 (C = 12), 254, 256, 258 behind a dx that alone is off the
    # 8-channel grid
    for nvox in (255, 256, 257):
        add("elementwise", nvox, 4)
        add("elementwise", nvox, 4, dxform="chan", dxchan=(12, 4))
    for nvox in (85, 86):
        add("elementwise", nvox, 12)
        add("elementwise", nvox, 12, dxform="tslice")
    for nvox in (127, 128, 129):
        add("dx_off_grid", nvox, 8, dxform="chan", dxchan=(12, 0))
        add("dx_off_grid", nvox, 8, dts=(BF16,), dxform="chan", dxchan=(16, 4))
    # views with two batch items, relu and bn_lean at both values
    forms = ("dense", "chan", "tslice", "both")
    for i, form in enumerate(forms):
        for relu in (0, 1):
            for Cc, chan in ((24, None), (12, (24, 4))):
                add("views", 260, Cc, dxform=form, inform=forms[(i + 1) % 4], dxchan=chan, relu=relu, split=Cc == 24)
                add("views", 260, Cc, dxform="inplace", inform=form, relu=relu, split=Cc == 24)
            add("views", 260, 24, dts=(BF16,), dxform=form, inform=forms[(i + 2) % 4], relu=relu, opts=dict(bn_lean=0))
    return out


@functools.lru_cache(maxsize=None)
def _apply_data(dims, dt, data):
    g = _gen("apply", dims, dt, data)
    Cc = dims[4]
    if data == "exact":
        x = torch.randint(-3, 4, dims, generator=g).float()
        dz = torch.randint(-2, 3, dims, generator=g).float()
        mean, scale, shift = _exact_params(Cc, g)
        invstd = _pick([1.0, 2.0], Cc, g)
        c1, c2 = _pick([-0.75, -0.25, 0.25, 0.75], Cc, g), torch.randint(-2, 3, (Cc,), generator=g).float()
    else:
        x = torch.randn(dims, generator=g) + 0.5 * torch.randn((Cc,), generator=g)
        dz = torch.randn(dims, generator=g)
        mean, invstd = 0.5 * torch.randn((Cc,), generator=g), 0.5 + 1.5 * torch.rand((Cc,), generator=g)
        scale = (0.5 + torch.rand((Cc,), generator=g)) * _pick([-1.0, 1.0], Cc, g)
        shift = 0.5 * torch.randn((Cc,), generator=g)
        c1, c2 = 0.3 * torch.randn((Cc,), generator=g), 0.3 * torch.randn((Cc,), generator=g)
    return x.to(TDT[dt]), dz.to(TDT[dt]), dict(mean=mean, invstd=invstd, scale=scale, shift=shift, c1=c1, c2=c2)


@functools.lru_cache(maxsize=None)
def _apply_ref(dims, dt, data, relu):
    """(float64 dx, the derived bound)"""
    x, dz, p = _apply_data(dims, dt, data)
    xw, d = x.double(), {k: v.double() for k, v in p.items()}
    g = dz.double() * relu_gate(xw, "affine" if relu else "none", p["scale"], p["shift"])
    ref = d["scale"] * (g - d["c1"] - (xw - d["mean"]) * d["invstd"] * d["c2"])
    bound = 8 * U32 * d["scale"].abs() * (g.abs() + d["c1"].abs() + (xw.abs() + d["mean"].abs()) * (d["invstd"] * d["c2"]).abs())
    if dt == BF16:
        bound = bound + bf16_half_ulp(ref.abs() + bound)
    if data == "exact":
        assert torch.equal(ref.to(TDT[dt]).double(), ref) and not bool((ref == 0).any()) and float(ref.abs().max()) <= 37.5, "not exact in its type"
    return ref, bound


def bf16_half_ulp(mag):
    """half a unit in the last place of bf16 (8 significant bits) at magnitude `mag`: 2^(floor(log2 mag) - 8), the most that rounding a
    value of at most that magnitude to nearest can move it.  It lies between 2^-9 and 2^-8 of `mag`."""
    return torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -126))) - 8)


def _same_bits(a, b, dt, what):
    a, b = a.contiguous().view(BITS[dt]), b.contiguous().view(BITS[dt])
    assert torch.equal(a, b), "%s: %d of %d elements differ in their bits" % (what, int((a != b).sum()), a.numel())


def check_apply(side, case):
    xv, gv, p = _apply_data(case.dims, case.dt, case.data)
    ref, bound = _apply_ref(case.dims, case.dt, case.data, case.relu)
    dz = Slab(case.dims, case.dt, fill=SENTINEL, values=gv, **case.geo("dz"))
    x = Slab(case.dims, case.dt, fill=NAN, values=xv, **case.geo("x"))
    inplace = case.dxform == "inplace"
    dx = dz if inplace else Slab(case.dims, case.dt, fill=SENTINEL, **case.geo("dx"))
    over = apply_vb(case.C) if case.C % 8 == 0 else 64          # a block's voxels
    xb = put_tailed(side, x, over, NAN)
    vec = {k: Vec(side, v, case.r0) for k, v in p.items()}
    aff = L.CAffine(vec["scale"].ptr, vec["shift"].ptr, case.relu)
    tail = (vec["mean"].ptr, vec["invstd"].ptr, vec["c1"].ptr, vec["c2"].ptr)
    errs = {}

    def launch(split):
        """-> host copies of dx's buffer (and of the hi / lo views), every tail and everything outside a written view checked"""
        gb = put_tailed(side, dz, over, SENTINEL)
        db = gb if inplace else put_tailed(side, dx, over, SENTINEL)
        hi = lo = None
        if not split:
            side.call("vinet_bn_bwd_apply", dz.ct(gb), x.ct(xb), case.dt, aff, *tail, dx.ct(db))
        else:
            hs, ls = (Slab(case.dims, BF16, fill=SENTINEL, **case.geo("dx")) for _ in range(2))
            hb, lb = put_tailed(side, hs, over, SENTINEL), put_tailed(side, ls, over, SENTINEL)
            side.call("vinet_bn_bwd_apply_split", dz.ct(gb), x.ct(xb), aff, *tail, dx.ct(db), hs.ct(hb), ls.ct(lb))
            planes = []
            for slab, buf, nm in ((hs, hb, "hi"), (ls, lb, "lo")):
                host = untailed(buf, slab, SENTINEL, "%r: %s" % (case, nm))
                slab.assert_outside_untouched(host, "%r: %s" % (case, nm))
                planes.append(slab.inner(host))
            hi, lo = planes
        what = "%r: dx%s" % (case, " of the split run" if split else "")
        host = untailed(db, dx, SENTINEL, what)
        dx.assert_outside_untouched(host, what)
        if not inplace:
            _same_bits(untailed(gb, dz, SENTINEL, "%r: dz" % case), dz.base, case.dt, "%r: dz" % case)
        return dx.inner(host), hi, lo

    with R.options(side.api, case.opts, OPT_DEFAULTS):
        got, _, _ = launch(False)
        if case.data == "exact":
            _same_bits(got, ref.to(TDT[case.dt]), case.dt, "%r: dx" % case)
        else:
            errs["err_over_bound"] = gate_bound(got, ref, bound, "%r: dx" % case)
        if case.split:
            got2, hi, lo = launch(True)
            _same_bits(got2, got, F32, "%r: dx of apply_split against apply" % case)
            _same_bits(hi, got2.bfloat16(), BF16, "%r: hi" % case)
            _same_bits(lo, (got2 - got2.bfloat16().float()).bfloat16(), BF16, "%r: lo" % case)
    _same_bits(untailed(xb, x, NAN, "%r: x" % case), x.base, case.dt, "%r: x" % case)
    return errs


# =====================================================================================================================
# vinet_bn_finalize, vinet_bn_bwd_finalize
# =====================================================================================================================
FIN_ROWS = (1, 63, 255, 256, 257, 1030)
FIN_CS = (1, 5, 64)
FIN_NULLS = ("gamma", "beta", "running_mean", "running_var", "mean", "invstd")
EPS = 1e-3


class FCase:
    """flavour: 'normal' | 'const' (channel 0 constant, its variance rounds negative) | 'bigmean' (|mean| = 1e3 std) | 'count1'"""

    def __init__(self, rows, Cc, wide, flavour="normal", null=None, momentum=0.1):
        self.rows, self.C, self.ld, self.flavour, self.null, self.momentum = rows, Cc, (Cc + 12 if wide else 0), flavour, null, momentum
        self.id = "r%d-c%d-ld%d-%s-null_%s-m%g" % (rows, Cc, self.ld, flavour, null, momentum)

    def __repr__(self):
        return self.id


FIN_CASES = ([FCase(r, c, w) for r in FIN_ROWS for c in FIN_CS for w in (0, 1)] +
             [FCase(r, c, w, fl) for fl in ("const", "bigmean") for r, c, w in ((63, 5, 1), (257, 64, 0), (1, 1, 0))] +
             [FCase(1, c, w, "count1") for c in (1, 5) for w in (0, 1)] +
             [FCase(257, 5, 1, null=n) for n in FIN_NULLS] + [FCase(63, 64, 0, null=n) for n in FIN_NULLS] +
             [FCase(r, 5, w, momentum=m) for m in (0.0, 1.0, 0.001) for r, w in ((1, 0), (256, 1))])


def _table(part, ld, Cc):
    """[rows, 2, C] fp32 laid out in rows of ld floats, NaN in the gaps and a NaN tail"""
    rows = part.shape[0]
    ld = ld or Cc
    flat = torch.full((rows * 2 * ld + 8,), NAN)
    torch.as_strided(flat, (rows, 2, Cc), (2 * ld, ld, 1)).copy_(part)
    return flat


@functools.lru_cache(maxsize=None)
def _fin_inputs(rows, Cc, flavour):
    g = _gen("finalize", rows, Cc, flavour)
    per = 1 if flavour == "count1" else 4
    xs = torch.randn((rows, per, Cc), generator=g, dtype=torch.float64) + (torch.rand((Cc,), generator=g, dtype=torch.float64) - 0.5)
    if flavour == "bigmean":
        xs = xs + 1000.0
    part = torch.stack([xs.sum(1), (xs * xs).sum(1)], 1).float()
    if flavour == "const":
        v = torch.tensor(0.1).float()
        part[:, 0, 0] = per * v
        part[:, 1, 0] = torch.nextafter((per * v * v).float(), torch.tensor(0.0))
    vecs = dict(gamma=0.5 + 0.5 * torch.rand((Cc,), generator=g), beta=torch.randn((Cc,), generator=g),
                running_mean=torch.randn((Cc,), generator=g), running_var=0.5 + torch.rand((Cc,), generator=g))
    return part, float(rows * per), vecs


def check_finalize(side, case):
    part, count, vecs = _fin_inputs(case.rows, case.C, case.flavour)
    Cc, m, eps = case.C, f32(case.momentum), f32(EPS)
    P = part.double()
    s, q = P[:, 0].sum(0), P[:, 1].sum(0)
    mean = s / count
    var_raw = q / count - mean * mean
    if case.flavour == "const":
        assert float(var_raw[0]) < -1e-12, "the constant channel's variance does not round negative"
    var = var_raw.clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    use = {k: (None if case.null == k else v) for k, v in vecs.items()}
    gam = use["gamma"].double() if use["gamma"] is not None else torch.ones(Cc, dtype=torch.float64)
    bet = use["beta"].double() if use["beta"] is not None else torch.zeros(Cc, dtype=torch.float64)
    ref = dict(mean=mean, invstd=invstd, scale=gam * invstd, shift=bet - mean * gam * invstd)
    unbiased = var * count / (count - 1.0) if count > 1 else var
    tab = side.put(_table(part, case.ld, Cc))
    vin = {k: (None if v is None else Vec(side, v, 4)) for k, v in use.items() if k in ("gamma", "beta")}
    run = {k: (None if use[k] is None else Vec(side, use[k], 4, out=True)) for k in ("running_mean", "running_var")}
    outs = {k: (None if case.null == k else Vec(side, torch.full((Cc,), NAN), 4, out=True)) for k in ("mean", "invstd", "scale", "shift")}
    side.call("vinet_bn_finalize", tab.data_ptr(), case.rows, Cc, case.ld, count, _vp(vin["gamma"]), _vp(vin["beta"]), EPS, case.momentum,
              _vp(run["running_mean"]), _vp(run["running_var"]), _vp(outs["mean"]), _vp(outs["invstd"]), outs["scale"].ptr, outs["shift"].ptr)
    errs = {}
    for k, o in outs.items():
        if o is not None:
            errs[k] = gate_bound(o.get("%r: %s" % (case, k)), ref[k], 4 * U32 * ref[k].abs().clamp_min(1.0), "%r: %s" % (case, k))
    if case.flavour == "const" and outs["invstd"] is not None:          # the clamp: invstd = 1 / sqrt(eps)
        want = 1.0 / np.sqrt(eps)
        assert abs(float(outs["invstd"].get("invstd")[0]) - want) <= 4 * U32 * want, "%r: invstd of a variance that rounds negative" % case
    for k, new in (("running_mean", mean), ("running_var", unbiased)):
        if run[k] is not None:
            old, upd = (1.0 - m) * use[k].double(), m * new
            errs[k] = gate_bound(run[k].get("%r: %s" % (case, k)), old + upd, 4 * U32 * (old.abs() + upd.abs()), "%r: %s" % (case, k))
    return errs


BFIN_NULLS = ("dgamma", "dbeta", "c1", "c2", "scale_invstd")
BFIN_CASES = ([FCase(r, c, w, "train1") for r in FIN_ROWS for c in FIN_CS for w in (0, 1)] +
              [FCase(r, c, w, "train0") for r, c, w in ((1, 1, 0), (257, 5, 1), (1030, 64, 0))] +
              [FCase(257, 5, 1, "train1", null=n) for n in BFIN_NULLS] + [FCase(63, 64, 0, "train0", null=n) for n in BFIN_NULLS])


def check_bwd_finalize(side, case):
    """dgamma / dbeta ADD onto non-zero accumulators; c1 = s / count, c2 = p / count (0 with train = 0); `scale` and `invstd` are
    accepted and unused (NULL in the 'scale_invstd' cases)"""
    g = _gen("bwd_finalize", case.rows, case.C)
    Cc, train = case.C, 1 if case.flavour == "train1" else 0
    part = torch.randn((case.rows, 2, Cc), generator=g)
    old = dict(dgamma=torch.randn((Cc,), generator=g), dbeta=torch.randn((Cc,), generator=g))
    count = float(case.rows * 4)
    s, p = part.double()[:, 0].sum(0), part.double()[:, 1].sum(0)
    tab = side.put(_table(part, case.ld, Cc))
    acc = {k: (None if case.null == k else Vec(side, v, 4, out=True)) for k, v in old.items()}
    cs = {k: (None if case.null == k else Vec(side, torch.full((Cc,), NAN), 12, out=True)) for k in ("c1", "c2")}
    unused = None if case.null == "scale_invstd" else Vec(side, torch.ones(Cc), 4)
    side.call("vinet_bn_bwd_finalize", tab.data_ptr(), case.rows, Cc, case.ld, count, _vp(unused), train, _vp(acc["dgamma"]), _vp(acc["dbeta"]),
              _vp(unused), _vp(cs["c1"]), _vp(cs["c2"]))
    errs = {}
    for k, upd in (("dgamma", p), ("dbeta", s)):
        if acc[k] is not None:
            o = old[k].double()
            errs[k] = gate_bound(acc[k].get("%r: %s" % (case, k)), o + upd, 4 * U32 * (o.abs() + upd.abs()), "%r: %s" % (case, k))
    for k, tot in (("c1", s), ("c2", p)):
        if cs[k] is not None:
            want = tot / count if train else torch.zeros(Cc, dtype=torch.float64)
            errs[k] = gate_bound(cs[k].get("%r: %s" % (case, k)), want, 4 * U32 * want.abs().clamp_min(1.0), "%r: %s" % (case, k))
    return errs


# =====================================================================================================================
# vinet_bn_partials_fold, vinet_bn_fold, vinet_channel_sum
# =====================================================================================================================
FOLD_PERS = (1, 3, 4, 5, 31, 32, 33, 36, 65)          # around the 8-deep unrolled trip `r + 28 < r1` of the four row lanes
FOLD_CS = (1, 8, 64, 65, 100)
# (per, C, out_rows): the last chunk holds max(1, per - 2) rows (out_rows 3) or max(1, per - 4) (out_rows 5); out_rows 1: one chunk
PFOLD_CASES = [(per, Cc, 3) for per in FOLD_PERS for Cc in FOLD_CS] + [(per, 65, 5) for per in (5, 33, 36, 65)] + [(per, 8, 1) for per in (1, 29, 65)]


def pfold_rows(per, out_rows):
    rows = per * (out_rows - 1) + max(1, per - (out_rows - 1))
    assert (rows + out_rows - 1) // out_rows == per and (out_rows - 1) * per < rows
    return rows


def check_partials_fold(side, per, Cc, out_rows):
    rows = pfold_rows(per, out_rows)
    part = torch.randn((rows, 2, Cc), generator=_gen("pfold", per, Cc, out_rows))
    src = side.put(torch.cat([part.reshape(-1), torch.full((8,), NAN)]))
    n = out_rows * 2 * Cc
    out = side.put(torch.cat([torch.full((n,), NAN), torch.full((SLACK,), SENTINEL)]))
    side.call("vinet_bn_partials_fold", src.data_ptr(), rows, Cc, out.data_ptr(), out_rows)
    got = out.cpu()
    assert bool((got[n:] == SENTINEL).all()), "partials_fold wrote behind its output"
    ref = torch.stack([part.double()[i * per:(i + 1) * per].sum(0) for i in range(out_rows)])
    return dict(out=gate_bound(got[:n].view(out_rows, 2, Cc), ref, 4 * U32 * ref.abs().clamp_min(1.0), "partials_fold per=%d C=%d" % (per, Cc)))


BNFOLD_CS = (1, 255, 256, 257)
BNFOLD_NULLS = (None, "gamma", "beta", "conv_bias", "invstd")


def check_bn_fold(side, Cc, null):
    """the kernel works in fp32: invstd = 1 / sqrtf(rv + eps) takes three roundings, so the data keeps every output below 1 in
    magnitude (rv in [1.5, 4], gamma in [0.5, 1], |conv_bias - rm| <= 0.5) and the gate's floor of 4u leaves them room"""
    g = _gen("bn_fold", Cc)
    v = dict(gamma=0.5 + 0.5 * torch.rand((Cc,), generator=g), beta=0.5 * (torch.rand((Cc,), generator=g) - 0.5),
             rm=0.5 * (torch.rand((Cc,), generator=g) - 0.5), rv=1.5 + 2.5 * torch.rand((Cc,), generator=g),
             conv_bias=0.5 * (torch.rand((Cc,), generator=g) - 0.5))
    vin = {k: (None if null == k else Vec(side, t, 4)) for k, t in v.items()}
    outs = {k: (None if null == k else Vec(side, torch.full((Cc,), NAN), 12, out=True)) for k in ("scale", "shift", "invstd")}
    side.call("vinet_bn_fold", _vp(vin["gamma"]), _vp(vin["beta"]), vin["rm"].ptr, vin["rv"].ptr, _vp(vin["conv_bias"]), EPS, Cc,
              outs["scale"].ptr, outs["shift"].ptr, _vp(outs["invstd"]))
    d = {k: (t.double() if null != k else torch.full((Cc,), 1.0 if k == "gamma" else 0.0, dtype=torch.float64)) for k, t in v.items()}
    istd = 1.0 / torch.sqrt(d["rv"] + f32(EPS))
    ref = dict(invstd=istd, scale=d["gamma"] * istd, shift=d["beta"] + (d["conv_bias"] - d["rm"]) * d["gamma"] * istd)
    return {k: gate_bound(o.get("bn_fold " + k), ref[k], 4 * U32 * ref[k].abs().clamp_min(1.0), "bn_fold C=%d null=%s: %s" % (Cc, null, k))
            for k, o in outs.items() if o is not None}


# (tag, nvox, C): the small kernel, the 8-channel route, the 4-channel route
CSUM_SHAPES = (("small", 30, 8), ("small", 64, 12), ("oct", 130, 8), ("oct", 4100, 24), ("quad", 130, 12), ("quad", 260, 4))
CSUM_CASES = [(tag, nvox, Cc, dt, cout, acc) for tag, nvox, Cc in CSUM_SHAPES for dt in DTS for cout in sorted({1, max(1, Cc // 4), Cc}) for acc in (0, 1)]


def check_channel_sum(side, tag, nvox, Cc, dt, cout, acc):
    """out[j] (+)= the sum over voxels and over channels c with c % Cout == j.  The workspace the call leaves behind is the partials
    table: it is gated like a reduction, and `out` against ITS float64 totals."""
    case = RCase("csum_" + tag, 0, dt, nvox, Cc, "rand", xform="chan" if tag != "small" else "tslice", xchan=(Cc + 8, 4) if Cc % 8 else None)
    x, _ = case.slabs()
    xb = put_tailed(side, x, nvox, NAN)
    rows = side.api.vinet_stats_rows(x.ct(xb))
    n = rows * 2 * Cc
    ws = side.put(torch.cat([torch.full((n,), NAN), torch.full((SLACK,), SENTINEL)]))
    old = torch.randn((cout,), generator=_gen("csum_old", Cc, cout))
    out = Vec(side, old, 4, out=True)
    side.call("vinet_channel_sum", x.ct(xb), dt, ws.data_ptr(), cout, out.ptr, acc)
    got_ws = ws.cpu()
    assert bool((got_ws[n:] == SENTINEL).all()), "channel_sum wrote behind its workspace"
    table = got_ws[:n].view(rows, 2, Cc)
    assert bool(torch.isfinite(table).all())
    ref, mag = reduce_ref(case)
    errs = dict(ws_over_bound=gate_bound(table.double().sum(0)[0], ref[0], 1.01 * (nvox + 4) * U32 * mag[0], "channel_sum workspace"))
    upd = table.double()[:, 0].sum(0).view(-1, cout).sum(0)
    if acc:
        o = old.double()
        errs["out"] = gate_bound(out.get("channel_sum out"), o + upd, 4 * U32 * (o.abs() + upd.abs()), "channel_sum, accumulate")
    else:
        errs["out"] = gate_bound(out.get("channel_sum out"), upd, 4 * U32 * upd.abs().clamp_min(1.0), "channel_sum")
    return errs


# =====================================================================================================================
# the chain: stats -> finalize -> bwd_reduce -> bwd_finalize -> apply against autograd of F.batch_norm
# =====================================================================================================================
CHAIN_DIMS = (2, 3, 5, 7, 24)


def check_chain(side):
    """fp32, no ReLU.  Gate per output: 4 x the error of torch's own fp32 CPU run of the same graph against its float64 run, with a
    floor of 16u * max |ref| (the margin of 4: another summation order, the folded coefficients)"""
    g = _gen("chain")
    B, T, H, W, Cc = CHAIN_DIMS
    n = B * T * H * W
    xv, dy = torch.randn(CHAIN_DIMS, generator=g) * 1.5 + 0.3, torch.randn(CHAIN_DIMS, generator=g)
    gamma, beta = 0.5 + torch.rand((Cc,), generator=g), torch.randn((Cc,), generator=g)

    def torch_run(dtype):
        x = xv.to(dtype).permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
        ga, be = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
        with torch.enable_grad():
            y = torch.nn.functional.batch_norm(x, None, None, ga, be, training=True, eps=f32(EPS))
            y.backward(dy.to(dtype).permute(0, 4, 1, 2, 3))
        return dict(dx=x.grad.permute(0, 2, 3, 4, 1).double(), dgamma=ga.grad.double(), dbeta=be.grad.double())

    ref, own = torch_run(torch.float64), torch_run(torch.float32)
    x, dz, dx = Slab(CHAIN_DIMS, F32, values=xv, fill=NAN), Slab(CHAIN_DIMS, F32, values=dy, fill=NAN), Slab(CHAIN_DIMS, F32, fill=SENTINEL)
    over = max(n, apply_vb(Cc))
    xb, gb, db = put_tailed(side, x, over, NAN), put_tailed(side, dz, over, NAN), put_tailed(side, dx, over, SENTINEL)
    rows = side.api.vinet_stats_rows(x.ct(xb))
    part = side.put(torch.full((rows * 2 * Cc,), NAN))
    side.call("vinet_channel_stats", x.ct(xb), F32, part.data_ptr())
    vg, vb = Vec(side, gamma), Vec(side, beta)
    mean, invstd, scale, shift, c1, c2 = (Vec(side, torch.full((Cc,), NAN), out=True) for _ in range(6))
    dg, dbt = Vec(side, torch.zeros(Cc), out=True), Vec(side, torch.zeros(Cc), out=True)
    side.call("vinet_bn_finalize", part.data_ptr(), rows, Cc, 0, float(n), vg.ptr, vb.ptr, EPS, 0.1, None, None, mean.ptr, invstd.ptr, scale.ptr, shift.ptr)
    aff = L.CAffine(scale.ptr, shift.ptr, 0)
    part2 = side.put(torch.full((rows * 2 * Cc,), NAN))
    side.call("vinet_bn_bwd_reduce", dz.ct(gb), x.ct(xb), F32, aff, mean.ptr, invstd.ptr, part2.data_ptr())
    side.call("vinet_bn_bwd_finalize", part2.data_ptr(), rows, Cc, 0, float(n), scale.ptr, 1, dg.ptr, dbt.ptr, invstd.ptr, c1.ptr, c2.ptr)
    side.call("vinet_bn_bwd_apply", dz.ct(gb), x.ct(xb), F32, aff, mean.ptr, invstd.ptr, c1.ptr, c2.ptr, dx.ct(db))
    got = dict(dx=dx.inner(untailed(db, dx, SENTINEL, "chain dx")).double(), dgamma=dg.get("dgamma").double(), dbeta=dbt.get("dbeta").double())
    errs = {}
    for k in ("dx", "dgamma", "dbeta"):
        torch_err = float((own[k] - ref[k]).abs().max())
        lim = max(4 * torch_err, 16 * U32 * float(ref[k].abs().max()))
        err = float((got[k] - ref[k]).abs().max())
        errs[k], errs[k + "_torch_fp32"], errs[k + "_gate"] = err, torch_err, lim
        assert err <= lim, "chain %s: %g > %g (torch's fp32 run: %g)" % (k, err, lim, torch_err)
    return errs


# =====================================================================================================================
# refusals: the return value and the message only -- a refused call launches nothing
# =====================================================================================================================
def _refused(side, needle, fn, *args):
    rc = getattr(side.api, fn)(*args, side.stream)
    assert rc != 0, fn + " accepted what it has to refuse"
    assert needle in side.api.vinet_last_error(), (fn, side.api.vinet_last_error())


def check_refusals(side):
    # a scale without a shift, a shift without a scale (relu at both values)
    x, g = Slab((1, 1, 3, 5, 8), F32, "bn_ref_x", 1), Slab((1, 1, 3, 5, 8), F32, "bn_ref_g", 2)
    xb, gb = side.put(x.base), side.put(g.base)
    vecs = [Vec(side, torch.ones(8)) for _ in range(4)]
    part = side.put(torch.zeros(2 * 8))
    before = part.cpu().clone()
    for relu in (0, 1):
        for aff in (L.CAffine(vecs[0].ptr, None, relu), L.CAffine(None, vecs[1].ptr, relu)):
            _refused(side, b"needs both its scale and its shift", "vinet_bn_bwd_reduce", g.ct(gb), x.ct(xb), F32, aff, vecs[2].ptr, vecs[3].ptr, part.data_ptr())
    # more than 256 channel groups that do not fill whole passes: 257 groups of 8, 257 groups of 4 (C % 8 == 4: the quad route),
    # 514 groups of 4 where a view off the 8-channel grid sends 257 groups of 8 down the quad route
    for Cc, ld, needle in ((2056, 2056, b"8-channel group loop"), (1028, 1028, b"4-channel group loop"), (2056, 2060, b"4-channel group loop")):
        for dt in DTS:
            x, g = Slab((1, 1, 1, 2, Cc), dt, fill=1.0, ld=ld), Slab((1, 1, 1, 2, Cc), dt, fill=1.0, ld=ld)
            xb, gb = side.put(x.base), side.put(g.base)
            big = [Vec(side, torch.ones(Cc)) for _ in range(4)]
            ws, out = side.put(torch.zeros(2 * Cc)), side.put(torch.zeros(Cc))
            _refused(side, needle, "vinet_channel_stats", x.ct(xb), dt, ws.data_ptr())
            _refused(side, needle, "vinet_bn_bwd_reduce", g.ct(gb), x.ct(xb), dt, L.CAffine(big[0].ptr, big[1].ptr, 1), big[2].ptr, big[3].ptr, ws.data_ptr())
            _refused(side, needle, "vinet_channel_sum", x.ct(xb), dt, ws.data_ptr(), 1, out.data_ptr(), 0)
            assert not bool(ws.cpu().any()) and not bool(out.cpu().any())
    x = Slab((1, 1, 3, 5, 8), F32, "bn_ref_x", 1)
    xb, ws, out = side.put(x.base), side.put(torch.zeros(16)), side.put(torch.zeros(8))
    _refused(side, b"channel_sum: bad arguments", "vinet_channel_sum", x.ct(xb), F32, ws.data_ptr(), 3, out.data_ptr(), 0)
    src, dst = side.put(torch.ones(10 * 2 * 8)), side.put(torch.zeros(7 * 2 * 8))
    _refused(side, b"empty chunks", "vinet_bn_partials_fold", src.data_ptr(), 10, 8, dst.data_ptr(), 7)
    assert torch.equal(part.cpu(), before) and not bool(ws.cpu().any()) and not bool(out.cpu().any()) and not bool(dst.cpu().any())


REDUCE_CASES = _build_reduce()
APPLY_CASES = _build_apply()
REDUCE_KERNELS = ("channel_reduce_small_kernel", "channel_reduce_kernel", "channel_reduce8_kernel", "bn_bwd_reduce8_bf16_kernel")
APPLY_KERNELS = ("bn_bwd_apply_kernel", "bn_bwd_apply8_kernel", "bn_bwd_apply8_bf16_kernel", "bn_bwd_apply8_kernel<split>")
