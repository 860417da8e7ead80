"""vinet_bn_bwd_reduce_pool / vinet_bn_bwd_apply_pool (csrc/bn.hip: BatchNorm backward with the 1x3x3 / s(1,2,2) / p(0,1,1) max-pool
backward folded in) against the composition of entry points that are pinned on their own: vinet_maxpool3d_bwd (bit-exact,
tests/test_gpu_pool_kernels.py), then vinet_bn_bwd_reduce / vinet_bn_bwd_apply (float64, tests/bn_cases.py).  The reference is never
the fused kernels themselves.  Shared by tests/test_gpu_bn_pool_kernels.py (the library on the device) and tests/test_bn_pool_host.py
(the refusals, which the library answers before any launch and therefore without a device).

  apply                dy bit-identical to the composition, over the whole buffer (what lies outside the view keeps its bits): same
                       operations, same order, same rounding points
  reduce, exact data   z integers in [-3, 3], dp and the old gradient in [-2, 2], mean in halves, invstd and scale powers of two, shift
                       integers (bn_cases._exact_params): dz is an integer of magnitude <= 10, every term a multiple of 1/4, every fp32
                       sum exact in ANY order -- the column totals equal the composition's bit for bit
  reduce, random data  the float64 column totals against the float64 model (terms g, g * (z - mean) * invstd with g = the dz the
                       composition stored, gated in float64) within the bound of bn_cases.check_reduce, which is called itself (its
                       runner and reference replaced by this module's): the bound is imported, not restated
  partials table       prefilled with NaN, a sentinel behind it: every row written, nothing behind them
  the old gradient     the reduce pass leaves it alone; the apply pass out of place leaves it alone
"""
import ctypes as C

import torch

from tests import bn_cases as BC
from tests.tail_cases import BF16, BITS, F32, Slab
from vinet_amd import _lib as L

K133 = ((1, 3, 3), (1, 2, 2), (0, 1, 1))
DIMS = ((1, 1, 1, 1), (1, 1, 2, 2), (2, 3, 5, 7), (1, 2, 6, 4), (2, 2, 9, 16))
CS = (8, 24, 64, 192, 520)
PLANES = ("real", "ties", "fan", "corner")


class FusedPoolStubs:
    """mixed into the CPU model of the ABI (tests/abi_emulator.py, which itself stays without them): the predicate and the two
    fused entry points, built from the model's own pool backward and BatchNorm backward (the reduce stub stores dz as the pool
    backward would, the apply stub continues from it).  For tests of what the ENGINE calls."""

    def vinet_bn_bwd_pool_ok(self, pd, z, dp, dx, dtype):
        return 1

    def vinet_bn_bwd_reduce_pool(self, pd, dp, argmax, gacc, accumulate, z, dtype, fwd, mean, invstd, partials, stream):
        rc = self.vinet_maxpool3d_bwd(pd, dp, argmax, gacc, accumulate, stream)
        return rc or self.vinet_bn_bwd_reduce(gacc, z, dtype, fwd, mean, invstd, partials, stream)

    def vinet_bn_bwd_apply_pool(self, pd, dp, argmax, gacc, accumulate, z, dtype, fwd, mean, invstd, c1, c2, dx, stream):
        return self.vinet_bn_bwd_apply(gacc, z, dtype, fwd, mean, invstd, c1, c2, dx, stream)


def pool_desc(dt=BF16, geo=K133):
    k, s, p = geo
    return L.CPoolDesc(dt, *k, *s, *p)


def pooled(dims):
    B, T, H, W, Cc = dims
    return (B, T, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc)


def synthetic_plane(kind, dims):
    """argmax codes [B,T,oH,oW,C] (uint8) that no forward pool need produce but every backward has to honour.
    fan: windows (even, even) pick tap (2,2), (even, odd) tap (2,0), (odd, even) tap (0,2), (odd, odd) tap (0,0) -- all four windows of
    every block (even, even) point at its odd/odd input (the maximum fan-in), and no window points into a block (odd, odd);
    corner: every window picks tap (0,0), the odd/odd input of the block up and left of it: the last block row and column get nothing.
    A tap that would lie outside the image is replaced by the centre tap (1,1), which never does."""
    B, T, H, W, Cc = dims
    _, _, oH, oW, _ = pooled(dims)
    ho = torch.arange(oH).view(oH, 1).expand(oH, oW)
    wo = torch.arange(oW).view(1, oW).expand(oH, oW)
    if kind == "fan":
        kh, kw = 2 - 2 * (ho % 2), 2 - 2 * (wo % 2)
    else:
        kh, kw = torch.zeros_like(ho), torch.zeros_like(wo)
    h, w = 2 * ho - 1 + kh, 2 * wo - 1 + kw
    ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
    code = torch.where(ok, kh * 3 + kw, torch.full_like(kh, 4)).to(torch.uint8)
    return code.view(1, 1, oH, oW, 1).expand(B, T, oH, oW, Cc).contiguous()


def _vectors(Cc, data, g):
    if data == "exact":
        mean, scale, shift = BC._exact_params(Cc, g)
        invstd = BC._pick([0.5, 1.0, 2.0], Cc, g)
        c1 = BC._pick([-0.75, -0.25, 0.25, 0.75], Cc, g)
        c2 = torch.randint(-2, 3, (Cc,), generator=g).float()
    else:
        mean, invstd = 0.5 * torch.randn((Cc,), generator=g), 0.5 + 1.5 * torch.rand((Cc,), generator=g)
        scale = (0.5 + torch.rand((Cc,), generator=g)) * BC._pick([-1.0, 1.0], Cc, g)
        shift = 0.5 * torch.randn((Cc,), generator=g)
        c1, c2 = 0.1 * torch.randn((Cc,), generator=g), 0.1 * torch.randn((Cc,), generator=g)
    return mean, invstd, scale, shift, c1, c2


def _tensor(dims, data, lim, g):
    if data == "exact":
        return torch.randint(-lim, lim + 1, dims, generator=g).float()
    return torch.randn(dims, generator=g)


class _ReduceCase:
    """what bn_cases.check_reduce reads of a case"""

    def __init__(self, what, nvox, data, z):
        self.what, self.nvox, self.data, self.opts, self._z = what, nvox, data, {}, z

    def slabs(self):
        return self._z, None

    def __repr__(self):
        return self.what


def gate_reduce(monkeypatch, side, what, nvox, data, z, rows, table, ref, mag):
    """bn_cases.check_reduce on a table and a reference of this module's: exact data bit-equal, random data within ITS bound"""
    monkeypatch.setattr(BC, "run_reduce", lambda *a: (rows, table))
    monkeypatch.setattr(BC, "reduce_ref", lambda case: (ref, mag))
    try:
        return BC.check_reduce(side, _ReduceCase(what, nvox, data, z))
    finally:
        monkeypatch.undo()


def _table(side, rows, Cc):
    n = rows * 2 * Cc
    return side.put(torch.cat([torch.full((n,), BC.NAN), torch.full((BC.SLACK,), BC.SENTINEL)])), n


def _read_table(part, n, rows, Cc, what):
    got = part.cpu()
    assert bool((got[n:] == BC.SENTINEL).all()), what + ": wrote behind the partials table"
    table = got[:n].view(rows, 2, Cc)
    assert bool(torch.isfinite(table).all()), "%s: %d of the table's floats were not written" % (what, int((~torch.isfinite(table)).sum()))
    return table


def _same_bits(a, b, what):
    a, b = a.cpu().view(BITS[BF16]), b.cpu().view(BITS[BF16])
    assert torch.equal(a, b), "%s: %d elements differ" % (what, int((a != b).sum()))


def check_case(side, monkeypatch, dims4, Cc, acc):
    """every (data, ReLU, argmax plane, gradient view) combination of one shape; returns the worst reduce error / bound"""
    dims, worst = tuple(dims4) + (Cc,), 0.0
    B, T, H, W, _ = dims
    nvox, pdims = B * T * H * W, pooled(dims)
    api, pd = side.api, pool_desc()
    for data in ("exact", "random"):
        g = BC._gen("bn_pool", dims, acc, data)
        z = Slab(dims, BF16, values=_tensor(dims, data, 3, g))
        dp = Slab(pdims, BF16, values=_tensor(pdims, data, 2, g))
        mean, invstd, scale, shift, c1, c2 = _vectors(Cc, data, g)
        zb, dpb = side.put(z.base), side.put(dp.base)
        vm, vi, vs, vh, v1, v2 = (BC.Vec(side, v) for v in (mean, invstd, scale, shift, c1, c2))
        rows = api.vinet_stats_rows(z.ct(zb))
        planes = {}
        for kind in PLANES:
            if kind in ("real", "ties"):
                # the forward pool itself, over relu(bn(z)) (ties: over a constant, where the first maximum in scan order wins)
                src = z if kind == "real" else Slab(dims, BF16, fill=1.0)
                am = side.put(torch.full((pdims[0] * pdims[1] * pdims[2] * pdims[3] * Cc,), 255, dtype=torch.uint8))
                y = Slab(pdims, BF16, fill=0.0)
                sb, yb = side.put(src.base), side.put(y.base)
                side.call("vinet_maxpool3d", C.byref(pd), src.ct(sb), L.CAffine(vs.ptr, vh.ptr, 1), y.ct(yb), am.data_ptr())
                assert int(am.max()) <= 8
            else:
                am = side.put(synthetic_plane(kind, dims).reshape(-1))
            planes[kind] = am
        for relu in (1, 0):
            fwd = L.CAffine(vs.ptr, vh.ptr, relu)
            for kind, am in planes.items():
                for form in ("dense", "tslice"):
                    what = "%r C%d acc%d %s relu%d %s %s" % (dims4, Cc, acc, data, relu, kind, form)
                    old = Slab(dims, BF16, values=_tensor(dims, data, 2, g), **BC.view_geo(form, dims, Cc))
                    # ---- the composition: pool backward into the gradient buffer, reduce and apply (in place) over it
                    rb = side.put(old.base)
                    side.call("vinet_maxpool3d_bwd", C.byref(pd), dp.ct(dpb), am.data_ptr(), old.ct(rb), acc)
                    dz = old.inner(rb.cpu()).clone()
                    rpart, n = _table(side, rows, Cc)
                    side.call("vinet_bn_bwd_reduce", old.ct(rb), z.ct(zb), BF16, fwd, vm.ptr, vi.ptr, rpart.data_ptr())
                    rtable = _read_table(rpart, n, rows, Cc, what + " (composition)")
                    side.call("vinet_bn_bwd_apply", old.ct(rb), z.ct(zb), BF16, L.CAffine(vs.ptr, vh.ptr, relu), vm.ptr, vi.ptr, v1.ptr, v2.ptr, old.ct(rb))
                    # ---- fused reduce
                    fb = side.put(old.base)
                    fpart, n = _table(side, rows, Cc)
                    side.call("vinet_bn_bwd_reduce_pool", C.byref(pd), dp.ct(dpb), am.data_ptr(), old.ct(fb), acc, z.ct(zb), BF16, fwd, vm.ptr, vi.ptr,
                              fpart.data_ptr())
                    _same_bits(fb, old.base, what + ": the reduce pass changed the gradient buffer")
                    ftable = _read_table(fpart, n, rows, Cc, what)
                    if data == "exact":
                        ref, mag = rtable.double().sum(0), None
                    else:
                        t0 = dz.double() * BC.relu_gate(z.wide(), "affine" if relu else "none", scale, shift)
                        t1 = t0 * (z.wide() - mean.double()) * invstd.double()
                        flat = lambda t: t.reshape(-1, Cc)
                        ref = torch.stack([flat(t0).sum(0), flat(t1).sum(0)])
                        mag = torch.stack([flat(t0).abs().sum(0), flat(t1).abs().sum(0)])
                    res = gate_reduce(monkeypatch, side, what, nvox, data, z, rows, ftable, ref, mag)
                    worst = max(worst, res.get("err_over_bound", 0.0))
                    # ---- fused apply, in place and out of place (dense result beside an untouched gradient buffer)
                    side.call("vinet_bn_bwd_apply_pool", C.byref(pd), dp.ct(dpb), am.data_ptr(), old.ct(fb), acc, z.ct(zb), BF16, fwd, vm.ptr, vi.ptr,
                              v1.ptr, v2.ptr, old.ct(fb))
                    _same_bits(fb, rb, what + ": apply in place")
                    gb = side.put(old.base)
                    out = Slab(dims, BF16, fill=BC.SENTINEL)
                    ob = side.put(out.base)
                    side.call("vinet_bn_bwd_apply_pool", C.byref(pd), dp.ct(dpb), am.data_ptr(), old.ct(gb), acc, z.ct(zb), BF16, fwd, vm.ptr, vi.ptr,
                              v1.ptr, v2.ptr, out.ct(ob))
                    _same_bits(gb, old.base, what + ": apply out of place changed the gradient buffer")
                    _same_bits(out.inner(ob.cpu()).contiguous(), old.inner(rb.cpu()).contiguous(), what + ": apply out of place")
        for v in (vm, vi, vs, vh, v1, v2):
            v.get("parameter vector")
    return worst


def check_refusals(side):
    """a wrong geometry, fp32, C not a multiple of 8 and mismatched dims: the predicate says no with a reason, both entry points return an
    error, and nothing is launched -- the partials and the gradient buffer keep their bits"""
    api = side.api
    dims = (1, 2, 5, 6, 16)
    vecs = [BC.Vec(side, torch.ones(16)) for _ in range(6)]
    fwd = L.CAffine(vecs[0].ptr, vecs[1].ptr, 1)
    part = side.put(torch.full((4 * 2 * 16,), BC.SENTINEL))

    def refused(needle, pd, z, dp, dx, dt):
        zb, dpb, xb = side.put(z.base), side.put(dp.base), side.put(dx.base)
        am = side.put(torch.zeros(dp.base.numel(), dtype=torch.uint8))
        assert api.vinet_bn_bwd_pool_ok(C.byref(pd), z.ct(zb), dp.ct(dpb), dx.ct(xb), dt) == 0, needle
        assert needle in api.vinet_last_error(), (needle, api.vinet_last_error())
        for accum in (0, 1):
            BC._refused(side, needle, "vinet_bn_bwd_reduce_pool", C.byref(pd), dp.ct(dpb), am.data_ptr(), dx.ct(xb), accum, z.ct(zb), dt, fwd,
                        vecs[2].ptr, vecs[3].ptr, part.data_ptr())
            BC._refused(side, needle, "vinet_bn_bwd_apply_pool", C.byref(pd), dp.ct(dpb), am.data_ptr(), dx.ct(xb), accum, z.ct(zb), dt, fwd,
                        vecs[2].ptr, vecs[3].ptr, vecs[4].ptr, vecs[5].ptr, dx.ct(xb))
        assert torch.equal(xb.cpu().view(BITS[dx.dt]), dx.base.view(BITS[dx.dt])), needle + ": a refused call wrote the gradient"
        assert bool((part.cpu() == BC.SENTINEL).all()), needle + ": a refused call wrote partials"

    def slabs(d, dt=BF16, pd=None):
        return Slab(d, dt, fill=1.0), Slab(pooled(d) if pd is None else pd, dt, fill=1.0), Slab(d, dt, fill=1.0)

    ok = pool_desc()
    z, dp, dx = slabs(dims)
    zb, dpb, xb = side.put(z.base), side.put(dp.base), side.put(dx.base)
    assert api.vinet_bn_bwd_pool_ok(C.byref(ok), z.ct(zb), dp.ct(dpb), dx.ct(xb), BF16) == 1, api.vinet_last_error()
    for geo in (((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((1, 3, 3), (1, 1, 1), (0, 1, 1)), ((1, 3, 3), (1, 2, 2), (0, 0, 0)), ((1, 2, 2), (1, 2, 2), (0, 0, 0))):
        refused(b"is not the 1x3x3 / s(1,2,2) / p(0,1,1) pool", pool_desc(BF16, geo), z, dp, dx, BF16)
    refused(b"bf16 only", pool_desc(F32), *slabs(dims, F32), F32)
    refused(b"bf16 only", ok, z, dp, dx, F32)
    refused(b"not a whole number of 8-channel groups", ok, *slabs((1, 2, 5, 6, 12)), BF16)
    refused(b"is not the pooled shape", ok, *slabs(dims, pd=(1, 2, 2, 3, 16)), BF16)
    refused(b"is not the pooled shape", ok, *slabs(dims, pd=(1, 1, 3, 3, 16)), BF16)
    refused(b"z and dx differ", ok, z, dp, Slab((1, 2, 5, 7, 16), BF16, fill=1.0), BF16)
