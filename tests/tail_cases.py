"""The small kernels around the network at their edges: case tables, float64 references and the runners that the host test
(tests/test_tail_cases_host.py, CPU model of the ABI) and the GPU test (tests/test_gpu_tail_kernels.py, libvinet_hip.so) share.

Families: the losses, Adam, fill and the bilinear fusion (csrc/loss_adam.hip, csrc/layout.hip), the 2x upsample
(csrc/resample.hip), vinet_act_bwd (csrc/bn.hip) and vinet_unfold1d (csrc/layout.hip).  Every reference here is plain torch /
numpy in float64 and shares no code with tests/abi_emulator.py.  References read the inputs AFTER rounding to the storage
type (bf16 inputs are drawn, rounded, then widened), so what a gate measures is the kernel's own arithmetic and its final
rounding.  A `Side` says where a case runs; each check_* function runs one case there, asserts its gates and returns the
measured errors (the GPU test writes them into the parity report)."""
import ctypes as C
import functools

import numpy as np
import torch

from vinet_amd import engine as E
from vinet_amd import synth

F32, BF16 = E.F32, E.BF16
DTS = [F32, BF16]
DTN = {F32: "f32", BF16: "bf16"}
TDT = E.TORCH_DT
BITS = {F32: torch.int32, BF16: torch.int16}
U32 = 2.0 ** -24        # unit round-off of fp32 (24-bit significand, round to nearest)


def f32(x):
    """a host double as the library receives it through a `float` argument"""
    return float(np.float32(x))


class Side:
    """where a case runs: the CPU model of the ABI on host memory, or the library on the device"""

    def __init__(self, api, dev="cpu", stream=0):
        self.api, self.dev, self.stream = api, torch.device(dev), stream

    def put(self, t):
        return t.detach().contiguous().clone().to(self.dev)

    def call(self, fn, *args):
        rc = getattr(self.api, fn)(*args, self.stream)
        if rc != 0:
            raise AssertionError("%s rc=%d: %r" % (fn, rc, self.api.vinet_last_error()))
        if self.dev.type != "cpu":
            torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


def gate(got, ref, tol, what):
    """max |got - ref| <= tol * max(1, max |ref|), the scaling of tests/test_gpu_kernels.py; returns the measured error"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(ref).all()), what + ": reference not finite"
    assert bool(torch.isfinite(got).all()), what + ": result not finite"
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    lim = tol * max(1.0, float(ref.abs().max())) if ref.numel() else tol
    assert err <= lim, "%s: max abs diff %g > %g" % (what, err, lim)
    return err


def gate_bound(got, ref, bound, what):
    """elementwise |got - ref| <= bound (a derived round-off bound); returns the worst error / bound"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), what + ": not finite"
    err = (got - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), "%s: %d elements over their bound, worst %g against %g" % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
    return float((err / bound.clamp_min(1e-300)).max())


class Slab:
    """a channels-last [B,T,H,W,C] view inside a flat buffer: dense, or a channel slice (ld > C) and / or a T slice of a wider
    one.  `base` is the CPU buffer in its storage type; the same geometry is then laid over a copy of it on either side."""

    def __init__(self, dims, dt, name=None, seed=0, ld=None, c_off=0, t_total=None, t_off=0, fill=None, values=None):
        B, T, H, W, Cc = dims
        self.dims, self.dt = dims, dt
        self.ld = Cc if ld is None else ld
        tt = T if t_total is None else t_total
        self.sB = tt * H * W * self.ld
        self.off = t_off * H * W * self.ld + c_off
        n = B * self.sB
        self.base = (synth.normal(name, (n,), seed) if fill is None else torch.full((n,), float(fill))).to(TDT[dt])
        if values is not None:
            self.inner(self.base).copy_(values.to(TDT[dt]))

    def view(self, buf):
        B, T, H, W, Cc = self.dims
        return E.View(buf, self.off, B, T, H, W, Cc, self.ld, self.sB, self.dt)

    def inner(self, buf):
        return self.view(buf).torch5()

    def ct(self, buf):
        return C.byref(self.view(buf).ct())

    def wide(self):
        """the view's contents in float64"""
        return self.inner(self.base).double()

    def assert_outside_untouched(self, after, what):
        """every element of the buffer that the view does not cover has the bits it started with"""
        mask = torch.ones(self.base.numel(), dtype=torch.bool)
        self.view(mask).torch5()[...] = False
        a, b = after.cpu().view(BITS[self.dt])[mask], self.base.view(BITS[self.dt])[mask]
        assert torch.equal(a, b), "%s: %d elements outside the view changed" % (what, int((a != b).sum()))


# =====================================================================================================================
# losses: vinet_loss_fwd / vinet_loss_bwd
# =====================================================================================================================
LOSS_EPS = 2.2204e-16
LOSS_NAMES = ["kldiv", "cc", "similarity", "nss"]
# (B, n): below one wave, a wave + 1, below / at / past the 1024-lane workgroup, B = 1
LOSS_SHAPES = [(1, 2), (3, 3), (1, 63), (3, 65), (2, 1023), (1, 1024), (3, 1025), (2, 2241)]
LOSS_HW = {2: (1, 2), 3: (1, 3), 63: (7, 9), 65: (5, 13), 1023: (31, 33), 1024: (32, 32), 1025: (25, 41), 2241: (27, 83)}
LOSS_BWD_SHAPES = [(1, 63), (3, 65), (3, 1025)]          # n < 64, 64 < n < 1024, n > 1024
# name, *gscale (None: NULL), coeff, accumulate
LOSS_BWD_ARGS = [("gs_neg", 0.7, -1.0, 0), ("nogs_quarter", None, 0.25, 0), ("gs_acc", 0.7, 1.0, 1)]


def loss_inputs(which, g64, B, n):
    """s uniform in [0.01, 0.99]; gt = synth.gt_map reshaped (NSS: its upper half as a 0/1 fixation map)"""
    s = synth.uniform("tail_loss_s", (B, n), 100 + n, 0.01, 0.99)
    H, W = LOSS_HW[n]
    g = synth.gt_map(B, H, W, 200 + n).reshape(B, n)
    if which == 3:
        g = (g > 0.5 * g.amax(1, keepdim=True)).float()
    return s, (g.double() if g64 else g)


def loss_per_sample(which, s, g):
    """loss.py's kldiv / cc / similarity / nss per sample, on float64 [B, n]"""
    def norm01(m):
        lo, hi = m.min(1, keepdim=True)[0], m.max(1, keepdim=True)[0]
        return (m - lo) / (hi - lo)
    if which == 0:
        p, q = s / s.sum(1, keepdim=True), g / g.sum(1, keepdim=True)
        return (q * torch.log(LOSS_EPS + q / (p + LOSS_EPS))).sum(1)
    if which == 1:
        a = (s - s.mean(1, keepdim=True)) / s.std(1, keepdim=True)
        b = (g - g.mean(1, keepdim=True)) / g.std(1, keepdim=True)
        return (a * b).sum(1) / torch.sqrt((a * a).sum(1) * (b * b).sum(1))
    if which == 2:
        a, b = norm01(s), norm01(g)
        return torch.min(a / a.sum(1, keepdim=True), b / b.sum(1, keepdim=True)).sum(1)
    z = (s - s.mean(1, keepdim=True)) / (s.std(1, keepdim=True) + LOSS_EPS)
    return (z * g).sum(1) / g.sum(1)


def loss_grad_ref(which, s, g):
    """d mean_b(loss_b) / d s by autograd, float64"""
    x = s.double().clone().requires_grad_(True)
    with torch.enable_grad():
        loss_per_sample(which, x, g.double()).mean().backward()
    return x.grad


def loss_well_posed(which, s, g):
    """what the cases promise: a unique minimum of s per sample (the similarity gradient at a tie is not defined), a
    non-constant ground truth, at least one fixation per NSS sample"""
    for b in range(s.shape[0]):
        assert int((s[b] == s[b].min()).sum()) == 1, "tied minimum in sample %d" % b
        assert float(g[b].max()) > float(g[b].min()), "constant ground truth in sample %d" % b
    if which == 3:
        assert s.shape[1] >= 2 and bool((g.sum(1) >= 1).all()) and bool(((g == 0) | (g == 1)).all())


def _loss_fwd(side, which, g64, s, g):
    B, n = s.shape
    sd, gd = side.put(s), side.put(g)
    saved, loss = side.put(torch.zeros(B * 8, dtype=torch.float64)), side.put(torch.zeros(1))
    side.call("vinet_loss_fwd", which, sd.data_ptr(), gd.data_ptr(), g64, B, n, saved.data_ptr(), loss.data_ptr())
    return sd, gd, saved, loss


def check_loss_fwd(side, which, g64, B, n):
    """the batch value and the per-sample slot of `saved` (2: kldiv, 5: the others, csrc/loss_adam.hip) at 1e-6"""
    s, g = loss_inputs(which, g64, B, n)
    per = loss_per_sample(which, s.double(), g.double())
    _, _, saved, loss = _loss_fwd(side, which, g64, s, g)
    return dict(loss=gate(loss.cpu(), per.mean().reshape(1), 1e-6, "loss value"),
                per_sample=gate(saved.cpu().view(B, 8)[:, 2 if which == 0 else 5], per, 1e-6, "per-sample slot of saved"))


def check_loss_bwd(side, which, g64, B, n, gscale, coeff, accumulate):
    s, g = loss_inputs(which, g64, B, n)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32)
    ref = loss_grad_ref(which, s, g) * ((1.0 if gs is None else float(gs[0])) * coeff)
    gmax = float(ref.abs().max())
    # accumulate: ds starts from random values of magnitude <= max |g_ref|
    d0 = (synth.uniform("tail_loss_d0", (B, n), 300 + n, -1.0, 1.0) * gmax).float() if accumulate else torch.zeros(B, n)
    sd, gd, saved, _ = _loss_fwd(side, which, g64, s, g)
    ds, gsd = side.put(d0), None if gs is None else side.put(gs)
    side.call("vinet_loss_bwd", which, sd.data_ptr(), gd.data_ptr(), g64, B, n, saved.data_ptr(), _p(gsd), coeff, accumulate, ds.data_ptr())
    got = ds.cpu().double()
    assert bool(torch.isfinite(got).all())
    if not accumulate:
        err = float((got - ref).abs().max())
        assert err <= 1e-6 * gmax + 1e-12, "loss bwd: %g against scale %g" % (err, gmax)
        return dict(grad_rel=err / gmax)
    # ds = fl32(d0 + fl32(g)): TWO fp32 roundings on the path (g computed in fp64 and converted, then the fp32 addition), so
    # |error| <= 2 * 2^-24 * (|d0| + |g|); the largest such sum bounds every element.  (2.4e-7 of the scale: tighter than the
    # plain gradient's 1e-6 gate, which no longer means anything once d0 is in the sum.)  1e-12: the plain gate's floor.
    lim = 2 * U32 * float((d0.double().abs() + ref.abs()).max()) + 1e-12
    err = float((got - (d0.double() + ref)).abs().max())
    assert err <= lim, "loss bwd, accumulate: %g > %g" % (err, lim)
    return dict(acc_err_over_bound=err / lim)


# =====================================================================================================================
# Adam and fill
# =====================================================================================================================
ADAM_HP = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
ADAM_CAP_N = 8192 * 256 * 4 + 5          # just past the grid cap of 8192 blocks x 256 lanes x 4 elements: the stride loop repeats
# name, n, grad_scale, steps, step count before (non-zero: a resumed run with non-zero m, v)
ADAM_CASES = [("n%d_gs%s" % (n, nm), n, gs, 3, 0) for n in (1, 3, 4, 5, 1027) for nm, gs in (("1", 1.0), ("8th", 0.125), ("3rd", 1.0 / 3.0))]
ADAM_CASES += [("resumed", 1027, 1.0 / 3.0, 3, 7), ("grid_cap", ADAM_CAP_N, 0.125, 1, 0)]
ADAM_PAD = 2.5                            # value of the padding floats behind n: the kernel must not touch them


def adam_inputs(case):
    name, n, gs, steps, t0 = case
    n4 = (n + 3) // 4 * 4                 # optim.py allocates the flat buffers at a multiple of 4 floats
    def pad(t):
        return torch.cat([t.float(), torch.full((n4 - n,), ADAM_PAD)])
    p = pad(synth.uniform("tail_adam_p", (n,), 1, -2.0, 2.0))
    g = [pad(synth.uniform("tail_adam_g", (n,), 10 + k, -1.0, 1.0)) for k in range(steps)]
    if t0:
        m, v = pad(synth.uniform("tail_adam_m", (n,), 2, -0.3, 0.3)), pad(synth.uniform("tail_adam_v", (n,), 3, 1e-4, 1e-1))
    else:
        m, v = pad(torch.zeros(n)), pad(torch.zeros(n))
    return p, g, m, v


def adam_ref(case):
    """the Adam recurrence in float64 on the fp32 inputs and the fp32-rounded scalars"""
    name, n, gs, steps, t0 = case
    p, g, m, v = adam_inputs(case)
    p, m, v = p[:n].double().numpy(), m[:n].double().numpy(), v[:n].double().numpy()
    lr, b1, b2, eps = (f32(ADAM_HP[k]) for k in ("lr", "b1", "b2", "eps"))
    for k in range(steps):
        t = t0 + k + 1
        bc1, bc2 = f32(1 - 0.9 ** t), f32(1 - 0.999 ** t)
        ge = g[k][:n].double().numpy() * f32(gs)
        m = b1 * m + (1 - b1) * ge
        v = b2 * v + (1 - b2) * ge * ge
        p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def check_adam(side, case):
    name, n, gs, steps, t0 = case
    p, g, m, v = (adam_inputs(case))
    pd, md, vd = side.put(p), side.put(m), side.put(v)
    for k in range(steps):
        t = t0 + k + 1
        gd = side.put(g[k])
        side.call("vinet_adam_step", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, ADAM_HP["lr"], ADAM_HP["b1"],
                  ADAM_HP["b2"], ADAM_HP["eps"], 1 - 0.9 ** t, 1 - 0.999 ** t, gs)
    errs = {}
    for nm, got, ref in zip("pmv", (pd, md, vd), adam_ref(case)):
        got = got.cpu()
        errs[nm] = gate(got[:n], ref, 1e-6, "adam " + nm)
        assert bool((got[n:] == ADAM_PAD).all()), "adam %s: wrote behind n" % nm
    return errs


FILL_NS = [0, 1, 4096 * 256 + 3]         # nothing to do; one element; past the grid cap of 4096 blocks x 256 lanes


def check_fill(side, n):
    """vinet_fill_f32 writes exactly n floats: a sentinel sits just behind them (and, at n = 0, where the first would go)"""
    buf = side.put(torch.full((n + 8,), -1.5))
    side.call("vinet_fill_f32", buf.data_ptr(), n, 3.5)
    got = buf.cpu()
    assert bool((got[:n] == 3.5).all()), "fill: %d of %d elements not written" % (int((got[:n] != 3.5).sum()), n)
    assert bool((got[n:] == -1.5).all()), "fill wrote past n"


# =====================================================================================================================
# bilinear fusion: vinet_bilinear_fwd / vinet_bilinear_bwd
# =====================================================================================================================
BIL_CASES = [
    ("smallest", (1, 1, 1, 1, 1)),
    ("lane_guard_o_tail", (2, 63, 5, 2, 15)),        # c < C lane guard, O no multiple of 16, I = 5: the fourth wave has no input
    ("two_ctiles_j4", (2, 65, 3, 4, 17)),            # two channel tiles, J = 4, I = 3: one input per wave, one wave idle
    ("avinet_ijo", (1, 128, 42, 3, 336)),
    ("b33_pairs", (33, 64, 6, 1, 16)),               # B * ctiles = 33 > 32: the pair loop of the weight gradient repeats, J = 1
    ("c704_pairs", (3, 704, 4, 3, 32)),              # 33 pairs through 11 channel tiles
    ("i48", (1, 8, 48, 2, 9)),                       # I at BIL_MAX_I with I * J + 1 <= 128
]
# which of dx1, dx2, dw, dbias are asked for (the others are NULL)
BIL_BWD_MODES = [("all", (1, 1, 1, 1)), ("dx1_only", (1, 0, 0, 0)), ("dx2_only", (0, 1, 0, 0)), ("dw_no_dbias", (0, 0, 1, 0)),
                 ("dx_no_dw", (1, 1, 0, 0))]
BIL_FWD_TOL = {F32: 2e-5, BF16: 2e-2}
BIL_BWD_TOL = {F32: 5e-5, BF16: 3e-2}
BIL_FWD_ONLY = (1, 8, 48, 4, 9)                     # I * J = 192: accepted forward, refused backward (see check_bilinear_rejects)


BIL_FENCE = 1024                                     # elements behind every flat buffer of a case: more than one row of C <= 704
BIL_MARK = 9.0


def _fenced(side, t, mark=float("nan")):
    """the flat tensor with a fence behind it.  Inputs: NaN, so a row read one past the end (an `o < O` guard gone) poisons the
    result instead of reading someone else's memory unnoticed; outputs: a mark that must survive."""
    return side.put(torch.cat([t, torch.full((BIL_FENCE,), mark).to(t.dtype)]))


def _unfenced(buf, n, what):
    got = buf.cpu()
    assert bool((got[n:] == BIL_MARK).all()), "bilinear: wrote behind the end of " + what
    return got[:n]


@functools.lru_cache(maxsize=None)
def bil_inputs(shape, dt):
    B, Cc, I, J, O = shape
    r = lambda name, n, seed, scale=1.0: synth.normal("tail_bil_" + name, (n,), seed) * scale
    return dict(x1=r("x1", B * I * Cc, 1).to(TDT[dt]), x2=r("x2", B * J * Cc, 2).to(TDT[dt]), dout=r("do", B * O * Cc, 5).to(TDT[dt]),
                w=r("w", O * I * J, 3, 0.1), bias=r("b", O, 4), dw0=r("dw0", O * I * J, 6), db0=r("db0", O, 7))


@functools.lru_cache(maxsize=None)
def bil_ref(shape, dt):
    """einsum in float64; `abs_dw` / `abs_db`: the sums of |terms| of the weight / bias gradient"""
    B, Cc, I, J, O = shape
    t = bil_inputs(shape, dt)
    a, b, g = t["x1"].double().view(B, I, Cc), t["x2"].double().view(B, J, Cc), t["dout"].double().view(B, O, Cc)
    w = t["w"].double().view(O, I, J)
    wb = torch.einsum("oij,bjc->boic", w, b)
    return dict(out=torch.einsum("bic,boic->boc", a, wb), dx1=torch.einsum("boc,boic->bic", g, wb),
                dx2=torch.einsum("boc,oij,bic->bjc", g, w, a), dw=torch.einsum("boc,bic,bjc->oij", g, a, b), db=g.sum((0, 2)),
                abs_dw=torch.einsum("boc,bic,bjc->oij", g.abs(), a.abs(), b.abs()), abs_db=g.abs().sum((0, 2)))


def check_bilinear_fwd(side, shape, dt, with_bias):
    B, Cc, I, J, O = shape
    t, ref = bil_inputs(shape, dt), bil_ref(shape, dt)
    x1, x2, w = _fenced(side, t["x1"]), _fenced(side, t["x2"]), _fenced(side, t["w"])
    bias = _fenced(side, t["bias"]) if with_bias else None
    out = _fenced(side, torch.zeros(B * O * Cc).to(TDT[dt]), BIL_MARK)
    side.call("vinet_bilinear_fwd", x1.data_ptr(), x2.data_ptr(), dt, w.data_ptr(), _p(bias), B, Cc, I, J, O, out.data_ptr())
    want = ref["out"] + (t["bias"].double().view(1, O, 1) if with_bias else 0.0)
    return dict(out=gate(_unfenced(out, B * O * Cc, "out").view(B, O, Cc), want, BIL_FWD_TOL[dt], "bilinear fwd"))


def bil_w_roundings(B, Cc):
    """fp32 roundings between one product and the final dw[o][i][j] / dbias[o] in bilinear_bwd_w_kernel (csrc/loss_adam.hip): a
    workgroup takes `per` of the B * ceil(C/64) (batch, channel tile) pairs; per pair a weight-gradient term is the rounded
    product g*a (1), one of 32 fused multiply-adds of its half of the 64 channels (<= 32), and a0 + a1 (1); then the
    workgroup's `per` additions into its accumulator and one atomic addition per workgroup (`splits`) onto the caller's value.
    A bias term goes through the 64 additions of its channel sweep in place of 1 + 32 + 1."""
    pairs = B * ((Cc + 63) // 64)
    splits = min(pairs, 32)
    per = -(-pairs // splits)
    return 1 + 32 + 1 + per + splits, 64 + per + splits, pairs


def check_bilinear_bwd(side, shape, dt, mode):
    """`mode`: which outputs are asked for.  dx1 / dx2 are stored, dw / dbias ADD to what the caller's buffers hold."""
    B, Cc, I, J, O = shape
    want1, want2, wantw, wantb = mode
    t, ref = bil_inputs(shape, dt), bil_ref(shape, dt)
    x1, x2, do, w = _fenced(side, t["x1"]), _fenced(side, t["x2"]), _fenced(side, t["dout"]), _fenced(side, t["w"])
    d1 = _fenced(side, torch.zeros(B * I * Cc).to(TDT[dt]), BIL_MARK) if want1 else None
    d2 = _fenced(side, torch.zeros(B * J * Cc).to(TDT[dt]), BIL_MARK) if want2 else None
    dw = _fenced(side, t["dw0"], BIL_MARK) if wantw else None
    db = _fenced(side, t["db0"], BIL_MARK) if wantb else None
    side.call("vinet_bilinear_bwd", x1.data_ptr(), x2.data_ptr(), do.data_ptr(), dt, w.data_ptr(), B, Cc, I, J, O, _p(d1), _p(d2), _p(dw), _p(db))
    errs = {}
    if want1:
        errs["dx1"] = gate(_unfenced(d1, B * I * Cc, "dx1").view(B, I, Cc), ref["dx1"], BIL_BWD_TOL[dt], "bilinear bwd dx1")
    if want2:
        errs["dx2"] = gate(_unfenced(d2, B * J * Cc, "dx2").view(B, J, Cc), ref["dx2"], BIL_BWD_TOL[dt], "bilinear bwd dx2")
    kw, kb, pairs = bil_w_roundings(B, Cc)
    for key, buf, init, r, absr, k in (("dw", dw, t["dw0"].double().view(O, I, J), ref["dw"], ref["abs_dw"], kw),
                                       ("dbias", db, t["db0"].double(), ref["db"], ref["abs_db"], kb)):
        if buf is None:
            continue
        got = _unfenced(buf, init.numel(), key).view(init.shape)
        if pairs <= 32:
            errs[key] = gate(got, init + r, BIL_BWD_TOL[dt], "bilinear bwd " + key)
        else:
            # more than 32 pairs: sums of ~2000 terms, whose size (not the largest result) sets the round-off.  Bound:
            # k * 2^-24 * (|initial| + sum |terms|), k as counted in bil_w_roundings; dw and dbias are fp32 whatever the
            # activation type (the bf16 inputs are widened exactly), so there is no output rounding to add.
            errs[key + "_over_bound"] = gate_bound(got, init + r, k * U32 * (init.abs() + absr), "bilinear bwd " + key)
    return errs


def check_bilinear_rejects(lib, put):
    """I = 48, J = 4 passes vinet_bilinear_fwd's limits (I <= 48, J <= 4) but not vinet_bilinear_bwd's: its weight-gradient kernel
    keeps 16 x (I*J + 1) accumulators in 8 x 256 lanes, so I*J <= 127.  The asymmetry is the entry points' contract today (a
    model with such a fusion could run forward and not train): the refusal must be clean -- negative, explained, nothing written."""
    B, Cc, I, J, O = BIL_FWD_ONLY
    t = bil_inputs(BIL_FWD_ONLY, F32)
    x1, x2, do, w, dw = put(t["x1"]), put(t["x2"]), put(t["dout"]), put(t["w"]), put(t["dw0"])
    d1, d2 = put(torch.zeros(B * I * Cc)), put(torch.zeros(B * J * Cc))
    rc = lib.vinet_bilinear_bwd(x1.data_ptr(), x2.data_ptr(), do.data_ptr(), F32, w.data_ptr(), B, Cc, I, J, O, d1.data_ptr(), d2.data_ptr(),
                                dw.data_ptr(), None, 0)
    assert rc < 0 and b"I*J too large" in lib.vinet_last_error()
    assert torch.equal(dw.cpu(), t["dw0"]) and not bool(d1.cpu().any()) and not bool(d2.cpu().any())


# =====================================================================================================================
# 2x upsample: vinet_upsample2x / _bwd / _bwd_relu
# =====================================================================================================================
UP_CASES = [
    ("h1_w1", (1, 1, 1, 1, 8)),          # both clamps at once: every output is the one input
    ("h1", (2, 2, 1, 5, 8)),
    ("w1", (2, 2, 4, 1, 16)),
    ("quad_c4", (1, 3, 2, 2, 4)),        # C % 8 != 0: the 4-channel kernels even with up_blk = 1
    ("quad_c12", (2, 1, 3, 5, 12)),
    ("general_c40", (2, 3, 5, 7, 40)),
]
UP_FWD_TOL = {F32: 1e-6, BF16: 1e-2}
UP_BWD_TOL = {F32: 1e-5, BF16: 2e-2}


def _up_slabs(dims, dt):
    B, T, H, W, Cc = dims
    x = Slab(dims, dt, "tail_up_x", 1, ld=Cc + 16, c_off=8)
    ydims = (B, T, 2 * H, 2 * W, Cc)
    ygeo = dict(ld=Cc + 8, c_off=8, t_total=T + 2, t_off=1)
    return x, ydims, ygeo


def _interp(x):
    """[B,T,H,W,C] float64 -> [B,T,2H,2W,C]"""
    y = torch.nn.functional.interpolate(x.permute(0, 4, 1, 2, 3), scale_factor=(1, 2, 2), mode="trilinear", align_corners=False)
    return y.permute(0, 2, 3, 4, 1)


def _interp_t(dims, dy):
    """the transpose of _interp applied to dy, by autograd"""
    x = torch.zeros(dims, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        (_interp(x) * dy).sum().backward()
    return x.grad


def check_upsample_fwd(side, dims, dt):
    """from a channel slice into a T- and channel-sliced y whose other bytes keep their fill value"""
    x, ydims, ygeo = _up_slabs(dims, dt)
    y = Slab(ydims, dt, fill=7.0, **ygeo)
    xb, yb = side.put(x.base), side.put(y.base)
    side.call("vinet_upsample2x", x.ct(xb), y.ct(yb), dt)
    y.assert_outside_untouched(yb, "upsample fwd")
    return dict(y=gate(y.inner(yb.cpu()), _interp(x.wide()), UP_FWD_TOL[dt], "upsample fwd"))


def check_upsample_bwd(side, dims, dt, accumulate):
    _, ydims, ygeo = _up_slabs(dims, dt)
    dy = Slab(ydims, dt, "tail_up_dy", 2, **ygeo)
    dx = Slab(dims, dt, "tail_up_dx", 3, ld=dims[4] + 8, c_off=8)        # (16-byte aligned in both types: the 8-channel kernels stay eligible)
    dyb, dxb = side.put(dy.base), side.put(dx.base)
    side.call("vinet_upsample2x_bwd", dy.ct(dyb), dx.ct(dxb), dt, accumulate)
    dx.assert_outside_untouched(dxb, "upsample bwd")
    ref = _interp_t(dims, dy.wide()) + (dx.wide() if accumulate else 0.0)
    return dict(dx=gate(dx.inner(dxb.cpu()), ref, UP_BWD_TOL[dt], "upsample bwd, accumulate %d" % accumulate))


def up_relu_xf(dims, dt):
    """the ReLU's output in front of the upsample: exact zeros, negative values (the gate is xf > 0, whatever produced xf)"""
    xf = synth.normal("tail_up_xf", dims, 4)
    xf.view(-1)[::3] = 0.0
    xf.view(-1)[1::7] = -0.0
    return xf


def check_upsample_bwd_relu(side, dims, dt):
    _, ydims, ygeo = _up_slabs(dims, dt)
    dy = Slab(ydims, dt, "tail_up_dy", 2, **ygeo)
    dx = Slab(dims, dt, "tail_up_dx", 3, ld=dims[4] + 8, c_off=8)        # (16-byte aligned in both types: the 8-channel kernels stay eligible)
    xf = Slab(dims, dt, fill=0.0, ld=dims[4] + 16, c_off=8, values=up_relu_xf(dims, dt))
    dyb, dxb, xfb = side.put(dy.base), side.put(dx.base), side.put(xf.base)
    side.call("vinet_upsample2x_bwd_relu", dy.ct(dyb), dx.ct(dxb), xf.ct(xfb), dt)
    dx.assert_outside_untouched(dxb, "upsample bwd + ReLU gate")
    open_ = xf.wide() > 0
    assert bool(open_.any()) and bool((xf.wide() == 0).any()) and bool((xf.wide() < 0).any())
    got = dx.inner(dxb.cpu())
    assert bool((got[~open_] == 0).all()), "gradient behind a closed gate"
    return dict(dx=gate(got, _interp_t(dims, dy.wide()) * open_, UP_BWD_TOL[dt], "upsample bwd + ReLU gate"))


# =====================================================================================================================
# vinet_act_bwd
# =====================================================================================================================
ACT_DIMS = (2, 2, 3, 5, 12)
ACT_COMBOS = [(F32, F32, F32), (BF16, BF16, BF16), (F32, F32, BF16), (F32, BF16, BF16), (BF16, F32, BF16)]      # (dz, z, dy)
ACT_BAD_COMBO = (BF16, BF16, F32)
ACT_LAYOUTS = {          # per tensor (dz, z, dy): Slab geometry
    "dense": [dict(), dict(), dict()],
    "chan_slices": [dict(ld=24, c_off=4), dict(ld=24, c_off=8), dict(ld=24, c_off=12)],
    "t_slice": [dict(t_total=3, t_off=1), dict(t_total=4, t_off=2), dict(t_total=3, t_off=0)],       # sB != T*H*W*ld: linear == 0
}
ACT_TOL = {F32: 1e-6, BF16: 1e-2}
TINY = 2.0 ** -126       # the smallest positive normal of fp32 and of bf16


def act_z(act):
    """ReLU: N(0,1); sigmoid: outputs in (0, 1).  Both with +0, -0 and the smallest positive normal spread over several quads."""
    z = synth.normal("tail_act_z", ACT_DIMS, 1) if act == 1 else synth.uniform("tail_act_z", ACT_DIMS, 1, 0.02, 0.98)
    f = z.view(-1)
    for at, val in ((0, 0.0), (1, -0.0), (2, TINY), (17, 0.0), (30, -0.0), (43, TINY), (716, 0.0), (718, TINY), (719, -0.0)):
        f[at] = val
    return z


def check_act_bwd(side, combo, act, layout):
    gdt, zdt, ydt = combo
    geo = ACT_LAYOUTS[layout]
    dz = Slab(ACT_DIMS, gdt, "tail_act_dz", 2, **geo[0])
    z = Slab(ACT_DIMS, zdt, fill=0.5, values=act_z(act), **geo[1])
    dy = Slab(ACT_DIMS, ydt, "tail_act_dy", 3, **geo[2])
    zb, gb, yb = side.put(z.base), side.put(dz.base), side.put(dy.base)
    side.call("vinet_act_bwd", dz.ct(gb), gdt, z.ct(zb), zdt, act, dy.ct(yb), ydt)
    dy.assert_outside_untouched(yb, "act_bwd")
    zw, gw = z.wide(), dz.wide()
    assert int((zw == 0).sum()) == 6 and int((zw == TINY).sum()) == 3
    ref = gw * (zw > 0) if act == 1 else gw * zw * (1 - zw)
    got = dy.inner(yb.cpu())
    if act == 1:         # the gate is z > 0: closed at +0 and -0, open at the smallest normal (where the gradient passes unchanged)
        assert bool((got[zw == 0] == 0).all()) and bool((got.double()[zw == TINY] == dz.wide().to(TDT[ydt]).double()[zw == TINY]).all())
    return dict(dy=gate(got, ref, ACT_TOL[ydt], "act_bwd"))


# =====================================================================================================================
# vinet_unfold1d
# =====================================================================================================================
# (B, L, Cpad, k, stride, pad): a window of exactly 8 at stride 1 without padding (one output row; two rows and 8 channels);
# stride 3 with pad 5; SoundNet's conv1
UNFOLD_CASES = [(1, 8, 1, 8, 1, 0), (2, 9, 8, 8, 1, 0), (3, 40, 4, 16, 3, 5), (2, 501, 8, 64, 2, 32)]


def check_unfold1d(side, case, dt):
    """y[b, m, c] = x[b, stride*m - pad + c, channel 0], zero outside: a copy, so bit-exact.  x is a channel slice (channel 0 is
    read at stride ld > C), y a channel slice of a wider buffer whose other bytes stay."""
    B, Ln, Cpad, k, stride, pad = case
    Lo = (Ln + 2 * pad - k) // stride + 1
    x = Slab((B, Ln, 1, 1, Cpad), dt, "tail_unf_x", 1, ld=Cpad + 4, c_off=2)
    y = Slab((B, Lo, 1, 1, k), dt, "tail_unf_y", 2, ld=k + 8, c_off=8)
    xb, yb = side.put(x.base), side.put(y.base)
    side.call("vinet_unfold1d", x.ct(xb), y.ct(yb), dt, stride, pad)
    y.assert_outside_untouched(yb, "unfold1d")
    pos = torch.arange(Lo).view(Lo, 1) * stride - pad + torch.arange(k).view(1, k)          # the index table
    ok = (pos >= 0) & (pos < Ln)
    x0 = x.inner(x.base)[:, :, 0, 0, 0]                                                     # [B, L], storage type
    ref = torch.where(ok.unsqueeze(0), x0[:, pos.clamp(0, Ln - 1)], torch.zeros((), dtype=TDT[dt]))
    assert bool(ok.any()) and (pad == 0 or not bool(ok.all()))
    got = y.inner(yb.cpu())[:, :, 0, 0, :]
    assert torch.equal(got.view(BITS[dt]), ref.view(BITS[dt])), "unfold1d: %d elements differ" % int((got != ref).sum())
    return {}


# =====================================================================================================================
# refusals (argument checks: they return before any launch)
# =====================================================================================================================
def check_other_rejects(lib, put):
    """vinet_adam_step refuses a pointer off the 16-byte grid, vinet_loss_bwd refuses NSS (forward only), vinet_act_bwd a sixth
    dtype combination"""
    bufs = [put(torch.zeros(12)) for _ in range(4)]
    for bad in range(4):
        ptrs = [b.data_ptr() + (4 if k == bad else 0) for k, b in enumerate(bufs)]
        assert lib.vinet_adam_step(*ptrs, 4, 1e-4, 0.9, 0.999, 1e-8, 0.1, 0.001, 1.0, 0) < 0
        assert b"16-byte" in lib.vinet_last_error()
    assert not any(bool(b.cpu().any()) for b in bufs)
    s, g = loss_inputs(3, 0, 3, 65)
    sd, gd, saved, ds = put(s), put(g), put(torch.zeros(24, dtype=torch.float64)), put(torch.zeros(3, 65))
    assert lib.vinet_loss_bwd(3, sd.data_ptr(), gd.data_ptr(), 0, 3, 65, saved.data_ptr(), None, 1.0, 0, ds.data_ptr(), 0) < 0
    assert not bool(ds.cpu().any())
    gdt, zdt, ydt = ACT_BAD_COMBO
    dz, z, dy = Slab(ACT_DIMS, gdt, "tail_act_dz", 2), Slab(ACT_DIMS, zdt, "tail_act_z", 1), Slab(ACT_DIMS, ydt, fill=3.0)
    gb, zb, yb = put(dz.base), put(z.base), put(dy.base)
    assert lib.vinet_act_bwd(dz.ct(gb), gdt, z.ct(zb), zdt, 1, dy.ct(yb), ydt, 0) < 0
    assert b"unsupported dtype combination" in lib.vinet_last_error()
    assert bool((yb.cpu() == 3.0).all())
