"""The fused decoder tail (csrc/decoder_tail.hip: vinet_decoder_tail_ok / _fwd / _bwd): the case table, buffers with sentinel
guards, a float64 reference for integer data, and the COMPOSITION the pair replaces, run through the engine's own functions on the
same buffers -- conv_forward x2 + vinet_export_ncdhw forward; vinet_import_ncdhw, vinet_act_bwd x2 and the two data gradients
(engine._data_grad) backward.  Used by tests/test_gpu_decoder_tail.py (the library on a GPU), tests/test_decoder_tail_host.py (the
table's claims, the reference against itself, the library's refusals on host memory) and tests/headline_decoder_tail.py."""
import collections
import ctypes as C

import torch

from vinet_amd import _lib as L
from vinet_amd import engine as E

BF16, F32 = L.BF16, L.F32
EXACT = 1 << 24
BF_FILL = 0x7FC1            # bf16 bits of a NaN with a payload: nothing the kernels compute
F_FILL = -0.28125           # no sigmoid value, no integer

Case = collections.namedtuple("Case", "id B H W kT mid_bias a6 uform planes")
#   a6      False: the forward gets a6 = NULL (inference); such a case has no backward
#   uform   "dense" | "tslice": u (and du) are frames [1, 1 + kT) of a buffer of kT + 2 frames whose clip stride exceeds its extent;
#           dz6 then has row stride 40 and dy_head row stride 16
#   planes  "dense" | "strided": out and g with pixel stride 2, row stride 2 W + 3 and a plane stride beyond the extent


def _cases():
    out = []
    # pixel counts that are no multiple of 16 (1 x 3 x 5: under one group), of 64 (one workgroup's share at these sizes) or of
    # the grid; every kT; bias on / off; a6 NULL; sliced u; strided planes
    small = [(1, 3, 5), (2, 9, 29), (3, 17, 23)]
    k = 0
    for kT in (2, 3, 4):
        for B, H, W in small:
            for mid_bias in (False, True):
                uform = ("dense", "tslice")[k % 2]
                planes = ("dense", "strided")[(k // 2) % 2]
                a6 = k % 5 != 3
                out.append(Case("k%d_B%dH%dW%d_%s_%s_%s_%s" % (kT, B, H, W, "bias" if mid_bias else "nobias", uform, planes,
                                                                "a6" if a6 else "null"), B, H, W, kT, mid_bias, a6, uform, planes))
                k += 1
    # a wave walks more than one group from 2 x 8192 groups on (tail_shape): 513 x 513 pixels = 16449 groups, an odd count, so the
    # last wave stops after its first group, and the last group holds one pixel
    out.append(Case("k2_B1H513W513_nobias_dense_dense_a6_walk", 1, 513, 513, 2, False, True, "dense", "dense"))
    return out


CASES = _cases()


def groups_per_wave(M):
    """tail_shape of csrc/decoder_tail.hip"""
    groups = (M + 15) // 16
    return max(1, min(32, groups // (4 * 256 * 8)))


# ---- buffers --------------------------------------------------------------------------------------------------------------
class Guarded:
    """a View inside a larger sentinel-filled buffer"""

    def __init__(self, dev, dt, B, T, H, W, Cc, ld=None, frames=None, t0=0, slack=0):
        ld = Cc if ld is None else ld
        frames = T if frames is None else frames
        sB = frames * H * W * ld + slack
        lead = 64
        n = lead + B * sB + 64
        tdt = E.TORCH_DT[dt]
        self.buf = torch.empty(n, dtype=tdt, device=dev)
        self.fill()
        self.v = E.View(self.buf, lead + t0 * H * W * ld, B, T, H, W, Cc, ld, sB, dt)

    def fill(self):
        if self.buf.dtype == torch.bfloat16:
            self.buf.view(torch.int16).fill_(BF_FILL)
        else:
            self.buf.fill_(F_FILL)

    def bits(self):
        return self.buf.view(torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32)

    def t5(self):
        return self.v.torch5()

    def outside_untouched(self):
        """True if nothing but the view changed since fill(); the view's contents are lost"""
        if self.buf.dtype == torch.bfloat16:
            self.t5().view(torch.int16).fill_(BF_FILL)
            return bool((self.buf.view(torch.int16) == BF_FILL).all())
        self.t5().fill_(F_FILL)
        return bool((self.buf == F_FILL).all())


class Plane:
    """[B, H, W] fp32 inside a sentinel-filled buffer, dense or strided"""

    def __init__(self, dev, B, H, W, form):
        if form == "dense":
            self.sw, self.sh, self.sb = 1, W, H * W
        else:
            self.sw, self.sh = 2, 2 * W + 3
            self.sb = H * self.sh + 5
        self.buf = torch.full((16 + B * self.sb + 16,), F_FILL, dtype=torch.float32, device=dev)
        self.t = torch.as_strided(self.buf, (B, H, W), (self.sb, self.sh, self.sw), 16)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def outside_untouched(self):
        self.t.fill_(F_FILL)
        return bool((self.buf == F_FILL).all())


class Problem:
    """weights, plans and buffers of one case on `dev`"""

    def __init__(self, case, dev, seed, exact):
        self.case, self.dev, self.exact = case, dev, exact
        g = self.gen = torch.Generator(device=dev)
        g.manual_seed(seed)
        c = case
        kT = c.kT

        def rnd(shape, std, lo=-2, hi=2):
            t = torch.empty(shape, dtype=torch.float32, device=dev)
            return t.random_(lo, hi + 1, generator=g) if exact else t.normal_(0.0, std, generator=g)
        self.w_mid = rnd((32, 32, kT, 1, 1), 0.12)
        self.b_mid = rnd((32,), 0.1, -1, 1) if c.mid_bias else None
        self.w_head = rnd((1, 32, 1, 1, 1), 0.15)
        self.b_head = rnd((1,), 0.1, -1, 1)
        self.mid = E.ConvPlan(self.w_mid, self.b_mid, (kT, 1, 1), (kT, 1, 1), (0, 0, 0))
        self.head = E.ConvPlan(self.w_head, self.b_head, (1, 1, 1), (1, 1, 1), (0, 0, 0))
        sl = c.uform == "tslice"
        uk = dict(frames=kT + 2, t0=1, slack=72) if sl else {}
        self.u = Guarded(dev, BF16, c.B, kT, c.H, c.W, 32, **uk)
        self.du = Guarded(dev, BF16, c.B, kT, c.H, c.W, 32, **uk)
        self.a6 = Guarded(dev, BF16, c.B, 1, c.H, c.W, 32)
        self.dz = Guarded(dev, BF16, c.B, 1, c.H, c.W, 32, ld=40 if sl else 32)
        self.dy = Guarded(dev, BF16, c.B, 1, c.H, c.W, 8, ld=16 if sl else 8)
        self.out = Plane(dev, c.B, c.H, c.W, c.planes)
        self.g = Plane(dev, c.B, c.H, c.W, c.planes)
        uv = self.u.t5()
        if exact:
            uv.copy_(torch.empty(uv.shape, dtype=torch.float32, device=dev).random_(-2, 3, generator=g))
        else:
            uv.copy_(torch.empty(uv.shape, dtype=torch.float32, device=dev).normal_(0.0, 1.0, generator=g))

    # -- the packs, as the engine makes them ------------------------------------------------------------------------------
    def ctx(self):
        return E.Ctx(self.dev, BF16, training=False, record=False)

    def packs(self, ctx):
        """(mid forward, mid transposed, head forward) packs as the engine makes them; ctx None (host memory, nothing is launched):
        zero-filled buffers of their sizes"""
        if ctx is None:
            return tuple(torch.zeros(n, dtype=torch.bfloat16) for n in (self.case.kT * 1024, self.case.kT * 1024, 32))
        return self.mid.packed(ctx, False), self.mid.packed(ctx, True), self.head.packed(ctx, False)

    def fwd_args(self, ctx, a6=True):
        """the arguments of vinet_decoder_tail_ok (+ strides and stream: vinet_decoder_tail_fwd)"""
        pk = self.packs(ctx)
        self._keep = (pk[0], pk[2])
        a6p = C.byref(self.a6.v.ct()) if a6 else None
        return [BF16, C.byref(self.u.v.ct()), self.case.kT, self._keep[0].data_ptr(), E._ptr(self.b_mid), self._keep[1].data_ptr(),
                self.b_head.data_ptr(), a6p, self.out.ptr]

    def run_fwd(self, ctx):
        a = self.fwd_args(ctx, self.case.a6)
        lib = ctx.lib
        assert lib.vinet_decoder_tail_ok(*a) == 1, lib.vinet_last_error()
        rc = lib.vinet_decoder_tail_fwd(*a, self.out.sb, self.out.sh, self.out.sw, ctx.stream)
        assert rc == 0, lib.vinet_last_error()

    def bwd_args(self, ctx, accumulate=0):
        o, g = self.out, self.g
        pk = self.packs(ctx)
        self._keep_b = (pk[1], pk[2])
        return [BF16, g.ptr, g.sb, g.sh, g.sw, o.ptr, o.sb, o.sh, o.sw, C.byref(self.a6.v.ct()), self.case.kT, self._keep_b[0].data_ptr(),
                self._keep_b[1].data_ptr(), C.byref(self.dy.v.ct()), C.byref(self.dz.v.ct()), C.byref(self.du.v.ct()), accumulate,
                ctx.stream if ctx is not None else 0]

    def run_bwd(self, ctx):
        rc = ctx.lib.vinet_decoder_tail_bwd(*self.bwd_args(ctx))
        assert rc == 0, ctx.lib.vinet_last_error()

    # -- today's launches on the same inputs ------------------------------------------------------------------------------
    def composed_fwd(self, ctx):
        """-> (a6 View, padded fp32 head View, planes [8, B, H, W])"""
        c = self.case
        a6 = E.conv_forward(ctx, self.mid, E.Act(self.u.v), act=L.ACT_RELU)
        head = E.conv_forward(ctx, self.head, a6, act=L.ACT_SIGMOID, out_dt=F32, n_pad=8)
        hv = head.v
        planes = torch.empty((hv.C, hv.B, hv.H, hv.W), dtype=torch.float32, device=self.dev)
        ctx.call("vinet_export_ncdhw", C.byref(hv.ct()), hv.dt, L.CAffine(None, None, 0), planes.data_ptr(), hv.H * hv.W,
                 hv.B * hv.H * hv.W, 0, hv.W, 1, 0, ctx.stream)
        assert (hv.B, hv.T, hv.H, hv.W) == (c.B, 1, c.H, c.W)
        return a6.v, hv, planes

    def composed_bwd(self, ctx, a6v, headv):
        """import, sigmoid', the head's data gradient, ReLU', the per-tap data gradients -> (dy_head, dz6, du) Views (dense)"""
        c, dev = self.case, self.dev
        g = self.g
        M = c.B * c.H * c.W
        gv = E.View.alloc(c.B, 1, c.H, c.W, 8, F32, dev)
        ctx.call("vinet_import_ncdhw", g.ptr, g.sb, 0, 0, g.sh, g.sw, 1, C.byref(gv.ct()), gv.dt, ctx.stream)
        dy = E.View.alloc(c.B, 1, c.H, c.W, 8, BF16, dev)
        ctx.call("vinet_act_bwd", C.byref(gv.ct()), gv.dt, C.byref(headv.ct()), headv.dt, L.ACT_SIGMOID, C.byref(dy.ct()), dy.dt, ctx.stream)
        a6 = E.Act(a6v, needs_grad=True)
        E._data_grad(ctx, self.head, a6, headv, dy, M)
        dz = a6.grad_view()
        ctx.call("vinet_act_bwd", C.byref(dz.ct()), dz.dt, C.byref(a6v.ct()), a6v.dt, L.ACT_RELU, C.byref(dz.ct()), dz.dt, ctx.stream)
        u = E.Act(self.u.v, needs_grad=True)
        E._data_grad(ctx, self.mid, u, a6v, dz, M)
        return dy, dz, u.grad_view()


# ---- float64 reference (integer data: every sum exact) ------------------------------------------------------------------------
def bf(v64):
    return v64.to(torch.float32).to(torch.bfloat16)


def ref_fwd(p, drop_tap=False):
    """-> (a6 bf16 [B,1,H,W,32], pre-sigmoid head float64 [B,H,W], largest sum of |terms|)"""
    u = p.u.t5().double()                                   # [B, kT, H, W, 32]
    w = bf(p.w_mid.double()).double()[:, :, :, 0, 0]         # [n, c, t]
    kT = p.case.kT - (1 if drop_tap else 0)
    z = sum(u[:, t] @ w[:, :, t].T for t in range(kT))
    mag = sum(u[:, t].abs() @ w[:, :, t].abs().T for t in range(kT))
    if p.b_mid is not None:
        z = z + p.b_mid.double()
        mag = mag + p.b_mid.double().abs()
    a6 = bf(z.clamp_min(0))
    wh = bf(p.w_head.double()).double()[0, :, 0, 0, 0]
    v = a6.double() @ wh + p.b_head.double()
    mag2 = a6.double().abs() @ wh.abs() + p.b_head.double().abs()
    return a6.unsqueeze(1), v, max(float(mag.max()), float(mag2.max()))


def ref_bwd(p, drop_tap=False):
    """from the buffers' a6, out and g -> (dy_head [B,1,H,W,8], dz6, du) bf16, largest sum of |terms|"""
    g, s = p.g.t.double(), p.out.t.double()
    a6 = p.a6.t5().double()[:, 0]
    dy1 = bf(g * (s * (1 - s)))
    dy = torch.zeros(dy1.shape + (8,), dtype=torch.bfloat16, device=dy1.device)
    dy[..., 0] = dy1
    wh = bf(p.w_head.double()).double()[0, :, 0, 0, 0]
    da = bf(dy1.double().unsqueeze(-1) * wh + 0.0)          # (a sum of K terms from +0: a lone product of -0 leaves +0)
    dz = torch.where(a6 > 0, da, torch.zeros_like(da))
    w = bf(p.w_mid.double()).double()[:, :, :, 0, 0]
    kT = p.case.kT
    du = torch.stack([bf(dz.double() @ w[:, :, t]) for t in range(kT)], 1)
    if drop_tap:
        du[:, kT - 1] = 0
    mag = max(float((dz.double().abs() @ w[:, :, t].abs()).max()) for t in range(kT))
    return dy.unsqueeze(1), dz.unsqueeze(1), du, mag


def shifted(t):
    """the same values one pixel later (over the flattened [B, ..., H, W] pixel order of a [B, T, H, W, C] tensor's frames)"""
    B, T, H, W, Cc = t.shape
    return t.permute(1, 0, 2, 3, 4).reshape(T, B * H * W, Cc).roll(1, 1).reshape(T, B, H, W, Cc).permute(1, 0, 2, 3, 4)


def last16_dropped(t):
    B, T, H, W, Cc = t.shape
    r = t.permute(1, 0, 2, 3, 4).reshape(T, B * H * W, Cc).clone()
    r[:, -16:] = 0
    return r.reshape(T, B, H, W, Cc).permute(1, 0, 2, 3, 4)


def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def sigmoid_gate(got, v64):
    """the gate tests/headline_step.py applies to the sigmoid head against a float64 sigmoid: |got - ref| <= 2^-8 |ref| + 2^-20"""
    ref = torch.sigmoid(v64)
    return bool(((got.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -20).all())


# ---- refusals: argument lists the entry points must turn down before any launch ---------------------------------------------
def refusals(p, ctx):
    """[(what, entry point name, args)] on Problem p; ctx None: p lives in host memory (nothing is launched either way)"""
    out = []

    def fwd(what, edit):
        a = p.fwd_args(ctx, True)
        edit(a)
        out.append((what, "vinet_decoder_tail_fwd", a + [p.out.sb, p.out.sh, p.out.sw, ctx.stream if ctx is not None else 0]))
        out.append((what, "vinet_decoder_tail_ok", a))

    def bwd(what, edit, accumulate=0):
        a = p.bwd_args(ctx, accumulate)
        edit(a)
        out.append((what, "vinet_decoder_tail_bwd", a))

    def ct(v, **kw):
        c = v.ct()
        for k, x in kw.items():
            setattr(c, k, x)
        return C.byref(c)
    uv, av = p.u.v, p.a6.v
    fwd("fp32", lambda a: a.__setitem__(0, F32))
    fwd("u with 24 channels", lambda a: a.__setitem__(1, ct(uv, C=24)))
    fwd("u with 64 channels", lambda a: a.__setitem__(1, ct(uv, C=64, ld=64)))
    fwd("a6 with 16 channels", lambda a: a.__setitem__(7, ct(av, C=16)))
    fwd("u two bytes off the 16-byte grid", lambda a: a.__setitem__(1, ct(uv, ptr=uv.ptr() + 2)))
    fwd("a6 eight bytes off the 16-byte grid", lambda a: a.__setitem__(7, ct(av, ptr=av.ptr() + 8)))
    fwd("u row stride 36", lambda a: a.__setitem__(1, ct(uv, ld=36)))
    fwd("map one byte off", lambda a: a.__setitem__(8, p.out.ptr + 1))
    fwd("weight pack off the 16-byte grid", lambda a: a.__setitem__(3, a[3] + 2))
    fwd("kT = 5", lambda a: a.__setitem__(2, 5))
    fwd("kT = 1", lambda a: a.__setitem__(2, 1))
    fwd("u.T != kT", lambda a: a.__setitem__(1, ct(uv, T=uv.T + 1)))
    fwd("no head bias", lambda a: a.__setitem__(6, None))
    fwd("a6 of another extent", lambda a: a.__setitem__(7, ct(av, W=av.W + 1)))
    bwd("accumulate", lambda a: None, accumulate=1)
    bwd("fp32", lambda a: a.__setitem__(0, F32))
    bwd("dy_head with 32 channels", lambda a: a.__setitem__(13, ct(p.dz.v)))
    bwd("dz6 with 8 channels", lambda a: a.__setitem__(14, ct(p.dy.v)))
    bwd("du off the 16-byte grid", lambda a: a.__setitem__(15, ct(p.du.v, ptr=p.du.v.ptr() + 4)))
    bwd("kT = 5", lambda a: a.__setitem__(10, 5))
    bwd("no a6", lambda a: a.__setitem__(9, None))
    bwd("gradient one byte off", lambda a: a.__setitem__(1, p.g.ptr + 1))
    return out
