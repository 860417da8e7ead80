"""vinet_maxpool3d_keep (csrc/pool.hip: the max-pool forward that also stores pre(x) to a second view): the case table, an
independent float64 / numpy reference, a CPU model of the kernel, and the runner that the host test (tests/test_pool_keep_host.py,
the model) and the GPU test (tests/test_gpu_pool_keep_kernels.py, libvinet_hip.so) share.

Nothing here takes a tolerance.  The reference scans each window's taps in (t, h, w) order over float64 values and takes a tap when it
is strictly greater: the first maximum wins.  Its `keep` is bf16(relu(fma(x, scale, shift))): the product and the sum are formed in
float64, where they are EXACT for this data (x has 8 significant bits, scale and shift 24, and all exponents lie within 40 bits of
each other), rounded once to fp32 -- that is what a fused multiply-add returns -- and once more to bf16, ties to even.  It shares no
code with the kernels, with tests/abi_emulator.py or with the model below.

Data: x is a multiple of 1/4 in [-4, 4] (many ties, both signs, zeros).  The `exact` affines (scales of +-{0.5, 1, 2}, shifts that
are multiples of 1/4) give multiples of 1/8 below 16 that bf16 holds exactly; the `general` affine (scales like 1.1, -0.7; shifts
like 0.05) gives values that every rounding step changes.  Inputs are NaN-free, no shift is -0 and no window lies wholly outside its
image, so pooled values and argmax have one right answer.  A -0 can still reach `keep`: vinet_copy_affine takes fmaxf before
rounding, the pool takes an integer max after it, so a tiny negative number behind a ReLU is +0 in one and may be -0 in the other.
The runner counts such elements (Report.zero_sign) and allows no other difference.

Views: x dense or a channel slice (ld = C + 8); `keep` a T slice (frames 2 .. 2 + T of T + 3, so sB exceeds its own extent), the same
in a channel slice, or dense; y dense or a channel slice; argmax null, or between two guards.  Every buffer carries 16 elements of
sentinel in front and behind, and everything outside a view -- its gaps included -- must keep its bits."""
import ctypes as C

import numpy as np
import torch

from vinet_amd import _lib as L
from vinet_amd import engine as E

F32, BF16 = E.F32, E.BF16
P0 = ((1, 3, 3), (1, 2, 2), (0, 1, 1))
P1 = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
T2 = ((2, 1, 1), (2, 1, 1), (0, 0, 0))
K3 = ((3, 3, 3), (1, 1, 1), (1, 1, 1))
S2 = ((1, 2, 2), (1, 2, 2), (0, 0, 0))
SERVED = (P0, P1, T2)
POOL_NAMES = {P0: "k133s2", P1: "k333s2", T2: "k211s2", K3: "k333s1", S2: "k122s2"}
PRE_FORMS = ["none", "affine_relu", "affine", "relu", "neg_scales", "general"]
X_FORMS = ["dense", "chan"]
KEEP_FORMS = ["tslice", "tslice_chan", "dense"]
Y_FORMS = ["dense", "chan"]
PAD = 16                    # sentinel elements in front of and behind every buffer (32 bytes: 16-byte alignment survives)
KEEP_FILL = 0x7FC1          # a quiet NaN with a payload: no case produces it (the inputs are NaN-free)
Y_FILL = 0x7FC3
AM_FILL = 0xA5
X_OUTSIDE = 3e38            # around x: wins every comparison it is wrongly part of
POOL_FILL_COLS = 65536      # csrc/pool.hip: from this many 8-channel columns on, 3x3x3/s1 leaves maxpool_fwd8_pk_kernel


def out_dims(pool, thw):
    k, s, p = pool
    return tuple((d + 2 * pp - kk) // ss + 1 for d, kk, ss, pp in zip(thw, k, s, p))


class Geo:
    """a channels-last [B,T,H,W,C] view inside a flat buffer of `n` elements"""

    def __init__(self, dims, form):
        B, T, H, W, Cc = dims
        chan, tsl = "chan" in form, "tslice" in form
        self.dims, self.form = dims, form
        self.ld = Cc + 8 if chan else Cc
        self.sB = (T + 3 if tsl else T) * H * W * self.ld
        self.off = PAD + (2 * H * W * self.ld if tsl else 0) + (8 if chan else 0)
        self.n = PAD + B * self.sB + PAD

    def strided(self, buf):
        B, T, H, W, Cc = self.dims
        return np.lib.stride_tricks.as_strided(buf[self.off:], (B, T, H, W, Cc), tuple(
            buf.itemsize * s for s in (self.sB, H * W * self.ld, W * self.ld, self.ld, 1)))

    def mask(self):
        m = np.zeros(self.n, dtype=bool)
        self.strided(m)[...] = True
        return m

    def ct(self, t):
        B, T, H, W, Cc = self.dims
        return L.CTensor(t.data_ptr() + self.off * t.element_size(), B, T, H, W, Cc, self.ld, self.sB)


class Case:
    def __init__(self, pool, dims, pre, xf, kf, yf, am, dt=BF16, serve=True, why=""):
        self.pool, self.dims, self.pre, self.xf, self.kf, self.yf, self.am, self.dt, self.serve, self.why = pool, dims, pre, xf, kf, yf, am, dt, serve, why
        self.odims = (dims[0],) + out_dims(pool, dims[1:4]) + (dims[4],)
        self.id = "%s_%s_B%dT%dH%dW%dC%d_%s_x%s_k%s_y%s_%s" % (("ok" if serve else "no_" + why, POOL_NAMES[pool]) + tuple(dims) + (
            pre, xf, kf, yf, "am" if am else "null"))

    def __repr__(self):
        return self.id


def _served_cases():
    out = []
    for pool in SERVED:
        j = 0
        for T in (1, 2, 4):
            if pool == T2 and T % 2:
                continue                # (T = 1 has no output frame; odd T is a refusal, below)
            for H in (1, 2, 3, 4, 5):
                for W in (1, 2, 3, 4, 5):
                    dims = (1 + (j // 5) % 2, T, H, W, (8, 24, 40)[(j // 2) % 3])
                    out.append(Case(pool, dims, PRE_FORMS[j % 6], X_FORMS[(j // 6) % 2], KEEP_FORMS[(j // 6) % 3],
                                    Y_FORMS[(j // 2 + j // 12) % 2], (j // 6 + j) % 2 == 1))
                    j += 1
        # more than one workgroup of 256 lanes, partial blocks at every border
        out.append(Case(pool, (2, 4, 9, 10, 40), "affine_relu", "chan", "tslice_chan", "chan", True))
    return out


SERVED_CASES = _served_cases()
REFUSED_CASES = [
    # 3x3x3/s1 at 65536 columns of 8 channels: the LDS kernel, which has no keeping form
    Case(K3, (1, 2, 128, 128, 32), "affine_relu", "dense", "tslice", "dense", True, serve=False, why="lds"),
    Case(T2, (2, 3, 2, 3, 8), "affine_relu", "dense", "tslice", "dense", True, serve=False, why="oddT"),        # frame 2 has no owner
    Case(S2, (1, 2, 3, 4, 8), "relu", "dense", "tslice", "dense", True, serve=False, why="oddH"),               # row 2 has no owner
    Case(P0, (2, 2, 3, 4, 8), "affine_relu", "dense", "tslice", "dense", True, dt=F32, serve=False, why="fp32"),
    Case(P1, (1, 2, 3, 3, 12), "none", "dense", "tslice", "dense", False, serve=False, why="quad"),              # C = 12: the 4-channel kernel
]
CASES = SERVED_CASES + REFUSED_CASES


# ---- bf16 on the host ---------------------------------------------------------------------------------------------------------
def bf16_bits(f32):
    """fp32 array -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def inputs(case):
    """(x values float64 [B,T,H,W,C], scale fp32 [C] or None, shift fp32 [C] or None, relu)"""
    rng = np.random.RandomState(sum(map(ord, case.id)))
    Cc = case.dims[4]
    x = rng.randint(-16, 17, size=case.dims).astype(np.float64) / 4
    c = np.arange(Cc)
    if case.pre in ("none", "relu"):
        return x, None, None, case.pre == "relu"
    if case.pre == "general":
        sc = np.array([1.1, -0.7, 0.3, 1.9, -1.3, 0.9], dtype=np.float32)[c % 6]
        sh = np.array([0.05, -0.3, 0.7, -0.011, 0.2], dtype=np.float32)[c % 5]
        return x, sc, sh, False
    if case.pre == "neg_scales":
        sc = np.array([-2.0, -1.0, -0.5], dtype=np.float32)[c % 3]
    else:
        sc = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], dtype=np.float32)[c % 6]
    sh = (np.array([-4, -1, 0, 2, 3, 1, -3], dtype=np.float32) / 4)[c % 7]
    return x, sc, sh, case.pre != "affine"


# ---- the reference ------------------------------------------------------------------------------------------------------------
def keep_ref(x, sc, sh, relu):
    """bf16(relu(fma(x, scale, shift))) as bf16 bit patterns"""
    v = x
    if sc is not None:
        v = (x * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32).astype(np.float64)
    if relu:
        v = np.maximum(v, 0.0)
    return bf16_bits(v.astype(np.float32))


def pool_ref(vals, pool, odims):
    """window scan over float64 `vals` [B,T,H,W,C]: (max, window-relative tap of the FIRST maximum)"""
    (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = pool
    B, T, H, W, Cc = vals.shape
    best = np.full(odims, -np.inf)
    arg = np.zeros(odims, dtype=np.uint8)
    for b in range(B):
        for to in range(odims[1]):
            for ho in range(odims[2]):
                for wo in range(odims[3]):
                    tap = -1
                    for kt in range(kT):
                        for kh in range(kH):
                            for kw in range(kW):
                                tap += 1
                                t, h, w = to * sT - pT + kt, ho * sH - pH + kh, wo * sW - pW + kw
                                if not (0 <= t < T and 0 <= h < H and 0 <= w < W):
                                    continue
                                v = vals[b, t, h, w]
                                m = v > best[b, to, ho, wo]
                                best[b, to, ho, wo][m] = v[m]
                                arg[b, to, ho, wo][m] = tap
    return best, arg


# ---- a CPU model of the kernel: one lane per output voxel, every tap transformed, owned taps stored ------------------------------
class Model:
    """what csrc/pool.hip does, in numpy on host buffers.  The `wrong` switches build the mistakes the case table must catch."""
    wrong = None            # "owner_shift" | "unrounded" | "drop_partial" | "x_strides"

    def __init__(self, wrong=None):
        self.wrong = wrong
        self.error = b""

    def vinet_last_error(self):
        return self.error

    @staticmethod
    def _oct(g, dt):
        Cc = g.dims[4]
        return Cc % 8 == 0 and g.ld % 8 == 0 and g.sB % 8 == 0 and (g.off * (4 if dt == F32 else 2)) % 16 == 0

    def keep_ok(self, case, gx, gy, gk, am_aligned=True):
        (k, s, p), (B, T, H, W, Cc), od = case.pool, case.dims, case.odims
        if case.dt != BF16:
            self.error = b"bf16 only"
            return 0
        if not (self._oct(gx, case.dt) and self._oct(gy, case.dt) and am_aligned):
            self.error = b"not on maxpool_fwd8_pk_kernel"
            return 0
        if case.pool == K3 and T >= 2 and B * H * W * (Cc // 8) >= POOL_FILL_COLS:
            self.error = b"not on maxpool_fwd8_pk_kernel"
            return 0
        if not self._oct(gk, case.dt) or gk.dims != gx.dims:
            self.error = b"keep off the grid"
            return 0
        if not all(kk >= pp + ss for kk, ss, pp in zip(k, s, p)):
            self.error = b"lacks the owning taps"
            return 0
        if not all(o * ss >= i for o, ss, i in zip(od[1:4], s, (T, H, W))):
            self.error = b"do not cover the input"
            return 0
        return 1

    @staticmethod
    def _pre(xb, sc, sh, relu, rounded=True):
        """bf16 bits -> transformed values (float64 of the bf16 result) and the bits stored"""
        v = bf16_value(xb)
        if sc is not None:
            v = (v * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)
            if relu:
                v = np.maximum(v, np.float32(0))
            bits = bf16_bits(v) if rounded else (v.view(np.uint32) >> 16).astype(np.uint16)
        else:
            bits = xb.copy()
            if relu:
                bits[bits >= 0x8000] = 0
        return bf16_value(bf16_bits(v.astype(np.float32))) if sc is not None else bf16_value(bits), bits

    def pool(self, case, xbuf, gx, pre, ybuf, gy, am, keep=None):
        """vinet_maxpool3d (keep None) / vinet_maxpool3d_keep on uint16 host buffers; returns rc"""
        if keep is not None and not self.keep_ok(case, gx, gy, keep[1]):
            return -1
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = case.pool
        sc, sh, relu = pre
        B, T, H, W, Cc = case.dims
        x, y = gx.strided(xbuf), gy.strided(ybuf)
        if keep is not None:
            kbuf, gk = keep
            kv = gk.strided(kbuf)
            if self.wrong == "x_strides":
                wrong = Geo(gx.dims, gx.form)
                wrong.off = gk.off
                kv = wrong.strided(kbuf) if wrong.off + (wrong.n - 2 * PAD) <= kbuf.size else None
        d = 1 if self.wrong == "owner_shift" else 0
        for b in range(B):
            for to in range(case.odims[1]):
                for ho in range(case.odims[2]):
                    for wo in range(case.odims[3]):
                        best, arg, tap = np.full(Cc, -np.inf), np.zeros(Cc, dtype=np.uint8), -1
                        for kt in range(kT):
                            for kh in range(kH):
                                for kw in range(kW):
                                    tap += 1
                                    t, h, w = to * sT - pT + kt, ho * sH - pH + kh, wo * sW - pW + kw
                                    if not (0 <= t < T and 0 <= h < H and 0 <= w < W):
                                        continue
                                    v, bits = self._pre(x[b, t, h, w], sc, sh, relu, self.wrong != "unrounded")
                                    m = v > best
                                    best[m], arg[m] = v[m], tap
                                    own = pT + d <= kt < pT + sT + d and pH + d <= kh < pH + sH + d and pW + d <= kw < pW + sW + d
                                    if self.wrong == "drop_partial" and (to * sT + sT > T or ho * sH + sH > H or wo * sW + sW > W):
                                        own = False
                                    if keep is not None and own and kv is not None:
                                        kv[b, t, h, w] = bits
                        y[b, to, ho, wo] = bf16_bits(best.astype(np.float32))
                        if am is not None:
                            o = (((b * case.odims[1] + to) * case.odims[2] + ho) * case.odims[3] + wo) * Cc
                            am[PAD + o:PAD + o + Cc] = arg
        return 0

    def copy_affine(self, case, xbuf, gx, pre, dbuf, gd):
        """vinet_copy_affine: fmaxf before the rounding"""
        sc, sh, relu = pre
        x = bf16_value(gx.strided(xbuf))
        if sc is not None:
            x = (x * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float32)
        if relu:
            x = np.maximum(x, 0)
        gd.strided(dbuf)[...] = bf16_bits(x.astype(np.float32))
        return 0


class HostSide:
    """runs a case on a Model, host buffers"""

    def __init__(self, model):
        self.m = model

    def run(self, case, bufs, pre, which):
        x, y, k, am = bufs["x"], bufs["y"], bufs["keep"], bufs["am"]
        if which == "ok":
            return self.m.keep_ok(case, x[1], y[1], k[1])
        if which == "keep":
            return self.m.pool(case, x[0], x[1], pre, y[0], y[1], am, (k[0], k[1]))
        if which == "plain":
            return self.m.pool(case, x[0], x[1], pre, y[0], y[1], am)
        return self.m.copy_affine(case, x[0], x[1], pre, k[0], k[1])

    def error(self):
        return self.m.vinet_last_error()


class LibSide:
    """runs a case on libvinet_hip.so: the buffers go to the device (or, for the refusals, stay on the host: the argument checks
    run before any launch) and come back after the call"""

    def __init__(self, lib, dev):
        self.lib, self.dev = lib, torch.device(dev)

    def run(self, case, bufs, pre, which):
        dev = {}
        for name in ("x", "y", "keep"):
            a = bufs[name][0]
            dev[name] = torch.from_numpy(a.view(np.int16) if case.dt == BF16 else a).to(self.dev)
        am = torch.from_numpy(bufs["am"]).to(self.dev) if bufs["am"] is not None else None
        sc, sh, relu = pre
        tsc = torch.from_numpy(np.concatenate([sc, np.zeros(4, np.float32)])).to(self.dev) if sc is not None else None
        tsh = torch.from_numpy(np.concatenate([sh, np.zeros(4, np.float32)])).to(self.dev) if sh is not None else None
        a = L.CAffine(tsc.data_ptr() if tsc is not None else None, tsh.data_ptr() if tsh is not None else None, 1 if relu else 0)
        k, s, p = case.pool
        pd = L.CPoolDesc(case.dt, *(k + s + p))
        xc, yc, kc = (bufs[n][1].ct(dev[n]) for n in ("x", "y", "keep"))
        amp = am.data_ptr() + PAD if am is not None else None
        st = torch.cuda.current_stream().cuda_stream if self.dev.type == "cuda" else 0
        if which == "ok":
            return self.lib.vinet_maxpool3d_keep_ok(C.byref(pd), C.byref(xc), a, C.byref(yc), amp, C.byref(kc))
        if which == "keep":
            rc = self.lib.vinet_maxpool3d_keep(C.byref(pd), C.byref(xc), a, C.byref(yc), amp, C.byref(kc), st)
        elif which == "plain":
            rc = self.lib.vinet_maxpool3d(C.byref(pd), C.byref(xc), a, C.byref(yc), amp, st)
        else:
            rc = self.lib.vinet_copy_affine(C.byref(xc), case.dt, a, C.byref(kc), case.dt, 0, st)
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        for name in ("y", "keep"):
            back = dev[name].cpu().numpy()
            bufs[name][0][...] = back.view(np.uint16) if case.dt == BF16 else back
        if am is not None:
            bufs["am"][...] = am.cpu().numpy()
        return rc

    def error(self):
        return self.lib.vinet_last_error()


# ---- the runner ---------------------------------------------------------------------------------------------------------------
def make_bufs(case, xvals):
    gx, gy, gk = Geo(case.dims, case.xf), Geo(case.odims, case.yf), Geo(case.dims, case.kf)
    if case.dt == F32:
        xb = np.full(gx.n, X_OUTSIDE, dtype=np.float32)
        gx.strided(xb)[...] = xvals
        yb, kb = np.full(gy.n, -77.0, dtype=np.float32), np.full(gk.n, -77.0, dtype=np.float32)
    else:
        xb = np.full(gx.n, bf16_bits(np.float32(X_OUTSIDE)), dtype=np.uint16)
        gx.strided(xb)[...] = bf16_bits(xvals.astype(np.float32))
        yb, kb = np.full(gy.n, Y_FILL, dtype=np.uint16), np.full(gk.n, KEEP_FILL, dtype=np.uint16)
    am = np.full(PAD + int(np.prod(case.odims)) + PAD, AM_FILL, dtype=np.uint8) if case.am else None
    return dict(x=(xb, gx), y=(yb, gy), keep=(kb, gk), am=am)


def _copy(bufs):
    return {n: (None if v is None else v.copy()) if n == "am" else (v[0].copy(), v[1]) for n, v in bufs.items()}


class Report:
    def __init__(self):
        self.cases = self.zero_sign = self.elements = 0


def run_case(side, case, report=None):
    """one case on `side`, every gate of the module docstring asserted"""
    x, sc, sh, relu = inputs(case)
    pre = (sc, sh, relu)
    fresh = make_bufs(case, x)
    if not case.serve:
        b = _copy(fresh)
        assert side.run(case, b, pre, "ok") == 0, "%s: the predicate accepts a refused form" % case
        assert side.error(), case
        assert side.run(case, b, pre, "keep") != 0, "%s: the launch of a refused form succeeded" % case
        for n in ("y", "keep"):
            assert np.array_equal(b[n][0], fresh[n][0]), "%s: a refused launch wrote into %s" % (case, n)
        assert b["am"] is None or np.array_equal(b["am"], fresh["am"]), "%s: a refused launch wrote the argmax" % case
        return
    assert case.dt == BF16
    kept, plain, copied = _copy(fresh), _copy(fresh), _copy(fresh)
    assert side.run(case, kept, pre, "ok") == 1, "%s: refused: %r" % (case, side.error())
    assert side.run(case, kept, pre, "keep") == 0, "%s: %r" % (case, side.error())
    assert side.run(case, plain, pre, "plain") == 0, "%s: %r" % (case, side.error())
    assert side.run(case, copied, pre, "copy") == 0, "%s: %r" % (case, side.error())
    gy, gk = fresh["y"][1], fresh["keep"][1]
    # y and argmax: the plain pool's bits
    assert np.array_equal(kept["y"][0], plain["y"][0]), "%s: y differs from vinet_maxpool3d in %d elements" % (
        case, int((kept["y"][0] != plain["y"][0]).sum()))
    if case.am:
        assert np.array_equal(kept["am"], plain["am"]), "%s: argmax differs from vinet_maxpool3d" % case
        assert (kept["am"][:PAD] == AM_FILL).all() and (kept["am"][-PAD:] == AM_FILL).all(), "%s: argmax guards" % case
    # keep: every element written, and the copy's numbers
    kk, cc = gk.strided(kept["keep"][0]), gk.strided(copied["keep"][0])
    assert not (kk == KEEP_FILL).any(), "%s: %d elements of keep were never written" % (case, int((kk == KEEP_FILL).sum()))
    diff = kk != cc
    zeros = diff & ((kk & 0x7FFF) == 0) & ((cc & 0x7FFF) == 0)
    assert np.array_equal(diff, zeros), "%s: keep differs from vinet_copy_affine in %d elements beyond the sign of a zero" % (
        case, int((diff & ~zeros).sum()))
    # everything outside the views
    for n, g in (("y", gy), ("keep", gk)):
        out = ~g.mask()
        assert np.array_equal(kept[n][0][out], fresh[n][0][out]), "%s: bytes outside %s changed" % (case, n)
    assert np.array_equal(kept["x"][0], fresh["x"][0])
    # ... and the independent reference
    kref = keep_ref(x, sc, sh, relu)
    assert np.array_equal(bf16_value(kk), bf16_value(kref)), "%s: keep differs from the float64 reference" % case
    best, arg = pool_ref(bf16_value(kref), case.pool, case.odims)
    assert np.array_equal(bf16_value(gy.strided(kept["y"][0])), best), "%s: y differs from the float64 reference" % case
    if case.am:
        assert np.array_equal(kept["am"][PAD:-PAD].reshape(case.odims), arg), "%s: argmax differs from the reference" % case
    if report is not None:
        report.cases += 1
        report.zero_sign += int(zeros.sum())
        report.elements += kk.size


def owners(n, k, s, p):
    """per input index 0 .. n-1 of one dimension: how many (output, owned tap) pairs address it"""
    out = (n + 2 * p - k) // s + 1
    cnt = [0] * n
    for o in range(max(out, 0)):
        for tap in range(p, p + s):
            i = o * s - p + tap
            if tap < k and 0 <= i < n:
                cnt[i] += 1
    return cnt, out
