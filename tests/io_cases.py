"""The input and output pipeline at value, size and tie edges: case tables, references, gates and the runners that the host test
(tests/test_io_cases_host.py, CPU model of the ABI) and the GPU test (tests/test_gpu_io_kernels.py, libvinet_hip.so) share.

Families: vinet_frames_preprocess, vinet_gt_preprocess, vinet_audio_excerpt (csrc/preproc.hip), vinet_resize_blur, vinet_minmax,
vinet_normalize_u8 (csrc/postproc.hip).  A `Side` (tests/tail_cases.py) says where a case runs; each check_* function runs one
case there, asserts its gates and returns what it measured: `bits`, the number of elements compared bit for bit, and for the
audio window the worst error beside its gate.

GATES.  Everything is bit for bit (np.array_equal on float32 / uint8 results and on the min / max keys) against
  * frames: the bytes the real Pillow resampler produced (tests/golden/io_edges.npz, recorded by make_io_edge_goldens.py), taken
    through ToTensor / Normalize as the plain float32 expression ((byte / 255) - mean) / std, written out here;
  * maps and ground truth: oracle/postproc_cpu.py and oracle/preproc_cpu.py.
The one exception is the Hanning window of vinet_audio_excerpt, which keeps the gate of test_gpu_kernels.py::test_audio_excerpt:
exact zeros outside [lo, lo + M), |got - ref| <= 1e-9 + 2e-7 * max|ref| inside (the window is a double cosine from two libms,
rounded to float32 and multiplied in float32: two roundings, 1.2e-7 relative).  The audio reference is
0.5 - 0.5 cos(2 pi n / (M - 1)) in float64 (M == 1 -> 1) times the float32 samples.

The keys of a map that holds only -0.0 and +0.0 are the one place where "bit for bit" is not defined: IEEE 754 minNum / maxNum
may return either zero, and so may numpy's min.  There both keys must decode to a zero of either sign and the bytes must be 0.

INDEPENDENT FLOAT64 REFERENCES.  A misreading shared by the oracle and the kernels would pass a bit gate between them, so the
cv2-derived paths are also held, on BOTH sides, against float64 references that share no code with the oracle, through
tests.tail_cases.gate_bound with these round-off bounds (u = 2^-24, gamma(k) = k u / (1 - k u)):

  resize (float32 maps).  The source coordinate is the spec's float32 f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s
      (exact: Sterbenz), with the border rule of resize.cpp; the reference then weighs the four taps in double.  The kernel rounds
      1 - f (1), each product of the row pass (1), its sum (1), and the same three in the column pass: 6 roundings on every path
      from a source sample to the result, all weights non-negative, so |error| <= gamma(6) * R|src| where R|src| is the same
      interpolation of |src|.
  blur.  scipy.ndimage.correlate1d(mode="mirror") (= BORDER_REFLECT_101) with the float32 kernel values in double, on the float64
      resize.  Row pass: a product (1) and at most 10 additions behind it (11); column pass: the pair sum (1), the product (1), at
      most 5 additions (7).  With the resize's 6 that is 24 roundings on the longest path; the kernel weights are non-negative, so
      |error| <= gamma(24) * blur(R|src|).
  ground truth.  float32 weights (1 - f is rounded to float32 BEFORE it is widened: that rounding is the spec, and it decides
      `max > 1` for an all-ones map), double sums in the spec's order, the decision, / 255.0, one conversion to float32:
      |error| <= (u + 2^-50) |ref| (the 2^-50 covers the handful of double roundings should a compiler order a sum differently).

These bounds come from the operation counts above and the number formats, not from what any implementation measures.

WRONG REFERENCES.  Ref is the reference side of every bit gate; its subclasses below are each wrong in one way a kernel could be
wrong (round half away, double weights, BORDER_REFLECT, no byte rounding between the Pillow passes, a reduction that drops the
last element, a channel mix-up).  The host test shows that each of them fails the case that was put in the tables for it."""
import contextlib
import ctypes as C
import functools
import zlib

import numpy as np
import torch

from oracle import postproc_cpu as P
from oracle import preproc_cpu as Q
from tests import goldens as G
from tests.tail_cases import U32, Side, gate_bound  # noqa: F401  (Side: re-exported for the two test modules)
from vinet_amd import synth

FENCE = 256              # bytes in front of and behind every output and scratch buffer (a multiple of 16: the scratch stays aligned)
F32_MARK = float("nan")
U8_MARK = 0xA5
KEY_MARK = 0xA5A5A5A5


def gamma(k):
    return k * U32 / (1.0 - k * U32)


class Fenced:
    """`n` elements of `dtype` for a kernel to write, inside a longer buffer filled with a sentinel that must survive"""

    def __init__(self, side, n, dtype, mark):
        self.n, self.dt = int(n), np.dtype(dtype)
        host = np.full(self.n + 2 * (FENCE // self.dt.itemsize), mark, self.dt)
        self.before = host.view(np.uint8).copy()
        self.buf = side.put(torch.from_numpy(host.view(np.uint8)))

    @property
    def ptr(self):
        return self.buf.data_ptr() + FENCE

    def read(self, what):
        after = self.buf.cpu().numpy()
        lo, hi = FENCE, FENCE + self.n * self.dt.itemsize
        assert np.array_equal(after[:lo], self.before[:lo]), what + ": bytes in front of the buffer changed"
        assert np.array_equal(after[hi:], self.before[hi:]), what + ": bytes behind the buffer changed"
        return after[lo:hi].view(self.dt).copy()


def _put(side, arr):
    return side.put(torch.from_numpy(np.ascontiguousarray(arr)))


def mm_key(f):
    """the order-preserving float32 -> uint32 map of the key table (include/vinet_hip.h)"""
    u = np.asarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def mm_unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# =====================================================================================================================
# independent float64 references
# =====================================================================================================================
def src_coords(dsize, ssize, zero_at_border):
    """resize.cpp: taps (s, s + 1) and the float32 fraction f of every destination index.  Horizontally a tap pair off the row
    becomes (edge, weight 1); vertically the rows are clipped and the weights stay."""
    scale = 1.0 / (float(dsize) / float(ssize))
    f = np.array([np.float32((d + 0.5) * scale - 0.5) for d in range(dsize)], dtype=np.float32)
    s = np.floor(f)
    f = f - s                                  # float32 - float32: exact
    s = s.astype(np.int64)
    if zero_at_border:
        for d in range(dsize):
            if s[d] < 0:
                s[d], f[d] = 0, 0.0
            if s[d] >= ssize - 1:
                s[d], f[d] = ssize - 1, 0.0
    return np.clip(s, 0, ssize - 1), np.clip(s + 1, 0, ssize - 1), f


def resize_ref64(src, oh, ow):
    """bilinear resize of [..., H, W] with the spec's float32 source coordinates and double weights and sums"""
    s = np.asarray(src).astype(np.float64)
    H, W = s.shape[-2:]
    x0, x1, fx = src_coords(ow, W, True)
    y0, y1, fy = src_coords(oh, H, False)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)[:, None]
    rows = s[..., :, x0] * (1.0 - fx) + s[..., :, x1] * fx
    return rows[..., y0, :] * (1.0 - fy) + rows[..., y1, :] * fy


def gaussian11():
    """getGaussianKernel(11, -1, CV_32F): sigma = 0.3 * ((11 - 1) * 0.5 - 1) + 0.8 = 2; float32 values, as doubles"""
    t = np.array([np.float32(np.exp(-0.125 * (i - 5) ** 2)) for i in range(11)], dtype=np.float32)
    total = float(np.sum(t.astype(np.float64)))
    return np.array([np.float32(float(v) * (1.0 / total)) for v in t], dtype=np.float64)


def blur_ref64(img):
    import scipy.ndimage as ndi
    k = gaussian11()
    return ndi.correlate1d(ndi.correlate1d(np.asarray(img, np.float64), k, axis=-1, mode="mirror"), k, axis=-2, mode="mirror")


def resize_blur_ref64(src, oh, ow):
    """(reference, elementwise round-off bound of a float32 implementation): module docstring"""
    return blur_ref64(resize_ref64(src, oh, ow)), gamma(24) * blur_ref64(resize_ref64(np.abs(np.asarray(src, np.float64)), oh, ow))


def gt_resized64(g8, oh=None, ow=None):
    """the float64 maps BEFORE the `max > 1` decision: float32 weights, widened; double sums, rows first"""
    g = np.asarray(g8, dtype=np.uint8).astype(np.float64)
    H, W = g.shape[-2:]
    if oh is not None and (oh, ow) != (H, W):
        x0, x1, fx = src_coords(ow, W, True)
        y0, y1, fy = src_coords(oh, H, False)
        a0, a1 = (np.float32(1) - fx).astype(np.float64), fx.astype(np.float64)
        b0, b1 = (np.float32(1) - fy).astype(np.float64)[:, None], fy.astype(np.float64)[:, None]
        rows = g[..., :, x0] * a0 + g[..., :, x1] * a1
        g = rows[..., y0, :] * b0 + rows[..., y1, :] * b1
    return g


def gt_ref64(g8, oh=None, ow=None):
    """dataloader.py:283-296 in float64 BEFORE the conversion to float32, and its bound"""
    out = np.stack([m / 255.0 if m.max() > 1.0 else m for m in gt_resized64(g8, oh, ow)])
    return out, (U32 + 2.0 ** -50) * np.abs(out)


def hanning64(M):
    if M == 1:
        return np.ones(1, np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(M, dtype=np.float64) / (M - 1))


# =====================================================================================================================
# the reference side of the bit gates, and its wrong variants
# =====================================================================================================================
@contextlib.contextmanager
def _patched(mod, name, value):
    old = getattr(mod, name)
    setattr(mod, name, value)
    try:
        yield
    finally:
        setattr(mod, name, old)


def _normalize_y(img):
    """utils.py:66-78 up to the rounding: y = clamp(x * 255 + 0.5, 0, 255) of ONE map in float32 (wrong variants and tie counts only)"""
    img = np.asarray(img, dtype=np.float32)
    mn, mx = float(img.min()), float(img.max())
    x = np.clip(img, np.float32(mn), np.float32(mx)).astype(np.float32)
    x = ((x + np.float32(-mn)).astype(np.float32) / np.float32(mx - mn + 1e-5)).astype(np.float32)
    y = ((x * np.float32(255)).astype(np.float32) + np.float32(0.5)).astype(np.float32)
    return np.clip(y, np.float32(0), np.float32(255))


class Ref:
    """what every bit gate compares with"""
    name = "reference"

    def pil(self, shape, kind):
        return frame_case(shape, kind)[1]

    def to_tensor(self, pil, mean, std):
        """ToTensor / Normalize on uint8 [N, h, w, 3] -> float32 [N, 3, h, w]"""
        x = (pil.astype(np.float32) / np.float32(255)).astype(np.float32)
        x = ((x - np.asarray(mean, np.float32)).astype(np.float32) / np.asarray(std, np.float32)).astype(np.float32)
        return np.ascontiguousarray(np.moveaxis(x, -1, -3))

    def gt(self, g8, oh, ow):
        return Q.gt_preprocess(g8, oh, ow)

    def resize_blur(self, src, oh, ow):
        return P.resize_blur(src, oh, ow)

    def u8(self, maps):
        """[B, H, W]: every map on its own"""
        assert maps.ndim == 3
        return P.normalize_u8(maps)

    def minmax(self, flat):
        return flat.min(1), flat.max(1)


class HalfAwayRef(Ref):
    """roundf / (int)(y + 0.5f) in place of rintf"""
    name = "round half away from zero"

    def u8(self, maps):
        return np.stack([np.floor(_normalize_y(m) + np.float32(0.5)).astype(np.uint8) for m in maps])


class DoubleWeightRef(Ref):
    """cv2.resize on CV_64F with the coefficients kept in double"""
    name = "cv2 weights in double"

    def gt(self, g8, oh, ow):
        orig = P._linear_coeffs

        def coeffs(dsize, ssize, zero_at_border):
            s, s1, _, a1 = orig(dsize, ssize, zero_at_border)
            return s, s1, 1.0 - a1.astype(np.float64), a1.astype(np.float64)
        with _patched(P, "_linear_coeffs", coeffs):
            return Q.gt_preprocess(g8, oh, ow)


def _reflect(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT): fedcba|abcdefgh|hgfedcb"""
    i = np.asarray(i, dtype=np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        lo, hi = i < 0, i >= n
        if not (lo.any() or hi.any()):
            return i
        i = np.where(lo, -i - 1, i)
        i = np.where(hi, 2 * n - 1 - i, i)


class ReflectRef(Ref):
    name = "BORDER_REFLECT"

    def resize_blur(self, src, oh, ow):
        with _patched(P, "reflect101", _reflect):
            return P.resize_blur(src, oh, ow)


class NoByteRoundingRef(Ref):
    """both Pillow passes in one go: the horizontal sums are not rounded to bytes before the vertical pass"""
    name = "no byte rounding between the passes"

    def pil(self, shape, kind):
        img = frame_case(shape, kind)[0].astype(np.int64)
        _, N, H, W, oh, ow = FRAME_SHAPES[shape]
        bh, kh = Q.resample_coeffs(W, ow)
        bv, kv = Q.resample_coeffs(H, oh)
        hz = np.stack([(img[:, :, a:a + n, :] * kh[xx, :n].astype(np.int64)[:, None]).sum(2) for xx, (a, n) in enumerate(bh)], 2)
        vt = np.stack([(hz[:, a:a + n] * kv[yy, :n].astype(np.int64)[:, None, None]).sum(1) for yy, (a, n) in enumerate(bv)], 1)
        return np.clip((vt + (1 << (2 * Q.PRECISION_BITS - 1))) >> (2 * Q.PRECISION_BITS), 0, 255).astype(np.uint8)


class DropsLastRef(Ref):
    """a reduction that never sees element n - 1"""
    name = "maximum over the first n - 1 elements"

    def minmax(self, flat):
        f = flat[:, :-1] if flat.shape[1] > 1 else flat
        return f.min(1), f.max(1)

    def gt(self, g8, oh, ow):
        if oh is not None and (oh, ow) != tuple(g8.shape[-2:]):
            return Q.gt_preprocess(g8, oh, ow)
        g = np.asarray(g8).astype(np.float64)
        return np.stack([(m / 255.0 if m.reshape(-1)[:-1].max() > 1.0 else m).astype(np.float32) for m in g])


class ChannelMixRef(Ref):
    name = "mean / std of another channel"

    def to_tensor(self, pil, mean, std):
        return Ref.to_tensor(self, pil, list(mean[1:]) + list(mean[:1]), list(std[1:]) + list(std[:1]))


REF = Ref()


# =====================================================================================================================
# 1. vinet_frames_preprocess
# =====================================================================================================================
# name -> (name, N, H, W, oH, oW)
_FRAME_SHAPES = [
    ("fullhd_54x", 1, 1080, 1920, 20, 31),          # 54x / 62x down: ksize 109 and 125
    ("src1x1", 1, 1, 1, 5, 5),
    ("src2x2_up", 1, 2, 2, 224, 384),
    ("src_w1", 1, 64, 1, 20, 7),
    ("src_h1", 1, 1, 64, 7, 20),
    ("out1x1", 1, 360, 640, 1, 1),
    ("out_w1", 1, 9, 640, 224, 1),
    ("coeff_seam", 1, 255, 257, 128, 129),         # resample_coeffs_kernel's 128-thread block: exactly one, and one thread more
    ("v_identity", 1, 17, 1000, 17, 3),
    ("same3x3", 1, 3, 3, 3, 3),
    ("three_frames", 3, 37, 53, 20, 31),           # row = n * H + y, a ragged last block
]
FRAME_SHAPES = {s[0]: s for s in _FRAME_SHAPES}
IMAGE_KINDS = ["random", "white", "black", "checker", "sparse"]
NORMS = [
    ("default", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    ("identity", (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),                    # the output is byte / 255 exactly
    ("distinct", (0.1, 0.2, 0.3), (0.5, 0.6, 0.7)),
]
STORE_INPUT_BYTES = 4096     # inputs up to this size are stored in the fixture; larger ones are regenerated and checked by CRC32
EDGE_FIXTURE = "io_edges"


def make_image(shape, kind):
    """uint8 [N, H, W, 3]: closed forms, or vinet_amd.synth streams named after the case"""
    _, N, H, W, _, _ = FRAME_SHAPES[shape]
    dims = (N, H, W, 3)
    n = N * H * W * 3
    if kind == "random":
        return np.floor(synth.uniform01("io_edges/" + shape, n, 1) * 256.0).astype(np.uint8).reshape(dims)
    if kind == "white":
        return np.full(dims, 255, np.uint8)
    if kind == "black":
        return np.zeros(dims, np.uint8)
    if kind == "checker":        # 0 / 255 by the parity of frame + row + column + channel
        f, y, x, c = np.ogrid[:N, :H, :W, :3]
        return (((f + y + x + c) & 1) * 255).astype(np.uint8)
    assert kind == "sparse"
    return ((synth.uniform01("io_edges/" + shape, n, 2) < 0.03) * 255).astype(np.uint8).reshape(dims)


@functools.lru_cache(maxsize=None)
def _edge_fixture():
    return G.load(EDGE_FIXTURE)


@functools.lru_cache(maxsize=8)
def frame_case(shape, kind):
    """(input bytes [N, H, W, 3], Pillow's resized bytes [N, oH, oW, 3]) of one case of the fixture"""
    z, meta = _edge_fixture()
    key = "%s.%s" % (shape, kind)
    assert meta["shapes"][shape] == list(FRAME_SHAPES[shape][1:]), "io_edges.npz was recorded for other shapes: rerun make_io_edge_goldens.py"
    img = z[key + ".in"] if key + ".in" in z else make_image(shape, kind)
    assert zlib.crc32(np.ascontiguousarray(img).tobytes()) == meta["crc32"][key], key + ": the input is not the one the fixture was recorded from"
    return img, z[key + ".pil"]


def check_frames(side, shape, kind, ref=REF, norms=None):
    """`norms`: names of the NORMS to run (None: all three)"""
    _, N, H, W, oh, ow = FRAME_SHAPES[shape]
    img = frame_case(shape, kind)[0]
    pil = ref.pil(shape, kind)
    assert img.shape == (N, H, W, 3) and pil.shape == (N, oh, ow, 3)
    src = _put(side, img)
    nws = side.api.vinet_frames_preprocess_ws_bytes(N, H, W, oh, ow)
    assert nws > 0
    bits = 0
    for nname, mean, std in NORMS:
        if norms is not None and nname not in norms:
            continue
        what = "frames %s/%s/%s" % (shape, kind, nname)
        out = Fenced(side, N * 3 * oh * ow, np.float32, F32_MARK)
        ws = Fenced(side, nws, np.uint8, U8_MARK)
        ms = (C.c_float * 6)(*(list(mean) + list(std)))
        side.call("vinet_frames_preprocess", src.data_ptr(), N, H, W, out.ptr, oh, ow, ms, ws.ptr)
        got = out.read(what).reshape(N, 3, oh, ow)
        ws.read(what + " scratch")
        want = ref.to_tensor(pil, mean, std)
        assert np.array_equal(got, want), "%s: %d of %d values differ from Pillow's" % (what, int((got != want).sum()), want.size)
        if nname == "identity":
            exact = np.moveaxis(pil.astype(np.float32) / np.float32(255), -1, -3)
            assert np.array_equal(got, exact), what + ": mean 0 / std 1 is not byte / 255"
        bits += want.size
    return dict(bits=bits)


# =====================================================================================================================
# 2. vinet_gt_preprocess
# =====================================================================================================================
def _gt_bytes(name, dims, seed=1):
    return np.floor(synth.uniform01("io_gt/" + name, int(np.prod(dims)), seed) * 256.0).astype(np.uint8).reshape(dims)


def _gt_binary(name, dims, seed=1):
    return (synth.uniform01("io_gt/" + name, int(np.prod(dims)), seed) < 0.1).astype(np.uint8).reshape(dims)


def _gt_last_two(at):
    g = _gt_binary("fullhd", (1, 1080, 1920))
    g.reshape(-1)[at] = 2
    return g


def _gt_mixed():
    g = np.stack([_gt_bytes("mix0", (45, 80)), _gt_binary("mix1", (45, 80)), _gt_bytes("mix2", (45, 80), 2), np.zeros((45, 80), np.uint8)])
    assert g[1].max() == 1
    return g


def _gt_max_one():
    g = np.zeros((1, 45, 80), np.uint8)
    g[0, 44, 79] = 1
    return g


# name -> (maps uint8 [N, H, W], (oH, oW) or None, what the result must be: "div" (every map / 255), "keep", or a list per map)
GT_CASES = {
    "ones_36x64_up": (lambda: np.ones((1, 36, 64), np.uint8), (224, 384), "div"),          # max = (1 + 2^-25)^2: divided
    "ones_360x640_down": (lambda: np.ones((1, 360, 640), np.uint8), (224, 384), "keep"),   # max = 1 exactly: kept
    "fullhd_two_at_end": (lambda: _gt_last_two(-1), None, "div"),                          # blocks capped at 1024, the 2 in the tail
    "fullhd_two_at_start": (lambda: _gt_last_two(0), None, "div"),
    "zeros": (lambda: np.zeros((1, 45, 80), np.uint8), None, "keep"),
    "max_one": (_gt_max_one, None, "keep"),
    "all255": (lambda: np.full((1, 45, 80), 255, np.uint8), None, "div"),
    "mixed4": (_gt_mixed, None, ["div", "keep", "div", "keep"]),
    "mixed4_resized": (_gt_mixed, (28, 48), ["div", None, "div", "keep"]),      # (a resized 0 / 1 map may end a rounding above 1)
    "src_h1": (lambda: _gt_bytes("h1", (2, 1, 64)), (7, 20), "div"),
    "src_w1": (lambda: _gt_bytes("w1", (2, 64, 1)), (20, 7), "div"),
    "src1x1": (lambda: np.full((1, 1, 1), 200, np.uint8), (5, 5), "div"),
    "hd_down": (lambda: _gt_bytes("hd", (1, 720, 1280)), (224, 384), "div"),
    "w_only": (lambda: _gt_bytes("wonly", (1, 224, 500)), (224, 384), "div"),
    "h_only": (lambda: _gt_bytes("honly", (1, 300, 384)), (224, 384), "div"),
}


def check_gt(side, name, ref=REF):
    make, size, expect = GT_CASES[name]
    g8 = make()
    N, H, W = g8.shape
    oh, ow = size if size is not None else (H, W)
    want = ref.gt(g8, *(size or (None, None)))
    r64, bound = gt_ref64(g8, *(size or (None, None)))
    what = "gt " + name
    src = _put(side, g8)
    nws = side.api.vinet_gt_preprocess_ws_bytes(N, oh, ow)
    assert nws > 0
    out = Fenced(side, N * oh * ow, np.float32, F32_MARK)
    ws = Fenced(side, nws, np.uint8, U8_MARK)
    side.call("vinet_gt_preprocess", src.data_ptr(), N, H, W, out.ptr, oh, ow, ws.ptr)
    got = out.read(what).reshape(N, oh, ow)
    ws.read(what + " scratch")
    assert np.array_equal(got, want), "%s: %d of %d values differ, max abs diff %g" % (what, int((got != want).sum()), want.size,
                                                                                  float(np.abs(got.astype(np.float64) - want).max()))
    gate_bound(_t64(got), _t64(r64), _t64(bound), what + " against float64")
    # the decision of every map, read off the result: a divided map cannot exceed 1, a kept one holds its integers
    for b, e in enumerate([expect] * N if isinstance(expect, str) else expect):
        top = float(g8[b].max())
        if e is None:
            continue
        if e == "div":
            assert top > 0 and float(got[b].max()) <= 1.0 + 2.0 ** -23 and float(got[b].max()) < top, "%s: map %d was not divided" % (what, b)
        else:
            assert top <= 1 and abs(float(got[b].max()) - top) <= 2.0 ** -24, "%s: map %d was divided" % (what, b)
    if name == "ones_36x64_up":
        assert bool((got == np.float32(1.0 / 255.0)).all()), what + ": the whole map must be 1 / 255"
    if name == "ones_360x640_down":
        assert float(np.abs(got.astype(np.float64) - 1.0).max()) <= 2.0 ** -24, what + ": the map must stay 1"
    return dict(bits=want.size)


# =====================================================================================================================
# 3. vinet_audio_excerpt
# =====================================================================================================================
AUDIO_WIN = 70560
# name -> (waveform length, start, end, win)
AUDIO_CASES = {
    "m0": (2000, 300, 299, AUDIO_WIN),
    "start_at_n": (2000, 2000, 2100, AUDIO_WIN),
    "start_past_n": (2000, 2500, 2600, AUDIO_WIN),
    "m1_last_sample": (2000, 1999, 5000, AUDIO_WIN),
    "m2_all_zero": (2000, 0, 1, AUDIO_WIN),
    "m_eq_win_odd": (2000, 0, 6, 7),
    "m_eq_win_even": (2000, 0, 1999, 2000),
    "m_win_minus_1": (2000, 0, 5, 7),
    "win1": (2000, 3, 3, 1),
    "win257": (2000, 100, 300, 257),
    "long_to_last_sample": (200000, 200000 - AUDIO_WIN, 199999, AUDIO_WIN),
    "long_end_clamped": (200000, 200000 - AUDIO_WIN, 260000, AUDIO_WIN),
}


@functools.lru_cache(maxsize=None)
def audio_wave(n):
    return (synth.normal("io_audio", (n,), n).numpy().astype(np.float32) * np.float32(2.0 ** -8)).astype(np.float32)


def audio_ref(wav, start, end, win):
    """(reference float64 [win], lo, M)"""
    seg = wav[start:end + 1].astype(np.float64)
    M = seg.shape[0]
    lo = win // 2 - M // 2
    out = np.zeros(win, np.float64)
    if M:
        out[lo:lo + M] = hanning64(M) * seg
    return out, lo, M


def check_audio(side, name):
    n, start, end, win = AUDIO_CASES[name]
    wav = audio_wave(n)
    ref, lo, M = audio_ref(wav, start, end, win)
    assert 0 <= M <= win
    what = "audio " + name
    wd = _put(side, wav)
    out = Fenced(side, win, np.float32, F32_MARK)
    side.call("vinet_audio_excerpt", wd.data_ptr(), n, start, end, out.ptr, win)
    got = out.read(what)
    outside = np.ones(win, bool)
    outside[lo:lo + M] = False
    assert not got[outside].any(), "%s: %d non-zero samples outside the excerpt" % (what, int((got[outside] != 0).sum()))
    lim = 1e-9 + 2e-7 * float(np.abs(ref).max())
    err = float(np.abs(got.astype(np.float64) - ref).max())
    assert err <= lim, "%s: %g > %g" % (what, err, lim)
    if name == "m2_all_zero":
        assert M == 2 and not got.any()
    return dict(bits=int(outside.sum()), audio_err=err, audio_gate=lim)


# =====================================================================================================================
# 4. vinet_resize_blur with vinet_minmax / vinet_normalize_u8 behind it
# =====================================================================================================================
# name -> (B, H, W, oH, oW)
_RB_SHAPES = [
    ("tile_exact", 1, 24, 40, 32, 64),
    ("tile_plus1", 1, 24, 40, 33, 65),
    ("tile_minus1", 2, 24, 40, 31, 63),
    ("four_tiles", 1, 24, 40, 64, 128),
    ("flat_wide", 1, 24, 40, 3, 130),              # lower than the blur radius, wider than two tiles
    ("tall_narrow", 1, 24, 40, 70, 2),
    ("batch5", 5, 7, 9, 20, 31),
    ("src1x1", 1, 1, 1, 40, 70),
    ("src_h1", 1, 1, 20, 33, 65),
    ("src_w1", 1, 17, 1, 33, 65),
    ("fullhd_down", 1, 1080, 1920, 36, 64),
]
RB_SHAPES = {s[0]: s for s in _RB_SHAPES}
RB_VALUES = ["sigmoid", "negative", "mixed", "constant"]
RB_IMPULSES = {"corner": (0, 0), "last": (63, 127), "tile_last": (31, 63), "tile_first": (32, 64)}      # on a 64 x 128 map, same size
RB_CONSTANT = 0.25       # a power of two: products and the weight sums are exact, so every sample of the result is the same float


def rb_source(shape, values):
    _, B, H, W, _, _ = RB_SHAPES[shape]
    if values == "sigmoid":
        return torch.sigmoid(synth.normal("io_rb/" + shape, (B, H, W), 3) * 2.0 - 1.0).numpy()
    if values == "negative":
        return (-synth.uniform("io_rb/" + shape, (B, H, W), 4, 1.0, 2.0)).numpy()
    if values == "mixed":
        return synth.uniform("io_rb/" + shape, (B, H, W), 5, -3e4, 3e4).numpy()
    assert values == "constant"
    return np.full((B, H, W), RB_CONSTANT, np.float32)


def rb_impulse(name):
    src = np.zeros((1, 64, 128), np.float32)
    src[(0,) + RB_IMPULSES[name]] = 1.0
    return src


def check_resize_blur(side, src, oh, ow, what, ref=REF, constant=False):
    src = np.ascontiguousarray(src, dtype=np.float32)
    B, H, W = src.shape
    n = oh * ow
    want = ref.resize_blur(src, oh, ow)
    r64, bound = resize_blur_ref64(src, oh, ow)
    want8 = ref.u8(want)
    lo, hi = ref.minmax(want.reshape(B, n))
    wkeys = np.stack([mm_key(lo), mm_key(hi)], 1)
    if constant:
        assert np.unique(want).size == 1 and not want8.any(), what + ": the reference of a constant map is not constant"
    sd = _put(side, src)
    out, out2 = Fenced(side, B * n, np.float32, F32_MARK), Fenced(side, B * n, np.float32, F32_MARK)
    mm, mm2 = Fenced(side, 2 * B, np.uint32, KEY_MARK), Fenced(side, 2 * B, np.uint32, KEY_MARK)
    u8 = Fenced(side, B * n, np.uint8, U8_MARK)
    side.call("vinet_resize_blur", sd.data_ptr(), B, H, W, out.ptr, oh, ow, mm.ptr)
    side.call("vinet_minmax", out.ptr, B, n, mm2.ptr)
    side.call("vinet_resize_blur", sd.data_ptr(), B, H, W, out2.ptr, oh, ow, None)
    side.call("vinet_normalize_u8", out.ptr, mm.ptr, B, n, u8.ptr)
    got = out.read(what).reshape(B, oh, ow)
    assert np.array_equal(got, want), "%s: %d of %d samples differ, max abs diff %g" % (what, int((got != want).sum()), want.size,
                                                                                   float(np.abs(got - want).max()))
    over = gate_bound(_t64(got), _t64(r64), _t64(bound), what + " against float64")
    keys = mm.read(what + " keys").reshape(B, 2)
    assert np.array_equal(keys, wkeys), "%s: keys %r, expected %r" % (what, mm_unkey(keys), mm_unkey(wkeys))
    assert np.array_equal(mm2.read(what + " keys of vinet_minmax").reshape(B, 2), keys), what + ": vinet_minmax disagrees with resize_blur's keys"
    assert np.array_equal(out2.read(what + " without keys").reshape(B, oh, ow), got), what + ": the call without keys gives another map"
    got8 = u8.read(what + " bytes").reshape(B, oh, ow)
    assert np.array_equal(got8, want8), "%s: %d bytes differ" % (what, int((got8 != want8).sum()))
    return dict(bits=2 * want.size + want8.size + 2 * wkeys.size, f64_over_bound=over)


def check_rb_case(side, shape, values, ref=REF):
    _, B, H, W, oh, ow = RB_SHAPES[shape]
    return check_resize_blur(side, rb_source(shape, values), oh, ow, "resize_blur %s/%s" % (shape, values), ref, values == "constant")


def check_rb_impulse(side, name, ref=REF):
    return check_resize_blur(side, rb_impulse(name), 64, 128, "resize_blur impulse/" + name, ref)


def impulse_outer64(name):
    """what an impulse becomes under the blur: the outer product of the kernel reflected at the borders (float64)"""
    k = gaussian11()
    iy, ix = RB_IMPULSES[name]

    def line(n, at):
        v = np.zeros(n)
        for p in range(n):
            for j in range(11):
                q = p + j - 5
                q = -q if q < 0 else (2 * (n - 1) - q if q >= n else q)
                if q == at:
                    v[p] += k[j]
        return v
    return np.outer(line(64, iy), line(128, ix))[None]


# =====================================================================================================================
# 5. vinet_minmax / vinet_normalize_u8 alone
# =====================================================================================================================
MM_SIZES = [1, 63, 64, 65, 255, 257, 2047, 2049, 2097152 + 2048 + 77]
MM_CAP_N = 1024 * 256 * 8          # past this the grid of both kernels is capped and the stride loop repeats
MM_LOW, MM_HIGH = -2.0, 3.0


def mm_positions(n, order):
    """(index of the minimum, index of the maximum): elements 0 and n - 1, for the capped size n - 77 and n - 1 (both in the ragged
    tail behind the last full round of the grid); "rev" swaps them"""
    first = 0 if n <= MM_CAP_N else n - 77
    return (first, n - 1) if order == "fwd" else (n - 1, first)


@functools.lru_cache(maxsize=4)
def mm_map(n, order):
    x = synth.uniform("io_mm", (n,), n, -1.0, 1.0).numpy().copy()
    lo, hi = mm_positions(n, order)
    x[lo] = MM_LOW
    x[hi] = MM_HIGH          # n = 1: the one element is both
    return x.reshape(1, n)


def mm_batch3():
    x = synth.uniform("io_mm3", (3, 2049), 1, -1.0, 1.0).numpy().copy()
    for b, (lo, vlo, hi, vhi) in enumerate([(0, -5.0, 2048, 7.0), (2048, -1.5, 0, 1.25), (1000, -9.0, 1001, 1.5)]):
        x[b, lo], x[b, hi] = vlo, vhi
    return x


def mm_zeros():
    x = np.zeros((1, 257), np.float32)
    x[0, ::2] = -0.0
    return x


def mm_ties():
    """16 x 16: the integers 0 .. 254 and nextafter(255, 0).  max - min + 1e-5 rounds to 255.0f, so x / 255 * 255 + 0.5 lands on
    k + 0.5 for every integer k: round half to even, half away and truncation give three different images"""
    x = np.arange(256, dtype=np.float32)
    x[255] = np.nextafter(np.float32(255), np.float32(0))
    return x.reshape(1, 256)


def check_minmax_u8(side, maps, what, ref=REF, zero_keys=False):
    maps = np.ascontiguousarray(maps, dtype=np.float32)
    B, n = maps.shape
    lo, hi = ref.minmax(maps)
    wkeys = np.stack([mm_key(lo), mm_key(hi)], 1)
    want8 = ref.u8(maps[:, None, :])[:, 0]
    sd = _put(side, maps)
    mm = Fenced(side, 2 * B, np.uint32, KEY_MARK)
    u8 = Fenced(side, B * n, np.uint8, U8_MARK)
    side.call("vinet_minmax", sd.data_ptr(), B, n, mm.ptr)
    side.call("vinet_normalize_u8", sd.data_ptr(), mm.ptr, B, n, u8.ptr)
    keys = mm.read(what + " keys").reshape(B, 2)
    if zero_keys:            # minNum(-0, +0) may be either zero (module docstring)
        assert not mm_unkey(keys).any() and not mm_unkey(wkeys).any(), what + ": the extremes of a map of zeros are not zero"
    else:
        assert np.array_equal(keys, wkeys), "%s: keys %r, expected %r" % (what, mm_unkey(keys), mm_unkey(wkeys))
    got8 = u8.read(what + " bytes").reshape(B, n)
    assert np.array_equal(got8, want8), "%s: %d of %d bytes differ" % (what, int((got8 != want8).sum()), want8.size)
    return dict(bits=want8.size + (0 if zero_keys else wkeys.size))


# =====================================================================================================================
# 6. refusals: argument checks that return before any device call, so they are asked of the real library on both machines
# =====================================================================================================================
def check_refusals(lib, put):
    f = put(torch.zeros(64))
    b = put(torch.zeros(256, dtype=torch.uint8))
    k = put(torch.zeros(8, dtype=torch.int32))
    ws = put(torch.zeros(1 << 16, dtype=torch.uint8))
    ms = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    F, Bp, K, WS = f.data_ptr(), b.data_ptr(), k.data_ptr(), ws.data_ptr()
    assert WS % 16 == 0
    BIG_B, BIG_OH = 65536, 32 * 65535 + 1
    calls = []

    def refused(fn, *args):
        calls.append(fn)
        rc = getattr(lib, fn)(*args, 0)
        assert rc < 0, "%s%r was not refused (rc = %d)" % (fn, args, rc)
        assert lib.vinet_last_error(), fn + ": refused without a message"

    # null pointers
    refused("vinet_frames_preprocess", None, 1, 4, 4, F, 2, 2, ms, WS)
    refused("vinet_frames_preprocess", Bp, 1, 4, 4, None, 2, 2, ms, WS)
    refused("vinet_frames_preprocess", Bp, 1, 4, 4, F, 2, 2, None, WS)
    refused("vinet_frames_preprocess", Bp, 1, 4, 4, F, 2, 2, ms, None)
    refused("vinet_gt_preprocess", None, 1, 4, 4, F, 2, 2, WS)
    refused("vinet_gt_preprocess", Bp, 1, 4, 4, None, 2, 2, WS)
    refused("vinet_gt_preprocess", Bp, 1, 4, 4, F, 2, 2, None)
    refused("vinet_audio_excerpt", None, 16, 0, 3, F, 8)
    refused("vinet_audio_excerpt", F, 16, 0, 3, None, 8)
    refused("vinet_resize_blur", None, 1, 4, 4, F, 4, 4, None)
    refused("vinet_resize_blur", F, 1, 4, 4, None, 4, 4, None)
    refused("vinet_minmax", None, 1, 16, K)
    refused("vinet_minmax", F, 1, 16, None)
    refused("vinet_normalize_u8", None, K, 1, 16, Bp)
    refused("vinet_normalize_u8", F, None, 1, 16, Bp)
    refused("vinet_normalize_u8", F, K, 1, 16, None)
    # zero and negative extents
    for bad in (0, -1):
        for at in range(5):
            dims = [1, 4, 4, 2, 2]
            dims[at] = bad
            N, H, W, oh, ow = dims
            refused("vinet_frames_preprocess", Bp, N, H, W, F, oh, ow, ms, WS)
            refused("vinet_gt_preprocess", Bp, N, H, W, F, oh, ow, WS)
            refused("vinet_resize_blur", F, N, H, W, F, oh, ow, None)
        refused("vinet_minmax", F, bad, 16, K)
        refused("vinet_minmax", F, 1, bad, K)
        refused("vinet_normalize_u8", F, K, bad, 16, Bp)
        refused("vinet_normalize_u8", F, K, 1, bad, Bp)
    # more maps than a grid dimension holds; more tile rows than one holds.  (vinet_frames_preprocess has no such limit: its
    # frames are part of a linear grid, so N = 65536 is a legitimate call and not in this list.)
    refused("vinet_gt_preprocess", Bp, BIG_B, 1, 1, F, 1, 1, WS)
    refused("vinet_resize_blur", F, BIG_B, 1, 1, F, 1, 1, None)
    refused("vinet_minmax", F, BIG_B, 1, K)
    refused("vinet_normalize_u8", F, K, BIG_B, 1, Bp)
    refused("vinet_resize_blur", F, 1, 4, 4, F, BIG_OH, 1, None)
    # scratch off the 16-byte grid
    refused("vinet_frames_preprocess", Bp, 1, 4, 4, F, 2, 2, ms, WS + 8)
    refused("vinet_gt_preprocess", Bp, 1, 4, 4, F, 2, 2, WS + 8)
    # audio
    refused("vinet_audio_excerpt", F, 16, -1, 3, F, 8)            # start < 0
    refused("vinet_audio_excerpt", F, 16, 0, 3, F, 0)             # win = 0
    refused("vinet_audio_excerpt", F, -1, 0, 3, F, 8)             # n_samples < 0
    refused("vinet_audio_excerpt", F, 64, 0, 8, F, 8)             # nine samples into a window of eight
    assert b"longer than the window" in lib.vinet_last_error()
    # the scratch queries
    for at in range(5):
        dims = [1, 4, 4, 2, 2]
        dims[at] = 0
        assert lib.vinet_frames_preprocess_ws_bytes(*dims) == -1
    for at in range(3):
        dims = [1, 2, 2]
        dims[at] = 0
        assert lib.vinet_gt_preprocess_ws_bytes(*dims) == -1
    assert lib.vinet_frames_preprocess_ws_bytes(1, 4, 4, 2, 2) > 0 and lib.vinet_gt_preprocess_ws_bytes(1, 2, 2) > 0
    # nothing was written
    assert not bool(f.cpu().any()) and not bool(b.cpu().any()) and not bool(k.cpu().any()) and not bool(ws.cpu().any())
    return len(calls)


# =====================================================================================================================
# 8. the Python surface: single items and non-contiguous views against the batched contiguous call
# =====================================================================================================================
def check_python_surface(dev):
    from vinet_amd import preprocess as PR
    from vinet_amd import utils as U
    dev = torch.device(dev)
    eq = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())       # noqa: E731
    bits = 0
    # frames: [N, H, W, 3] batched; one [H, W, 3]; a cropped (non-contiguous) slice
    fr = torch.from_numpy(make_image("three_frames", "random")).to(dev)
    full = PR.frames_to_tensor(fr, (20, 31))
    want = REF.to_tensor(frame_case("three_frames", "random")[1], *NORMS[0][1:])
    assert np.array_equal(full.cpu().numpy(), want)
    assert eq(PR.frames_to_tensor(fr[1], (20, 31)), full[1])
    wide = torch.zeros((3, 40, 60, 3), dtype=torch.uint8, device=dev)
    wide[:, 2:39, 5:58] = fr
    view = wide[:, 2:39, 5:58]
    assert not view.is_contiguous() and eq(PR.frames_to_tensor(view, (20, 31)), full)
    chan = fr.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)      # the same frames held planar in memory
    assert not chan.is_contiguous() and eq(PR.frames_to_tensor(chan, (20, 31)), full)
    bits += 3 * full.numel() + full[1].numel()
    # ground truth
    g = torch.from_numpy(GT_CASES["mixed4"][0]()).to(dev)
    for size in ((28, 48), None):
        gfull = PR.gt_to_tensor(g, size)
        assert np.array_equal(gfull.cpu().numpy(), Q.gt_preprocess(g.cpu().numpy(), *(size or (None, None))))
        for i in range(4):          # one map at a time: the decision is the map's own
            assert eq(PR.gt_to_tensor(g[i], size), gfull[i])
        gw = torch.full((4, 50, 90), 255, dtype=torch.uint8, device=dev)
        gw[:, 3:48, 4:84] = g
        gv = gw[:, 3:48, 4:84]
        assert not gv.is_contiguous() and eq(PR.gt_to_tensor(gv, size), gfull)
        bits += 3 * gfull.numel()
    # audio: [L] and [1, L]
    wav = torch.from_numpy(audio_wave(2000)).to(dev)
    a = PR.audio_excerpt(wav, 100, 300, 257)
    assert eq(PR.audio_excerpt(wav.view(1, -1), 100, 300, 257), a)
    stereo = torch.stack([wav, -wav], 1)                  # [L, 2]: one channel is a view of stride 2
    assert not stereo[:, 0].is_contiguous() and eq(PR.audio_excerpt(stereo[:, 0], 100, 300, 257), a)
    twice = torch.stack([wav, wav * 0.5], 1).reshape(-1)[::2]
    assert not twice.is_contiguous() and eq(PR.audio_excerpt(twice, 100, 300, 257), a)
    bits += 3 * a.numel()
    # maps: batch, single map, flipped view; with and without the keys; the uint8 wrapper of the harness
    m = torch.from_numpy(rb_source("batch5", "sigmoid")).to(dev)
    out = U.resize_blur(m, (20, 31))
    out_k, keys = U.resize_blur(m, (20, 31), return_minmax=True)
    assert np.array_equal(out.cpu().numpy(), P.resize_blur(m.cpu().numpy(), 20, 31)) and eq(out, out_k)
    assert eq(U.resize_blur(m[2], (20, 31)), out[2])
    one, k1 = U.resize_blur(m[2], (20, 31), return_minmax=True)
    assert eq(one, out[2]) and torch.equal(k1.cpu()[0], keys.cpu()[2])
    crop = torch.zeros((5, 12, 15), device=dev)
    crop[:, 2:9, 3:12] = m
    cv = crop[:, 2:9, 3:12]
    assert not cv.is_contiguous() and eq(U.resize_blur(cv, (20, 31)), out)
    u8 = U.postprocess(m, (20, 31))
    assert np.array_equal(u8.cpu().numpy(), P.normalize_u8(P.resize_blur(m.cpu().numpy(), 20, 31)))
    assert eq(U.postprocess(m[2], (20, 31)), u8[2]) and eq(U.postprocess(cv, (20, 31)), u8)
    assert eq(U.to_uint8(out), u8) and eq(U.to_uint8(out, keys), u8) and eq(U.to_uint8(out[2]), u8[2])
    ov = out.transpose(1, 2).contiguous().transpose(1, 2)   # the same maps, column-major in memory
    assert not ov.is_contiguous() and eq(U.to_uint8(ov), u8)
    bits += 5 * out.numel() + 4 * u8.numel()
    return dict(bits=bits)
