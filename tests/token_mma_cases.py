"""Cases, operand generators and a torch / numpy statement of the token encoder's two bf16 arithmetic forms
(include/vinet_hip.h: VINET_TK_MMA_BF16X3 and VINET_TK_MMA_BF16), shared by tests/test_token_mma_host.py and
tests/test_gpu_token_mma.py.  Nothing here calls the library.

The split:  hi(a) = bf16(a), round to nearest even;  lo(a) = bf16(a - hi(a)).
The terms of one product sum_k a b:
    F32      a b
    BF16X3   hi_a hi_b + hi_a lo_b + lo_a hi_b          ( = a b - lo_a lo_b wherever hi + lo == a )
    BF16     hi_a hi_b

Exact operands.  a = s (512 + n) with s = +-1 and n in {-1, 0, 1}, or a = 0.  |a| lies in [512, 1024), where bf16's 8
significant bits step by 4, so hi = 512 s and lo = s n BY CONSTRUCTION (split_np is asserted to agree).  A product |a b| is at
most 513^2 < 2^18.01, an integer, and every term of every mode is an integer too.  fp32 adds integers exactly, in ANY order
and grouping (the MFMA's internal order is not documented), as long as every partial sum stays below 2^24 in magnitude; the
generator guarantees the stronger sum_k |a_k| |b_k| + |bias| + |res| + |C| < 2^24 and asserts it in int64.  A wider family
(more significant bits in hi, as 256 m + n with 8 <= |m| <= 15) leaves room for ONE product below 2^24, so it cannot serve
K > 1; with 10-bit operands 63 nonzero products fit, and for K above 48 the operands are thinned with zeros (each element
kept with probability sqrt(30 / K), about 30 nonzero products per sum) instead of shrunk: the nonzero ones still exercise hi and lo, the zeros
fall at other places in every row and column, so every k position of the tile is read with a value somewhere."""
import numpy as np
import torch

from tests import transformer_model as TM

MODES = {"fp32": 0, "bf16x3": 1, "bf16": 2}          # name -> VINET_TK_MMA_*
FORMS = (0, 1, 2)                                    # A[m][k] B[n][k] | A[m][k] B[k][n] | A[k][m] B[k][n]
EPIS = (0, 1, 2, 3, 4)                               # plain | + bias | relu(. + bias) | + res | C +=
TILE_N, TILE_M, TILE_M_TALL, TALL_FROM = 64, 64, 128, 4096     # csrc/tk_gemm_bf16.h as built
SLICE = 512                                          # rows of a weight-gradient slice (TF_WGRAD_CHUNK)

# (M, N, K): every M and N of {4, 12, 60, 64, 68, one tile, one tile + 4} for both tile heights (the 128-row tile serves
# M >= 4096), every K of {16, 32, 48, 80, 256}; each value at least once, sizes crossed so that small meets large
SHAPES = [(4, 68, 16), (12, 4, 32), (60, 132, 48), (64, 12, 80), (68, 60, 256), (128, 64, 16), (132, 128, 80),
          (TALL_FROM, 4, 48), (TALL_FROM + 4, 68, 32), (TALL_FROM + TILE_M_TALL + 4, 12, 16)]
SLICED_SHAPE = (68, 132, SLICE + 16)                 # form 2 only: two slices, 512 + 16 rows


# ---- the split, in numpy (bit operations) and in torch ---------------------------------------------------------------------------
def hi_np(a):
    """bf16(a) as float32, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def split_np(a):
    a = np.asarray(a, dtype=np.float32)
    hi = hi_np(a)
    return hi, hi_np(a - hi)


def terms_np(mode, A, B):
    """[(a part, b part)] whose products the mode sums; A, B float32 arrays"""
    if mode == "fp32":
        return [(A, B)]
    ah, al = split_np(A)
    bh, bl = split_np(B)
    return [(ah, bh)] if mode == "bf16" else [(ah, bh), (ah, bl), (al, bh)]


def split_t(a):
    """torch: (hi, lo) in a's dtype, the roundings taken on the fp32 value"""
    a32 = a.float()
    hi = a32.bfloat16().float()
    lo = (a32 - hi).bfloat16().float()
    return hi.to(a.dtype), lo.to(a.dtype)


def mm_mode(mode, A, B):
    """A @ B as the mode sums it"""
    if mode == "fp32":
        return A @ B
    ah, al = split_t(A)
    bh, bl = split_t(B)
    if mode == "bf16":
        return ah @ bh
    return ah @ bh + ah @ bl + al @ bh


# ---- one product: operands in the memory orientation of a form --------------------------------------------------------------------
def logical(form, A, B):
    """(A as [M][K], B as [K][N]) from the arrays as they lie in memory"""
    return (A.T if form == 2 else A), (B.T if form == 0 else B)


def exact_operands(form, epi, M, N, K, seed):
    """dict(A, B, bias, res, c0 as float32 in memory orientation; want = {mode: float64 [M][N] BEFORE the epilogue's own part}):
    the exact family of the module docstring"""
    rng = np.random.default_rng(seed)
    keep = 1.0 if K <= 48 else (30.0 / K) ** 0.5

    def draw(shape):
        n = rng.integers(-1, 2, shape)
        s = rng.integers(0, 2, shape) * 2 - 1
        z = rng.random(shape) < keep
        return (s * (512 + n) * z).astype(np.int64), (s * 512 * z).astype(np.int64), (s * n * z).astype(np.int64)

    a, ahi, alo = draw((M, K))
    b, bhi, blo = draw((K, N))
    for x, h, l in ((a, ahi, alo), (b, bhi, blo)):
        sh, sl = split_np(x.astype(np.float32))
        assert np.array_equal(sh.astype(np.int64), h) and np.array_equal(sl.astype(np.int64), l), "the split is not the constructed one"
    bias = rng.integers(-100, 101, N).astype(np.int64)
    res = rng.integers(-1000, 1001, (M, N)).astype(np.int64)
    c0 = rng.integers(-1000, 1001, (M, N)).astype(np.int64)
    room = np.abs(a) @ np.abs(b) + np.abs(bias)[None, :] + np.abs(res) + np.abs(c0)
    assert int(room.max()) < 2 ** 24, "partial sums may leave fp32's exact integers: %d" % int(room.max())
    full, lolo, hihi = a @ b, alo @ blo, ahi @ bhi
    want = {"fp32": full, "bf16x3": full - lolo, "bf16": hihi}
    assert np.array_equal(want["bf16x3"], hihi + ahi @ blo + alo @ bhi)
    to_mem = lambda x, t: np.ascontiguousarray((x.T if t else x).astype(np.float32))
    return dict(A=to_mem(a, form == 2), B=to_mem(b, form == 0), bias=bias.astype(np.float32), res=res.astype(np.float32),
                c0=c0.astype(np.float32), want=want)


def epilogue_np(epi, v, bias, res, c0):
    """float64 statement of the five epilogues of vinet_token_gemm"""
    if epi == 1:
        return v + bias[None, :]
    if epi == 2:
        return np.maximum(v + bias[None, :], 0)
    if epi == 3:
        return v + res
    if epi == 4:
        return v + c0
    return v


# ---- the whole encoder in a mode: tests/transformer_model.py's stages around mode-arithmetic linears ------------------------------
class _ModeLinear(torch.autograd.Function):
    """y = x W^T + b with the three products (forward, data gradient, weight gradient) in the mode's terms; the bias gradient is a
    plain sum, as in the kernels"""

    @staticmethod
    def forward(ctx, x, w, b, mode):
        ctx.save_for_backward(x, w)
        ctx.mode = mode
        return mm_mode(mode, x, w.t()) + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
        dx = mm_mode(ctx.mode, dy2, w).reshape(x.shape)
        dw = mm_mode(ctx.mode, dy2.t(), x2)
        return dx, dw, dy2.sum(0), None


def encoder_layer_mode(x, P, nhead, mode, p=0.0, masks=None, eps=1e-5):
    """TM.encoder_layer with its four linears through _ModeLinear; attention, softmax, LayerNorm and dropout are TM's"""
    import math
    S, B, Efeat = x.shape
    D = Efeat // nhead
    m = masks if masks is not None else (None,) * 4
    lin = lambda t, w, b: _ModeLinear.apply(t, P[w], P[b], mode)
    xb = x.transpose(0, 1)
    qkv = lin(xb, "self_attn.in_proj_weight", "self_attn.in_proj_bias")
    q, k, v = (t.reshape(B, S, nhead, D).transpose(1, 2) for t in qkv.split(Efeat, dim=-1))
    att = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D), dim=-1)
    att = TM._drop(att, m[0], p)
    ao = (att @ v).transpose(1, 2).reshape(B, S, Efeat)
    proj = lin(ao, "self_attn.out_proj.weight", "self_attn.out_proj.bias")
    x1 = TM.layer_norm(xb + TM._drop(proj, m[1], p), P["norm1.weight"], P["norm1.bias"], eps)
    h = TM._drop(torch.relu(lin(x1, "linear1.weight", "linear1.bias")), m[2], p)
    o = lin(h, "linear2.weight", "linear2.bias")
    x2 = TM.layer_norm(x1 + TM._drop(o, m[3], p), P["norm2.weight"], P["norm2.bias"], eps)
    return x2.transpose(0, 1)


def torch_run_mode(sd, x, proj, mode, dtype=torch.float32, p=0.0, masks=None, nhead=2, n_layers=2):
    """forward + backward of the mode's encoder; tensors keyed like tests.test_gpu_transformer._torch_run"""
    layers = TM.layers_from_state_dict(sd, "transformer_encoder.", n_layers, dtype)
    for P in layers:
        for t in P.values():
            t.requires_grad_(True)
    xg = x.to(dtype).clone().requires_grad_(True)
    y = xg + sd["pos_encoder.pe"].to(dtype)
    for i, P in enumerate(layers):
        y = encoder_layer_mode(y, P, nhead, mode, p, None if masks is None else masks[i])
    (y * proj.to(dtype)).sum().backward()
    got = {"train_y": y.detach(), "train_gx": xg.grad}
    for i, P in enumerate(layers):
        for k, t in P.items():
            got["train_g:transformer_encoder.layers.%d.%s" % (i, k)] = t.grad
    return got
