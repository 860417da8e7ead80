"""The arithmetic modes of the token encoder's ATTENTION (include/vinet_hip.h, the `attn` argument; csrc/tk_attn_bf16.h): a numpy /
torch statement of the seven products in a mode, exact-case builders and the encoder emulation, shared by
tests/test_token_attn_host.py and tests/test_gpu_token_attn.py.  Nothing here calls the library.

    product             A operand                         B operand   k axis
    scores = A B^T      q qscale (scaled in fp32, split)  k           D
    AO     = A B        p m                               v           keys
    dP     = A B^T      dAO                               v           D
    dQ     = A B        dS                                k           keys
    dV     = A^T B      P m                               dAO         queries
    dK     = A^T B      dS                                q           queries
A mode sums the terms of tests/token_mma_cases.terms_np over k.  Softmax (maximum, expf, sum, normalisation), dS = P (dP m - dot)
qscale, dot = rowsum(dAO AO) and the saved P are fp32 in every mode.

Exactness of the builders.  Every operand of a multi-term sum is a dyadic number whose split is known by construction
((512 + n) 2^e, n in {-1, 0, 1}: hi = 512 2^e, lo = n 2^e; a power of two: lo = 0), and `_room` asserts in int64 that
sum_k |a_k| |b_k|, scaled to integers, stays below 2^24: every partial sum of every mode's terms is then an fp32 integer multiple
of one unit, in ANY order and grouping.  Sums that meet a value with a full significand (a product with a qscale that is no
power of two) have at most ONE nonzero product whose other factor is a power of two: the mode's terms hi 2^e + lo 2^e are then
both representable with their sum (`_single`)."""
import math

import numpy as np
import torch

from tests import token_mma_cases as TC
from tests import transformer_model as TM

MODES = TC.MODES
F32, F64 = np.float32, np.float64
WAVE_ROWS, ROW_TILE, KEY_TILE_FWD, TILE_BWD = 16, 64, 64, 32      # csrc/tk_attn_bf16.h as built
EDGE_S = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
HEADS = {4: 4, 12: 4, 16: 2, 32: 2, 64: 2, 80: 2, 128: 2}          # head width -> heads (E = H D is a multiple of 16, <= 512)
POW2_D = (16, 64)                                                 # qscale = 1 / sqrt(D) is a power of two
ANY_D = (4, 12, 32, 80, 128)
NB = 3


def sp_of(S):
    return (S + 15) & ~15


def qscale_of(D):
    return F32(1.0) / np.sqrt(F32(D))          # 1.f / sqrtf((float)D)


def mm_np(mode, A, B):
    """float64 sum over k of the mode's terms; A [..., M, K], B [..., K, N] float32"""
    return sum(a.astype(F64) @ b.astype(F64) for a, b in TC.terms_np(mode, np.asarray(A, F32), np.asarray(B, F32)))


# ---- one attention stage, per head arrays [B, H, S, D] / [B, H, S, S] -----------------------------------------------------------
def forward_np(mode, q, k, v, qs):
    """(P float32, AO float64, scores float64).  The softmax is fp32: maximum, exp, sum, 1 / sum, product"""
    s64 = mm_np(mode, (q * F32(qs)).astype(F32), np.swapaxes(k, -1, -2))
    s = s64.astype(F32)
    e = np.exp((s - s.max(-1, keepdims=True)).astype(F32)).astype(F32)
    P = (e * (F32(1.0) / e.sum(-1, keepdims=True, dtype=F32))).astype(F32)
    return P, mm_np(mode, P, v), s64


def backward_np(mode, q, k, v, P, dao, ao, qs):
    """dict(dot float32 [B, H, S], dq, dk, dv float64, ds float32) from caller-supplied P and ao (no dropout: m = 1)"""
    dot = (dao.astype(F64) * ao.astype(F64)).sum(-1).astype(F32)
    dp64 = mm_np(mode, dao, np.swapaxes(v, -1, -2))
    dp = dp64.astype(F32)
    ds = ((P * (dp - dot[..., None]).astype(F32)).astype(F32) * F32(qs)).astype(F32)
    return dict(dot=dot, dp=dp64, ds=ds, dq=mm_np(mode, ds, k), dv=mm_np(mode, np.swapaxes(P, -1, -2), dao),
                dk=mm_np(mode, np.swapaxes(ds, -1, -2), q))


# ---- the workspace's row layout -------------------------------------------------------------------------------------------------
def pack_rows(x, fill):
    """[B, H, S, D] -> [B Sp, H D] float32, `fill` in the padding rows"""
    B, H, S, D = x.shape
    out = np.full((B, sp_of(S), H * D), fill, F32)
    out[:, :S] = np.transpose(x, (0, 2, 1, 3)).reshape(B, S, H * D)
    return out.reshape(B * sp_of(S), H * D)


def pack_qkv(q, k, v, fill=np.nan):
    return np.ascontiguousarray(np.concatenate([pack_rows(t, fill) for t in (q, k, v)], axis=1))


def unpack_rows(m, B, H, S, D):
    """[B Sp, H D] -> ([B, H, S, D], the padding rows [B, Sp - S, H D])"""
    m = m.reshape(B, sp_of(S), H * D)
    return np.transpose(m[:, :S].reshape(B, S, H, D), (0, 2, 1, 3)), m[:, S:]


# ---- the checks of the module docstring -------------------------------------------------------------------------------------------
def _grid(a):
    """(|hi| + |lo| in units, unit): the largest power of two that a, hi(a) and lo(a) are all integer multiples of"""
    a = np.asarray(a, F32)
    hi, lo = TC.split_np(a)
    parts = [x.astype(F64) for x in (a, hi, lo)]
    for e in range(12, -41, -1):
        if all(np.array_equal(x / 2.0 ** e, np.round(x / 2.0 ** e)) for x in parts):
            return ((np.abs(parts[1]) + np.abs(parts[2])) / 2.0 ** e).astype(np.int64), 2.0 ** e
    raise AssertionError("operand is not a short dyadic number")


def _room(A, B, what):
    """A [..., M, K] @ B [..., K, N]: every term of every mode is an integer multiple of one unit, and sum_k (|hi_a| + |lo_a|)
    (|hi_b| + |lo_b|), which bounds every partial sum of every mode in any order, stays inside fp32's exact integers"""
    ia, _ = _grid(A)
    ib, _ = _grid(B)
    room = int((ia @ ib).max()) if ia.size and ib.size else 0
    assert room < 2 ** 24, "%s: partial sums may leave fp32's exact integers: %d" % (what, room)
    return room


def _single(A, B, what):
    """every sum of A @ B has at most one nonzero product, and B's nonzero elements are powers of two (lo = 0)"""
    nzp = (np.asarray(A) != 0).astype(np.int64) @ (np.asarray(B) != 0).astype(np.int64)
    assert int(nzp.max()) <= 1, "%s: %d nonzero products in one sum" % (what, int(nzp.max()))
    b = np.abs(np.asarray(B, F64)[np.asarray(B) != 0])
    assert np.array_equal(np.log2(b), np.round(np.log2(b))), "%s: the lone factor is not a power of two" % what


def _draw(rng, shape, keep, scale=1.0):
    """s (512 + n) scale with s = +-1, n in {-1, 0, 1}, thinned to `keep`; the split is asserted to be the constructed one"""
    n, s, z = rng.integers(-1, 2, shape), rng.integers(0, 2, shape) * 2 - 1, rng.random(shape) < keep
    a = (s * (512 + n) * z * scale).astype(F32)
    hi, lo = TC.split_np(a)
    assert np.array_equal(hi, (s * 512 * z * scale).astype(F32)) and np.array_equal(lo, (s * n * z * scale).astype(F32)), "the split is not the constructed one"
    return a


def _thin(n):
    return 1.0 if n <= 30 else (30.0 / n) ** 0.5


def edge_rows(S, count):
    """`count` different rows of [0, S) at the edges of the 16-row wave tiles and the 64-key tiles"""
    want = [S - 1, 0, 15, 16, 63, 64, 31, 32, 127, 128] + list(range(1, S))
    rows = []
    for r in want:
        if 0 <= r < S and r not in rows:
            rows.append(r)
    assert len(rows) >= count, (S, count)
    return rows[:count]


# ---- exact case 1: scores and AO, the construction with a power-of-two qscale -----------------------------------------------------
def exact_scores_case(S, D, seed):
    """every query row [a c, c, c, c, 0...] with a = 1 + 2^-9, c = 2^28; key A = a e0, key B = (1 + 2^-8) e1, keys C, C' = e2, e3, the
    rest 0.  F32: A wins alone (a^2 > 1 + 2^-8); BF16X3: a^2 loses its lo lo = 2^-18 and ties with B; BF16: a and 1 + 2^-8 round
    to 1, four keys tie.  exp of the gaps is exactly 0, so P is one-hot / 1/2, 1/2 / four times 1/4, and AO follows with V = +-(512 + n)"""
    assert D in POW2_D and S >= 4
    H, B = HEADS[D], NB
    rng = np.random.default_rng(seed)
    a, c, qs = F32(1 + 2.0 ** -9), F32(2.0 ** 28), qscale_of(D)
    assert float(qs) == 2.0 ** round(math.log2(float(qs)))
    q = np.zeros((B, H, S, D), F32)
    q[..., 0], q[..., 1], q[..., 2], q[..., 3] = a * c, c, c, c
    k = np.zeros((B, H, S, D), F32)
    rows = {}
    for b in range(B):
        for h in range(H):
            r = edge_rows(S, 4)
            r = r[(b + h) % 4:] + r[:(b + h) % 4]          # the roles move over the edge rows from clip to clip and head to head
            rows[(b, h)] = r
            k[b, h, r[0], 0], k[b, h, r[1], 1], k[b, h, r[2], 2], k[b, h, r[3], 3] = a, F32(1 + 2.0 ** -8), 1.0, 1.0
    v = _draw(rng, (B, H, S, D), 1.0)
    want = {}
    for mode in MODES:
        nzp = (q != 0).astype(np.int64) @ (np.swapaxes(k, -1, -2) != 0).astype(np.int64)
        assert int(nzp.max()) == 1, "a score is one product"
        P, ao, s64 = forward_np(mode, q, k, v, qs)
        assert np.array_equal(s64.astype(F32).astype(F64), s64), "a score is not an fp32 number"
        top = np.sort(np.unique(s64))[::-1]
        assert top[0] - top[1] >= 128.0, "exp of the gap under the top score is not exactly 0"
        for (b, h), r in rows.items():
            on = {"fp32": r[:1], "bf16x3": r[:2], "bf16": r[:4]}[mode]
            row = np.zeros(S, F32)
            row[on] = 1.0 / len(on)
            assert np.array_equal(P[b, h], np.broadcast_to(row, (S, S))), (mode, b, h)
        _room(P, v, "AO")
        want[mode] = dict(P=P, ao=ao)
    return dict(q=q, k=k, v=v, qs=qs, want=want, B=B, H=H, S=S, D=D)


# ---- exact case 2: scores all equal, any head width -------------------------------------------------------------------------------
def exact_flat_case(S, D, seed):
    """q = c e0; keys that are ON have k = 0 (score exactly 0 in every mode, whatever qscale is), the others k = -e0 (score about
    -2^28 qscale: exp is exactly 0).  1, 2 or 4 keys are on at edge rows, so P = 1 / on there and AO = (sum of their v) / on"""
    H, B = HEADS[D], NB
    rng = np.random.default_rng(seed)
    qs = qscale_of(D)
    n_on = 4 if S >= 4 else (2 if S >= 2 else 1)
    q = np.zeros((B, H, S, D), F32)
    q[..., 0] = 2.0 ** 28
    k = np.zeros((B, H, S, D), F32)
    k[..., 0] = -1.0
    rows = {}
    for b in range(B):
        for h in range(H):
            r = edge_rows(S, min(S, 8))
            r = [r[(i + b + 2 * h) % len(r)] for i in range(n_on)]
            assert len(set(r)) == n_on
            rows[(b, h)] = r
            k[b, h, r, 0] = 0.0
    v = _draw(rng, (B, H, S, D), 1.0)
    want = {}
    for mode in MODES:
        _single(q * qs, np.swapaxes(k, -1, -2), "scores")
        P, ao, s64 = forward_np(mode, q, k, v, qs)
        assert float(s64.max()) == 0.0 and (s64.size == (s64 == 0).sum() or float(s64[s64 != 0].max()) < -128.0)
        for (b, h), r in rows.items():
            row = np.zeros(S, F32)
            row[r] = 1.0 / n_on
            assert np.array_equal(P[b, h], np.broadcast_to(row, (S, S))), (mode, b, h)
        _room(P, v, "AO")
        want[mode] = dict(P=P, ao=ao)
    return dict(q=q, k=k, v=v, qs=qs, want=want, B=B, H=H, S=S, D=D)


# ---- exact case 3: dQ, dK, dV from a known dS (power-of-two qscale) ------------------------------------------------------------------
def exact_ds_case(S, D, seed):
    """V = 0, so dP = 0; dAO = +-(512 + n) with one element per row forced to +-512 where AO = -+2^2, so dot = -2^11 exactly (one
    product) and dS = P 2^11 qscale with P = (512 + n) 2^-12: a known split.  Q, K = +-(512 + n), thinned like the operands of
    tests/token_mma_cases.exact_operands.  dQ = dS K, dK = dS^T Q and dV = P^T dAO are sums of many exact terms"""
    assert D in POW2_D
    H, B = HEADS[D], NB
    rng = np.random.default_rng(seed)
    qs = qscale_of(D)
    keep = _thin(S)
    q, k = _draw(rng, (B, H, S, D), keep), _draw(rng, (B, H, S, D), keep)
    v = np.zeros((B, H, S, D), F32)
    P = _draw(rng, (B, H, S, S), keep, 2.0 ** -12)
    dao = _draw(rng, (B, H, S, D), keep)
    ao = np.zeros((B, H, S, D), F32)
    d0 = rng.integers(0, D, (B, H, S))
    sg = (rng.integers(0, 2, (B, H, S)) * 2 - 1).astype(F32)
    np.put_along_axis(dao, d0[..., None], (512 * sg)[..., None], -1)
    np.put_along_axis(ao, d0[..., None], (-4.0 * sg)[..., None], -1)
    want = {}
    for mode in MODES:
        w = backward_np(mode, q, k, v, P, dao, ao, qs)
        assert np.all(w["dot"] == -2048.0) and not w["dp"].any()
        assert np.array_equal(w["ds"], (P * F32(2048.0) * qs).astype(F32))
        _room(w["ds"], k, "dQ")
        _room(np.swapaxes(w["ds"], -1, -2), q, "dK")
        _room(np.swapaxes(P, -1, -2), dao, "dV")
        want[mode] = w
    return dict(q=q, k=k, v=v, P=P, dao=dao, ao=ao, qs=qs, want=want, B=B, H=H, S=S, D=D)


# ---- exact case 4: dP seen through split(dS), any head width -------------------------------------------------------------------------
def exact_dp_case(S, D, seed):
    """P = powers of two; V, dAO = +-(512 + n), thinned over D; AO = 0, so dot = 0 and dS = fl(fl(P dP) qscale): one rounding, the
    same in numpy.  Q and K hold ONE nonzero element (a power of two) per clip and head, so every dK and dQ element is one product
    dS 2^e: it shows dP through the split of dS.  dV = P^T dAO is a sum of many exact terms"""
    H, B = HEADS[D], NB
    rng = np.random.default_rng(seed)
    qs = qscale_of(D)
    P = (np.exp2(-rng.integers(1, 4, (B, H, S, S))) * (rng.random((B, H, S, S)) < _thin(S))).astype(F32)
    v, dao = _draw(rng, (B, H, S, D), _thin(D)), _draw(rng, (B, H, S, D), _thin(D))
    ao = np.zeros((B, H, S, D), F32)
    q, k = np.zeros((B, H, S, D), F32), np.zeros((B, H, S, D), F32)
    for b in range(B):
        for h in range(H):
            r = edge_rows(S, min(S, 4))
            q[b, h, r[(b + h) % len(r)], (3 * b + h) % D] = 8.0
            k[b, h, r[(b + h + 1) % len(r)], (5 * b + 2 * h + 1) % D] = 4.0
    want = {}
    for mode in MODES:
        _room(dao, np.swapaxes(v, -1, -2), "dP")
        w = backward_np(mode, q, k, v, P, dao, ao, qs)
        assert not w["dot"].any()
        pdp = P.astype(F64) * w["dp"]
        assert np.array_equal(pdp.astype(F32).astype(F64), pdp), "P dP is not an fp32 number"
        _single(w["ds"], k, "dQ")
        _single(np.swapaxes(w["ds"], -1, -2), q, "dK")
        _room(np.swapaxes(P, -1, -2), dao, "dV")
        want[mode] = w
    return dict(q=q, k=k, v=v, P=P, dao=dao, ao=ao, qs=qs, want=want, B=B, H=H, S=S, D=D)


# the cases the GPU test runs (tests/test_token_attn_host.py runs the builders' own assertions on every one of them)
SCORES_CASES = [(S, D) for D in POW2_D for S in (21, 65, 129)]
FLAT_CASES = [(S, D) for D in ANY_D for S in (1, 17, 65)] + [(S, 16) for S in EDGE_S]
DS_CASES = [(S, D) for D in POW2_D for S in EDGE_S]
DP_CASES = [(S, D) for D in ANY_D for S in (1, 17, 33, 65)] + [(S, 64) for S in (31, 129)]


def case_seed(kind, S, D):
    return 7000 + 1000 * kind + 8 * S + D


# ---- the whole encoder: linears in mode `mma`, attention (forward and autograd backward) in mode `attn` ----------------------------
class _ModeAttention(torch.autograd.Function):
    """softmax(q qscale k^T) (x keep mask / (1 - p)) v per head with the seven products in the mode's terms; everything else in the
    tensors' dtype, as the kernels keep it in fp32.  rowsum(dP P) is taken as rowsum(dAO AO), as in the kernels"""

    @staticmethod
    def forward(ctx, q, k, v, keep, mode, qs):
        att = torch.softmax(TC.mm_mode(mode, q * qs, k.transpose(-1, -2)), dim=-1)
        am = att if keep is None else att * keep
        ao = TC.mm_mode(mode, am, v)
        ctx.save_for_backward(q, k, v, att, ao)
        ctx.keep, ctx.mode, ctx.qs = keep, mode, qs
        return ao

    @staticmethod
    def backward(ctx, dao):
        q, k, v, att, ao = ctx.saved_tensors
        mode, keep, qs = ctx.mode, ctx.keep, ctx.qs
        dp = TC.mm_mode(mode, dao, v.transpose(-1, -2))
        if keep is not None:
            dp = dp * keep
        am = att if keep is None else att * keep
        ds = att * (dp - (dao * ao).sum(-1, keepdim=True)) * qs
        return (TC.mm_mode(mode, ds, k), TC.mm_mode(mode, ds.transpose(-1, -2), q), TC.mm_mode(mode, am.transpose(-1, -2), dao), None, None, None)


def encoder_layer_modes(x, P, nhead, mma, attn, p=0.0, masks=None, eps=1e-5):
    """tests/token_mma_cases.encoder_layer_mode with attention through _ModeAttention"""
    S, B, Efeat = x.shape
    D = Efeat // nhead
    m = masks if masks is not None else (None,) * 4
    lin = lambda t, w, b: TC._ModeLinear.apply(t, P[w], P[b], mma)
    xb = x.transpose(0, 1)
    qkv = lin(xb, "self_attn.in_proj_weight", "self_attn.in_proj_bias")
    q, k, v = (t.reshape(B, S, nhead, D).transpose(1, 2) for t in qkv.split(Efeat, dim=-1))
    if attn == "fp32":
        att = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D), dim=-1)
        ao = TM._drop(att, m[0], p) @ v
    else:
        keep = None if (m[0] is None or p == 0) else m[0].to(x.dtype) / (1.0 - p)
        ao = _ModeAttention.apply(q, k, v, keep, attn, 1.0 / math.sqrt(D))
    ao = ao.transpose(1, 2).reshape(B, S, Efeat)
    proj = lin(ao, "self_attn.out_proj.weight", "self_attn.out_proj.bias")
    x1 = TM.layer_norm(xb + TM._drop(proj, m[1], p), P["norm1.weight"], P["norm1.bias"], eps)
    h = TM._drop(torch.relu(lin(x1, "linear1.weight", "linear1.bias")), m[2], p)
    o = lin(h, "linear2.weight", "linear2.bias")
    x2 = TM.layer_norm(x1 + TM._drop(o, m[3], p), P["norm2.weight"], P["norm2.bias"], eps)
    return x2.transpose(0, 1)


def torch_run_modes(sd, x, proj, mma, attn, dtype=torch.float32, p=0.0, masks=None, nhead=2, n_layers=2):
    """forward + backward of the encoder with linears in `mma` and attention in `attn`; tensors keyed like
    tests.token_mma_cases.torch_run_mode (which it equals, operation for operation, at attn = "fp32")"""
    layers = TM.layers_from_state_dict(sd, "transformer_encoder.", n_layers, dtype)
    for P in layers:
        for t in P.values():
            t.requires_grad_(True)
    xg = x.to(dtype).clone().requires_grad_(True)
    y = xg + sd["pos_encoder.pe"].to(dtype)
    for i, P in enumerate(layers):
        y = encoder_layer_modes(y, P, nhead, mma, attn, p, None if masks is None else masks[i])
    (y * proj.to(dtype)).sum().backward()
    got = {"train_y": y.detach(), "train_gx": xg.grad}
    for i, P in enumerate(layers):
        for k, t in P.items():
            got["train_g:transformer_encoder.layers.%d.%s" % (i, k)] = t.grad
    return got
