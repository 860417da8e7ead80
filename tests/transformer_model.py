"""Plain-torch statement of the transformer fusion's encoder (post-norm nn.TransformerEncoderLayer semantics: ReLU, LayerNorm
eps 1e-5, dropout at the attention weights, after the attention projection, between the two linears and after the second),
with explicit matmuls and softmax, optional keep masks, in whatever dtype its inputs have (fp32 or fp64).  The comparator of
tests/test_transformer_host.py (pinned to the reference's recording there) and tests/test_gpu_transformer.py."""
import math

import torch

LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
              "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _drop(x, mask, p):
    """mask: keep mask of x's shape (0 / 1) or None"""
    if mask is None or p == 0:
        return x
    return x * mask.to(x.dtype) / (1.0 - p)


def encoder_layer(x, P, nhead, p=0.0, masks=None, eps=1e-5):
    """x [S, B, E]; P: dict of the twelve LAYER_KEYS tensors; masks: None or (attn [B,H,S,S], proj [B,S,E], hidden [B,S,F],
    out [B,S,E]) keep masks.  Returns [S, B, E]."""
    S, B, Efeat = x.shape
    D = Efeat // nhead
    m = masks if masks is not None else (None,) * 4
    xb = x.transpose(0, 1)                                                    # [B, S, E]
    qkv = xb @ P["self_attn.in_proj_weight"].t() + P["self_attn.in_proj_bias"]
    q, k, v = (t.reshape(B, S, nhead, D).transpose(1, 2) for t in qkv.split(Efeat, dim=-1))      # [B, H, S, D]
    att = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(D), dim=-1)
    att = _drop(att, m[0], p)
    ao = (att @ v).transpose(1, 2).reshape(B, S, Efeat)
    proj = ao @ P["self_attn.out_proj.weight"].t() + P["self_attn.out_proj.bias"]
    x1 = layer_norm(xb + _drop(proj, m[1], p), P["norm1.weight"], P["norm1.bias"], eps)
    h = _drop(torch.relu(x1 @ P["linear1.weight"].t() + P["linear1.bias"]), m[2], p)
    o = h @ P["linear2.weight"].t() + P["linear2.bias"]
    x2 = layer_norm(x1 + _drop(o, m[3], p), P["norm2.weight"], P["norm2.bias"], eps)
    return x2.transpose(0, 1)


def encoder(x, pe, layers, nhead, p=0.0, masks=None, eps=1e-5):
    """x [S, B, E] + pe [S, 1, E], then the layers (list of dicts); masks: None or one 4-tuple per layer"""
    y = x + pe
    for i, P in enumerate(layers):
        y = encoder_layer(y, P, nhead, p, None if masks is None else masks[i], eps)
    return y


def split_masks(flat, n_layers, B, S, Efeat, F, H):
    """the byte buffer the kernels export (include/vinet_hip.h: per layer [B][H][S][S] | [B S][E] | [B S][F] | [B S][E])"""
    out, o = [], 0
    for _ in range(n_layers):
        sizes = (B * H * S * S, B * S * Efeat, B * S * F, B * S * Efeat)
        shapes = ((B, H, S, S), (B, S, Efeat), (B, S, F), (B, S, Efeat))
        ms = []
        for n, sh in zip(sizes, shapes):
            ms.append(flat[o:o + n].reshape(sh))
            o += n
        out.append(tuple(ms))
    assert o == flat.numel()
    return out


def layers_from_state_dict(sd, prefix, n_layers, dtype=None):
    return [{k: (sd["%slayers.%d.%s" % (prefix, i, k)] if dtype is None else sd["%slayers.%d.%s" % (prefix, i, k)].to(dtype)) for k in LAYER_KEYS}
            for i in range(n_layers)]
