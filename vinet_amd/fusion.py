"""AViNet audio-visual fusion: nn.Bilinear(42, 3, 336) over channels
(model.py:230,235-237) and the transformer encoder behind it (model.py:211-221,
239-247) as HIP kernels on channels-last tensors."""
import ctypes as C

import torch

from . import _lib as L
from . import engine as E


def bilinear_forward(ctx, bil, y0, audio, out_thw):
    """y0 [B,1,7,6,C] (x1: I = 42 positions), audio [B,3,1,1,C] (x2: J = 3) ->
    Act [B,4,7,12,C] with out[b, o, c] = sum_ij x1[b,i,c] W[o,i,j] x2[b,j,c] + bias[o]."""
    x1 = E.materialize(ctx, y0) if not _dense_plain(y0) else y0
    x2 = E.materialize(ctx, audio) if not _dense_plain(audio) else audio
    E.note_reader(ctx, x1)
    E.note_reader(ctx, x2)
    v1, v2 = x1.v, x2.v
    B, Cc = v1.B, v1.C
    I, J = v1.T * v1.H * v1.W, v2.T * v2.H * v2.W
    O = bil.out_features
    assert (I, J) == (bil.in1_features, bil.in2_features) and O == out_thw[0] * out_thw[1] * out_thw[2]
    out = E.Act(E.View.alloc(B, out_thw[0], out_thw[1], out_thw[2], Cc, ctx.dt, ctx.device), needs_grad=True)
    w, bias = bil.weight, bil.bias
    ctx.call("vinet_bilinear_fwd", v1.ptr(), v2.ptr(), ctx.dt, w.data_ptr(), E._ptr(bias), B, Cc, I, J, O,
             out.v.ptr(), ctx.stream)
    if ctx.recording:
        def bwd():
            dg = out.grad_view()
            d1 = x1.grad_view() if x1.needs_grad else None
            d2 = x2.grad_view() if x2.needs_grad else None
            assert not (x1.is_grad_ready() or x2.is_grad_ready()), "bilinear inputs have a single consumer"
            gw = E._param_grad(w) if w.requires_grad else None
            gb = E._param_grad(bias) if (bias is not None and bias.requires_grad) else None
            ctx.call("vinet_bilinear_bwd", v1.ptr(), v2.ptr(), dg.ptr(), ctx.dt, w.data_ptr(), B, Cc, I, J, O,
                     d1.ptr() if d1 else None, d2.ptr() if d2 else None, E._ptr(gw), E._ptr(gb), ctx.stream)
            E._note_param_grad(ctx, w, bias)
            if d1 is not None:
                x1.mark_grad_ready()
            if d2 is not None:
                x2.mark_grad_ready()
        ctx.record(bwd)
    return out


def _dense_plain(a):
    v = a.v
    return a.plain and v.ld == v.C and v.sB == v.T * v.H * v.W * v.C


# parameter order of one encoder layer in VinetTransformerDesc::params / ::grads (include/vinet_hip.h)
def _layer_params(layer):
    a = layer.self_attn
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, layer.linear1.weight, layer.linear1.bias,
            layer.linear2.weight, layer.linear2.bias, layer.norm1.weight, layer.norm1.bias, layer.norm2.weight, layer.norm2.bias]


def transformer_forward(ctx, tf, x, masks=None):
    """x [B,4,7,12,S=32] as it leaves conv_in_1x1 -> Act of the same shape: PositionalEncoding + the encoder stack of `tf`
    (model._TransformerParams) with the 32 channels as tokens and the 336 positions as features.  Training mode (with or
    without gradients, like nn.Dropout) draws dropout masks from (tf.dropout_seed, the device step counter); `masks` (uint8, tf.mask_bytes(B)) receives them."""
    if not _dense_plain(x):
        x = E.materialize(ctx, x)
    E.note_reader(ctx, x)
    xv = x.v
    layers = list(tf.transformer_encoder.layers)
    l0 = layers[0]
    Etok, S = xv.T * xv.H * xv.W, xv.C
    pe = tf.pos_encoder.pe
    assert tuple(pe.shape) == (S, 1, Etok), "positional encoding %s does not fit %d tokens x %d features" % (tuple(pe.shape), S, Etok)
    p = float(l0.dropout.p) if ctx.training else 0.0
    for l in layers:
        assert (l.dropout.p, l.dropout1.p, l.dropout2.p, l.self_attn.dropout) == (l0.dropout.p,) * 4, "one dropout probability per stack"
    params = [q for l in layers for q in _layer_params(l)]
    assert all(q.dtype == torch.float32 and q.is_contiguous() for q in params)
    n = len(params)
    d = L.CTransformerDesc()
    d.dtype, d.B, d.S, d.E, d.H, d.F, d.L = ctx.dt, xv.B, S, Etok, l0.self_attn.num_heads, l0.linear1.out_features, len(layers)
    d.train = 1 if ctx.recording else 0
    d.p, d.eps, d.seed = p, float(l0.norm1.eps), int(tf.dropout_seed) & (2 ** 64 - 1)
    step = tf.step_counter(ctx.device) if p > 0 else None
    d.step, d.pe = E._ptr(step), pe.data_ptr()
    parr = (C.c_void_p * n)(*[q.data_ptr() for q in params])
    d.params = parr
    nbytes = ctx.lib.vinet_transformer_workspace(C.byref(d))
    if nbytes < 0:
        L.check(-1, "vinet_transformer_workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    d.masks = E._ptr(masks)
    out = E.Act(E.View.alloc(xv.B, xv.T, xv.H, xv.W, S, ctx.dt, ctx.device), needs_grad=True)
    ctx.call("vinet_transformer_fwd", C.byref(d), C.byref(xv.ct()), C.byref(out.v.ct()), ctx.stream)
    if ctx.recording:
        def bwd():
            dg = out.grad_view()
            assert not x.is_grad_ready(), "the encoder's input has a single consumer"
            dx = x.grad_view() if x.needs_grad else None
            grads = [E._param_grad(q) if q.requires_grad else None for q in params]
            garr = (C.c_void_p * n)(*[E._ptr(g) for g in grads])
            d.grads, d.masks = garr, None
            # (d keeps parr / ws / step alive through the closure: the descriptor is the forward's, workspace included)
            ctx.call("vinet_transformer_bwd", C.byref(d), C.byref(dg.ct()), C.byref(dx.ct()) if dx else None, ctx.stream)
            E._note_param_grad(ctx, *params)
            if dx is not None:
                x.mark_grad_ready()
        bwd.keep = (parr, ws, step, pe)
        ctx.record(bwd)
    return out


def transformer_tokens(tf, x, masks=None):
    """the encoder of `tf` alone as a root call: x [B, 32, 4, 7, 12] fp32 (channel c = token c, positions = features) -> the same
    shape; differentiable (input and parameters)"""
    body = E.BlockBody(tf, lambda ctx, a: transformer_forward(ctx, tf, a, masks))
    return E.run_root(body, [x], list(tf.parameters()))[0]


# ---- token-wise fusion (model.py:116-189): the rows of the channels-last activation are the tokens -------------------------------

def token_buffer(ctx, B, parts, Cc):
    """one token matrix [B][S = sum of the parts' positions][Cc] and one destination Act per part ((T, H, W) each) over its row
    range (Act.sub_rows): the convs that produce the tokens write straight into it and read their output gradients from the same
    rows of its gradient, which count as written once the buffer's consumer has stored the whole token gradient.
    Returns (tokens Act [B, S, 1, 1, Cc], [part Acts])."""
    S = sum(t * h * w for t, h, w in parts)
    tokens = E.Act(E.View.alloc(B, S, 1, 1, Cc, ctx.dt, ctx.device), needs_grad=True)
    acts, row = [], 0
    for thw in parts:
        acts.append(tokens.sub_rows(row, thw))
        row += thw[0] * thw[1] * thw[2]
    return tokens, acts


def token_encoder_forward(ctx, tf, tokens, out=None, masks=None):
    """tokens [B,T,H,W,E] (T H W = S positions = tokens, the E channels = features) -> Act of the same dims (or `out`, which
    may be a channel sub-view of a wider tensor): PositionalEncoding + the encoder stack of `tf` (model._TransformerParams with
    pe [S,1,E]).  Dropout as transformer_forward; `masks` (uint8, tf.mask_bytes(B)) receives the keep masks.
    The linear products run in the arithmetic of the engine option TOKEN_MMA, resolved HERE, once: the workspace, the forward and
    the backward closure all get that mode, whatever the option says by the time backward runs.  Attention's arithmetic
    (engine.TOKEN_ATTN) is resolved beside it; at F32 the calls are the _mma entry points, as before the option existed."""
    assert tokens.plain, "the token encoder reads plain activations"
    E.note_reader(ctx, tokens)
    xv = tokens.v
    layers = list(tf.transformer_encoder.layers)
    l0 = layers[0]
    S, Efeat = xv.T * xv.H * xv.W, xv.C
    pe = tf.pos_encoder.pe
    assert tuple(pe.shape) == (S, 1, Efeat), "positional encoding %s does not fit %d tokens x %d features" % (tuple(pe.shape), S, Efeat)
    p = float(l0.dropout.p) if ctx.training else 0.0
    for l in layers:
        assert (l.dropout.p, l.dropout1.p, l.dropout2.p, l.self_attn.dropout) == (l0.dropout.p,) * 4, "one dropout probability per stack"
    params = [q for l in layers for q in _layer_params(l)]
    assert all(q.dtype == torch.float32 and q.is_contiguous() for q in params)
    n = len(params)
    d = L.CTokenEncoderDesc()
    d.dtype, d.B, d.S, d.E, d.H, d.F, d.L = ctx.dt, xv.B, S, Efeat, l0.self_attn.num_heads, l0.linear1.out_features, len(layers)
    d.train = 1 if ctx.recording else 0
    d.p, d.eps, d.seed = p, float(l0.norm1.eps), int(tf.dropout_seed) & (2 ** 64 - 1)
    step = tf.step_counter(ctx.device) if p > 0 else None
    d.step, d.pe = E._ptr(step), pe.data_ptr()
    parr = (C.c_void_p * n)(*[q.data_ptr() for q in params])
    d.params = parr
    mma = E.token_mma_mode(ctx.cdt)        # (cdt: the context's arithmetic -- fp32s is a compute mode of the fp32 storage type)
    attn = E.token_attn_mode(ctx.cdt)
    if attn == L.TK_MMA_F32:
        sfx, mode = "_mma", (mma,)
    else:
        sfx, mode = "_attn", (mma, attn)
    nbytes = getattr(ctx.lib, "vinet_token_encoder_workspace" + sfx)(C.byref(d), *mode)
    if nbytes < 0:
        L.check(-1, "vinet_token_encoder_workspace" + sfx)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    d.masks = E._ptr(masks)
    if out is None:
        out = E.Act(E.View.alloc(xv.B, xv.T, xv.H, xv.W, Efeat, ctx.dt, ctx.device))
    out.needs_grad = True
    assert out.v.same_dims(xv) and out.plain, "the encoder's output has its input's dims"
    ctx.call("vinet_token_encoder_fwd" + sfx, C.byref(d), *mode, C.byref(xv.ct()), C.byref(out.v.ct()), ctx.stream)
    if ctx.recording:
        def bwd():
            dg = out.grad_view()
            assert not tokens.is_grad_ready(), "the encoder's input has a single consumer"
            dx = tokens.grad_view() if tokens.needs_grad else None
            grads = [E._param_grad(q) if q.requires_grad else None for q in params]
            garr = (C.c_void_p * n)(*[E._ptr(g) for g in grads])
            d.grads, d.masks = garr, None
            # (d keeps parr / ws / step alive through the closure: the descriptor is the forward's, workspace included)
            ctx.call("vinet_token_encoder_bwd" + sfx, C.byref(d), *mode, C.byref(dg.ct()), C.byref(dx.ct()) if dx else None, ctx.stream)
            E._note_param_grad(ctx, *params)
            if dx is not None:
                tokens.mark_grad_ready()
        bwd.keep = (parr, ws, step, pe)
        ctx.record(bwd)
    return out


def token_split_forward(ctx, tokens, n_audio, out_thw):
    """encoder output [B, Sv + n_audio rows, E] -> the decoder's input [B, T, H, W, 2E] (T H W = Sv): the video rows in channels
    [0, E), the mean of the audio rows in channels [E, 2E) at every position (model.py:175-185)"""
    assert tokens.plain
    E.note_reader(ctx, tokens)
    xv = tokens.v
    T, H, W = out_thw
    assert xv.T * xv.H * xv.W == T * H * W + n_audio
    out = E.Act(E.View.alloc(xv.B, T, H, W, 2 * xv.C, ctx.dt, ctx.device), needs_grad=True)
    ctx.call("vinet_token_split_fwd", C.byref(xv.ct()), ctx.dt, n_audio, C.byref(out.v.ct()), ctx.stream)
    if ctx.recording:
        def bwd():
            dg = out.grad_view()
            assert not tokens.is_grad_ready(), "the split's input has a single consumer"
            if tokens.needs_grad:
                dx = tokens.grad_view()
                ctx.call("vinet_token_split_bwd", C.byref(dg.ct()), ctx.dt, n_audio, C.byref(dx.ct()), ctx.stream)
                tokens.mark_grad_ready()
        ctx.record(bwd)
    return out


def token_encoder_tokens(tf, x, masks=None):
    """the token encoder alone as a root call: x [B, E, T, H, W] fp32 (position = token, channel = feature) -> the same shape;
    differentiable (input and parameters)"""
    body = E.BlockBody(tf, lambda ctx, a: token_encoder_forward(ctx, tf, a, masks=masks))
    return E.run_root(body, [x], list(tf.parameters()))[0]


def token_split(x, n_audio, out_thw):
    """split / mean / broadcast alone as a root call: x [B, E, Sv + n_audio, 1, 1] fp32 -> [B, 2E, T, H, W]; differentiable"""
    holder = torch.nn.Module()
    body = E.BlockBody(holder, lambda ctx, a: token_split_forward(ctx, a, n_audio, out_thw))
    return E.run_root(body, [x], [])[0]
