#!/usr/bin/env python3
"""Timing of the transformer fusion (bench.py measures the flagship workload and stays as it is).

  encoder   the fused HIP encoder stack (3 layers, 32 tokens x 336 features) forward and forward + backward at B = 1, 8, 32, 192
            against torch's own nn.TransformerEncoder in eager mode on the same device, weights and input (dropout 0 on both)
  tokens    the token-wise encoder of VideoAudioSaliencyFusionModel (3 layers, 339 tokens x 512 features, 4 heads) forward and
            forward + backward at --token_batches (default 1, 8, 32, 192) against eager nn.TransformerEncoder in fp32 on the same
            device, weights and input (dropout 0 on both), the two alternating inside each timed round; with the achieved share of
            the 155 TF/s fp32-MFMA rate (FLOPs counted from the shapes) and the workspace bytes per clip.  --token_mma fp32,bf16x3,bf16
            times the encoder in each of these arithmetic modes of its linear products (engine option TOKEN_MMA; --token_attn pairs an attention
            arithmetic, engine.TOKEN_ATTN, with each), all of them and
            aten taking turns inside each round; the first mode fills the hip_* columns, the others hip_<mode>_* columns
  step      the AViNet training step (kldiv + fused Adam, --dtype) with and without use_transformer at --step_batches (default 1, 8, 32, 192)

Warm-up, then the median of --repeats timed runs (device events around one call).  One JSON line per measurement on stdout.

    python tools/transformer_bench.py [--what encoder,tokens,step] [--repeats 30] [--encoder_batches 1,8,32,192] [--step_batches 1,8,32,192] [--dtype bf16]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from vinet_amd import engine as E
from vinet_amd import fusion, synth


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def bench_encoder(args, dev):
    from vinet_amd import model as VM
    E.set_default_dtype("fp32")
    tf = VM._TransformerParams(336, hidden_size=336, nhead=4, num_encoder_layers=3, max_len=32)
    sd = synth.synth_state_dict(tf.state_dict(), 1)
    sd["pos_encoder.pe"] = tf.state_dict()["pos_encoder.pe"]
    tf.load_state_dict(sd)
    for l in tf.transformer_encoder.layers:
        l.dropout.p = l.dropout1.p = l.dropout2.p = 0.0
        l.self_attn.dropout = 0.0
    tf = tf.to(dev).train()
    aten = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(336, 4, 336, dropout=0.0), 3).to(dev).train()
    aten.load_state_dict({k[len("transformer_encoder."):]: v for k, v in sd.items() if k.startswith("transformer_encoder.")})
    pe = sd["pos_encoder.pe"].to(dev)
    for B in [int(b) for b in args.encoder_batches.split(",")]:
        x = synth.normal("bench_x", (B, 32, 4, 7, 12), 2).to(dev)
        g = synth.normal("bench_g", (B, 32, 4, 7, 12), 3).to(dev)
        xt = x.reshape(B, 32, 336).permute(1, 0, 2).contiguous()
        gt = g.reshape(B, 32, 336).permute(1, 0, 2).contiguous()

        def hip_fwd():
            with torch.no_grad():
                return fusion.transformer_tokens(tf, x)

        def hip_fb():
            xr = x.detach().requires_grad_(True)
            (fusion.transformer_tokens(tf, xr) * g).sum().backward()

        def aten_fwd():
            with torch.no_grad():
                return aten(xt + pe)

        def aten_fb():
            xr = xt.detach().requires_grad_(True)
            (aten(xr + pe) * gt).sum().backward()

        row = dict(bench="encoder", B=B)
        for name, fn in (("hip_fwd", hip_fwd), ("aten_fwd", aten_fwd), ("hip_fwd_bwd", hip_fb), ("aten_fwd_bwd", aten_fb)):
            med, lo = median_ms(fn, args.warmup, args.repeats)
            row[name + "_ms"] = round(med, 4)
            row[name + "_min_ms"] = round(lo, 4)
        E.LAUNCH_LOG = []
        hip_fb()
        row["engine_calls_fwd_bwd"] = len(E.LAUNCH_LOG)
        E.LAUNCH_LOG = None
        print(json.dumps(row), flush=True)


FP32_MFMA_PEAK = 155e12      # dense fp32-input MFMA rate of the MI355X, FLOP/s


def token_layer_flops(S, Ef, F):
    """forward FLOPs of one clip and layer: QKV, the two attention products, the out-projection, the two linears"""
    return 2 * S * Ef * 3 * Ef + 2 * 2 * S * S * Ef + 2 * S * Ef * Ef + 2 * 2 * S * Ef * F


def alternating_ms(fns, warmup, repeats):
    """median and minimum ms of each callable, the callables taking turns inside every round (other people's work shares the host:
    a drift then falls on all of them alike)"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def bench_tokens(args, dev):
    import ctypes as C
    from vinet_amd import _lib as L
    from vinet_amd import model as VM
    E.set_default_dtype("fp32")
    S, Ef, H, NL = 339, 512, 4, 3
    tf = VM._TransformerParams(Ef, hidden_size=Ef, nhead=H, num_encoder_layers=NL, max_len=S, max_head_width=VM.TOKEN_ENCODER_MAX_HEAD_WIDTH)
    sd = synth.synth_state_dict(tf.state_dict(), 1)
    sd["pos_encoder.pe"] = tf.state_dict()["pos_encoder.pe"]
    tf.load_state_dict(sd)
    for l in tf.transformer_encoder.layers:
        l.dropout.p = l.dropout1.p = l.dropout2.p = 0.0
        l.self_attn.dropout = 0.0
    tf = tf.to(dev).train()
    aten = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(Ef, H, Ef, dropout=0.0), NL, enable_nested_tensor=False).to(dev).train()
    aten.load_state_dict({k[len("transformer_encoder."):]: v for k, v in sd.items() if k.startswith("transformer_encoder.")})
    pe = sd["pos_encoder.pe"].to(dev)
    flops = NL * token_layer_flops(S, Ef, Ef)
    # a configuration = (arithmetic of the linears, arithmetic of attention); the two lists pair up element by element, a list of one
    # goes with every element of the other.  Named by the linears' mode alone while attention is fp32 (the columns of before the option)
    mmas, attns = [m for m in args.token_mma.split(",") if m], [m for m in args.token_attn.split(",") if m]
    n_cfg = max(len(mmas), len(attns))
    assert len(mmas) in (1, n_cfg) and len(attns) in (1, n_cfg), "--token_mma and --token_attn: lists of equal length, or one of them a single value"
    pairs = [(mmas[i % len(mmas)], attns[i % len(attns)]) for i in range(n_cfg)]
    cfg = {(m if a == "fp32" else "%s_attn_%s" % (m, a)): (m, a) for m, a in pairs}
    modes = list(cfg)
    for B in [int(b) for b in args.token_batches.split(",")]:
        x = synth.normal("bench_tok_x", (B, Ef, S, 1, 1), 2).to(dev)          # NCDHW: position = token, channel = feature
        g = synth.normal("bench_tok_g", (B, Ef, S, 1, 1), 3).to(dev)
        xt = x.reshape(B, Ef, S).permute(2, 0, 1).contiguous()                  # [S, B, E] for nn.TransformerEncoder
        gt = g.reshape(B, Ef, S).permute(2, 0, 1).contiguous()

        def hip_fwd(mode=modes[0]):
            old, old_attn = E.configure(token_mma=cfg[mode][0]), E.set_token_attn(cfg[mode][1])
            try:
                with torch.no_grad():
                    return fusion.token_encoder_tokens(tf, x)
            finally:
                E.configure(**old)
                E.set_token_attn(old_attn)

        def hip_fb(mode=modes[0]):
            old, old_attn = E.configure(token_mma=cfg[mode][0]), E.set_token_attn(cfg[mode][1])
            try:
                xr = x.detach().requires_grad_(True)
                (fusion.token_encoder_tokens(tf, xr) * g).sum().backward()
            finally:
                E.configure(**old)
                E.set_token_attn(old_attn)

        def aten_fwd():
            with torch.no_grad():
                return aten(xt + pe)

        def aten_fb():
            xr = xt.detach().requires_grad_(True)
            (aten(xr + pe) * gt).sum().backward()

        def col(mode, what):
            return "hip_" + what if mode == modes[0] else "hip_%s_%s" % (mode, what)

        with torch.no_grad():
            ref = aten(xt + pe)
            diffs = {m: float((hip_fwd(m).reshape(B, Ef, S).permute(2, 0, 1) - ref).abs().max()) for m in modes}
        reps = max(5, args.repeats // (1 if B <= 32 else 3))
        row = dict(bench="token_encoder", B=B, S=S, E=Ef, H=H, L=NL, token_mma=modes, token_attn=[a for _, a in pairs], max_abs_diff_to_aten=diffs[modes[0]], repeats=reps)
        for m in modes[1:]:
            row["max_abs_diff_to_aten_" + m] = diffs[m]
        fw = {col(m, "fwd"): (lambda m=m: hip_fwd(m)) for m in modes}
        fb = {col(m, "fwd_bwd"): (lambda m=m: hip_fb(m)) for m in modes}
        t = alternating_ms(dict(fw, aten_fwd=aten_fwd), args.warmup, reps)
        t.update(alternating_ms(dict(fb, aten_fwd_bwd=aten_fb), args.warmup, reps))
        for name, (med, lo) in t.items():
            row[name + "_ms"] = round(med, 4)
            row[name + "_min_ms"] = round(lo, 4)
        row["aten_over_hip_fwd"] = round(row["aten_fwd_ms"] / row["hip_fwd_ms"], 3)
        row["aten_over_hip_fwd_bwd"] = round(row["aten_fwd_bwd_ms"] / row["hip_fwd_bwd_ms"], 3)
        for m in modes[1:]:
            row["aten_over_hip_%s_fwd" % m] = round(row["aten_fwd_ms"] / row[col(m, "fwd") + "_ms"], 3)
            row["aten_over_hip_%s_fwd_bwd" % m] = round(row["aten_fwd_bwd_ms"] / row[col(m, "fwd_bwd") + "_ms"], 3)
        # whole-call rates (import / export of the NCDHW boundary and the host's launches included), not a kernel's share of peak
        row["hip_fwd_share_of_fp32_mfma_peak"] = round(B * flops / (row["hip_fwd_ms"] * 1e-3) / FP32_MFMA_PEAK, 4)
        row["hip_fwd_bwd_share_of_fp32_mfma_peak"] = round(3 * B * flops / (row["hip_fwd_bwd_ms"] * 1e-3) / FP32_MFMA_PEAK, 4)
        d = L.CTokenEncoderDesc()
        d.dtype, d.B, d.S, d.E, d.H, d.F, d.L, d.train, d.p, d.eps = L.F32, B, S, Ef, H, Ef, NL, 1, 0.0, 1e-5
        row["workspace_bytes_per_clip"] = int(L.load().vinet_token_encoder_workspace(C.byref(d))) // B
        print(json.dumps(row), flush=True)


def bench_step(args, dev):
    from vinet_amd import loss as VL
    from vinet_amd import model as VM
    from vinet_amd import optim as VO
    E.set_default_dtype(args.dtype)
    for B in [int(b) for b in args.step_batches.split(",")]:
        x = synth.clip(B, 32, 224, 384, 5).permute(0, 2, 1, 3, 4).contiguous().to(dev)
        a = synth.audio(B, 70560, 5).to(dev)
        gt = synth.gt_map(B, 224, 384, 5).to(dev)
        row = dict(bench="avinet_step", B=B, dtype=args.dtype)
        for flag in (False, True):
            m = VM.VideoAudioSaliencyModel(use_transformer=flag, num_clips=32)
            sd = synth.synth_state_dict(m.state_dict(), 3)
            if flag:
                sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
            m.load_state_dict(sd)
            m = m.to(dev).train()
            opt = VO.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-5)

            def step():
                opt.zero_grad()
                VL.kldiv(m(x, a), gt).backward()
                opt.step()

            try:
                med, lo = median_ms(step, 3, args.step_repeats)
            except torch.OutOfMemoryError:
                row["oom_%s" % ("on" if flag else "off")] = True
                del m, opt
                torch.cuda.empty_cache()
                continue
            E.LAUNCH_LOG = []
            step()
            row["launches_%s" % ("on" if flag else "off")] = len(E.LAUNCH_LOG)
            E.LAUNCH_LOG = None
            row["step_ms_%s" % ("on" if flag else "off")] = round(med, 3)
            del m, opt
            torch.cuda.empty_cache()
        if "step_ms_on" in row and "step_ms_off" in row:
            row["overhead_ms"] = round(row["step_ms_on"] - row["step_ms_off"], 3)
        print(json.dumps(row), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--what", default="encoder,step")
    p.add_argument("--warmup", default=5, type=int)
    p.add_argument("--repeats", default=30, type=int)
    p.add_argument("--step_repeats", default=9, type=int)
    p.add_argument("--step_batches", default="1,8,32,192")
    p.add_argument("--encoder_batches", default="1,8,32,192")
    p.add_argument("--token_batches", default="1,8,32,192")
    p.add_argument("--token_mma", default="fp32", help="tokens: comma list of fp32, bf16x3, bf16 (the encoder's linear arithmetic), timed side by side")
    p.add_argument("--token_attn", default="fp32", help="tokens: comma list of fp32, bf16x3, bf16 (the encoder's attention arithmetic), paired with "
                   "--token_mma element by element (a single value goes with all of them); columns hip_<mma>_attn_<attn>_*")
    p.add_argument("--dtype", default="bf16")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    if "encoder" in args.what:
        bench_encoder(args, dev)
    if "tokens" in args.what:
        bench_tokens(args, dev)
    if "step" in args.what:
        bench_step(args, dev)


if __name__ == "__main__":
    main()
