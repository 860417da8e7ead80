#!/usr/bin/env python3
"""Fixtures of the token-wise fusion FROM THE REAL REFERENCE (imported unmodified, like make_transformer_goldens.py: stub
packages, a synthetic soundnet8_final.pth, procedural weights from vinet_amd/synth.py).  Writes data only:

  fusion_block.npz     the reference's Transformer(512, hidden_size=512, nhead=4, num_encoder_layers=3, max_len=339) on tokens
                       [339, 2, 512], fp64: eval output; train-mode (every dropout p = 0) output, input gradient, parameter
                       gradients.  Stored as samples: every 8th token row of the activations, every 8th row + Frobenius norm of the
                       four weight-matrix gradients per layer, the small gradients in full; meta["fp32_err"] is the reference's
                       own fp32-vs-fp64 error per tensor (over ALL of its elements)
  avfusion32.npz       VideoAudioSaliencyFusionModel().eval() at 32x224x384 with a 70 560-sample waveform: map, argmax, top-2 gap,
                       calibrated head, the tensor entering the encoder
  avfusion_keys.json   the reference's ordered (key, shape) list of that model

Usage:  python tests/golden/make_fusion_goldens.py [block] [avfusion]
"""
import importlib.util
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tests import goldens as G
from vinet_amd import synth

spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
MG = importlib.util.module_from_spec(spec)
spec.loader.exec_module(MG)

BLOCK_SEED = 67
ROW_STRIDE = 8
SEED_TRIES = 32          # seeds tried for the whole-model case until the top-2 gap reaches avinet32.npz's
S_TOKENS, FEATURES = 4 * 7 * 12 + 3, 512
MATRICES = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight")
ACTIVATIONS = ("eval_y", "train_y", "train_gx")


def _zero_dropout(tf):
    for l in tf.transformer_encoder.layers:
        l.dropout.p = l.dropout1.p = l.dropout2.p = 0.0
        l.self_attn.dropout = 0.0


def _block_run(RM, dtype):
    tf = RM.Transformer(FEATURES, hidden_size=FEATURES, nhead=4, num_encoder_layers=3, max_len=S_TOKENS)
    sd = synth.synth_state_dict(tf.state_dict(), BLOCK_SEED)
    sd["pos_encoder.pe"] = tf.state_dict()["pos_encoder.pe"]          # (a buffer, not a weight: the sinusoid table stays)
    tf.load_state_dict(sd)
    tf = tf.to(dtype)
    x = synth.normal("fusion_tokens", (S_TOKENS, 2, FEATURES), BLOCK_SEED).to(dtype)
    proj = synth.normal("fusion_proj", (S_TOKENS, 2, FEATURES), BLOCK_SEED).to(dtype)
    res = {}
    tf.eval()
    with torch.no_grad():
        res["eval_y"] = tf(x, -1)
    tf.train()
    _zero_dropout(tf)
    xg = x.clone().requires_grad_(True)
    y = tf(xg, -1)
    (y * proj).sum().backward()
    res["train_y"] = y.detach()
    res["train_gx"] = xg.grad
    for k, p in tf.named_parameters():
        res["train_g:" + k] = p.grad
    return res


def block_case(RM, out):
    r64, r32 = _block_run(RM, torch.float64), _block_run(RM, torch.float32)
    arrays, err = {}, {}
    for k, v in r64.items():
        err[k] = float((r32[k].double() - v).abs().max())
        if k in ACTIVATIONS:
            arrays[k + "#rows"] = v[::ROW_STRIDE].numpy()
        elif k.split("layers.")[-1].split(".", 1)[1] in MATRICES:
            arrays[k + "#rows"] = v[::ROW_STRIDE].numpy()
            arrays[k + "#norm"] = np.array(float(v.norm()))
        else:
            arrays[k] = v.numpy()
    meta = dict(seed=BLOCK_SEED, row_stride=ROW_STRIDE, fp32_err=err, shape=[S_TOKENS, 2, FEATURES], nhead=4, layers=3,
                scale={k: float(v.abs().max()) for k, v in r64.items()})
    G.save(os.path.join(out, "fusion_block.npz"), meta=np.array(json.dumps(meta)), **arrays)
    print("fusion_block ok: worst fp32-vs-fp64 error %.3g (%s)" % (max(err.values()), max(err, key=err.get)))


def avfusion_case(RM, seed, out, min_gap):
    cwd, tmp = os.getcwd(), tempfile.mkdtemp(prefix="vinet_snd_")
    os.chdir(tmp)
    try:
        torch.save(RM.SoundNet().state_dict(), "soundnet8_final.pth")
        ref = RM.VideoAudioSaliencyFusionModel().eval()
    finally:
        os.chdir(cwd)
    keys = [[k, list(v.shape)] for k, v in ref.state_dict().items()]
    with open(os.path.join(out, "avfusion_keys.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(k) for k in keys) + "\n]\n")          # one [key, shape] pair per line
    pe = ref.state_dict()["transformer.pos_encoder.pe"].clone()

    best = None
    for s in range(seed, seed + SEED_TRIES):
        x = synth.clip(1, 32, 224, 384, s).permute(0, 2, 1, 3, 4)
        a = synth.audio(1, 70560, s)

        def run_logits(m):
            box, h = MG._logits_hook(m, m.visual_model.decoder)
            with torch.no_grad():
                m(x, a)
            h.remove()
            return box["l"]

        ref.load_state_dict(dict(synth.synth_state_dict(ref.state_dict(), s), **{"transformer.pos_encoder.pe": pe}))
        sd, wk, bk = MG._calibrated_sd(ref, s, run_logits)
        sd["transformer.pos_encoder.pe"] = pe
        ref.load_state_dict(sd)
        box = {}
        h = ref.transformer.register_forward_hook(lambda m, i, o: box.__setitem__("t", i[0].detach()))
        with torch.no_grad():
            y = ref(x, a)
        h.remove()
        idx, gap = MG._top2(y[0])
        print("avfusion32 seed %d: argmax %d gap %.3g" % (s, idx, gap))
        if best is None or gap > best[3]:
            best = (s, sd, y, gap, idx, wk, bk, box["t"])
        if gap >= min_gap:
            break
    s, sd, y, gap, idx, wk, bk, tokens = best
    if gap < min_gap:
        raise SystemExit("no seed with a top-2 gap >= %g (avinet32.npz's)" % min_gap)
    G.save(os.path.join(out, "avfusion32.npz"), y=MG._np(y), tokens=MG._np(tokens), head_w=MG._np(sd[wk]), head_b=MG._np(sd[bk]),
           meta=np.array(json.dumps(dict(seed=s, argmax=idx, top2_gap=gap, head_w_key=wk, head_b_key=bk))))
    print("avfusion32 ok: seed %d range [%.4f, %.4f] argmax %d gap %.3g" % (s, y.min(), y.max(), idx, gap))


def main():
    torch.set_num_threads(os.cpu_count())
    RM, RU, RL = MG._import_reference()
    if "block" in sys.argv[1:] or not sys.argv[1:]:
        block_case(RM, HERE)
    if "avfusion" in sys.argv[1:] or not sys.argv[1:]:
        _, m0 = G.load("avinet32")
        avfusion_case(RM, 83, HERE, float(m0["top2_gap"]))


if __name__ == "__main__":
    main()
