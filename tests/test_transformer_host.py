"""Transformer fusion, host side: the torch comparator is pinned to the reference's recording, and the public surface
(constructor, state_dict layout, argument checks, the trainer's model factory) matches the reference's."""
import json
import os

import pytest
import torch

from tests import goldens as G
from tests import transformer_model as TM
from vinet_amd import synth

KEYS = os.path.join(G.GOLDEN_DIR, "avinet_tf_keys.json")


def _block_inputs(dtype):
    from vinet_amd import model as VM
    z, meta = G.load("transformer_block")
    tf = VM._TransformerParams(336, hidden_size=336, nhead=4, num_encoder_layers=3, max_len=32)
    sd = synth.synth_state_dict(tf.state_dict(), meta["seed"])
    sd["pos_encoder.pe"] = tf.state_dict()["pos_encoder.pe"]
    x = synth.normal("tf_tokens", (32, 2, 336), meta["seed"]).to(dtype)
    proj = synth.normal("tf_proj", (32, 2, 336), meta["seed"]).to(dtype)
    return z, meta, sd, x, proj


def _torch_model_run(dtype):
    z, meta, sd, x, proj = _block_inputs(dtype)
    layers = TM.layers_from_state_dict(sd, "transformer_encoder.", 3, dtype)
    for P in layers:
        for t in P.values():
            t.requires_grad_(True)
    pe = sd["pos_encoder.pe"].to(dtype)
    xg = x.clone().requires_grad_(True)
    y = TM.encoder(xg, pe, layers, 4)
    (y * proj).sum().backward()
    got = {"eval_y": y.detach(), "train_y": y.detach(), "train_gx": xg.grad}
    for i, P in enumerate(layers):
        for k, t in P.items():
            got["train_g:transformer_encoder.layers.%d.%s" % (i, k)] = t.grad
    return z, meta, got


def check_against_block_golden(z, meta, got, factor=4.0, report=None):
    """every tensor of the fixture against `got` (full tensors): max abs error against the fp64 recording <= factor x the
    reference's own fp32-vs-fp64 error of that tensor; weight matrices on their stored rows, and their Frobenius norm within
    factor x that error x sqrt(numel) (|  ||a|| - ||b||  | <= ||a - b|| <= sqrt(n) max|a - b|).  Returns the worst ratio."""
    worst = (0.0, None)
    stride = meta["row_stride"]
    for k, e32 in meta["fp32_err"].items():
        mine = got[k].detach().double().cpu()
        if k + "#rows" in z:
            ref = torch.from_numpy(z[k + "#rows"])
            err = float((mine[::stride] - ref).abs().max())
            nerr = abs(float(mine.norm()) - float(z[k + "#norm"]))
            assert nerr <= factor * e32 * mine.numel() ** 0.5, "%s: Frobenius norm off by %g" % (k, nerr)
        else:
            ref = torch.from_numpy(z[k])
            assert ref.shape == mine.shape, (k, ref.shape, mine.shape)
            err = float((mine - ref).abs().max())
        ratio = err / e32
        if report is not None:
            report[k] = ratio
        if ratio > worst[0]:
            worst = (ratio, k)
        print("%-70s err %.3e  reference fp32 %.3e  ratio %.2f" % (k, err, e32, ratio))
        assert err <= factor * e32, "%s: error %g against the fp64 recording > %g x the reference's own fp32 error %g" % (k, err, factor, e32)
    return worst


def test_torch_model_reproduces_the_reference_recording():
    """tests/transformer_model.py in fp32 against the reference's fp64 run: within 4 x the reference's own fp32 error"""
    z, meta, got = _torch_model_run(torch.float32)
    check_against_block_golden(z, meta, got)


def test_torch_model_fp64_matches_the_recording():
    z, meta, got = _torch_model_run(torch.float64)
    for k in meta["fp32_err"]:
        ref = torch.from_numpy(z[k + "#rows"] if k + "#rows" in z else z[k])
        mine = got[k][::meta["row_stride"]] if k + "#rows" in z else got[k]
        assert float((mine - ref).abs().max()) <= 1e-9 * max(1.0, meta["scale"][k]), k


def _model(**kw):
    from vinet_amd import model as VM
    return VM.VideoAudioSaliencyModel(**kw)


def test_constructor_and_state_dict_layout_match_the_reference():
    m = _model(use_transformer=True, num_clips=32)
    assert m.use_transformer is True
    want = [(k, tuple(s)) for k, s in json.load(open(KEYS))]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want


def test_reference_style_state_dict_loads_strictly_and_round_trips():
    m = _model(use_transformer=True, num_clips=32)
    sd = {k: synth.normal(k, tuple(s), 9) if len(s) else torch.tensor(3) for k, s in json.load(open(KEYS))}
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k].to(back[k].dtype)), k


def test_flag_off_keeps_todays_keys():
    off = list(_model(num_clips=32).state_dict())
    on = list(_model(use_transformer=True, num_clips=32).state_dict())
    extra = [k for k in on if k not in off]
    assert [k for k in on if k in off] == off
    assert all(k.startswith(("conv_in_1x1.", "conv_out_1x1.", "transformer.")) for k in extra) and len(extra) == 4 + 1 + 3 * 12
    assert not any(k.startswith(("conv_in_1x1", "conv_out_1x1", "transformer")) for k in off)


def test_argument_checks():
    with pytest.raises(NotImplementedError, match="32"):
        _model(use_transformer=True, transformer_in_channel=64)
    with pytest.raises(ValueError):
        _model(use_transformer=True, num_encoder_layers=0)
    with pytest.raises(ValueError):
        _model(use_transformer=True, nhead=5)                  # does not divide 336
    with pytest.raises(NotImplementedError, match="width"):
        _model(use_transformer=True, nhead=2)                  # heads of 168 > 96
    assert len(_model(use_transformer=True, num_encoder_layers=1).transformer.transformer_encoder.layers) == 1
    assert _model(use_transformer=True, nhead=6).transformer.transformer_encoder.layers[0].self_attn.num_heads == 6
    _model(use_transformer=False, transformer_in_channel=512)  # (ignored without the flag, as in the reference)


def test_trainer_and_inference_factories_build_the_model():
    from vinet_amd import generate_result_audio_visual as AV
    from vinet_amd import train
    args = train.build_parser().parse_args(["--use_sound", "True", "--use_transformer", "True"])
    m = train.build_model(args)
    assert m.use_transformer and len(m.transformer.transformer_encoder.layers) == 3
    a = AV.build_parser().parse_args([])
    assert a.use_transformer is False


def test_new_parameters_reach_the_optimizer_and_the_gradient_buckets():
    from vinet_amd import parallel
    m = _model(use_transformer=True)
    names = {k for k, _ in m.named_parameters() if k.startswith(("transformer.", "conv_in_1x1.", "conv_out_1x1."))}
    assert len(names) == 4 + 36
    trainable = {id(p) for p in parallel.trainable_parameters(m)}
    assert all(id(p) in trainable for k, p in m.named_parameters() if k in names)


@pytest.mark.parametrize("Ef, F, H, NL", [(48, 80, 4, 2), (96, 16, 1, 2)], ids=["e48_f80_h4_l2", "e96_f16_h1_l2"])
def test_torch_model_equals_nn_transformer_encoder_at_the_small_shapes(Ef, F, H, NL):
    """tests/transformer_model.py against torch.nn.TransformerEncoder, both fp64, eval mode, at the small shapes
    tests/test_gpu_transformer_shapes.py leans on: output and every gradient to 1e-12"""
    from vinet_amd import model as VM
    torch.manual_seed(5)
    tf = VM._TransformerParams(Ef, hidden_size=F, nhead=H, num_encoder_layers=NL, max_len=32)
    sd = synth.synth_state_dict(tf.state_dict(), 13)
    sd["pos_encoder.pe"] = tf.state_dict()["pos_encoder.pe"]
    x = synth.normal("tf_small_tokens", (32, 3, Ef), 13).double()
    proj = synth.normal("tf_small_proj", (32, 3, Ef), 13).double()
    pe = sd["pos_encoder.pe"].double()
    layers = TM.layers_from_state_dict(sd, "transformer_encoder.", NL, torch.float64)
    for P in layers:
        for t in P.values():
            t.requires_grad_(True)
    xa = x.clone().requires_grad_(True)
    ya = TM.encoder(xa, pe, layers, H)
    (ya * proj).sum().backward()
    enc = torch.nn.TransformerEncoder(torch.nn.TransformerEncoderLayer(Ef, H, F), NL, enable_nested_tensor=False).double().eval()
    enc.load_state_dict({k[len("transformer_encoder."):]: v.double() for k, v in sd.items() if k.startswith("transformer_encoder.")})
    xb = x.clone().requires_grad_(True)
    yb = enc(xb + pe)
    (yb * proj).sum().backward()
    assert float((ya - yb).detach().abs().max()) <= 1e-12
    assert float((xa.grad - xb.grad).abs().max()) <= 1e-12
    theirs = dict(enc.named_parameters())
    for i, P in enumerate(layers):
        for k, t in P.items():
            assert float((t.grad - theirs["layers.%d.%s" % (i, k)].grad).abs().max()) <= 1e-12, (i, k)
