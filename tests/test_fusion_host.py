"""Token-wise fusion, host side: the torch comparator is pinned to the reference's recording at S = 339, E = 512, and the public
surface of VideoAudioSaliencyFusionModel (constructor, state_dict layout, optimizer parameters, argument and descriptor checks)
is the reference's."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import goldens as G
from tests import transformer_model as TM
from vinet_amd import _lib as L
from vinet_amd import synth

KEYS = os.path.join(G.GOLDEN_DIR, "avfusion_keys.json")
S_TOKENS, FEATURES, HEADS, LAYERS = 339, 512, 4, 3


def block_inputs(dtype):
    """(fixture, meta, state dict, tokens [339, 2, 512], projection) of fusion_block.npz"""
    from vinet_amd import model as VM
    z, meta = G.load("fusion_block")
    tf = VM._TransformerParams(FEATURES, hidden_size=FEATURES, nhead=HEADS, num_encoder_layers=LAYERS, max_len=S_TOKENS,
                               max_head_width=VM.TOKEN_ENCODER_MAX_HEAD_WIDTH)
    sd = synth.synth_state_dict(tf.state_dict(), meta["seed"])
    sd["pos_encoder.pe"] = tf.state_dict()["pos_encoder.pe"]
    x = synth.normal("fusion_tokens", (S_TOKENS, 2, FEATURES), meta["seed"]).to(dtype)
    proj = synth.normal("fusion_proj", (S_TOKENS, 2, FEATURES), meta["seed"]).to(dtype)
    return z, meta, sd, x, proj


def torch_model_run(sd, x, proj, dtype, nhead=HEADS, n_layers=LAYERS):
    layers = TM.layers_from_state_dict(sd, "transformer_encoder.", n_layers, dtype)
    for P in layers:
        for t in P.values():
            t.requires_grad_(True)
    xg = x.to(dtype).clone().requires_grad_(True)
    y = TM.encoder(xg, sd["pos_encoder.pe"].to(dtype), layers, nhead)
    (y * proj.to(dtype)).sum().backward()
    got = {"eval_y": y.detach(), "train_y": y.detach(), "train_gx": xg.grad}
    for i, P in enumerate(layers):
        for k, t in P.items():
            got["train_g:transformer_encoder.layers.%d.%s" % (i, k)] = t.grad
    return got


def against_block_golden(z, meta, got, allowance):
    """every tensor of the fixture against `got` (full tensors) on the stored samples: `allowance(key)` bounds max |got - recording|;
    a weight matrix's Frobenius norm within allowance x sqrt(numel).  Returns {key: error / allowance}; asserts after measuring all."""
    stride, ratios, bad = meta["row_stride"], {}, []
    for k in meta["fp32_err"]:
        mine = got[k].detach().double().cpu()
        allow = allowance(k)
        if k + "#rows" in z:
            ref = torch.from_numpy(z[k + "#rows"])
            assert mine[::stride].shape == ref.shape, (k, mine.shape, ref.shape)
            err = float((mine[::stride] - ref).abs().max())
            if k + "#norm" in z:
                nerr = abs(float(mine.norm()) - float(z[k + "#norm"]))
                if not nerr <= allow * mine.numel() ** 0.5:
                    bad.append((k, "norm", nerr))
        else:
            ref = torch.from_numpy(z[k])
            assert ref.shape == mine.shape, (k, ref.shape, mine.shape)
            err = float((mine - ref).abs().max())
        ratios[k] = err / allow
        print("%-70s err %.3e allowance %.3e" % (k, err, allow))
        if not err <= allow:
            bad.append((k, err, allow))
    assert not bad, bad
    return ratios


def test_torch_model_fp64_reproduces_the_reference_recording_at_339_tokens():
    """tests/transformer_model.py in fp64 at S = 339, E = 512 on the sampled rows: 1e-12 relative to the tensor's largest element"""
    z, meta, sd, x, proj = block_inputs(torch.float64)
    got = torch_model_run(sd, x, proj, torch.float64)
    against_block_golden(z, meta, got, lambda k: 1e-12 * max(1.0, meta["scale"][k]))


def _model(**kw):
    from vinet_amd import model as VM
    return VM.VideoAudioSaliencyFusionModel(**kw)


def test_constructor_defaults_and_state_dict_layout_match_the_reference():
    import inspect
    from vinet_amd import model as VM
    sig = inspect.signature(VM.VideoAudioSaliencyFusionModel.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
        ("use_transformer", True), ("transformer_in_channel", 512), ("num_encoder_layers", 3), ("nhead", 4), ("use_upsample", True),
        ("num_hier", 3), ("num_clips", 32)]
    m = _model()
    assert m.use_transformer is True
    want = [(k, tuple(s)) for k, s in json.load(open(KEYS))]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want
    assert tuple(m.state_dict()["transformer.pos_encoder.pe"].shape) == (339, 1, 512)
    assert isinstance(m.audio_conv_1x1, torch.nn.Conv2d) and m.audio_conv_1x1.kernel_size == (1, 1)


def test_reference_style_state_dict_loads_strictly_and_round_trips():
    m = _model()
    sd = {k: synth.normal(k, tuple(s), 9) if len(s) else torch.tensor(3) for k, s in json.load(open(KEYS))}
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k].to(back[k].dtype)), k


def test_optimizer_parameters_leave_out_bilinear_and_the_soundnet_heads():
    from vinet_amd import parallel
    m = _model()
    named = dict(m.named_parameters())
    trainable = {id(p) for p in parallel.trainable_parameters(m)}
    left_out = sorted(k for k, p in named.items() if id(p) not in trainable)
    assert left_out == sorted(["bilinear.weight", "bilinear.bias", "audionet.conv8_objs.weight", "audionet.conv8_objs.bias",
                               "audionet.conv8_scns.weight", "audionet.conv8_scns.bias"])
    for k in ("conv_in_1x1.weight", "conv_in_1x1.bias", "audio_conv_1x1.weight", "audio_conv_1x1.bias",
              "transformer.transformer_encoder.layers.2.norm2.bias", "audionet.conv1.weight", "visual_model.decoder.convtsp1.0.weight"):
        assert id(named[k]) in trainable, k


def test_refused_constructor_arguments_say_why():
    with pytest.raises(NotImplementedError, match="1024"):
        _model(transformer_in_channel=256)
    with pytest.raises(NotImplementedError, match="does not divide"):
        _model(nhead=3)
    with pytest.raises(NotImplementedError, match="width 256"):
        _model(nhead=2)
    with pytest.raises(NotImplementedError, match=r"4\*7\*12\+3"):
        _model(num_clips=16)
    assert _model(nhead=8, num_encoder_layers=1).transformer.transformer_encoder.layers[0].self_attn.num_heads == 8
    assert _model(use_transformer=False).use_transformer is False        # (stored, ignored)


def test_driver_factories_build_the_fusion_model_only_when_asked():
    from vinet_amd import generate_result_audio_visual as AV
    from vinet_amd import model as VM
    from vinet_amd import train
    args = train.build_parser().parse_args(["--use_sound", "True", "--token_fusion", "True"])
    assert isinstance(train.build_model(args), VM.VideoAudioSaliencyFusionModel)
    assert train.build_parser().parse_args([]).token_fusion is False
    assert type(train.build_model(train.build_parser().parse_args(["--use_sound", "True"]))) is VM.VideoAudioSaliencyModel
    with pytest.raises(ValueError, match="use_sound"):
        train.build_model(train.build_parser().parse_args(["--token_fusion", "True"]))
    a = AV.build_parser().parse_args([])
    assert a.token_fusion is False
    assert isinstance(AV.build_token_fusion_model(AV.build_parser().parse_args(["--token_fusion", "True"])), VM.VideoAudioSaliencyFusionModel)


def _desc(**kw):
    d = L.CTokenEncoderDesc()
    d.dtype, d.B, d.S, d.E, d.H, d.F, d.L, d.train, d.p, d.eps, d.seed = L.F32, 2, 339, 512, 4, 512, 3, 1, 0.0, 1e-5, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _workspace(**kw):
    lib = L.load()
    n = lib.vinet_token_encoder_workspace(C.byref(_desc(**kw)))
    return n, (lib.vinet_last_error() or b"").decode()


@pytest.mark.parametrize("fields, named", [
    (dict(E=528, H=6), "E = 528"),
    (dict(E=24, H=2), "E = 24"),
    (dict(E=528, H=4), "E = 528"),                  # head width 132: only reachable with E > 512 (132 H is a multiple of 16 from H = 4)
    (dict(E=272, H=2), "E / H = 272 / 2"),          # head width 136: the nearest width above 128 that a valid E reaches
    (dict(E=512, H=2), "E / H = 512 / 2"),          # head width 256
    (dict(E=80, H=8), "E / H = 80 / 8"),            # head width 10: not a multiple of 4
    (dict(S=0), "S = 0"),
    (dict(S=1025), "S = 1025"),
    (dict(F=40), "F = 40"),
    (dict(p=1.0), "p = 1.0"),
], ids=["e528", "e24", "width132", "width136", "width256", "width10", "s0", "s1025", "f40", "p1"])
def test_descriptor_limits_are_checked_without_a_gpu(fields, named):
    """the limits of include/vinet_hip.h, answered by vinet_token_encoder_workspace before anything touches a device"""
    assert _workspace()[0] > 0
    n, msg = _workspace(**fields)
    print(n, msg)
    assert n == -1 and named in msg, (n, msg)


def test_descriptors_at_the_limits_are_accepted():
    for kw in (dict(E=512, H=4), dict(E=400, H=5), dict(E=144, H=4), dict(E=16, H=1), dict(E=16, H=4), dict(S=1), dict(S=1024, B=1), dict(F=16), dict(p=0.5)):
        n, msg = _workspace(**kw)
        assert n > 0, (kw, msg)


def test_workspace_of_the_real_shape_is_what_the_design_states():
    """per clip and layer with train = 1 at S = 339 (352 rows), E = F = 512, H = 4: the saved matrices (x, qkv, ao, z1, x1, h, z2 =
    9 E-wide matrices of 352 rows), the softmax rows and the LayerNorm statistics"""
    per = lambda B, NL: _workspace(B=B, L=NL)[0]
    layer = per(1, 2) - per(1, 1)
    assert layer == 4 * (352 * 512 * 9 + 4 * 339 * 339 + 2 * (2 * 352))


def test_index_guard_counts_the_widest_token_matrix():
    """the keep masks of sites 1..3 count elements of [B Sp][E] and [B Sp][F] in 32 bits: F, which has no bound of its own, is part
    of the guard (2 clips x 1024 rows x F = 2^20 is 2^31 elements)"""
    assert _workspace(B=2, S=1024, E=16, H=1, F=1 << 19, L=1)[0] > 0
    n, msg = _workspace(B=2, S=1024, E=16, H=1, F=1 << 20, L=1)
    assert n == -1 and "32-bit" in msg, (n, msg)


def test_graph_capture_of_the_fusion_model_is_refused_with_the_reason():
    """graph.GraphedTrainStep / GraphedInference: a captured step of this model has never been replayed under test, so capture is
    refused before anything is run (no GPU needed); other models are not affected by the check"""
    from vinet_amd import graph as VG
    from vinet_amd import model as VM
    m = _model()
    x, a, gt = torch.zeros(1, 3, 32, 224, 384), torch.zeros(1, 1, 70560, 1), torch.zeros(1, 224, 384)
    with pytest.raises(NotImplementedError, match="never been replayed under test"):
        VG.GraphedTrainStep(m, None, None, (x, a), gt)
    with pytest.raises(NotImplementedError, match="VideoAudioSaliencyFusionModel cannot be captured"):
        VG.GraphedInference(m, x, a)
    wrapped = torch.nn.Sequential(m)                     # (a wrapper, as DistributedDataParallel is, does not hide it)
    with pytest.raises(NotImplementedError):
        VG.GraphedTrainStep(wrapped, None, None, (x, a), gt)
    VG._refuse_uncapturable(VM.VideoSaliencyModel())
    assert getattr(VM.VideoAudioSaliencyModel, "graph_capture_refusal", None) is None


def test_inference_driver_flag_reads_false_as_false():
    from vinet_amd import generate_result_audio_visual as AV
    parse = lambda *a: AV.build_parser().parse_args(list(a)).token_fusion
    assert parse("--token_fusion", "False") is False and parse("--token_fusion", "0") is False
    assert parse("--token_fusion", "True") is True and parse() is False


def _stage_text(path, begin, end):
    """the text of one shared stage: from the line that starts with `begin` through the first line after it that equals `end`"""
    lines = open(path).read().split("\n")
    i = next(k for k, l in enumerate(lines) if l.startswith(begin))
    j = next(k for k in range(i, len(lines)) if lines[k] == end)
    return "\n".join(lines[i:j + 1])


@pytest.mark.parametrize("begin, end", [
    ("struct Drop {", "VN_DEV bool drop_keep(const DropKey& k, uint32_t elem) { return mix32(mix32(elem ^ k.k0) ^ k.k1) >= k.thr; }"),
    ("__global__ void tf_step_kernel(", "}"),
    ("enum { EPI_BIAS = 0,", "};"),
    ("template <int MT, bool AK, bool BK, int EPI>", "}"),
    ("__global__ __launch_bounds__(256) void tf_reduce_split(", "}"),
    ("struct SmallGrads {", "}"),
], ids=["keep_masks", "step_kernel", "gemm_epilogue_struct", "tf_gemm", "reduce_split", "reduce_clips"])
def test_stages_that_exist_in_both_encoders_are_the_same_text(begin, end):
    """csrc/tf_common.h repeats stages of csrc/transformer.hip (keep-mask hash and stream numbering, the step kernel, the token
    GEMM with its epilogues, the fixed-order reductions).  The mask layout, `tests/transformer_model.split_masks` and the step
    counter's meaning assume that both encoders run the same code: until the two are folded into one, their texts must be equal"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vinet_amd", "csrc")
    a = _stage_text(os.path.join(csrc, "transformer.hip"), begin, end)
    b = _stage_text(os.path.join(csrc, "tf_common.h"), begin, end)
    assert len(a) > 40 and a == b
