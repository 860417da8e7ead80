"""Transformer fusion on the MI355X: the encoder kernels against the reference's recording and the torch model
(tests/transformer_model.py), the audio-visual model end to end, batching, repeatability, dropout, training, inference."""
import json
import os

import numpy as np
import pytest
import torch

from tests import goldens as G
from tests import model_cases as MC
from tests import transformer_model as TM
from tests.test_transformer_host import _block_inputs, check_against_block_golden
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, EF, H, NL = 32, 336, 4, 3


@pytest.fixture(autouse=True)
def _real_library():
    assert not L.is_test_double()
    L.load()
    yield
    E.set_default_dtype("bf16")


from tests.gpu_report import note as _note


def _to_ncdhw(tokens, thw=(4, 7, 12)):
    """[S, B, E] -> [B, S, T, H, W] with T H W = E (the model's own 4 x 7 x 12 positions unless told otherwise)"""
    return tokens.permute(1, 0, 2).reshape(tokens.shape[1], S, *thw).contiguous()


def _to_tokens(x):
    return x.reshape(x.shape[0], S, -1).permute(1, 0, 2)


def _encoder(sd, p=None, train=True, seed=1234):
    from vinet_amd import model as VM
    tf = VM._TransformerParams(EF, hidden_size=EF, nhead=H, num_encoder_layers=NL, max_len=S)
    tf.load_state_dict(sd)
    tf.dropout_seed = seed
    if p is not None:
        for l in tf.transformer_encoder.layers:
            l.dropout.p = l.dropout1.p = l.dropout2.p = p
            l.self_attn.dropout = p
    return tf.to(DEV).train(train)


def _run(tf, x_tokens, proj_tokens, masks=None, thw=(4, 7, 12)):
    """forward + backward of the HIP encoder on tokens [S, B, E]; returns tensors keyed like the block fixture"""
    from vinet_amd import fusion
    for q in tf.parameters():
        q.grad = None
    x = _to_ncdhw(x_tokens, thw).to(DEV).requires_grad_(True)
    y = fusion.transformer_tokens(tf, x, masks)
    (y * _to_ncdhw(proj_tokens, thw).to(DEV)).sum().backward()
    got = {"train_y": _to_tokens(y.detach()), "train_gx": _to_tokens(x.grad)}
    for k, q in tf.named_parameters():
        got["train_g:" + k] = q.grad.clone()
    return got


def _torch_run(sd, x, proj, dtype, p=0.0, masks=None, nhead=H, n_layers=NL):
    layers = TM.layers_from_state_dict(sd, "transformer_encoder.", n_layers, dtype)
    for P in layers:
        for t in P.values():
            t.requires_grad_(True)
    xg = x.to(dtype).clone().requires_grad_(True)
    y = TM.encoder(xg, sd["pos_encoder.pe"].to(dtype), layers, nhead, p, masks)
    (y * proj.to(dtype)).sum().backward()
    got = {"train_y": y.detach(), "train_gx": xg.grad}
    for i, P in enumerate(layers):
        for k, t in P.items():
            got["train_g:transformer_encoder.layers.%d.%s" % (i, k)] = t.grad
    return got


def test_block_against_the_reference_recording_fp32():
    """output, input gradient, small gradients in full, sampled rows and norms of the weight gradients: error against the
    reference's fp64 recording <= 4 x the reference's own fp32 error, per tensor"""
    from vinet_amd import fusion
    E.set_default_dtype("fp32")
    z, meta, sd, x, proj = _block_inputs(torch.float32)
    got = _run(_encoder(sd, p=0.0), x, proj)
    tf_eval = _encoder(sd, train=False)
    with torch.no_grad():
        got["eval_y"] = _to_tokens(fusion.transformer_tokens(tf_eval, _to_ncdhw(x).to(DEV)))
    report = {}
    try:
        worst = check_against_block_golden(z, meta, got, 4.0, report)
    finally:
        if report:
            _note("transformer_block_fp32", dict(worst_ratio_to_reference_fp32_error=max(report.values()), gate=4.0,
                                                 worst_tensor=max(report, key=report.get)))
    assert worst[0] <= 4.0


def test_block_against_the_torch_model_on_every_row():
    """the same run against tests/transformer_model.py in fp64 on ALL rows of every gradient, same bound per tensor"""
    E.set_default_dtype("fp32")
    z, meta, sd, x, proj = _block_inputs(torch.float32)
    got = _run(_encoder(sd, p=0.0), x, proj)
    ref = _torch_run(sd, x, proj, torch.float64)
    for k, r in ref.items():
        err = float((got[k].double().cpu() - r).abs().max())
        print("%-70s err %.3e bound %.3e" % (k, err, 4 * meta["fp32_err"][k]))
        assert err <= 4 * meta["fp32_err"][k], (k, err, meta["fp32_err"][k])


def _avinet_tf(dtype):
    from vinet_amd import model as VM
    E.set_default_dtype(dtype)
    z, meta = G.load("avinet32_tf")
    m = VM.VideoAudioSaliencyModel(use_transformer=True, num_clips=32).eval()
    sd = G.state_dict_for(m, meta["seed"], z, meta)
    sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
    m.load_state_dict(sd)
    m = m.to(DEV)
    x = synth.clip(1, 32, 224, 384, meta["seed"]).to(DEV).permute(0, 2, 1, 3, 4)
    a = synth.audio(1, 70560, meta["seed"]).to(DEV)
    with torch.no_grad():
        y = m(x, a)
    return y, z, meta


@pytest.mark.parametrize("dtype", ["fp32", "fp32s"])
def test_avinet_transformer_map(dtype):
    y, z, meta = _avinet_tf(dtype)
    d = float((y.cpu().double() - torch.from_numpy(z["y"]).double()).abs().max())
    _note("avinet_tf_" + dtype, dict(max_abs=d, top2_gap=meta["top2_gap"]))
    print("avinet_tf", dtype, "max abs", d)
    MC.close(y, z["y"], 1e-4, "avinet transformer map (%s)" % dtype)
    assert int(y.reshape(-1).argmax()) == meta["argmax"]


def test_avinet_transformer_map_bf16():
    y, z, meta = _avinet_tf("bf16")
    ref = torch.from_numpy(z["y"]).double().reshape(-1)
    mine = y.cpu().double().reshape(-1)
    d = float((mine - ref).abs().max())
    cc = float(np.corrcoef(mine.numpy(), ref.numpy())[0, 1])
    top5 = torch.topk(mine, 5).indices.tolist()
    _note("avinet_tf_bf16", dict(max_abs=d, cc=cc, argmax_matches=int(mine.argmax()) == meta["argmax"]))
    print("avinet_tf bf16 max abs", d, "cc", cc)
    assert d <= 2.5e-2 and cc >= 0.999 and meta["argmax"] in top5


def test_batch_items_equal_single_clips_and_runs_repeat():
    """B = 1, 3, 8: every item of a batch equals the same clip run alone (output and input gradient, exactly); two runs
    of the same batch agree bit for bit, gradients included"""
    E.set_default_dtype("fp32")
    z, meta, sd, _, _ = _block_inputs(torch.float32)
    tf = _encoder(sd, p=0.0)
    x = synth.normal("tf_batch", (S, 8, EF), 3)
    proj = synth.normal("tf_batch_proj", (S, 8, EF), 3)
    single = [_run(tf, x[:, b:b + 1], proj[:, b:b + 1]) for b in range(8)]
    for B in (1, 3, 8):
        a = _run(tf, x[:, :B], proj[:, :B])
        b = _run(tf, x[:, :B], proj[:, :B])
        for k in a:
            assert torch.equal(a[k], b[k]), "B = %d: %s differs between two runs" % (B, k)
        for i in range(B):
            assert torch.equal(a["train_y"][:, i], single[i]["train_y"][:, 0]), (B, i)
            assert torch.equal(a["train_gx"][:, i], single[i]["train_gx"][:, 0]), (B, i)


def test_many_clips_take_the_sliced_weight_gradients():
    """B = 32 (1024 tokens: weight gradients summed over two 512-token slices): output and every gradient
    against the torch model in fp64, bound per tensor 4 x the torch model's own fp32-vs-fp64 error; two runs bit-identical"""
    E.set_default_dtype("fp32")
    z, meta, sd, _, _ = _block_inputs(torch.float32)
    tf = _encoder(sd, p=0.0)
    x = synth.normal("tf_many", (S, 32, EF), 4)
    proj = synth.normal("tf_many_proj", (S, 32, EF), 4)
    a, b = _run(tf, x, proj), _run(tf, x, proj)
    r64, r32 = _torch_run(sd, x, proj, torch.float64), _torch_run(sd, x, proj, torch.float32)
    worst = 0.0
    for k, r in r64.items():
        assert torch.equal(a[k], b[k]), k
        e32 = float((r32[k].double() - r).abs().max())
        err = float((a[k].double().cpu() - r).abs().max())
        worst = max(worst, err / e32)
        print("%-70s err %.3e torch-fp32 %.3e" % (k, err, e32))
        assert err <= 4 * e32, (k, err, e32)
    _note("transformer_block_b32_fp32", dict(worst_ratio_to_torch_fp32_error=worst))


def test_dropout_matches_the_torch_model_under_the_exported_masks():
    """p = 0.1: forward and every gradient equal the torch model given the kernels' own keep masks.  Bound per tensor: 4 x the
    torch model's own fp32-vs-fp64 error under the same masks.  Keep fraction within 5 sigma of 0.9 per site; the same
    (seed, counter) gives the same masks, the next step different ones."""
    E.set_default_dtype("fp32")
    z, meta, sd, x, proj = _block_inputs(torch.float32)
    p, B = 0.1, 2
    tf = _encoder(sd, p=p, seed=77)
    masks = torch.zeros(tf.mask_bytes(B), dtype=torch.uint8, device=DEV)
    got = _run(tf, x, proj, masks)
    assert int(tf.step_counter(DEV)) == 1
    mk = TM.split_masks(masks.cpu(), NL, B, S, EF, EF, H)
    for li, ms in enumerate(mk):
        for si, m in enumerate(ms):
            n, frac = m.numel(), float(m.float().mean())
            assert set(m.unique().tolist()) <= {0, 1}
            assert abs(frac - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, "layer %d site %d keeps %.4f" % (li, si, frac)
    r64 = _torch_run(sd, x, proj, torch.float64, p, mk)
    r32 = _torch_run(sd, x, proj, torch.float32, p, mk)
    worst = 0.0
    for k, r in r64.items():
        e32 = float((r32[k].double() - r).abs().max())
        err = float((got[k].double().cpu() - r).abs().max())
        worst = max(worst, err / e32)
        print("%-70s err %.3e torch-fp32 %.3e" % (k, err, e32))
        assert err <= 4 * e32, (k, err, e32)
    _note("transformer_dropout_fp32", dict(worst_ratio_to_torch_fp32_error=worst))
    # same (seed, counter) -> same masks; the next step -> new ones
    tf.step_counter(DEV).zero_()
    again = torch.zeros_like(masks)
    got2 = _run(tf, x, proj, again)
    assert torch.equal(again, masks)
    for k in got:
        assert torch.equal(got[k], got2[k]), k
    nxt = torch.zeros_like(masks)
    _run(tf, x, proj, nxt)
    assert int(tf.step_counter(DEV)) == 2
    assert 0.7 < float((nxt == masks).float().mean()) < 0.9          # independent masks agree on 0.81 + 0.01 of the elements
    # eval mode draws nothing
    tf.eval()
    e = torch.full_like(masks, 7)
    from vinet_amd import fusion
    with torch.no_grad():
        fusion.transformer_tokens(tf, _to_ncdhw(x).to(DEV), e)
    assert int(tf.step_counter(DEV)) == 2 and bool((e == 7).all())
    # training mode WITHOUT gradients drops like nn.Dropout does: masks are drawn and the counter advances
    tf.train()
    ng = torch.zeros_like(masks)
    with torch.no_grad():
        y_ng = fusion.transformer_tokens(tf, _to_ncdhw(x).to(DEV), ng)
    assert int(tf.step_counter(torch.device("cuda"))) == 3          # ("cuda" and "cuda:0" name the same counter)
    frac = float(ng.float().mean())
    assert abs(frac - (1 - p)) <= 5 * (p * (1 - p) / ng.numel()) ** 0.5
    tf.step_counter(DEV).fill_(2)
    got3 = _run(tf, x, proj, torch.zeros_like(masks))               # the same step with gradients: the same forward
    assert torch.equal(_to_tokens(y_ng), got3["train_y"])


def _train_setup(dtype="fp32"):
    from vinet_amd import model as VM
    E.set_default_dtype(dtype)
    m = VM.VideoAudioSaliencyModel(use_transformer=True, num_clips=32)
    sd = synth.synth_state_dict(m.state_dict(), 3)
    sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    x = synth.clip(1, 32, 224, 384, 5).permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    a = synth.audio(1, 70560, 5).to(DEV)
    gt = synth.gt_map(1, 224, 384, 5).to(DEV)
    return m, x, a, gt


def test_training_step_moves_every_transformer_parameter_and_the_loss_falls():
    from vinet_amd import loss as VL
    from vinet_amd import optim as VO
    m, x, a, gt = _train_setup()
    before = {k: p.detach().clone() for k, p in m.named_parameters() if k.startswith(("transformer.", "conv_in_1x1.", "conv_out_1x1."))}
    assert len(before) == 40
    opt = VO.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = VL.kldiv(m(x, a), gt)
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if step == 0:
            now = dict(m.named_parameters())
            for k, v in before.items():
                assert not torch.equal(now[k].detach(), v), "%s did not move" % k
    _note("avinet_tf_train_fp32", dict(losses=losses))
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0], losses
    assert int(m.transformer.step_counter(DEV)) == 3


def test_graph_replay_of_a_training_step_draws_new_masks():
    """graph.GraphedTrainStep captures the training step of this model like any other; the step counter lives in device memory
    and the captured forward reads and advances it, so every replay draws new masks (masks are a function of the counter:
    test_dropout_matches_the_torch_model_under_the_exported_masks)"""
    from vinet_amd import graph as VG
    from vinet_amd import loss as VL
    from vinet_amd import optim as VO
    m, x, a, gt = _train_setup("bf16")
    # lr = 0: the weights stay put, so on one batch the replays' losses can differ through the dropout masks alone
    opt = VO.Adam([p for p in m.parameters() if p.requires_grad], lr=0.0)
    step = VG.GraphedTrainStep(m, opt, VL.kldiv, (x, a), gt)
    c0 = int(m.transformer.step_counter(DEV))
    losses = []
    for _ in range(3):
        losses.append(float(step((x, a), gt)))
    assert int(m.transformer.step_counter(DEV)) == c0 + 3
    assert all(np.isfinite(losses)) and len(set(losses)) == 3, losses
    # the same counter value replays the same masks: the same loss, bit for bit
    m.transformer.step_counter(DEV).fill_(c0)
    assert float(step((x, a), gt)) == losses[0]


def test_trainer_runs_an_epoch_with_the_transformer(tmp_path, monkeypatch):
    """python -m vinet_amd.train --dataset synthetic --use_sound True --use_transformer True: one epoch (train, validate, save)"""
    from vinet_amd import train
    monkeypatch.chdir(tmp_path)
    train.main(["--dataset", "synthetic", "--use_sound", "True", "--use_transformer", "True", "--no_epochs", "1",
                "--synthetic_steps", "4", "--batch_size", "2", "--no_workers", "0", "--model_val_path", str(tmp_path / "tf.pt")])
    sd = torch.load(tmp_path / "tf.pt", map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    assert any(k.endswith("transformer.transformer_encoder.layers.2.norm2.bias") for k in sd)


def test_audio_visual_inference_with_the_transformer(tmp_path):
    """generate_result_audio_visual's flow with --use_transformer on a synthetic DIEM-like tree: one map per frame"""
    import wave
    from PIL import Image
    from vinet_amd import generate_result_audio_visual as AV
    from vinet_amd import model as VM
    E.set_default_dtype("bf16")
    args = AV.build_parser().parse_args(["--use_sound", "True", "--use_transformer", "True", "--transformer_in_channel", "32", "--batch", "2"])
    m = VM.VideoAudioSaliencyModel(use_transformer=args.use_transformer, transformer_in_channel=args.transformer_in_channel,
                                   num_encoder_layers=args.num_encoder_layers, nhead=args.nhead, num_clips=32).eval()
    sd = synth.synth_state_dict(m.state_dict(), 5)
    sd["transformer.pos_encoder.pe"] = m.state_dict()["transformer.pos_encoder.pe"]
    m.load_state_dict(sd)
    m = m.to(DEV)
    rng = np.random.default_rng(8)
    N, h, w, fps, Fs = 63, 45, 80, 25, 22050
    root = tmp_path / "data"
    for d in ("fold_lists", "video_frames/DIEM/v1", "video_audio/DIEM/v1", "annotations/DIEM/v1/maps"):
        os.makedirs(root / d)
    (root / "fold_lists" / "DIEM_list_test_fps.txt").write_text("v1 %d %d\n" % (N, fps))
    u8 = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    for i in range(N):
        Image.fromarray(u8[i]).save(root / "video_frames" / "DIEM" / "v1" / ("%04d.png" % (i + 1)))
        Image.fromarray(u8[i, :, :, 0]).save(root / "annotations" / "DIEM" / "v1" / "maps" / ("%04d.png" % (i + 1)))
    pcm = rng.integers(-20000, 20000, int(Fs * N / fps), dtype=np.int16)
    with wave.open(str(root / "video_audio" / "DIEM" / "v1" / "v1.wav"), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(Fs); f.writeframes(pcm.tobytes())
    args.path_indata, args.save_path = str(root), str(tmp_path / "out")
    assert AV.validate(args, m, DEV) == N
    files = sorted(os.listdir(tmp_path / "out" / "v1"))
    assert len(files) == N
    img = np.asarray(Image.open(tmp_path / "out" / "v1" / files[-1]))
    assert img.shape[:2] == (h, w) and img.max() > img.min()
