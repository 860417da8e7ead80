"""vinet_decoder_tail_fwd / _bwd on a real MI355X: the cases of tests/decoder_tail_cases.py on libvinet_hip.so.

  * integer data: a6, dz6, du and dy_head equal a float64 reference rounded to bf16 bit for bit (every partial sum below 2^24,
    asserted), the map passes the sigmoid gate of tests/headline_step.py against a float64 sigmoid, and the comparison rejects
    three wrong references (a dropped tap, a one-pixel shift, the last 16 pixels dropped);
  * realistic data: every output equals, bit for bit, what today's launches leave on the same buffers (conv_forward x2 +
    vinet_export_ncdhw; vinet_import_ncdhw, vinet_act_bwd x2, the two data gradients): that equality is the contract;
  * nothing outside the outputs is written (sentinel fill);
  * one training step of ViNet-32 at 1 clip of 32 x 32 x 64 with engine.DECODER_TAIL_FUSED on and off: the same bits."""
import pytest
import torch

from tests import decoder_tail_cases as DC
from tests import headline_decoder_tail  # noqa: F401  (registers the two entry points in headline_step.NONCONV)
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import loss, model, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.id)
def test_integer_data_against_float64(case):
    L.load()
    p = DC.Problem(case, DEV, 100 + DC.CASES.index(case), exact=True)
    ctx = p.ctx()
    many = case.B * case.H * case.W > 16
    p.run_fwd(ctx)
    torch.cuda.synchronize()
    a6r, v, mag = DC.ref_fwd(p)
    assert mag < DC.EXACT, "exactness bound: sum |terms| = %g reaches 2^24" % mag
    assert DC.sigmoid_gate(p.out.t, v), "map against the float64 sigmoid"
    if not case.a6:
        assert bool((p.a6.bits() == DC.BF_FILL).all()), "a6 = NULL, yet a6's buffer changed"
        assert p.out.outside_untouched()
        return
    a6 = p.a6.t5().clone()
    assert DC.same_bits(a6, a6r), "a6: %d elements differ" % int((a6.view(torch.int16) != a6r.view(torch.int16)).sum())
    assert not DC.same_bits(a6, DC.ref_fwd(p, drop_tap=True)[0]), "the check accepted a reference with a dropped tap"
    if many:
        assert not DC.same_bits(a6, DC.shifted(a6r)) and not DC.same_bits(a6, DC.last16_dropped(a6r))
    # backward from dyadic map values {1/4, 1/2, 3/4} and integer gradients: every product and sum exact
    p.out.t.copy_(torch.randint(1, 4, p.out.t.shape, generator=p.gen, device=DEV).float() / 4)
    p.g.t.copy_(torch.randint(-2, 3, p.g.t.shape, generator=p.gen, device=DEV).float())
    p.run_bwd(ctx)
    torch.cuda.synchronize()
    dyr, dzr, dur, mag = DC.ref_bwd(p)
    assert mag < DC.EXACT
    dy, dz, du = p.dy.t5().clone(), p.dz.t5().clone(), p.du.t5().clone()
    assert DC.same_bits(dy, dyr), "dy_head"
    assert DC.same_bits(dz, dzr), "dz6"
    assert DC.same_bits(du, dur), "du: %d elements differ" % int((du.view(torch.int16) != dur.view(torch.int16)).sum())
    assert not DC.same_bits(du, DC.ref_bwd(p, drop_tap=True)[2]), "the check accepted a reference with a dropped tap"
    if many:
        assert not DC.same_bits(du, DC.shifted(dur)) and not DC.same_bits(du, DC.last16_dropped(dur))
        assert not DC.same_bits(dz, DC.shifted(dzr)) and not DC.same_bits(dy, DC.last16_dropped(dyr))
    assert bool((dz.float() != 0).any()) and bool((du.float() != 0).any()), "an all-zero gradient checks nothing"
    # write bounds
    assert bool((p.u.t5().view(torch.int16) != DC.BF_FILL).all())
    for name in ("a6", "dy", "dz", "du", "out", "g"):
        assert getattr(p, name).outside_untouched(), "bytes outside %s changed" % name


@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.id)
def test_realistic_data_against_the_composition(case):
    L.load()
    p = DC.Problem(case, DEV, 500 + DC.CASES.index(case), exact=False)
    ctx = p.ctx()
    p.run_fwd(ctx)
    a6c, headc, planes = p.composed_fwd(ctx)
    torch.cuda.synchronize()
    assert DC.same_bits(p.out.t.contiguous(), planes[0]), "map: %d pixels differ from conv + conv + export" % int((p.out.t != planes[0]).sum())
    assert bool(((planes[0] > 0) & (planes[0] < 1)).all())
    if not case.a6:
        return
    assert DC.same_bits(p.a6.t5(), a6c.torch5()), "a6"
    p.g.t.copy_(torch.empty(p.g.t.shape, device=DEV).normal_(0.0, 1e-3, generator=p.gen))
    p.run_bwd(ctx)
    dyc, dzc, duc = p.composed_bwd(ctx, a6c, headc)
    torch.cuda.synchronize()
    assert DC.same_bits(p.dy.t5(), dyc.torch5()), "dy_head (all 8 channels)"
    assert DC.same_bits(p.dz.t5(), dzc.torch5()), "dz6"
    assert DC.same_bits(p.du.t5(), duc.torch5()), "du"
    assert bool((duc.torch5().float() != 0).any())
    for name in ("a6", "dy", "dz", "du", "out"):
        assert getattr(p, name).outside_untouched(), "bytes outside %s changed" % name


def _step(fused):
    """one training step of ViNet-32, 1 clip of 32 x 32 x 64, bf16 -> launch names and the tensors of the tail, as bits"""
    old = E.set_decoder_tail_fused(fused)
    old_dt = E.default_dtype()
    E.set_default_dtype("bf16")
    log = E.LAUNCH_LOG = []
    ups, jobs = [], []
    orig_up, orig_job = E.upsample2x_forward, E._WgradJob.__init__

    def up(ctx, x, dst=None):
        r = orig_up(ctx, x, dst)
        ups.append((x, r))              # the last one: (convtsp4[3]'s output behind its ReLU, u)
        return r

    def job(self, ctx, plan, x, dy, *a):
        orig_job(self, ctx, plan, x, dy, *a)
        jobs.append((x, dy))            # in backward order: the head's (a6, dy_head), then the mid conv's (u, dz6)

    def bits(v):
        return v.torch5().contiguous().view(torch.int16).cpu()

    E.upsample2x_forward, E._WgradJob.__init__ = up, job
    try:
        B, T, H, W = 1, 32, 32, 64
        m = model.VideoSaliencyModel(num_clips=T)
        m.load_state_dict(synth.synth_state_dict(m.state_dict(), 7))
        m = m.to(DEV).train()
        x = synth.clip(B, T, H, W, 7).permute(0, 2, 1, 3, 4).to(DEV)
        gt = synth.gt_map(B, H, W, 7).to(DEV)
        y = m(x)
        lo = loss.kldiv(y, gt)
        lo.backward()
        torch.cuda.synchronize()
        (a6, dyh), (u, dz) = jobs[0], jobs[1]
        z5, u2 = ups[-1]
        assert u2 is u
        got = dict(a6=bits(a6.v), dy_head=bits(dyh), u=bits(u.v), dz6=bits(dz), du=bits(u.grad_view()), d5=bits(z5.grad_view()),
                   map=y.detach().cpu().view(torch.int32), loss=lo.detach().cpu().reshape(1).view(torch.int32))
        return [n for n, _, _ in log], got
    finally:
        E.upsample2x_forward, E._WgradJob.__init__ = orig_up, orig_job
        E.LAUNCH_LOG = None
        E.set_default_dtype({E.F32: "fp32", E.BF16: "bf16", E.F32S: "fp32s"}[old_dt])
        E.set_decoder_tail_fused(old)


def test_training_step_with_the_switch_on_and_off():
    """the map, the loss, a6, dz6, du, dy_head and the gradient arriving at convtsp4[3]'s output are bit-identical.  The weight
    gradients are NOT compared (atomics order their sums by chance: tests/test_pool_keep_engine.py shows what a bound on that
    noise costs); the operands of the tail's two weight-gradient launches are asserted identical instead."""
    L.load()
    names_on, on = _step(True)
    names_off, off = _step(False)
    assert names_on.count("vinet_decoder_tail_fwd") == 1 and names_on.count("vinet_decoder_tail_bwd") == 1
    assert not any(n.startswith("vinet_decoder_tail") for n in names_off)
    for n in ("vinet_export_ncdhw", "vinet_act_bwd"):
        assert n not in names_on and n in names_off, n
    assert names_off.count("vinet_conv3d") - names_on.count("vinet_conv3d") == 2 + 1 + 2, "two forward convs, the head's and two per-tap data gradients"
    assert names_on.count("vinet_conv3d_wgrad") == names_off.count("vinet_conv3d_wgrad")
    assert names_on.count("vinet_channel_sum") == names_off.count("vinet_channel_sum")
    for k in sorted(off):
        assert on[k].shape == off[k].shape and bool(torch.equal(on[k], off[k])), "%s differs with the fused tail" % k
    assert on["dy_head"].shape[-1] == 8 and on["a6"].shape[-1] == 32 and on["du"].shape[1:] == (2, 32, 64, 32)
    assert bool((on["du"] != 0).any()) and bool((on["d5"] != 0).any())
