"""Full-shape replays of vinet_decoder_tail_fwd and vinet_decoder_tail_bwd for the coverage gate of tests/test_gpu_headline_step.py:
importing this module registers them in headline_step.NONCONV (tests/test_gpu_decoder_tail.py imports it, so any run that collects
tests/ replays both entry points at the extent of the benchmarked step, 192 x 224 x 384).  The reference is the composition at that
extent on the same inputs (tests/decoder_tail_cases.py: conv_forward x2 + vinet_export_ncdhw; vinet_import_ncdhw, vinet_act_bwd x2
and the two data gradients), compared bit for bit over the whole tensors, with nothing outside the outputs written."""
import torch

from tests import decoder_tail_cases as DC
from tests import headline_step as H
from vinet_amd import _lib as L


def _problem(e, u, a6, kT, b_mid, seed):
    assert e.args[0] == H.BF16 and (u.T, u.C) == (kT, 32) and a6 is not None and (a6.B, a6.H, a6.W) == (u.B, u.H, u.W), repr(e)
    for t in (u, a6):
        assert t is None or (t.ld == t.C and t.sB == t.T * t.H * t.W * t.ld), "%r: a view the replay does not rebuild" % e
    case = DC.Case("headline", u.B, u.H, u.W, kT, bool(b_mid), True, "dense", "dense")
    return DC.Problem(case, torch.device("cuda:0"), seed, exact=False)


def _forward(p, ctx, errs, e):
    p.run_fwd(ctx)
    a6c, headc, planes = p.composed_fwd(ctx)
    torch.cuda.synchronize()
    if not DC.same_bits(p.out.t, planes[0]):
        errs.append("%r: the map differs from conv + conv + export in %d pixels" % (e, int((p.out.t != planes[0]).sum())))
    if not DC.same_bits(p.a6.t5(), a6c.torch5()):
        errs.append("%r: a6 differs from the conv's" % e)
    return a6c, headc


def replay_tail_fwd(e, seed):
    L.load()
    _, u, kT, _, b_mid, _, _, a6 = e.args[:8]
    p = _problem(e, u, a6, kT, b_mid, seed)
    errs = []
    _forward(p, p.ctx(), errs, e)
    for name in ("a6", "out"):
        if not getattr(p, name).outside_untouched():
            errs.append("%r: bytes outside %s changed" % (e, name))
    if not bool((p.dz.bits() == DC.BF_FILL).all() and (p.du.bits() == DC.BF_FILL).all()):
        errs.append("%r: the forward wrote to a gradient buffer" % e)
    return errs


def replay_tail_bwd(e, seed):
    L.load()
    a6, kT = e.args[9], e.args[10]
    du = e.args[15]
    p = _problem(e, du, a6, kT, None, seed)
    ctx, errs = p.ctx(), []
    a6c, headc = _forward(p, ctx, errs, e)
    p.g.t.normal_(0.0, 1e-3, generator=p.gen)
    p.run_bwd(ctx)
    dyc, dzc, duc = p.composed_bwd(ctx, a6c, headc)
    torch.cuda.synchronize()
    for name, got, ref in (("dy_head", p.dy, dyc), ("dz6", p.dz, dzc), ("du", p.du, duc)):
        if not DC.same_bits(got.t5(), ref.torch5()):
            errs.append("%r: %s differs from the composition in %d elements" % (e, name, int((got.t5().view(torch.int16) != ref.torch5().view(torch.int16)).sum())))
    if not bool((duc.torch5()[-1].float() != 0).any()):
        errs.append("%r: an all-zero gradient checks nothing" % e)
    del dyc, dzc, duc, a6c, headc
    for name in ("dy", "dz", "du", "a6", "out", "g"):
        if not getattr(p, name).outside_untouched():
            errs.append("%r: bytes outside %s changed" % (e, name))
    return errs


H.NONCONV.setdefault("vinet_decoder_tail_fwd", replay_tail_fwd)
H.NONCONV.setdefault("vinet_decoder_tail_bwd", replay_tail_bwd)
