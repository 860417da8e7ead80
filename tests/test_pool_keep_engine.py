"""engine.POOL_KEEPS_SKIP in a whole training step: ViNet-8 on 2 clips of 128 x 192, bf16, with the option on and off.  The pools
behind the three decoder skips write the skips' slices of the decoder's T-concats (vinet_maxpool3d_keep), so exactly three
vinet_copy_affine launches disappear and nothing else changes: the same maps and loss bit for bit, the same parameter gradients
(on the GPU: within what runs WITHOUT the option differ by among themselves -- the split-K atomics order their sums by chance), and
the 1x3x3/s2 pool backwards are still formed inside the BatchNorm backward (engine.POOL_BWD_IN_BN).

The CPU variant runs on the CPU model of the ABI (tests/abi_emulator.py) extended by this file's stubs of the keeping pool (the
model's own pool + copy) and by the stubs of the fused BatchNorm-pool entry points (tests/bn_pool_cases.py): what the engine
launches is the point there.  The GPU variant runs the library."""
import collections

import pytest
import torch

from tests.abi_emulator import AbiEmulator, _deref
from tests.bn_pool_cases import FusedPoolStubs
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import loss, model, synth

SKIP_POOLS = 3


class _Keeping(FusedPoolStubs, AbiEmulator):
    def vinet_maxpool3d_keep_ok(self, pd, x, pre, y, argmax, keep):
        d, x, y, keep = _deref(pd), _deref(x), _deref(y), _deref(keep)
        k, s, p = (d.kT, d.kH, d.kW), (d.sT, d.sH, d.sW), (d.pT, d.pH, d.pW)
        return int(d.dtype == E.BF16 and x.C % 8 == 0 and (keep.B, keep.T, keep.H, keep.W, keep.C) == (x.B, x.T, x.H, x.W, x.C)
                   and all(kk >= pp + ss for kk, ss, pp in zip(k, s, p))
                   and all(o * ss >= i for o, ss, i in zip((y.T, y.H, y.W), s, (x.T, x.H, x.W))))

    def vinet_maxpool3d_keep(self, pd, x, pre, y, argmax, keep, stream):
        if not self.vinet_maxpool3d_keep_ok(pd, x, pre, y, argmax, keep):
            return -1
        rc = self.vinet_maxpool3d(pd, x, pre, y, argmax, stream)
        return rc or self.vinet_copy_affine(x, _deref(pd).dtype, pre, keep, _deref(pd).dtype, 0, stream)


def _step(dev, option):
    """one training step -> (launch names, [map, loss] as bits, parameter gradients)"""
    old = E.configure(pool_keeps_skip=option)
    old_dt = E.default_dtype()
    E.set_default_dtype("bf16")
    log = E.LAUNCH_LOG = []
    try:
        B, T, H, W = 2, 8, 128, 192
        m = model.VideoSaliencyModel(num_clips=T)
        m.load_state_dict(synth.synth_state_dict(m.state_dict(), 11))
        m = m.to(dev).train()
        x = synth.clip(B, T, H, W, 11).permute(0, 2, 1, 3, 4).to(dev)
        gt = synth.gt_map(B, H, W, 11).to(dev)
        y = m(x)
        lo = loss.kldiv(y, gt)
        lo.backward()
        grads = [p.grad.detach().float().cpu() for p in m.parameters()]
        assert all(bool(torch.isfinite(g).all()) for g in grads)
        return [n for n, _, _ in log], [y.detach().cpu().view(torch.int32), lo.detach().cpu().reshape(1).view(torch.int32)], grads
    finally:
        E.LAUNCH_LOG = None
        E.set_default_dtype({E.F32: "fp32", E.BF16: "bf16", E.F32S: "fp32s"}[old_dt])
        E.configure(**old)


def _check(dev, off_runs):
    names_on, out_on, g_on = _step(dev, 1)
    offs = [_step(dev, 0) for _ in range(off_runs)]
    names_off, out_off, g_off = offs[0]
    # forward: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(out_on, out_off)), "map or loss changed with pool_keeps_skip"
    # launches: three copies fewer, the three pools behind the skips in their keeping form, nothing else
    on, off = collections.Counter(names_on), collections.Counter(names_off)
    assert on["vinet_maxpool3d_keep"] == SKIP_POOLS and off["vinet_maxpool3d_keep"] == 0
    assert off - on == collections.Counter(vinet_copy_affine=SKIP_POOLS, vinet_maxpool3d=SKIP_POOLS), off - on
    assert on - off == collections.Counter(vinet_maxpool3d_keep=SKIP_POOLS), on - off
    renamed = ["vinet_maxpool3d" if n == "vinet_maxpool3d_keep" else n for n in names_on]
    it = iter(names_off)
    assert all(any(n == m_ for m_ in it) for n in renamed), "the launches that remain changed their order"
    # the 1x3x3/s2 pool backwards still go into the BatchNorm backward behind them
    for n in ("vinet_bn_bwd_reduce_pool", "vinet_bn_bwd_apply_pool", "vinet_maxpool3d_bwd"):
        assert on[n] == off[n], (n, on[n], off[n])
    assert on["vinet_bn_bwd_apply_pool"] >= 1, "no pool backward was deferred: _pool_bwd_defers"
    # gradients: within what the runs WITHOUT the option differ by among themselves.  The atomics' chance ordering perturbs an
    # fp32 sum by rounding errors relative to the sum's size, so differences are measured per parameter relative to that
    # parameter's largest gradient, and the bound is the largest such figure anywhere among the option-off runs (three runs, three
    # pairs, every parameter: ~900 samples of the noise against the ~300 it is then held against); bit-equal off runs (the CPU
    # model) leave a bound of zero.  A wrong skip would show at 1e-2 and above.
    def rel(a, b, i):
        return float((a[i] - b[i]).abs().max()) / max(float(g_off[i].abs().max()), 1e-30)
    spread = max([rel(a[2], b[2], i) for k, a in enumerate(offs) for b in offs[k + 1:] for i in range(len(g_on))] or [0.0])
    worst = max(rel(g_on, g_off, i) for i in range(len(g_on)))
    print("largest relative gradient difference: %g with the option against %g among %d runs without" % (worst, spread, len(offs)))
    assert worst <= spread, "gradients: |on - off| = %g of the largest gradient, the runs without the option differ by %g" % (worst, spread)
    # ... and over all parameters at once, where a parameter whose whole gradient is noise cannot set the scale: the L2 norm of the
    # difference, against twice the largest among the runs without the option (a sum over 3e7 elements varies by a few per cent
    # from draw to draw, not by a factor)
    def l2(a, b):
        return sum(float(((u - v).double() ** 2).sum()) for u, v in zip(a, b)) ** 0.5
    spread2 = max([l2(a[2], b[2]) for k, a in enumerate(offs) for b in offs[k + 1:]] or [0.0])
    d2 = l2(g_on, g_off)
    print("L2 of the gradient difference: %g with the option against %g among the runs without; |gradient| = %g" % (d2, spread2, l2(g_off, [0 * g for g in g_off])))
    assert d2 <= 2 * spread2, "gradients: ||on - off|| = %g, the runs without the option differ by %g" % (d2, spread2)
    print("%s: %d launches with the option, %d without" % (dev, len(names_on), len(names_off)))


def test_training_step_on_the_model_of_the_abi():
    L._install_test_double(_Keeping())
    try:
        _check(torch.device("cpu"), 1)
    finally:
        L._install_test_double(None)


@pytest.mark.gpu
def test_training_step_on_the_library():
    L.load()
    _check(torch.device("cuda:0"), 3)
