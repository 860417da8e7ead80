"""The pool backward folded into BatchNorm backward (engine.POOL_BWD_IN_BN), without a GPU: the refusals of the real library, and the
engine's defer / flush bookkeeping on the CPU model of the ABI (tests/abi_emulator.py), which has no vinet_bn_bwd_pool_ok -- so with
the option on the engine takes today's path there, and a library object that does have the predicate is a stub of this file's."""
import torch

from tests import bn_pool_cases as PC
from tests.abi_emulator import AbiEmulator
from tests.tail_cases import Side
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import synth
from vinet_amd.model_utils import BasicConv3d, SepConv3d, _Block

K133 = ((1, 3, 3), (1, 2, 2), (0, 1, 1))


def test_refusals_of_the_library():
    """the argument checks run before any launch: the real library answers them on host memory, without a device"""
    PC.check_refusals(Side(L.load()))


class _Net(_Block):
    """SepConv -> pool -> conv; `late`: a second consumer of the SepConv's output recorded BEFORE the pool, whose backward therefore
    writes that gradient AFTER the pool's"""
    compute_dtype = E.BF16

    def __init__(self, late, geo=K133):
        super().__init__()
        self.a = SepConv3d(8, 16, kernel_size=3, stride=1, padding=1)
        self.b = BasicConv3d(16, 8, kernel_size=1, stride=1)
        self.c = BasicConv3d(16, 8, kernel_size=1, stride=1) if late else None
        self.geo = geo

    def forward(self, x):
        return E.run_root(E.BlockBody(self, self._fwd, self._cpad), [x], list(self.parameters()))

    def _fwd(self, ctx, x):
        y = self.a._fwd(ctx, x)
        side = self.c._fwd(ctx, y) if self.c is not None else None
        out = self.b._fwd(ctx, E.maxpool_forward(ctx, y, *self.geo))
        return [out] if side is None else [out, side]


class _Fused(PC.FusedPoolStubs, AbiEmulator):
    """a library object WITH the predicate and the two entry points (stubs: tests/bn_pool_cases.py): what the engine calls is the point"""


def _step(lib, late, option, geo=K133, force_defer=False, monkeypatch=None):
    """one training step -> (launch names in order, every gradient and output as bits)"""
    L._install_test_double(lib)
    old = E.configure(pool_bwd_in_bn=option)
    if force_defer:
        monkeypatch.setattr(E, "_pool_bwd_defers", lambda *a: True)
    log = E.LAUNCH_LOG = []
    try:
        torch.manual_seed(0)
        net = _Net(late, geo).train()
        x = synth.normal("bn_pool_host_x", (2, 8, 2, 7, 10), 1).requires_grad_(True)
        outs = net(x)
        sum((o * synth.normal("bn_pool_host_p%d" % i, tuple(o.shape), 2 + i)).sum() for i, o in enumerate(outs)).backward()
        vals = [x.grad] + [p.grad for p in net.parameters()] + [o.detach() for o in outs]
        assert all(v is not None and bool(torch.isfinite(v).all()) for v in vals)
        return [n for n, _, _ in log], [v.clone().view(torch.int32) for v in vals]
    finally:
        E.LAUNCH_LOG = None
        E.configure(**old)
        L._install_test_double(None)
        if force_defer:
            monkeypatch.undo()


def _same(a, b):
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _count(names, what):
    return sum(n == what for n in names)


def test_the_model_without_the_predicate_takes_the_fallback():
    assert not hasattr(AbiEmulator(), "vinet_bn_bwd_pool_ok")
    on, off = _step(AbiEmulator(), False, 1), _step(AbiEmulator(), False, 0)
    assert on[0] == off[0] and _count(on[0], "vinet_maxpool3d_bwd") == 1 and _count(on[0], "vinet_bn_bwd_reduce_pool") == 0
    _same(on[1], off[1])


def test_the_last_writer_is_deferred_into_the_batchnorm_backward():
    names, vals = _step(_Fused(), False, 1)
    assert _count(names, "vinet_maxpool3d_bwd") == 0
    assert _count(names, "vinet_bn_bwd_reduce_pool") == 1 and _count(names, "vinet_bn_bwd_apply_pool") == 1
    # the fused pair stands where the layer's reduce and apply stood, around the same finalize
    i = names.index("vinet_bn_bwd_reduce_pool")
    assert names[i:i + 3] == ["vinet_bn_bwd_reduce_pool", "vinet_bn_bwd_finalize", "vinet_bn_bwd_apply_pool"]
    ref_names, ref = _step(_Fused(), False, 0)
    assert _count(ref_names, "vinet_maxpool3d_bwd") == 1 and _count(ref_names, "vinet_bn_bwd_reduce_pool") == 0
    assert len(ref_names) == len(names) + 1
    _same(vals, ref)


def test_a_late_second_reader_keeps_the_ordinary_pool_backward():
    """the pool is not the last writer of the gradient: the other consumer's data gradient accumulates after it"""
    names, vals = _step(_Fused(), True, 1)
    assert _count(names, "vinet_maxpool3d_bwd") == 1 and _count(names, "vinet_bn_bwd_reduce_pool") == 0 and _count(names, "vinet_bn_bwd_apply_pool") == 0
    ref_names, ref = _step(_Fused(), True, 0)
    assert names == ref_names
    _same(vals, ref)


def test_a_deferred_pool_backward_runs_before_anybody_else_touches_the_gradient(monkeypatch):
    """the last-writer proof replaced by `yes`: the late reader's data gradient asks for the gradient, which launches the deferred pool
    backward first, with the accumulate flag of the moment it was deferred -- the same launches and the same bits as without the option"""
    names, vals = _step(_Fused(), True, 1, force_defer=True, monkeypatch=monkeypatch)
    ref_names, ref = _step(_Fused(), True, 0)
    assert sorted(names) == sorted(ref_names) and _count(names, "vinet_maxpool3d_bwd") == 1 and _count(names, "vinet_bn_bwd_reduce_pool") == 0
    # (later than its place on the tape, but in front of the launch that asked: the late reader's data gradient)
    i = names.index("vinet_maxpool3d_bwd")
    assert i > ref_names.index("vinet_maxpool3d_bwd") and "vinet_conv3d" in names[i + 1:]
    _same(vals, ref)


def test_other_geometries_and_fp32_are_not_deferred():
    names, _ = _step(_Fused(), False, 1, geo=((1, 3, 3), (1, 1, 1), (0, 1, 1)))
    assert _count(names, "vinet_maxpool3d_bwd") == 1 and _count(names, "vinet_bn_bwd_reduce_pool") == 0
    old = _Net.compute_dtype
    _Net.compute_dtype = E.F32
    try:
        names, _ = _step(_Fused(), False, 1)
    finally:
        _Net.compute_dtype = old
    assert _count(names, "vinet_maxpool3d_bwd") == 1 and _count(names, "vinet_bn_bwd_reduce_pool") == 0
