"""Full-shape replays of vinet_bn_bwd_reduce_pool / vinet_bn_bwd_apply_pool for the coverage gate of tests/test_gpu_headline_step.py:
importing this module registers them in headline_step.NONCONV (tests/test_gpu_bn_pool_kernels.py imports it, so any run that
collects tests/ replays the two entry points at the largest extent of the benchmarked step).  The reference is the composition at
that extent: vinet_maxpool3d_bwd into a copy of the gradient buffer, then vinet_bn_bwd_apply in place (the fused result must equal it
bit for bit, over the whole buffer) or vinet_bn_bwd_reduce (per-channel totals within replay_bn_bwd's bound, 2^-16 of sum |terms|)."""
import ctypes as C

import torch

from tests import headline_step as H
from vinet_amd import _lib as L


def replay_bn_bwd_pool(e, seed):
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    pd, dpc, _, gc_, acc, zc, dt, fwd = e.args[:8]
    tdt, Cc = H.TDT[dt], zc.C
    dxc = e.args[12] if e.name == "vinet_bn_bwd_apply_pool" else gc_
    dpb, dpc = H._fresh(dpc, tdt, gen, dev)
    zb, zc = H._fresh(zc, tdt, gen, dev)
    gb, gc_ = H._fresh(gc_, tdt, gen, dev)
    am = torch.randint(0, 9, (dpc.B * dpc.T * dpc.H * dpc.W * Cc,), dtype=torch.uint8, device=dev, generator=gen)
    fs, fb = H.vec(Cc, "scale", gen, dev, True), H.vec(Cc, "shift", gen, dev, True)
    f = L.CAffine(fs.data_ptr(), fb.data_ptr(), fwd.relu)
    mean, inv = H.vec(Cc, "shift", gen, dev, True), H.vec(Cc, "scale", gen, dev, True)
    st = torch.cuda.current_stream().cuda_stream
    errs = []
    # the composition, in a copy of the gradient buffer
    rb = H.tensor_buf(gc_, tdt, dev)
    rb.t.copy_(gb.t)
    rc_ = L.CTensor.from_buffer_copy(gc_)
    rc_.ptr = rb.ptr
    assert lib.vinet_maxpool3d_bwd(C.byref(pd), C.byref(dpc), am.data_ptr(), C.byref(rc_), acc, st) == 0, lib.vinet_last_error()
    if e.name == "vinet_bn_bwd_apply_pool":
        c1, c2 = H.vec(Cc, "shift", gen, dev, True), H.vec(Cc, "shift", gen, dev, True)
        assert lib.vinet_bn_bwd_apply(C.byref(rc_), C.byref(zc), dt, f, mean.data_ptr(), inv.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                      C.byref(rc_), st) == 0, lib.vinet_last_error()
        assert dxc.ptr == e.args[3].ptr, "the step runs the apply pass in place"
        rc = lib.vinet_bn_bwd_apply_pool(C.byref(pd), C.byref(dpc), am.data_ptr(), C.byref(gc_), acc, C.byref(zc), dt, f, mean.data_ptr(),
                                         inv.data_ptr(), c1.data_ptr(), c2.data_ptr(), C.byref(gc_), st)
        assert rc == 0, lib.vinet_last_error()
        torch.cuda.synchronize()
        n = H.span(gc_.B, gc_.T, gc_.H, gc_.W, gc_.C, gc_.ld, gc_.sB)
        a, b = gb.t[gb.lead:gb.lead + n].view(torch.int16), rb.t[rb.lead:rb.lead + n].view(torch.int16)
        if not torch.equal(a, b):
            errs.append("%r: %d elements differ from pool backward -> bn_bwd_apply" % (e, int((a != b).sum())))
        return errs
    rows = lib.vinet_stats_rows(C.byref(zc))
    P = torch.full((2, rows * 2 * Cc), float("nan"), dtype=torch.float32, device=dev)
    assert lib.vinet_bn_bwd_reduce(C.byref(rc_), C.byref(zc), dt, f, mean.data_ptr(), inv.data_ptr(), P[0].data_ptr(), st) == 0, lib.vinet_last_error()
    rc = lib.vinet_bn_bwd_reduce_pool(C.byref(pd), C.byref(dpc), am.data_ptr(), C.byref(gc_), acc, C.byref(zc), dt, f, mean.data_ptr(),
                                      inv.data_ptr(), P[1].data_ptr(), st)
    assert rc == 0, lib.vinet_last_error()
    torch.cuda.synchronize()
    s = torch.zeros((4, Cc), dtype=torch.float64, device=dev)
    for b in range(zc.B):
        g, xh = H._bn_terms(H.view_of(rb, rc_)[b].reshape(-1, Cc).double(), H.view_of(zb, zc)[b].reshape(-1, Cc).double(), fs, fb, fwd.relu, mean, inv, Cc)
        s[0] += g.sum(0)
        s[1] += (g * xh).sum(0)
        s[2] += g.abs().sum(0)
        s[3] += (g * xh).abs().sum(0)
    for which, tab in (("composition", P[0]), ("fused", P[1])):
        got = tab.view(rows, 2, Cc).double().sum(0)
        for k in range(2):
            if not bool(((got[k] - s[k]).abs() <= 2.0 ** -16 * s[k + 2] + 1e-6).all()):
                errs.append("%r (%s): sum %d: %s vs %s" % (e, which, k, got[k][:4].tolist(), s[k][:4].tolist()))
    return errs


H.NONCONV.setdefault("vinet_bn_bwd_reduce_pool", replay_bn_bwd_pool)
H.NONCONV.setdefault("vinet_bn_bwd_apply_pool", replay_bn_bwd_pool)
