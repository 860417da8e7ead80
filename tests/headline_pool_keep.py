"""Full-shape replay of vinet_maxpool3d_keep for the coverage gate of tests/test_gpu_headline_step.py: importing this module
registers it in headline_step.NONCONV (tests/test_gpu_pool_keep_kernels.py imports it, so any run that collects tests/ replays the
entry point at the largest extent of the benchmarked step).  The reference is the composition at that extent, on the same inputs:
vinet_maxpool3d for y and the argmax (bit for bit, over the whole buffers), vinet_copy_affine for `keep` (equal as numbers at every
element; bits may differ in the sign of a zero only, and those are counted), and nothing outside y, keep and the argmax written."""
import ctypes as C

import torch

from tests import headline_step as H
from vinet_amd import _lib as L

KEEP_FILL = 0x7FC1          # bf16 bits of a NaN with a payload: integer inputs cannot produce it


def replay_pool_keep(e, seed):
    lib, dev = L.get(), torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    pd, xc0, pre, yc0, am0, kc0 = e.args[:6]
    assert pd.dtype == H.BF16
    tdt = H.TDT[pd.dtype]
    st = torch.cuda.current_stream().cuda_stream
    xb, xc = H._fresh(xc0, tdt, gen, dev)
    Cc = xc.C
    ps = H.vec(Cc, "scale", gen, dev, True) if pre.scale else None
    pb = H.vec(Cc, "shift", gen, dev, True) if pre.shift else None
    a = L.CAffine(ps.data_ptr() if ps is not None else None, pb.data_ptr() if pb is not None else None, pre.relu)
    nam = yc0.B * yc0.T * yc0.H * yc0.W * yc0.C
    got = {}
    for which in ("composition", "fused"):
        yb, yc = H._fresh(yc0, tdt, gen, dev, fill=H.SENTINEL)
        kb, kc = H._fresh(kc0, tdt, gen, dev, fill=H.SENTINEL)
        kb.t.view(torch.int16).fill_(KEEP_FILL)
        am = torch.full((nam + 32,), 255, dtype=torch.uint8, device=dev) if am0 else None
        amp = am.data_ptr() + 16 if am is not None else None
        if which == "fused":
            assert lib.vinet_maxpool3d_keep_ok(C.byref(pd), C.byref(xc), a, C.byref(yc), amp, C.byref(kc)) == 1, lib.vinet_last_error()
            assert lib.vinet_maxpool3d_keep(C.byref(pd), C.byref(xc), a, C.byref(yc), amp, C.byref(kc), st) == 0, lib.vinet_last_error()
        else:
            assert lib.vinet_maxpool3d(C.byref(pd), C.byref(xc), a, C.byref(yc), amp, st) == 0, lib.vinet_last_error()
            assert lib.vinet_copy_affine(C.byref(xc), pd.dtype, a, C.byref(kc), pd.dtype, 0, st) == 0, lib.vinet_last_error()
        got[which] = (yb, kb, kc, am)
    torch.cuda.synchronize()
    errs = []
    (yr, kr, krc, amr), (yf, kf, kfc, amf) = got["composition"], got["fused"]
    if not torch.equal(yf.t.view(torch.int16), yr.t.view(torch.int16)):
        errs.append("%r: y (or the bytes around it) differs from vinet_maxpool3d" % e)
    if amr is not None and not torch.equal(amf, amr):
        errs.append("%r: argmax (or its guards) differs from vinet_maxpool3d" % e)
    fb, rb = kf.t.view(torch.int16), kr.t.view(torch.int16)
    if bool((H.view_of(kf, kfc).view(torch.int16) == KEEP_FILL).any()):
        errs.append("%r: elements of keep were never written" % e)
    diff = fb != rb
    ndiff = int(diff.sum())
    if ndiff:
        zeros = int((diff & ((fb & 0x7FFF) == 0) & ((rb & 0x7FFF) == 0)).sum())
        print("%r: %d of %d keep elements differ from vinet_copy_affine in the sign of a zero" % (e, zeros, fb.numel()))
        if zeros != ndiff:
            errs.append("%r: keep differs from vinet_copy_affine in %d elements beyond the sign of a zero" % (e, ndiff - zeros))
    del diff
    H.view_of(kf, kfc).view(torch.int16).fill_(KEEP_FILL)
    if bool((fb != KEEP_FILL).any()):
        errs.append("%r: elements outside keep changed" % e)
    return errs


H.NONCONV.setdefault("vinet_maxpool3d_keep", replay_pool_keep)
