"""What the engine launches, and what comes out, in one training step on the CPU model of the ABI -- as two digests per
configuration, for comparing two checkouts of the engine that must behave alike (a refactor): run this same file in both and
diff the printouts (profiles/grad_ledger_launches_vs_parent.txt).  No GPU is needed.

    python tools/launch_digest.py [--skip-avinet] [--device]

Per row: the number of launches, a digest of the ordered (entry point, tag) list, and a digest of the bits of every output, the
loss, the input gradient where there is one and every parameter gradient.  The library object is tests/abi_emulator.py with the
stubs of the keeping pool and of the fused BatchNorm-pool entry points (tests/test_pool_keep_engine.py), so that those routes
are taken.  The CPU model has no transformer entry points: the two transformer fusions cannot run on it and are listed as such.

The CPU model has no streams.  --device runs the three `vinet ... defaults` rows on the HIP device through the built library instead:
the launch digest then also folds in the stream of every launch, renamed to the order of its first appearance in the step (0, 1,
2 ...), so two checkouts agree only if they put every launch on the same stream.  The bits digest is printed but means little there:
the weight gradients are accumulated with atomics."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_bn_pool_host as BP                      # noqa: E402
from tests.test_pool_keep_engine import _Keeping               # noqa: E402
from vinet_amd import _lib as L                                # noqa: E402
from vinet_amd import engine as E                              # noqa: E402
from vinet_amd import loss, model, synth                       # noqa: E402


def _digest(items):
    h = hashlib.sha256()
    for it in items:
        h.update(it if isinstance(it, bytes) else repr(it).encode())
        h.update(b"\0")
    return h.hexdigest()[:16]


def _bits(tensors):
    return [t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes() for t in tensors]


DEVICE = None       # --device: torch.device("cuda")


def _logged(fn):
    """fn() -> tensors, under E.LAUNCH_LOG: (launches, launch digest, bits digest)"""
    log = E.LAUNCH_LOG = []
    try:
        vals = fn()
    finally:
        E.LAUNCH_LOG = None
    if DEVICE is None:
        return len(log), _digest([(n, t) for n, _, t in log]), _digest(_bits(vals))
    order = {}          # stream handle (the last argument of every launch) -> order of first appearance
    return len(log), _digest([(n, order.setdefault(getattr(st, "value", st), len(order)), t) for n, st, t in log]), _digest(_bits(vals))


def _vinet_step(dtype, audio=False, **cfg):
    """VideoSaliencyModel on 2 clips of 8 frames, 128 x 192 (tests/test_pool_keep_engine.py); audio: the bilinear audio-visual
    model on one clip of its only shape, 32 frames of 224 x 384"""
    old, old_dt = E.configure(**cfg), E.default_dtype()
    E.set_default_dtype(dtype)
    try:
        B, T, H, W = (1, 32, 224, 384) if audio else (2, 8, 128, 192)
        m = model.VideoAudioSaliencyModel() if audio else model.VideoSaliencyModel(num_clips=T)
        m.load_state_dict(synth.synth_state_dict(m.state_dict(), 11))
        m.train()
        x = synth.clip(B, T, H, W, 11).permute(0, 2, 1, 3, 4)
        gt = synth.gt_map(B, H, W, 11)
        if DEVICE is not None:
            m, x, gt = m.to(DEVICE), x.to(DEVICE), gt.to(DEVICE)

        def run():
            y = m(x, synth.audio(B, seed=11)) if audio else m(x)
            lo = loss.kldiv(y, gt)
            lo.backward()
            return [y, lo.reshape(1)] + [p.grad for p in m.parameters() if p.grad is not None]
        return _logged(run)
    finally:
        E.set_default_dtype({E.F32: "fp32", E.BF16: "bf16", E.F32S: "fp32s"}[old_dt])
        E.configure(**old)


def _tiny_step(late, option):
    """the two tiny nets of tests/test_bn_pool_host.py: SepConv -> pool -> conv, without and with a late second reader"""
    out = {}

    def run():
        out["names"], vals = BP._step(_Keeping(), late, option)
        return vals
    n, _, bits = _logged(run)            # (_step keeps a log of its own: the digest is over its names)
    return len(out["names"]), _digest(out["names"]), bits


ROWS = [("vinet bf16 defaults", lambda: _vinet_step("bf16"))]
ROWS += [("vinet bf16 %s=%d" % (k, v), lambda k=k, v=v: _vinet_step("bf16", **{k: v}))
         for k, v in (("dgrad_bn_stats", 0), ("dgrad_bn_stats", 2), ("pool_bwd_in_bn", 0), ("pool_keeps_skip", 0), ("share_skip_grad", 0),
                      ("upsample_bwd_relu", 0))]
ROWS += [("vinet fp32s defaults", lambda: _vinet_step("fp32s")), ("vinet fp32 defaults", lambda: _vinet_step("fp32"))]
ROWS += [("tiny net late=%d pool_bwd_in_bn=%d" % (late, o), lambda late=late, o=o: _tiny_step(bool(late), o)) for late in (0, 1) for o in (1, 0)]
ROWS += [("audio-visual (bilinear) bf16 defaults", lambda: _vinet_step("bf16", audio=True))]


def main():
    global DEVICE
    skip_av = "--skip-avinet" in sys.argv[1:]
    if "--device" in sys.argv[1:]:
        DEVICE = torch.device("cuda")
        L.load()
    print("%-44s %9s  %-16s  %-16s" % ("configuration", "launches", "launch digest", "bits digest"))
    for name, fn in ROWS:
        if skip_av and name.startswith("audio-visual"):
            continue
        if DEVICE is not None:
            if name.startswith("vinet") and name.endswith("defaults"):
                print("%-44s %9d  %-16s  %-16s" % ((name,) + fn()), flush=True)
            continue
        L._install_test_double(_Keeping())
        try:
            print("%-44s %9d  %-16s  %-16s" % ((name,) + fn()), flush=True)
        finally:
            L._install_test_double(None)
    if DEVICE is None:
        print("%-44s %9s  the CPU model has no vinet_transformer_* / vinet_token_* entry points" % ("transformer fusion, token-wise fusion", "-"))


if __name__ == "__main__":
    main()
