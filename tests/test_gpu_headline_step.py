"""Every kernel launch of the benchmarked training step, at full shape, against float64 (tests/headline_step.py).

The kernel tests (test_gpu_kernels.py) check each family at small shapes and forced routes; this module records the
launches of ONE real step -- ViNet-32, 224 x 384, kldiv, fused Adam, weight-gradient side stream, 192 clips in bf16 (the
bench headline) and 64 clips in fp32s (bench --full's parity_path) -- and replays each distinct conv, data-gradient and
weight-gradient launch with the captured geometry on fresh seeded data:

  * the replayed descriptor must reach the kernel instance the step used (the route itself is under test);
  * integer data: the stored values must equal the float64 reference bit for bit, on batch items 0, 1, B-2, B-1 and every
    item holding element 2^31 or 2^32 of the largest tensors; storage outside the output view must keep its sentinel;
    weight gradients from a sparse dy (first / last row of every 32-row block and of every image row, a random subset) so
    that every sum stays exact -- the fused BatchNorm-backward form with non-trivial mean, invstd, c1 and c2 chosen so that
    the rows without dy cancel exactly; the comparison must reject three deliberately wrong references per entry (a
    dropped K chunk, the route's last M tile dropped, a one-voxel shift);
  * statistics and BatchNorm-backward partial sums: per-channel totals against float64 sums over the stored outputs,
    under stated bounds (they sum squares over millions of rows and are not exact);
  * one realistic-data pass (normal data, items 0 and B-1) for forward / data-gradient launches under a stated bound;
  * the largest extent of the big non-conv launches (BatchNorm backward, pooling, upsampling, copies, the input import);
  * a coverage gate: every (entry point, kernel) of the step is replayed here or exempted below with a reason.
Wall time and peak HBM are printed (run with -s)."""
import time

import pytest
import torch

from tests import headline_step as H
from vinet_amd import _lib as L

pytestmark = pytest.mark.gpu

# entry points of the step that are not replayed here, with the reason
EXEMPT = {
    "vinet_adam_step": "flat elementwise over the parameters (~30 M floats, far from 2^31); test_gpu_kernels / test_gpu_model check it",
    "vinet_loss_fwd": "per-sample fp64 reductions over 224 x 384 maps; test_gpu_kernels checks them at these map sizes",
    "vinet_loss_bwd": "same extents as vinet_loss_fwd; test_gpu_kernels",
    "vinet_pack_weights": "weight-sized (< 4 M elements); test_gpu_kernels test_pack_unpack",
    "vinet_pack_weights_multi": "weight-sized; test_gpu_kernels test_pack_weights_multi_matches_single_packs",
    "vinet_unpack_wgrad": "weight-sized; test_gpu_kernels test_pack_unpack",
    "vinet_unpack_wgrad_multi": "weight-sized; test_gpu_kernels test_unpack_wgrad_multi_matches_single_unpacks",
    "vinet_bn_finalize": "per-channel (<= 1024 channels x <= 256 folded rows); test_gpu_kernels test_bn_kernels",
    "vinet_bn_bwd_finalize": "per-channel; test_gpu_kernels test_bn_kernels",
    "vinet_bn_partials_fold": "partials tables (<= 10^5 rows x 64); test_gpu_kernels test_bn_partials_fold at 5000 x 64",
    "vinet_fill_f32": "a fill",
    "vinet_export_ncdhw": "the 224 x 384 output map only (B x 1 channel)",
    "vinet_import_ncdhw": "the ground-truth map only (B x 224 x 384 x 1)",
    "vinet_act_bwd": "decoder head only (1-channel maps at 224 x 384); test_gpu_kernels test_act_bwd",
    "vinet_channel_sum": "decoder bias gradients over the decoder's tensors; test_gpu_kernels",
    "vinet_upsample2x_bwd": "same index math as vinet_upsample2x_bwd_relu, which is replayed at its largest extent here",
    "vinet_debug_spin": "a test aid that touches no memory",
}

@pytest.fixture(scope="module", params=sorted(H.CONFIGS), ids=sorted(H.CONFIGS))
def step(request):
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    entries, peak = H.census(request.param)
    n_conv = sum(e.name in H.CONV_ENTRIES for e in entries)
    n_wg = sum(e.name in H.WGRAD_ENTRIES for e in entries)
    print("\n[census %s] %d distinct launches (%d conv / data gradient, %d weight gradient) of %d; step peak %.1f GB; %.1f s"
          % (request.param, len(entries), n_conv, n_wg, sum(e.count for e in entries), peak, time.perf_counter() - t0))
    torch.cuda.reset_peak_memory_stats()
    yield request.param, entries
    print("[replay %s] peak HBM of the replays %.1f GB" % (request.param, torch.cuda.max_memory_allocated() / 1e9))
    torch.cuda.empty_cache()


def _report(tag, results):
    bad = [m for r in results for m in r.errors]
    weak = [m for r in results for m in r.selftest]
    exact = sum(1 for r in results if r.exact and not r.errors)
    print("[%s] %d replays, %d item checks; %d entirely bit-exact, %d with a toleranced part (statistics / partial sums / "
          "sigmoid / realistic data)" % (tag, len(results), sum(r.checked for r in results), exact, len(results) - exact))
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:20]))
    assert not weak, "the check accepted deliberately wrong references:\n%s" % "\n".join(weak[:20])


def test_census_holds_the_expected_routes(step):
    cfg, entries = step
    names = {e.kname for e in entries if e.kname}
    assert all(e.kname for e in entries if e.name in H.CONV_ENTRIES + H.WGRAD_ENTRIES), "a launch without a kernel name"
    if cfg == "bf16":
        want = ["conv_ht_kernel<96,t,pre>", "conv_pp_kernel<192>", "conv_pp_kernel<256>", "conv_pw_kernel<", "conv_tsd_kernel",
                "conv_hs_kernel", "conv_ts_kernel<pre>", "conv_wgrad_ts_kernel", "conv_wgrad_tf_kernel", "conv_wgrad_rs_kernel",
                "conv_wgrad_pp_kernel", "conv_wgrad_dma_kernel", "conv_wgrad_hs_kernel<bn_bwd>", "wgrad_skinny_kernel"]
    else:
        want = ["conv_dma3_kernel", "conv_ht3_kernel<", "conv_ts3_kernel", "conv_hs3_kernel", "conv_wgrad_hs_kernel", "conv_wgrad_tf_kernel"]
    missing = [w for w in want if not any(n.startswith(w) for n in names)]
    assert not missing, "routes missing from the %s step: %s (kernels seen: %s)" % (cfg, missing, sorted(names))


def test_conv_and_dgrad_launches_exact(step):
    cfg, entries = step
    results = []
    for i, e in enumerate(x for x in entries if x.name in H.CONV_ENTRIES):
        results.append(H.replay_conv(e, exact=True, seed=1000 + i))
    _report("%s conv exact" % cfg, results)


def test_conv_and_dgrad_launches_realistic(step):
    cfg, entries = step
    results = []
    for i, e in enumerate(x for x in entries if x.name in H.CONV_ENTRIES):
        results.append(H.replay_conv(e, exact=False, seed=2000 + i, selftest=False, only_items=(0, -1)))
    _report("%s conv realistic" % cfg, results)


def test_weight_gradient_launches_exact(step):
    cfg, entries = step
    results = []
    for i, e in enumerate(x for x in entries if x.name in H.WGRAD_ENTRIES):
        results.append(H.replay_wgrad(e, seed=3000 + i))
    _report("%s wgrad exact" % cfg, results)


def test_large_nonconv_launches(step):
    cfg, entries = step
    errs, done = [], []
    for i, (name, fn) in enumerate(sorted(H.NONCONV.items())):
        e = H.largest(entries, name)
        if e is None:
            continue
        errs += fn(e, 4000 + i)
        done.append("%s %s" % (name, e.site))
    print("[%s non-conv] %s" % (cfg, "; ".join(done)))
    assert not errs, "\n".join(errs[:20])


def test_coverage_gate(step):
    """every distinct (entry point, kernel) of the step is replayed above or exempted in EXEMPT"""
    cfg, entries = step
    replayed = set(H.CONV_ENTRIES + H.WGRAD_ENTRIES) | set(H.NONCONV)
    uncovered = sorted({(e.name, e.kname) for e in entries if e.name not in replayed and e.name not in EXEMPT})
    assert not uncovered, "launches of the %s step with neither a replay nor an exemption: %s" % (cfg, uncovered)
    unused = sorted(set(EXEMPT) - {e.name for e in entries})
    assert set(EXEMPT) <= set(L.SIGNATURES), "EXEMPT names an entry point the library does not have"
    print("[%s gate] exemptions not used by this step: %s" % (cfg, unused))
