"""tests/decoder_tail_cases.py without a GPU: what the case table claims to cover, the float64 reference against its own wrong
variants, the real library's refusals (its argument checks run on host memory, before any launch), the kernels' occupancy as the
compiler reports it, and the engine on the CPU model of the ABI, which has no fused entry points and so takes the unfused path."""
import json
import os

import pytest
import torch

from tests import decoder_tail_cases as DC
from tests.abi_emulator import AbiEmulator
from vinet_amd import _lib as L
from vinet_amd import engine as E
from vinet_amd import loss, model, synth


def test_the_case_table_covers_what_it_says():
    cs = DC.CASES
    assert len({c.id for c in cs}) == len(cs)
    assert {c.kT for c in cs} == {2, 3, 4}
    for kT in (2, 3, 4):
        k = [c for c in cs if c.kT == kT]
        assert {c.mid_bias for c in k} == {True, False} and {c.uform for c in k} == {"dense", "tslice"}, kT
        assert {c.planes for c in k} == {"dense", "strided"} and {c.a6 for c in k} == {True, False}, kT
        assert {(c.B, c.H, c.W) for c in k} >= {(1, 3, 5), (2, 9, 29), (3, 17, 23)}, kT
    M = [c.B * c.H * c.W for c in cs]
    assert any(m < 16 for m in M) and any(m % 16 and m % 64 and m > 64 for m in M), "under one group; ragged beyond one workgroup"
    assert all(DC.groups_per_wave(c.B * c.H * c.W) == 1 for c in cs if max(c.H, c.W) < 100)
    walk = [c for c in cs if DC.groups_per_wave(c.B * c.H * c.W) > 1]
    assert walk and all(((c.B * c.H * c.W + 15) // 16) % DC.groups_per_wave(c.B * c.H * c.W) for c in walk), "a wave that stops early"


@pytest.mark.parametrize("case", [c for c in DC.CASES if c.a6 and c.H < 100][:6], ids=lambda c: c.id)
def test_the_reference_tells_wrong_references_apart(case):
    p = DC.Problem(case, torch.device("cpu"), 5, exact=True)
    a6, v, mag = DC.ref_fwd(p)
    assert mag < DC.EXACT
    assert not DC.same_bits(a6, DC.ref_fwd(p, drop_tap=True)[0])
    if case.B * case.H * case.W > 16:
        assert not DC.same_bits(a6, DC.shifted(a6)) and not DC.same_bits(a6, DC.last16_dropped(a6))
    # backward from dyadic map values and integer gradients
    p.a6.t5().copy_(a6)
    p.out.t.copy_(torch.randint(1, 4, p.out.t.shape, generator=p.gen).float() / 4)
    p.g.t.copy_(torch.randint(-2, 3, p.g.t.shape, generator=p.gen).float())
    dy, dz, du, mag = DC.ref_bwd(p)
    assert mag < DC.EXACT
    assert not DC.same_bits(du, DC.ref_bwd(p, drop_tap=True)[2])
    if case.B * case.H * case.W > 16:
        assert not DC.same_bits(du, DC.shifted(du)) and not DC.same_bits(du, DC.last16_dropped(du))
    assert bool((dy[..., 1:].float() == 0).all())


def test_refusals_on_the_library():
    lib = L.load()
    case = next(c for c in DC.CASES if c.kT == 2 and c.a6 and c.H == 9)
    p = DC.Problem(case, torch.device("cpu"), 1, exact=True)
    assert lib.vinet_decoder_tail_ok(*p.fwd_args(None, True)) == 1, lib.vinet_last_error()
    assert lib.vinet_decoder_tail_ok(*p.fwd_args(None, False)) == 1, lib.vinet_last_error()
    rows = DC.refusals(p, None)
    assert {"fp32", "kT = 5", "accumulate"} <= {w for w, _, _ in rows}
    for what, name, args in rows:
        rc = getattr(lib, name)(*args)
        assert rc == (0 if name.endswith("_ok") else -1), (what, name, rc)
        assert lib.vinet_last_error(), (what, name)


def test_kernels_hold_four_waves_per_simd():
    """the lean class: >= 4 waves per SIMD, nothing spilled (the compiler's own resource remarks, written by the build)"""
    from vinet_amd import build
    if not os.path.exists(build.RESOURCES):
        build.build(verbose=False)
    res = json.load(open(build.RESOURCES)).get("decoder_tail.hip")
    assert res, "no resource table for decoder_tail.hip: was the library built by vinet_amd.build?"
    kern = {k: v for k, v in res.items() if "decoder_tail_" in k and "_kernel" in k}
    assert len(kern) == 6, sorted(kern)
    for k, v in kern.items():
        assert v["occupancy"] >= 4 and v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)


def _step(fused):
    """one training step of ViNet-32 on the CPU model of the ABI -> the ordered (entry point, tag) list"""
    old = E.set_decoder_tail_fused(fused)
    old_dt = E.default_dtype()
    E.set_default_dtype("bf16")
    log = E.LAUNCH_LOG = []
    try:
        B, T, H, W = 1, 32, 32, 64
        m = model.VideoSaliencyModel(num_clips=T)
        m.load_state_dict(synth.synth_state_dict(m.state_dict(), 3))
        m = m.train()
        x = synth.clip(B, T, H, W, 3).permute(0, 2, 1, 3, 4)
        lo = loss.kldiv(m(x), synth.gt_map(B, H, W, 3))
        lo.backward()
        return [(n, t) for n, _, t in log]
    finally:
        E.LAUNCH_LOG = None
        E.set_default_dtype({E.F32: "fp32", E.BF16: "bf16", E.F32S: "fp32s"}[old_dt])
        E.set_decoder_tail_fused(old)


def test_the_engine_takes_the_unfused_path_on_a_library_without_the_entry_points():
    emu = AbiEmulator()
    assert not hasattr(emu, "vinet_decoder_tail_ok")
    L._install_test_double(emu)
    try:
        assert E.DECODER_TAIL_FUSED in (True, False)
        on, off = _step(True), _step(False)
    finally:
        L._install_test_double(None)
    assert on == off, "the switch changed the launches on a library that cannot serve it"
    assert not any(n.startswith("vinet_decoder_tail") for n, _ in on)
    names = [n for n, _ in on if not n.startswith("vinet_pack_weights")]
    # the seven launch kinds of the unfused tail are all there, in the forward's and the backward's order
    i_exp = names.index("vinet_export_ncdhw")
    assert names[i_exp - 2:i_exp] == ["vinet_conv3d", "vinet_conv3d"]
    i_imp = max(i for i, n in enumerate(names[:i_exp + 8]) if n == "vinet_import_ncdhw")
    assert i_imp > i_exp and names[i_imp + 1] == "vinet_act_bwd" and names.count("vinet_act_bwd") == 2


def test_the_switch_is_a_module_attribute_not_a_config_key():
    assert "DECODER_TAIL_FUSED" not in E._CONFIG and "decoder_tail_fused" not in E.config()
    old = E.set_decoder_tail_fused(False)
    try:
        assert E.DECODER_TAIL_FUSED is False and E.set_decoder_tail_fused(True) is False and E.DECODER_TAIL_FUSED is True
    finally:
        E.set_decoder_tail_fused(old)
