"""The layout and weight-pack kernels of csrc/layout.hip on a real MI355X against the references of tests/layout_cases.py (gates and
their derivations: that module's docstring).  tests/test_layout_cases_host.py runs the same cases through the CPU model of the ABI.

Which case reaches which kernel (pack and unpack case ids are `<tag>-<type>` and `<tag>-flags<n>`; every such case runs the paths
single / tiled / elementwise, i.e. vinet_pack_weights per job, then the multi call with pack_tiled = 1 and with pack_tiled = 0; the
tile shape of every job and the route of every copy are worked out by the mirrors of layout_cases and asserted in the host test):

  pack_weights_kernel<f32 | bf16 | f32s>         path single of taps1 ... taps257 and misc (not the side-by-side jobs: only a table has `ld`)
  pack_weights_multi_kernel<f32 | bf16 | f32s>   path elementwise of every pack case; path tiled of njobs1025 (past PT_MAXJOBS)
  pack_weights_tiled_kernel<f32 | bf16 | f32s>   path tiled: taps1, taps27, taps32 (256 pairs: forward 8 x 32, transposed 32 x 8), taps33, taps64
                                                 (128 pairs: 4 x 32, 16 x 8), taps65, taps128 (64 pairs: 2 x 32, 8 x 8 -- never launched by a
                                                 kernel test before), taps129, taps256 (32 pairs: 1 x 32, 4 x 8 -- neither), taps257 (the
                                                 element-wise branch inside the tiled launch); misc (both stems, side-by-side jobs at
                                                 col 0, 32, 160, 272, one with two taps; for f32s too, which no test packed side by side
                                                 before); njobs1 ... njobs1024 (per = 1, 2 with a ragged last thread, 4 = the cap); units
                                                 (2085 units on 2048 workgroups)
  unpack_wgrad_kernel                            path single of the unpack cases, flags 0 ... 3
  unpack_wgrad_multi_kernel                      path elementwise; path tiled of njobs1025
  unpack_wgrad_tiled_kernel                      path tiled of the same tags as the tiled pack (forward jobs only), flags 0 ... 3
  import_ncdhw_kernel<float | bf16>              test_import, ids import-*: 1, 255, 256, 257 voxels, an extent of 1 in T, H, W, C = 1 ... 5 into
                                                 4 or 8 channels, four view forms, a permuted source and one with sc = st = 0
  import_pad_kernel<float | bf16>                test_import, ids import_pad-*: pads (0, 0), (3, 3), (0, 5), flush and short of the far edge, a
                                                 1 x 1 source, a row longer than a block, the folded stem's geometry for odd and even W
  export_ncdhw_kernel<float | bf16>              test_export: store and accumulate, three affine forms, NCDHW and [C, B, ...] destinations that
                                                 are channel slices of a sentinel-filled tensor
  copy_affine_kernel<TI, TO>, four pairs         test_copy, tags quad (1 ... 258 quads), ptr8mod16 / ld_c_plus4 / sB4mod8 / sB_alone (bf16 at 65 536 voxels,
                                                 off the 8-channel grid for one reason), seam at 65 535 voxels, pairs (the other pairs at 65 536)
  copy_affine8_kernel<bf16, bf16>                test_copy, tag seam at 65 536, + 1, + vb - 1, + vb + 1 voxels, C = 8, 24, 200 (R = 256, 85, 10: idle
                                                 threads), one of C = 512; in place and between slices
  split_bf16_kernel                              test_split: 1, 255, 257 quads, planes of different ld, one a T slice
  wgrad_skinny_kernel                            tests/test_gpu_kernels.py::test_conv3d_wgrad_skinny, now with Cin = 16 (G = 2)
  (unfold1d_kernel, fill_f32_kernel: tests/test_gpu_tail_kernels.py.)

NOT COVERED: the doubling of copy_affine8's voxels per block past 16 384 blocks, which needs about 1 GB of tensors; C > 2048, which
takes two group passes and is in no net; element-wise launches at or past 2^31 items; vinet_debug_spin.  The refusals are asked for
their return value only, never launched."""
import pytest

from tests import gpu_report
from tests import layout_cases as LC
from tests.test_gpu_kernels import _dev, _lib, _stream

pytestmark = pytest.mark.gpu

_WORST = {}      # family -> {measure: (worst value, case)}
_RUN = {}        # kernel -> cases that reached it and passed their gates
_BITS = {}       # family -> elements compared bit for bit (all equal: a difference fails the case)


def _side():
    return LC.Side(_lib(), _dev(), _stream())


def _note(family, case, errs, kernels=()):
    for k in kernels:
        _RUN[k] = _RUN.get(k, 0) + 1
    slot = _WORST.setdefault(family, {})
    _BITS[family] = _BITS.get(family, 0) + int(errs.get("elements", 0))
    for k, v in errs.items():
        if isinstance(v, float) and v >= slot.get(k, (-1.0, None))[0]:
            slot[k] = (v, repr(case))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    gpu_report.note("layout_kernels", dict(
        gate="pack, unpack, import, import_pad: bit-equal (the whole sentinel-filled arena or buffer); export, copy_affine: exact data "
             "bit-equal, random within 2u (|x scale| + |shift| + |old|) (+ half a bf16 ulp for a bf16 destination); split_bf16: hi, lo "
             "bit-equal on exact and affine-free data, hi + lo within the same bound + 2^-16 |v| otherwise; the figures are error / bound "
             "(<= 1 passes), families without a figure passed bit equality",
        worst={f: {k: dict(value=v, case=c, gate=1.0) for k, (v, c) in slot.items()} for f, slot in sorted(_WORST.items())},
        bit_equal=dict(gate="0 differing elements", differing=0, elements=dict(sorted(_BITS.items()))), cases=dict(sorted(_RUN.items()))))


@pytest.mark.parametrize("dt", LC.PDTS, ids=[LC.PDTN[d] for d in LC.PDTS])
@pytest.mark.parametrize("case", LC.PACK_CASES, ids=[repr(c) for c in LC.PACK_CASES])
def test_pack(case, dt):
    ran = LC.check_pack(_side(), case, dt)
    _note("pack", case, dict(elements=sum(ran.values())), [LC.pack_kernel(p, dt, len(case.jobs)) for p in ran])


@pytest.mark.parametrize("case,flags", LC.UNPACK_CASES, ids=["%r-flags%d" % cf for cf in LC.UNPACK_CASES])
def test_unpack(case, flags):
    ran = LC.check_unpack(_side(), case, flags)
    _note("unpack", case, dict(elements=2 * sum(ran.values())), [LC.pack_kernel(p, LC.F32, len(case.jobs), True) for p in ran])


@pytest.mark.parametrize("case", LC.IMPORT_CASES, ids=[c.id for c in LC.IMPORT_CASES])
def test_import(case):
    _note(case.kind, case, LC.check_import(_side(), case), ["%s_kernel<%s>" % ("import_ncdhw" if case.pad is None else "import_pad", LC.DTN[case.dt])])


@pytest.mark.parametrize("case", LC.EXPORT_CASES, ids=[c.id for c in LC.EXPORT_CASES])
def test_export(case):
    _note("export", case, LC.check_export(_side(), case), ["export_ncdhw_kernel<%s>" % LC.DTN[case.dt]])


@pytest.mark.parametrize("case", LC.COPY_CASES, ids=[c.id for c in LC.COPY_CASES])
def test_copy(case):
    _note("copy_affine8" if case.kernel == "copy_affine8_kernel" else "copy_affine", case, LC.check_copy(_side(), case), [case.kernel])


@pytest.mark.parametrize("case", LC.SPLIT_CASES, ids=["q%d-hi_%s-lo_%s-%s-%s-src_%s" % (c[0], c[1], c[2], c[5], c[6], c[7]) for c in LC.SPLIT_CASES])
def test_split(case):
    _note("split_bf16", case, LC.check_split(_side(), *case), ["split_bf16_kernel"])


def test_refusals():
    LC.check_refusals(_side())
