"""The input and output pipeline (csrc/preproc.hip, csrc/postproc.hip) on a real MI355X at the value, size and tie edges of
tests/io_cases.py (gates, references and bound derivations: that module's docstring).  tests/test_io_cases_host.py runs the same
cases through the CPU model of the ABI and shows that six wrong references fail them.  This module reads only the repository:
Pillow's bytes come from tests/golden/io_edges.npz.

Which case reaches which of the eleven kernels:

  resample_coeffs_kernel     test_frames, every shape (twice per call: columns, rows); one block exactly and one thread into a second
                             at coeff_seam (128 x 129 outputs); ksize 109 / 125 at fullhd_54x; ksize 3 with one source pixel at
                             src1x1, src_w1, src_h1; one output at out1x1, out_w1
  resample_h_kernel          test_frames: 125 taps per output at fullhd_54x, `n * H + y` rows and a ragged last block at three_frames
                             and coeff_seam; white / black / checker / sparse images at the clip
  resample_v_norm_kernel     test_frames: the identity pass at v_identity and same3x3, the three normalisations (the distinct triple
                             would show a channel mix-up; mean 0 / std 1 must give byte / 255 exactly)
  gt_key_init_kernel,        test_gt: one decision per map (mixed4: a 0 / 1 map between two 0 .. 255 maps and a zero map); the
  gt_resize_kernel,          threshold itself (ones_36x64_up is a rounding above 1 and divided, ones_360x640_down exactly 1 and kept);
  gt_scale_kernel            the block cap of 1024 with the deciding pixel last / first (fullhd_two_at_end / _start); 1 x W, H x 1
                             and 1 x 1 sources; resizes of one axis only
  audio_excerpt_kernel       test_audio: M = 0, 1, 2, win - 1, win (odd and even), win = 1 and 257, start at / past the end, an
                             excerpt that ends on the last sample and one whose end is clamped to it
  resize_blur_kernel         test_resize_blur: the 32 x 64 tile exactly, one more and one less in both directions, four tiles, an
                             output lower than the blur radius and wider than two tiles and the reverse, sources of one pixel, one row,
                             one column, a 30x downscale; sigmoid, all-negative, +-3e4 and constant maps; test_resize_blur_impulse: the
                             reflected kernel at both corners and on both sides of a tile seam
  pp_minmax_init_kernel,     behind every resize_blur case (keys of the call against vinet_minmax on its output; bytes from those
  minmax_kernel,             keys) and alone in test_minmax_u8_sizes: n = 1 .. 2049 around a wave, a block and one round of eight, and
  normalize_u8_kernel        2 099 277 elements past the cap of 1024 blocks with both extremes in the last 77; three maps with their own
                             extremes; a map of -0.0 and +0.0; the tie map, whose 255 integer values all land on k + 0.5

Every output and the exactly-sized scratch buffers sit between sentinels that must survive.  The refusals are asked for their return
value only, never launched.

NOT COVERED: non-finite and subnormal map values (the kernels' fminf / fmaxf skip a NaN where torch.min / max propagate it: stated,
not changed); grids past 2^31 threads; vinet_normalize_u8 with keys taken from a different map (the clamp to [min, max] in front of
the division)."""
import pytest

from tests import gpu_report
from tests import io_cases as IO
from tests.test_gpu_kernels import _dev, _lib, _stream

pytestmark = pytest.mark.gpu

_BITS = {}               # family -> elements compared bit for bit (all equal: a difference fails the case)
_CASES = {}              # family -> cases run
_AUDIO = [0.0, 0.0]      # the worst |got - ref| of the Hanning window and the gate of that case
_GATES = {
    "frames": "bit for bit against Pillow's recorded bytes through ((byte / 255) - mean) / std",
    "gt": "bit for bit against oracle/preproc_cpu.py; (2^-24 + 2^-50) |ref| against float64",
    "audio": "exact zeros outside the excerpt; 1e-9 + 2e-7 max|ref| inside",
    "resize_blur": "maps, keys and bytes bit for bit against oracle/postproc_cpu.py; gamma(24) blur(resize|src|) against float64",
    "minmax_u8": "keys and bytes bit for bit against oracle/postproc_cpu.py",
    "python": "single items and non-contiguous views bit-equal to the batched contiguous call",
}


def _side():
    return IO.Side(_lib(), _dev(), _stream())


def _done(family, res):
    _BITS[family] = _BITS.get(family, 0) + res["bits"]
    _CASES[family] = _CASES.get(family, 0) + 1
    if res.get("audio_err", -1.0) >= _AUDIO[0]:
        _AUDIO[:] = [res["audio_err"], res["audio_gate"]]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for family, bits in _BITS.items():
        gpu_report.note("io_kernels/" + family, dict(gate=_GATES[family], cases=_CASES[family], bit_compared=bits,
                                                     audio_worst_err=_AUDIO[0], audio_gate=_AUDIO[1]))


@pytest.mark.parametrize("kind", IO.IMAGE_KINDS)
@pytest.mark.parametrize("shape", list(IO.FRAME_SHAPES))
def test_frames(shape, kind):
    _done("frames", IO.check_frames(_side(), shape, kind))


@pytest.mark.parametrize("name", list(IO.GT_CASES))
def test_gt(name):
    _done("gt", IO.check_gt(_side(), name))


@pytest.mark.parametrize("name", list(IO.AUDIO_CASES))
def test_audio(name):
    _done("audio", IO.check_audio(_side(), name))


@pytest.mark.parametrize("values", IO.RB_VALUES)
@pytest.mark.parametrize("shape", list(IO.RB_SHAPES))
def test_resize_blur(shape, values):
    _done("resize_blur", IO.check_rb_case(_side(), shape, values))


@pytest.mark.parametrize("name", list(IO.RB_IMPULSES))
def test_resize_blur_impulse(name):
    _done("resize_blur", IO.check_rb_impulse(_side(), name))


@pytest.mark.parametrize("order", ["fwd", "rev"])
@pytest.mark.parametrize("n", IO.MM_SIZES)
def test_minmax_u8_sizes(n, order):
    _done("minmax_u8", IO.check_minmax_u8(_side(), IO.mm_map(n, order), "minmax n=%d %s" % (n, order)))


def test_minmax_u8_batch_zeros_and_ties():
    side = _side()
    _done("minmax_u8", IO.check_minmax_u8(side, IO.mm_batch3(), "minmax batch of 3"))
    _done("minmax_u8", IO.check_minmax_u8(side, IO.mm_zeros(), "minmax zeros", zero_keys=True))
    _done("minmax_u8", IO.check_minmax_u8(side, IO.mm_ties(), "minmax ties"))


def test_refusals():
    """null pointers, zero and negative extents, 65536 maps, 65536 tile rows, scratch off the 16-byte grid, the four audio
    refusals, the scratch queries: negative, explained, nothing written, nothing launched"""
    IO.check_refusals(_lib(), lambda t: t.clone().to(_dev()))


def test_python_surface_single_items_and_views():
    """frames_to_tensor, gt_to_tensor, audio_excerpt, resize_blur with and without keys, postprocess / to_uint8"""
    _done("python", IO.check_python_surface(_dev()))
