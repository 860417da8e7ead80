"""tests/io_cases.py without a GPU: every case runs through the CPU model of the ABI (tests/abi_emulator.py) at the gates the GPU
test applies to the library, which shows that each case is well posed and that the oracle stays inside the float64 bounds.  The
module then proves that the cases discriminate: six references that are each wrong in one way a kernel could be wrong must fail
the case that was put in the tables for them.  The argument checks of the entry points run on the real library: they return before
any device call."""
import numpy as np
import pytest

from oracle import postproc_cpu as P
from oracle import preproc_cpu as Q
from tests import io_cases as IO
from tests.abi_emulator import AbiEmulator
from vinet_amd import _lib as L


def _side():
    return IO.Side(AbiEmulator())


# ---- 1. frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", IO.IMAGE_KINDS)
@pytest.mark.parametrize("shape", list(IO.FRAME_SHAPES))
def test_frame_cases(shape, kind):
    """the oracle (inside the CPU model) against Pillow's recorded bytes, under all three normalisations"""
    IO.check_frames(_side(), shape, kind)


def test_frame_tables_reach_their_edges():
    s = IO.FRAME_SHAPES
    ks = lambda a, b: int(np.ceil(max(a / b, 1.0))) * 2 + 1          # noqa: E731  (Resample.c: ksize)
    assert ks(1080, 20) == 109 and ks(1920, 31) == 125
    assert {s["coeff_seam"][4], s["coeff_seam"][5]} == {128, 129}
    assert (s["coeff_seam"][2] * s["coeff_seam"][5]) % 256 and (s["coeff_seam"][4] * s["coeff_seam"][5]) % 256
    assert s["v_identity"][2] == s["v_identity"][4] and s["three_frames"][1] == 3
    assert (3 * 37 * 31) % 256 and (3 * 20 * 31) % 256                # a ragged last block in both passes
    assert any(v[2] == 1 and v[3] == 1 for v in s.values()) and any(v[4] == 1 and v[5] == 1 for v in s.values())
    img = IO.make_image("three_frames", "random")
    assert not np.array_equal(img[0], img[1]) and not np.array_equal(img[1], img[2])
    sp = IO.make_image("coeff_seam", "sparse")
    assert set(np.unique(sp)) == {0, 255} and 0.02 < (sp == 255).mean() < 0.04
    ck = IO.make_image("same3x3", "checker")
    assert set(np.unique(ck)) == {0, 255} and ck[0, 0, 0, 0] != ck[0, 0, 1, 0] and ck[0, 0, 0, 0] != ck[0, 0, 0, 1]
    means, stds = IO.NORMS[2][1], IO.NORMS[2][2]
    assert len(set(means + stds)) == 6
    # saturated images come near the clip: the white image stays white through both passes
    assert (IO.frame_case("fullhd_54x", "white")[1] == 255).all() and not IO.frame_case("fullhd_54x", "black")[1].any()


# ---- 2. ground truth -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IO.GT_CASES))
def test_gt_cases(name):
    IO.check_gt(_side(), name)


def test_gt_threshold_cases_sit_on_the_threshold():
    """the double maximum of the resized all-ones maps, before the decision: a rounding above 1 from 36 x 64 (the float32 weights
    1 - f and f do not add up to 1 in either direction: (1 + 2^-25)^2), exactly 1 from 360 x 640"""
    up = IO.gt_resized64(np.ones((1, 36, 64), np.uint8), 224, 384)
    down = IO.gt_resized64(np.ones((1, 360, 640), np.uint8), 224, 384)
    assert 1.0 < float(up.max()) <= 1.0 + 2.0 ** -23 and float(up.min()) == 1.0
    assert float(down.max()) == 1.0 and 1.0 - 2.0 ** -23 <= float(down.min()) < 1.0
    n = 1080 * 1920
    assert n > 1024 * 256 * 4 and (n - 1) % (1024 * 256) != 0        # the block cap is taken; the last pixel is in a later round


# ---- 3. audio ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IO.AUDIO_CASES))
def test_audio_cases(name):
    IO.check_audio(_side(), name)


def test_audio_table_reaches_its_edges():
    ms = {}
    for name, (n, start, end, win) in IO.AUDIO_CASES.items():
        ms[name] = (max(0, min(end + 1, n) - start), win)
    assert ms["m0"][0] == 0 and ms["start_at_n"][0] == 0 and ms["start_past_n"][0] == 0 and ms["m1_last_sample"][0] == 1
    assert ms["m2_all_zero"][0] == 2 and ms["m_eq_win_odd"] == (7, 7) and ms["m_eq_win_even"] == (2000, 2000)
    assert ms["m_win_minus_1"] == (6, 7) and ms["win1"] == (1, 1) and ms["win257"][1] == 257
    assert ms["long_to_last_sample"] == (IO.AUDIO_WIN, IO.AUDIO_WIN) and ms["long_end_clamped"] == (IO.AUDIO_WIN, IO.AUDIO_WIN)
    # the written-out window against the oracle's statement of numpy 1.18's
    for M in (1, 2, 7, 2000):
        assert np.array_equal(IO.hanning64(M), Q.hanning_np118(M))


# ---- 4. resize + blur + keys + bytes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", IO.RB_VALUES)
@pytest.mark.parametrize("shape", list(IO.RB_SHAPES))
def test_resize_blur_cases(shape, values):
    IO.check_rb_case(_side(), shape, values)


@pytest.mark.parametrize("name", list(IO.RB_IMPULSES))
def test_resize_blur_impulses(name):
    """a same-size resize is the identity, so an impulse becomes the outer product of the kernel reflected at the borders"""
    IO.check_rb_impulse(_side(), name)
    src = IO.rb_impulse(name)
    assert np.array_equal(P.resize_linear(src, 64, 128), src)
    assert float(np.abs(IO.resize_blur_ref64(src, 64, 128)[0] - IO.impulse_outer64(name)).max()) < 1e-15


def test_independent_references_are_independent_and_agree():
    """the written-out kernel is cv2's; the float64 resize agrees with torch's bilinear interpolation (another implementation of
    half-pixel sampling) to the float32 round-off of its coordinates"""
    import torch
    assert np.array_equal(IO.gaussian11(), P.gaussian_kernel().astype(np.float64))
    src = IO.rb_source("batch5", "sigmoid")
    t = torch.nn.functional.interpolate(torch.from_numpy(src)[None].double(), size=(20, 31), mode="bilinear", align_corners=False)[0].numpy()
    assert float(np.abs(IO.resize_ref64(src, 20, 31) - t).max()) < 1e-5


def test_resize_blur_tables_reach_their_edges():
    s = IO.RB_SHAPES
    outs = {(v[4], v[5]) for v in s.values()}
    assert {(32, 64), (33, 65), (31, 63), (64, 128), (3, 130), (70, 2)} <= outs
    assert any(v[2] == 1 and v[3] == 1 for v in s.values()) and any(v[2] == 1 and v[3] > 1 for v in s.values())
    assert any(v[3] == 1 and v[2] > 1 for v in s.values()) and any(v[1] > 1 for v in s.values())
    assert (IO.rb_source("tile_exact", "negative") < 0).all()
    m = IO.rb_source("tile_exact", "mixed")
    assert m.min() < -2e4 and m.max() > 2e4


# ---- 5. keys and bytes alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["fwd", "rev"])
@pytest.mark.parametrize("n", IO.MM_SIZES)
def test_minmax_u8_sizes(n, order):
    x = IO.mm_map(n, order)
    lo, hi = IO.mm_positions(n, order)
    assert int(x.argmin()) == (lo if n > 1 else 0) and int(x.argmax()) == hi and float(x.max()) == IO.MM_HIGH
    assert n == 1 or float(x.min()) == IO.MM_LOW
    if n > IO.MM_CAP_N:
        assert min(lo, hi) >= n - 77 and (n - 77) >= IO.MM_CAP_N + 2048
    IO.check_minmax_u8(_side(), x, "minmax n=%d %s" % (n, order))


def test_minmax_u8_batch_zeros_and_ties():
    side = _side()
    IO.check_minmax_u8(side, IO.mm_batch3(), "minmax batch of 3")
    z = IO.mm_zeros()
    assert not z.any() and np.signbit(z).any() and not np.signbit(z).all()
    IO.check_minmax_u8(side, z, "minmax zeros", zero_keys=True)
    IO.check_minmax_u8(side, IO.mm_ties(), "minmax ties")


def test_the_tie_map_is_all_ties():
    t = IO.mm_ties()
    assert np.float32(float(t.max()) - float(t.min()) + 1e-5) == np.float32(255)
    y = IO._normalize_y(t[0])
    assert np.array_equal(y[:255], np.arange(255, dtype=np.float32) + np.float32(0.5))          # every integer value: an exact tie
    even = P.normalize_u8(t)[0]
    assert np.array_equal(even, np.rint(y).astype(np.uint8))
    assert int((even != np.floor(y + np.float32(0.5)).astype(np.uint8)).sum()) == 128           # round half away
    assert int((even != y.astype(np.uint8)).sum()) == 127                                      # truncation


# ---- 7. the cases discriminate ---------------------------------------------------------------------------------------------------
def _fails(at, fn, *args, **kw):
    """the case fails, and at the gate it was made for: `at` is a regular expression for the message of that gate"""
    with pytest.raises(AssertionError, match=at):
        fn(_side(), *args, **kw)


def test_round_half_away_fails_the_tie_map():
    """(the minimum of ANY map lands on y = 0.5 and must become 0, so one byte per map is a tie already; here 255 are)"""
    _fails(r"ties: 128 of 256 bytes differ", IO.check_minmax_u8, IO.mm_ties(), "ties", ref=IO.HalfAwayRef())


def test_double_cv2_weights_fail_the_all_ones_map():
    _fails(r"gt ones_36x64_up: 86016 of 86016 values differ", IO.check_gt, "ones_36x64_up", ref=IO.DoubleWeightRef())


def test_border_reflect_fails_the_corner_impulse():
    _fails(r"impulse/corner: \d+ of 8192 samples differ", IO.check_rb_impulse, "corner", ref=IO.ReflectRef())
    _fails(r"impulse/last: \d+ of 8192 samples differ", IO.check_rb_impulse, "last", ref=IO.ReflectRef())


def test_unrounded_pillow_passes_fail_the_fixture():
    _fails(r"frames three_frames/random/default: \d+ of 5580 values differ from Pillow's", IO.check_frames, "three_frames", "random",
           ref=IO.NoByteRoundingRef())
    # the one-pass form is not wrong everywhere: where one pass is the identity there is nothing to round in between
    IO.check_frames(_side(), "v_identity", "white", ref=IO.NoByteRoundingRef())


def test_a_maximum_that_drops_the_last_element_fails_the_last_pixel_cases():
    _fails(r"gt fullhd_two_at_end: \d+ of 2073600 values differ", IO.check_gt, "fullhd_two_at_end", ref=IO.DropsLastRef())
    IO.check_gt(_side(), "fullhd_two_at_start", ref=IO.DropsLastRef())
    for n in (2049, IO.MM_SIZES[-1]):
        _fails(r"max last: keys .*expected", IO.check_minmax_u8, IO.mm_map(n, "fwd"), "max last", ref=IO.DropsLastRef())
        _fails(r"min last: keys .*expected", IO.check_minmax_u8, IO.mm_map(n, "rev"), "min last", ref=IO.DropsLastRef())
    _fails(r"impulse/last: keys .*expected", IO.check_rb_impulse, "last", ref=IO.DropsLastRef())


def test_a_channel_mix_up_fails_the_distinct_triple():
    """each triple on its own: the identity triple cannot see a mix-up, the distinct one (and the default, whose channels differ
    too) must"""
    IO.check_frames(_side(), "same3x3", "random", ref=IO.ChannelMixRef(), norms=["identity"])
    _fails(r"frames same3x3/random/distinct: \d+ of 27 values differ", IO.check_frames, "same3x3", "random", ref=IO.ChannelMixRef(),
           norms=["distinct"])
    _fails(r"frames same3x3/random/default: ", IO.check_frames, "same3x3", "random", ref=IO.ChannelMixRef(), norms=["default"])


# ---- 6. refusals, 8. the Python surface ----------------------------------------------------------------------------------------
def test_entry_points_refuse_what_the_cases_say_they_refuse():
    lib = L.load()
    assert not L.is_test_double()
    assert IO.check_refusals(lib, lambda t: t.clone()) > 60


def test_python_surface_single_items_and_views():
    L._install_test_double(AbiEmulator())
    try:
        IO.check_python_surface("cpu")
    finally:
        L._install_test_double(None)
