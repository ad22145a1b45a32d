"""tests/guard.py can tell: planted faults on CPU tensors are reported, an intact run passes.  No GPU."""
import pytest
import torch

from tests import guard as G

CPU = "cpu"
DTYPES = [torch.float32, torch.float64, torch.int32]


def _fill(view):
    """What a correct kernel does: writes every element of its output, and nothing else."""
    if view.dtype.is_floating_point:
        view.copy_(torch.arange(view.numel(), dtype=torch.float64).view(view.shape) * 0.5 - 3.0)
    else:
        view.copy_(torch.arange(view.numel(), dtype=torch.int64).view(view.shape) - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1,), (3, 5), (2, 7, 12), (129, 20)])
def test_an_intact_run_passes(shape, dtype):
    whole, view = G.banded(shape, dtype=dtype, device=CPU)
    assert view.shape == shape and view.dtype == dtype and view.data_ptr() % 256 == whole.data_ptr() % 256
    assert G.bands_intact(whole, view) and not G.written(view) and G.sentinel_only(view)
    _fill(view)
    assert G.bands_intact(whole, view) and G.written(view)


def test_band_width_is_128_rows_or_256_elements_and_keeps_the_alignment():
    assert G.band_width((5,)) == 256 and G.band_width((7, 1)) == 256
    assert G.band_width((9, 20)) == 128 * 20 and G.band_width((27, 36, 132)) == 128 * 132
    assert G.band_width((3, 5), torch.float64) == 640 and G.band_width((3, 3)) == 384
    for shape in [(3,), (4, 68), (2, 2052)]:
        b = G.dense_band(shape)
        assert b % 8 == 4 and b >= max(256, 128 * (shape[-1] if len(shape) > 1 else 1))
        whole, view = G.banded(shape, band=b, device=CPU)
        off = view.data_ptr() - whole.data_ptr()
        assert off % 16 == 0 and off % 32 == 16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["before", "after", "first band word", "last band word"])
def test_a_planted_write_outside_the_payload_is_reported(where, dtype):
    whole, view = G.banded((6, 10), dtype=dtype, device=CPU)
    _fill(view)
    band, n = G.band_width((6, 10), dtype), 60
    at = {"before": band - 1, "after": band + n, "first band word": 0, "last band word": whole.numel() - 1}[where]
    whole[at] = 1
    assert not G.bands_intact(whole, view)
    assert G.written(view)                      # the payload itself is complete: only the band check can see this


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("at", [0, 31, 59])
def test_one_unwritten_element_is_reported(at, dtype):
    whole, view = G.banded((6, 10), dtype=dtype, device=CPU)
    _fill(view)
    words = view.view(torch.int64 if dtype == torch.float64 else torch.int32).view(-1)
    words[at] = G.SENTINEL64 if dtype == torch.float64 else G.SENTINEL   # put the sentinel back
    assert G.bands_intact(whole, view) and not G.written(view)


def test_float64_sentinel_is_finite_but_still_counts_as_unwritten():
    _, view = G.banded((4,), dtype=torch.float64, device=CPU)
    assert bool(torch.isfinite(view).all()) and not G.written(view)
    assert not bool(torch.isfinite(view * view).all())                     # and it does not survive a square


def test_an_operand_band_that_reaches_an_output_is_reported():
    data = torch.arange(12, dtype=torch.float32).view(3, 4)
    whole, x = G.banded((3, 4), data, device=CPU)
    assert torch.equal(x, data) and bool(torch.isnan(whole[:G.band_width((3, 4))]).all()) and bool(torch.isnan(whole[-1:]).all())
    w_out, out = G.banded((4,), device=CPU)
    out.copy_(x.sum(0))
    assert G.written(out) and G.bands_intact(w_out, out)
    # a column sum that runs one row too far reads the band, even with a weight of zero on it
    start = x.storage_offset()
    over = whole[start:start + 16].view(4, 4)
    weights = torch.tensor([1.0, 1.0, 1.0, 0.0]).view(4, 1)
    out.copy_((over * weights).sum(0))
    assert not G.written(out)


def test_inout_keeps_the_data_between_sentinel_bands():
    data = torch.tensor([0.5, -1.0, 2.0])
    whole, view = G.banded((3,), data, inout=True, device=CPU)
    assert torch.equal(view, data) and G.bands_intact(whole, view) and G.written(view)
    whole[view.storage_offset() + 3] = 0.0
    assert not G.bands_intact(whole, view)


def test_integer_operands_are_refused():
    with pytest.raises(AssertionError):
        G.banded((3,), torch.zeros(3, dtype=torch.int32), dtype=torch.int32, device=CPU)


@pytest.mark.parametrize("nbytes", [0, 256, 4 * 1000, 8 * 3 * 20])
def test_workspace_is_exact_aligned_and_poisoned(nbytes):
    whole, ws = G.banded_bytes(nbytes, device=CPU)
    assert ws.numel() * 4 == nbytes and G.sentinel_only(whole) and G.bands_intact(whole, ws)
    assert (ws.storage_offset() * 4) % 256 == 0
    assert bool(torch.isnan(whole.view(torch.float32)).all())              # a read of an unwritten part poisons a float result
    ws.zero_()
    assert G.bands_intact(whole, ws)
    whole[ws.storage_offset() + ws.numel()] = 0                            # one word past the *_workspace_bytes figure
    assert not G.bands_intact(whole, ws)
    whole, ws = G.banded_bytes(nbytes, device=CPU)
    whole[ws.storage_offset() - 1] = 0
    assert not G.bands_intact(whole, ws)


# ---------------------------------------------------------------------------------------------------------------- uint8 images
def _image(h, w, seed=0):
    g = torch.Generator().manual_seed(seed + h * 131 + w)
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)


def _invert(src, dst):
    """A correct byte kernel: reads the (h, w, 3) view of its source, writes every byte of the view of its output."""
    dst.copy_(255 - src)


U8_SHAPES = [(1, 1, 0, 0), (5, 7, 24, 1), (3, 130, 400, 3), (2, 4, 12, 2)]     # h, w, pitch, offset


@pytest.mark.parametrize("h,w,pitch,offset", U8_SHAPES)
def test_u8_view_has_the_pitch_the_offset_and_the_fill(h, w, pitch, offset):
    pitch = pitch or 3 * w
    data = _image(h, w)
    whole, view = G.banded_u8((h, w, 3), data, pitch=pitch, offset=offset, fill=0x3C, device=CPU)
    assert view.shape == (h, w, 3) and view.stride() == (pitch, 3, 1) and torch.equal(view, data)
    assert (view.data_ptr() - whole.data_ptr()) % 256 == offset
    assert G.bands_intact_u8(whole, view, 0x3C)
    outside = whole.numel() - 3 * h * w
    assert int((whole == 0x3C).sum()) >= outside and outside == 2 * G.U8_BAND_BYTES + h * (pitch - 3 * w)
    with pytest.raises(AssertionError):
        G.banded_u8((h, w, 3), pitch=3 * w - 1, device=CPU)
    with pytest.raises(AssertionError):
        G.banded_u8((h, w, 3), offset=4, device=CPU)


@pytest.mark.parametrize("h,w,pitch,offset", U8_SHAPES)
def test_u8_a_correct_byte_kernel_passes(h, w, pitch, offset):
    src = _image(h, w)

    def run(fill):
        whole, view = G.banded_u8((h, w, 3), pitch=pitch or 3 * w, offset=offset, fill=fill, device=CPU)
        _invert(src, view)
        return whole, view
    assert G.written_u8(run)
    whole, view = run(0xA5)
    assert G.bands_intact_u8(whole, view) and torch.equal(view, 255 - src)


@pytest.mark.parametrize("where", ["byte behind the last pixel", "row slack", "byte in front", "last band byte"])
def test_u8_a_stray_byte_is_reported(where):
    h, w, pitch = 5, 7, 24
    src = _image(h, w)

    def run(fill):
        whole, view = G.banded_u8((h, w, 3), pitch=pitch, offset=1, fill=fill, device=CPU)
        _invert(src, view)
        start = view.storage_offset()
        at = {"byte behind the last pixel": start + (h - 1) * pitch + 3 * w, "row slack": start + 2 * pitch + 3 * w + 1,
              "byte in front": start - 1, "last band byte": whole.numel() - 1}[where]
        whole[at] = 255 - fill                      # what a dword store over the end of a row does
        return whole, view
    whole, view = run(0xA5)
    assert not G.bands_intact_u8(whole, view) and not G.written_u8(run)


@pytest.mark.parametrize("at", [(0, 0, 0), (2, 3, 1), (4, 6, 2)])
def test_u8_an_unwritten_byte_is_reported(at):
    h, w = 5, 7
    src = _image(h, w)

    def run(fill):
        whole, view = G.banded_u8((h, w, 3), pitch=24, offset=3, fill=fill, device=CPU)
        keep = view[at].clone()
        _invert(src, view)
        view[at] = keep                              # the kernel skipped this byte: it still holds the fill
        return whole, view
    whole, view = run(0xA5)
    assert G.bands_intact_u8(whole, view)            # the band check alone cannot see it
    assert not G.written_u8(run)


def test_u8_a_read_of_the_row_slack_is_reported():
    h, w, pitch = 4, 5, 20
    data = _image(h, w)

    def blur(fill, over):
        """A horizontal 2-tap average; over = 1 reads one byte past the end of every row (the slack, or the band behind the last row)."""
        whole, view = G.banded_u8((h, w, 3), data, pitch=pitch, offset=2, fill=fill, device=CPU)
        rows = torch.as_strided(whole, (h, 3 * w + 1), (pitch, 1), view.storage_offset()).to(torch.int32)
        right = rows[:, 1:] if over else torch.cat([rows[:, 1:3 * w], rows[:, 3 * w - 1:3 * w]], 1)
        return ((rows[:, :3 * w] + right) // 2).to(torch.uint8)
    assert G.same_across_fills(lambda fill: blur(fill, 0))
    assert not G.same_across_fills(lambda fill: blur(fill, 1))


# ---------------------------------------------------------------------------------------------------------------- arena poison
@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("nbytes", [0, 256, 4 * 1000])
def test_arena_poison_fills_the_payload_and_keeps_sentinel_bands(nbytes, fill):
    whole, arena = G.banded_bytes(nbytes, device=CPU, fill=fill)
    assert arena.numel() * 4 == nbytes and G.bands_intact(whole, arena) and (arena.storage_offset() * 4) % 256 == 0
    assert bool((arena.view(torch.uint8) == fill).all())
    if fill == 0xFF and nbytes:
        assert bool(torch.isnan(arena.view(torch.float32)).all()) and bool(torch.isnan(arena.view(torch.float64)).all())
        assert bool((arena == -1).all()) and bool((arena.view(torch.int64) == -1).all())     # "absent", never an address
    whole[arena.storage_offset() + arena.numel()] = 0                      # one word past the *_arena_bytes figure
    assert not G.bands_intact(whole, arena)
    with pytest.raises(AssertionError):
        G.banded_bytes(nbytes, device=CPU, fill=0xA5)


def test_a_result_that_depends_on_the_arena_fill_is_reported():
    x = torch.arange(12, dtype=torch.float32)

    def scan(fill, words_written):
        """A two-pass sum through a workspace of three words; words_written = 2 leaves the last partial unwritten and reads it."""
        _, ws = G.banded_bytes(12, device=CPU, fill=fill)
        part = ws.view(torch.float32)
        part[:words_written] = x.view(3, 4).sum(1)[:words_written]
        return part.sum().view(1)
    assert G.same_across_fills(lambda fill: scan(fill, 3))
    assert not G.same_across_fills(lambda fill: scan(fill, 2))
    # an index workspace: -1 in one run, 0 in the other, so a row taken from an unwritten word changes the gather
    table = torch.arange(10, dtype=torch.int32) * 3

    def gather(fill, words_written):
        _, ws = G.banded_bytes(16, device=CPU, fill=fill)
        ws[:words_written] = torch.tensor([4, 2, 9, 1], dtype=torch.int32)[:words_written]
        rows = ws.long()
        return torch.where(rows >= 0, table[rows.clamp(min=0)], torch.full_like(table[:4], -1)), ws.clone()
    assert G.same_across_fills(lambda fill: gather(fill, 4))
    assert not G.same_across_fills(lambda fill: gather(fill, 3))


def test_same_bits_compares_words():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert G.same_bits(a, a.clone()) and not G.same_bits(a, torch.tensor([-0.0, float("nan"), 1.0]))
