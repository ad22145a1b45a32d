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


def test_same_bits_compares_words():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert G.same_bits(a, a.clone()) and not G.same_bits(a, torch.tensor([-0.0, float("nan"), 1.0]))
