"""Guard bands for direct C-ABI calls: where a kernel writes, and what it reads, besides the values it computes.

A reference comparison sees values only.  It cannot see a write past the end of an output or a workspace (torch's allocator pads
every block and functional._carve hands out slices of one large scratch buffer, so the stray store lands in slack or in the next
temporary), an element that was never written (a reused scratch buffer holds plausible floats of the previous layer), or a read
outside an operand whose value is multiplied by zero.  The helpers here make all three visible:

  * a float OPERAND is a copy of the data between two bands of NaN: a read outside it poisons whatever it is multiplied into;
  * an OUTPUT holds the sentinel word 0x7FA5A5A5 everywhere, bands included: as a float32 it is a NaN with a payload, as a float64
    pair of words it is about 8e305 (finite, so `written` also looks for the bit pattern itself), as an int32 it is no valid index
    at the sizes tested; an element that was never written is found by `written`, a band that was written by `bands_intact`;
  * an IN/OUT tensor (running_mean, running_var) is data between sentinel bands;
  * a WORKSPACE (`banded_bytes`) is exactly the number of bytes asked for, sentinel-filled, between sentinel bands, its first byte
    256-byte aligned as functional._carve supplies it: it starts out poisoned, so a read of a part the kernel never wrote poisons
    the result, and a use beyond the entry's own *_workspace_bytes figure changes a band.

Band width: the larger of 256 elements and 128 rows (last dimension) of the tensor -- 128 rows is the pair-GEMM / weight-gradient
tile height, so a whole stray tile still lands inside the band, i.e. inside the test's own allocation -- rounded up so that the
view stays 256-byte aligned.  `dense_band` is the exception for the dense GEMM entries, whose header contract is "every pointer
16-byte aligned": widths = 4 (mod 8) floats put every tensor at the weakest alignment the header permits.

Integer OPERANDS (gather / scatter indices, koff, pos, nbr, idx, order, seg_off) are NOT banded: a band value read as an index would
address memory, and nothing here may cause a stray access.  Over-reads of index arrays are therefore out of scope of this helper."""
import numpy as np
import torch

SENTINEL = 0x7FA5A5A5
SENTINEL64 = (SENTINEL << 32) | SENTINEL
ALIGN = 256
WORKSPACE_BAND_BYTES = 1 << 18      # more than one 192 x 192 float32 weight-gradient tile

_WORDS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64}


def _default_device():
    return "cuda" if torch.cuda.is_available() else "cpu"


def _sentinel_of(dtype):
    return SENTINEL if _WORDS[dtype] == torch.int32 else SENTINEL64


def band_width(shape, dtype=torch.float32):
    """Elements per band: max(256, 128 rows), rounded up to a multiple of 256 bytes."""
    row = int(shape[-1]) if len(shape) >= 2 else 1
    per = ALIGN // torch.empty((), dtype=dtype).element_size()
    return -(-max(256, 128 * row) // per) * per


def dense_band(shape):
    """Band width for the dense GEMM entries: as band_width, but = 4 (mod 8) floats, so that the view is 16-byte aligned and no more."""
    row = int(shape[-1]) if len(shape) >= 2 else 1
    return -(-max(256, 128 * row) // 8) * 8 + 4


def banded(shape, data=None, dtype=torch.float32, band=None, inout=False, device=None):
    """A tensor of `shape` as a view into the middle of a larger allocation: (whole, view).
    data given, inout False: an operand, NaN bands (float dtypes only).  data None: an output, the sentinel everywhere.
    data given, inout True: data between sentinel bands."""
    device = device or _default_device()
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape)) if shape else 1
    if band is None:
        band = band_width(shape, dtype)
    if data is not None and not inout:
        assert dtype.is_floating_point, "integer operands stay unbanded (module docstring)"
        whole = torch.full((n + 2 * band,), float("nan"), dtype=dtype, device=device)
    else:
        whole = torch.full((n + 2 * band,), _sentinel_of(dtype), dtype=_WORDS[dtype], device=device).view(dtype)
    view = whole[band:band + n].view(shape)
    if data is not None:
        view.copy_(data.to(device=device, dtype=dtype))
    return whole, view


def banded_bytes(nbytes, band_bytes=WORKSPACE_BAND_BYTES, device=None):
    """A workspace of exactly nbytes bytes (a multiple of 4): (whole, payload), both int32 words, sentinel everywhere; the payload
    starts 256-byte aligned."""
    device = device or _default_device()
    nbytes = int(nbytes)
    assert nbytes % 4 == 0 and band_bytes % ALIGN == 0
    whole = torch.full(((nbytes + 2 * band_bytes) // 4,), SENTINEL, dtype=torch.int32, device=device)
    payload = whole[band_bytes // 4:(band_bytes + nbytes) // 4]
    assert not whole.is_cuda or whole.data_ptr() % ALIGN == 0      # torch's device allocator aligns every block to 512 bytes
    return whole, payload


def address(whole, payload):
    """Device address of the payload's first byte (an empty payload has no data_ptr of its own)."""
    return whole.data_ptr() + (payload.storage_offset() - whole.storage_offset()) * whole.element_size()


def _words(t):
    return t.view(_WORDS[t.dtype])


def sentinel_only(t):
    """Every word of t still holds the sentinel (an untouched region)."""
    return bool((_words(t) == _sentinel_of(t.dtype)).all())


def bands_intact(whole, payload):
    """Both bands of `whole` around `payload` (the view banded / banded_bytes returned with it) still hold the sentinel."""
    assert payload.is_contiguous() and payload.dtype == whole.dtype
    start = payload.storage_offset() - whole.storage_offset()
    end = start + payload.numel()
    assert 0 < start and end < whole.numel()
    return sentinel_only(whole[:start]) and sentinel_only(whole[end:])


def written(view):
    """Every element was written: floats are all finite and none is the sentinel pattern; ints hold no sentinel word."""
    fresh = bool((_words(view) != _sentinel_of(view.dtype)).all())
    if view.dtype.is_floating_point:
        return fresh and bool(torch.isfinite(view).all())
    return fresh


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_words(a.contiguous()) == _words(b.contiguous())).all())
