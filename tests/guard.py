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

Bytes and a second poison (the image kernels, the index entries and the executors' arenas):

  * a uint8 IMAGE (`banded_u8`) is an (h, w, 3) view with row pitch >= 3 w, starting 0..3 bytes past a 256-byte boundary, inside a larger
    allocation whose row slack and bands hold one fill byte.  `bands_intact_u8` finds a store into the slack or a band; an OUTPUT has no
    byte value that means "unwritten", so `written_u8` runs the kernel on two fills and wants the payload equal both times; a SOURCE is
    built twice, slack and bands 0x00 and then 0xFF, and the result must not change (a read beside a crop view);
  * an ARENA or a workspace that holds indices (`banded_bytes(nbytes, fill=0xFF | 0x00)`) keeps the sentinel in its bands and holds the
    fill byte in its payload: 0xFF.. is a NaN as float32 and float64 and -1, the library's own "absent", as int32 and int64; 0x00 is the
    second run.  The 0x7FA5A5A5 word would be a huge row index there and is never used for these.  `same_across_fills` is the check.

Integer OPERANDS (gather / scatter indices, koff, pos, nbr, idx, order, seg_off) are NOT banded: a band value read as an index would
address memory, and nothing here may cause a stray access.  Over-reads of index arrays are therefore out of scope of this helper."""
import numpy as np
import torch

SENTINEL = 0x7FA5A5A5
SENTINEL64 = (SENTINEL << 32) | SENTINEL
ALIGN = 256
WORKSPACE_BAND_BYTES = 1 << 18      # more than one 192 x 192 float32 weight-gradient tile

_WORDS = {torch.float32: torch.int32, torch.int32: torch.int32, torch.float64: torch.int64, torch.int64: torch.int64,
          torch.uint8: torch.uint8, torch.int8: torch.int8}


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


def banded_bytes(nbytes, band_bytes=WORKSPACE_BAND_BYTES, device=None, fill=None):
    """A workspace of exactly nbytes bytes (a multiple of 4): (whole, payload), both int32 words, sentinel everywhere; the payload
    starts 256-byte aligned.  fill = 0xFF or 0x00: the payload holds that byte instead (an arena, or a workspace that holds indices);
    the bands keep the sentinel."""
    device = device or _default_device()
    nbytes = int(nbytes)
    assert nbytes % 4 == 0 and band_bytes % ALIGN == 0 and fill in (None, 0x00, 0xFF)
    whole = torch.full(((nbytes + 2 * band_bytes) // 4,), SENTINEL, dtype=torch.int32, device=device)
    payload = whole[band_bytes // 4:(band_bytes + nbytes) // 4]
    if fill is not None:
        payload.fill_(-1 if fill == 0xFF else 0)
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


# ---------------------------------------------------------------------------------------------------------------- uint8 images
U8_BAND_BYTES = 1 << 12
FILLS = (0x00, 0xFF)


def banded_u8(shape, data=None, pitch=None, offset=0, fill=0xA5, device=None):
    """An (h, w, 3) uint8 view with row pitch `pitch` >= 3 w bytes whose first byte lies `offset` (0..3) bytes past a 256-byte boundary,
    inside a larger allocation: (whole, view).  Row slack (the pitch - 3 w bytes behind every row, the last included) and both bands
    hold `fill`; the payload holds data, or `fill` too when data is None (an output)."""
    device = device or _default_device()
    h, w, ch = (int(s) for s in shape)
    pitch = 3 * w if pitch is None else int(pitch)
    assert ch == 3 and h >= 1 and w >= 1 and pitch >= 3 * w and 0 <= offset <= 3 and 0 <= fill <= 255
    whole = torch.full((2 * U8_BAND_BYTES + h * pitch,), fill, dtype=torch.uint8, device=device)
    assert not whole.is_cuda or whole.data_ptr() % ALIGN == 0
    view = torch.as_strided(whole, (h, w, 3), (pitch, 3, 1), U8_BAND_BYTES + offset)
    if data is not None:
        view.copy_(data.to(device=device, dtype=torch.uint8))
    return whole, view


def _payload_mask_u8(whole, view):
    h, w, _ = view.shape
    mask = torch.zeros(whole.numel(), dtype=torch.bool, device=whole.device)
    torch.as_strided(mask, (h, 3 * w), (view.stride(0), 1), view.storage_offset() - whole.storage_offset()).fill_(True)
    return mask


def bands_intact_u8(whole, view, fill=0xA5):
    """Every byte of `whole` outside the (h, 3 w) payload of `view` -- both bands and the slack behind every row -- still holds fill."""
    return bool((whole[~_payload_mask_u8(whole, view)] == fill).all())


def written_u8(run, fills=(0x5A, 0xC3)):
    """A byte has no value that means "not written": run(fill) -> (whole, view) builds a banded_u8 output holding `fill` everywhere, runs
    the kernel into it and returns it.  Every payload byte was written iff the payload is the same for two fills (fills that differ in
    every bit, so a byte only part of which was merged in shows too), and nothing else was written iff slack and bands hold the fill."""
    a, b = (run(f) for f in fills)
    intact = bands_intact_u8(a[0], a[1], fills[0]) and bands_intact_u8(b[0], b[1], fills[1])
    return intact and bool((a[1] == b[1]).all())


def same_across_fills(run, fills=FILLS):
    """run(fill) -> a tensor or a tuple of tensors computed with a source's slack and bands, a workspace or an arena holding `fill`:
    the results are bit-identical for the two fills (nothing outside the view, and nothing the kernel did not write, reaches them)."""
    a, b = (run(f) for f in fills)
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
