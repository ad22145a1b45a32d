"""Where the rest of the C ABI writes and what it reads: the entries tests/test_guard_bands_gpu.py left out, called directly on
guard-banded tensors, byte images and poisoned workspaces and arenas (tests/guard.py).  Every assertion is bitwise or structural; the
one tolerance in this file is the one-step comparison of ftx_adam_step with torch.optim.Adam, at the tolerances of
tests/test_ops_gpu.py::test_adam_one_launch_matches_torch_adam.

Every case asserts, of
  (a)  every band of every output, in/out tensor and workspace is intact, the workspace being of exactly the entry's own
       *_workspace_bytes (for byte images: both bands and the slack behind every row);
  (b)  every output element was written and is finite (a byte has no "unwritten" value: a byte output is run on two fills and must
       come out equal); where include/ftx.h documents a region as untouched or unspecified only what the header promises;
  (c)  the output is bit-identical to the same entry called on plain contiguous tensors with a plain workspace;
  (c') for byte sources and for 0xFF / 0x00 poisoned workspaces and arenas: the output is bit-identical across the two fills,
what the table below says.  Integer operands are plain tensors with in-range contents (tests/guard.py says why).  A call whose launch
fails or whose synchronize reports a fault ends the session.  Shapes are the smallest that reach each write pattern: 2048 * 256 + 1
elements take the second trip of a grid-stride loop (grid_for caps at 2048 blocks of 256; for a (k, n) output it is k * n that
counts), 256 * 256 + 1 points that of the losses' 256 blocks, 2049 original points give the scatter-back two blocks.

Per entry of include/ftx.h that launches a kernel and is not covered by tests/test_guard_bands_gpu.py or by the guard tests of
attention, the affine sampling and the localisation net:

  hashing, coordinates, tables (element-wise, one grid-stride loop each)
    ftx_hash, ftx_hash_kernel               a b c
    ftx_floor_coords, ftx_downsample_coords, ftx_gather_coords, ftx_level_coords      a b c
    ftx_rotate_points, ftx_trilinear_weights                                         a b c   float operands between NaN bands
    ftx_sorted_rank, ftx_hashtable_query, ftx_kernel_map_build                        a b c
    ftx_count                               a b c   counts (m) "is zeroed here": m > n included
    ftx_hashtable_build                     a b     "fully (re)initialised"; the slot layout depends on the order of the inserts, so
                                                    (c) is asserted on what ftx_hashtable_query returns from the built tables
                                                    ("Duplicate keys keep the smallest row index")
  sort-based entries, workspace 0xFF then 0x00
    ftx_unique_sorted                       a b c c'   b, c, c' on n_unique and on the first n_unique rows: "Rows past n_unique are
                                                       unspecified", so behind them only the bands are checked
    ftx_levels_unique                       a b c c'   likewise up to level_off[n_levels]; sorted_keys / order (n_levels * n, fully
                                                       written) given and NULL
    ftx_level_segments                      a b c
  pair lists
    ftx_kernel_map_count                    a b c c'   pos (k, n_out), koff (k + 1); c' on the scan workspace
    ftx_kernel_map_pairs                    a b c      pos in/out, pos_t (k, n_in), pair_in / pair_out (n_pairs) fully written
  image branch input
    ftx_sample_down_fwd                     a b c   out, saved (33) float64; running_* in/out: bit-untouched in eval mode, NULL in
                                                    training exercised
    ftx_sample_down_bwd                     a b c   the four gradients (9, 3, 3, 3)
  losses and evaluation
    ftx_fusion_loss, ftx_fusion_loss_mix    a b c   losses (2), two or four gradients, conf* in/out int64
    ftx_seg_loss                            a b c   grad NULL: "a forward-only kernel that contains no gradient stores": a banded
                                                    tensor standing where the gradient would be is not passed and must stay sentinel
    ftx_eval_scatter_back                   a b c   out-of-range points "are skipped": their pred_* words keep the sentinel
    ftx_project_points                      a b c   keep (n) uint8 between bands of a byte of its own, rowcol (n, 2)
  byte images
    ftx_color_jitter_u8, ftx_color_jitter_chw                                        a b c c'   c' across the workspace fills, and across the
                                                       fills of the bytes beside the source view
    ftx_resize_bilinear_u8                  a b c c'   likewise; the pad bytes of the intermediate rows are never written
  optimizer
    ftx_adam_step                           a b c   a tensor with g = NULL is "skipped": p, m, v bit-untouched; (c) holds across the
                                                    pointer alignments too: how an element is rounded depends on its place, not on the path
  rows
    ftx_rows_concat, ftx_rows_split, ftx_rows_add, ftx_rows_add_bias    a b c
  ViT input side, every tensor at 16-byte alignment only (guard.dense_band)
    ftx_vit_patch_embed_split, ftx_vit_patch_embed_bf16    a b c   tokens (b, t0 + gp, dim) fully written, class / distillation rows included
    ftx_vit_tap_stem_split, ftx_vit_tap_stem_bf16          a b c
  executors and the native index builder, every arena of exactly its *_arena_bytes figure, 0xFF then 0x00, between sentinel bands;
  (c) is the run on a torch.empty arena that the existing bit-for-bit test makes
    ftx_spvcnn_eval                         a b c c'   the two-op program on an empty map, and the full program on the C-caller recipe
    ftx_spvcnn_index_levels, ftx_spvcnn_index_maps, ftx_spvcnn_index_pairs          a b c c'
                                                       arenas A, B, C, with and without backward segments; every table the phases hand
                                                       back, and the sizes in rows / maps; b on the float tables (x0, the weights); the
                                                       hash tables' slots depend on the order of the inserts and are compared through
                                                       what they answer (nbr, the corner rows)
    ftx_vit_eval                            a b c c'   the small trunk, whole and block by block on one arena; tap outputs between bands
    ftx_spvcnn_train_fwd, ftx_spvcnn_train_bwd    a b c c'   through native_train's own table builder (NativeTrain.begin(arena=))
  not covered: ftx_stream_scratch_reset (one memset of the counter region that ftx_stream_scratch_attach also issues, and the attach is
    checked by the ticket fixture of tests/test_guard_bands_gpu.py; ftx_stream_scratch_release launches nothing).
  host only (launch nothing): ftx_version, ftx_last_error, ftx_hashtable_capacity, every *_workspace_bytes / *_arena_bytes / *_bytes
    query, ftx_adam_chunk_elements, ftx_resize_ksize, ftx_resize_coeffs_host, ftx_spvcnn_index_layout(_words), ftx_vit_eval_release."""
import ctypes

import numpy as np
import pytest
import torch

from tests import guard as GD
from tests.norm_ref import gen, randn
from tests.test_guard_bands_gpu import Banded, L, Plain, dev, ptr    # noqa: F401  (L is the module's library fixture)

pytestmark = pytest.mark.gpu
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
GRID = 2048 * 256                  # grid_for: at most 2048 blocks of 256 threads
BYTE_FILL = 0xA5


# ------------------------------------------------------------------------------------------------------------------ the harness
class Extra:
    """What the entries of this file need beyond tests/test_guard_bands_gpu.py: a workspace fill, outputs of which only the leading
    rows are specified, and flat byte outputs."""
    fill = None

    def upto(self, name, count):
        """Only the first count() rows of output `name` are specified (count is evaluated after the call)."""
        self.limits = getattr(self, "limits", {})
        self.limits[name] = count

    def limit(self, name):
        return int(getattr(self, "limits", {})[name]())

    def specified(self, name):
        view = self.outs[name][1]
        return view[:self.limit(name)] if name in getattr(self, "limits", {}) else view


class Fill(Extra, Banded):
    def __init__(self, lib, fill=None, tickets=None, band=None):
        Banded.__init__(self, lib, tickets, band)
        self.fill, self.byte_outs = fill, {}

    def ws(self, name, nbytes, untouched=False):
        whole, payload = GD.banded_bytes(nbytes, fill=self.fill)
        self.spaces[name] = (whole, payload, untouched)
        return GD.address(whole, payload)

    def out_bytes(self, name, n):
        """n bytes between bands of BYTE_FILL, for an output whose values are never BYTE_FILL (keep: 0 or 1)."""
        whole = torch.full((2 * GD.U8_BAND_BYTES + n,), BYTE_FILL, dtype=U8, device="cuda")
        view = whole[GD.U8_BAND_BYTES:GD.U8_BAND_BYTES + n]
        self.byte_outs[name] = (whole, view)
        return view.data_ptr()

    def check(self, what):
        limits = getattr(self, "limits", {})
        for name in limits:
            whole, view, _ = self.outs[name]
            assert GD.bands_intact(whole, view), "%s: a guard band of %s was written" % (what, name)
            assert GD.written(self.specified(name)), "%s: a specified row of %s was not written, or depends on memory nobody wrote" % (what, name)
        outs, self.outs = self.outs, {n: v for n, v in self.outs.items() if n not in limits}
        try:
            Banded.check(self, what)
        finally:
            self.outs = outs
        for name, (whole, view) in self.byte_outs.items():
            assert bool((whole[:GD.U8_BAND_BYTES] == BYTE_FILL).all()) and bool((whole[GD.U8_BAND_BYTES + view.numel():] == BYTE_FILL).all()), \
                "%s: a guard band of %s was written" % (what, name)
            assert bool((view != BYTE_FILL).all()), "%s: %s has a byte that was not written" % (what, name)


class PlainFill(Extra, Plain):
    def __init__(self, lib, tickets=None):
        Plain.__init__(self, lib, tickets)
        self.byte_outs = {}

    def out_bytes(self, name, n):
        t = torch.full((max(n, 1),), BYTE_FILL, dtype=U8, device="cuda")
        self.byte_outs[name] = (t, t[:n])
        return t.data_ptr()


def run(lib, case, what, fills=(None,), bitwise=True, tickets=None, band=None):
    """case(g) builds its tensors from g and calls the entry through g.call.  One guarded run per workspace fill, each checked for
    (a) and (b) and compared bit for bit with the run on plain tensors: (c), and through it (c') across the fills.  Returns the
    first guarded run."""
    runs = []
    for fill in fills:
        g = Fill(lib, fill, tickets, band)
        case(g)
        g.check(what if fill is None else "%s, workspace 0x%02X" % (what, fill))
        runs.append(g)
    if bitwise:
        p = PlainFill(lib, tickets)
        case(p)
        for g in runs:
            for name in g.outs:
                assert GD.same_bits(g.specified(name), p.specified(name)), "%s: %s differs from the call on plain tensors" % (what, name)
            for name, (_, view) in g.byte_outs.items():
                assert torch.equal(view, p.byte_outs[name][1]), "%s: %s differs from the call on plain tensors" % (what, name)
    for g in runs[1:]:
        for name in g.outs:
            assert GD.same_bits(g.specified(name), runs[0].specified(name)), "%s: %s changes with the workspace fill" % (what, name)
    return runs[0]


POISON = GD.FILLS[::-1]            # 0xFF first, then 0x00


def host(array):
    """A numpy array as a host pointer argument (the array must outlive the call: the caller keeps it)."""
    return array.ctypes.data_as(ctypes.c_void_p)


def coords_of(g0, n, span=40):
    """(n, 4) int32 voxel coordinates [x, y, z, batch], negative ones included, many duplicates once n is large."""
    c = torch.randint(-span, span, (n, 4), generator=g0, dtype=I32)
    c[:, 3] = torch.randint(0, 2, (n,), generator=g0, dtype=I32)
    return c


def offsets_of(k):
    r = {27: (-1, 0, 1), 8: (0, 1)}[k]
    return torch.tensor([(x, y, z) for x in r for y in r for z in r], dtype=I32)


def rows_for(n, k=1):
    """n itself for the small sizes; for "large", the fewest rows whose k * rows elements take the second trip of the grid-stride loop."""
    return n if n != "large" else -(-(GRID + 1) // k)


def built_table(lib, keys_d):
    """A hash table over keys_d, built by the library on plain tensors: (table_keys, table_vals, capacity)."""
    from fusiontransformer_amd._lib import check, stream
    n = keys_d.numel()
    cap = int(lib.ftx_hashtable_capacity(n))
    tk, tv = torch.empty(cap, dtype=I64, device="cuda"), torch.empty(cap, dtype=I32, device="cuda")
    check(lib.ftx_hashtable_build(ptr(keys_d), n, tk.data_ptr(), tv.data_ptr(), cap, stream()), "ftx_hashtable_build")
    torch.cuda.synchronize()
    return tk, tv, cap


def hashes_of(lib, coords_d):
    from fusiontransformer_amd._lib import check, stream
    out = torch.empty(coords_d.shape[0], dtype=I64, device="cuda")
    check(lib.ftx_hash(ptr(coords_d), coords_d.shape[0], out.data_ptr(), stream()), "ftx_hash")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------------------------ element-wise index entries
def _hash(lib, g0, n):
    n = rows_for(n)
    c = dev(coords_of(g0, n))
    return lambda g: g.call("ftx_hash", ptr(c), n, g.out("out", (n,), I64))


def _hash_kernel(k):
    def build(lib, g0, n):
        n = rows_for(n, k)
        c, off = dev(coords_of(g0, n)), dev(offsets_of(k))
        return lambda g: g.call("ftx_hash_kernel", ptr(c), n, ptr(off), k, g.out("out", (k, n), I64))
    return build


def _floor_coords(lib, g0, n):
    n = rows_for(n)
    pc = (torch.rand((n, 4), generator=g0) - 0.5) * 90.0
    pc[:, 3] = torch.randint(0, 2, (n,), generator=g0).float()
    return lambda g: g.call("ftx_floor_coords", g.op(pc), n, 2, g.out("out", (n, 4), I32))


def _downsample_coords(lib, g0, n):
    n = rows_for(n)
    c = dev(coords_of(g0, n))
    return lambda g: g.call("ftx_downsample_coords", ptr(c), n, 2, g.out("out", (n, 4), I32))


def _gather_coords(lib, g0, n):
    n = rows_for(n)
    src = dev(coords_of(g0, 301))
    index = torch.randint(0, 301, (n,), generator=g0)
    index[n // 2] = 300
    index_d = dev(index)
    return lambda g: g.call("ftx_gather_coords", ptr(src), ptr(index_d), n, g.out("out", (n, 4), I32))


def _level_coords(lib, g0, n):
    n = rows_for(n)
    pts = dev(coords_of(g0, 301))
    first = torch.randint(0, 301, (n,), generator=g0)
    first[n // 2] = 300
    first_d = dev(first)
    return lambda g: g.call("ftx_level_coords", ptr(pts), ptr(first_d), n, 4, g.out("out", (n, 4), I32))


def _rotate_points(lib, g0, n):
    n = rows_for(n)
    pts = randn(g0, n, 3) * 20.0
    rot = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(5).standard_normal((3, 3)))[0].astype(np.float32))
    return lambda g: g.call("ftx_rotate_points", g.op(pts), n, host(rot), g.out("out", (n, 3)))


def _sorted_rank(lib, g0, n):
    n = rows_for(n)
    cap, n_sorted = 700, 613                                                    # the count is read on the device and is below the capacity
    sorted_keys = torch.sort(torch.randperm(5000, generator=g0)[:cap])[0]
    queries = torch.randint(0, 5000, (n,), generator=g0)
    queries[n // 2] = sorted_keys[n_sorted - 1]                                 # the last key that counts
    queries[0] = sorted_keys[cap - 1]                                           # present in the array, behind the count: absent
    s_d, q_d, count_d = dev(sorted_keys, I64), dev(queries, I64), dev(torch.tensor([n_sorted]))
    return lambda g: g.call("ftx_sorted_rank", ptr(s_d), ptr(count_d), cap, ptr(q_d), n, g.out("rank", (n,), I32))


def _hashtable_query(lib, g0, n):
    n = rows_for(n)
    keys = hashes_of(lib, dev(coords_of(g0, 900, span=8)))
    tk, tv, cap = built_table(lib, keys)
    queries = torch.cat([keys, hashes_of(lib, dev(coords_of(g0, 300, span=30)))])[torch.randint(0, 1200, (n,), generator=g0).cuda()].contiguous()
    return lambda g: g.call("ftx_hashtable_query", ptr(queries), n, ptr(tk), ptr(tv), cap, g.out("out", (n,), I32))


def _kernel_map_build(k):
    def build(lib, g0, n):
        n = rows_for(n, k)
        table_coords = dev(coords_of(g0, 900, span=6))
        tk, tv, cap = built_table(lib, hashes_of(lib, table_coords))
        out_coords, off = dev(coords_of(g0, n, span=7)), dev(offsets_of(k))
        return lambda g: g.call("ftx_kernel_map_build", ptr(out_coords), n, ptr(off), k, ptr(tk), ptr(tv), cap, g.out("nbr", (k, n), I32))
    return build


def _count(lib, g0, n):
    m = {1: 300, 255: 100}.get(n, 1000)                                         # m > n: rows nobody counts into must still be zeroed
    n = rows_for(n)
    idx = torch.randint(-1, m + 1, (n,), generator=g0)                          # -1 and m: dropped
    idx_d = dev(idx)
    valid = idx[(idx >= 0) & (idx < m)]
    expect = torch.bincount(valid, minlength=m)

    def case(g):
        g.call("ftx_count", ptr(idx_d), n, g.out("counts", (m,), I32), m)
        assert torch.equal(g.view("counts").cpu().long(), expect)
    return case


def _trilinear_weights(lib, g0, n):
    n = rows_for(n)
    pc = (torch.rand((n, 4), generator=g0) - 0.5) * 60.0
    idx = torch.randint(0, 1000, (n, 8), generator=g0)
    idx[torch.rand((n, 8), generator=g0) < 0.3] = -1
    idx[n // 3] = -1                                                            # a point with no corner: 0 / 1e-8
    idx_d = dev(idx)
    return lambda g: g.call("ftx_trilinear_weights", g.op(pc), ptr(idx_d), n, 2, g.out("weights", (n, 8)))


ELEMENTWISE = {
    "ftx_hash": _hash, "ftx_hash_kernel k=27": _hash_kernel(27), "ftx_hash_kernel k=8": _hash_kernel(8), "ftx_floor_coords": _floor_coords,
    "ftx_downsample_coords": _downsample_coords, "ftx_gather_coords": _gather_coords, "ftx_level_coords": _level_coords,
    "ftx_rotate_points": _rotate_points, "ftx_sorted_rank": _sorted_rank, "ftx_hashtable_query": _hashtable_query,
    "ftx_kernel_map_build k=27": _kernel_map_build(27), "ftx_kernel_map_build k=8": _kernel_map_build(8), "ftx_count": _count,
    "ftx_trilinear_weights": _trilinear_weights,
}


@pytest.mark.parametrize("n", [1, 255, "large"])
@pytest.mark.parametrize("entry", sorted(ELEMENTWISE))
def test_elementwise_index_entries(L, entry, n):
    case = ELEMENTWISE[entry](L, gen(len(entry) + (n if n != "large" else 7)), n)
    run(L, case, "%s n=%s" % (entry, n))


@pytest.mark.parametrize("n", [1, 255, 4097])
def test_hashtable_build_reinitialises_both_tables(L, n):
    g0 = gen(n)
    keys = hashes_of(L, dev(coords_of(g0, n, span=5)))                          # 2000 distinct cells at the most: duplicates at 4097
    cap = int(L.ftx_hashtable_capacity(n))
    assert n < 4097 or torch.unique(keys).numel() < n

    def case(g):
        g.call("ftx_hashtable_build", ptr(keys), n, g.out("table_keys", (cap,), I64), g.out("table_vals", (cap,), I32), cap)
    r = run(L, case, "ftx_hashtable_build n=%d" % n, bitwise=False)              # (c) below: the slots depend on the order of the inserts
    tk, tv = r.view("table_keys"), r.view("table_vals")
    pk, pv, _ = built_table(L, keys)
    absent = hashes_of(L, dev(coords_of(g0, 64, span=5) + 100))
    queries = torch.cat([keys, absent]).contiguous()
    nq = queries.numel()

    def query(table_keys, table_vals):
        def case_q(g):
            g.call("ftx_hashtable_query", ptr(queries), nq, ptr(table_keys), ptr(table_vals), cap, g.out("out", (nq,), I32))
        return run(L, case_q, "ftx_hashtable_query on the guarded table").view("out").cpu().long()
    got, plain = query(tk, tv), query(pk, pv)
    assert torch.equal(got, plain)
    keys_h = keys.cpu()
    first = {}
    for i, key in enumerate(keys_h.tolist()):
        first.setdefault(key, i)                                                 # the smallest row index of every key
    assert got[:n].tolist() == [first[key] for key in keys_h.tolist()] and bool((got[n:] == -1).all())


# ------------------------------------------------------------------------------------------------------------------ sort-based entries
@pytest.mark.parametrize("n", [1, 4097])
def test_unique_sorted(L, n):
    g0 = gen(n + 1)
    keys = hashes_of(L, dev(coords_of(g0, n, span=5)))
    ws_bytes = int(L.ftx_unique_workspace_bytes(n))
    assert ws_bytes > 0 and ws_bytes % 256 == 0

    def case(g):
        uniq, first, count = g.out("uniq", (n,), I64), g.out("first_index", (n,), I32), g.out("n_unique", (1,), I32)
        g.upto("uniq", lambda: g.view("n_unique")[0])
        g.upto("first_index", lambda: g.view("n_unique")[0])
        g.call("ftx_unique_sorted", ptr(keys), n, uniq, first, count, g.ws("ws", ws_bytes), ws_bytes)
    r = run(L, case, "ftx_unique_sorted n=%d" % n, fills=POISON)
    expect, inverse = torch.unique(keys.cpu(), return_inverse=True)
    nu = int(r.view("n_unique")[0])
    assert nu == expect.numel() and torch.equal(r.view("uniq")[:nu].cpu(), expect)
    first = r.view("first_index")[:nu].cpu().long()
    assert torch.equal(keys.cpu()[first], expect)
    assert all(int(first[j]) == int(torch.nonzero(inverse == j)[0]) for j in range(0, nu, max(1, nu // 50)))


LEVEL_STRIDES = {1: [2], 8: [1, 2, 4, 8, 16, 3, 5, 1]}


@pytest.mark.parametrize("with_sorted", [0, 1])
@pytest.mark.parametrize("n_levels", [1, 8])
@pytest.mark.parametrize("n", [1, 4097])
def test_levels_unique_and_level_segments(L, n, n_levels, with_sorted):
    g0 = gen(n + n_levels)
    pts = dev(coords_of(g0, n, span=9))
    strides = np.array(LEVEL_STRIDES[n_levels], dtype=np.int32)
    ws_bytes = int(L.ftx_levels_workspace_bytes(n, n_levels))
    assert ws_bytes > 0 and ws_bytes % 256 == 0
    total = n_levels * n

    def case(g):
        uniq, first, off = g.out("uniq", (total,), I64), g.out("first_index", (total,), I32), g.out("level_off", (n_levels + 1,), I32)
        g.upto("uniq", lambda: g.view("level_off")[n_levels])
        g.upto("first_index", lambda: g.view("level_off")[n_levels])
        skeys = g.out("sorted_keys", (total,), I64) if with_sorted else 0
        order = g.out("order", (total,), I32) if with_sorted else 0
        g.call("ftx_levels_unique", ptr(pts), n, host(strides), n_levels, uniq, first, off, skeys, order, g.ws("ws", ws_bytes), ws_bytes)
    r = run(L, case, "ftx_levels_unique n=%d levels=%d sorted=%d" % (n, n_levels, with_sorted), fills=POISON)
    off = r.view("level_off").cpu().tolist()
    assert off[0] == 0 and all(1 <= b - a <= n for a, b in zip(off, off[1:]))
    if n_levels == 8:
        assert off[1] - off[0] == off[8] - off[7]                              # stride 1 twice: the same set
    if not with_sorted:
        return
    skeys, order = r.view("sorted_keys"), r.view("order")
    assert bool((skeys[1:] >= skeys[:-1]).all()) and int(order.min()) == 0 and int(order.max()) == n - 1
    for level in sorted({0, n_levels - 1}):
        m = off[level + 1] - off[level]
        level_keys, level_uniq = skeys[level * n:(level + 1) * n].contiguous(), r.view("uniq")[off[level]:off[level + 1]].contiguous()

        def seg(g):
            g.call("ftx_level_segments", ptr(level_keys), n, ptr(level_uniq), m, level, g.out("seg_off", (m + 1,), I32))
        s = run(L, seg, "ftx_level_segments n=%d level=%d" % (n, level)).view("seg_off").cpu().long()
        assert int(s[0]) == 0 and int(s[m]) == n and bool((s[1:] > s[:-1]).all())


# ------------------------------------------------------------------------------------------------------------------ pair lists
def injective_map(g0, k, n_out, n_in, empty):
    """nbr (k, n_out): per offset an injective partial map into the n_in input rows (a kernel map never sends two outputs of one
    offset to the same input), about a third absent, the offsets in `empty` absent altogether, the last input row present."""
    nbr = torch.stack([torch.randperm(n_in, generator=g0)[:n_out] for _ in range(k)])
    nbr[torch.rand((k, n_out), generator=g0) < 0.35] = -1
    for kk in empty:
        nbr[kk] = -1
    last = max(kk for kk in range(k) if kk not in empty)
    if not bool((nbr[last] == n_in - 1).any()):
        nbr[last, n_out // 2] = n_in - 1                                          # nobody else of this offset points there
    return nbr.to(I32)


def scan_regimes(lib, k):
    """The two regimes of the validity scan (rocprim::exclusive_scan over k * n_out flags): one block, and the look-back scan over
    more than one, told apart by the entry's own workspace query, which grows with the number of blocks.  Returns the smallest n_out
    of each: 1, and the first size whose workspace is larger than that of one flag row."""
    one = int(lib.ftx_kernel_map_count_workspace_bytes(1, k))
    lo, hi = 1, 1 << 20
    assert int(lib.ftx_kernel_map_count_workspace_bytes(hi, k)) > one
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if int(lib.ftx_kernel_map_count_workspace_bytes(mid, k)) > one else (mid + 1, hi)
    return {"one-block": 1, "largest-of-the-first-workspace-step": lo - 1, "look-back": lo}


@pytest.mark.parametrize("regime", ["one-block", "largest-of-the-first-workspace-step", "look-back"])
@pytest.mark.parametrize("k", [8, 27])
def test_kernel_map_count_and_pairs(L, k, regime):
    n_out = scan_regimes(L, k)[regime]
    if regime != "one-block":
        assert n_out >= 2 and (int(L.ftx_kernel_map_count_workspace_bytes(n_out, k)) > int(L.ftx_kernel_map_count_workspace_bytes(1, k))) == (regime == "look-back")
    n_in = n_out + 37
    g0 = gen(k * 1000 + n_out)
    nbr = injective_map(g0, k, n_out, n_in, empty=[] if n_out == 1 else [3])
    nbr_d = dev(nbr)
    ws_bytes = int(L.ftx_kernel_map_count_workspace_bytes(n_out, k))
    assert ws_bytes % 4 == 0

    def count(g):
        g.call("ftx_kernel_map_count", ptr(nbr_d), n_out, k, g.out("pos", (k, n_out), I32), g.out("koff", (k + 1,), I32), g.ws("ws", ws_bytes), ws_bytes)
    c = run(L, count, "ftx_kernel_map_count k=%d n_out=%d (%s)" % (k, n_out, regime), fills=POISON)
    valid = (nbr >= 0).view(-1).long()
    scan = torch.cumsum(valid, 0) - valid
    koff = c.view("koff").cpu().long()
    assert torch.equal(c.view("pos").cpu().long().view(-1), scan)
    assert torch.equal(koff, torch.cat([scan.view(k, n_out)[:, 0], valid.sum().view(1)]))
    n_pairs = int(koff[k])
    assert n_pairs >= 1 and (n_out == 1 or int(koff[4] - koff[3]) == 0)
    pos0 = c.view("pos").clone()

    def pairs(g):
        g.call("ftx_kernel_map_pairs", ptr(nbr_d), n_out, n_in, k, g.inout("pos", pos0), g.out("pos_t", (k, n_in), I32), g.out("pair_in", (n_pairs,), I32),
               g.out("pair_out", (n_pairs,), I32), n_pairs)
    p = run(L, pairs, "ftx_kernel_map_pairs k=%d n_out=%d" % (k, n_out))
    kk, oo = torch.nonzero(nbr >= 0, as_tuple=True)
    assert torch.equal(p.view("pair_in").cpu().long(), nbr[kk, oo].long()) and torch.equal(p.view("pair_out").cpu().long(), oo)
    pos = p.view("pos").cpu().long()
    assert bool((pos[nbr < 0] == -1).all()) and torch.equal(pos[kk, oo], torch.arange(n_pairs))
    pos_t = p.view("pos_t").cpu().long()
    assert int((pos_t >= 0).sum()) == n_pairs and torch.equal(pos_t[kk, nbr[kk, oo].long()], torch.arange(n_pairs))


# ------------------------------------------------------------------------------------------------------------------ sample_down
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("h,w,oh,ow", [(37, 53, 24, 24), (16, 16, 24, 24), (1, 1, 1, 1)])
def test_sample_down(L, h, w, oh, ow, training):
    b = 2
    g0 = gen(h * 100 + w + training)
    img, go = torch.rand((b, 3, h, w), generator=g0), randn(g0, b, 3, oh, ow)
    conv_w, conv_b = randn(g0, 3, 3) * 0.7, randn(g0, 3) * 0.2 + 0.3
    gamma, beta = torch.rand(3, generator=g0) + 0.5, randn(g0, 3)
    rm0, rv0 = randn(g0, 3), torch.rand(3, generator=g0) + 0.5
    ws_bytes = int(L.ftx_sample_down_workspace_bytes())
    saved = None
    for with_running in ((1, 0) if training else (1,)):
        tag = "%dx%d->%dx%d training=%d running=%d" % (h, w, oh, ow, training, with_running)

        def fwd(g):
            rm = g.inout("running_mean", rm0) if with_running else 0
            rv = g.inout("running_var", rv0) if with_running else 0
            g.call("ftx_sample_down_fwd", g.op(img), b, h, w, oh, ow, g.op(conv_w), g.op(conv_b), g.op(gamma), g.op(beta), rm, rv, 0.1, 1e-5, training,
                   g.out("out", (b, 3, oh, ow)), g.out("saved", (33,), F64), g.ws("ws", ws_bytes), ws_bytes)
        f = run(L, fwd, "ftx_sample_down_fwd " + tag)
        if with_running:
            same = GD.same_bits(f.view("running_mean").cpu(), rm0) and GD.same_bits(f.view("running_var").cpu(), rv0)
            assert same == (not training), "running statistics: updated in training, bit-untouched in eval mode"
        saved = f.view("saved").cpu()
    if not training:
        return

    def bwd(g):
        g.call("ftx_sample_down_bwd", g.op(img), g.op(go), b, h, w, oh, ow, g.op(conv_w), g.op(conv_b), g.op(gamma), g.op(saved), g.out("grad_conv_w", (3, 3)),
               g.out("grad_conv_b", (3,)), g.out("grad_gamma", (3,)), g.out("grad_beta", (3,)), g.ws("ws", ws_bytes), ws_bytes)
    run(L, bwd, "ftx_sample_down_bwd %dx%d->%dx%d" % (h, w, oh, ow))


# ------------------------------------------------------------------------------------------------------------------ losses
LOSS_N = [1, 257, 256 * 256 + 1]
IGNORE = 0


def labels_of(g0, n, c):
    """Labels with ignore_index, values below and past the range, and at least one counted label (so the total weight is positive)."""
    y = torch.randint(0, c, (n,), generator=g0)
    if n > 1:
        y[::7] = IGNORE
        y[3::11] = -1
        y[5::13] = c
        y[n // 2] = c - 1
    else:
        y[0] = c - 1
    return y


def conf_of(g0, c):
    return torch.randint(1, 1000, (c, c), generator=g0)                          # non-zero before the call: the entry accumulates


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("c", [4, 20, 32])
def test_fusion_losses(L, c, n):
    g0 = gen(c * 7 + n)
    logits = [randn(g0, n, c) * 3.0 for _ in range(4)]
    y, y_d = labels_of(g0, n, c), None
    y_d = dev(y, I64)
    cw = torch.rand(c, generator=g0) + 0.25
    conf3, conf2 = conf_of(g0, c), conf_of(g0, c)
    ws_bytes = int(L.ftx_fusion_loss_workspace_bytes())
    counted = int(((y >= 0) & (y < c) & (y != IGNORE)).sum())
    for entry in ("ftx_fusion_loss", "ftx_fusion_loss_mix"):
        for dual, lam, weights, with_conf in [(1, 0.5, 1, 1), (1, 0.0, 0, 1), (0, 0.5, 0, 0), (0, 0.0, 1, 1)]:
            def case(g):
                l3, l2 = g.op(logits[0]), g.op(logits[1])
                l3b, l2b = (g.op(logits[2]), g.op(logits[3])) if dual else (0, 0)
                w_ = g.op(cw) if weights else 0
                outs = [g.out("losses", (2,)), g.out("grad_lidar", (n, c)), g.out("grad_img", (n, c))]
                outs += [g.out("grad_lidar2", (n, c)), g.out("grad_img2", (n, c))] if dual else [0, 0]
                outs += [g.inout("conf3d", conf3), g.inout("conf2d", conf2)] if with_conf else [0, 0]
                mix = (0.5, lam) if entry.endswith("_mix") else (lam,)
                g.call(entry, l3, l2, l3b, l2b, ptr(y_d), w_, *mix, n, c, IGNORE, *outs, g.ws("ws", ws_bytes), ws_bytes)
            r = run(L, case, "%s n=%d c=%d dual=%d lambda=%g weights=%d conf=%d" % (entry, n, c, dual, lam, weights, with_conf))
            if with_conf:
                assert int((r.view("conf3d").cpu() - conf3).sum()) == counted and int((r.view("conf2d").cpu() - conf2).sum()) == counted
                assert bool((r.view("conf3d").cpu() >= conf3).all())


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("c", [4, 20, 32])
def test_seg_loss(L, c, n):
    g0 = gen(c * 11 + n)
    logit = randn(g0, n, c) * 3.0
    y = labels_of(g0, n, c)
    y_d = dev(y, I64)
    cw = torch.rand(c, generator=g0) + 0.25
    conf = conf_of(g0, c)
    ws_bytes = int(L.ftx_seg_loss_workspace_bytes())
    losses = {}
    for with_grad, weights, with_conf in [(1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 0, 1)]:
        def case(g):
            grad = g.out("grad", (n, c), rows=None if with_grad else [])       # grad NULL: the tensor is not passed and must stay sentinel
            g.call("ftx_seg_loss", g.op(logit), ptr(y_d), g.op(cw) if weights else 0, n, c, IGNORE, g.out("loss", (1,)), grad if with_grad else 0,
                   g.inout("conf", conf) if with_conf else 0, g.ws("ws", ws_bytes), ws_bytes)
        r = run(L, case, "ftx_seg_loss n=%d c=%d grad=%d weights=%d conf=%d" % (n, c, with_grad, weights, with_conf))
        losses[(with_grad, weights)] = r.view("loss").clone()
    assert GD.same_bits(losses[(1, 1)], losses[(0, 1)])                          # the forward-only kernel returns the same loss


# ------------------------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("m", [1, 2049])
def test_eval_scatter_back(L, m):
    c, n_rows = 20, 97
    g0 = gen(m)
    l3, l2 = randn(g0, n_rows, c) * 2.0, randn(g0, n_rows, c) * 2.0
    class_labels = dev(torch.tensor([0] + list(range(40, 40 + c - 2)) + [c]))    # id 0 -> num_classes, which is a label id here
    inverse = torch.randint(0, n_rows, (m,), generator=g0)
    inverse[m // 2] = n_rows - 1
    gt = torch.randint(0, c, (m,), generator=g0)
    conf = [conf_of(g0, c) for _ in range(3)]
    names = ["pred3d", "pred2d", "pred_ens", "conf3d", "conf2d", "conf_ens"]

    def make(inv, gt_, skipped, drop):
        inv_d, gt_d = dev(inv, I64), dev(gt_)
        kept = [i for i in range(m) if i not in skipped]

        def case(g):
            a3, a2 = (0 if drop == "logits3d" else g.op(l3)), (0 if drop == "logits2d" else g.op(l2))
            outs = []
            for j, name in enumerate(names):
                # without both logits there is no ensemble, and a head without logits predicts nothing: those outputs stay untouched
                dead = (drop == "logits3d" and name in ("pred3d", "pred_ens")) or (drop == "logits2d" and name in ("pred2d", "pred_ens"))
                if name == drop:
                    outs.append(0)
                elif j < 3:
                    outs.append(g.out(name, (m,), I32, rows=[] if dead else (kept if skipped else None)))
                else:
                    outs.append(g.inout(name, conf[j - 3]))
            g.call("ftx_eval_scatter_back", a3, a2, n_rows, c, ptr(inv_d), ptr(gt_d), m, ptr(class_labels), *outs, g.inout("bad_flag", torch.zeros(1, dtype=I32)))
        return case
    for drop in [None, "logits3d", "logits2d"] + names:
        r = run(L, make(inverse, gt, [], drop), "ftx_eval_scatter_back m=%d without %s" % (m, drop))
        assert int(r.view("bad_flag")[0]) == 0
    bad_inv, bad_gt = inverse.clone(), gt.clone()
    skipped = [0] if m == 1 else [5, 300, 2048]
    bad_inv[skipped[0]] = n_rows                                                 # an inverse index past the rows
    if m > 1:
        bad_inv[skipped[1]] = -1
        bad_gt[skipped[2]] = c                                                   # a gt id past the classes
    r = run(L, make(bad_inv, bad_gt, skipped, None), "ftx_eval_scatter_back m=%d with out-of-range points" % m)
    assert int(r.view("bad_flag")[0]) == 1
    assert int((r.view("conf3d").cpu() - conf[0]).sum()) == m - len(skipped)     # every class id is a label id: every kept point counts


@pytest.mark.parametrize("n", [1, 255, "large"])
def test_project_points(L, n):
    n = rows_for(n)
    g0 = gen(n)
    pts = randn(g0, n, 3) * torch.tensor([20.0, 10.0, 2.0]) + torch.tensor([10.0, 0.0, 0.0])
    proj = torch.tensor([[600.0, -700.0, 5.0, 40.0], [300.0, 4.0, -700.0, -30.0], [1.0, 0.003, 0.002, -0.3]])

    def case(g):
        g.call("ftx_project_points", g.op(pts), n, g.op(proj), 1226, 370, g.out_bytes("keep", n), g.out("rowcol", (n, 2)))
    # rowcol = h / h[2]: a point on the camera plane would divide by zero; the seed has none (the run checks every element finite)
    r = run(L, case, "ftx_project_points n=%d" % n)
    keep = r.byte_outs["keep"][1]
    assert bool((keep <= 1).all()) and (n < 255 or 0 < int(keep.sum()) < n)


# ------------------------------------------------------------------------------------------------------------------ byte images
OPS = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}
CHAINS = {"none": [], "contrast first": [("contrast", 1.3), ("brightness", 0.8)], "contrast in the middle": [("saturation", 1.4), ("contrast", 0.7), ("hue", 0.1)],
          "hue last": [("brightness", 1.2), ("hue", -0.2)]}
OUT_FILLS = (0x5A, 0xC3)


def guarded_call(lib, name, *args):
    """One direct call, as Banded.call makes it: a fault at the launch or at the synchronize ends the session."""
    Fill(lib).call(name, *args)


def image_of(g0, *shape):
    return torch.randint(0, 256, shape, generator=g0, dtype=U8)


def chain_args(chain):
    codes = np.array([OPS[op] for op, _ in chain] + [0] * (4 - len(chain)), dtype=np.int32)
    factors = np.array([f for _, f in chain] + [0.0] * (4 - len(chain)), dtype=np.float64)
    return codes, factors, len(chain)


def byte_workspace(nbytes, fill):
    """(whole, payload, address, nbytes) of a poisoned workspace; nbytes = 0: NULL, as the header allows."""
    if nbytes == 0:
        return None, None, 0, 0
    whole, payload = GD.banded_bytes(nbytes, fill=fill)
    return whole, payload, GD.address(whole, payload), nbytes


JITTER_SIZES = [(1, 1), (5, 7), (33, 128), (33, 130), (513, 2050)]


def jitter_plan(h, w):
    """(chain, source byte offset, destination byte offset) of every run of one size: every chain at every source offset, except on the
    large frame (one pass over it is all the grid cap and the per-block luma partials need)."""
    if h * w > 100000:
        assert h * -(-w // 4) > 2048 * 128                                      # more four-pixel chunks than IMG_MAX_BLOCKS blocks of 128
        return [("contrast first", 1, 0), ("contrast in the middle", 3, 2)]
    return [(name, off, (off + i) % 4) for i, name in enumerate(sorted(CHAINS)) for off in range(4)]


@pytest.mark.parametrize("h,w", JITTER_SIZES)
def test_color_jitter_u8(L, h, w):
    data = image_of(gen(h * 7 + w), h, w, 3)
    ws_bytes = int(L.ftx_color_jitter_workspace_bytes(h, w))
    pitch = 3 * w + 17                                                            # odd: the rows' alignment changes from row to row
    for name, off, dst_off in jitter_plan(h, w):
        codes, factors, n_ops = chain_args(CHAINS[name])
        what = "ftx_color_jitter_u8 %dx%d %s, source at +%d, destination at +%d" % (h, w, name, off, dst_off)

        def go(src_fill, ws_fill, out_fill):
            _, src = GD.banded_u8((h, w, 3), data, pitch=pitch, offset=off, fill=src_fill)
            whole, dst = GD.banded_u8((h, w, 3), offset=dst_off, fill=out_fill)
            ws_whole, ws, ws_ptr, _ = byte_workspace(ws_bytes, ws_fill)
            guarded_call(L, "ftx_color_jitter_u8", src.data_ptr(), pitch, h, w, 3, host(codes), host(factors), n_ops, dst.data_ptr(), ws_ptr, ws_bytes)
            assert GD.bands_intact(ws_whole, ws), what + ": the workspace was used beyond ftx_color_jitter_workspace_bytes"
            return whole, dst
        assert GD.written_u8(lambda fill: go(0x00, 0xFF, fill), OUT_FILLS), what + ": a byte outside the frame was written, or one inside was not"
        first = go(0x00, 0xFF, OUT_FILLS[0])[1]
        assert torch.equal(first, go(0x00, 0x00, OUT_FILLS[0])[1]), what + ": the result changes with the workspace fill"
        assert torch.equal(first, go(0xFF, 0xFF, OUT_FILLS[0])[1]), what + ": the result changes with the bytes beside the source view"
        plain, out = data.cuda().contiguous(), torch.empty((h, w, 3), dtype=U8, device="cuda")
        ws_plain = torch.zeros(ws_bytes, dtype=U8, device="cuda")
        guarded_call(L, "ftx_color_jitter_u8", plain.data_ptr(), 3 * w, h, w, 3, host(codes), host(factors), n_ops, out.data_ptr(), ws_plain.data_ptr(), ws_bytes)
        assert torch.equal(first, out), what + ": differs from the call on a contiguous copy"
        if name == "none":
            assert torch.equal(first.cpu(), data)


@pytest.mark.parametrize("h,w", JITTER_SIZES)
def test_color_jitter_chw(L, h, w):
    data = image_of(gen(h * 11 + w), h, w, 3)
    ws_bytes = int(L.ftx_color_jitter_workspace_bytes(h, w))
    pitch = 3 * w + 17
    mean, std = np.array([0.485, 0.456, 0.406], dtype=np.float32), np.array([0.229, 0.224, 0.225], dtype=np.float32)
    for i, (name, off, _) in enumerate(jitter_plan(h, w)):
        codes, factors, n_ops = chain_args(CHAINS[name])
        flip, norm = i % 2, (i // 2) % 2                                           # flip 0 and 1, mean / std given and NULL, over the runs
        tail = (flip, host(mean) if norm else None, host(std) if norm else None)
        what = "ftx_color_jitter_chw %dx%d %s, source at +%d, flip=%d, normalised=%d" % (h, w, name, off, flip, norm)

        def go(src_fill, ws_fill):
            _, src = GD.banded_u8((h, w, 3), data, pitch=pitch, offset=off, fill=src_fill)
            whole, dst = GD.banded((3, h, w))
            ws_whole, ws, ws_ptr, _ = byte_workspace(ws_bytes, ws_fill)
            guarded_call(L, "ftx_color_jitter_chw", src.data_ptr(), pitch, h, w, 3, host(codes), host(factors), n_ops, *tail, GD.address(whole, dst), ws_ptr, ws_bytes)
            assert GD.bands_intact(ws_whole, ws), what + ": the workspace was used beyond ftx_color_jitter_workspace_bytes"
            assert GD.bands_intact(whole, dst), what + ": a guard band of the output was written"
            assert GD.written(dst), what + ": an output element was not written"
            return dst
        first = go(0x00, 0xFF)
        assert GD.same_bits(first, go(0x00, 0x00)), what + ": the result changes with the workspace fill"
        assert GD.same_bits(first, go(0xFF, 0xFF)), what + ": the result changes with the bytes beside the source view"
        plain, out = data.cuda().contiguous(), torch.empty((3, h, w), dtype=F32, device="cuda")
        ws_plain = torch.zeros(ws_bytes, dtype=U8, device="cuda")
        guarded_call(L, "ftx_color_jitter_chw", plain.data_ptr(), 3 * w, h, w, 3, host(codes), host(factors), n_ops, *tail, out.data_ptr(), ws_plain.data_ptr(), ws_bytes)
        assert GD.same_bits(first, out), what + ": differs from the call on a contiguous copy"


def frames_u8(data, pitch, frame_stride, offset, fill):
    """(n_frames, h, w, 3) frames `frame_stride` bytes apart with row pitch `pitch`, the first byte `offset` bytes past a 256-byte
    boundary, inside a larger allocation that holds `fill` everywhere else: between the rows, between the frames and in both bands."""
    nf, h, w, _ = data.shape
    assert pitch >= 3 * w and frame_stride >= h * pitch
    whole = torch.full((2 * GD.U8_BAND_BYTES + (nf - 1) * frame_stride + h * pitch,), fill, dtype=U8, device="cuda")
    view = torch.as_strided(whole, (nf, h, w, 3), (frame_stride, pitch, 3, 1), GD.U8_BAND_BYTES + offset)
    view.copy_(data)
    return whole, view


# (in_h, in_w, out_h, out_w): both axes shrinking (out_w % 4 = 3) and enlarging (1); x only (2: no workspace); y only (0: no workspace);
# 520 -> 4 columns: ksize 261, 261 * 64 coefficients > RS_LDS_INTS = 8192, so they are read from the table and not from LDS
RESIZE_CASES = [(37, 53, 24, 31), (9, 7, 20, 33), (12, 53, 12, 30), (37, 16, 24, 16), (5, 520, 3, 4)]


@pytest.mark.parametrize("in_h,in_w,out_h,out_w", RESIZE_CASES)
def test_resize_bilinear_u8(L, in_h, in_w, out_h, out_w):
    from fusiontransformer_amd import functional as spf
    nf = 2
    data = image_of(gen(in_h * 13 + in_w), nf, in_h, in_w, 3)
    bx, kx, ksx = spf.resize_table(in_w, out_w, "cuda") if in_w != out_w else (None, None, 0)
    by, ky, ksy = spf.resize_table(in_h, out_h, "cuda") if in_h != out_h else (None, None, 0)
    ws_bytes = int(L.ftx_resize_workspace_bytes(nf, in_h, in_w, out_h, out_w))
    assert (ws_bytes == 0) == (in_h == out_h or in_w == out_w) and (in_w != 520 or ksx == 261)
    pitch = 3 * in_w + 7
    stride = in_h * pitch + 2 * pitch + 5                                         # larger than the frame, and odd
    tables = (ptr(bx), ptr(kx), ksx, ptr(by), ptr(ky), ksy, out_h, out_w)
    for off, dst_off in ((1, 0), (3, 1), (2, 3)):
        what = "ftx_resize_bilinear_u8 %dx%d -> %dx%d, source at +%d, destination at +%d" % (in_h, in_w, out_h, out_w, off, dst_off)

        def go(src_fill, ws_fill, out_fill):
            _, src = frames_u8(data, pitch, stride, off, src_fill)
            whole, dst = GD.banded_u8((nf * out_h, out_w, 3), offset=dst_off, fill=out_fill)
            ws_whole, ws, ws_ptr, _ = byte_workspace(ws_bytes, ws_fill)
            guarded_call(L, "ftx_resize_bilinear_u8", src.data_ptr(), stride, pitch, nf, in_h, in_w, 3, *tables, dst.data_ptr(), ws_ptr, ws_bytes)
            assert ws_whole is None or GD.bands_intact(ws_whole, ws), what + ": the workspace was used beyond ftx_resize_workspace_bytes"
            return whole, dst
        assert GD.written_u8(lambda fill: go(0x00, 0xFF, fill), OUT_FILLS), what + ": a byte outside the frames was written, or one inside was not"
        first = go(0x00, 0xFF, OUT_FILLS[0])[1]
        assert torch.equal(first, go(0x00, 0x00, OUT_FILLS[0])[1]), what + ": the result changes with the workspace fill"
        assert torch.equal(first, go(0xFF, 0xFF, OUT_FILLS[0])[1]), what + ": the result changes with the bytes beside the source view"
        plain, out = data.cuda().contiguous(), torch.empty((nf, out_h, out_w, 3), dtype=U8, device="cuda")
        ws_plain = torch.zeros(max(ws_bytes, 16), dtype=U8, device="cuda")
        guarded_call(L, "ftx_resize_bilinear_u8", plain.data_ptr(), in_h * in_w * 3, in_w * 3, nf, in_h, in_w, 3, *tables, out.data_ptr(),
                     ws_plain.data_ptr() if ws_bytes else 0, ws_bytes)
        assert torch.equal(first.reshape(nf, out_h, out_w, 3), out), what + ": differs from the call on contiguous frames"


# ------------------------------------------------------------------------------------------------------------------ Adam
ADAM_SIZES = [1, 5, 16384, 16385, 16387, 70001]
ADAM_FORMS = {"all four pointers 16-byte aligned": (0, 0, 0, 0), "only g at 4-byte alignment": (0, 0, 0, 1), "p, m, v at 4-byte alignment": (1, 2, 3, 0)}
ADAM = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=5e-4, step=3)


def adam_tables(lib, tensors):
    """The device table and the chunk map of ftx_adam_step for [(p, m, v, g or None)], built here from optim._REC."""
    from fusiontransformer_amd.optim import _REC
    assert int(lib.ftx_adam_tensor_bytes()) == _REC.itemsize
    chunk = int(lib.ftx_adam_chunk_elements())
    rec = np.zeros(len(tensors), dtype=_REC)
    t = float(ADAM["step"])
    for r, (p, m, v, g) in zip(rec, tensors):
        r["p"], r["m"], r["v"], r["g"], r["n"] = p.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if g is None else g.data_ptr(), p.numel()
        r["step_size"] = np.float32(ADAM["lr"] / (1.0 - ADAM["beta1"] ** t))
        r["inv_bc2_sqrt"] = np.float32(1.0 / np.sqrt(1.0 - ADAM["beta2"] ** t))
    per = [-(-p.numel() // chunk) for p, _, _, _ in tensors]
    tid = np.repeat(np.arange(len(tensors), dtype=np.int32), per)
    off = np.concatenate([np.arange(k, dtype=np.int64) * chunk for k in per])
    table = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    return table, torch.from_numpy(tid).cuda(), torch.from_numpy(off).cuda(), int(sum(per))


@pytest.mark.parametrize("form", sorted(ADAM_FORMS))
def test_adam_step(L, form):
    g0 = gen(len(form))
    sizes = ADAM_SIZES + [16385]                                                   # the last tensor has no gradient this step
    skipped = len(sizes) - 1
    base = [(randn(g0, n), randn(g0, n) * 0.1, torch.rand(n, generator=g0) * 0.01, randn(g0, n)) for n in sizes]
    shift = ADAM_FORMS[form]

    def build(guarded):
        rows = []
        for i, (p, m, v, g) in enumerate(base):
            if not guarded:
                rows.append([(None, t.cuda().clone()) for t in (p, m, v)] + [(None, g.cuda())])
                continue
            band = GD.band_width(p.shape)
            rows.append([GD.banded(p.shape, t, inout=True, band=band + s) for t, s in zip((p, m, v), shift[:3])] + [GD.banded(g.shape, g, band=band + shift[3])])
            assert [view.data_ptr() % 16 for _, view in rows[-1]] == [4 * s % 16 for s in shift]
        tensors = [(r[0][1], r[1][1], r[2][1], None if i == skipped else r[3][1]) for i, r in enumerate(rows)]
        table, tid, off, n_chunks = adam_tables(L, tensors)
        guarded_call(L, "ftx_adam_step", table.data_ptr(), tid.data_ptr(), off.data_ptr(), n_chunks, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], ADAM["weight_decay"])
        return rows
    guarded, plain = build(True), build(False)
    for i, (rows_g, rows_p) in enumerate(zip(guarded, plain)):
        for name, (whole, view), (_, ref), before in zip("pmv", rows_g, rows_p, base[i]):
            what = "ftx_adam_step, %s, tensor of %d: %s" % (form, sizes[i], name)
            assert GD.bands_intact(whole, view), what + ": a guard band was written"
            assert GD.written(view), what + ": an element was not written, or a gradient band was read"
            assert GD.same_bits(view, ref), what + " differs from the call on plain tensors"
            assert GD.same_bits(view.cpu(), before) == (i == skipped), what + (": a skipped tensor was touched" if i == skipped else ": nothing was updated")
    # one step of torch.optim.Adam from the same state, at the tolerances of test_adam_one_launch_matches_torch_adam
    params = [torch.nn.Parameter(p.cuda().clone()) for p, _, _, _ in base[:skipped]]
    opt = torch.optim.Adam(params, lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"], weight_decay=ADAM["weight_decay"])
    for prm, (_, m, v, g) in zip(params, base):
        opt.state[prm].update(step=torch.tensor(float(ADAM["step"] - 1)), exp_avg=m.cuda().clone(), exp_avg_sq=v.cuda().clone())
        prm.grad = g.cuda().clone()
    opt.step()
    for prm, rows_g in zip(params, guarded):
        np.testing.assert_allclose(rows_g[0][1].cpu().numpy(), prm.detach().cpu().numpy(), rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(rows_g[1][1].cpu().numpy(), opt.state[prm]["exp_avg"].cpu().numpy(), rtol=2e-6, atol=1e-8)
        np.testing.assert_allclose(rows_g[2][1].cpu().numpy(), opt.state[prm]["exp_avg_sq"].cpu().numpy(), rtol=2e-6, atol=1e-10)


# ------------------------------------------------------------------------------------------------------------------ rows
# (ca, cb): the header's minimum, the widths SPVCNN concatenates (32 + 96) and the ViT's token width beside the minimum
@pytest.mark.parametrize("ca,cb", [(4, 4), (32, 96), (768, 4)])
@pytest.mark.parametrize("n", [1, 257])
def test_rows_entries(L, n, ca, cb):
    g0 = gen(n + ca + cb)
    a, b, both, a2, pb = randn(g0, n, ca), randn(g0, n, cb), randn(g0, n, ca + cb), randn(g0, n, ca), randn(g0, ca)
    tag = "n=%d %d+%d" % (n, ca, cb)

    def concat(g):
        g.call("ftx_rows_concat", g.op(a), ca, g.op(b), cb, n, g.out("out", (n, ca + cb)))
    r = run(L, concat, "ftx_rows_concat " + tag, band=GD.dense_band)
    assert GD.same_bits(r.view("out").cpu(), torch.cat([a, b], 1))

    def split(g):
        g.call("ftx_rows_split", g.op(both), n, ca, cb, g.out("a", (n, ca)), g.out("b", (n, cb)))
    r = run(L, split, "ftx_rows_split " + tag, band=GD.dense_band)
    assert GD.same_bits(r.view("a").cpu(), both[:, :ca].contiguous()) and GD.same_bits(r.view("b").cpu(), both[:, ca:].contiguous())

    def add(g):
        g.call("ftx_rows_add", g.op(a), g.op(a2), n, ca, g.out("out", (n, ca)))
    run(L, add, "ftx_rows_add " + tag, band=GD.dense_band)
    for with_p in (1, 0):
        def add_bias(g):
            g.call("ftx_rows_add_bias", g.op(a), g.op(a2) if with_p else 0, g.op(pb) if with_p else 0, n, ca, g.out("out", (n, ca)))
        run(L, add_bias, "ftx_rows_add_bias %s p=%d" % (tag, with_p), band=GD.dense_band)


# ------------------------------------------------------------------------------------------------------------------ ViT input side
VIT_P, VIT_C, VIT_CO = 16, 3, 96
# the two smallest of tests/test_native_image_gpu.py::PATCH_CASES by operand size, and the smaller one again without a distillation token
VIT_PATCH = [(1, 384, 256, 2), (3, 80, 768, 2), (3, 80, 768, 1)]
VIT_TAP = [(3, 25, 768), (1, 576, 256)]              # the two smallest of that file's tap-stem list


def test_vit_cases_are_the_smallest_of_the_value_tests():
    from tests.test_native_image_gpu import PATCH_CASES
    order = sorted(PATCH_CASES, key=lambda c: c[0] * c[1] * c[1] * VIT_C + c[2] * VIT_C * VIT_P * VIT_P)
    assert [tuple(c[:4]) for c in order[:2]] == VIT_PATCH[:2]


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("b,side,dim,t0", VIT_PATCH)
def test_vit_patch_embed(L, b, side, dim, t0, mode):
    g0 = gen(b + side + dim + t0)
    gp = (side // VIT_P) ** 2
    img, w, bias = randn(g0, b, VIT_C, side, side), randn(g0, dim, VIT_C * VIT_P * VIT_P) * 0.02, randn(g0, dim) * 0.1
    cls, dist, pos = randn(g0, dim) * 0.02, randn(g0, dim) * 0.02, randn(g0, t0 + gp, dim) * 0.02

    def case(g):
        args = [g.op(img), g.op(w), g.op(bias), g.op(cls), g.op(dist) if t0 == 2 else 0, g.op(pos)]
        tokens = g.out("tokens", (b, t0 + gp, dim))
        if not isinstance(g, Plain):                                             # 16-byte aligned and no more
            assert all(v % 32 == 16 for v in args + [tokens] if v)
        g.call("ftx_vit_patch_embed_" + mode, *args, b, VIT_C, side, side, VIT_P, dim, t0, tokens)
    run(L, case, "ftx_vit_patch_embed_%s b=%d side=%d dim=%d t0=%d" % (mode, b, side, dim, t0), band=GD.dense_band)


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("t0", [2, 0])
@pytest.mark.parametrize("b,gp,dim", VIT_TAP)
def test_vit_tap_stem(L, b, gp, dim, t0, mode):
    g0 = gen(b + gp + dim + t0)
    tokens, w, bias = randn(g0, b, t0 + gp, dim), randn(g0, VIT_CO, dim) * 0.05, randn(g0, VIT_CO) * 0.5
    gamma, beta, rm, rv = torch.rand(VIT_CO, generator=g0) + 0.5, randn(g0, VIT_CO) * 0.2, randn(g0, VIT_CO) * 0.3, torch.rand(VIT_CO, generator=g0) + 0.5

    def case(g):
        args = [g.op(t) for t in (tokens, w, bias, gamma, beta, rm, rv)]
        g.call("ftx_vit_tap_stem_" + mode, *args, 1e-5, b, gp, t0, dim, VIT_CO, g.out("out", (b, gp, VIT_CO)))
    run(L, case, "ftx_vit_tap_stem_%s b=%d g=%d dim=%d t0=%d" % (mode, b, gp, dim, t0), band=GD.dense_band)


# ------------------------------------------------------------------------------------------------------------------ arenas of the executors
class Arenas:
    """arena(nbytes): exactly nbytes bytes, the first 256-byte aligned, holding `fill`, between sentinel bands; every arena handed out
    is kept, so that the bands of all of them can be checked after every call."""

    def __init__(self, fill):
        self.fill, self.made = fill, []

    def __call__(self, nbytes):
        whole, payload = GD.banded_bytes(nbytes, fill=self.fill)
        arena = payload.view(U8)
        assert arena.shape[0] == nbytes and arena.data_ptr() % GD.ALIGN == 0
        self.made.append((whole, payload))
        return arena

    def refill(self):
        for _, payload in self.made:
            payload.fill_(-1 if self.fill == 0xFF else 0)

    def check(self, what):
        settle(what)
        for i, (whole, payload) in enumerate(self.made):
            assert GD.bands_intact(whole, payload), "%s: arena %d (%d bytes, 0x%02X) was used beyond its *_arena_bytes figure" % (what, i, 4 * payload.numel(), self.fill)


def settle(what):
    """Wait for the device; a fault ends the session, as in Banded.call."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("%s faulted on the GPU: %s" % (what, e), returncode=3)


def finite(t):
    return bool(torch.isfinite(t).all())


def test_spvcnn_eval_arena_on_the_empty_map_program(L):
    from fusiontransformer_amd import functional as spf
    from tests.test_native_eval_gpu import empty_map_program
    args, need, shape, ref, keep = empty_map_program(spf)
    plain, out0 = torch.empty(need, dtype=U8, device="cuda"), torch.empty(shape, dtype=F32, device="cuda")
    spf.check(L.ftx_spvcnn_eval(*args, plain.data_ptr(), need, out0.data_ptr(), spf.stream()), "ftx_spvcnn_eval")
    settle("ftx_spvcnn_eval")
    assert GD.same_bits(out0, ref)                                               # what the existing test asserts of a torch.empty arena
    for fill in POISON:
        pool = Arenas(fill)
        arena = pool(need)
        whole, out = GD.banded(shape)
        spf.check(L.ftx_spvcnn_eval(*args, arena.data_ptr(), need, GD.address(whole, out), spf.stream()), "ftx_spvcnn_eval")
        pool.check("ftx_spvcnn_eval, empty map, arena 0x%02X" % fill)
        assert GD.bands_intact(whole, out) and GD.written(out)
        assert GD.same_bits(out, out0), "the result changes with the arena's contents (0x%02X)" % fill


def index_tables(t):
    """Every table the three phases hand back, as clones of the views ftx_spvcnn_index_layout names (the hash tables' slot layout depends
    on the order of the inserts and stays out; what they answer is in nbr and in the corner rows)."""
    from fusiontransformer_amd import native_index as nx
    from fusiontransformer_amd.native_eval import MAP_KEYS, PV_STRIDES, STRIDES
    n, c_in, off, bwd = t["n"], t["c_in"], t["off"], t["bwd"]
    lay = nx.layout(n, c_in, off, t["pairs"], bwd)
    A, B, C = t["a"], t["b"], t["c"]
    assert (A.shape[0], B.shape[0], C.shape[0]) == (lay["a_total"], lay["b_total"], lay["c_total"])
    sizes, total = [int(off[l + 1] - off[l]) for l in range(5)], int(off[5])
    out = {"points": nx._view(A, lay["a_points"], "i32", n, 4), "uniq": nx._view(A, lay["a_uniq"], "i64", 5 * n)[:total],
           "first": nx._view(A, lay["a_first"], "i32", 5 * n)[:total], "sorted_keys": nx._view(A, lay["a_skeys"], "i64", 5, n),
           "order": nx._view(A, lay["a_order"], "i32", 5, n), "x0": nx._view(B, lay["x0"], "f32", sizes[0], c_in)}
    for l in range(5):
        out["coords%d" % l] = nx._view(B, lay["coords%d" % l], "i32", sizes[l], 4)
    for m, (ks, s, stride) in enumerate(MAP_KEYS):
        l, sub = STRIDES.index(s), stride == 1
        k, n_in, n_out = (27, sizes[l], sizes[l]) if sub else (8, sizes[l], sizes[l + 1])
        n_pairs, arena = (int(t["pairs"][l]), C) if sub else (n_in, B)
        out["nbr%d" % m], out["pos%d" % m] = nx._view(B, lay["nbr%d" % m], "i32", k, n_out), nx._view(B, lay["pos%d" % m], "i32", k, n_out)
        out["koff%d" % m], out["pos_t%d" % m] = nx._view(B, lay["koff%d" % m], "i32", k + 1), nx._view(arena, lay["pos_t%d" % m], "i32", k, n_in)
        out["pair_in%d" % m], out["pair_out%d" % m] = nx._view(arena, lay["pair_in%d" % m], "i32", n_pairs), nx._view(arena, lay["pair_out%d" % m], "i32", n_pairs)
    for j, s in enumerate(PV_STRIDES):
        m = sizes[STRIDES.index(s)]
        out["vidx%d" % j], out["vcnt%d" % j], out["vseg%d" % j] = (nx._view(B, lay["vidx%d" % j], "i32", n), nx._view(B, lay["vcnt%d" % j], "i32", m),
                                                                    nx._view(B, lay["vseg%d" % j], "i32", m + 1))
        out["didx%d" % j], out["dw%d" % j] = nx._view(B, lay["didx%d" % j], "i32", n, 8), nx._view(B, lay["dw%d" % j], "f32", n, 8)
        if bwd:
            seg = nx._view(B, lay["dseg%d" % j], "i32", m + 1)
            out["dseg%d" % j] = seg
            out["dorder%d" % j] = nx._view(B, lay["dorder%d" % j], "i32", 8 * n)[:int(seg[m])]      # behind the last segment: dropped entries
    return {k: v.clone() for k, v in out.items()}


@pytest.fixture(scope="module")
def c_caller():
    from tests.test_native_index_gpu import c_caller_inputs
    return c_caller_inputs()


@pytest.mark.parametrize("bwd", [0, 1], ids=["forward", "with_backward_segments"])
def test_index_builder_arenas(L, c_caller, bwd):
    """ftx_spvcnn_index_levels / _maps / _pairs of the C-caller recipe: arenas A, B and C of exactly their own figures, 0xFF then 0x00."""
    from tests.test_native_index_gpu import c_caller_index
    feats, coords, _ = c_caller
    plain = c_caller_index(L, feats, coords, with_backward_segments=bwd)
    want = index_tables(plain)
    assert finite(want["x0"]) and all(finite(want["dw%d" % j]) for j in range(3))
    for fill in POISON:
        pool = Arenas(fill)
        t = c_caller_index(L, feats, coords, arena=pool, with_backward_segments=bwd, after=lambda phase, buf: pool.check("ftx_spvcnn_index_" + phase))
        assert len(pool.made) == 3
        assert list(t["off"]) == list(plain["off"]) and list(t["pairs"]) == list(plain["pairs"]) and list(t["rows"]) == list(plain["rows"])
        for key in ("n_pairs", "n_in", "n_out", "kvol", "fine_bijective"):
            assert list(t["maps"][key]) == list(plain["maps"][key]), key
        assert list(t["pvs"]["n_vox"]) == list(plain["pvs"]["n_vox"])
        got = index_tables(t)
        assert got.keys() == want.keys()
        for key in want:
            assert GD.same_bits(got[key], want[key]), "%s changes with the arenas' contents (0x%02X)" % (key, fill)


def test_spvcnn_eval_arena_on_the_full_program(L, c_caller):
    from tests.test_native_index_gpu import _build, c_caller_eval, c_caller_index
    cfg, model, net, _ = _build("lidar", seed=2)
    model.eval()
    feats, coords, _ = c_caller
    tables = c_caller_index(L, feats, coords)
    z3, _ = c_caller_eval(L, net, tables)
    assert finite(z3)
    for fill in POISON:
        pool = Arenas(fill)
        got, _ = c_caller_eval(L, net, tables, arena=pool)
        pool.check("ftx_spvcnn_eval, full program, arena 0x%02X" % fill)
        assert len(pool.made) == 1 and GD.same_bits(got, z3), "the point features change with the arena's contents (0x%02X)" % fill


def test_vit_eval_arena(L):
    from fusiontransformer_amd import native_image as ni
    from tests.test_native_image_gpu import CO, GRID as VGRID, SIDE, C, _image_net, rnd
    kind, depth, b = "middle", 3, 2
    net = _image_net(kind, depth, "split")
    x = rnd(gen(5), b, C, SIDE, SIDE)
    with torch.no_grad():
        tokens_in = net.backbone._embed(x).contiguous()
    model, blocks, taps, _ = ni.emit(net)
    lin, att = ni.modes(net)
    need = ni.arena_bytes(model, len(blocks), b)
    plain = torch.empty(need, dtype=U8, device="cuda")
    want = [torch.full((b, VGRID, VGRID, CO), float("nan"), device="cuda") for _ in taps]
    ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, depth - 1, lin, att, want, plain)
    settle("ftx_vit_eval")
    assert L.ftx_vit_eval_release(plain.data_ptr()) == 0 and all(finite(o) for o in want)

    def outs():
        made = [GD.banded((b, VGRID, VGRID, CO)) for _ in taps]
        return made, [view for _, view in made]
    for fill in POISON:
        pool = Arenas(fill)
        arena = pool(need)
        what = "ftx_vit_eval, arena 0x%02X" % fill
        try:
            made, whole_run = outs()
            ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, depth - 1, lin, att, whole_run, arena)
            pool.check(what + ", one call")
            pool.refill()                                                        # block by block on the same arena, poisoned again
            made2, parts = outs()
            for i in range(depth):
                n = sum(1 for t in taps if int(t["block"]) <= i)
                ni.eval_call(model, blocks, taps, b, None, tokens_in if i == 0 else None, i, i, lin, att, parts[:n], arena)
                pool.check(what + ", block %d" % i)
        finally:
            assert L.ftx_vit_eval_release(arena.data_ptr()) == 0
        for (w1, o1), (w2, o2), ref in zip(made, made2, want):
            assert GD.bands_intact(w1, o1) and GD.bands_intact(w2, o2) and GD.written(o1) and GD.written(o2)
            assert GD.same_bits(o1, ref) and GD.same_bits(o2, ref), "a tap output changes with the arena's contents (0x%02X)" % fill


def test_spvcnn_train_arena(L, monkeypatch):
    """ftx_spvcnn_train_fwd / _bwd through native_train's own table builder on the smallest batch of tests/test_native_train_gpu.py: the
    model runs in banded arenas of exactly ftx_spvcnn_train_arena_bytes (0xFF for one step, 0x00 for the next), its twin in torch.empty
    arenas; predictions, losses, gradients, parameters and buffers agree bit for bit after every step."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.native_train import NativeTrain
    from tests.test_native_train_gpu import _pair, _twin_steps
    batch = make_batch([2], max_points=1700)
    cfg, model, twin, net, net_twin = _pair("lidar", seed=3)
    net.set_native_train(True)
    net_twin.set_native_train(True)
    begin, pools = NativeTrain.begin, []

    def banded_begin(self, z, x0):
        if self is net_twin._native_tr or not pools:
            return begin(self, z, x0)
        return begin(self, z, x0, arena=pools[-1])
    monkeypatch.setattr(NativeTrain, "begin", banded_begin)
    for fill in POISON:
        pools.append(Arenas(fill))
        preds = _twin_steps("lidar", cfg, model, twin, net, net_twin, [(batch, None)])
        pools[-1].check("ftx_spvcnn_train_fwd / _bwd, arena 0x%02X" % fill)
        assert len(pools[-1].made) == 1 and pools[-1].made[0][1].numel() * 4 == net._native_tr.last_arena_bytes
        assert all(finite(v) for v in preds.values() if torch.is_tensor(v) and v.dtype.is_floating_point)
    assert net._native_tr.runs == 2 and net_twin._native_tr.runs == 2


# ------------------------------------------------------------------------------------------------------------------ the gates can tell
def test_the_gates_report_planted_faults(L):
    """On the device, with torch ops standing in for a faulty kernel: a word behind an arena, a byte behind a row of a byte image, a
    byte of it left unwritten, and a specified row of a partly specified output left on the sentinel."""
    pool = Arenas(0xFF)
    arena = pool(1024)
    pool.check("intact")
    whole, payload = pool.made[0]
    end = payload.storage_offset() + payload.numel()
    whole[end] = 0
    with pytest.raises(AssertionError, match="beyond its"):
        pool.check("planted")
    assert bool((arena == 0xFF).all())
    data = image_of(gen(3), 5, 7, 3)
    codes, factors, n_ops = chain_args(CHAINS["none"])

    def go(fill, plant):
        whole, dst = GD.banded_u8((5, 7, 3), offset=1, fill=fill)
        src = data.cuda()
        guarded_call(L, "ftx_color_jitter_u8", src.data_ptr(), 21, 5, 7, 3, host(codes), host(factors), n_ops, dst.data_ptr(), 0, 0)
        if plant == "stray":
            whole[dst.storage_offset() + 21 * 5] = 255 - fill                    # the byte behind the last pixel
        if plant == "unwritten":
            dst[2, 3, 1] = fill
        return whole, dst
    assert GD.written_u8(lambda fill: go(fill, None), OUT_FILLS)
    assert not GD.written_u8(lambda fill: go(fill, "stray"), OUT_FILLS) and not GD.written_u8(lambda fill: go(fill, "unwritten"), OUT_FILLS)
    keys = hashes_of(L, dev(coords_of(gen(4), 300, span=3)))
    ws_bytes = int(L.ftx_unique_workspace_bytes(300))

    def case(g):
        uniq, first, count = g.out("uniq", (300,), I64), g.out("first_index", (300,), I32), g.out("n_unique", (1,), I32)
        g.upto("uniq", lambda: g.view("n_unique")[0])
        g.upto("first_index", lambda: g.view("n_unique")[0])
        g.call("ftx_unique_sorted", ptr(keys), 300, uniq, first, count, g.ws("ws", ws_bytes), ws_bytes)
    r = run(L, case, "ftx_unique_sorted")
    nu = int(r.view("n_unique")[0])
    assert 1 < nu < 300
    r.view("first_index")[nu - 1] = GD.SENTINEL
    with pytest.raises(AssertionError, match="specified row"):
        r.check("planted")
