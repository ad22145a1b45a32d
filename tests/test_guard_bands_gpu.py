"""Where the LiDAR and ViT-linear kernels write and what they read: every entry called directly through the C ABI on guard-banded
tensors (tests/guard.py).  Every assertion is bitwise or structural; there is no tolerance in this file.

Every case calls its entry with float operands between NaN bands, outputs between sentinel bands and a poisoned workspace of exactly
the size the entry's own *_workspace_bytes query returns, and asserts
  (a) every band of every output, in/out tensor and workspace is intact;
  (b) every output element was written and is finite (or, where include/ftx.h documents a region as untouched, that it still holds
      the sentinel word for word);
  (c) the output is bit-identical to the same entry called on plain contiguous tensors with a plain workspace.
Integer operands are plain tensors with in-range contents (tests/guard.py says why).  Shapes are the smallest that reach each write
pattern; which tile, block count, split or reduce width a case reaches is asserted through the library's host queries
(tests/spconv_regimes.py).  The sixteen weight-gradient instantiations need the ordered reduce at its 16 lanes: 40 000 pairs do
that for fourteen of them, the two with a 128 x 128 tile on both sides need 450 000 (spread evenly over the offsets, so the operands
stay at 9 MB and the workspace at 23 MB).  A call whose launch fails or whose synchronize reports a fault ends the session.

Per entry (include/ftx.h), which of (a) (b) (c) is asserted:

  sparse convolution, fp32 and bf16 twins alike ("no float atomics, bit-reproducible" / "No atomics")
    ftx_spconv_pairs_gemm[_bf16]            a b c   tmp (n_pairs, co)
    ftx_spconv_pairs_gemm_scatter[_bf16]    a b c   b: rows named by scatter finite, every other row still the sentinel ("left untouched")
    ftx_rows_gemm[_bf16]                    a b c
    ftx_spconv_reduce                       a b c
    ftx_spconv_reduce_stats                 a b c   out and part (nb + 1, 2, co) float64; ticket counters zero afterwards
    ftx_spconv_reduce_bn_eval               a b c
    ftx_spconv_ostat                        a b c   out, and part when given; ticket counters zero afterwards
    ftx_spconv_pairs_wgrad[_bf16]           a b c   dW; the workspace is an upper bound (ceil(P / len) + kvol tiles) and may stay partly
                                                    sentinel: only its bands are asserted
    ftx_spconv_gemm_block_cols, _ostat_supported, _ostat_blocks, _reduce_stats_blocks, _wgrad_*_blocks, *_workspace_bytes: host
    queries, launch nothing; used here to pick and assert the regimes.
  norms (fixed summation orders, no atomics on floats: the ticket counters are integers)
    ftx_bn_train_fwd                        a b c   y, save_mean, save_invstd, running_* (in/out); ticket counters zero afterwards
    ftx_bn_train_fwd_totals                 a b c
    ftx_bn_eval_fwd                         a b c
    ftx_bn_train_bwd                        a b c   grad_x, grad_residual (when given), grad_gamma, grad_beta; recompute and y paths
    ftx_colsum                              a b c
    ftx_add_layernorm_fwd                   a b c   y NULL: s_out is documented as not written and must keep the sentinel
    ftx_add_layernorm_bwd                   a b c   grad_params (2, c) or (3, c)
    ftx_stream_scratch_attach / _release    the attached buffer's bands; the counter region is zero after every statistics call
  dense GEMM, ftx_dense_*_bf16 and ftx_dense_*_split ("No atomics ... deterministic"), every tensor at 16-byte alignment only
    ftx_dense_gemm_*                        a b c   pre_out written under BIAS_GELU, sentinel under the other epilogues ("ignored")
    ftx_dense_wgrad_*                       a b c   one split: the workspace must stay untouched
    ftx_dense_*_tile, ftx_dense_wgrad_*_workspace_bytes: host queries.
  point <-> voxel and lift
    ftx_voxelize_fwd, ftx_devoxelize_bwd, ftx_lift_gather_bwd     a b     float atomics (they have _sorted / segment forms beside them)
    ftx_resample_nearest_bwd                a b     its kernel scatter-adds with atomicAdd (csrc/ftx_pointvoxel.hip)
    ftx_voxelize_bwd, ftx_devoxelize_fwd    a b c   gathers
    ftx_segment_build                       a b c   order (n), seg_off (m + 1) int32; also equal to a stable sort on the host
    ftx_voxelize_fwd_sorted, ftx_devoxelize_bwd_sorted, ftx_segment_sum    a b c
    ftx_lift_gather_fwd, ftx_lift_cells, ftx_resample_nearest_fwd          a b c
  every other entry that launches a kernel (sample_down, the kernel-map, hashing and index entries, the losses, the evaluation, resize /
  jitter, Adam, the rows entries, the ViT patch-embed / tap-stem entries, the executors and the native index builder):
  tests/test_guard_bands_rest_gpu.py.  Attention, the affine sampling and the localisation net have guard tests of their own."""
import ctypes

import pytest
import torch

from tests import guard as GD
from tests import spconv_regimes as S
from tests.norm_ref import gen, randn
from tests.test_spconv_bf16_gpu import wgrad_bf16_tile_len
from tests.test_spconv_regimes_gpu import GEMM_CASES, WGRAD_CASES, pair_list, random_sizes

pytestmark = pytest.mark.gpu
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


# ------------------------------------------------------------------------------------------------------------------ the harness
class Tickets:
    """A side stream with a banded ticket buffer of the test's own attached to it (never the default stream's buffer)."""

    def __init__(self, lib):
        from fusiontransformer_amd._lib import check
        self.lib, self.stream = lib, torch.cuda.Stream()
        self.raw = self.stream.cuda_stream
        nbytes = int(lib.ftx_stream_scratch_bytes())
        self.whole, self.buf = GD.banded_bytes(nbytes)
        torch.cuda.synchronize()
        check(lib.ftx_stream_scratch_attach(self.raw, GD.address(self.whole, self.buf), nbytes), "ftx_stream_scratch_attach")
        torch.cuda.synchronize()
        # the attach zeroes the counters and nothing else: the zero words in front are the counter region, the group rows stay poisoned
        nonzero = torch.nonzero(self.buf != 0)
        self.counters = int(nonzero[0]) if nonzero.numel() else self.buf.numel()
        assert 2 <= self.counters < self.buf.numel() and GD.sentinel_only(self.buf[self.counters:])

    def check(self, what):
        assert bool((self.buf[:self.counters] == 0).all()), "%s left a ticket counter dirty" % what
        assert GD.bands_intact(self.whole, self.buf), "%s wrote a band of the ticket buffer" % what

    def release(self):
        from fusiontransformer_amd._lib import check
        check(self.lib.ftx_stream_scratch_release(self.raw), "ftx_stream_scratch_release")


@pytest.fixture(scope="module")
def L():
    from fusiontransformer_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


@pytest.fixture(scope="module")
def tickets(L):
    t = Tickets(L)
    try:
        yield t
    finally:
        torch.cuda.synchronize()
        t.release()


class Banded:
    """One guarded call: hands out device addresses of banded tensors and keeps the tensors for the checks."""

    def __init__(self, lib, tickets=None, band=None):
        from fusiontransformer_amd import _lib
        self.lib, self.tickets, self.band = lib, tickets, band
        self.stream = tickets.raw if tickets is not None else _lib.stream()
        self.outs, self.spaces, self.keep = {}, {}, []

    def _band(self, shape):
        return self.band(shape) if self.band is not None else None

    def op(self, data):
        """A float operand between NaN bands."""
        whole, view = GD.banded(data.shape, data, dtype=data.dtype, band=self._band(data.shape))
        self.keep.append(whole)
        return GD.address(whole, view)

    def out(self, name, shape, dtype=F32, rows=None):
        """An output.  rows None: every element must be written; a list of row numbers: those rows written, every other row still
        the sentinel ([] = the whole tensor untouched)."""
        whole, view = GD.banded(shape, dtype=dtype, band=self._band(shape))
        self.outs[name] = (whole, view, rows)
        return GD.address(whole, view)

    def inout(self, name, data):
        whole, view = GD.banded(data.shape, data, dtype=data.dtype, band=self._band(data.shape), inout=True)
        self.outs[name] = (whole, view, None)
        return GD.address(whole, view)

    def ws(self, name, nbytes, untouched=False):
        whole, payload = GD.banded_bytes(nbytes)
        self.spaces[name] = (whole, payload, untouched)
        return GD.address(whole, payload)

    def call(self, name, *args):
        from fusiontransformer_amd._lib import check
        torch.cuda.synchronize()                       # the operands were filled on torch's stream
        rc = getattr(self.lib, name)(*args, self.stream)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                      # a fault on the device: nothing more may run on it in this session
            pytest.exit("%s faulted on the GPU: %s" % (name, e), returncode=3)
        if rc == -2:                                   # FTX_ELAUNCH
            pytest.exit("%s: %s" % (name, self.lib.ftx_last_error().decode("utf-8", "replace")), returncode=3)
        check(rc, name)
        if self.tickets is not None:
            self.tickets.check(name)

    def view(self, name):
        return self.outs[name][1]

    def check(self, what):
        for name, (whole, view, rows) in self.outs.items():
            assert GD.bands_intact(whole, view), "%s: a guard band of %s was written" % (what, name)
            if rows is None:
                assert GD.written(view), "%s: %s has an element that was not written, or something outside an operand was read" % (what, name)
            else:
                named = torch.zeros(view.shape[0], dtype=torch.bool, device=view.device)
                if len(rows):
                    named[torch.as_tensor(rows, device=view.device).long()] = True
                    assert GD.written(view[named]), "%s: a named row of %s was not written, or something outside an operand was read" % (what, name)
                if not bool(named.all()):
                    assert GD.sentinel_only(view[~named]), "%s: %s was written outside the rows it may touch" % (what, name)
        for name, (whole, payload, untouched) in self.spaces.items():
            assert GD.bands_intact(whole, payload), "%s: workspace %s was used beyond the size its query returns" % (what, name)
            assert not untouched or GD.sentinel_only(payload), "%s: workspace %s must stay untouched" % (what, name)


class Plain(Banded):
    """The same call on plain contiguous tensors (outputs pre-filled with the sentinel, so partly written ones compare too)."""

    def _address(self, t):
        if t.numel() == 0:                             # an empty tensor: still a valid address, as in the guarded run
            t = torch.zeros(64, device="cuda")
            self.keep.append(t)
        return t.data_ptr()

    def op(self, data):
        t = data.cuda().contiguous()
        self.keep.append(t)
        return self._address(t)

    def out(self, name, shape, dtype=F32, rows=None):
        whole, view = GD.banded(shape, dtype=dtype, band=0)
        self.outs[name] = (whole, view, rows)
        return self._address(whole)

    def inout(self, name, data):
        t = data.cuda().clone().contiguous()
        self.outs[name] = (t, t, None)
        return t.data_ptr()

    def ws(self, name, nbytes, untouched=False):
        t = torch.zeros((max(int(nbytes), 256),), dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t.data_ptr()

    def check(self, what):
        pass


def run(lib, case, what, bitwise=True, tickets=None, band=None):
    """case(g) builds its tensors from g and calls the entry through g.call.  Returns the guarded run."""
    g = Banded(lib, tickets, band)
    case(g)
    g.check(what)
    if bitwise:
        p = Plain(lib, tickets)
        case(p)
        for name, (_, view, _) in g.outs.items():
            assert GD.same_bits(view, p.outs[name][1]), "%s: %s differs from the call on plain tensors" % (what, name)
    return g


def dev(t, dtype=I32):
    return t.to(dtype).cuda().contiguous()


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else 0


# ------------------------------------------------------------------------------------------------------------------ sparse convolution
PREC = {
    "fp32": dict(gemm="ftx_spconv_pairs_gemm", scatter="ftx_spconv_pairs_gemm_scatter", rows="ftx_rows_gemm", wgrad="ftx_spconv_pairs_wgrad",
                 wgrad_ws="ftx_spconv_pairs_wgrad_workspace_bytes", cols="ftx_spconv_gemm_block_cols", tile_len=S.wgrad_tile_len),
    "bf16": dict(gemm="ftx_spconv_pairs_gemm_bf16", scatter="ftx_spconv_pairs_gemm_scatter_bf16", rows="ftx_rows_gemm_bf16",
                 wgrad="ftx_spconv_pairs_wgrad_bf16", wgrad_ws="ftx_spconv_pairs_wgrad_bf16_workspace_bytes", cols="ftx_spconv_gemm_bf16_block_cols",
                 tile_len=wgrad_bf16_tile_len),
}
PRECS = sorted(PREC)
_LISTS = {}


def random_list(n_pairs, kvol, n_src=5000):
    """A pair list of random offset sizes (one empty, a dominant centre), shared by the cases that use the same one."""
    key = ("random", n_pairs, kvol, n_src)
    if key not in _LISTS:
        g = gen(n_pairs + kvol)
        sizes = random_sizes(g, n_pairs, kvol)
        n_dst = max(sizes) + 17
        _LISTS[key] = (sizes, n_src, n_dst) + pair_list(g, sizes, n_src, n_dst)
    return _LISTS[key]


def edge_list(lib, prec, ca, cg, kvol):
    """The tile-edge pair list of tests/spconv_regimes.py for this precision's weight-gradient tile length."""
    key = ("edge", prec, ca, cg, kvol)
    if key not in _LISTS:
        sizes, length = S.edge_sizes(lib, ca, cg, kvol, PREC[prec]["tile_len"])
        g = gen(kvol * 100 + ca)
        n_src, n_dst = 3001, max(sizes) + 11
        _LISTS[key] = (sizes, n_src, n_dst) + pair_list(g, sizes, n_src, n_dst) + (length,)
    return _LISTS[key]


def wgrad_tiles(lib, prec, n_pairs, ca, cg, kvol):
    return int(getattr(lib, PREC[prec]["wgrad_ws"])(n_pairs, ca, cg, kvol)) // (4 * ca * cg)


def gemm_case(lib, prec, what, A, W, w_t, d, n_pairs, co, kvol):
    n_src, ca = A.shape

    def case(g):
        a, w, tmp = g.op(A), g.op(W), g.out("tmp", (n_pairs, co))
        g.call(PREC[prec]["gemm"], a, n_src, ptr(d["src"]), w, w_t, ptr(d["koff"]), n_pairs, ca, co, kvol, tmp)
    return run(lib, case, what)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("w_t", [0, 1])
@pytest.mark.parametrize("ca,co,n_pairs,cols", GEMM_CASES)
def test_pairs_gemm_every_column_block(L, ca, co, n_pairs, cols, w_t, prec):
    sizes, n_src, n_dst, src, dst, koff, d = random_list(n_pairs, 27)
    assert getattr(L, PREC[prec]["cols"])(co, n_pairs, 27) == cols
    g = gen(ca * 7 + co * 13 + w_t)
    A, W = randn(g, n_src, ca), randn(g, 27, co, ca) if w_t else randn(g, 27, ca, co)
    gemm_case(L, prec, "%s %d->%d wT=%d" % (PREC[prec]["gemm"], ca, co, w_t), A, W, w_t, d, n_pairs, co, 27)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kvol", [27, 8, 5])
@pytest.mark.parametrize("ca,cg", [(36, 20), (100, 132)])
def test_pairs_gemm_tile_edges(L, ca, cg, kvol, prec):
    """Empty first / middle / last offsets, offsets of 1, 31-33, 127-129 pairs and around the weight-gradient tile length."""
    sizes, n_src, n_dst, src, dst, koff, d, length = edge_list(L, prec, ca, cg, kvol)
    n_pairs = sum(sizes)
    g = gen(kvol + ca)
    A, W = randn(g, n_src, ca), randn(g, kvol, ca, cg)
    gemm_case(L, prec, "%s edges kvol=%d %d->%d" % (PREC[prec]["gemm"], kvol, ca, cg), A, W, 0, d, n_pairs, cg, kvol)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("w_t", [0, 1])
@pytest.mark.parametrize("co", [20, 96, 132])
def test_pairs_gemm_scatter_leaves_unnamed_rows_alone(L, co, w_t, prec):
    ca, kvol, n_pairs = 36, 8, 3000
    sizes, n_src, n_dst, src, dst, koff, d = random_list(n_pairs, kvol, n_src=700)
    rows_out = n_pairs + 301
    g = gen(co + w_t)
    scatter = torch.randperm(rows_out, generator=g)[:n_pairs]
    if not bool((scatter == rows_out - 1).any()):
        scatter[n_pairs // 3] = rows_out - 1                      # the last row is named; the list stays injective
    if not bool((scatter == 0).any()):
        scatter[2 * n_pairs // 3] = 0
    assert torch.unique(scatter).numel() == n_pairs and int(scatter.max()) == rows_out - 1 and int(scatter.min()) == 0
    sc_d = dev(scatter)
    A, W = randn(g, n_src, ca), randn(g, kvol, co, ca) if w_t else randn(g, kvol, ca, co)

    def case(g_):
        a, w, out = g_.op(A), g_.op(W), g_.out("out", (rows_out, co), rows=scatter)
        g_.call(PREC[prec]["scatter"], a, n_src, ptr(d["src"]), ptr(sc_d), w, w_t, ptr(d["koff"]), n_pairs, ca, co, kvol, out, rows_out)
    run(L, case, "%s ->%d wT=%d" % (PREC[prec]["scatter"], co, w_t))


def block_edge_rows(blocks, n_list):
    """Row counts around the block count `blocks(n)` of a statistics launch: one row, the largest count with 1 block, the largest with
    nb - 1 blocks and the smallest with nb + 1, nb the block count at the pair list's own row count (kept below the grid's cap)."""
    def smallest_with(t):
        lo, hi = 1, 1 << 24
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if blocks(mid) >= t else (mid + 1, hi)
        return lo
    cap = blocks(1 << 24)
    nb = max(3, min(blocks(n_list), cap - 1))
    rows = [1, smallest_with(2) - 1, smallest_with(nb) - 1, smallest_with(nb + 1)]
    assert [blocks(r) for r in rows] == [1, 1, nb - 1, nb + 1], (rows, nb)
    return sorted(set(rows))


def pos_for(pos, n):
    """The position table (kvol, n_dst) cut or padded with absent entries to n rows."""
    kvol, n_dst = pos.shape
    if n <= n_dst:
        return pos[:, :n].contiguous()
    return torch.cat([pos, torch.full((kvol, n - n_dst), -1, dtype=pos.dtype, device=pos.device)], 1).contiguous()


REDUCE_LISTS = [(27, 36, 20), (27, 100, 132), (8, 36, 20), (8, 100, 132)]


@pytest.mark.parametrize("kvol,ca,co", REDUCE_LISTS + [(5, 36, 20), (5, 100, 132)])
def test_reduce(L, kvol, ca, co):
    sizes, n_src, n_dst, src, dst, koff, d, _ = edge_list(L, "fp32", ca, co, kvol)
    n_pairs = sum(sizes)
    tmp = randn(gen(kvol + co), n_pairs, co)
    for n in block_edge_rows(lambda r: int(L.ftx_spconv_reduce_stats_blocks(r, co)), n_dst):
        pos = pos_for(d["pos"], n)

        def case(g):
            t, out = g.op(tmp), g.out("out", (n, co))
            g.call("ftx_spconv_reduce", t, ptr(pos), n, co, kvol, out)
        run(L, case, "ftx_spconv_reduce kvol=%d co=%d n=%d" % (kvol, co, n))


@pytest.mark.parametrize("kvol,ca,co", REDUCE_LISTS)
def test_reduce_stats_and_its_tickets(L, tickets, kvol, ca, co):
    sizes, n_src, n_dst, src, dst, koff, d, _ = edge_list(L, "fp32", ca, co, kvol)
    n_pairs = sum(sizes)
    tmp = randn(gen(kvol + co + 1), n_pairs, co)
    blocks = lambda r: int(L.ftx_spconv_reduce_stats_blocks(r, co))     # noqa: E731
    for n in block_edge_rows(blocks, n_dst):
        pos, nb = pos_for(d["pos"], n), blocks(n)

        def case(g):
            t, out, part = g.op(tmp), g.out("out", (n, co)), g.out("part", (nb + 1, 2, co), F64)
            g.call("ftx_spconv_reduce_stats", t, ptr(pos), n, co, kvol, out, part, nb)
        run(L, case, "ftx_spconv_reduce_stats kvol=%d co=%d n=%d nb=%d" % (kvol, co, n, nb), tickets=tickets)


@pytest.mark.parametrize("kvol,ca,co", REDUCE_LISTS)
def test_reduce_bn_eval(L, kvol, ca, co):
    sizes, n_src, n_dst, src, dst, koff, d, _ = edge_list(L, "fp32", ca, co, kvol)
    n_pairs = sum(sizes)
    g0 = gen(kvol + co + 2)
    tmp, gamma, beta, rm, rv = randn(g0, n_pairs, co), randn(g0, co), randn(g0, co), randn(g0, co), torch.rand(co, generator=g0) + 0.5
    for i, n in enumerate(block_edge_rows(lambda r: int(L.ftx_spconv_reduce_stats_blocks(r, co)), n_dst)):
        pos, res, relu = pos_for(d["pos"], n), (randn(g0, n, co) if i % 2 == 0 else None), int(i % 3 != 1)

        def case(g):
            t, out = g.op(tmp), g.out("out", (n, co))
            r = g.op(res) if res is not None else 0
            g.call("ftx_spconv_reduce_bn_eval", t, ptr(pos), n, co, kvol, r, g.op(gamma), g.op(beta), g.op(rm), g.op(rv), 1e-5, relu, out)
        run(L, case, "ftx_spconv_reduce_bn_eval kvol=%d co=%d n=%d" % (kvol, co, n))


# include/ftx.h: ca in {4, 32, 64}, co in {32, 64}; which of these (in which layout of W) the kernel takes is the library's to say
OSTAT_CANDIDATES = [(ca, co, wt) for ca in (4, 32, 64) for co in (32, 64) for wt in (0, 1)]


def test_ostat_takes_nine_of_the_candidate_layers(L):
    assert sum(bool(L.ftx_spconv_ostat_supported(ca, co, 27, wt)) for ca, co, wt in OSTAT_CANDIDATES) == 9
    assert not any(L.ftx_spconv_ostat_supported(ca, co, 27, 0) for ca, co in [(8, 32), (32, 16), (128, 64), (64, 128), (96, 96)])


@pytest.mark.parametrize("ca,co,w_t", OSTAT_CANDIDATES)
def test_ostat(L, tickets, ca, co, w_t):
    kvol, rows_a = 27, 500
    if not L.ftx_spconv_ostat_supported(ca, co, kvol, w_t):         # not a layer of this kernel: the entry must say so and launch nothing
        t = torch.zeros(64, device="cuda")
        assert L.ftx_spconv_ostat(ptr(t), 1, ptr(t), 1, ptr(t), w_t, 0, ca, co, kvol, ptr(t), 0, 0, 0) == -1
        assert b"unsupported layer" in L.ftx_last_error()
        return
    blocks = lambda r: int(L.ftx_spconv_ostat_blocks(r))     # noqa: E731
    one = next(r for r in range(1, 1 << 16) if blocks(r + 1) == 2)            # rows of one block
    g0 = gen(ca + co + w_t)
    A, W = randn(g0, rows_a, ca), randn(g0, kvol, co, ca) if w_t else randn(g0, kvol, ca, co)
    for n_out in (1, one - 1, one, one + 1, 33 * one + 1):
        nbr = torch.randint(0, rows_a, (kvol, n_out), generator=g0)
        nbr[torch.rand((kvol, n_out), generator=g0) < 0.4] = -1
        nbr[kvol // 2, n_out // 2] = rows_a - 1                               # the last row of A
        nbr_d, nb = dev(nbr), blocks(n_out)
        assert nb == {1: 1, one - 1: 1, one: 1, one + 1: 2}.get(n_out, 34)
        for flip in (0, 1):
            for with_part in (0, 1):
                def case(g):
                    a, w, out = g.op(A), g.op(W), g.out("out", (n_out, co))
                    part = g.out("part", (nb + 1, 2, co), F64) if with_part else 0
                    g.call("ftx_spconv_ostat", a, rows_a, ptr(nbr_d), n_out, w, w_t, flip, ca, co, kvol, out, part, nb if with_part else 0)
                run(L, case, "ftx_spconv_ostat %d->%d wT=%d n_out=%d flip=%d part=%d" % (ca, co, w_t, n_out, flip, with_part), tickets=tickets)


def wgrad_case(lib, prec, what, A, G, src_d, dst_d, koff_d, n_pairs, kvol):
    (n_src, ca), (n_dst, cg) = A.shape, G.shape
    ws_bytes = int(getattr(lib, PREC[prec]["wgrad_ws"])(n_pairs, ca, cg, kvol))

    def case(g):
        a, gg, dW, ws = g.op(A), g.op(G), g.out("dW", (kvol, ca, cg)), g.ws("ws", ws_bytes)
        g.call(PREC[prec]["wgrad"], a, n_src, ptr(src_d), gg, n_dst, ptr(dst_d), ptr(koff_d), n_pairs, ca, cg, kvol, dW, ws, ws_bytes)
    return run(lib, case, what)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ca,cg,sides", WGRAD_CASES)
def test_wgrad_every_instantiation(L, ca, cg, sides, prec):
    kvol = 27
    assert S.wgrad_config(ca, cg) == (sides if sides != (3, 1, 3, 1) else (2, 2, 3, 1))
    # the smallest of two pair counts that gives the ordered reduce its 16 lanes: 40 000 pairs with a dominant centre offset, or, for
    # the 128 x 128 tiles (four tiles per offset matrix, so a quarter of the slots), 450 000 pairs spread evenly
    n_pairs = next(p for p in (40000, 450000) if S.wgrad_reduce_lanes(wgrad_tiles(L, prec, p, ca, cg, kvol), kvol) == 16)
    if prec == "fp32":
        assert S.wgrad_regime(L, n_pairs, ca, cg, kvol)[2] == 16             # and the restated tile length agrees with the query
    else:
        wgrad_bf16_tile_len(L, n_pairs, ca, cg, kvol)
    if n_pairs == 40000:
        sizes, n_src, n_dst, src, dst, koff, d = random_list(n_pairs, kvol)
    else:
        key = ("even", n_pairs, kvol)
        if key not in _LISTS:
            sizes = [0] + [n_pairs // 26] * 25 + [n_pairs - 25 * (n_pairs // 26)]
            _LISTS[key] = (sizes, 5000, max(sizes) + 17) + pair_list(gen(n_pairs), sizes, 5000, max(sizes) + 17)
        sizes, n_src, n_dst, src, dst, koff, d = _LISTS[key]
    g = gen(ca * 31 + cg)
    wgrad_case(L, prec, "%s %dx%d" % (PREC[prec]["wgrad"], ca, cg), randn(g, n_src, ca), randn(g, n_dst, cg), d["src"], d["dst"], d["koff"], n_pairs, kvol)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ca,cg", [(36, 20), (100, 132)])
def test_wgrad_tile_edges(L, ca, cg, prec):
    """One-tile offsets written straight to dW[k], two-tile offsets that are reduced, empty offsets that must be exact zeros."""
    kvol = 27
    sizes, n_src, n_dst, src, dst, koff, d, length = edge_list(L, prec, ca, cg, kvol)
    n_pairs = sum(sizes)
    assert length in sizes and length + 1 in sizes and length - 1 in sizes and 0 in sizes
    assert S.wgrad_reduce_lanes(wgrad_tiles(L, prec, n_pairs, ca, cg, kvol), kvol) == 16
    g = gen(ca + cg)
    run_ = wgrad_case(L, prec, "%s edges %dx%d" % (PREC[prec]["wgrad"], ca, cg), randn(g, n_src, ca), randn(g, n_dst, cg), d["src"], d["dst"], d["koff"],
                      n_pairs, kvol)
    dW = run_.view("dW")
    empty = [k for k, c in enumerate(sizes) if c == 0]
    assert len(empty) >= 3 and bool((dW[empty] == 0).all())
    assert all(bool((dW[k] != 0).any()) for k, c in enumerate(sizes) if c > 0)


@pytest.mark.parametrize("prec", PRECS)
def test_wgrad_dense_rows_with_one_reduce_lane(L, prec):
    n, ca, cg = 700, 32, 64
    assert S.wgrad_reduce_lanes(wgrad_tiles(L, prec, n, ca, cg, 1), 1) == 1
    g = gen(700)
    wgrad_case(L, prec, "%s dense 700 rows" % PREC[prec]["wgrad"], randn(g, n, ca), randn(g, n, cg), None, None, None, n, 1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("ca,co", [(32, 256), (96, 20)])
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_rows_gemm(L, n, ca, co, bias, prec):
    g0 = gen(n + ca + co)
    A, b = randn(g0, n, ca), randn(g0, co)
    for w_t in (0, 1):
        W = randn(g0, 1, co, ca) if w_t else randn(g0, 1, ca, co)

        def case(g):
            a, w, out = g.op(A), g.op(W), g.out("out", (n, co))
            g.call(PREC[prec]["rows"], a, n, w, w_t, g.op(b) if bias else 0, ca, co, out)
        run(L, case, "%s n=%d %d->%d wT=%d bias=%d" % (PREC[prec]["rows"], n, ca, co, w_t, bias))


# ------------------------------------------------------------------------------------------------------------------ norms
BN_ROWS = [1, 47, 48, 49, 48 * 32, 48 * 32 + 1, 48 * 33 + 1]     # the rows-per-block and LB_GROUP edges of the statistics grid


def test_bn_rows_are_the_block_edges(L):
    """ftx_bn_workspace_bytes = (blocks + 1) rows of (2, c) float64: the block counts BN_ROWS reach."""
    blocks = [int(L.ftx_bn_workspace_bytes(n, 4)) // 64 - 1 for n in BN_ROWS]
    assert blocks == [1, 1, 1, 2, 32, 33, 34]


@pytest.mark.parametrize("c", [4, 96, 512])
@pytest.mark.parametrize("n", BN_ROWS)
def test_batch_norm(L, tickets, n, c):
    g0 = gen(n * 7 + c)
    x, gy = randn(g0, n, c) * 1.5 + 0.3, randn(g0, n, c)
    gamma, beta = torch.rand(c, generator=g0) + 0.5, randn(g0, c)
    rm0, rv0 = randn(g0, c), torch.rand(c, generator=g0) + 0.5
    totals = torch.stack([x.double().sum(0), (x.double() ** 2).sum(0)])
    ws_bytes = int(L.ftx_bn_workspace_bytes(n, c))
    mom, eps = 0.1, 1e-5
    for with_res in (0, 1):
        res = randn(g0, n, c) if with_res else None
        for relu in (0, 1):
            tag = "n=%d c=%d residual=%d relu=%d" % (n, c, with_res, relu)

            def fwd(g):
                args = (g.op(x), g.op(res) if with_res else 0, g.op(gamma), g.op(beta), g.inout("running_mean", rm0), g.inout("running_var", rv0),
                        mom, eps, n, c, relu, g.out("y", (n, c)), g.out("save_mean", (c,)), g.out("save_invstd", (c,)))
                g.call("ftx_bn_train_fwd", *args, g.ws("ws", ws_bytes), ws_bytes)
            f = run(L, fwd, "ftx_bn_train_fwd " + tag, tickets=tickets)
            y, mean, invstd = f.view("y").cpu(), f.view("save_mean").cpu(), f.view("save_invstd").cpu()

            def fwd_totals(g):
                args = (g.op(x), g.op(res) if with_res else 0, g.op(gamma), g.op(beta), g.inout("running_mean", rm0), g.inout("running_var", rv0),
                        mom, eps, n, c, relu, g.out("y", (n, c)), g.out("save_mean", (c,)), g.out("save_invstd", (c,)))
                g.call("ftx_bn_train_fwd_totals", *args, g.op(totals))
            run(L, fwd_totals, "ftx_bn_train_fwd_totals " + tag)

            def ev(g):
                g.call("ftx_bn_eval_fwd", g.op(x), g.op(res) if with_res else 0, g.op(gamma), g.op(beta), g.op(rm0), g.op(rv0), eps, n, c, relu,
                       g.out("y", (n, c)))
            run(L, ev, "ftx_bn_eval_fwd " + tag)

            # backward: with a residual the mask comes from y; without one it is recomputed from x (y = NULL, beta given) or, when
            # beta is withheld, read from y
            modes = ["y"] if with_res or not relu else ["recompute", "y"]
            for mode in modes:
                give_y = relu and mode == "y"
                give_beta = not (relu and mode == "y" and not with_res)

                def bwd(g):
                    g.call("ftx_bn_train_bwd", g.op(gy), g.op(x), g.op(y) if give_y else 0, g.op(gamma), g.op(beta) if give_beta else 0, g.op(mean),
                           g.op(invstd), n, c, relu, g.out("grad_x", (n, c)), g.out("grad_residual", (n, c)) if with_res else 0,
                           g.out("grad_gamma", (c,)), g.out("grad_beta", (c,)), g.ws("ws", ws_bytes), ws_bytes)
                run(L, bwd, "ftx_bn_train_bwd %s mask=%s" % (tag, mode), tickets=tickets)


@pytest.mark.parametrize("rows,cols", [(1, 4), (300, 260), (2312, 768)])
def test_colsum(L, rows, cols):
    x = randn(gen(rows + cols), rows, cols)
    ws_bytes = int(L.ftx_colsum_workspace_bytes(rows, cols))

    def case(g):
        g.call("ftx_colsum", g.op(x), rows, cols, g.out("out", (cols,)), g.ws("ws", ws_bytes), ws_bytes)
    run(L, case, "ftx_colsum %dx%d" % (rows, cols))


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("c", [256, 512, 768, 1024])
def test_add_layernorm(L, rows, c):
    g0 = gen(rows + c)
    x, y, yb, gamma, beta = randn(g0, rows, c), randn(g0, rows, c), randn(g0, c), torch.rand(c, generator=g0) + 0.5, randn(g0, c)
    gh, gs = randn(g0, rows, c), randn(g0, rows, c)
    ws_bytes = int(L.ftx_layernorm_bwd_workspace_bytes(rows, c))
    for with_y, with_bias in ((0, 0), (1, 0), (1, 1)):
        tag = "rows=%d c=%d y=%d y_bias=%d" % (rows, c, with_y, with_bias)

        def fwd(g):
            s_out = g.out("s", (rows, c), rows=None if with_y else [])           # y NULL: s_out is not written
            g.call("ftx_add_layernorm_fwd", g.op(x), g.op(y) if with_y else 0, g.op(yb) if with_bias else 0, g.op(gamma), g.op(beta), 1e-6, rows, c,
                   s_out, g.out("h", (rows, c)), g.out("mean", (rows,)), g.out("rstd", (rows,)))
        f = run(L, fwd, "ftx_add_layernorm_fwd " + tag)
        s = f.view("s").cpu() if with_y else x
        mean, rstd = f.view("mean").cpu(), f.view("rstd").cpu()
        for with_gs in (0, 1):
            def bwd(g):
                g.call("ftx_add_layernorm_bwd", g.op(gh), g.op(gs) if with_gs else 0, g.op(s), g.op(gamma), g.op(mean), g.op(rstd), rows, c, with_bias,
                       g.out("grad_x", (rows, c)), g.out("grad_params", (3 if with_bias else 2, c)), g.ws("ws", ws_bytes), ws_bytes)
            run(L, bwd, "ftx_add_layernorm_bwd %s grad_s=%d" % (tag, with_gs))


def test_ticket_buffer_is_the_tests_own_and_clean(L, tickets):
    """The side stream's buffer: counters zero, group rows partly written by now or still poisoned, bands intact; the default stream's
    buffer (functional._stream_scratch) is another allocation."""
    from fusiontransformer_amd import functional as spf
    tickets.check("the statistics entries so far")
    own = GD.address(tickets.whole, tickets.buf)
    for buf in spf._TICKETS.values():
        assert not (buf.data_ptr() <= own < buf.data_ptr() + buf.numel())


# ------------------------------------------------------------------------------------------------------------------ dense GEMM
DENSE = {"bf16": dict(gemm="ftx_dense_gemm_bf16", wgrad="ftx_dense_wgrad_bf16", ws="ftx_dense_wgrad_bf16_workspace_bytes", tile="ftx_dense_bf16_tile"),
         "split": dict(gemm="ftx_dense_gemm_split", wgrad="ftx_dense_wgrad_split", ws="ftx_dense_wgrad_split_workspace_bytes", tile="ftx_dense_split_tile")}
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU = 0, 1, 2, 3


def dense_tile(lib, fam, form, m, n, k):
    tm, tn, sp = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert getattr(lib, DENSE[fam]["tile"])(form, m, n, k, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
    return tm.value, tn.value, sp.value


# (m, n, tile): m = a multiple of the tile height + 1; n = 68, 1028, 2052: multiples of 4 that are no multiple of the tile width
DENSE_GEMM = [(65, 68, (64, 64)), (65, 64, (64, 64)), (1985, 1024, (64, 128)), (1985, 1028, (64, 128)), (1921, 2048, (128, 128)),
              (1921, 2052, (128, 128))]


@pytest.mark.parametrize("fam", sorted(DENSE))
@pytest.mark.parametrize("w_kn", [0, 1])
@pytest.mark.parametrize("m,n,tile", DENSE_GEMM)
def test_dense_gemm(L, m, n, tile, w_kn, fam):
    k = 64                                                                     # the reduction length changes no store
    assert dense_tile(L, fam, 0, m, n, k) == tile + (1,) and m % tile[0] == 1
    g0 = gen(m + n + w_kn)
    A, W, bias, pre = randn(g0, m, k), (randn(g0, k, n) if w_kn else randn(g0, n, k)) * 0.125, randn(g0, n), randn(g0, m, n)
    for epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU):
        def case(g):
            a, w, b, p = g.op(A), g.op(W), g.op(bias), g.op(pre)
            out = g.out("out", (m, n))
            pre_out = g.out("pre_out", (m, n), rows=None if epi == EPI_BIAS_GELU else [])
            if not isinstance(g, Plain):                              # 16-byte aligned and no more: the weakest the header permits
                assert all(v % 32 == 16 for v in (a, w, b, p, out, pre_out))
            g.call(DENSE[fam]["gemm"], a, w, w_kn, b, p, m, n, k, epi, out, pre_out)
        run(L, case, "%s m=%d n=%d w_kn=%d epilogue=%d" % (DENSE[fam]["gemm"], m, n, w_kn, epi), band=GD.dense_band)


@pytest.mark.parametrize("fam", sorted(DENSE))
@pytest.mark.parametrize("k", [64, 68])
@pytest.mark.parametrize("m,splits", [(300, 1), (513, 2), (769, 3), (2241, 8)])
def test_dense_wgrad(L, m, splits, k, fam):
    n = 68
    assert dense_tile(L, fam, 1, m, n, k)[2] == splits
    ws_bytes = int(getattr(L, DENSE[fam]["ws"])(m, n, k))
    assert ws_bytes == (max(256, 4 * splits * n * k) if splits > 1 else 256)
    g0 = gen(m + k)
    dY, X = randn(g0, m, n), randn(g0, m, k)

    def case(g):
        g.call(DENSE[fam]["wgrad"], g.op(dY), g.op(X), m, n, k, g.out("dW", (n, k)), g.ws("ws", ws_bytes, untouched=splits == 1), ws_bytes)
    run(L, case, "%s m=%d k=%d splits=%d" % (DENSE[fam]["wgrad"], m, k, splits), band=GD.dense_band)


# ------------------------------------------------------------------------------------------------------------------ point <-> voxel, lift
PV_SIZES = [(1, 0), (255, 100), (257, 130)]      # (points, voxels): m < n


def voxel_indices(g0, n, m):
    """idx (n): voxel of each point, some voxels empty (every 7th), some points dropped (-1 and m: below and past the range)."""
    if m == 0:
        return torch.full((n,), -1, dtype=I64), torch.zeros((0,), dtype=I64)
    idx = torch.randint(0, m, (n,), generator=g0)
    idx[idx % 7 == 3] = (idx[idx % 7 == 3] + 1) % m
    idx[idx % 7 == 3] = -1
    idx[::11] = -1
    idx[5::13] = m
    idx[n // 2] = m - 1 if (m - 1) % 7 != 3 else m - 2
    valid = (idx >= 0) & (idx < m)
    return idx, torch.bincount(idx[valid], minlength=m)


def host_segments(keys, m):
    """What ftx_segment_build returns: entries sorted by key, stable, out-of-range keys at the end; first position of every key."""
    valid = (keys >= 0) & (keys < m)
    order = torch.argsort(torch.where(valid, keys, torch.full_like(keys, m)), stable=True)
    counts = torch.bincount(keys[valid], minlength=m)
    return order, torch.cat([torch.zeros(1, dtype=I64), torch.cumsum(counts, 0)])


def segment_build_case(L, keys, m, what):
    n = keys.numel()
    keys_d, ws_bytes = dev(keys), int(L.ftx_segment_workspace_bytes(n, m))

    def case(g):
        g.call("ftx_segment_build", ptr(keys_d), n, m, g.out("order", (n,), I32), g.out("seg_off", (m + 1,), I32), g.ws("ws", ws_bytes), ws_bytes)
    r = run(L, case, what)
    order, seg_off = host_segments(keys, m)
    assert torch.equal(r.view("order").cpu().long(), order) and torch.equal(r.view("seg_off").cpu().long(), seg_off)
    return dev(order), dev(seg_off)


@pytest.mark.parametrize("c", [1, 4, 5, 96])
@pytest.mark.parametrize("n,m", PV_SIZES)
def test_voxelize(L, n, m, c):
    g0 = gen(n + c)
    idx, counts = voxel_indices(g0, n, m)
    idx_d, counts_d = dev(idx), dev(counts)
    feats, go = randn(g0, n, c), randn(g0, m, c)

    def fwd(g):
        g.call("ftx_voxelize_fwd", g.op(feats), ptr(idx_d), ptr(counts_d), n, c, m, g.out("out", (m, c)))
    run(L, fwd, "ftx_voxelize_fwd n=%d m=%d c=%d" % (n, m, c), bitwise=False)            # float atomics

    def bwd(g):
        g.call("ftx_voxelize_bwd", g.op(go), ptr(idx_d), ptr(counts_d), n, c, m, g.out("grad_feats", (n, c)))
    run(L, bwd, "ftx_voxelize_bwd n=%d m=%d c=%d" % (n, m, c))
    if c % 4:
        return
    order_d, seg_d = segment_build_case(L, idx, m, "ftx_segment_build (voxelize) n=%d m=%d" % (n, m))

    def fwd_sorted(g):
        g.call("ftx_voxelize_fwd_sorted", g.op(feats), ptr(order_d), ptr(seg_d), n, c, m, g.out("out", (m, c)))
    run(L, fwd_sorted, "ftx_voxelize_fwd_sorted n=%d m=%d c=%d" % (n, m, c))

    def seg_sum(g):
        g.call("ftx_segment_sum", g.op(feats), ptr(order_d), ptr(seg_d), n, c, m, g.out("out", (m, c)))
    run(L, seg_sum, "ftx_segment_sum n=%d m=%d c=%d" % (n, m, c))


@pytest.mark.parametrize("c", [4, 96])
@pytest.mark.parametrize("n,m", PV_SIZES)
def test_devoxelize(L, n, m, c):
    g0 = gen(n + c + 1)
    idx = torch.randint(0, max(m, 1), (n, 8), generator=g0)
    idx[idx % 7 == 3] = -1                                                          # empty voxels and absent corners
    if m == 0:
        idx[:] = -1
    else:
        idx[n // 2, 3] = m - 1 if (m - 1) % 7 != 3 else m - 2
    weights = torch.rand((n, 8), generator=g0)
    weights[torch.rand((n, 8), generator=g0) < 0.2] = 0.0                            # zero-weight corners are dropped from the segments
    idx_d = dev(idx)
    feats, go = randn(g0, m, c), randn(g0, n, c)

    def fwd(g):
        g.call("ftx_devoxelize_fwd", g.op(feats), ptr(idx_d), g.op(weights), n, c, m, g.out("out", (n, c)))
    run(L, fwd, "ftx_devoxelize_fwd n=%d m=%d c=%d" % (n, m, c))

    def bwd(g):
        g.call("ftx_devoxelize_bwd", g.op(go), ptr(idx_d), g.op(weights), n, c, m, g.out("grad_feats", (m, c)))
    run(L, bwd, "ftx_devoxelize_bwd n=%d m=%d c=%d" % (n, m, c), bitwise=False)          # float atomics
    keys = torch.where(weights != 0, idx, torch.full_like(idx, -1)).view(-1)
    order_d, seg_d = segment_build_case(L, keys, m, "ftx_segment_build (devoxelize) n=%d m=%d" % (8 * n, m))

    def bwd_sorted(g):
        g.call("ftx_devoxelize_bwd_sorted", g.op(go), g.op(weights), ptr(order_d), ptr(seg_d), n, c, m, g.out("grad_feats", (m, c)))
    run(L, bwd_sorted, "ftx_devoxelize_bwd_sorted n=%d m=%d c=%d" % (n, m, c))


@pytest.mark.parametrize("c", [4, 96])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_lift(L, n, c):
    b, gh, gw, H, W = 2, 3, 5, 30, 44
    g0 = gen(n + c + 2)
    img_idx = torch.stack([torch.randint(0, H, (n,), generator=g0), torch.randint(0, W, (n,), generator=g0)], 1)
    img_idx[n // 2] = torch.tensor([H - 1, W - 1])
    frame = torch.randint(0, b, (n,), generator=g0)
    frame[n // 2] = b - 1
    idx_d, frame_d = dev(img_idx, I64), dev(frame)
    grid, go = randn(g0, b, gh, gw, c), randn(g0, n, c)

    def fwd(g):
        g.call("ftx_lift_gather_fwd", g.op(grid), ptr(idx_d), ptr(frame_d), n, b, gh, gw, c, H, W, g.out("out", (n, c)))
    run(L, fwd, "ftx_lift_gather_fwd n=%d c=%d" % (n, c))

    def bwd(g):
        g.call("ftx_lift_gather_bwd", g.op(go), ptr(idx_d), ptr(frame_d), n, b, gh, gw, c, H, W, g.out("grad_grid", (b, gh, gw, c)))
    run(L, bwd, "ftx_lift_gather_bwd n=%d c=%d" % (n, c), bitwise=False)                 # float atomics
    # the keys of the atomic-free backward; frames outside [0, b) give -1 (this entry checks the frame, the gathers above do not)
    frame_k = frame.clone()
    frame_k[::9] = b
    frame_k[4::9] = -1
    frame_kd = dev(frame_k)

    def cells(g):
        g.call("ftx_lift_cells", ptr(idx_d), ptr(frame_kd), n, b, gh, gw, H, W, g.out("cells", (n,), I32))
    r = run(L, cells, "ftx_lift_cells n=%d" % n)
    keys = r.view("cells").cpu().long()
    bad = (frame_k < 0) | (frame_k >= b)
    assert bool((keys[bad] == -1).all()) and bool((keys[~bad] >= 0).all()) and int(keys.max()) < b * gh * gw
    order_d, seg_d = segment_build_case(L, keys, b * gh * gw, "ftx_segment_build (lift) n=%d" % n)

    def seg_sum(g):
        g.call("ftx_segment_sum", g.op(go), ptr(order_d), ptr(seg_d), n, c, b * gh * gw, g.out("grad_grid", (b * gh * gw, c)))
    run(L, seg_sum, "ftx_segment_sum (lift) n=%d c=%d" % (n, c))


@pytest.mark.parametrize("b,c,ih,iw,oh,ow", [(1, 1, 1, 1, 1, 1), (2, 3, 5, 7, 16, 16), (1, 5, 17, 15, 3, 4), (2, 96, 3, 5, 7, 9)])
def test_resample_nearest(L, b, c, ih, iw, oh, ow):
    g0 = gen(b + c + ih + ow)
    x, go = randn(g0, b, c, ih, iw), randn(g0, b, c, oh, ow)

    def fwd(g):
        g.call("ftx_resample_nearest_fwd", g.op(x), b, c, ih, iw, oh, ow, g.out("out", (b, c, oh, ow)))
    run(L, fwd, "ftx_resample_nearest_fwd %s" % ((b, c, ih, iw, oh, ow),))

    def bwd(g):
        g.call("ftx_resample_nearest_bwd", g.op(go), b, c, ih, iw, oh, ow, g.out("grad_in", (b, c, ih, iw)))
    run(L, bwd, "ftx_resample_nearest_bwd %s" % ((b, c, ih, iw, oh, ow),), bitwise=False)  # atomicAdd in resample_bwd_kernel


# ------------------------------------------------------------------------------------------------------------------ the gate can tell
def test_the_gate_reports_a_written_band_and_an_unwritten_element(L):
    n, ca, co = 129, 96, 20
    g0 = gen(1)
    A, W = randn(g0, n, ca), randn(g0, 1, ca, co)

    def case(g):
        g.call("ftx_rows_gemm", g.op(A), n, g.op(W), 0, 0, ca, co, g.out("out", (n, co)))
    r = run(L, case, "ftx_rows_gemm")
    whole, view, _ = r.outs["out"]
    r.check("intact")
    end = view.storage_offset() + view.numel()
    whole[end:end + 1].zero_()                                        # one word into the band behind the output, with a torch op
    assert not GD.bands_intact(whole, view)
    with pytest.raises(AssertionError, match="guard band"):
        r.check("planted")
    whole[end:end + 1].view(I32).fill_(GD.SENTINEL)
    r.check("repaired")
    view.view(I32)[n // 2, 3] = GD.SENTINEL                           # one output element back to the sentinel
    assert GD.bands_intact(whole, view) and not GD.written(view)
    with pytest.raises(AssertionError, match="not written"):
        r.check("planted")
