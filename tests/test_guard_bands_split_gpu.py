"""Guard bands (tests/guard.py, the harness of tests/test_guard_bands_gpu.py) for the entries of the three-piece split sparse
convolution (csrc/ftx_spconv_split.hip): every output element written, no band of an output or of the workspace touched, nothing read
outside an operand, the same bits as on plain tensors.

    ftx_spconv_pairs_gemm_split            tmp (n_pairs, co)
    ftx_spconv_pairs_gemm_scatter_split    rows named by scatter finite, every other row still the sentinel ("left untouched")
    ftx_rows_gemm_split                    out (n, co), with and without bias
    ftx_spconv_pairs_wgrad_split           dW; the workspace exactly as large as ftx_spconv_pairs_wgrad_split_workspace_bytes says

A 128 -> 96 layer on 6 000 pairs (a 128 x 96 weight-gradient tile at the family's full LDS budget, 96-column GEMM blocks) and dense
rows 2 500 x 96 -> 20."""
import pytest
import torch

from tests.norm_ref import gen, randn
from tests.spconv_split_ref import split_tile_len
from tests.test_guard_bands_gpu import L, dev, ptr, random_list, run  # noqa: F401

pytestmark = pytest.mark.gpu
CA, CO, PAIRS, KVOL = 128, 96, 6000, 27
ROWS, RCA, RCO = 2500, 96, 20


@pytest.mark.parametrize("w_t", [0, 1])
def test_pairs_gemm_split(L, w_t):
    sizes, n_src, n_dst, src, dst, koff, d = random_list(PAIRS, KVOL)
    assert L.ftx_spconv_gemm_split_block_cols(CO, PAIRS, KVOL) == 96
    g0 = gen(CA + CO + w_t)
    A, W = randn(g0, n_src, CA), randn(g0, KVOL, CO, CA) if w_t else randn(g0, KVOL, CA, CO)

    def case(g):
        a, w, tmp = g.op(A), g.op(W), g.out("tmp", (PAIRS, CO))
        g.call("ftx_spconv_pairs_gemm_split", a, n_src, ptr(d["src"]), w, w_t, ptr(d["koff"]), PAIRS, CA, CO, KVOL, tmp)
    run(L, case, "ftx_spconv_pairs_gemm_split %d->%d wT=%d" % (CA, CO, w_t))


@pytest.mark.parametrize("w_t", [0, 1])
def test_pairs_gemm_scatter_split_leaves_unnamed_rows_alone(L, w_t):
    sizes, n_src, n_dst, src, dst, koff, d = random_list(PAIRS, KVOL)
    rows_out = PAIRS + 301
    g0 = gen(CO + w_t + 1)
    scatter = torch.randperm(rows_out, generator=g0)[:PAIRS]
    if not bool((scatter == rows_out - 1).any()):
        scatter[PAIRS // 3] = rows_out - 1                      # the last row is named; the list stays injective
    if not bool((scatter == 0).any()):
        scatter[2 * PAIRS // 3] = 0
    assert torch.unique(scatter).numel() == PAIRS and int(scatter.max()) == rows_out - 1 and int(scatter.min()) == 0
    sc_d = dev(scatter)
    A, W = randn(g0, n_src, CA), randn(g0, KVOL, CO, CA) if w_t else randn(g0, KVOL, CA, CO)

    def case(g):
        a, w, out = g.op(A), g.op(W), g.out("out", (rows_out, CO), rows=scatter)
        g.call("ftx_spconv_pairs_gemm_scatter_split", a, n_src, ptr(d["src"]), ptr(sc_d), w, w_t, ptr(d["koff"]), PAIRS, CA, CO, KVOL, out, rows_out)
    run(L, case, "ftx_spconv_pairs_gemm_scatter_split ->%d wT=%d" % (CO, w_t))


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("w_t", [0, 1])
def test_rows_gemm_split(L, w_t, bias):
    g0 = gen(ROWS + w_t + bias)
    A, b = randn(g0, ROWS, RCA), randn(g0, RCO)
    W = randn(g0, 1, RCO, RCA) if w_t else randn(g0, 1, RCA, RCO)

    def case(g):
        a, w, out = g.op(A), g.op(W), g.out("out", (ROWS, RCO))
        g.call("ftx_rows_gemm_split", a, ROWS, w, w_t, g.op(b) if bias else 0, RCA, RCO, out)
    run(L, case, "ftx_rows_gemm_split n=%d %d->%d wT=%d bias=%d" % (ROWS, RCA, RCO, w_t, bias))


def _wgrad(L, what, A, G, src_d, dst_d, koff_d, n_pairs, kvol):
    (n_src, ca), (n_dst, cg) = A.shape, G.shape
    ws_bytes = int(L.ftx_spconv_pairs_wgrad_split_workspace_bytes(n_pairs, ca, cg, kvol))
    split_tile_len(L, n_pairs, ca, cg, kvol)       # the restated tile length agrees with the query

    def case(g):
        a, gg, dW, ws = g.op(A), g.op(G), g.out("dW", (kvol, ca, cg)), g.ws("ws", ws_bytes)
        g.call("ftx_spconv_pairs_wgrad_split", a, n_src, ptr(src_d), gg, n_dst, ptr(dst_d), ptr(koff_d), n_pairs, ca, cg, kvol, dW, ws, ws_bytes)
    return run(L, case, what)


def test_wgrad_split(L):
    sizes, n_src, n_dst, src, dst, koff, d = random_list(PAIRS, KVOL)
    g0 = gen(CA * 31 + CO)
    r = _wgrad(L, "ftx_spconv_pairs_wgrad_split %dx%d" % (CA, CO), randn(g0, n_src, CA), randn(g0, n_dst, CO), d["src"], d["dst"], d["koff"], PAIRS, KVOL)
    dW = r.view("dW")
    empty = [k for k, c in enumerate(sizes) if c == 0]
    assert empty and bool((dW[empty] == 0).all())


@pytest.mark.parametrize("ca,cg", [(RCO, RCA), (RCA, RCO)])
def test_wgrad_split_dense_rows(L, ca, cg):
    g0 = gen(ROWS + ca)
    _wgrad(L, "ftx_spconv_pairs_wgrad_split dense %d rows %dx%d" % (ROWS, ca, cg), randn(g0, ROWS, ca), randn(g0, ROWS, cg), None, None, None, ROWS, 1)
