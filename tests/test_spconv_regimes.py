"""The tile shapes of the sparse-convolution kernels, without a GPU: the Python restatement in tests/spconv_regimes.py against the
library's host queries, and the layers of the full-size GPU tests (tests/test_spconv_regimes_gpu.py) against the regimes they are
there to reach.  A retune of a threshold that moves a listed layer onto another tile shape fails here, not silently there."""
import itertools

import pytest

from tests import spconv_regimes as S


@pytest.fixture(scope="module")
def lib(ftx_lib):
    return ftx_lib


def test_block_cols_query_matches_the_restated_dispatch(lib):
    for co in (4, 20, 32, 36, 64, 96, 100, 128, 132, 192, 256, 384, 512):
        for n in (0, 1, 127, 128, 129, 40000, 51072, 51073, 51200, 51201, 382735):
            for kvol in (0, 1, 8, 27):
                assert lib.ftx_spconv_gemm_block_cols(co, n, kvol) == S.block_cols(co, n, kvol), (co, n, kvol)
    # the 128 -> 64 step at 400 row tiles, on both sides (dense rows: 400 tiles of 128 rows)
    assert lib.ftx_spconv_gemm_block_cols(128, 400 * 128, 0) == 64 and lib.ftx_spconv_gemm_block_cols(128, 400 * 128 + 1, 0) == 128
    assert lib.ftx_spconv_gemm_block_cols(128, 373 * 128, 27) == 64 and lib.ftx_spconv_gemm_block_cols(128, 373 * 128 + 1, 27) == 128
    assert lib.ftx_spconv_gemm_block_cols(6, 100, 1) == -1 and lib.ftx_spconv_gemm_block_cols(32, -1, 1) == -1


def test_wgrad_regime_restatement_matches_the_workspace_query(lib):
    for ca, cg in itertools.product((4, 20, 32, 36, 64, 96, 100, 128, 132, 192, 256, 384), repeat=2):
        for n, kvol in ((1, 1), (700, 1), (81237, 1), (5970, 27), (39949, 27), (382735, 27), (11139, 8), (81237, 8), (544, 5)):
            S.wgrad_regime(lib, n, ca, cg, kvol)     # asserts the tile count of the workspace query


def test_production_table_reaches_its_regimes(lib):
    """Each listed layer reaches the tile shapes written next to it, and together the table covers every regime the issue of the
    full-size tests named: 128-column blocks in the forward, data-gradient, dense and scatter forms, TL = 16 and TL = 4 reduces,
    tiles of 832 pairs and more, and the wgrad instantiations of the benched step."""
    fwd_cols, dgrad_cols, scatter_cols, tls, lens, insts = set(), set(), set(), set(), set(), set()
    for e in S.PRODUCTION:
        kvol = 27 if e["map"][0] == "subm" else 8
        level = e["map"][1]
        expect = S.BENCH_SUBM_PAIRS[level] if e["map"][0] == "subm" else S.BENCH_VOXELS[level]
        assert e["n_pairs"] == expect, e["name"]
        ca, co, p = e["ca"], e["co"], e["n_pairs"]
        got = (lib.ftx_spconv_gemm_block_cols(co, p, kvol), lib.ftx_spconv_gemm_block_cols(ca, p, kvol), S.wgrad_regime(lib, p, ca, co, kvol))
        assert got == (e["fwd"], e["dgrad"], e["wgrad"]), (e["name"], got)
        if e["form"] == "conv":
            fwd_cols.add(e["fwd"])
            dgrad_cols.add(e["dgrad"])
        else:
            scatter_cols.add(e["fwd"] if e["form"] == "deconv" else e["dgrad"])
        insts.add(e["wgrad"][0])
        lens.add(e["wgrad"][1])
        tls.add(e["wgrad"][2])
    dense_cols = set()
    for e in S.DENSE:
        got = (lib.ftx_spconv_gemm_block_cols(e["co"], e["rows"], 0), lib.ftx_spconv_gemm_block_cols(e["ca"], e["rows"], 0),
               S.wgrad_regime(lib, e["rows"], e["co"], e["ca"], 1))
        assert got == (e["fwd"], e["dgrad"], e["wgrad"]), (e["name"], got)
        dense_cols.add(e["fwd"])
    assert 128 in fwd_cols and 128 in dgrad_cols and 128 in scatter_cols and 128 in dense_cols
    assert {4, 16} <= tls and max(lens) >= 832 and 256 in lens
    assert {(1, 1, 1, 1), (2, 2, 3, 1), (3, 1, 2, 2), (2, 1, 2, 2), (2, 2, 2, 2)} <= insts
    # the stem's weight gradient (M tile mostly padding) at full size with TL = 16
    stem = [e for e in S.PRODUCTION if e["ca"] == 4]
    assert stem and stem[0]["wgrad"][2] == 16 and stem[0]["n_pairs"] == S.BENCH_SUBM_PAIRS[1]


def test_synthetic_cases_reach_every_instantiation_and_reduce_form(lib):
    """The synthetic weight-gradient cases: every (MI, WMG) x (NI, WNG) pair of sides; the one combination wgrad_config remaps,
    (3,1) x (3,1), lands on (2,2) x (3,1), so pairs_wgrad_kernel<3,3,1,1> is compiled but reached by no argument.  The tile-edge lists
    reach TL = 16 (kvol 27 and 8) and TL = 4 (kvol 5), one-tile offsets and empty ones; dense rows of at most three tiles reach TL = 1."""
    reached = set()
    for (ms, ca_opts), (ns, cg_opts) in itertools.product(S.WGRAD_SIDES.items(), repeat=2):
        for ca, cg in zip(ca_opts, cg_opts):
            inst = S.wgrad_config(ca, cg)
            assert inst == (ms + ns if (ms, ns) != ((3, 1), (3, 1)) else (2, 2, 3, 1)), (ca, cg)
            reached.add(inst)
    assert len(reached) == 15 and (3, 1, 3, 1) not in reached
    for kvol, tl in ((27, 16), (8, 16), (5, 4)):
        sizes, length = S.edge_sizes(lib, 36, 20, kvol)
        assert S.wgrad_regime(lib, sum(sizes), 36, 20, kvol)[1:] == (length, tl)
        assert sizes[0] == 0 and sizes[-1] == 0 and length in sizes and length + 1 in sizes
    assert S.wgrad_regime(lib, 700, 32, 64, 1)[2] == 1
