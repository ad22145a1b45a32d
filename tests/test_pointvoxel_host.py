"""CPU half of tests/test_pointvoxel_fullsize_gpu.py: the float64 references against the oracle, the index restatement on the
production batch, the float32 restatements' sensitivity to summation order, and the strength of every gate (each planted kernel
mistake must fail it)."""
import numpy as np
import pytest
import torch

from oracle import ft_oracle as O
from tests import pointvoxel_ref as R


def _skewed(rng, n, m, p=0.01):
    """Destinations with a geometric spread of segment lengths (the longest a few hundred), some -1 and some >= m."""
    idx = np.minimum(rng.geometric(p, n) - 1, m - 1).astype(np.int32)
    r = rng.random(n)
    idx[r < 0.02] = -1
    idx[(r >= 0.02) & (r < 0.03)] = m + 3
    return idx


# ------------------------------------------------------------------------------------------------ references against the oracle
def test_references_match_the_oracle():
    rng = np.random.default_rng(0)
    n, m, c = 3000, 120, 12
    idx = _skewed(rng, n, m)
    idx[idx >= m] = -1                                # the oracle knows -1 only
    counts = O.spcount(idx, m)
    f = rng.standard_normal((n, c))
    ref, Rabs, L = R.voxelize_ref(f, idx, counts)
    want = O.spvoxelize(torch.from_numpy(f), idx, counts).numpy()
    np.testing.assert_allclose(ref, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(Rabs, O.spvoxelize(torch.from_numpy(np.abs(f)), idx, counts).numpy(), rtol=1e-13, atol=1e-15)
    assert np.array_equal(L, counts)
    # the voxelize backward in float32: the oracle's autograd divides the same way
    f32 = torch.from_numpy(f.astype(np.float32)).requires_grad_(True)
    go = rng.standard_normal((m, c)).astype(np.float32)
    O.spvoxelize(f32, idx, counts).backward(torch.from_numpy(go))
    np.testing.assert_array_equal(R.voxelize_bwd_exact(go, idx, counts), f32.grad.numpy())
    # devoxelize forward and backward (float64 autograd through the oracle)
    idx8 = rng.integers(-1, m, (n, 8)).astype(np.int32)
    w8 = rng.uniform(0, 1, (n, 8))
    w8[rng.random((n, 8)) < 0.1] = 0
    fv = torch.from_numpy(rng.standard_normal((m, c))).requires_grad_(True)
    out = O.spdevoxelize(fv, idx8, w8)
    ref, Rabs, L = R.devoxelize_ref(fv.detach().numpy(), idx8, w8)
    np.testing.assert_allclose(ref, out.detach().numpy(), rtol=1e-13, atol=1e-15)
    gp = rng.standard_normal((n, c))
    out.backward(torch.from_numpy(gp))
    bref, bR, bL = R.devoxelize_bwd_ref(gp, idx8, w8, m)
    np.testing.assert_allclose(bref, fv.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert np.array_equal(bL, np.bincount(np.where(w8 != 0, idx8, -1)[(idx8 >= 0) & (w8 != 0)], minlength=m))
    # segment sum
    keys = _skewed(rng, n, m)
    ref, _, L = R.segment_sum_ref(f, keys, m)
    ok = (keys >= 0) & (keys < m)
    want = torch.zeros(m, c, dtype=torch.float64).index_add_(0, torch.from_numpy(keys[ok].astype(np.int64)), torch.from_numpy(f[ok]))
    np.testing.assert_allclose(ref, want.numpy(), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("H,W", [(370, 1226), (384, 1248), (900, 1600), (24, 24), (7, 50)])
def test_lift_cells_follow_nn_upsample(H, W):
    """The nearest rule of the references against a materialised nn.Upsample((H, W)) of a 2 x 24 x 24 grid of cell numbers."""
    g = R.LIFT_GRID
    ids = torch.arange(2 * g * g, dtype=torch.float32).view(2, 1, g, g)
    up = torch.nn.Upsample((H, W))(ids)[:, 0].long().numpy()
    fr, rr, cc = np.meshgrid(np.arange(2), np.arange(H), np.arange(W), indexing="ij")
    cells = R.lift_cells(np.stack([rr.ravel(), cc.ravel()], 1), fr.ravel(), H, W)
    assert np.array_equal(cells, up.ravel())
    down = torch.nn.Upsample((384, 384))(torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W))[0, 0].long().numpy()
    assert np.array_equal(down, O.nearest_src_index(384, H)[:, None] * W + O.nearest_src_index(384, W)[None, :])


def test_index_restatement_on_the_production_batch():
    """The restatement on make_batch([0, 1, 2, 3]): the sizes of the issue's table, every point's own voxel found as its corner 0,
    and segments that pass their own check."""
    from fusiontransformer_amd.data.synth import make_batch
    coords = make_batch([0, 1, 2, 3])["coords"].astype(np.int32)
    assert coords.shape[0] == 81237
    for s, m_want, longest in ((1, 81237, 1), (4, 20197, 32), (16, 2949, 457)):
        rows, idx, counts = R.level_index(coords, s)
        assert rows.shape[0] == m_want and counts.max() == longest and counts.sum() == coords.shape[0]
        assert np.array_equal(rows[idx], R.level_coords(coords, s))
        assert np.array_equal(R.corner_index(coords, rows, s)[:, 0], idx)
        order, off = R.segments(idx, rows.shape[0])
        assert R.check_segments(order, off, idx, rows.shape[0], f"s{s}") == longest


def test_check_segments_rejects_broken_segments():
    rng = np.random.default_rng(1)
    m = 40
    keys = _skewed(rng, 2000, m, 0.05)
    order, off = R.segments(keys, m)
    R.check_segments(order, off, keys, m, "ok")
    v = int(np.argmax(np.diff(off)))
    lo = int(off[v])
    swapped, duplicated = order.copy(), order.copy()
    duplicated[lo] = duplicated[lo + 1]
    swapped[[lo, lo + 1]] = swapped[[lo + 1, lo]]
    shifted = off.copy()
    shifted[v + 1] -= 1
    for o, s in ((swapped, off), (order, shifted), (duplicated, off)):
        with pytest.raises(AssertionError):
            R.check_segments(o, s, keys, m, "broken")


# ------------------------------------------------------------------------------------------------ summation order
def test_sequential_restatements_tell_summation_orders_apart():
    """On one constructed segment the ascending-order float32 sum differs from the reversed-order one, so the exact checks of the
    sorted kernels would catch a change of order."""
    vals = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32)
    off = np.array([0, 5], dtype=np.int32)
    up = R.segment_sum_seq(vals, np.arange(5, dtype=np.int32), off)
    down = R.segment_sum_seq(vals, np.arange(5, dtype=np.int32)[::-1].copy(), off)
    assert up[0, 0] == np.float32(1.0) and down[0, 0] == np.float32(1.0 + 2.0 ** -22)
    vals5 = vals * np.float32(5)
    up = R.segment_sum_seq(vals5, np.arange(5, dtype=np.int32), off, mean=True)
    down = R.segment_sum_seq(vals5, np.arange(5, dtype=np.int32)[::-1].copy(), off, mean=True)
    assert up[0, 0] != down[0, 0]


# ------------------------------------------------------------------------------------------------ gate strength
def _rejects(got, ref, Rabs, L):
    return R.ratio(np.asarray(got, dtype=np.float32), ref, R.bound(Rabs, L)) > 1.0


def _accepts(got, ref, Rabs, L):
    return R.ratio(np.asarray(got, dtype=np.float32), ref, R.bound(Rabs, L)) <= 1.0


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(2)
    n, m, c = 20000, 200, 32
    idx = _skewed(rng, n, m, 0.005)
    counts = np.bincount(idx[(idx >= 0) & (idx < m)], minlength=m).astype(np.int32)
    order, off = R.segments(idx, m)
    v = int(np.argmax(counts))
    e = int(order[off[v] + counts[v] // 2])          # an entry in the middle of the longest segment
    return dict(rng=rng, n=n, m=m, c=c, idx=idx, counts=counts, order=order, off=off, v=v, e=e,
                f=rng.standard_normal((n, c)).astype(np.float32))


def test_voxelize_gates_reject_planted_mistakes(planted):
    p = planted
    f, idx, counts, m, v, e = p["f"], p["idx"], p["counts"], p["m"], p["v"], p["e"]
    assert counts[v] >= 300
    ref, Rabs, L = R.voxelize_ref(f, idx, counts)
    good = R.segment_sum_seq(f, p["order"], p["off"], mean=True)
    assert _accepts(good, ref, Rabs, L)
    rev = np.concatenate([p["order"][p["off"][i]:p["off"][i + 1]][::-1] for i in range(m)])
    assert _accepts(R.segment_sum_seq(f, rev, p["off"], mean=True), ref, Rabs, L)       # any order passes the bound
    dropped, moved = idx.copy(), idx.copy()
    dropped[e] = -1
    moved[e] = v + 1
    assert _rejects(R.voxelize_ref(f, dropped, counts)[0], ref, Rabs, L)
    assert _rejects(R.voxelize_ref(f, moved, counts)[0], ref, Rabs, L)
    assert _rejects(R.voxelize_ref(f, idx, counts + 1)[0], ref, Rabs, L)
    assert not np.array_equal(R.segment_sum_seq(f, rev, p["off"], mean=True), good)     # and the exact check sees the order
    # the backward is checked exactly: division by counts + 1 changes it
    go = p["rng"].standard_normal((m, p["c"])).astype(np.float32)
    exact = R.voxelize_bwd_exact(go, idx, counts)
    assert not np.array_equal(R.voxelize_bwd_exact(go, idx, counts + 1), exact)
    # the mutants the GPU module feeds to the gate are rejected too
    muts = R.scatter_mutants(idx, m, lambda ents: f[ents].astype(np.float64) / counts[idx[ents]][:, None])
    R.gate("planted voxelize", good, ref, Rabs, L, muts)


def test_lift_gates_reject_planted_mistakes(planted):
    p = planted
    f, idx, m, v, e = p["f"], p["idx"], p["m"], p["v"], p["e"]
    ref, Rabs, L = R.segment_sum_ref(f, idx, m)
    good = R.segment_sum_seq(f, p["order"], p["off"])
    assert _accepts(good, ref, Rabs, L)
    dropped, moved = idx.copy(), idx.copy()
    dropped[e] = -1
    moved[e] = v - 1
    assert _rejects(R.segment_sum_ref(f, dropped, m)[0], ref, Rabs, L)
    assert _rejects(R.segment_sum_ref(f, moved, m)[0], ref, Rabs, L)
    R.gate("planted segment sum", good, ref, Rabs, L, R.scatter_mutants(idx, m, lambda ents: f[ents]))


def test_devoxelize_gates_reject_planted_mistakes(planted):
    p = planted
    rng, m, c = p["rng"], p["m"], p["c"]
    n = 6000
    idx8 = np.minimum(rng.geometric(0.02, (n, 8)) - 1, m - 1).astype(np.int32)
    idx8[rng.random((n, 8)) < 0.05] = -1
    w8 = rng.uniform(0, 1, (n, 8)).astype(np.float32)
    w8[rng.random((n, 8)) < 0.1] = 0
    fv = rng.standard_normal((m, c)).astype(np.float32)
    # forward: float32 fma chain over the corners against the float64 reference
    ref, Rabs, L = R.devoxelize_ref(fv, idx8, w8)
    good = R.devoxelize_ref(fv, idx8, w8)[0].astype(np.float32)
    assert _accepts(good, ref, Rabs, L)
    swapped = w8[:, [1, 0, 2, 3, 4, 5, 6, 7]]                       # a wrong corner weight
    assert _rejects(R.devoxelize_ref(fv, idx8, swapped)[0], ref, Rabs, L)
    one_corner = idx8.copy()
    one_corner[:, 3] = -1                                           # a corner dropped
    assert _rejects(R.devoxelize_ref(fv, one_corner, w8)[0], ref, Rabs, L)
    R.gate("planted devoxelize", good, ref, Rabs, L, R.gather_mutants(idx8, w8, fv, m))
    # backward: the sorted form's float32 chain, then a dropped, a moved and a mis-weighted entry
    go = rng.standard_normal((n, c)).astype(np.float32)
    bref, bR, bL = R.devoxelize_bwd_ref(go, idx8, w8, m)
    keys = np.where(w8 != 0, idx8, -1).reshape(-1)
    order, off = R.segments(keys, m)
    terms = (w8.reshape(-1)[:, None] * go[np.arange(8 * n) >> 3]).astype(np.float32)
    good = R.segment_sum_seq(terms, order, off)
    assert _accepts(good, bref, bR, bL)
    v = int(np.argmax(np.diff(off)))
    ent = int(order[off[v] + (off[v + 1] - off[v]) // 2])
    i, k = ent >> 3, ent & 7
    dropped, moved, misweighted = idx8.copy(), idx8.copy(), w8.copy()
    dropped[i, k] = -1
    moved[i, k] = v + 1 if v + 1 < m else v - 1
    misweighted[i, k] = w8[i, k] * 2 if w8[i, k] < 0.5 else w8[i, k] / 2
    for bad in (R.devoxelize_bwd_ref(go, dropped, w8, m)[0], R.devoxelize_bwd_ref(go, moved, w8, m)[0],
                R.devoxelize_bwd_ref(go, idx8, misweighted, m)[0], R.devoxelize_bwd_ref(go, idx8, w8[:, ::-1], m)[0]):
        assert _rejects(bad, bref, bR, bL)
    R.gate("planted devoxelize backward", good, bref, bR, bL,
           R.scatter_mutants(keys, m, lambda ents: w8.reshape(-1)[ents][:, None].astype(np.float64) * go[ents >> 3]))


def test_gate_rejects_non_finite_and_nonzero_where_the_bound_is_zero():
    ref = np.zeros((3, 2))
    Rabs = np.zeros((3, 2))
    L = np.ones(3)
    assert R.ratio(np.array([[0, 0], [0, 1e-30], [0, 0]], dtype=np.float32), ref, R.bound(Rabs, L)) == float("inf")
    with pytest.raises(AssertionError):
        R.gate("nan", np.full((3, 2), np.nan, dtype=np.float32), ref, Rabs, L, [[(0, np.ones(2))], [(0, np.ones(2))]])
