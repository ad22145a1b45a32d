"""Point <-> voxel feature movement and the image lift (csrc/ftx_pointvoxel.hip) at production size, against float64 and exact
float32 restatements (tests/pointvoxel_ref.py).

The index structures come from the model's own code (initial_voxelize_steps with the one-pass level sort, unet_levels_steps,
point_index, voxel_index, lift_segments) over make_batch([0, 1, 2, 3]) at the KITTI and NuScenes shapes, and are checked bit for
bit against a numpy restatement from the integer coordinates.

Exact (assert_array_equal): the voxelize backward float32(go / count); the sorted voxelize forward (a float32 left-to-right sum
of float32(f / len) in ascending point order); the lift backward's segment sum; both voxelize forms at stride 1 (every segment
has length 1); the lift gather; the NCHW nearest resample both ways (at most two outputs per input pixel: one rounding); the
nearest-index rule; the trilinear weights.  hipcc emits correctly rounded float32 division and the code does not reassociate.

Bound-gated, |got - ref| <= (L + 8) * 2^-24 * R with R the computation on absolute values and L the element's addition chain:
the atomic voxelize forward and lift backward (L = entries of the destination), the devoxelize forward (L = 8, fma-contracted),
both devoxelize backwards (L = entries of the voxel).  Every such gate must also reject two mutants of the reference: one entry
of the longest segment removed, and that entry credited to the neighbouring destination."""
import numpy as np
import pytest
import torch

from oracle import ft_oracle as O
from tests import pointvoxel_ref as R

pytestmark = pytest.mark.gpu

WORST = {}       # kernel -> worst error / bound
LONGEST = {}     # case -> longest segment


@pytest.fixture(scope="module")
def spf():
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield spf
    print("\nworst error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    print("longest segment per case: " + ", ".join(f"{k} {v}" for k, v in LONGEST.items()))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def randn(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the production index
_CASES = {}


def build_case(batch, H, W):
    """The index structures of one batch, built the way SPVCNN._index_steps(ahead=True) builds them in training."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models.image_models_billinear import pack_img_indices
    from fusiontransformer_amd.models.utils import initial_voxelize_steps, point_index, voxel_index
    from fusiontransformer_amd.sparse import PointTensor, drain
    coords = torch.from_numpy(batch["coords"]).int().cuda()
    z = PointTensor(torch.from_numpy(batch["feats"]).cuda(), coords.float().contiguous())
    x0 = drain(initial_voxelize_steps(z, 1, 1, levels=R.LEVELS))
    cm = x0.cm
    drain(cm.unet_levels_steps(R.LEVELS))
    point_index(cm, 1, z, cm.coords[1].shape[0], with_segments=True)
    for s in (16, 4):
        n_s = cm.coords[s].shape[0]
        point_index(cm, s, z, n_s, with_segments=True)
        voxel_index(cm, s, z, n_s)
    pi, pb = pack_img_indices(batch["img_indices"], "cuda")
    B = len(batch["img_indices"])
    g = R.LIFT_GRID
    af = z.additional_features
    case = {"coords": batch["coords"].astype(np.int32), "pc": host(z.C), "n": coords.shape[0], "B": B, "H": H, "W": W,
            "img_idx": host(pi), "frame": host(pb), "pi": pi, "pb": pb, "lift_seg": spf.lift_segments(pi, pb, B, g, g, H, W), "s": {}}
    for s in (1, 4, 16):
        case["s"][s] = {"rows": host(cm.coords[s]), "idx": af["idx_query"][s], "counts": af["counts"][s], "vox_seg": af["vox_seg"][s],
                        "idx8": z.idx_query[s], "w8": z.weights[s], "devox_seg": af["devox_seg"][s], "m": cm.coords[s].shape[0]}
    return case


def production(shape):
    if shape not in _CASES:
        from fusiontransformer_amd.data.synth import make_batch
        _CASES[shape] = build_case(make_batch([0, 1, 2, 3], shape), *R.IMAGE_HW[shape])
    return _CASES[shape]


def check_index(case, name):
    """Every integer structure of the case against the numpy restatement, bit for bit; fills in the reference arrays."""
    for s, d in case["s"].items():
        rows, idx, counts = R.level_index(case["coords"], s)
        assert np.array_equal(d["rows"], rows), f"{name}: voxel rows at stride {s}"
        assert np.array_equal(host(d["idx"]), idx), f"{name}: idx_query at stride {s}"
        assert np.array_equal(host(d["counts"]), counts), f"{name}: counts at stride {s}"
        m = d["m"]
        L = R.check_segments(host(d["vox_seg"].order), host(d["vox_seg"].seg_off), idx, m, f"{name} voxelize s{s}")
        # the sorted forward divides by the segment length, the backward by counts: the two must be the same number
        assert np.array_equal(np.diff(host(d["vox_seg"].seg_off)), counts)
        LONGEST[f"{name} voxelize s{s}"] = L
        idx8 = R.corner_index(case["coords"], rows, s)
        assert np.array_equal(host(d["idx8"]), idx8), f"{name}: corner rows at stride {s}"
        w8 = host(d["w8"])
        np.testing.assert_array_equal(w8, O.calc_ti_weights(case["pc"], idx8.T, s).T, err_msg=f"{name}: weights at stride {s}")
        keys = np.where(w8 != 0, idx8, -1)
        LONGEST[f"{name} devoxelize s{s}"] = R.check_segments(host(d["devox_seg"].order), host(d["devox_seg"].seg_off), keys, m,
                                                              f"{name} devoxelize s{s}")
        d.update(ref_idx=idx, ref_counts=counts, ref_idx8=idx8, ref_keys=keys.reshape(-1),
                 ref_vox=R.segments(idx, m), ref_devox=R.segments(keys, m))
    g = R.LIFT_GRID
    cells = R.lift_cells(case["img_idx"], case["frame"], case["H"], case["W"])
    m = case["B"] * g * g
    LONGEST[f"{name} lift"] = R.check_segments(host(case["lift_seg"].order), host(case["lift_seg"].seg_off), cells, m, f"{name} lift")
    case["ref_cells"], case["ref_lift"] = cells, R.segments(cells, m)
    case["checked"] = True


def checked(shape):
    case = production(shape)
    if not case.get("checked"):
        check_index(case, shape)
    return case


# ------------------------------------------------------------------------------------------------ kernel checks on a case
def voxelize_checks(spf, case, name, s, c, rng):
    d = case["s"][s]
    n, m = case["n"], d["m"]
    idx, counts = d["ref_idx"], d["ref_counts"]
    f, go = randn(rng, n, c), randn(rng, m, c)
    ref, Rabs, L = R.voxelize_ref(f, idx, counts)
    muts = R.scatter_mutants(idx, m, lambda e: f[e].astype(np.float64) / counts[idx[e]][:, None])
    fd = dev(f).requires_grad_(True)
    out = spf.spvoxelize(fd, d["idx"], d["counts"], d["vox_seg"])         # c % 4 != 0: the wrapper takes the atomic form
    if c % 4 == 0:
        exact = R.segment_sum_seq(f, *d["ref_vox"], mean=True)
        np.testing.assert_array_equal(host(out), exact, err_msg=f"{name} voxelize_fwd_sorted s{s} c{c}")
        again = spf.spvoxelize(dev(f), d["idx"], d["counts"], d["vox_seg"])
        assert torch.equal(out, again), "sorted voxelize forward differs run to run"
    R.gate(f"{name} voxelize s{s} c{c}", host(out), ref, Rabs, L, muts, WORST, "voxelize_fwd_sorted" if c % 4 == 0 else "voxelize_fwd (c % 4 != 0)")
    (gf,) = torch.autograd.grad(out, fd, dev(go))
    np.testing.assert_array_equal(host(gf), R.voxelize_bwd_exact(go, idx, counts), err_msg=f"{name} voxelize_bwd s{s} c{c}")
    atomic = spf.spvoxelize(dev(f), d["idx"], d["counts"])
    R.gate(f"{name} atomic voxelize s{s} c{c}", host(atomic), ref, Rabs, L, muts, WORST, "voxelize_fwd (atomic)")
    if s == 1 and counts.max() == 1:        # every segment has length 1: both forms are copies
        want = np.zeros((m, c), dtype=np.float32)
        want[idx] = f
        np.testing.assert_array_equal(host(atomic), want)
        np.testing.assert_array_equal(host(out), want)


def devoxelize_checks(spf, case, name, s, c, rng):
    d = case["s"][s]
    n, m = case["n"], d["m"]
    idx8, w8 = d["ref_idx8"], host(d["w8"])
    f, go = randn(rng, m, c), randn(rng, n, c)
    ref, Rabs, L = R.devoxelize_ref(f, idx8, w8)
    fd = dev(f).requires_grad_(True)
    out = spf.spdevoxelize(fd, d["idx8"], d["w8"], d["devox_seg"])
    R.gate(f"{name} devoxelize s{s} c{c}", host(out), ref, Rabs, L, R.gather_mutants(idx8, w8, f, m), WORST, "devoxelize_fwd")
    bref, bR, bL = R.devoxelize_bwd_ref(go, idx8, w8, m)
    keys = d["ref_keys"]
    muts = R.scatter_mutants(keys, m, lambda e: w8.reshape(-1)[e][:, None].astype(np.float64) * go[e >> 3])
    (g1,) = torch.autograd.grad(out, fd, dev(go))
    R.gate(f"{name} devoxelize_bwd_sorted s{s} c{c}", host(g1), bref, bR, bL, muts, WORST, "devoxelize_bwd_sorted")
    fd2 = dev(f).requires_grad_(True)
    (g2,) = torch.autograd.grad(spf.spdevoxelize(fd2, d["idx8"], d["w8"], d["devox_seg"]), fd2, dev(go))
    assert torch.equal(g1, g2), "sorted devoxelize backward differs run to run"
    fd3 = dev(f).requires_grad_(True)
    (g3,) = torch.autograd.grad(spf.spdevoxelize(fd3, d["idx8"], d["w8"]), fd3, dev(go))
    R.gate(f"{name} devoxelize_bwd (atomic) s{s} c{c}", host(g3), bref, bR, bL, muts, WORST, "devoxelize_bwd (atomic)")


def upsample_cells(B, H, W, g=R.LIFT_GRID):
    """(B, H, W) int64: the flat grid cell under every pixel of a materialised nn.Upsample((H, W)) of a B x g x g grid."""
    ids = torch.arange(B * g * g, dtype=torch.float32).view(B, 1, g, g)
    return torch.nn.Upsample((H, W))(ids)[:, 0].long().numpy()


def lift_checks(spf, case, name, rng, c=R.LIFT_C):
    B, H, W, g = case["B"], case["H"], case["W"], R.LIFT_GRID
    n, m = case["img_idx"].shape[0], B * g * g
    grid, go = randn(rng, B, g, g, c), randn(rng, n, c)
    cells_up = upsample_cells(B, H, W)[case["frame"], case["img_idx"][:, 0], case["img_idx"][:, 1]] if n else np.zeros(0, np.int64)
    assert np.array_equal(cells_up, case["ref_cells"]), f"{name}: lift cells != nn.Upsample"
    gd = dev(grid).requires_grad_(True)
    out = spf.lift_gather(gd, case["pi"], case["pb"], H, W, case["lift_seg"])
    np.testing.assert_array_equal(host(out), grid.reshape(m, c)[cells_up], err_msg=f"{name} lift_gather_fwd")
    (g1,) = torch.autograd.grad(out, gd, dev(go))
    np.testing.assert_array_equal(host(g1).reshape(m, c), R.segment_sum_seq(go, *case["ref_lift"]), err_msg=f"{name} segment_sum")
    gd2 = dev(grid).requires_grad_(True)
    (g2,) = torch.autograd.grad(spf.lift_gather(gd2, case["pi"], case["pb"], H, W), gd2, dev(go))
    ref, Rabs, L = R.segment_sum_ref(go, case["ref_cells"], m)
    muts = R.scatter_mutants(case["ref_cells"], m, lambda e: go[e])
    R.gate(f"{name} lift_gather_bwd (atomic)", host(g2).reshape(m, c), ref, Rabs, L, muts, WORST, "lift_gather_bwd (atomic)")
    R.gate(f"{name} segment_sum", host(g1).reshape(m, c), ref, Rabs, L, muts, WORST, "segment_sum")


# ------------------------------------------------------------------------------------------------ full size
SHAPES = ["kitti", "nuscenes"]


@pytest.mark.parametrize("shape", SHAPES)
def test_production_index_structures(spf, shape):
    case = checked(shape)
    assert case["n"] > 80000 and case["s"][1]["m"] == case["n"]       # synthetic frames are voxel-unique at stride 1


@pytest.mark.parametrize("shape", SHAPES)
def test_trilinear_weights_of_jittered_points_are_exact(spf, shape):
    """calc_ti_weights at strides 1, 4, 16 on the production corner rows, with points moved off the integer grid."""
    case = checked(shape)
    rng = np.random.default_rng(1)
    pc = case["pc"].copy()
    pc[:, :3] += rng.uniform(0, 1, size=(pc.shape[0], 3)).astype(np.float32)
    for s in (1, 4, 16):
        idx8 = case["s"][s]["ref_idx8"]
        w = host(spf.calc_ti_weights(dev(pc), dev(idx8), s))
        np.testing.assert_array_equal(w, O.calc_ti_weights(pc, idx8.T, s).T, err_msg=f"stride {s}")


@pytest.mark.parametrize("shape", SHAPES)
def test_voxelize_full_size(spf, shape):
    case = checked(shape)
    rng = np.random.default_rng(2)
    for s, c in R.VOXELIZE_RUNS:
        voxelize_checks(spf, case, shape, s, c, rng)


@pytest.mark.parametrize("shape", SHAPES)
def test_devoxelize_full_size(spf, shape):
    case = checked(shape)
    rng = np.random.default_rng(3)
    for s, c in R.DEVOXELIZE_RUNS:
        devoxelize_checks(spf, case, shape, s, c, rng)


@pytest.mark.parametrize("shape", SHAPES)
def test_lift_full_size(spf, shape):
    lift_checks(spf, checked(shape), shape, np.random.default_rng(4))


@pytest.mark.parametrize("shape", SHAPES)
def test_resample_full_size(spf, shape):
    """sample_down's NCHW nearest resample of the image to 384 x 384, forward and backward."""
    H, W = R.IMAGE_HW[shape]
    rng = np.random.default_rng(5)
    img, go = randn(rng, 4, 3, H, W), randn(rng, 4, 3, 384, 384)
    x = dev(img).requires_grad_(True)
    out = spf.resample_nearest(x, (384, 384))
    it = torch.from_numpy(img).requires_grad_(True)
    up = torch.nn.Upsample((384, 384))(it)
    np.testing.assert_array_equal(host(out), up.detach().numpy())
    (gi,) = torch.autograd.grad(out, x, dev(go))
    rows, cols = O.nearest_src_index(384, H), O.nearest_src_index(384, W)
    hits = np.zeros((H, W), dtype=np.int64)
    np.add.at(hits, (rows[:, None], cols[None, :]), 1)
    assert hits.max() <= 2          # at most two terms per input pixel: the float64 sum rounded once is the float32 result
    ref = np.zeros((4, 3, H * W))
    flat = (rows[:, None] * W + cols[None, :]).reshape(-1)
    for b in range(4):
        for ch in range(3):
            ref[b, ch] = np.bincount(flat, weights=go[b, ch].reshape(-1).astype(np.float64), minlength=H * W)
    np.testing.assert_array_equal(host(gi), ref.reshape(4, 3, H, W).astype(np.float32))
    up.backward(torch.from_numpy(go))
    np.testing.assert_array_equal(host(gi), it.grad.numpy())


@pytest.mark.parametrize("H,W", [(370, 1226), (384, 1248), (900, 1600)])
def test_nearest_rule_every_row_and_column(spf, H, W):
    """The nearest source index of every output row and column: 24 x 24 -> H x W (the lift) and H x W -> 384 x 384 (sample_down),
    through the resample and through the lift gather, against nn.Upsample and the float32 rule."""
    g = R.LIFT_GRID
    rows, cols = O.nearest_src_index(H, g), O.nearest_src_index(W, g)
    cells = (rows[:, None] * g + cols[None, :]).astype(np.float32)
    ids = torch.arange(g * g, dtype=torch.float32).view(1, 1, g, g)
    up = host(spf.resample_nearest(dev(ids.numpy()), (H, W)))[0, 0]
    np.testing.assert_array_equal(up, cells)
    np.testing.assert_array_equal(up, torch.nn.Upsample((H, W))(ids)[0, 0].numpy())
    big = np.arange(H * W, dtype=np.float32).reshape(1, 1, H, W)         # < 2^24: exact in float32
    down = host(spf.resample_nearest(dev(big), (384, 384)))[0, 0]
    want = (O.nearest_src_index(384, H)[:, None] * W + O.nearest_src_index(384, W)[None, :]).astype(np.float32)
    np.testing.assert_array_equal(down, want)
    np.testing.assert_array_equal(down, torch.nn.Upsample((384, 384))(torch.from_numpy(big))[0, 0].numpy())
    # the lift gather: one point on every row and one on every column
    r = np.concatenate([np.arange(H), np.arange(W) % H])
    c = np.concatenate([np.arange(H) % W, np.arange(W)])
    pi, pb = dev(np.stack([r, c], 1).astype(np.int64)), dev(np.zeros(r.shape[0], dtype=np.int32))
    grid = np.arange(g * g * 4, dtype=np.float32).reshape(1, g, g, 4)
    out = host(spf.lift_gather(dev(grid), pi, pb, H, W))
    np.testing.assert_array_equal(out[:, 0], 4 * (rows[r] * g + cols[c]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ forms, fallbacks, edges
def test_voxelize_segments_equal_level_segments(spf):
    """The generic sort (voxelize_segments) and the one-pass level sort give the same segments and the same outputs."""
    case = checked("kitti")
    rng = np.random.default_rng(6)
    for s in (4, 16):
        d = case["s"][s]
        seg = spf.voxelize_segments(d["idx"], d["m"])
        assert torch.equal(seg.order, d["vox_seg"].order) and torch.equal(seg.seg_off, d["vox_seg"].seg_off)
        f = dev(randn(rng, case["n"], 64))
        assert torch.equal(spf.spvoxelize(f, d["idx"], d["counts"], seg), spf.spvoxelize(f, d["idx"], d["counts"], d["vox_seg"]))


@pytest.mark.parametrize("c", [3, 18])
def test_channels_not_a_multiple_of_four_take_the_atomic_path(spf, c):
    """A `seg` is passed, but c % 4 != 0: spvoxelize runs the float-atomic form, within the bound, at stride 16's longest segments."""
    voxelize_checks(spf, checked("kitti"), "kitti", 16, c, np.random.default_rng(7))


def test_channels_not_a_multiple_of_four_are_refused_by_the_gathers(spf):
    x6 = torch.zeros((10, 6), device="cuda")
    idx8 = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
    w8 = torch.ones((4, 8), device="cuda")
    with pytest.raises(RuntimeError):
        spf.spdevoxelize(x6, idx8, w8)
    with pytest.raises(RuntimeError):
        spf.spdevoxelize(x6, idx8, w8, spf.devoxelize_segments(idx8, w8, 10))
    pi = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    pb = torch.zeros((4,), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        spf.lift_gather(torch.zeros((1, 24, 24, 6), device="cuda"), pi, pb, 370, 1226)


def small_case(idx, m):
    """A voxelize case from an explicit point -> row map (entries outside [0, m) are dropped by every form)."""
    from fusiontransformer_amd import functional as spf
    idx = np.asarray(idx, dtype=np.int32)
    valid = idx[(idx >= 0) & (idx < m)]
    counts = np.bincount(valid, minlength=m).astype(np.int32)
    return {"n": idx.shape[0], "s": {0: {"m": m, "idx": dev(idx), "counts": dev(counts), "vox_seg": spf.voxelize_segments(dev(idx), m),
                                         "ref_idx": idx, "ref_counts": counts, "ref_vox": R.segments(idx, m)}}}


def small_devox(idx8, w8, m):
    from fusiontransformer_amd import functional as spf
    idx8, w8 = np.asarray(idx8, dtype=np.int32), np.asarray(w8, dtype=np.float32)
    keys = np.where(w8 != 0, idx8, -1)
    seg = spf.devoxelize_segments(dev(idx8), dev(w8), m)
    R.check_segments(host(seg.order), host(seg.seg_off), keys, m, "devoxelize_segments")
    return {"n": idx8.shape[0], "s": {0: {"m": m, "idx8": dev(idx8), "w8": dev(w8), "devox_seg": seg, "ref_idx8": idx8,
                                          "ref_keys": keys.reshape(-1)}}}


def test_sorted_and_atomic_forms_on_skewed_segments(spf):
    """Segment lengths from 1 to ~2000 (a geometric spread), every channel count the network uses."""
    rng = np.random.default_rng(8)
    m = 300
    idx = np.minimum(rng.geometric(0.01, 6000) - 1, m - 1).astype(np.int32)
    case = small_case(idx, m)
    for c in (4, 32, 96, 128, 256):
        voxelize_checks(spf, case, "skewed", 0, c, rng)
    idx8 = np.minimum(rng.geometric(0.01, (3000, 8)) - 1, m - 1).astype(np.int32)
    w8 = rng.uniform(0, 1, (3000, 8)).astype(np.float32)
    dcase = small_devox(idx8, w8, m)
    for c in (4, 96, 256):
        devoxelize_checks(spf, dcase, "skewed", 0, c, rng)


def test_invalid_indices_and_empty_voxels(spf):
    """idx entries of -1 and >= m are dropped by every form; voxels that receive no point come back as zero rows."""
    rng = np.random.default_rng(9)
    m = 50
    idx = rng.integers(-1, m + 5, 2000).astype(np.int32)
    idx[np.isin(idx, [3, 17, 49])] = -1              # three voxels with no points
    case = small_case(idx, m)
    for c in (8, 6):
        voxelize_checks(spf, case, "invalid", 0, c, rng)
        out = host(spf.spvoxelize(dev(randn(rng, 2000, c)), case["s"][0]["idx"], case["s"][0]["counts"], case["s"][0]["vox_seg"]))
        assert not out[[3, 17, 49]].any()
    idx8 = rng.integers(-1, m + 5, (1500, 8)).astype(np.int32)
    w8 = rng.uniform(0, 1, (1500, 8)).astype(np.float32)    # non-zero weights on the invalid corners too
    idx8[np.isin(idx8, [3, 17, 49])] = -1
    dcase = small_devox(idx8, w8, m)
    devoxelize_checks(spf, dcase, "invalid", 0, 8, rng)
    f = dev(randn(rng, m, 8)).requires_grad_(True)
    (g,) = torch.autograd.grad(spf.spdevoxelize(f, dcase["s"][0]["idx8"], dcase["s"][0]["w8"], dcase["s"][0]["devox_seg"]), f,
                               dev(randn(rng, 1500, 8)))
    assert not host(g)[[3, 17, 49]].any()


def test_zero_weight_corners_with_valid_indices(spf):
    """As in voxel_to_point(nearest=True) before its indices are cleared: corners 1..7 weigh 0 but point at real voxels.  The
    sorted backward drops them; the forward adds exact zeros after float32(w0 * f0)."""
    rng = np.random.default_rng(10)
    m, n, c = 400, 5000, 32
    idx8 = rng.integers(0, m, (n, 8)).astype(np.int32)
    w8 = np.zeros((n, 8), dtype=np.float32)
    w8[:, 0] = rng.uniform(0.1, 1, n).astype(np.float32)
    dcase = small_devox(idx8, w8, m)
    devoxelize_checks(spf, dcase, "zero-weight", 0, c, rng)
    f = randn(rng, m, c)
    out = host(spf.spdevoxelize(dev(f), dcase["s"][0]["idx8"], dcase["s"][0]["w8"]))
    np.testing.assert_array_equal(out, w8[:, :1] * f[idx8[:, 0]])


def test_one_voxel_holds_every_point(spf):
    """L = n: every point in voxel 1 of 3 (voxels 0 and 2 empty), and every corner of every point on voxel 1.  The sizes keep
    L^2 * 2^-24 well below 1, so that the bound still resolves one point (4096 points; 1024 points = 8192 corner entries)."""
    rng = np.random.default_rng(11)
    case = small_case(np.ones(4096, dtype=np.int32), 3)
    for c in (4, 32, 3):
        voxelize_checks(spf, case, "one-voxel", 0, c, rng)
    n = 1024
    dcase = small_devox(np.ones((n, 8), dtype=np.int32), rng.uniform(0, 1, (n, 8)).astype(np.float32), 3)
    devoxelize_checks(spf, dcase, "one-voxel", 0, 32, rng)


def test_empty_sizes(spf):
    """n = 0 (no points, m > 0: zero rows) and m = 0 (points but no voxels: zero gradients), every form."""
    for n, m in ((0, 5), (7, 0)):
        idx = np.full(n, -1, dtype=np.int32)
        case = small_case(idx, m)
        d = case["s"][0]
        for seg in (None, d["vox_seg"]):
            f = torch.ones((n, 8), device="cuda", requires_grad=True)
            out = spf.spvoxelize(f, d["idx"], d["counts"], seg)
            assert out.shape == (m, 8) and not out.any()
            (g,) = torch.autograd.grad(out, f, torch.ones((m, 8), device="cuda"))
            assert g.shape == (n, 8) and not g.any()
        idx8, w8 = dev(np.zeros((n, 8), dtype=np.int32)), dev(np.ones((n, 8), dtype=np.float32))
        for seg in (None, spf.devoxelize_segments(idx8, w8, m)):
            f = torch.ones((m, 8), device="cuda", requires_grad=True)
            out = spf.spdevoxelize(f, idx8, w8, seg)
            assert out.shape == (n, 8) and not out.any()
            (g,) = torch.autograd.grad(out, f, torch.ones((n, 8), device="cuda"))
            assert g.shape == (m, 8) and not g.any()
    pi, pb = dev(np.zeros((0, 2), dtype=np.int64)), dev(np.zeros(0, dtype=np.int32))
    for seg in (None, spf.lift_segments(pi, pb, 2, 24, 24, 370, 1226)):
        grid = torch.ones((2, 24, 24, 8), device="cuda", requires_grad=True)
        out = spf.lift_gather(grid, pi, pb, 370, 1226, seg)
        assert out.shape == (0, 8)
        (g,) = torch.autograd.grad(out, grid, torch.ones((0, 8), device="cuda"))
        assert not g.any()


def test_batch_with_an_empty_frame(spf):
    """Frames 0 and 2 of a three-frame batch: the index structures, the kernels, and zero lift gradients for frame 1."""
    from fusiontransformer_amd.data.synth import make_batch
    b = make_batch([0, 1, 2], max_points=4000)
    keep = b["coords"][:, 3] != 1
    b = dict(b, coords=b["coords"][keep], feats=b["feats"][keep])
    b["img_indices"] = [b["img_indices"][0], np.zeros((0, 2), dtype=np.int64), b["img_indices"][2]]
    case = build_case(b, *R.IMAGE_HW["kitti"])
    check_index(case, "empty frame")
    rng = np.random.default_rng(12)
    for s, c in R.VOXELIZE_RUNS:
        voxelize_checks(spf, case, "empty frame", s, c, rng)
    for s, c in R.DEVOXELIZE_RUNS[:3]:
        devoxelize_checks(spf, case, "empty frame", s, c, rng)
    lift_checks(spf, case, "empty frame", rng)
    grid = torch.ones((3, 24, 24, 8), device="cuda", requires_grad=True)
    (g,) = torch.autograd.grad(spf.lift_gather(grid, case["pi"], case["pb"], 370, 1226, case["lift_seg"]), grid,
                               torch.ones((case["img_idx"].shape[0], 8), device="cuda"))
    assert not g[1].any() and g[0].any() and g[2].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_lift_on_the_four_image_corners(spf, shape):
    """Every frame has points on the four image corners (and 2000 random pixels): forward, both backwards."""
    from fusiontransformer_amd import functional as F
    H, W = R.IMAGE_HW[shape]
    rng = np.random.default_rng(13)
    B = 2
    idx = [np.concatenate([[[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]],
                           np.stack([rng.integers(0, H, 2000), rng.integers(0, W, 2000)], 1)]).astype(np.int64) for _ in range(B)]
    img_idx = np.concatenate(idx)
    frame = np.repeat(np.arange(B, dtype=np.int32), 2004)
    pi, pb = dev(img_idx), dev(frame)
    g = R.LIFT_GRID
    case = {"B": B, "H": H, "W": W, "img_idx": img_idx, "frame": frame, "pi": pi, "pb": pb, "lift_seg": F.lift_segments(pi, pb, B, g, g, H, W)}
    cells = R.lift_cells(img_idx, frame, H, W)
    assert set(cells[:4].tolist()) == {0, g - 1, (g - 1) * g, g * g - 1}
    R.check_segments(host(case["lift_seg"].order), host(case["lift_seg"].seg_off), cells, B * g * g, "corners")
    case["ref_cells"], case["ref_lift"] = cells, R.segments(cells, B * g * g)
    lift_checks(spf, case, f"{shape} corners", rng)
