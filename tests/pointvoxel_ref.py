"""Host references and assertion gates for the point <-> voxel and image-lift kernels (csrc/ftx_pointvoxel.hip), shared by
tests/test_pointvoxel_host.py (CPU) and tests/test_pointvoxel_fullsize_gpu.py.

* Index structures: a numpy restatement from the integer coordinates.  A level's voxel rows are its distinct coordinates in
  ascending sphash order (the library's row order); a point's voxel, its 8 trilinear corners and its lift cell follow from the
  coordinates alone.  The sorted segments of every scatter are the stable argsort of the entries' destinations.
* Exact restatements (float32, numpy): the sorted voxelize forward (a left-to-right sum of float32(f / len) in ascending entry
  order), the plain segment sum of the lift backward, the voxelize backward float32(go / count).
* float64 references with the absolute-value twin R for the bound |got - ref| <= (L + 8) * 2^-24 * R, L the element's chain of
  float32 additions.
* gate(): the bound on a kernel result and on two mutants of the reference (one entry of the longest segment removed; that entry
  credited to the neighbouring destination instead), which it must reject."""
import numpy as np
import torch

from oracle import ft_oracle as O

U = 2.0 ** -24
LEVELS = (1, 2, 4, 8, 16)
LIFT_GRID = 24                       # 384 / 16: the ViT token grid the lift reads
IMAGE_HW = {"kitti": (370, 1226), "nuscenes": (900, 1600)}
# (stride, channels) of point_to_voxel and voxel_to_point in the SPVCNN backbone, in the order the network runs them
VOXELIZE_RUNS = ((1, 32), (16, 256), (4, 128))
DEVOXELIZE_RUNS = ((1, 32), (16, 256), (4, 128), (1, 96))
LIFT_C = 96


# ------------------------------------------------------------------------------------------------ index structures
def level_coords(coords, s):
    """floor_div(xyz, s) * s with the batch column kept (int32)."""
    c = np.asarray(coords, dtype=np.int64).copy()
    c[:, :3] = np.floor_divide(c[:, :3], s) * s
    return c.astype(np.int32)


def level_index(coords, s):
    """(rows (m, 4): the level's voxels in ascending sphash order, idx (n,) int32: each point's row, counts (m,) int32)."""
    lc = level_coords(coords, s)
    h = O.sphash(lc)
    _, first, inv = np.unique(h, return_index=True, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int32)
    return lc[first], inv, np.bincount(inv, minlength=first.shape[0]).astype(np.int32)


def corner_index(coords, rows, s):
    """(n, 8) int32: the row among `rows` (a level's voxels, ascending sphash) of each of the point's 8 corners
    floor_div(p, s) * s + KernelRegion(2, s) offsets (z fastest), -1 where that voxel does not exist."""
    rh = O.sphash(rows)
    order = np.argsort(rh, kind="stable")
    srt = rh[order]
    q = O.sphash(level_coords(coords, s), O.kernel_offsets(2, s)).T          # (n, 8)
    pos = np.minimum(np.searchsorted(srt, q), max(srt.shape[0] - 1, 0))
    hit = srt[pos] == q if srt.shape[0] else np.zeros(q.shape, dtype=bool)
    return np.where(hit, order[pos], -1).astype(np.int32)


def lift_cells(img_idx, frame, H, W, g=LIFT_GRID):
    """Flat (frame, source row, source column) cell of nn.Upsample((H, W)) from a g x g grid read by each point."""
    rows, cols = O.nearest_src_index(H, g), O.nearest_src_index(W, g)
    img_idx = np.asarray(img_idx, dtype=np.int64)
    return ((np.asarray(frame, dtype=np.int64) * g + rows[img_idx[:, 0]]) * g + cols[img_idx[:, 1]]).astype(np.int32)


def segments(keys, m):
    """The sorted segments of a scatter with destinations `keys` (entries outside [0, m) dropped): (order, seg_off), entries in
    ascending order inside every destination."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    k = np.where((k >= 0) & (k < m), k, m)
    order = np.argsort(k, kind="stable")
    cnt = np.bincount(k[k < m], minlength=m)
    return order[:int(cnt.sum())].astype(np.int32), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)


def check_segments(order, seg_off, keys, m, what):
    """A Segments (order, seg_off) against its destinations, bit for bit; returns the longest segment."""
    order, seg_off = np.asarray(order), np.asarray(seg_off)
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    valid = (k >= 0) & (k < m)
    assert seg_off.shape == (m + 1,) and seg_off[0] == 0, (what, seg_off.shape, seg_off[:1])
    lens = np.diff(seg_off.astype(np.int64))
    assert np.array_equal(lens, np.bincount(k[valid], minlength=m)), f"{what}: segment lengths != per-destination counts"
    end = int(seg_off[-1])
    got = order[:end].astype(np.int64)
    assert np.array_equal(np.sort(got), np.nonzero(valid)[0]), f"{what}: order[:seg_off[-1]] is not a permutation of the valid entries"
    assert np.array_equal(k[got], np.repeat(np.arange(m), lens)), f"{what}: an entry sits in another destination's segment"
    inside = np.repeat(np.arange(m), lens)
    same = inside[1:] == inside[:-1]
    assert (np.diff(got)[same] > 0).all(), f"{what}: entries are not in ascending order inside a segment"
    return int(lens.max()) if m else 0


# ------------------------------------------------------------------------------------------------ exact float32 restatements
def segment_sum_seq(src, order, seg_off, mean=False, rows=None):
    """float32: out[v] = sum over the entries e of segment v, left to right, of src[rows(e)] (mean: each term float32(src / len)).
    Vectorised over segments, one step per position in the segment.  `rows`: entry -> source row (default: the entry)."""
    src = np.asarray(src, dtype=np.float32)
    order, seg_off = np.asarray(order, dtype=np.int64), np.asarray(seg_off, dtype=np.int64)
    m = seg_off.shape[0] - 1
    lens = np.diff(seg_off)
    out = np.zeros((m, src.shape[1]), dtype=np.float32)
    for p in range(int(lens.max()) if m else 0):
        act = np.nonzero(lens > p)[0]
        e = order[seg_off[act] + p]
        t = src[e if rows is None else rows[e]]
        if mean:
            t = t / lens[act].astype(np.float32)[:, None]
        out[act] = out[act] + t
    return out


def voxelize_bwd_exact(go, idx, counts):
    """float32(go[idx] / counts[idx]); zero rows for points outside [0, m) or in a voxel of count 0."""
    go = np.asarray(go, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64)
    m = go.shape[0]
    ok = (idx >= 0) & (idx < m)
    r = np.where(ok, idx, 0)
    cnt = np.asarray(counts)[r] if m else np.zeros(idx.shape, dtype=np.int32)
    ok &= cnt > 0
    out = np.zeros((idx.shape[0], go.shape[1]), dtype=np.float32)
    out[ok] = go[r[ok]] / cnt[ok].astype(np.float32)[:, None]
    return out


# ------------------------------------------------------------------------------------------------ float64 references
def _scatter(dst, vals, m):
    """float64 (sum, sum of |.|) of vals[e] into rows dst[e] (torch's index_add_ on the CPU)."""
    d = torch.from_numpy(np.asarray(dst, dtype=np.int64))
    v = torch.from_numpy(np.asarray(vals, dtype=np.float64))
    z = torch.zeros((m, v.shape[1]), dtype=torch.float64)
    return z.index_add(0, d, v).numpy(), z.index_add(0, d, v.abs()).numpy()


def voxelize_ref(f, idx, counts):
    """float64 scatter-mean (ref, R, L): out[idx[i]] += f[i] / counts[idx[i]]; L = counts."""
    f = np.asarray(f, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    m = counts.shape[0]
    ok = (idx >= 0) & (idx < m)
    ok[ok] &= counts[idx[ok]] > 0
    return _scatter(idx[ok], f[ok] / counts[idx[ok]][:, None], m) + (counts,)


def segment_sum_ref(src, keys, m):
    """float64 scatter-add (ref, R, L) of src rows to keys (outside [0, m) dropped); L = entries per destination."""
    src = np.asarray(src, dtype=np.float64)
    k = np.asarray(keys, dtype=np.int64)
    ok = (k >= 0) & (k < m)
    return _scatter(k[ok], src[ok], m) + (np.bincount(k[ok], minlength=m),)


def devoxelize_ref(f, idx8, w8):
    """float64 8-corner gather (ref, R, L = 8): out[i] = sum_k w[i,k] * f[idx[i,k]] over corners inside [0, m)."""
    f = torch.from_numpy(np.asarray(f, dtype=np.float64))
    idx8, w8 = np.asarray(idx8, dtype=np.int64), np.asarray(w8, dtype=np.float64)
    m = f.shape[0]
    out, R = torch.zeros((idx8.shape[0], f.shape[1]), dtype=torch.float64), torch.zeros((idx8.shape[0], f.shape[1]), dtype=torch.float64)
    for k in range(8):
        ok = (idx8[:, k] >= 0) & (idx8[:, k] < m)
        if not m:
            break
        g = f[torch.from_numpy(np.where(ok, idx8[:, k], 0))] * torch.from_numpy(np.where(ok, w8[:, k], 0.0))[:, None]
        out += g
        R += g.abs()
    return out.numpy(), R.numpy(), np.full(idx8.shape[0], 8)


def devoxelize_bwd_ref(go, idx8, w8, m):
    """float64 transpose of the gather (ref, R, L): grad[idx[i,k]] += w[i,k] * go[i] over corners inside [0, m) with w != 0;
    L = entries per voxel."""
    go = np.asarray(go, dtype=np.float64)
    idx8, w8 = np.asarray(idx8, dtype=np.int64), np.asarray(w8, dtype=np.float64)
    keys = np.where(w8 != 0, idx8, -1)
    ok = (keys >= 0) & (keys < m)
    out, R = np.zeros((m, go.shape[1])), np.zeros((m, go.shape[1]))
    for k in range(8):
        sel = ok[:, k]
        a, b = _scatter(keys[sel, k], go[sel] * w8[sel, k][:, None], m)
        out += a
        R += b
    return out, R, np.bincount(keys[ok], minlength=m)


def bound(R, L):
    """(L + 8) * 2^-24 * R with L per destination row."""
    return (np.asarray(L, dtype=np.float64).reshape(-1, 1) + 8) * U * R


# ------------------------------------------------------------------------------------------------ mutants and the gate
def scatter_mutants(keys, m, term):
    """The two mutants of a scatter's reference: the largest term of the longest destination removed, and that term credited to
    the neighbouring destination instead.  keys (E,): each entry's destination; term(entries) -> (len, c) float64 terms."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    ok = (k >= 0) & (k < m)
    v = int(np.argmax(np.bincount(k[ok], minlength=m)))
    ents = np.nonzero(k == v)[0]
    t = np.asarray(term(ents), dtype=np.float64)
    t = t[int(np.argmax(np.abs(t).max(1)))]
    vn = v + 1 if v + 1 < m else v - 1
    return [[(v, -t)], [(v, -t), (vn, t)]]


def gather_mutants(idx8, w8, f, m):
    """devoxelize forward: the largest corner term of one point removed, and that term credited to the next point instead."""
    idx8, w8 = np.asarray(idx8, dtype=np.int64), np.asarray(w8, dtype=np.float64)
    ok = (idx8 >= 0) & (idx8 < m)
    mag = np.where(ok, np.abs(w8), 0.0) * np.abs(np.asarray(f, dtype=np.float64)).max(1)[np.where(ok, idx8, 0)]
    i, k = np.unravel_index(int(np.argmax(mag)), mag.shape)
    t = w8[i, k] * np.asarray(f, dtype=np.float64)[idx8[i, k]]
    j = i + 1 if i + 1 < idx8.shape[0] else i - 1
    return [[(int(i), -t)], [(int(i), -t), (int(j), t)]]


def ratio(got, ref, bnd):
    """max |got - ref| / bound; an element whose bound is 0 must match exactly."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if ((bnd <= 0) & (d > 0)).any():
        return float("inf")
    r = np.where(bnd > 0, d / np.where(bnd > 0, bnd, 1.0), 0.0)
    return float(r.max()) if r.size else 0.0


def gate(what, got, ref, R, L, mutants, worst=None, kernel=None):
    """Assert the bound on `got`; assert it rejects each mutant (a list of (row, delta) parts applied to the reference).
    Returns the worst ratio of error to bound; `worst[kernel]` keeps the maximum over calls."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    b = bound(R, L)
    r = ratio(got, ref, b)
    if worst is not None:
        worst[kernel] = max(worst.get(kernel, 0.0), r)
    assert r <= 1.0, f"{what}: error is {r:.3g} x the bound"
    assert len(mutants) == 2
    for i, parts in enumerate(mutants):
        assert any(ratio(ref[v] + dl, ref[v], b[v]) > 1.0 for v, dl in parts), f"{what}: the gate accepts mutant {i}"
    return r
