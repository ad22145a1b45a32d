"""Float64 restatement of the spatial transformers' affine grid sampling, the float32 yardstick the GPU tests take their bars from,
and the input selection of the gradient-with-respect-to-theta cases.

Semantics: F.grid_sample(src, F.affine_grid(theta, (b, ., H, W), align_corners=False), mode="bilinear", padding_mode="zeros",
align_corners=False).  Output pixel (r, c) of an (H, W) target:
    xn = (2c+1)/W - 1,  yn = (2r+1)/H - 1
    gx = t00 xn + t01 yn + t02,  gy = t10 xn + t11 yn + t12
    ix = ((gx+1) iw - 1)/2,  iy = ((gy+1) ih - 1)/2
and the value is the four-corner bilinear sum with corners outside the source counted as 0.  Written with torch ops so that autograd
gives the gradients of the closed form itself (floor carries none, exactly as in grid_sample's backward).

tests/golden/make_stn_golden.py checks this file against the reference's modules; tests/test_stn_host.py checks it against the
stored golden; tests/test_stn_gpu.py uses it as the truth."""
import numpy as np
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------------------------- closed form
def pixel_coords(theta, frame, row, col, H, W, ih, iw):
    """Source coordinates (ix, iy) of target pixels (frame, row, col) -- 1-d index tensors -- in theta's dtype."""
    dt = theta.dtype
    xn = (2 * col.to(dt) + 1) / W - 1
    yn = (2 * row.to(dt) + 1) / H - 1
    t = theta[frame]
    gx = t[:, 0, 0] * xn + t[:, 0, 1] * yn + t[:, 0, 2]
    gy = t[:, 1, 0] * xn + t[:, 1, 1] * yn + t[:, 1, 2]
    return ((gx + 1) * iw - 1) / 2, ((gy + 1) * ih - 1) / 2


def bilinear(src, frame, ix, iy):
    """(m, c) bilinear values of src (b, c, ih, iw) at (frame, iy, ix); corners outside count as 0."""
    ih, iw = src.shape[-2:]
    x0, y0 = torch.floor(ix.detach()), torch.floor(iy.detach())
    fx, fy = ix - x0, iy - y0
    out = 0
    for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        xi, yi = x0 + dx, y0 + dy
        inside = (xi >= 0) & (xi < iw) & (yi >= 0) & (yi < ih)
        xi, yi = xi.clamp(0, iw - 1).long(), yi.clamp(0, ih - 1).long()
        out = out + src[frame, :, yi, xi] * (w * inside.to(w.dtype))[:, None]
    return out


def sample_points(src, theta, img_idx, frame, H, W):
    """Rows (n, c) of the resampled (H, W) map at img_idx (n, 2) (row, col) of `frame` (n,), without the map.  Points whose frame
    or pixel is out of range give zero rows."""
    b = src.shape[0]
    frame, row, col = frame.long(), img_idx[:, 0].long(), img_idx[:, 1].long()
    ok = (frame >= 0) & (frame < b) & (row >= 0) & (row < H) & (col >= 0) & (col < W)
    out = torch.zeros((img_idx.shape[0], src.shape[1]), dtype=src.dtype)
    sel = torch.nonzero(ok).view(-1)
    if sel.numel():
        ix, iy = pixel_coords(theta, frame[sel], row[sel], col[sel], H, W, src.shape[2], src.shape[3])
        out = out.index_add(0, sel, bilinear(src, frame[sel], ix, iy))
    return out


def dense_pixels(b, H, W):
    f, r, c = torch.meshgrid(torch.arange(b), torch.arange(H), torch.arange(W), indexing="ij")
    return f.reshape(-1), r.reshape(-1), c.reshape(-1)


def sample(src, theta, size):
    """The dense form: (b, c, H, W)."""
    b, c, ih, iw = src.shape
    H, W = size
    f, r, col = dense_pixels(b, H, W)
    ix, iy = pixel_coords(theta, f, r, col, H, W, ih, iw)
    return bilinear(src, f, ix, iy).view(b, H, W, c).permute(0, 3, 1, 2)


def pick(dense, img_idx, frame):
    """The reference's per-frame pick (image_models_stn.py:91-98) for in-range points: dense[frame, :, row, col]."""
    return dense[frame.long(), :, img_idx[:, 0].long(), img_idx[:, 1].long()]


# ---------------------------------------------------------------------------------------------------------------- modules
def theta_of(params, prefix, x):
    """SpatialTransformer's localisation net + regressor (reference models/transformers.py:106-131) from a name -> tensor dict."""
    p = lambda k: params[prefix + k].to(x.dtype)
    xs = F.conv2d(x, p("localization.0.weight"), p("localization.0.bias"))
    xs = F.relu(F.max_pool2d(xs, 2, stride=2))
    xs = F.conv2d(xs, p("localization.3.weight"), p("localization.3.bias"))
    xs = F.relu(F.max_pool2d(xs, 2, stride=2))
    xs = xs.mean((2, 3))
    xs = F.relu(F.linear(xs, p("fc_loc.0.weight"), p("fc_loc.0.bias")))
    return F.linear(xs, p("fc_loc.2.weight"), p("fc_loc.2.bias")).view(-1, 2, 3)


def spatial_transformer(params, prefix, x, size):
    return sample(x, theta_of(params, prefix, x), size)


def up_conv(params, prefix, x, stride):
    return F.conv_transpose2d(x, params[prefix + "up_conv.weight"].to(x.dtype), params[prefix + "up_conv.bias"].to(x.dtype), stride=stride)


def scale_up(params, prefix, x, size, stride):
    return spatial_transformer(params, prefix + "up_stn.", up_conv(params, prefix, x, stride), size)


def scale_up_points(params, prefix, x, img_idx, frame, H, W, stride):
    m = up_conv(params, prefix, x, stride)
    return sample_points(m, theta_of(params, prefix + "up_stn.", m), img_idx, frame, H, W)


# ---------------------------------------------------------------------------------------------------------------- yardstick
def torch_points(src, theta, img_idx, frame, H, W):
    """torch's own affine_grid + grid_sample (in src's dtype, on the CPU) at the in-range points: the grid rows of the points' pixels go
    through grid_sample frame by frame, so this is torch's arithmetic on exactly those pixels, and autograd reaches src and theta."""
    b, c = src.shape[:2]
    grid = F.affine_grid(theta, (b, c, H, W), align_corners=False)
    out = torch.zeros((img_idx.shape[0], c), dtype=src.dtype)
    ok = (img_idx[:, 0] >= 0) & (img_idx[:, 0] < H) & (img_idx[:, 1] >= 0) & (img_idx[:, 1] < W)    # the rest: zero rows
    for f in range(b):
        sel = torch.nonzero((frame.long() == f) & ok).view(-1)
        if sel.numel() == 0:
            continue
        g = grid[f, img_idx[sel, 0].long(), img_idx[sel, 1].long()].view(1, 1, -1, 2)
        v = F.grid_sample(src[f:f + 1], g, mode="bilinear", padding_mode="zeros", align_corners=False)
        out = out.index_add(0, sel, v[0, :, 0].t())
    return out


def torch_dense(src, theta, size):
    grid = F.affine_grid(theta, (src.shape[0], src.shape[1]) + tuple(size), align_corners=False)
    return F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def rel_l2_per_frame(got, want):
    """Worst relative L2 error over the frames of a (b, 2, 3) gradient; 0 where both are exactly 0."""
    got, want = got.double().reshape(got.shape[0], -1), want.double().reshape(want.shape[0], -1)
    worst = 0.0
    for g, w in zip(got, want):
        d, n = (g - w).norm().item(), w.norm().item()
        if d == 0.0:
            continue
        worst = max(worst, d / n if n > 0 else float("inf"))
    return worst


# ---------------------------------------------------------------------------------------------------------------- inputs
def theta_case(kind, b, rng=None):
    """(b, 2, 3) float32 theta of a named case; `rng` adds a small seeded perturbation where the case allows one."""
    base = {"identity": [[1, 0, 0], [0, 1, 0]],
            "scale": [[1.4, 0, 0], [0, 1.4, 0]],                                   # samples fall outside the source
            "rotate": [[np.cos(np.pi / 6), -np.sin(np.pi / 6) + 0.2, 0.05], [np.sin(np.pi / 6), np.cos(np.pi / 6), -0.1]],   # 30 degrees + shear
            "flip": [[-1, 0, 0], [0, 1, 0]],
            "outside": [[1, 0, 5.0], [0, 1, 0]]}[kind]                             # every sample outside: all-zero output and gradients
    t = np.tile(np.asarray(base, dtype=np.float64)[None], (b, 1, 1))
    if rng is not None and kind != "outside":
        t = t + rng.uniform(-0.03, 0.03, size=t.shape)
    return torch.from_numpy(t.astype(np.float32))


def kink_distance(theta, frame, row, col, H, W, ih, iw):
    """Distance (in source pixels, float64) of every sample's coordinates from the nearest integer: d/d theta jumps there."""
    ix, iy = pixel_coords(theta.double(), frame, row, col, H, W, ih, iw)
    return torch.minimum((ix - torch.round(ix)).abs(), (iy - torch.round(iy)).abs())


def draw_dense_theta(kind, b, size, ih, iw, seed, margin=1e-3, tries=400):
    """Draws perturbed thetas of `kind` by seed until every float64 coordinate of the dense target is >= margin from an integer.
    Returns (theta float32, number of draws)."""
    H, W = size
    f, r, c = dense_pixels(b, H, W)
    for k in range(tries):
        th = theta_case(kind, b, np.random.default_rng(seed * 1000 + k))
        if kind == "outside" or kink_distance(th, f, r, c, H, W, ih, iw).min().item() >= margin:
            return th, k + 1
    raise AssertionError("no theta of kind %r is %g px clear of every kink in %d draws" % (kind, margin, tries))


def select_points(theta, img_idx, frame, H, W, ih, iw, margin):
    """Keeps the in-range candidate points whose float64 coordinates are >= margin from an integer.  Returns (kept mask, kept share)."""
    clear = kink_distance(theta, frame.long(), img_idx[:, 0].long(), img_idx[:, 1].long(), H, W, ih, iw) >= margin
    return clear, clear.double().mean().item()
