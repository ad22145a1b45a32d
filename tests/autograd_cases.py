"""One table entry per public differentiable entry point of fusiontransformer_amd/functional.py, for tests/test_autograd_contract_gpu.py.

A Case says how to build good operands (seeded; `scale` 2 is a different, larger input with different values), how to call the
entry, and what every tensor operand is:

  role "diff"     a differentiable input: asks for a gradient and gets one;
  role "refused"  a float input the node has no gradient for: the entry refuses it when it requires grad, by name;
  role "data"     indices, labels, running statistics, class weights.

`reads`: the backward reads the operand, so it went through save_for_backward and an in-place change after the forward must raise;
an input the node is linear in (reads False) may change, and the gradients must not.

`bad`: which of VARIATIONS are bad for the operand, i.e. must raise ValueError before anything is launched.  A variation is left
out where the call it makes is legal (a row count that only defines the output's, a layout the node copies or takes as it is, an
image of another size) or leaves the kernels' domain, so that the entry's dispatch hands it to the library path and torch answers
(linear, rows_matmul, vit_linear, vit_mlp); the reason stands beside every such entry.  `axis`: the dimension short / long change.

The shapes are the smallest that still cross each node's tiling edge: 257 and 300 rows (one 256-row block plus a part), 130 tokens
(two 64-row query tiles plus a part), 33 token rows, more than 128 pairs per kernel offset (one pair-GEMM tile plus a part)."""
import functools
import itertools

import numpy as np
import torch

VARIATIONS = ("float64", "cpu", "short", "long", "extra_dim", "strided")
ALL = frozenset(VARIATIONS)
F32, I32, I64 = torch.float32, torch.int32, torch.int64


class Op:
    def __init__(self, role="data", bad=ALL, axis=0, reads=True):
        self.role, self.bad, self.axis, self.reads = role, frozenset(bad), axis, reads


def diff(bad=ALL, axis=0, reads=True):
    return Op("diff", bad, axis, reads)


def but(*legal):
    return ALL - set(legal)


class Case:
    def __init__(self, cid, entry, build, call, ops, saves_output=False, nondet=(), truth=None, fullest=True, check=None):
        self.id, self.entry, self.build, self.call, self.ops = cid, entry, build, call, ops
        self.saves_output = saves_output    # the node keeps (a view of) its output for the backward
        self.nondet = frozenset(nondet)     # "out" / "grad": float atomics, judged at the scatter bound instead of bit for bit
        self.truth = truth                  # nondet cases: (operands, grad_out) -> {"out" | "grad": (float64 ref, R, L)}
        self.fullest = fullest              # every optional operand is given: the option set the bad-operand check runs at
        self.check = check                  # a property of the built operands the shapes were chosen for

    def names(self, role, o):
        return [k for k, op in self.ops.items() if op.role == role and o.get(k) is not None]

    def __repr__(self):
        return self.id


def rnd(seed, *shape, scale=1.0, shift=0.0):
    """Seeded on the CPU (the same values wherever the table is built), then moved to the device."""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F32) * scale + shift
    return t.cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- point <-> voxel, lift, resample
def _cloud(scale):
    """300 points in about 70 voxels (some points outside every voxel), 8 corners per point with zero-weight and absent ones."""
    rng = np.random.default_rng(40 + scale)
    n, m = 300 * scale, 70 * scale
    idx = rng.integers(-1, m, n).astype(np.int32)
    counts = np.bincount(idx[idx >= 0], minlength=m).astype(np.int32)
    idx8 = rng.integers(-1, m, (n, 8)).astype(np.int32)
    w8 = rng.uniform(0, 1, (n, 8)).astype(np.float32)
    w8[rng.random((n, 8)) < 0.1] = 0
    return n, m, idx, counts, idx8, w8


def _voxelize_case(with_seg):
    def build(scale=1):
        from fusiontransformer_amd import functional as spf
        n, m, idx, counts, _, _ = _cloud(scale)
        o = dict(feats=rnd(1 + scale, n, 32), idx=dev(idx), counts=dev(counts))
        o["seg"] = spf.voxelize_segments(o["idx"], m) if with_seg else None
        return o

    def truth(o, go):
        from tests import pointvoxel_ref as PV
        return {"out": PV.voxelize_ref(o["feats"].cpu().numpy(), o["idx"].cpu().numpy(), o["counts"].cpu().numpy())}

    ops = dict(feats=diff(but("strided"), reads=False),        # strided: copied
               idx=Op(),
               counts=Op(bad=ALL if with_seg else but("short", "long")))     # without segments the length of counts IS the voxel count
    return Case("spvoxelize[%s]" % ("seg" if with_seg else "atomic"), "spvoxelize", build,
                lambda spf, o: (spf.spvoxelize(o["feats"], o["idx"], o["counts"], o["seg"]),), ops,
                nondet=() if with_seg else ("out",), truth=truth)


def _devoxelize_case(with_seg):
    def build(scale=1):
        from fusiontransformer_amd import functional as spf
        n, m, _, _, idx8, w8 = _cloud(scale)
        o = dict(feats=rnd(3 + scale, m, 32), idx=dev(idx8), weights=dev(w8))
        o["seg"] = spf.devoxelize_segments(o["idx"], o["weights"], m) if with_seg else None
        return o

    def truth(o, go):
        from tests import pointvoxel_ref as PV
        return {"grad": PV.devoxelize_bwd_ref(go.cpu().numpy(), o["idx"].cpu().numpy(), o["weights"].cpu().numpy(), o["feats"].shape[0])}

    # feats: its row count IS the voxel count (corners at or beyond it are dropped); strided: copied
    ops = dict(feats=diff(but("short", "long", "strided"), reads=False), idx=Op(), weights=Op("refused"))
    return Case("spdevoxelize[%s]" % ("seg" if with_seg else "atomic"), "spdevoxelize", build,
                lambda spf, o: (spf.spdevoxelize(o["feats"], o["idx"], o["weights"], o["seg"]),), ops,
                nondet=() if with_seg else ("grad",), truth=truth)


LIFT_HW = (20, 28)


def _lift_points(scale):
    rng = np.random.default_rng(50 + scale)
    n = 65 * scale
    frame = np.sort(rng.integers(0, 2, n)).astype(np.int32)
    img_idx = np.stack([rng.integers(0, LIFT_HW[0], n), rng.integers(0, LIFT_HW[1], n)], 1).astype(np.int64)
    img_idx[n // 2] = img_idx[0]
    frame[n // 2] = frame[0]          # two points on one pixel
    return img_idx, frame


def _lift_case(with_seg):
    H, W = LIFT_HW

    def build(scale=1):
        from fusiontransformer_amd import functional as spf
        img_idx, frame = _lift_points(scale)
        o = dict(grid=rnd(5 + scale, 2, 5, 7, 8), img_idx=dev(img_idx), point_batch=dev(frame))
        o["seg"] = spf.lift_segments(o["img_idx"], o["point_batch"], 2, 5, 7, H, W) if with_seg else None
        return o

    def truth(o, go):
        from oracle import ft_oracle as O
        from tests import pointvoxel_ref as PV
        rows, cols = O.nearest_src_index(H, 5), O.nearest_src_index(W, 7)
        ii, fr = o["img_idx"].cpu().numpy(), o["point_batch"].cpu().numpy().astype(np.int64)
        cells = (fr * 5 + rows[ii[:, 0]]) * 7 + cols[ii[:, 1]]
        return {"grad": PV.segment_sum_ref(go.cpu().numpy(), cells, 2 * 5 * 7)}

    # grid: another frame count is another legal grid (long; 2 frames cannot lose 4); strided: copied
    ops = dict(grid=diff(but("long", "strided"), reads=False), img_idx=Op(), point_batch=Op())
    return Case("lift_gather[%s]" % ("seg" if with_seg else "atomic"), "lift_gather", build,
                lambda spf, o: (spf.lift_gather(o["grid"], o["img_idx"], o["point_batch"], H, W, o["seg"]),), ops,
                nondet=() if with_seg else ("grad",), truth=truth)


RESAMPLE_TO = (11, 13)


def _resample_case():
    """An upsample: up to 3 x 2 target pixels per source pixel.  The backward adds them with float atomics (ftx_resample_nearest_bwd),
    so beyond two terms per pixel it does not repeat bit for bit and is held to the scatter bound like the other atomic forms."""
    def build(scale=1):
        return dict(x=rnd(7 + scale, 2, 4, 5 * scale, 7 * scale))

    def truth(o, go):
        from oracle import ft_oracle as O
        from tests import pointvoxel_ref as PV
        b, c, ih, iw = o["x"].shape
        rows, cols = O.nearest_src_index(RESAMPLE_TO[0], ih), O.nearest_src_index(RESAMPLE_TO[1], iw)
        cells = (np.arange(b * c)[:, None, None] * ih + rows[None, :, None]) * iw + cols[None, None, :]
        return {"grad": PV.segment_sum_ref(go.cpu().numpy().reshape(-1, 1), cells.reshape(-1), b * c * ih * iw)}

    # x: any frame count is legal; strided: copied
    return Case("resample_nearest", "resample_nearest", build, lambda spf, o: (spf.resample_nearest(o["x"], RESAMPLE_TO),),
                dict(x=diff(but("short", "long", "strided"), reads=False)), nondet=("grad",), truth=truth)


# ---------------------------------------------------------------------------------------------------- sparse convolution
@functools.lru_cache(maxsize=None)
def conv_maps(scale=1):
    """The 3^3 stride-1 map and the 2^3 stride-2 map of one 2-frame cloud, built once and never modified."""
    from fusiontransformer_amd.sparse import CoordinateManager
    from tests.helpers import random_coords
    c = random_coords(np.random.default_rng(60 + scale), 1500 * scale, extent=10 + 4 * scale, batch=2)
    cm = CoordinateManager()
    cm.coords[1] = dev(c)
    return {"k3s1": cm.kernel_map(3, 1, 1), "k2s2": cm.kernel_map(2, 1, 2)}


def pairs_per_offset(km):
    return (km.koff[1:] - km.koff[:-1]).cpu().numpy()


# (name, map, transposed, ca, co)
CONV_GEOMETRIES = (("k3s1", "k3s1", False, 32, 64), ("k2s2", "k2s2", False, 32, 32), ("k2s2T", "k2s2", True, 32, 32))


def _conv_operands(geom, scale, seed):
    _, key, transposed, ca, co = geom
    km = conv_maps(scale)[key]
    rows_in, rows_out = (km.n_out, km.n_in) if transposed else (km.n_in, km.n_out)
    o = dict(feats=rnd(seed, rows_in, ca), kernel=rnd(seed + 1, km.kvol, ca, co, scale=0.1), km=km, transposed=transposed)
    return o, rows_out, co


def _tile_and_part(o):
    assert pairs_per_offset(o["km"]).max() > 128, "no kernel offset with one full pair-GEMM tile plus a partial one"


def _sparse_conv_case(geom, bf16):
    def build(scale=1):
        return _conv_operands(geom, scale, 70 + scale)[0]

    # feats, kernel: strided: copied
    ops = dict(feats=diff(but("strided")), kernel=diff(but("strided")))
    return Case("sparse_conv[%s-%s]" % (geom[0], "bf16" if bf16 else "fp32"), "sparse_conv", build,
                lambda spf, o: (spf.sparse_conv(o["feats"], o["kernel"], o["km"], o["transposed"], bf16=bf16),), ops, check=_tile_and_part)


def _bn_parameters(o, seed, c):
    o.update(gamma=rnd(seed, c, scale=0.2, shift=1.0), beta=rnd(seed + 1, c, scale=0.2),
             running_mean=rnd(seed + 2, c, scale=0.3), running_var=rnd(seed + 3, c, scale=0.1).abs() + 0.5)


def _conv_bn_case(geom, bf16, residual, relu, remask):
    def build(scale=1):
        o, rows_out, co = _conv_operands(geom, scale, 80 + scale)
        o["residual"] = rnd(82 + scale, rows_out, co) if residual else None
        _bn_parameters(o, 84 + scale, co)
        return o

    def call(spf, o):
        return (spf.conv_bn_train(o["feats"], o["kernel"], o["km"], o["transposed"], o["gamma"], o["beta"], o["running_mean"], o["running_var"],
                                  residual=o["residual"], relu=relu, bf16=bf16, remask=remask),)

    # beta is read by the backward only to recompute the ReLU mask (remask, no residual); the residual enters by addition
    ops = dict(feats=diff(but("strided")), kernel=diff(but("strided")), residual=diff(but("strided"), reads=False), gamma=diff(),
               beta=diff(reads=bool(relu and remask)), running_mean=Op(), running_var=Op())
    cid = "conv_bn_train[%s-%s-res%d-relu%d-remask%d]" % (geom[0], "bf16" if bf16 else "fp32", residual, relu, remask)
    return Case(cid, "conv_bn_train", build, call, ops, saves_output=True, fullest=residual, check=_tile_and_part)


# ---------------------------------------------------------------------------------------------------- dense rows, BatchNorm
def _linear_case(bias, bf16):
    def build(scale=1):
        return dict(x=rnd(90 + scale, 257 * scale, 32), weight=rnd(92 + scale, 20, 32, scale=0.2), bias=rnd(94 + scale, 20) if bias else None)

    # x: its row count is the output's; 3-d rows and a 21-row or 3-d weight are outside the tile kernel's shapes: the library path
    ops = dict(x=diff(but("short", "long", "extra_dim", "strided")), weight=diff(but("long", "extra_dim", "strided")), bias=diff(reads=False))
    return Case("linear[bias%d-%s]" % (bias, "bf16" if bf16 else "fp32"), "linear", build,
                lambda spf, o: (spf.linear(o["x"], o["weight"], o["bias"], bf16=bf16),), ops, fullest=bias)


def _rows_matmul_case(bf16):
    def build(scale=1):
        return dict(x=rnd(96 + scale, 257 * scale, 32), kernel=rnd(98 + scale, 32, 20, scale=0.2))

    # as linear; a 33-row or 3-d kernel runs on the library path
    ops = dict(x=diff(but("short", "long", "extra_dim", "strided")), kernel=diff(but("long", "extra_dim", "strided")))
    return Case("rows_matmul[%s]" % ("bf16" if bf16 else "fp32"), "rows_matmul", build,
                lambda spf, o: (spf.rows_matmul(o["x"], o["kernel"], bf16=bf16),), ops)


def _batch_norm_case(training, residual, relu):
    def build(scale=1):
        o = dict(x=rnd(100 + scale, 300 * scale, 32, scale=1.5, shift=0.3), residual=rnd(102 + scale, 300 * scale, 32) if residual else None)
        _bn_parameters(o, 104 + scale, 32)
        return o

    def call(spf, o):
        return (spf.batch_norm(o["x"], o["gamma"], o["beta"], o["running_mean"], o["running_var"], training, residual=o["residual"], relu=relu),)

    if training:    # remask (the default): beta recomputes the ReLU mask of a residual-free layer
        ops = dict(x=diff(but("strided")), residual=diff(but("strided"), reads=False), gamma=diff(), beta=diff(reads=bool(relu)),
                   running_mean=Op(), running_var=Op())
    else:           # eval: gamma scales dx; x and the running mean make d gamma; the running variance scales both
        ops = dict(x=diff(but("strided")), residual=diff(but("strided"), reads=False), gamma=diff(), beta=diff(reads=False),
                   running_mean=Op(), running_var=Op())
    return Case("batch_norm[%s-res%d-relu%d]" % ("train" if training else "eval", residual, relu), "batch_norm", build, call, ops,
                saves_output=True, fullest=residual)


# ---------------------------------------------------------------------------------------------------- LayerNorm, attention, ViT linears
def _ln_parameters(o, seed, c=256):
    o.update(weight=rnd(seed, c, scale=0.2, shift=1.0), bias=rnd(seed + 1, c, scale=0.2))


def _layer_norm_case():
    def build(scale=1):
        o = dict(x=rnd(110 + scale, 2 * scale, 5, 256, scale=1.3))
        _ln_parameters(o, 112 + scale)
        return o

    # x: rows of 256 floats in any number of leading dimensions (short / long change the row length); strided: copied.  bias adds
    ops = dict(x=diff(but("extra_dim", "strided"), axis=-1), weight=diff(), bias=diff(reads=False))
    return Case("layer_norm", "layer_norm", build, lambda spf, o: (spf.layer_norm(o["x"], o["weight"], o["bias"]),), ops)


ADD_LN_USES = ("both", "s", "h")


def _add_layer_norm_case(y_bias, use):
    def build(scale=1):
        o = dict(x=rnd(114 + scale, 2 * scale, 5, 256, scale=1.3), y=rnd(116 + scale, 2 * scale, 5, 256),
                 y_bias=rnd(118 + scale, 256, scale=0.3) if y_bias else None)
        _ln_parameters(o, 120 + scale)
        return o

    def call(spf, o):
        s, h = spf.add_layer_norm(o["x"], o["y"], o["weight"], o["bias"], y_bias=o["y_bias"])
        return {"both": (s, h), "s": (s,), "h": (h,)}[use]

    # the backward reads the sum s = x + y (+ y_bias), an output, not the addends
    ops = dict(x=diff(but("extra_dim", "strided"), axis=-1, reads=False), y=diff(but("extra_dim", "strided"), axis=-1, reads=False),
               y_bias=diff(reads=False), weight=diff(), bias=diff(reads=False))
    return Case("add_layer_norm[ybias%d-%s]" % (y_bias, use), "add_layer_norm", build, call, ops, saves_output=(use != "h"), fullest=y_bias)


def _attention_case(bf16):
    def build(scale=1):
        return dict(qkv=rnd(130 + scale, 1, 130 * scale, 3, 2, 64))

    # strided: copied; short / long change the head dimension, which must be 64
    return Case("attention[%s]" % ("bf16" if bf16 else "fp32"), "attention", build,
                lambda spf, o: (spf.attention(o["qkv"], 0.125, tiling=(0, 0), bf16=bf16),), dict(qkv=diff(but("strided"), axis=-1)),
                saves_output=True)


# x and the weights of the ViT linears: every variation fails vit_linear_supported (or is a layout the node copies), so the library
# path answers it; the biases are read by the kernel's epilogue whatever the dispatch saw
_ROUTED = frozenset()


def _vit_linear_case(mode, b):
    def build(scale=1):
        return dict(x=rnd(140 + scale, 1, 33 * scale, 64), w=rnd(142 + scale, 128, 64, scale=0.1), b=rnd(144 + scale, 128) if b else None)

    ops = dict(x=diff(_ROUTED), w=diff(_ROUTED), b=diff(reads=False))
    return Case("vit_linear[%s-b%d]" % (mode, b), "vit_linear", build, lambda spf, o: (spf.vit_linear(o["x"], o["w"], o["b"], mode=mode),), ops,
                fullest=b)


def _vit_mlp_case(mode, b2):
    def build(scale=1):
        return dict(x=rnd(150 + scale, 1, 33 * scale, 64), w1=rnd(152 + scale, 128, 64, scale=0.1), b1=rnd(154 + scale, 128, scale=0.5),
                    w2=rnd(156 + scale, 64, 128, scale=0.1), b2=rnd(158 + scale, 64) if b2 else None)

    # b1 is inside the saved pre-activation
    ops = dict(x=diff(_ROUTED), w1=diff(_ROUTED), b1=diff(reads=False), w2=diff(_ROUTED), b2=diff(reads=False))
    return Case("vit_mlp[%s-b2%d]" % (mode, b2), "vit_mlp", build,
                lambda spf, o: (spf.vit_mlp(o["x"], o["w1"], o["b1"], o["w2"], o["b2"], mode=mode),), ops, fullest=b2)


# ---------------------------------------------------------------------------------------------------- image entries
def _sample_down_case():
    def build(scale=1):
        o = dict(img=rnd(160 + scale, 2, 3, 20 * scale, 28 * scale), conv_w=rnd(162 + scale, 3, 3, 1, 1, scale=0.6), conv_b=rnd(164 + scale, 3, scale=0.3))
        _bn_parameters(o, 166 + scale, 3)
        return o

    def call(spf, o):
        return (spf.sample_down(o["img"], o["conv_w"], o["conv_b"], o["gamma"], o["beta"], o["running_mean"], o["running_var"], 0.1, 1e-5, True,
                                (8, 12)),)

    # img: strided: copied; long makes a 4-channel image (3 channels cannot lose 4).  conv_w: any 9 floats, copied
    ops = dict(img=Op("refused", but("short", "strided"), axis=1), conv_w=diff(but("short", "extra_dim", "strided")), conv_b=diff(), gamma=diff(),
               beta=diff(reads=False), running_mean=Op(), running_var=Op())
    return Case("sample_down", "sample_down", build, call, ops)


def _affine_sample_case():
    from tests.test_stn_gpu import DENSE_FWD
    shape, size, kind, _ = DENSE_FWD[1]

    def build(scale=1):
        from tests import stn_ref
        b, c, ih, iw = shape
        return dict(src=rnd(170 + scale, b, c, ih * scale, iw * scale), theta=stn_ref.theta_case(kind, b, np.random.default_rng(scale)).cuda())

    # src: any strides that do not alias
    ops = dict(src=Op("refused", but("strided")), theta=diff())
    return Case("affine_sample", "affine_sample", build, lambda spf, o: (spf.affine_sample(o["src"], o["theta"], size),), ops)


def _affine_lift_case():
    from tests.test_stn_gpu import POINTS
    shape, size, n, kind, _, empty = POINTS[1]

    def build(scale=1):
        from tests import stn_ref
        from tests.test_stn_gpu import points
        b, c, ih, iw = shape
        theta = stn_ref.theta_case(kind, b, np.random.default_rng(11 + scale))
        idx, frame = points(b, size[0], size[1], n * scale, 5, theta, ih * scale, iw * scale, 1e-3, empty_frame=empty)
        return dict(src=rnd(172 + scale, b, c, ih * scale, iw * scale), theta=theta.cuda(), img_idx=idx.cuda(), point_batch=frame.cuda())

    ops = dict(src=diff(but("strided")), theta=diff(), img_idx=Op(), point_batch=Op())
    return Case("affine_lift", "affine_lift", build,
                lambda spf, o: (spf.affine_lift(o["src"], o["theta"], o["img_idx"], o["point_batch"], size[0], size[1]),), ops)


def _loc_case(shape, mean):
    def build(scale=1):
        from tests import loc_ref
        b, c, ih, iw, k, co = shape
        x, w, bias = loc_ref.inputs((b, c, ih * scale, iw * scale, k, co), seed=2 + scale)
        return dict(x=x.cuda(), weight=w.cuda(), bias=bias.cuda())

    # x: any strides that do not alias, any frame count up to 128
    ops = dict(x=diff(but("long", "strided")), weight=diff(), bias=diff(reads=False))
    return Case("loc_conv_pool_relu[k%d-mean%d]" % (shape[4], mean), "loc_conv_pool_relu", build,
                lambda spf, o: (spf.loc_conv_pool_relu(o["x"], o["weight"], o["bias"], mean=mean),), ops, saves_output=True)


# ---------------------------------------------------------------------------------------------------- losses
def _loss_inputs(scale, dual):
    from tests import loss_metric_ref as LR
    rng = np.random.default_rng(180 + scale)
    n, c = 257 * scale, 20
    lg = LR.make_logits(rng, n, c, 1.0, dual=dual, ties=8)
    cw = rng.uniform(0.5, 2.0, c).astype(np.float32)
    return lg, LR.make_labels(rng, n, c, "zero30"), cw, c


def _fusion_loss_case(dual):
    from tests.loss_metric_ref import NAMES

    def build(scale=1):
        lg, label, cw, c = _loss_inputs(scale, dual)
        o = {k: (dev(lg[k]) if k in lg else None) for k in NAMES}
        o.update(label=dev(label), class_weights=dev(cw), conf3d=torch.zeros((c, c), dtype=I64, device="cuda"),
                 conf2d=torch.zeros((c, c), dtype=I64, device="cuda"))
        return o

    def call(spf, o):
        l2d, l3d = spf.fusion_loss({k: o[k] for k in NAMES}, o["label"], o["class_weights"], 0.1, dual, conf3d=o["conf3d"], conf2d=o["conf2d"])
        return (l2d, l3d) if dual else (l2d + l3d,)      # one head: the two losses share their logits, backward runs on the sum

    # the gradients are made in the forward.  label: fusion_loss converts it to int64 and copies it
    ops = {k: diff(but("strided"), reads=False) for k in (NAMES if dual else NAMES[:2])}
    ops.update(label=Op(bad=but("float64", "strided")), class_weights=Op(), conf3d=Op(), conf2d=Op())
    return Case("fusion_loss[dual%d]" % dual, "fusion_loss", build, call, ops, fullest=dual)


def _seg_loss_case():
    def build(scale=1):
        lg, label, cw, c = _loss_inputs(scale, False)
        return dict(logit=dev(lg["lidar_seg_logit"]), label=dev(label), class_weights=dev(cw), conf=torch.zeros((c, c), dtype=I64, device="cuda"))

    ops = dict(logit=diff(but("strided"), reads=False), label=Op(bad=but("strided")), class_weights=Op(), conf=Op())
    return Case("seg_loss", "seg_loss", build, lambda spf, o: (spf.seg_loss(o["logit"], o["label"], o["class_weights"], conf=o["conf"]),), ops)


def _all_cases():
    from tests import loc_ref
    tf = (False, True)
    cases = [_voxelize_case(True), _voxelize_case(False), _devoxelize_case(True), _devoxelize_case(False)]
    cases += [_sparse_conv_case(g, bf16) for g in CONV_GEOMETRIES for bf16 in tf]
    cases += [_conv_bn_case(g, *opt) for g in CONV_GEOMETRIES for opt in itertools.product(tf, repeat=4)]
    cases += [_linear_case(bias, bf16) for bias in tf for bf16 in tf] + [_rows_matmul_case(bf16) for bf16 in tf]
    cases += [_batch_norm_case(*opt) for opt in itertools.product((True, False), tf, tf)]
    cases += [_layer_norm_case()] + [_add_layer_norm_case(yb, use) for yb in tf for use in ADD_LN_USES]
    cases += [_attention_case(bf16) for bf16 in tf]
    cases += [_vit_linear_case(mode, b) for mode in ("bf16", "split") for b in tf]
    cases += [_vit_mlp_case(mode, b2) for mode in ("bf16", "split") for b2 in tf]
    cases += [_sample_down_case(), _lift_case(True), _lift_case(False), _resample_case(), _affine_sample_case(), _affine_lift_case()]
    cases += [_loc_case(loc_ref.SMALL[i][0], mean) for i in (1, 4) for mean in tf]     # one case per layer of the localisation net
    cases += [_fusion_loss_case(False), _fusion_loss_case(True), _seg_loss_case()]
    assert len({c.id for c in cases}) == len(cases)
    return cases


CASES = _all_cases()
