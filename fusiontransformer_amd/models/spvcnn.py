"""SPVCNN sparse-voxel U-Net on libftx.

Mirror of the reference's FusionTransformer/models/spvcnn.py:22-233: same
class names, constructor arguments, attribute names (hence the same
state_dict keys: `stem.0.kernel`, `stage1.1.net.1.running_mean`, ...) and the
same wiring.  `spnn.Conv3d / BatchNorm / ReLU` are the classes below; at run
time each Conv->BN(->+residual)->ReLU chain is executed as one sparse-conv
launch plus one fused BN/residual/ReLU pass instead of four separate ops."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as spf
from ..sparse import PendingIndex, PointTensor, PreparedIndex, SparseTensor, cat, drain, index_stream as _index_stream
from .utils import initial_voxelize_steps, point_index, point_to_voxel, voxel_index, voxel_to_point

__all__ = ["SPVCNN", "Conv3d", "BatchNorm", "ReLU"]
_U64 = (1 << 64) - 1


class Conv3d(nn.Module):
    """spnn.Conv3d (torchsparse v1.1.0): no bias, kernel (K^3, inc, outc), (inc, outc) when K=1."""

    def __init__(self, inc, outc, kernel_size=3, stride=1, dilation=1, bias=False, transpose=False):
        super().__init__()
        if bias:
            raise NotImplementedError("the reference never enables the conv bias")
        if dilation != 1:
            raise NotImplementedError("dilation != 1 is not used by the reference (spvcnn.py passes 1 everywhere)")
        self.in_channels, self.out_channels = inc, outc
        self.kernel_size, self.stride, self.dilation, self.t = kernel_size, stride, dilation, transpose
        self.k = kernel_size ** 3
        self.kernel = nn.Parameter(torch.zeros(self.k, inc, outc)) if self.k > 1 else nn.Parameter(torch.zeros(inc, outc))
        self.init_weight()

    def init_weight(self):
        std = 1.0 / math.sqrt(self.out_channels if self.t else self.in_channels * self.k)
        self.kernel.data.uniform_(-std, std)

    def forward(self, x: SparseTensor) -> SparseTensor:
        if self.kernel_size == 1 and self.stride == 1:
            out = x.derive(spf.rows_matmul(x.F, self.kernel, operands=operand_mode(self)))
        else:
            km, coords, stride = _conv_map(self, x)
            out = x.derive(spf.sparse_conv(x.F, self.kernel, km, self.t, operands=operand_mode(self)), coords, stride)
        out.check()
        return out


def operand_mode(module):
    """SPVCNN.set_bf16 / set_split as they stand on a Conv3d or a point-branch nn.Linear: "fp32", "bf16" or "split", the `operands=`
    of the functional layer (functional.OPERANDS numbers them for the executors' layer records).  The one reader of `ftx_bf16` and
    `ftx_split` for the LiDAR branch."""
    if getattr(module, "ftx_split", False):
        return "split"
    return "bf16" if getattr(module, "ftx_bf16", False) else "fp32"


def bf16_operands(module):
    """Whether the module's GEMM operands are rounded to bf16 (SPVCNN.set_bf16), through operand_mode."""
    return operand_mode(module) == "bf16"


def step_counter(bn):
    """The `num_batches_tracked` a BatchNorm (any nn.BatchNorm*) bumps itself in this forward, or None: not in training mode, no
    running statistics, or _fusion_common.bump_batchnorm_counters counts for it (it marks the module `_nbt_external`)."""
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None and not getattr(bn, "_nbt_external", False):
        return bn.num_batches_tracked
    return None


def bump_step_counter(bn):
    counter = step_counter(bn)
    if counter is not None:
        counter.add_(1)


class BatchNorm(nn.BatchNorm1d):
    """spnn.BatchNorm: BatchNorm1d over the voxel rows; `fused` adds the residual and ReLU in the same pass."""

    def fused(self, feats, residual=None, relu=False):
        bump_step_counter(self)
        return spf.batch_norm(feats, self.weight, self.bias, self.running_mean, self.running_var, self.training,
                              self.momentum, self.eps, residual=residual, relu=relu)

    def forward(self, x):
        if isinstance(x, SparseTensor):
            return x.derive(self.fused(x.F))
        return self.fused(x)


class ReLU(nn.ReLU):
    """spnn.ReLU."""

    def forward(self, x):
        if isinstance(x, SparseTensor):
            return x.derive(F.relu(x.F))
        return F.relu(x)


def _conv_map(conv, x):
    """(kernel map, output coordinates, output stride) of a k > 1 Conv3d on x."""
    ks, s = conv.kernel_size, conv.stride
    if not conv.t:
        km = x.cm.kernel_map(ks, x.s, s)
        return km, km.out_coords, x.s * s
    original_stride = x.s // s
    km = x.cm.kernel_maps.get((ks, original_stride, s))
    if km is None:
        raise RuntimeError("transposed Conv3d needs the kernel map of the paired strided Conv3d")
    return km, x.cm.coords[original_stride], original_stride


def _conv_bn(conv, bn, x, residual=None, relu=True):
    """Conv3d -> BatchNorm (-> + residual) (-> ReLU).  In training a k>1 convolution and its BatchNorm run as one autograd node whose
    reduce pass also produces the batch statistics (functional.conv_bn_train); eval and 1x1x1 layers run the two separately."""
    fused_eval = getattr(conv, "ftx_native_eval", False) and not bn.training and not torch.is_grad_enabled()
    if (conv.kernel_size == 1 and conv.stride == 1) or not x.F.is_cuda or not (bn.training or fused_eval):
        y = conv(x)
        return y.derive(bn.fused(y.F, residual=residual, relu=relu))
    km, coords, stride = _conv_map(conv, x)
    if bn.training:
        bump_step_counter(bn)
        feats = spf.conv_bn_train(x.F, conv.kernel, km, conv.t, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                                  residual=residual, relu=relu, operands=operand_mode(conv))
    else:
        # SPVCNN.set_native_eval where the executor does not run (a layer option it refuses): the reduce carries the eval BatchNorm
        feats = spf.conv_bn_eval(x.F, conv.kernel, km, conv.t, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, residual=residual,
                                 relu=relu, operands=operand_mode(conv))
    out = x.derive(feats, coords, stride)
    out.check()
    return out


def _addend_steps(f, token):
    """A fusion addend `f` (the image features, or the call that waits for them: _fusion_common._Lazy.get) after yielding `token`
    where they are first touched; None without a yield where nothing is fused."""
    if f is None:
        return None
    yield token
    return f() if callable(f) else f


def _linear_bn_relu(seq, feats):
    """nn.Sequential(Linear, BatchNorm1d, ReLU) on point rows (spvcnn.py:164-180)."""
    return seq[1].fused(spf.linear(feats, seq[0].weight, seq[0].bias, operands=operand_mode(seq[0])), relu=True)


class BasicConvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(Conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride), BatchNorm(outc), ReLU(True))

    def forward(self, x):
        return _conv_bn(self.net[0], self.net[1], x, relu=True)


class BasicDeconvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1):
        super().__init__()
        self.net = nn.Sequential(Conv3d(inc, outc, kernel_size=ks, stride=stride, transpose=True), BatchNorm(outc), ReLU(True))

    def forward(self, x):
        return _conv_bn(self.net[0], self.net[1], x, relu=True)


class ResidualBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(
            Conv3d(inc, outc, kernel_size=ks, dilation=dilation, stride=stride), BatchNorm(outc), ReLU(True),
            Conv3d(outc, outc, kernel_size=ks, dilation=dilation, stride=1), BatchNorm(outc))
        self.downsample = nn.Sequential() if (inc == outc and stride == 1) else nn.Sequential(
            Conv3d(inc, outc, kernel_size=1, dilation=1, stride=stride), BatchNorm(outc))
        self.relu = ReLU(True)

    def forward(self, x):
        # relu(net(x) + downsample(x)), spvcnn.py:77-79; the add and ReLU ride on the last BN pass
        if len(self.downsample) == 0:
            shortcut = x.F
        else:
            shortcut = _conv_bn(self.downsample[0], self.downsample[1], x, relu=False).F
        h = _conv_bn(self.net[0], self.net[1], x, relu=True)
        return _conv_bn(self.net[3], self.net[4], h, residual=shortcut, relu=True)


class SPVCNN(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        cr = kwargs.get("cr", 1.0)
        cs = [32, 32, 64, 128, 256, 256, 128, 96, 96]
        cs = [int(cr * x) for x in cs]
        self.cs = cs
        if "pres" in kwargs and "vres" in kwargs:
            self.pres = kwargs["pres"]
            self.vres = kwargs["vres"]
        else:
            self.pres = 1
            self.vres = self.pres

        self.stem = nn.Sequential(
            Conv3d(4, cs[0], kernel_size=3, stride=1), BatchNorm(cs[0]), ReLU(True),
            Conv3d(cs[0], cs[0], kernel_size=3, stride=1), BatchNorm(cs[0]), ReLU(True))

        def stage(i, o):
            return nn.Sequential(BasicConvolutionBlock(i, i, ks=2, stride=2, dilation=1),
                                 ResidualBlock(i, o, ks=3, stride=1, dilation=1),
                                 ResidualBlock(o, o, ks=3, stride=1, dilation=1))

        self.stage1 = stage(cs[0], cs[1])
        self.stage2 = stage(cs[1], cs[2])
        self.stage3 = stage(cs[2], cs[3])
        self.stage4 = stage(cs[3], cs[4])

        def up(i, o, skip):
            return nn.ModuleList([BasicDeconvolutionBlock(i, o, ks=2, stride=2),
                                  nn.Sequential(ResidualBlock(o + skip, o, ks=3, stride=1, dilation=1),
                                                ResidualBlock(o, o, ks=3, stride=1, dilation=1))])

        self.up1 = up(cs[4], cs[5], cs[3])
        self.up2 = up(cs[5], cs[6], cs[2])
        self.up3 = up(cs[6], cs[7], cs[1])
        self.up4 = up(cs[7], cs[8], cs[0])

        self.point_transforms = nn.ModuleList([
            nn.Sequential(nn.Linear(cs[0], cs[4]), BatchNorm(cs[4]), nn.ReLU(True)),
            nn.Sequential(nn.Linear(cs[4], cs[6]), BatchNorm(cs[6]), nn.ReLU(True)),
            nn.Sequential(nn.Linear(cs[6], cs[8]), BatchNorm(cs[8]), nn.ReLU(True)),
        ])
        self.weight_initialization()
        self.dropout = nn.Dropout(0.3, True)
        # cfg.MODEL.lidar_bf16: the LiDAR branch on bf16-operand kernels, see set_bf16
        self.lidar_bf16 = bool(kwargs.get("lidar_bf16", False))
        # cfg.MODEL.lidar_split: the LiDAR branch fp32-accurate on the bf16 MFMA (three-piece operand split), see set_split
        self.lidar_split = bool(kwargs.get("lidar_split", False))
        if self.lidar_bf16 and self.lidar_split:
            raise ValueError("lidar_bf16 and lidar_split are two operand modes of the same GEMMs: set at most one")
        self.set_bf16(self.lidar_bf16)
        self.set_split(self.lidar_split)
        # cfg.MODEL.lidar_native_eval: the eval-mode, no-gradient forward through the native executor, see set_native_eval
        self._native = None
        self.set_native_eval(bool(kwargs.get("lidar_native_eval", False)))
        # cfg.MODEL.lidar_native_index: the coordinate structures of a batch through the native index build, see set_native_index
        self.set_native_index(bool(kwargs.get("lidar_native_index", False)))
        # cfg.MODEL.lidar_native_train: the training forward and backward through the native executor, see set_native_train
        self._native_tr = None
        self.set_native_train(bool(kwargs.get("lidar_native_train", False)))
        # cfg.MODEL.lidar_native_dropout: Dropout from the library's counter-based stream, see set_native_dropout.  Plain attributes, not
        # buffers: the state_dict keys stay the reference's
        self._drop_seed, self._drop_forwards, self._drop_last = 0, 0, None
        self.set_native_dropout(bool(kwargs.get("lidar_native_dropout", False)))
        # optional injected keep-masks {'y1': (N4,C), 'y3': (N2,C)} so a train-mode run can be
        # compared with the oracle (Dropout RNG streams differ between CPU and GPU)
        self.dropout_masks = None

    # the point-branch Linears of the fusion models (early / middle_fusion.py) that set_bf16 switches with the U-Net
    _FUSION_TRANSFORMS = ("early_fusion_transform", "middle_fusion_transform")

    def set_bf16(self, on=True):
        """bf16-operand mode of the LiDAR branch: every Conv3d (sparse convolutions and the 1x1x1 ones) and the nn.Linear of
        point_transforms and of the early / middle fusion transform run their forward, data gradient and weight gradient with the GEMM
        operands rounded to bf16 and fp32 accumulation (include/ftx.h).  BatchNorm, the reduce over offsets and all storage stay fp32.
        The segmentation heads (`linear`, `linear2`) stay fp32.  Subclasses that add a fusion transform call this again after adding it."""
        if on and getattr(self, "lidar_split", False):
            raise ValueError("lidar_bf16 and lidar_split are two operand modes of the same GEMMs: set at most one")
        self.lidar_bf16 = bool(on)
        for m in self._operand_modules():
            m.ftx_bf16 = bool(on)
        return self

    def set_split(self, on=True):
        """fp32-accurate mode of the LiDAR branch on the bf16 matrix cores: exactly the modules set_bf16 flags -- every Conv3d and the
        nn.Linear of point_transforms and of the early / middle fusion transform, no head -- run their forward, data gradient and weight
        gradient with every fp32 GEMM operand split into three bf16 pieces and six piece products summed in fp32 (include/ftx.h:
        ftx_spconv_pairs_gemm_split).  Results are fp32-class: the model meets the gates of the default path, not those of set_bf16.
        The thin forward layers that the default path sends to the output-stationary kernel keep it (it is exact fp32).  Not both
        this and set_bf16: ValueError.  Subclasses that add a fusion transform call this again after adding it."""
        if on and getattr(self, "lidar_bf16", False):
            raise ValueError("lidar_bf16 and lidar_split are two operand modes of the same GEMMs: set at most one")
        self.lidar_split = bool(on)
        for m in self._operand_modules():
            m.ftx_split = bool(on)
        return self

    def _operand_modules(self):
        """The modules whose GEMM operands set_bf16 / set_split switch: every Conv3d and the first module of each point / fusion transform."""
        convs = [m for m in self.modules() if isinstance(m, Conv3d)]
        seqs = list(self.point_transforms) + [getattr(self, n) for n in self._FUSION_TRANSFORMS if hasattr(self, n)]
        return convs + [seq[0] for seq in seqs]

    def set_native_eval(self, on=True):
        """Opt-in native executor for the eval-mode forward (include/ftx.h: ftx_spvcnn_eval).  With it on, a forward in eval mode, with
        gradients disabled and features on the GPU, builds the batch's coordinate structures as before and then issues the whole network
        -- first convolution of the stem to z3.F -- as one library call per segment (stem / encoder / decoder) over an arena this module
        owns, instead of a few hundred calls through Python; pair-list convolutions run the reduce that carries the eval BatchNorm
        (ftx_spconv_reduce_bn_eval).  The results are bit-identical to the switch being off.  In training mode, with gradients enabled,
        on CPU tensors or for a layer option the executor refuses, the existing path runs exactly as with the switch off."""
        self.lidar_native_eval = bool(on)
        for m in self.modules():
            if isinstance(m, Conv3d):
                m.ftx_native_eval = bool(on)
        if not on:
            self._native = None
        return self

    def set_native_index(self, on=True):
        """Opt-in native index build (include/ftx.h: ftx_spvcnn_index_levels / _maps / _pairs).  With it on, the coordinate structures of a
        batch on the GPU -- level coordinates, hash tables, the nine kernel maps, the point <-> voxel indices of strides 1, 16 and 4 and
        the voxelised input features -- come from three library calls with the same two host reads, instead of ~110 launches through
        Python; with gradients enabled also the sorted segments of the devoxelise backward.  Every array is bit-identical to the per-op
        build, in eval and in training, and independent of set_native_eval.  CPU tensors and batches the library refuses take the
        existing path."""
        self.lidar_native_index = bool(on)
        return self

    def set_native_train(self, on=True):
        """Opt-in native training executor (include/ftx.h: ftx_spvcnn_train_fwd / _bwd).  With it on, a forward in training mode, with
        gradients enabled and features on the GPU, builds the batch's coordinate structures as before and then runs the network -- first
        convolution of the stem to z3.F -- as five segments, each ONE autograd node whose forward and backward are one library call
        (stem | encoder | z1 -> y1 | up1, up2, z2 -> y3 | up3, up4, z3: a segment ends where a Dropout follows, which stays torch's),
        over one arena per forward instead of ~200 nodes through Python; with set_native_dropout also on, Dropout is an op of the program
        and the segments are three (stem | encoder | decoder).  Same kernels in the same order: logits, every gradient and
        every running statistic are bit-identical to the switch being off.  Independent of set_native_eval, set_native_index and
        set_bf16.  In eval mode, without gradients, on CPU tensors, with a frozen parameter, for a module tree the emitter refuses or
        a batch the library refuses, the existing path runs exactly as with the switch off."""
        self.lidar_native_train = bool(on)
        if not on:
            self._native_tr = None
        return self

    def set_native_dropout(self, on=True, seed=None):
        """Opt-in Dropout from the library's counter-based stream (include/ftx.h: ftx_dropout) instead of torch's.  With it on, a forward in
        training mode with gradients enabled draws both Dropouts (y1: site 0, y3: site 1, p of self.dropout) as functional.dropout with
        call = call_base + site, where call_base = 2 * (training forwards so far that reached Dropout): the masks are a pure function of
        (seed, call, element), identical on every device and torch version, recomputed in the backward, and last_dropout_masks() states
        them after the fact.  `seed`: None takes torch.initial_seed() as it is NOW, masked to 64 bits.  With set_native_train also on,
        Dropout is an op of the training program, which then runs in three segments (stem | encoder | decoder) as the eval executor
        does; the two paths agree bit for bit for equal dropout_state().  Injected `dropout_masks` and this switch exclude each other
        (ValueError in the forward).  Eval mode and forwards without gradients are unchanged; independent of every other switch.  Not
        for a forward captured into a HIP graph: seed and call go to the kernel by value, so a replay would repeat its masks."""
        self.lidar_native_dropout = bool(on)
        if on:
            self._drop_seed = (torch.initial_seed() if seed is None else int(seed)) & _U64
        self._native_tr = None        # the training program is another one: emitted again at the next forward
        return self

    def dropout_state(self):
        """{seed, forwards} of the native Dropout: what set_dropout_state takes to make the next training forward draw the same masks."""
        return {"seed": self._drop_seed, "forwards": self._drop_forwards}

    def set_dropout_state(self, state):
        seed, forwards = int(state["seed"]), int(state["forwards"])
        if not 0 <= seed <= _U64 or forwards < 0:
            raise ValueError("set_dropout_state: seed in [0, 2^64) and forwards >= 0 expected")
        self._drop_seed, self._drop_forwards = seed, forwards
        return self

    def last_dropout_masks(self):
        """{'y1': (N4, C) bool, 'y3': (N2, C) bool}: the keep-masks the most recent native-Dropout training forward applied, recomputed
        from its (seed, call_base) and the row counts of last_index -- what an oracle takes as `dropout_masks`."""
        if self._drop_last is None:
            raise RuntimeError("last_dropout_masks: no training forward has drawn a native Dropout mask yet")
        seed, base = self._drop_last
        x4, x2 = self.last_index["x4"].C, self.last_index["x2"].C
        return {"y1": spf.dropout_mask((x4.shape[0], self.cs[4]), self.dropout.p, seed, base & _U64, device=x4.device),
                "y3": spf.dropout_mask((x2.shape[0], self.cs[6]), self.dropout.p, seed, (base + 1) & _U64, device=x2.device)}

    def _native_dropout_here(self):
        """Whether this forward draws its Dropout from the library's stream (see set_native_dropout)."""
        if not (self.lidar_native_dropout and self.training and torch.is_grad_enabled()):
            return False
        if self.dropout_masks is not None:
            raise ValueError("SPVCNN: dropout_masks are injected while set_native_dropout is on: it is one or the other")
        return True

    def _take_call_base(self):
        """call_base of this training forward (its two sites draw call_base and call_base + 1); counts the forward."""
        base = 2 * self._drop_forwards
        self._drop_forwards += 1
        self._drop_last = (self._drop_seed, base)
        return base

    def _native_trainer(self, x):
        """The training executor when this forward is one it runs (see set_native_train), else None."""
        if not self.lidar_native_train or not self.training or not torch.is_grad_enabled() or not torch.is_tensor(x.F) or not x.F.is_cuda \
                or x.F.requires_grad:
            return None
        if self._native_tr is None:
            from .. import native_train
            try:
                self._native_tr = native_train.NativeTrain(self, native_dropout=self.lidar_native_dropout)
            except native_train.Unsupported:
                self._native_tr = False
        if not self._native_tr or not self._native_tr.trainable():
            return None
        return self._native_tr

    def _native_train_steps(self, run, z, x0, fuse_early, fuse_middle):
        """_backbone_steps from "voxelized" on through the training executor: one autograd node per segment, Dropout between them --
        or, with set_native_dropout, inside the third and last (run.rng holds the pair its two ops draw with)."""
        z0 = run.segment(0, x0.F)
        early = yield from _addend_steps(fuse_early, "need_early")
        yield "stem"
        z1 = run.segment(1, z0, early)
        middle = yield from _addend_steps(fuse_middle, "need_middle")
        yield "stage4"
        if run.rng is not None:
            feats = run.segment(2, z1, middle)
        else:
            y1 = self._drop(run.segment(2, z1, middle), "y1")
            y3 = self._drop(run.segment(3, y1), "y3")
            yield "up2"
            feats = run.segment(4, y3)
        yield "up4"
        self._keep_index(z, x0)
        return feats

    def _native_executor(self, x):
        """The executor when this forward is one it runs (see set_native_eval), else None."""
        if not self.lidar_native_eval or self.training or torch.is_grad_enabled() or not x.F.is_cuda:
            return None
        if self._native is None:
            from .. import native_eval
            try:
                self._native = native_eval.NativeEval(self)
            except native_eval.Unsupported:
                self._native = False
        return self._native or None

    def _native_steps(self, ex, x, fuse_early, fuse_middle):
        """_backbone_steps through the executor: the same index build, then one call per segment; "need_early" / "need_middle" are
        yielded where the image features are first touched, the stage tokens are the segment boundaries."""
        z, x0 = yield from self._batch_index_steps(x, ahead=True)
        yield "voxelized"
        run = ex.begin(z, x0)
        run.segments(0, 0)
        early = yield from _addend_steps(fuse_early, "need_early")
        yield "stem"
        run.segments(1, 1, add_early=early)
        middle = yield from _addend_steps(fuse_middle, "need_middle")
        yield "stage4"
        feats = run.segments(2, 2, add_middle=middle)
        yield "up4"
        self._keep_index(z, x0)
        return feats

    def weight_initialization(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _drop(self, feats, name):
        if self._native_dropout_here():
            site = ("y1", "y3").index(name)
            if site == 0:
                self._take_call_base()
            seed, base = self._drop_last
            return spf.dropout(feats, self.dropout.p, seed, (base + site) & _U64, inplace=True)
        if self.dropout_masks is not None and self.training:
            return feats * self.dropout_masks[name] / (1.0 - 0.3)
        return self.dropout(feats)

    def _stem(self, x):
        x = _conv_bn(self.stem[0], self.stem[1], x, relu=True)
        return _conv_bn(self.stem[3], self.stem[4], x, relu=True)

    def _backbone(self, x, fuse_early=None, fuse_middle=None):
        """spvcnn.py:191-233 with the fusion adds of early_fusion.py:39 / middle_fusion.py:48."""
        return drain(self._backbone_steps(x, fuse_early, fuse_middle))

    def _backbone_steps(self, x, fuse_early=None, fuse_middle=None):
        """The same forward as a generator that yields at stage boundaries, so a scheduler can interleave
        the issue of this branch with the image branch (see _fusion_common.run_fusion).  It yields
        "need_early" / "need_middle" right before it touches the image features."""
        ex = self._native_executor(x)
        if ex is not None:
            return (yield from self._native_steps(ex, x, fuse_early, fuse_middle))
        trainer = self._native_trainer(x)
        z, x0 = yield from self._batch_index_steps(x, ahead=trainer is not None)
        yield "voxelized"
        if trainer is not None:
            from ..native_train import Refused
            rng = (self._drop_seed, (2 * self._drop_forwards) & _U64) if self._native_dropout_here() else None
            try:
                run = trainer.begin(z, x0) if rng is None else trainer.begin(z, x0, rng=rng)
            except Refused:
                run = None        # refused before anything was launched: the per-op path below
            if run is not None:
                if rng is not None:
                    self._take_call_base()      # what `rng` holds: counted once the executor has taken the forward
                return (yield from self._native_train_steps(run, z, x0, fuse_early, fuse_middle))
        x0 = self._stem(x0)
        z0 = voxel_to_point(x0, z, nearest=False)
        early = yield from _addend_steps(fuse_early, "need_early")
        if early is not None:
            z0.F = z0.F + early
        yield "stem"

        x1 = point_to_voxel(x0, z0)
        x1 = self.stage1(x1)
        yield "stage1"
        x2 = self.stage2(x1)
        yield "stage2"
        x3 = self.stage3(x2)
        yield "stage3"
        x4 = self.stage4(x3)
        z1 = voxel_to_point(x4, z0)
        z1.F = z1.F + _linear_bn_relu(self.point_transforms[0], z0.F)
        middle = yield from _addend_steps(fuse_middle, "need_middle")
        if middle is not None:
            z1.F = z1.F + middle
        yield "stage4"

        y1 = point_to_voxel(x4, z1)
        y1.F = self._drop(y1.F, "y1")
        y1 = self.up1[0](y1)
        y1 = cat([y1, x3])
        y1 = self.up1[1](y1)
        yield "up1"

        y2 = self.up2[0](y1)
        y2 = cat([y2, x2])
        y2 = self.up2[1](y2)
        z2 = voxel_to_point(y2, z1)
        z2.F = z2.F + _linear_bn_relu(self.point_transforms[1], z1.F)
        yield "up2"

        y3 = point_to_voxel(y2, z2)
        y3.F = self._drop(y3.F, "y3")
        y3 = self.up3[0](y3)
        y3 = cat([y3, x1])
        y3 = self.up3[1](y3)
        yield "up3"

        y4 = self.up4[0](y3)
        y4 = cat([y4, x0])
        y4 = self.up4[1](y4)
        yield "up4"
        z3 = voxel_to_point(y4, z2)
        z3.F = z3.F + _linear_bn_relu(self.point_transforms[2], z2.F)
        self.last_index = dict(x0=x0, x1=x1, x2=x2, x3=x3, x4=x4, z=z)
        return z3.F

    def _batch_index_steps(self, x, ahead):
        """(z, x0) of batch `x` at the start of a forward: what prepare() hung on it, else built here (_index_steps)."""
        prepared = getattr(x, "prepared", None)
        if isinstance(prepared, PendingIndex):
            # started ahead of this forward (prepare(wait=False)) and parked at a host read: finish it here, on its own stream
            while prepared.done is None:
                yield "sync"
                prepared.step()
            prepared = prepared.done
        if prepared is None:
            return (yield from self._index_steps(x, ahead=ahead))
        # built ahead of this forward on the index stream (prepare()): wait for it, and tell the allocator this stream uses it
        z, x0 = prepared.take(torch.cuda.current_stream() if x.F.is_cuda else None)
        x.prepared = None
        return z, x0

    def _keep_index(self, z, x0):
        """`last_index` of a forward through an executor: the levels' coordinates without features (those stay in the arena)."""
        cm = x0.cm
        levels = {"x%d" % l: SparseTensor(None, cm.coords[s], s) for l, s in enumerate((1, 2, 4, 8, 16)) if l}
        self.last_index = dict(x0=x0, z=z, **levels)

    def _index_steps(self, x, ahead=False):
        """Everything of a batch that depends on its coordinates only: the voxelisation of the points, the voxel hash, the
        coordinates and kernel maps of the five U-Net levels and (ahead=True) the point <-> voxel index structures of the strides
        the network visits.  Each data-dependent size is read back after a "sync" yield (two per batch: all level sizes, then all
        pair counts), so a scheduler can issue image-branch work instead of waiting for it."""
        if self.lidar_native_index and torch.is_tensor(x.F) and x.F.is_cuda:
            from .. import native_index
            try:
                return (yield from native_index.index_steps(x, self.pres, self.vres))
            except native_index.Refused:
                pass          # refused before anything was launched: the per-op build below
        coords = x.C
        if coords.dtype != torch.float32:
            coords = coords.float()
        z = PointTensor(x.F, coords.contiguous())
        x0 = yield from initial_voxelize_steps(z, self.pres, self.vres, levels=(1, 2, 4, 8, 16))
        yield from x0.cm.unet_levels_steps((1, 2, 4, 8, 16))
        if ahead:
            cm, seg = x0.cm, torch.is_grad_enabled()
            # the strides of voxel_to_point / point_to_voxel in _backbone_steps: x0 / y4 (1), x4 (16), y2 (4)
            point_index(cm, 1, z, cm.coords[1].shape[0], with_segments=seg)
            for s_ in (16, 4):
                n = cm.coords[s_].shape[0]
                point_index(cm, s_, z, n, with_segments=seg)
                voxel_index(cm, s_, z, n)
        return z, x0

    def prepare(self, x, ready=None, wait=True):
        """Build the coordinate structures of batch `x` (a SparseTensor as the forward takes it) NOW, on a stream of their own, and
        hang them on `x`; the forward that later receives `x` starts at the first convolution.  Meant to be called for batch i+1
        while step i is in flight (trainer.TrainStep(next_batch=...)): inside the forward each host read of the build waits for
        everything queued before it -- the previous step's backward.
        `ready`: an event after which the batch's tensors are valid (default: all work queued on the current stream so far).
        `wait=False`: issue the build up to its FIRST host read only and return without blocking (the one-pass level build: the sort
        and the level sizes on their way to the host); the forward resumes it from there.  The caller's thread never waits for the
        GPU in this form, which is what the training loop wants while the backward is still executing."""
        if getattr(x, "prepared", None) is not None or not x.F.is_cuda:
            return x
        with torch.cuda.device(x.F.device):      # the current device is per thread (prepare may run on a helper thread)
            s_idx = _index_stream(x.F.device)
            if ready is not None:
                s_idx.wait_event(ready)          # the batch was valid at `ready`: do not queue behind what the caller issued since
            else:
                s_idx.wait_stream(torch.cuda.current_stream())
        pending = PendingIndex(self._index_steps(x, ahead=True), s_idx, x.F.device, self.training)   # training: also the backward's sorted segments
        finished = pending.step()
        while wait and not finished:
            finished = pending.step()
        x.prepared = pending.done if finished else pending
        return x

    def forward(self, x):
        return self._backbone(x)
