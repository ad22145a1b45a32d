"""The case table of the autograd contract (tests/autograd_cases.py) covers every torch.autograd.Function node of functional.py: a node
added without an entry fails here, on the CPU, before its contract can go unchecked on the GPU."""
import inspect

import torch

from fusiontransformer_amd import functional as spf
from tests.autograd_cases import CASES, VARIATIONS

# node -> the public entry whose cases run it
NODE_ENTRY = {"_Voxelize": "spvoxelize", "_Devoxelize": "spdevoxelize", "_SparseConv": "sparse_conv", "_RowsLinear": "linear",
              "_RowsMatmul": "rows_matmul", "_BatchNormTrain": "batch_norm", "_BatchNormEval": "batch_norm", "_ConvBNTrain": "conv_bn_train",
              "_LiftGather": "lift_gather", "_ResampleNearest": "resample_nearest", "_AffineSample": "affine_sample", "_AffineLift": "affine_lift",
              "_LocConvPoolRelu": "loc_conv_pool_relu", "_LayerNorm": "layer_norm", "_AddLayerNorm": "add_layer_norm", "_Attention": "attention",
              "_VitLinear": "vit_linear", "_VitMlp": "vit_mlp", "_SampleDown": "sample_down", "_FusionLoss": "fusion_loss", "_SegLoss": "seg_loss"}
TORCH_ONLY = {"_LibraryMatmulBf16"}      # library GEMMs on rounded operands: no kernel of this project, no raw pointer


def test_every_node_has_cases():
    nodes = {n for n, c in inspect.getmembers(spf, inspect.isclass) if issubclass(c, torch.autograd.Function) and c.__module__ == spf.__name__}
    assert nodes == set(NODE_ENTRY) | TORCH_ONLY
    entries = {c.entry for c in CASES}
    assert entries == set(NODE_ENTRY.values())
    assert all(callable(getattr(spf, e)) for e in entries)


def test_table_is_well_formed():
    assert len({c.id for c in CASES}) == len(CASES)
    for entry in {c.entry for c in CASES}:
        assert any(c.fullest for c in CASES if c.entry == entry), entry      # the bad-operand check has an option set to run at
    for c in CASES:
        assert c.names("diff", {k: 0 for k in c.ops}), c.id
        for op in c.ops.values():
            assert op.role in ("diff", "refused", "data") and op.bad <= set(VARIATIONS)
        assert (c.truth is not None) or not c.nondet, c.id                   # a float-atomic quantity has a bound to be held to
