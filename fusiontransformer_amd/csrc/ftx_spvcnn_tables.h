// Table records of the SPVCNN entry points (layouts documented in include/ftx.h).  The batch tables (map, pv) are read by ftx_spvcnn_eval
// (ftx_exec.hip) and ftx_spvcnn_train_fwd / _bwd (ftx_exec_train.hip) and written by ftx_spvcnn_index_pairs (ftx_native_index.hip); the model
// table (layer), the program (op) and the train-only side tables are the two executors'.  ftx_spvcnn_*_bytes report their sizes.
// What the two executors do with these records on the host before they place or launch anything -- the view of one call's tables,
// the two sides of a kernel map, the checker of the program -- is ftx_spvcnn_program.h.
#pragma once
#include <stdint.h>

namespace ftx {

struct SpvcnnMap {
  const int32_t *nbr, *pos, *pos_t, *pair_in, *pair_out, *koff;
  int64_t n_pairs, n_in, n_out;
  int32_t kvol, fine_bijective;
};
struct SpvcnnPV {
  const int32_t *vox_idx, *vox_counts, *vox_order, *vox_seg_off, *devox_idx;
  const float *devox_weights;
  int64_t n_vox;
  int32_t level, reserved;
};
struct SpvcnnLayer {
  const float *weight, *bias, *gamma, *beta, *mean, *var;
  int32_t ca, co, kvol, stride, transposed, bf16;
  float eps;
  int32_t kind;
};
struct SpvcnnOp {
  int32_t kind, segment, layer, map, src, src2, dst, relu, level, channels, reserved0, reserved1;
};
// train-only side tables, parallel to the model table and to the pv table
struct SpvcnnTrainLayer {
  float *dweight, *dbias, *dgamma, *dbeta;
  float momentum;
  int32_t reserved;
};
struct SpvcnnTrainPV {
  const int32_t *devox_order, *devox_seg_off;
};
static_assert(sizeof(SpvcnnMap) == 80 && sizeof(SpvcnnPV) == 64 && sizeof(SpvcnnLayer) == 80 && sizeof(SpvcnnOp) == 48, "table records are packed");
static_assert(sizeof(SpvcnnTrainLayer) == 40 && sizeof(SpvcnnTrainPV) == 16, "table records are packed");

}  // namespace ftx
