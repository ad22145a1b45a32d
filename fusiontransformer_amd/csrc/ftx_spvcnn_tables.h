// Batch-table records of the SPVCNN entry points (layouts documented in include/ftx.h): read by ftx_spvcnn_eval (ftx_exec.hip), written by
// ftx_spvcnn_index_pairs (ftx_native_index.hip).  ftx_spvcnn_map_bytes / ftx_spvcnn_pv_bytes report their sizes.
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
static_assert(sizeof(SpvcnnMap) == 80 && sizeof(SpvcnnPV) == 64, "table records are packed");

}  // namespace ftx
