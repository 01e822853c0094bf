// srhip_grad.h — argument block and launchers of the constant-gradient kernels (srhip_grad.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srhip_isa.h"

namespace srhip {

constexpr int GRAD_WAVES = 8;  // wavefronts per workgroup
constexpr int GRAD_KT = 8;     // tangent components per pass (constants per chunk)
// What a launch computes:
//   GMODE_LOSS  loss + d loss / d constants per (chunk, row block) -> slab (the optimiser's objective)
//   GMODE_ROWC  per-row d out / d constants -> out_der (eval_grad_tree_array, variable = false)
//   GMODE_ROWF  per-row d out / d features -> out_der (variable = true, and eval_diff_tree_array)
constexpr int GMODE_LOSS = 0, GMODE_ROWC = 1, GMODE_ROWF = 2;
constexpr int GRAD_ROW_KT = 4;  // tangent components per chunk of the per-row modes

struct GradArgs {
  const Ins* code;          // gradient programs of all trees
  const int32_t* prog_off;  // [ntrees]
  const int32_t* chunks;    // GMODE_LOSS: [nchunks][2] (tree, first constant); per-row modes:
                            // [nchunks][4] (tree, first component c0, end component, output row of
                            // component c0)
  const void* X;            // [nfeat][ld]
  const void* y;            // [ld]
  const void* w;            // [ld] or nullptr
  double* slab;             // [nchunks][nrb][GRAD_KT + 2]: loss sum, gradient sums, check statistic
  int64_t ld;
  int64_t nvalid;
  int32_t nchunks;
  int32_t nfeat;
  int32_t rb_rows;          // rows per workgroup (multiple of 64)
  int32_t nrb;
  int32_t chunks_per_group;
  int32_t loss_kind;
  double loss_p0;
  int32_t weighted;
  int32_t max_steps;
  // a derived view's derived-column count (its tangent-zero columns follow at + gd_nd); 0: none
  int32_t gd_nd;
  // row blocks of this launch: blockIdx.x + block0 (slab rows keep their global block index)
  int32_t block0;
  // value-only screening (GMODE_LOSS, KT = 0): a chunk whose block-0 record (written by an earlier
  // launch on the stream) already holds a non-finite check statistic is skipped -- its tree fails
  // did_succeed whatever the other blocks hold
  int32_t screened;
  // per-row modes: out_der[row + j][nvalid] for the components c0 + j < end (the values come from the
  // evaluator, which also decides did_succeed)
  void* out_der;
  // GMODE_LOSS launches of at most GRAD_INLINE chunks pass their (tree, c0) list here, in the kernel
  // arguments (chunks = nullptr): no host-to-device copy on the stream before the launch
  int32_t inl[2 * 96];
};
constexpr int GRAD_INLINE = 96;  // (448 measured the same on C4)
// a chunk is a (tree, c0) pair: the inline list holds GRAD_INLINE of them
static_assert(2 * GRAD_INLINE == sizeof(GradArgs::inl) / sizeof(int32_t), "inline chunk list size");
static_assert(sizeof(GradArgs) <= 4096, "kernel arguments are limited to 4 KB");

// kt = tangent components per chunk: 4 or GRAD_KT (the slab / reduced layout stride is kt + 2)
hipError_t launch_grad(int dtype, int K, int kt, const GradArgs& a, dim3 grid, hipStream_t s);
// per-row modes (GMODE_ROWC / GMODE_ROWF), GRAD_ROW_KT tangents per chunk
hipError_t launch_grad_rows(int dtype, int K, int gmode, const GradArgs& a, dim3 grid, hipStream_t s);
hipError_t launch_grad_reduce(int dtype, int kt, const double* slab, int nrb, int nchunks, double* out, hipStream_t s);
// The reduction of a row shard: grad_reduce_kernel's fold (the same bits), the record of launch-order chunk c
// written at exchange position pos[c] (nullptr: c) of a device buffer split by reduction operator --
// sum[nchunks][kt + 1] (loss sum, gradient sums: SUM across ranks) and chk[nchunks] (the check statistic: MAX for
// Float32, a non-finite value stored as +Inf; SUM for Float64).
hipError_t launch_grad_reduce_shard(int dtype, int kt, const double* slab, int nrb, int nchunks, const int32_t* pos,
                                    double* sum, double* chk, hipStream_t s);
// derived columns of a derived view: Xd[j] = U(X[f]) over ld rows, keys[j] = U << 16 | f (nd <= 32)
hipError_t launch_grad_derive(int dtype, const void* X, void* Xd, int64_t ld, const uint32_t* keys, int nd,
                              hipStream_t s);

// ---- one row subset per chunk (srhip_grad_rowsets.hip; srhip_eval_loss_grad_rowsets and the optimiser
// behind srhip_optimize_constants_rowsets) ---------------------------------------------------------
// A chunk is (program slot, first constant c0, tree whose row set it reads).  The sets are packed once
// per call by launch_grad_rowsets_pack: set t at element offset set_off[t], [nfeat + 1 (+ 1 weighted)]
// columns (features, y, w) of ld_t = set_m[t] rounded up to GRAD_ROWSET_RB rows, the positions past the
// set's end replicating its last row (the padding weight -0.0) as a gathered view's padding does.
constexpr int GRAD_ROWSET_RB = 256;  // the row block of grad_plan: a set's partial sums are per 256 rows
struct GradRowsetArgs {
  const Ins* code;          // gradient programs of all slots
  const int32_t* prog_off;  // [slots]
  const int32_t* chunks;    // [nchunks][3] (slot, c0, set), in launch order
  const void* packed;       // the packed sets
  const int64_t* set_off;   // [trees] element offset of each set in packed
  const int32_t* set_m;     // [trees] rows of each set (1 .. the cap)
  double* out;              // [nchunks][kt + 2] final records (coherent host memory)
  int64_t ld;               // (unused: the tile body's derived-column reads, never taken here)
  int32_t nchunks;
  int32_t nfeat;
  int32_t gd_nd;            // 0: row sets never use a derived view (it is off below 8192 rows)
  int32_t loss_kind;
  double loss_p0;
  int32_t weighted;
  int32_t max_steps;
};
// rows a wave can stage: whole 256-row blocks under ROWSET_LDS_BUDGET (0: the set's columns do not fit)
int grad_rowset_cap(int dtype, int64_t nfeat, bool weighted);
// max_ld: the longest padded set among the launch's chunks (sizes the per-wave LDS region)
hipError_t launch_grad_rowsets(int dtype, int kt, const GradRowsetArgs& a, int max_ld, hipStream_t s);
// the pack: rows[row_off[t] ..] of every column of the resident dataset -> packed (see above)
hipError_t launch_grad_rowsets_pack(int dtype, const void* X, const void* y, const void* w, int64_t src_ld, int nfeat,
                                    const int64_t* row_off, const int64_t* rows, const int64_t* set_off, int ntrees,
                                    void* packed, hipStream_t s);

}  // namespace srhip
