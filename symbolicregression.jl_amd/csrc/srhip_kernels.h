// srhip_kernels.h — kernel argument blocks and launcher declarations (host <-> srhip_eval.hip and the srhip_eval_<slice>.hip variant units).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srhip_isa.h"
#include "srhip_lossx.h"
#include "srhip_tail_shares.h"

namespace srhip {

#ifndef SRHIP_EVAL_WAVES
#define SRHIP_EVAL_WAVES 8
#endif
constexpr int EVAL_WAVES = SRHIP_EVAL_WAVES;  // wavefronts per workgroup of the interpreter kernel
// ... except the wide Float32 variant (R = 16, K = 2: the C2 / C3 kernel), which runs 16-wave
// workgroups, one per CU, over 4096-row blocks: twice the rows per staged block and per tree (the
// early exit of failed trees saves more of each block), the same 4 waves per SIMD (C2, one MI355X:
// 1.47 -> 1.34 ms)
constexpr int EVAL_WAVES_WIDE = 16;
constexpr int eval_waves(int R, int K) { return (R == 16 && K <= 2) ? EVAL_WAVES_WIDE : EVAL_WAVES; }
constexpr int EVAL_WAVES_MAX = EVAL_WAVES_WIDE > EVAL_WAVES ? EVAL_WAVES_WIDE : EVAL_WAVES;
#ifndef SRHIP_R_F32
#define SRHIP_R_F32 8
#endif
constexpr int R_F32 = SRHIP_R_F32;  // rows per lane per dispatch, 4-byte types
constexpr int R_F64 = 4;       // rows per lane per dispatch, Float64
// Float32 trees whose stack fits K = 2 on datasets of at least WIDE_MIN_ROWS rows run with twice
// the rows per lane: the per-instruction dispatch cost is paid once per 16 rows (121 VGPRs,
// 4 waves per SIMD; the VALU-bound operators are unaffected, the cheap ones get ~20 % faster).
constexpr int R_F32_WIDE = 16;
constexpr int64_t WIDE_MIN_ROWS = 4096;
constexpr int ROW_ALIGN = 4096;  // device datasets are padded to a multiple of this many rows
constexpr int MODE_LOSS = 0, MODE_PRED = 1, MODE_PRECISE = 2;
// Loss partials are kept per fixed chunk of rows (not per workgroup row block): every lane adds
// its rows of a chunk in the same order whatever R, K, row-block size or program (derived columns
// or not) evaluates the tree, so a tree's loss on a dataset is one bit pattern in every launch.
// Row blocks are whole chunks.
constexpr int LOSS_CHUNK_4B = 1024, LOSS_CHUNK_8B = 256;
inline int loss_chunk(int dtype) { return dtype == SRHIP_F64 ? LOSS_CHUNK_8B : LOSS_CHUNK_4B; }
// The rows that pad a weighted dataset, a gathered view or a staged row set up to whole tiles repeat
// the last row with the weight -0.0, the one weight no row of the caller has (an uploaded -0.0 is
// stored as +0.0, which is the same weight in every product and sum).  The loss epilogue tells a
// padded row by it (loss_tile): the repeated row's loss may be Inf at a finite prediction, and
// 0 * Inf is NaN, where a caller's own zero weight must give what sum(w .* l) gives.
template <typename T> __host__ __device__ inline T pad_weight() { return T(0); }  // (Int32: no weights)
template <> __host__ __device__ inline float pad_weight<float>() { return -0.0f; }
template <> __host__ __device__ inline double pad_weight<double>() { return -0.0; }
__host__ __device__ inline bool is_pad_weight(float w) { return w == 0.0f && __builtin_signbit(w); }
__host__ __device__ inline bool is_pad_weight(double w) { return w == 0.0 && __builtin_signbit(w); }

struct FeatStat {
  double sum;           // f64 sum (Float64 data: sum of x * 2^-64)
  long long nonfinite;  // count of Inf/NaN entries
  double maxabs;        // max |x| over the finite entries (round 6: the Float32 interpreter's +/- bound)
};
// launch_feature_stats splits each column into at most FEAT_STAT_BLOCKS row chunks; its output
// buffer holds the nfeat results followed by the partials.
constexpr int FEAT_STAT_BLOCKS = 64;
inline size_t feature_stats_scratch(int64_t nfeat) { return (size_t)(nfeat < 1 ? 1 : nfeat) * (1 + FEAT_STAT_BLOCKS); }

// Forms of the interpreter kernel (eval_kernel's last template argument).  FORM_HOT: the persistent
// main launch of the wide Float32 loss kernel -- whole-tree claims over staged row blocks, slab
// results only; its launch carries EvalArgs::recs.  Everything else runs FORM_GENERAL.
constexpr int FORM_GENERAL = 0, FORM_HOT = 1;
// What a hot-form wave reads per tree, by order slot, in one 16-byte scalar load.  Built by the host
// with the launch order (the program of the launch: pc0 and the mask are the derived-column
// program's when the launch uses it) and uploaded in the same copy.
struct alignas(16) SlotRec {
  int32_t tree;       // order[slot]
  int32_t pc0;        // prog_off[tree]
  uint32_t dmask_lo;  // dmask[tree] (0 without derived columns)
  uint32_t dmask_hi;
};
static_assert(sizeof(SlotRec) == 16, "one s_load_dwordx4");

struct EvalArgs {
  const Ins* code;          // all trees' bytecode
  const int32_t* prog_off;  // [ntrees] first instruction of each tree
  const int32_t* order;     // [ntrees] processing order (grouped, cost-sorted)
  const void* X;            // [>= nfeat][ld] SoA, padded (the first nfeat columns are staged)
  const void* y;            // [ld] (nullptr for prediction-only)
  const void* w;            // [ld] or nullptr
  void* slab_loss;          // [nrb][ntrees][rb_rows / loss chunk] loss partials per row chunk, by order slot
                            // (double; int64 for Int32)
  void* slab_chk;           // [nrb][ntrees] check partials by order slot (float max|v| / double sum|v|*2^-512)
  void* out_pred;           // [ntrees][nvalid] (MODE_PRED)
  void* slab_prec;          // [n][prec_stride][nrb] double (MODE_PRECISE)
  int64_t ld;               // padded rows of X / y / w
  int64_t nvalid;           // rows evaluated
  int32_t ntrees;
  int32_t nfeat;
  int32_t rb_rows;          // rows per workgroup (multiple of 64*R)
  int32_t nrb;              // row blocks
  int32_t nch;              // loss chunks: ceil(nvalid / loss_chunk)
  int32_t cpb;              // loss chunks per row block (rb_rows / loss_chunk)
  int32_t trees_per_group;  // trees per grid.y group (group_off == nullptr)
  const int32_t* group_off; // [grid.y + 1] first order slot of each group, or nullptr (uniform groups)
  int32_t loss_kind;
  double loss_p0;
  int32_t weighted;
  int32_t prec_stride;      // operator nodes per tree slot in slab_prec
  int32_t has_y;            // stage y into LDS (MODE_LOSS)
  int32_t max_steps;        // longest tree program (instructions): bounds every interpreter loop
  int32_t debug_stop;       // diagnostic early exits (SRHIP_DEBUG_STOP); 0 in normal runs
  int32_t nd;               // derived columns (LDS columns nfeat .. nfeat+nd-1); 0 unless XLDS
  const uint32_t* dspec;    // [nd] (U << 16) | feature of each derived column
  const uint64_t* dmask;    // [program trees] bit d: the tree reads derived column d
  int32_t* dbg;             // SRHIP_TRACE: host-coherent progress words of block (0,0) wave 0, else nullptr
  int32_t early_exit;       // MODE_LOSS: a wave stops a tree's row block once its check statistic is
                            // non-finite (the tree has failed: DynamicExpressions' early return) and
                            // marks the tree failed for the row blocks that have not started it
  int32_t epoch;            // this launch's mark (> 0; fail_flag[slot] == epoch: failed in this launch)
  int32_t* fail_flag;       // [ntrees] by order slot
  // single-row-block launches (nrb == 1, small datasets): each wave finishes its tree's reduction
  // itself, in reduce_kernel's order, and writes the results to these (coherent pinned host) arrays
  // indexed by tree; no reduce launch
  int32_t fused;
  void* fused_loss;         // [program trees] LAccT (MODE_LOSS) or nullptr
  void* fused_chk;          // [program trees] check statistic type, or nullptr (Int32)
  // persistent launches (one tree group, the whole population): grid.x workgroups claim row blocks
  // block0 .. nrb-1 from *block_ctr (zeroed before the launch)
  int32_t persistent;
  int32_t block0;
  int32_t tail_blocks;      // the last tail_blocks row blocks, tail_slices units each, are claimed as
  int32_t tail_slices;      // tail_shares equal shares of their units (srhip_tail_shares.h); 0 blocks:
  int32_t tail_shares;      // every block is claimed whole
  int32_t grid_interleave;  // grid launches: workgroup (x, y) takes order slots y, y + grid.y, ... (group_off unused)
  int32_t tile_claims;      // a wave claims one (tree, tile) at a time (R = 16 probe; slab_chk / slab_rows zeroed first)
  int32_t block_stride;     // grid launches: workgroup x takes row blocks x, x + grid.x, ... (< nrb)
  int32_t* block_ctr;
  // probe launches (tile_claims): zero_ctr, if set, is the persistent launch's block counter, zeroed
  // by workgroup (0, 0) -- the persistent launch follows on the same stream; and every workgroup zeroes
  // its own (row block, slot) entries of slab_chk / slab_rows before its waves combine into them
  int32_t* zero_ctr;
  // MODE_PRECISE launches over a device-built list of undecided trees (order = the list): the number
  // of listed trees is read here (*dev_count, capped at trees_per_group); each wave zeroes its
  // (tree, row block) slab entries before accumulating into them
  const int32_t* dev_count;
  int32_t wg_waves;         // waves per workgroup (0: the variant's eval_waves; fewer claim the same trees)
  int32_t prec_assign;      // MODE_PRECISE with one tile per (tree, row block): store the per-operator
                            // sums instead of adding to them (no dependent load per operator)
  int32_t* slab_rows;       // [nrb][ntrees] valid rows each (row block, order slot) evaluated, or nullptr
  int64_t* fused_rows;      // fused launches: [program trees] rows evaluated (coherent pinned host), or nullptr
  const SlotRec* recs;      // [ntrees] by order slot: FORM_HOT launches (else nullptr)
};

int rows_per_lane(int dtype);
// rows per lane of the kernel variant that evaluates a launch (K stack slots, mode, m rows)
int pick_rows_per_lane(int dtype, int K, int mode, int64_t m);
hipError_t launch_eval(int dtype, const EvalArgs& a, int R, int K, int mode, bool xlds, dim3 grid, size_t lds,
                       hipStream_t s);
// per-tree reduction of eval_kernel's slabs: nslots order slots, cpb loss chunks per row block, results
// at out[order[slot]]
// slab_rows (optional): [nrb][nslots] rows evaluated, summed per tree into out_rows (int64)
// The device's share of the did_succeed decision: a tree whose check statistic is finite
// but whose overflow bound reaches half the threshold (Float32: chk x rows >= 2^127 - 2^102 exactly;
// Float64: chk >= 2^511) is appended to ulist (ulist[0] = count, trees from ulist[1], at most umax;
// the count keeps growing past umax) for the precise pass that follows on the stream.
struct UndecidedList {
  int32_t* ulist = nullptr;  // nullptr: no device list (the host decides after the launch)
  int32_t umax = 0;
  double rows = 0.0;
  // Float32 programs (round 6): + and - fold no check statistic in the interpreter.  Per program tree
  // (cM, cF, c0, 0) bounds every +/- output by cM M + cF fbound + c0 (M: the statistic of the folded
  // values, fbound: the features' max |x|, +Inf if any is non-finite; TreeCompiler::skip_bounds); the
  // reduction raises each tree's statistic to that bound (skip_bound_apply) before it is written or
  // tested.  nullptr: no bound (Float64, Int32)
  const float* sbound = nullptr;
  float fbound = 0.0f;
};
// max(M, cM M + cF F + c0) clamped to FLT_MAX for a finite M (a non-finite M stands): a finite bound
// only ever turns a decided tree into an undecided one -- which the exact precise pass then decides --
// and never a finite statistic into a failure.  The same function on the host (fused single-block
// launches) and in the reduction.
__host__ __device__ inline float skip_bound_apply(float M, const float* sb, float F) {
  if (!(sb[0] > 0.0f || sb[1] > 0.0f || sb[2] > 0.0f) || !(M - M == 0.0f)) return M;
  const double fb = sb[1] > 0.0f ? (double)sb[1] * (double)F : 0.0;
  const double bd = (double)sb[0] * (double)M + (fb + (double)sb[2]);
  const double mb = bd > (double)M ? bd : (double)M;
  return mb < (double)__FLT_MAX__ ? (float)mb : __FLT_MAX__;
}
hipError_t launch_reduce(int dtype, const void* slab_loss, int nch, int cpb, const void* slab_chk, int nrb, int nslots,
                         const int32_t* order, void* out_loss, void* out_chk, hipStream_t s,
                         const int32_t* slab_rows = nullptr, int64_t* out_rows = nullptr,
                         const UndecidedList& ul = UndecidedList(), bool chk_inf = false,
                         int32_t* items_done = nullptr, int64_t* out_items = nullptr);
// The precise pass's per-(listed tree, operator) sums over the row blocks (fixed order, compensated),
// written to out (coherent host memory: out_count, then [umax][stride] doubles); the last workgroup
// resets ulist[0] (ulist[1 + done_slot]: its finished-workgroup counter, zero between launches).
hipError_t launch_precise_reduce(const double* slab, int nrb, int stride, int32_t* ulist, int umax, int groups, int done_slot,
                                 int32_t* out_list, double* out, hipStream_t s);
hipError_t launch_gather(int dtype, const void* X, const void* y, const void* w, int64_t ld_src, int nfeat,
                         const int64_t* idx, int64_t m, int64_t ld_dst, void* Xd, void* yd, void* wd, hipStream_t s);
hipError_t launch_feature_stats(int dtype, const void* X, int64_t ld, int64_t m, int nfeat, FeatStat* out,
                                hipStream_t s);

// One row subset per tree in one launch (srhip_rowsets.hip; srhip_eval_loss_rowsets).  e is a fused
// single-row-block MODE_LOSS launch of one-tree groups over the plain program: X / y / w the RESIDENT
// dataset (the kernel gathers from it), ld = rb_rows = ld_lds, cpb = the loss chunks of ld_lds rows,
// order = the launched trees, ntrees = their number, nfeat = the program's feature columns.
struct RowsetArgs {
  EvalArgs e;
  const int64_t* row_off;  // [program trees + 1] first position of each tree's set in rows
  const int64_t* rows;     // the sets' dataset rows (0-based, in [0, n))
  int64_t src_ld;          // padded rows of the resident X / y / w
  int32_t nstage;          // feature columns staged and measured: the dataset's
  int32_t ld_lds;          // rows of a wave's LDS region per column: whole tiles, >= the longest launched set
  FeatStat* fstat;         // [program trees][nstage] each set's feature statistics (coherent host)
  double* wsum;            // [program trees] each set's weight sum, position order (coherent host), or nullptr
};
// LDS bytes a wave may stage, and the longest set (whole tiles) that fits for a dataset of nfeat
// feature columns: Float32 with 8 features, y and w: 1024 rows; four such waves per CU
constexpr int ROWSET_LDS_BUDGET = 40 * 1024;
int rowset_cap(int dtype, int64_t nfeat, bool weighted);
hipError_t launch_rowsets(int dtype, const RowsetArgs& a, int nlaunch, hipStream_t s);

// The same under a loss given as an expression (srhip_rowsets_lossx.hip; srhip_eval_loss_expr_rowsets).  r.e is
// a fused single-row-block MODE_PRED launch of one-tree groups (no y / w / loss kind: the kernel stages y and w
// itself; fused_chk and fused_rows as above, fused_loss unused); the loss program travels beside it.
struct RowsetLossxArgs {
  RowsetArgs r;
  LossxProgram lx;
  void* pred;        // [launched trees][ld_lds] T: each wave's predictions (device scratch)
  double* out_loss;  // [program trees] each set's loss sum in lossx_kernel's order (coherent host)
  double* out_wsum;  // [program trees] each set's weight sum in the same order (coherent host), or nullptr
};
static_assert(sizeof(RowsetLossxArgs) <= 4096, "kernel arguments are limited to 4 KB");
// the longest set a wave stages under an expression loss: rowset_cap (Float32 / Float64; 0 otherwise)
int rowset_lossx_cap(int dtype, int64_t nfeat, bool weighted);
hipError_t launch_rowsets_lossx(int dtype, const RowsetArgs& a, const LossxProgram& lx, void* pred, double* out_loss,
                                double* out_wsum, int nlaunch, hipStream_t s);

// A whole view under a loss given as an expression, in one launch (srhip_eval_lossx.hip;
// srhip_eval_loss_expr_fused, srhip_eval_loss_expr_submit, the expression coalescer).  e is a MODE_PRED launch
// over the plain program in the shape of ONE item: rb_rows = LOSSX_BLOCK_ROWS, uniform groups of trees_per_group
// order slots, no y / w / loss kind, not fused, not persistent; slab_chk / slab_rows are [nblocks][ntrees] by
// order slot, as launch_reduce reads them.  The launch relabels its trees by order slot: e.order is the
// identity and e.prog_off is indexed by slot, so a workgroup's predictions pack into its own slab.
struct EvalLossxArgs {
  EvalArgs e;
  LossxProgram lx;
  const void* y;     // [ld] the view's targets
  const void* w;     // [ld] its weights (weighted datasets), or nullptr
  void* pred;        // [workgroups][trees_per_group][LOSSX_BLOCK_ROWS] T: each workgroup's predictions of its item
  double* partials;  // [ntrees + (w ? 1 : 0)][nblocks] by order slot, then the weights' slot: lossx_kernel's partials
  int64_t m;         // rows of the view
  int32_t nblocks;   // loss blocks: ceil(m / LOSSX_BLOCK_ROWS)
  int32_t ngroups;   // tree groups: ceil(ntrees / trees_per_group)
};
static_assert(sizeof(EvalLossxArgs) <= 4096, "kernel arguments are limited to 4 KB");
// the launch, then the per-slot sums of the partials in ascending block order (lossx_finish_kernel's text)
// into out[ntrees + (w ? 1 : 0)] (coherent host memory)
hipError_t launch_eval_lossx(int dtype, const EvalLossxArgs& q, bool xlds, int wgs, size_t lds, double* out,
                             hipStream_t s);

}  // namespace srhip
