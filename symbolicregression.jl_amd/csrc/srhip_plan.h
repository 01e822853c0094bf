// srhip_plan.h — how a population evaluation runs, decided from shapes, device limits and the
// SRHIP_* switches alone (srhip_plan.cpp: no HIP runtime call, no device).  eval_issue enqueues the
// plan; plan_persistent_order (the order made at srhip_program_create) asks the same function, so the
// two cannot drift apart; srhip_plan_eval (include/srhip.h) shows the plan to the tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "srhip_kernels.h"

struct srhip_program;

namespace srhip {

struct LaunchPlan {
  int rb_rows, nrb, groups, tpg;
  bool xlds;
  size_t lds;
};
// ncols: feature (+ derived) columns staged; lds_budget: bytes of LDS a workgroup may use
LaunchPlan plan_launch(int num_cu, int dtype, int64_t ncols, bool weighted, bool with_y, int64_t m, int32_t ntrees,
                       int rows_per_tile, size_t lds_budget = 64 * 1024 - 64, int waves = EVAL_WAVES);

struct EvalPlanIn {  // everything the decision reads, and nothing else
  int dtype, mode;      // SRHIP_F32 / F64 / I32, MODE_*
  int32_t nlive;        // trees not failed statically
  int64_t m;            // rows of the view
  int32_t maxfeat, nd;  // staged feature columns, derived columns
  int32_t kmax, dkmax;  // stack depth: plain / derived-column program
  bool wide_ops;        // asin / acos / atanh_clip present (the K_MAX variant only)
  bool weighted;        // weights used by this launch
  bool sharded;         // partials go to an exchange buffer (no fused reduce)
  bool have_recs;       // the order carries slot records
  int32_t loss_kind;
  int num_cu;
  int64_t lds_max;      // the device's LDS per workgroup
};
enum { PLAN_SMALL = 0, PLAN_PERSISTENT = 1, PLAN_GRID = 2 };
struct EvalPlan {
  int kind;        // PLAN_SMALL, PLAN_PERSISTENT, PLAN_GRID
  int R, K;        // the kernel variant: rows per lane, stack slots
  bool use_d;      // the derived-column program
  LaunchPlan L;    // persistent and small launches: one group of all live trees
  int nch, cpb;    // loss chunks of the view; loss chunks per row block (row blocks are whole chunks)
  int wg_waves;    // small: one wave per tree (0: the variant's)
  int probe_blocks, wgs;  // persistent: row blocks of the probe launch, workgroups of the main launch
  bool probe_tile_claims;  // ... whose probe claims (tree, tile) pairs and zeroes the block counter itself
  int tail_slices, tail_blocks, tail_shares;  // ... its last round (srhip_tail_shares.h)
  int expect_items;                           // ... the items its workgroups must report evaluated
  bool fused;  // single-block launch: the interpreter writes the records (no reduction)
  bool hot;    // persistent: the hot form (FORM_HOT)
};
EvalPlan plan_eval(const EvalPlanIn& in);

// The one-launch form of a loss expression (srhip_eval_lossx.hip): items of (tree group, loss block) dealt to a
// persistent-style grid.  The row block is the loss block (a block's partial is one butterfly over 256 virtual
// threads, so it is never split); its feature columns are staged in LDS when they fit, else read from global
// memory; the predictions' scratch is wgs x tpg x rb_rows elements whatever ntrees x m is.  plan_eval is not
// asked: this launch has none of its forms.
struct LossxPlanIn {
  int dtype;        // SRHIP_F32 / SRHIP_F64
  int32_t nlive;    // trees not failed statically
  int64_t m;        // rows of the view
  int32_t maxfeat;  // staged feature columns
  int num_cu;
  int64_t lds_max;  // the device's LDS per workgroup
};
struct LossxPlan {
  int rb_rows, R;       // rows of an item; rows per lane of the interpreter variant
  bool xlds;
  int tpg, ngroups;     // trees per item, tree groups
  int64_t nblocks;      // row blocks
  int wgs, wg_per_cu;   // workgroups of the launch: at most wg_per_cu (the resident ones: 1) per CU, one per item
  size_t lds, lds_cols, lds_budget, scratch_bytes;
};
LossxPlan plan_eval_lossx(const LossxPlanIn& in);

// asin / acos / atanh_clip among a program's unary operators: they live only in the K_MAX variant
bool has_wide_ops(const std::vector<int32_t>& unaops);
std::vector<int32_t> shape_groups(const LaunchPlan& L, int32_t ntrees, int num_cu);
std::vector<int32_t> make_order(const srhip_program& P, const std::vector<int32_t>& trees,
                                const std::vector<int32_t>& goff, bool derived);
int append_slot_records(const srhip_program& P, std::vector<int32_t>& order, int nl, bool derived);

}  // namespace srhip
