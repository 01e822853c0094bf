// srhip_plan.cpp — the launch decision of a population evaluation (srhip_plan.h), the tree groups and
// the cost-sorted order behind it.  Host arithmetic only: nothing here calls the HIP runtime.
#include "srhip_plan.h"

#include <algorithm>

#include "srhip_internal.h"

using namespace srhip;

bool srhip::has_wide_ops(const std::vector<int32_t>& unaops) {
  bool wide = false;
  for (int32_t u : unaops) wide |= u == SRHIP_OP_ASIN || u == SRHIP_OP_ACOS || u == SRHIP_OP_ATANH_CLIP;
  return wide;
}

LaunchPlan srhip::plan_launch(int num_cu, int dtype, int64_t nxcols, bool weighted, bool with_y, int64_t m,
                              int32_t ntrees, int tile, size_t budget, int waves) {
  LaunchPlan L;
  ntrees = std::max<int32_t>(1, ntrees);  // every tree may have failed statically
  m = std::max<int64_t>(1, m);
  const size_t es = dtype_size(dtype);
  const int ncols = (int)nxcols + (with_y ? 1 : 0) + (weighted ? 1 : 0);
  const int lo = std::max(tile, loss_chunk(dtype));  // row blocks are whole tiles and loss chunks
  int rb = ROW_ALIGN;
  while (rb > lo && (size_t)ncols * rb * es > budget) rb /= 2;
  // do not make blocks much larger than the data
  while (rb > lo && rb / 2 >= m) rb /= 2;
  // diagnostic override (tuning runs): SRHIP_RB_ROWS = rows per workgroup, a power of two >= tile
  static const int rb_env = [] { const char* e = getenv("SRHIP_RB_ROWS"); return e ? atoi(e) : 0; }();
  if (rb_env >= lo && rb_env <= ROW_ALIGN && (rb_env & (rb_env - 1)) == 0 && rb_env < rb) rb = rb_env;
  L.rb_rows = rb;
  L.xlds = (size_t)ncols * rb * es <= budget;
  L.lds = (L.xlds ? (size_t)ncols * rb * es : 0) + 16;
  L.nrb = (int)((m + rb - 1) / rb);
  const int target_blocks = 4 * num_cu;
  int g = (target_blocks + L.nrb - 1) / L.nrb;
  const int max_g = std::max(1, ntrees / (2 * waves));
  g = std::max(1, std::min(g, max_g));
  L.groups = g;
  L.tpg = (ntrees + g - 1) / g;
  L.groups = (ntrees + L.tpg - 1) / L.tpg;
  return L;
}

EvalPlan srhip::plan_eval(const EvalPlanIn& in) {
  // ---- the switches (read per launch: tests and the bench toggle them inside one process) ----
  // SRHIP_NO_PERSISTENT=1: the grid launch; SRHIP_PRB_ROWS: row-block rows (default 2048: C2, one
  // MI355X, same box: 1024 rows 1.31 ms, 2048 1.19, 4096 1.35, grid launch 1.33);
  // SRHIP_PROBE_BLOCKS: probe row blocks (default 4).
  const bool no_persistent = env_flag("SRHIP_NO_PERSISTENT");
  const int prb_env = env_int("SRHIP_PRB_ROWS", 0);
  const int probe_env = env_int("SRHIP_PROBE_BLOCKS", -1);
  const bool probe_tree_claims = env_flag("SRHIP_PROBE_TREE_CLAIMS");  // the probe claims whole trees
  const int small_max = env_int("SRHIP_SMALL_POP", 16);  // the largest population launched small (0: never)
  const bool derive_always = env_flag("SRHIP_DERIVE_ALWAYS");  // (tests: the derived program whatever the blocks)
  const bool no_fuse = env_flag("SRHIP_NO_FUSED_REDUCE");  // the reduce kernel after a single-block launch too
  //   SRHIP_TAIL_BALANCE=0: whole blocks; SRHIP_TAIL_SLICES=S > 1: units per block (default
  //   TAIL_UNITS, at most 128); SRHIP_TAIL_SHARE_ROUNDS=2: 2 wgs shares; SRHIP_PERSISTENT_WGS=n
  //   (tests): at most n workgroups.
  constexpr int TAIL_UNITS = 128;
  const int wgs_cap = std::max(1, std::min(env_int("SRHIP_PERSISTENT_WGS", in.num_cu), in.num_cu));
  const int units_env = env_int("SRHIP_TAIL_SLICES", 0);
  const int units = units_env > 1 ? std::min(units_env, 128) : TAIL_UNITS;
  const bool tail_balance = env_int("SRHIP_TAIL_BALANCE", 1) != 0;
  const int share_rounds = env_int("SRHIP_TAIL_SHARE_ROUNDS", 1) == 2 ? 2 : 1;
  const bool no_hot = env_flag("SRHIP_NO_HOT_FORM");  // the general form
  const int dstop = debug_stop();  // SRHIP_DEBUG_STOP, SRHIP_TRACE: read once per process
  const bool trace = trace_on();

  const int dtype = in.dtype, mode = in.mode, nd = in.nd, nl = in.nlive;
  const int64_t m = in.m;
  const bool weighted = in.weighted, with_y = mode == MODE_LOSS;
  const size_t es = dtype_size(dtype);
  EvalPlan p{};
  LaunchPlan& L = p.L;
  // stack slots of the kernel variant; the wide operators live only in the K_MAX variant
  auto kvariant = [&](int32_t kmax) { return in.wide_ops ? K_MAX : (kmax <= 2 ? 2 : (kmax <= 4 ? 4 : 8)); };
  // LDS a workgroup may stage: the 16-wave variant runs one workgroup per CU (160 KB, less the
  // kernel's static arrays); 8-wave workgroups run two (derived-column programs) or more
  // (the device's LDS per workgroup, read once per context, less 8 KB for the kernel's static arrays)
  const size_t lds_dev = (size_t)in.lds_max;
  auto lds_budget = [lds_dev](int r, int k, bool derived) -> size_t {
    if (eval_waves(r, k) >= 16) return lds_dev - 8 * 1024;
    return std::min<size_t>(lds_dev / 2, derived ? 64 * 1024 - 512 : 64 * 1024 - 64);
  };
  auto grid_plan = [&](int K, int ncols, bool derived) {  // (sets the plan's variant to K's)
    p.K = K;
    p.R = pick_rows_per_lane(dtype, K, mode, m);
    return plan_launch(in.num_cu, dtype, ncols, weighted, with_y, m, nl, 64 * p.R, lds_budget(p.R, K, derived),
                       eval_waves(p.R, K));
  };
  // Few trees over many rows (the search's coalesced launches: C3 carries ~2.4 trees per launch over
  // 10M rows): a workgroup of one wave per tree per loss chunk of rows, X read from global memory.
  // The staged launches give each tree one wave per CU -- a 2048-row block staged for 2 trees leaves
  // 14 of its 16 waves idle.
  const bool small = (mode == MODE_LOSS || mode == MODE_PRED) && dstop == 0 && nl <= small_max &&
                     m >= (int64_t)64 * ROW_ALIGN;
  // Persistent launch (the wide Float32 variant's loss launches): one workgroup per CU claims short
  // row blocks from a counter and interprets the WHOLE population over each -- the dataset is read
  // from HBM once, every derived column is computed once per row block for all trees, and the tail
  // is one short block instead of a wave of workgroups.  A probe launch first evaluates the leading
  // row blocks with many small tree groups, so trees that fail there (DynamicExpressions' early
  // return: did_succeed = false whatever the other rows hold) are skipped by every later block.
  bool persistent = false;
  if (small) {
    p.K = kvariant(in.kmax);
    p.R = pick_rows_per_lane(dtype, p.K, mode, m);
    const int rb = std::max(64 * p.R, loss_chunk(dtype));
    L = LaunchPlan{rb, (int)((m + rb - 1) / rb), 1, nl, false, 16};  // one group, nothing staged
    p.wg_waves = nl;  // one wave per tree (at most the variant's waves)
  } else {
    const int Kp = kvariant(in.kmax);
    persistent = !no_persistent && mode == MODE_LOSS && dstop == 0 && dtype == SRHIP_F32 &&
                 pick_rows_per_lane(dtype, Kp, mode, m) == R_F32_WIDE && R_F32_WIDE != R_F32 &&
                 (nd == 0 || kvariant(in.dkmax) == Kp);
    if (persistent) {
      p.K = Kp;
      p.R = R_F32_WIDE;
      const int tile = 64 * p.R;
      int rb = prb_env >= tile && prb_env <= ROW_ALIGN && (prb_env & (prb_env - 1)) == 0 ? prb_env : 2048;
      rb = std::max(rb, std::max(tile, loss_chunk(dtype)));
      // derived-column program when its staging fits LDS; otherwise the plain program
      const int base_cols = in.maxfeat + 1 + (weighted ? 1 : 0);
      p.use_d = nd > 0 && (size_t)(base_cols + nd) * rb * es <= lds_budget(p.R, p.K, true);
      const int ncols = base_cols + (p.use_d ? nd : 0);
      if ((size_t)ncols * rb * es > lds_budget(p.R, p.K, false)) {
        persistent = false;  // the block does not fit LDS: grid launch over global reads
        p.use_d = false;
      } else {
        L = LaunchPlan{rb, (int)((m + rb - 1) / rb), 1, nl, true, (size_t)ncols * rb * es + 16};  // one group
        p.probe_blocks = probe_env >= 0 ? probe_env : 4;
        p.probe_blocks = L.nrb >= 16 * std::max(1, p.probe_blocks) ? p.probe_blocks : 0;
        p.probe_tile_claims = p.probe_blocks > 0 && !probe_tree_claims;
      }
    }
  }
  if (!small && !persistent && nd > 0 && mode != MODE_PRECISE) {
    const LaunchPlan Lp = grid_plan(kvariant(in.kmax), in.maxfeat, false);
    L = grid_plan(kvariant(in.dkmax), in.maxfeat + nd, true);
    p.use_d = L.xlds;
    // ... and only when its columns do not shrink the row block: a wave's early exit of a failed tree
    // saves the rest of its row block, and shorter blocks lose more than the shared columns save
    // (C2, one MI355X, warm, separate processes: 10 columns at 2048-row blocks 1.29 ms vs the plain
    // program at 4096 rows 1.27 ms with 16-wave workgroups; 1.56 vs 1.41 ms at 1024 / 2048 rows with
    // 8-wave workgroups)
    if (p.use_d && !derive_always && Lp.xlds && Lp.rb_rows > L.rb_rows) p.use_d = false;
  }
  if (!small && !persistent && !p.use_d) L = grid_plan(kvariant(in.kmax), in.maxfeat, false);
  p.kind = small ? PLAN_SMALL : persistent ? PLAN_PERSISTENT : PLAN_GRID;
  p.nch = (int)((m + loss_chunk(dtype) - 1) / loss_chunk(dtype));
  p.cpb = L.rb_rows / loss_chunk(dtype);
  // one row block: the waves finish the per-tree reduction themselves
  p.fused = L.nrb == 1 && !in.sharded && !no_fuse;
  if (!persistent) return p;
  const int nmain = L.nrb - p.probe_blocks;
  // The last round in equal shares (srhip_tail_shares.h).  Whole blocks on wgs workgroups leave the
  // Lb = nmain % wgs blocks past the last whole round to Lb workgroups while the others idle for a
  // block: C2's 485 blocks on 256 workgroups last 2.0 block times for 1.894 of work, and 49 blocks
  // (100k rows) run on 49 of 256 CUs.  Claiming those blocks as S population slices each, one by
  // one, cannot help: the round then lasts ceil(Lb S / wgs) / S block times -- C2: 8/8 at S = 8,
  // 15/16 at S = 16 -- and every slice restages its block and re-derives its columns (C2, same box:
  // whole blocks 1.215 ms, S = 8 1.250, 16 1.278).  Instead the Lb S units are dealt to the
  // workgroups as nshares contiguous ranges of near-equal length, one claim each: a share stages at
  // most two blocks however many units it holds, and at S = 128 C2's round lasts 115/128 block times
  // (units are an index mapping, not a staging: the finest S of the measured 32 / 64 / 128 is as fast
  // or faster at 300k and 1M rows, profiles/r07_tail_shares.txt).
  // A launch of fewer blocks than workgroups is all last round (nfull = 0) and fills the device.
  // Gate: the average share holds a tree per wave of a workgroup, nl Lb >= waves nshares -- below
  // that a share's waves idle and its staging buys nothing; then whole blocks, as before.
  p.wgs = std::max(1, std::min(nmain, wgs_cap));
  p.tail_slices = 1;
  if (tail_balance && nmain % wgs_cap != 0) {
    const int lb = nmain % wgs_cap;
    const int nshares = wgs_cap * share_rounds;
    if ((int64_t)nl * lb >= (int64_t)eval_waves(p.R, p.K) * nshares &&
        (int64_t)lb * units * nshares < ((int64_t)1 << 31)) {
      p.wgs = wgs_cap;
      p.tail_slices = units;
      p.tail_blocks = lb;
      p.tail_shares = nshares;
    }
  }
  p.expect_items = nmain - p.tail_blocks + p.tail_shares;
  // the hot form (FORM_HOT; launch_eval_f32w takes it when the launch carries records): this launch of
  // the wide Float32 loss kernel, slab results, no diagnostics, every slab index in 32 bits
  p.hot = p.R == R_F32_WIDE && p.K == 2 && in.have_recs && !p.fused && !trace && dstop == 0 && in.loss_kind >= 0 &&
          in.loss_kind < 256 && (int64_t)nl * L.nrb * p.cpb < ((int64_t)1 << 31) && !no_hot;
  return p;
}

LossxPlan srhip::plan_eval_lossx(const LossxPlanIn& in) {
  LossxPlan p{};
  const size_t es = dtype_size(in.dtype);
  const int32_t nl = std::max<int32_t>(1, in.nlive);
  const int64_t m = std::max<int64_t>(1, in.m);
  p.rb_rows = LOSSX_BLOCK_ROWS;
  p.R = in.dtype == SRHIP_F64 ? R_F64 : R_F32;
  const int waves = eval_waves(p.R, K_MAX);
  p.nblocks = lossx_blocks(m);
  // the device's LDS less 8 KB for the interpreter's static arrays, as plan_eval's one-workgroup-per-CU budget
  p.lds_budget = (size_t)std::max<int64_t>(0, in.lds_max - 8 * 1024);
  p.lds_cols = (size_t)std::max<int32_t>(0, in.maxfeat) * p.rb_rows * es;
  p.xlds = p.lds_cols <= p.lds_budget;
  p.lds = (p.xlds ? p.lds_cols : 0) + 16;
  // two trees per wave of an item (the waves claim them costliest first, so they end within a cheap tree of
  // each other, and a staged block serves 16 trees); one per wave while that leaves workgroups without an item
  p.tpg = 2 * waves;
  if (p.nblocks * ((nl + p.tpg - 1) / p.tpg) < 2 * (int64_t)in.num_cu) p.tpg = waves;
  p.tpg = std::min<int>(p.tpg, nl);
  p.ngroups = (nl + p.tpg - 1) / p.tpg;
  // one workgroup per CU: at the kernel's 162-164 VGPRs in 512-thread workgroups (2 waves per SIMD) one is
  // resident, whatever LDS it stages; a second would wait for the first to end and only add a slab
  p.wg_per_cu = 1;
  const int64_t items = p.nblocks * p.ngroups;
  p.wgs = (int)std::max<int64_t>(1, std::min<int64_t>(items, (int64_t)in.num_cu * p.wg_per_cu));
  p.scratch_bytes = (size_t)p.wgs * p.tpg * p.rb_rows * es;
  return p;
}

// Tree groups of a launch (grid.y), as offsets into the order: the plan's uniform groups, or —
// when the launch spans several waves of workgroups over the chip's 2-per-CU slots — the bulk in
// g equal groups plus ~1/32 of the trees in halving tail groups (..., 32, 16, <=16).  Workgroups
// dispatch group by group, so the small ones come last and fill the slots the bulk leaves idle:
// identical workgroups over 977 row tiles x 2 groups use <= 95 % of 512 slots.  Measured on C2
// (scripts/tail_sweep.sh): uniform 2.13 ms, tail 1/32 2.04-2.06 ms, 1/16 2.10, 1/8 2.18 (every
// extra workgroup restages its rows and derived columns, so bigger tails or more bulk groups lose).
// SRHIP_NO_TAIL=1: uniform groups.
std::vector<int32_t> srhip::shape_groups(const LaunchPlan& L, int32_t ntrees, int num_cu) {
  static const bool no_tail = [] { const char* e = getenv("SRHIP_NO_TAIL"); return e && *e && *e != '0'; }();
  std::vector<int32_t> off(1, 0);
  const bool tail = !no_tail && ntrees >= 128 && (int64_t)L.groups * L.nrb > 2 * (int64_t)num_cu;
  if (!tail) {
    for (int g = 0; g < L.groups; ++g) off.push_back(std::min(ntrees, off.back() + L.tpg));
    return off;
  }
  // tuning hooks: SRHIP_TAIL_DIV (tail = trees / DIV, default 32), SRHIP_BULK_GROUPS (default: the
  // plan's), SRHIP_TAIL_MIN (smallest tail group, default 16)
  static const int tail_div = [] { const char* e = getenv("SRHIP_TAIL_DIV"); return e && atoi(e) >= 2 ? atoi(e) : 32; }();
  static const int bulk_g = [] { const char* e = getenv("SRHIP_BULK_GROUPS"); return e ? atoi(e) : 0; }();
  const int32_t tl = std::max<int32_t>(16, ntrees / tail_div), bulk = ntrees - tl;
  const int groups = bulk_g > 0 ? std::min<int>(bulk_g, std::max(1, bulk / 16)) : L.groups;
  const int32_t tpg = (bulk + groups - 1) / groups;
  while (off.back() < bulk) off.push_back(std::min(bulk, off.back() + tpg));
  static const int tail_min = [] { const char* e = getenv("SRHIP_TAIL_MIN"); return e && atoi(e) > 0 ? atoi(e) : 16; }();
  int32_t t = tl;
  while (t > tail_min) {
    const int32_t h = t / 2;
    off.push_back(off.back() + h);
    t -= h;
  }
  if (t > 0) off.push_back(off.back() + t);
  return off;
}

// trees sorted by estimated cost (desc), dealt to the groups in proportion to their sizes (each
// tree to the group with the largest free fraction), so every group gets the same cost mix;
// returns order [ntrees], group g's trees at [goff[g], goff[g+1])
std::vector<int32_t> srhip::make_order(const srhip_program& P, const std::vector<int32_t>& trees,
                                       const std::vector<int32_t>& goff, bool derived) {
  std::vector<int32_t> s(trees);
  auto cost = [&](int32_t t) { return derived ? P.dcost[t] : P.info[t].cost; };
  std::stable_sort(s.begin(), s.end(), [&](int32_t a, int32_t b) { return cost(a) > cost(b); });
  const int groups = (int)goff.size() - 1;
  std::vector<int32_t> order(s.size());
  std::vector<int> fill(groups, 0);
  for (int32_t t : s) {
    int best = -1;
    double bf = -1.0;
    for (int g = 0; g < groups; ++g) {
      const int cap = goff[g + 1] - goff[g];
      if (fill[g] >= cap) continue;
      const double f = (double)(cap - fill[g]) / cap;
      if (f > bf) {
        bf = f;
        best = g;
      }
    }
    order[(size_t)goff[best] + fill[best]++] = t;
  }
  return order;
}

// The hot form's slot records (SlotRec: what a wave reads per tree, in one scalar load) behind an
// order and its group offsets: [order | goff | pad to 16 bytes | records], one upload.  The records
// belong to the plan the order was made for: pc0 and the mask are the derived-column program's when
// that plan evaluates it.  Returns the records' offset in int32 units.
int srhip::append_slot_records(const srhip_program& P, std::vector<int32_t>& order, int nl, bool derived) {
  while (order.size() % 4 != 0) order.push_back(0);
  const int at = (int)order.size();
  order.resize((size_t)at + 4 * (size_t)nl);
  for (int sl = 0; sl < nl; ++sl) {
    const int32_t t = order[sl];
    const uint64_t m = derived ? P.dmask[t] : 0;
    int32_t* r = order.data() + at + 4 * (size_t)sl;
    r[0] = t;
    r[1] = derived ? P.dprog_off[t] : P.prog_off[t];
    r[2] = (int32_t)(uint32_t)m;
    r[3] = (int32_t)(uint32_t)(m >> 32);
  }
  return at;
}

// ---- the plan as the tests see it (include/srhip.h) ------------------------------------------------
extern "C" int srhip_plan_eval_lossx(const srhip_lossx_plan_query* q, srhip_lossx_plan_info* out) {
  if (!q || !out || q->nlive < 0 || q->m <= 0 || q->maxfeat < 0 || q->num_cu <= 0 || q->lds_max <= 0 ||
      (q->dtype != SRHIP_F32 && q->dtype != SRHIP_F64))
    return -1;
  const LossxPlan p = plan_eval_lossx(LossxPlanIn{q->dtype, q->nlive, q->m, q->maxfeat, q->num_cu, q->lds_max});
  *out = srhip_lossx_plan_info{};
  out->rb_rows = p.rb_rows;
  out->R = p.R;
  out->xlds = p.xlds;
  out->tpg = p.tpg;
  out->ngroups = p.ngroups;
  out->wgs = p.wgs;
  out->wg_per_cu = p.wg_per_cu;
  out->nblocks = p.nblocks;
  out->lds = (int64_t)p.lds;
  out->lds_cols = (int64_t)p.lds_cols;
  out->lds_budget = (int64_t)p.lds_budget;
  out->scratch_bytes = (int64_t)p.scratch_bytes;
  return 0;
}

extern "C" int srhip_plan_eval(const srhip_plan_query* q, srhip_plan_info* out) {
  if (!q || !out || q->nlive < 0 || q->m <= 0 || q->num_cu <= 0 || q->lds_max <= 0 || q->maxfeat < 0 || q->nd < 0 ||
      (q->dtype != SRHIP_F32 && q->dtype != SRHIP_F64 && q->dtype != SRHIP_I32) ||
      (q->mode != MODE_LOSS && q->mode != MODE_PRED && q->mode != MODE_PRECISE))
    return -1;
  EvalPlanIn in{};
  in.dtype = q->dtype;
  in.mode = q->mode;
  in.nlive = q->nlive;
  in.m = q->m;
  in.maxfeat = q->maxfeat;
  in.nd = q->nd;
  in.kmax = q->kmax;
  in.dkmax = q->dkmax;
  in.wide_ops = q->wide_ops != 0;
  in.weighted = q->weighted != 0;
  in.sharded = q->sharded != 0;
  in.have_recs = q->have_recs != 0;
  in.loss_kind = q->loss_kind;
  in.num_cu = q->num_cu;
  in.lds_max = q->lds_max;
  const EvalPlan p = plan_eval(in);
  out->kind = p.kind;
  out->R = p.R;
  out->K = p.K;
  out->use_d = p.use_d;
  out->rb_rows = p.L.rb_rows;
  out->nrb = p.L.nrb;
  out->groups = p.L.groups;
  out->tpg = p.L.tpg;
  out->xlds = p.L.xlds;
  out->lds = (int64_t)p.L.lds;
  out->nch = p.nch;
  out->cpb = p.cpb;
  out->wg_waves = p.wg_waves;
  out->probe_blocks = p.probe_blocks;
  out->wgs = p.wgs;
  out->probe_tile_claims = p.probe_tile_claims;
  out->tail_slices = p.tail_slices;
  out->tail_blocks = p.tail_blocks;
  out->tail_shares = p.tail_shares;
  out->expect_items = p.expect_items;
  out->fused = p.fused;
  out->hot = p.hot;
  return 0;
}
