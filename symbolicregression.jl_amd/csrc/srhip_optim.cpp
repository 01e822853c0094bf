// srhip_optim.cpp — constant gradients and the batched constant optimizer of libsrhip.so.
//
// srhip_eval_loss_grad: loss + exact d loss / d constants for every tree of a program (one launch of
//   the dual-number kernel, srhip_grad.hip, over (tree, constant-chunk) pairs).
// srhip_optimize_constants: optimize_constants / _optimize_constants (src/ConstantOptimization.jl:
//   11-81) for a whole population at once.  dispatch_optimize_constants (:22-41) picks the method
//   per tree: no constants -> untouched; one constant -> Optim.Newton(linesearch=BackTracking());
//   otherwise options.optimizer_algorithm = BFGS(linesearch=BackTracking()) (src/Options.jl:429-431).
//   LineSearches' BackTracking: order 3, c1 = 1e-4, rho in [0.1, 0.5]; `iterations` iterations per
//   start (Optim.Options(iterations = 8), src/Options.jl:691-705) from the current constants and from
//   `nrestarts` perturbed starts x0 .* (1 + randn/2); a tree's constants are replaced only if the best
//   minimum beats its baseline loss (:70-78).  Every tree runs its own state machine and each kernel
//   launch evaluates the one point every still-active tree needs next.  The state machine (BFGS, Newton,
//   BackTracking, best of the starts, value-only trials, the speculative run-ahead) is the device-free
//   unit srhip_bfgs.h / srhip_bfgs.cpp; this file holds its device evaluator (DeviceEvaluator: constants
//   into the program, speculative slots, eval_grad) and the driver that joins the two (bfgs_pipelined).
//   Differences from the reference, by design: exact (dual-number) gradients instead of Optim's
//   finite differences, and Newton's Hessian as a central difference of those exact gradients instead
//   of a second difference of losses -- parity is on the optimised loss, SURVEY.md 8(a) A13.
// srhip_eval_loss_grad_rowsets / srhip_optimize_constants_rowsets: the same two with one row subset per
//   tree (the batching mode's batch_sample per member, src/ConstantOptimization.jl:14-17): the optimiser's
//   evaluation primitive (eval_grad_items) runs every item on its tree's own set (RowsetBackend over
//   srhip_grad_rowsets.hip, in place of ViewBackend over srhip_grad.hip), everything above it is the
//   one code path.
#include <algorithm>
#include <numeric>
#include <chrono>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include "srhip_bfgs.h"
#include "srhip_grad.h"
#include "srhip_grad_lossx.h"
#include "srhip_internal.h"
#include "srhip_decide.h"

using namespace srhip;

namespace {

// Launch geometry of the dual-number kernel: row blocks of a fixed size (SRHIP_GRAD_RB, default 256
// rows = 4 tiles per wave, fewer for smaller datasets), independent of how many chunks a launch
// carries -- a tree's per-block partial sums, and so its loss and gradient bits, depend on the dataset
// alone -- and enough tree groups to fill the chip.  The optimiser's last rounds evaluate a handful
// of trees: small blocks keep those launches short (many workgroups, each a few tiles deep).
LaunchPlan grad_plan(const srhip_ctx* ctx, int64_t m, int32_t nchunks) {
  static const int rb_env = [] { const char* e = getenv("SRHIP_GRAD_RB"); return e ? atoi(e) : 0; }();
  int rb = (rb_env >= 256 && rb_env <= 4096 && (rb_env & (rb_env - 1)) == 0) ? rb_env : 256;
  m = std::max<int64_t>(1, m);
  while (rb > 256 && rb / 2 >= m) rb /= 2;  // >= 256: the value-only pass runs 4 rows per lane
  LaunchPlan L{};
  L.rb_rows = rb;
  L.nrb = (int)((m + rb - 1) / rb);
  L.xlds = false;
  L.lds = 0;
  const int target_blocks = 4 * ctx->num_cu;
  int g = (target_blocks + L.nrb - 1) / L.nrb;
  g = std::max(1, std::min(g, std::max(1, nchunks / (2 * GRAD_WAVES))));
  L.tpg = (std::max(1, nchunks) + g - 1) / g;
  L.groups = (std::max(1, nchunks) + L.tpg - 1) / L.tpg;
  return L;
}

// constant offsets (get_constants order) of every tree: coff[t] .. coff[t+1]
std::vector<int64_t> const_offsets(const srhip_program& P) {
  std::vector<int64_t> c(P.ntrees + 1, 0);
  for (int32_t t = 0; t < P.ntrees; ++t) c[t + 1] = c[t] + P.info[t].nconst;
  return c;
}

std::vector<double> get_all_consts(const srhip_program& P) {
  std::vector<double> out(const_offsets(P).back());
  double* c = out.data();
  for (int32_t t = 0; t < P.ntrees; ++t) get_consts(P.nodes.data() + P.offsets[t], 0, c);
  return out;
}
void set_all_consts(srhip_program& P, const double* c) {
  for (int32_t t = 0; t < P.ntrees; ++t) set_consts(P.nodes.data() + P.offsets[t], 0, c);
  P.grad_ready = false;
  P.ghint.clear();  // every tree may have changed
}

}  // namespace

// Loss and gradient for `trees` (f[t] = +Inf where did_succeed fails or is undecided); gradients
// land at g[coff[t] ..].  The gradient program must match the program's current constants.
// SRHIP_OPTIM_TIMING=1: host-side time split of the optimiser (compile/patch vs the rest), stderr
static thread_local double g_t_compile = 0.0, g_t_eval = 0.0, g_t_host = 0.0;
static thread_local double g_patch_copy_s = 0.0;  // of g_t_compile: the patched uploads (the scans: g_patch_scan_s)
static thread_local int64_t g_n_launch = 0;
static thread_local bool g_stats_on = false;
static thread_local bool g_launch_log = false;  // SRHIP_OPTIM_TIMING=3: one stderr line per launch (caller's group)
static thread_local int64_t g_hist[5] = {0, 0, 0, 0, 0}, g_nonfinite_trials = 0;
static thread_local int64_t g_spec_launched = 0, g_spec_used = 0;  // speculative trial points
// (SRHIP_OPTIM_TIMING=2) evaluated items by pass (0 gradient, 1 value-only) and launch size (items
// <= 64 / > 64): [pass][big][all, non-finite f]
static thread_local int64_t g_items[2][2][2] = {};
// One gradient evaluation of the launch: program slot `slot` (a tree, or a speculative slot holding
// tree `tree` at other constants) -> f (+Inf where did_succeed fails), g[0 .. nconst of tree), ok.
struct GradItem {
  int32_t slot, tree;
  double* f;
  double* g;     // unused for value_only items
  uint8_t* ok;   // nullable
  bool value_only = false;  // loss only (a line-search trial point): the cheap KT = 0 kernel
};
// The derived view of constant-gradient launches (GMODE_LOSS: the optimiser and srhip_eval_loss_grad):
// X' = [the program's feature columns | its derived columns U(X[f]) | their tangent-zero columns] in
// the context's g_xd, built once per call (one copy + one launch; reused by the next call over the
// same dataset and spec), so a gradient program reads every heavy operator of a feature as a column
// instead of evaluating it per row, per trial point (C4: ~0.9 per tree, cos / exp of a feature).
// Off below SRHIP_GRAD_DERIVED_MIN_ROWS rows (default 8192), above SRHIP_GRAD_DERIVED_MAX_MB of view
// (default 256) and with SRHIP_GRAD_DERIVED=0.
static int derived_view(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, View& v) {
  P->g_want_derived = false;
  const char* e = env_get("SRHIP_GRAD_DERIVED");
  if (e && *e == '0') return SRHIP_OK;
  if (v.m < env_int("SRHIP_GRAD_DERIVED_MIN_ROWS", 8192)) return SRHIP_OK;
  grad_derived_spec(*P);
  const int nd = (int)P->gdspec.size();
  if (nd == 0 || P->gdbase <= 0) return SRHIP_OK;
  const size_t es = P->dtype == SRHIP_F64 ? 8 : 4;
  const size_t bytes = (size_t)(P->gdbase + 2 * nd) * v.ld * es;
  if (bytes > ((size_t)env_int("SRHIP_GRAD_DERIVED_MAX_MB", 256) << 20)) return SRHIP_OK;  // (a copy per call)
  // a view of the whole dataset (not a gathered batch) with the same spec as the last build: reused
  const bool whole = v.X == ds->X.p;
  const bool same = whole && ctx->g_xd.p && ctx->g_xd_serial == ds->serial && ctx->g_xd_ld == v.ld &&
                    ctx->g_xd_dtype == P->dtype && ctx->g_xd_base == P->gdbase && ctx->g_xd_spec == P->gdspec;
  if (!same) {
    ctx->g_xd_serial = 0;  // (until rebuilt)
    HIP_TRY(ctx->g_xd.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(ctx->g_xd.p, v.X, (size_t)P->gdbase * v.ld * es, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(launch_grad_derive(P->dtype, v.X, (uint8_t*)ctx->g_xd.p + (size_t)P->gdbase * v.ld * es, v.ld,
                               P->gdspec.data(), nd, ctx->stream));
    // the split optimiser's auxiliary contexts read the view from their own streams: it must be
    // complete before this returns (as make_view's is), not merely queued on ctx->stream
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (C4 unchanged: 141.7-142.5 ms without it, 142.5-144.3 with)
    if (whole) {
      ctx->g_xd_serial = ds->serial;
      ctx->g_xd_ld = v.ld;
      ctx->g_xd_dtype = P->dtype;
      ctx->g_xd_base = P->gdbase;
      ctx->g_xd_spec = P->gdspec;
    }
  }
  v.X = ctx->g_xd.p;
  v.nfeat_x = P->gdbase;
  v.nd_x = nd;
  P->g_want_derived = true;
  return SRHIP_OK;
}

// The row-set batch of one call (srhip_eval_loss_grad_rowsets / srhip_optimize_constants_rowsets): every
// tree's own row subset, gathered once into a packed device buffer, with the per-set statistics the
// decisions need.  Where a batch is given it replaces the View: item (slot, tree) is evaluated on tree's
// set by grad_rowsets_kernel (RowsetBackend) instead of on the view's rows.
struct RowsetBatch {
  const int64_t* row_off = nullptr;  // the caller's [ntrees + 1] offsets and row indices (validated)
  const int64_t* rows = nullptr;
  std::vector<uint8_t> staged;       // [ntrees] the set fits a wave's LDS region (others: the single-idx path)
  std::vector<int32_t> m;            // [ntrees] rows of each set
  std::vector<FeatStat> fstat;       // [ntrees][nfeat] each staged set's feature statistics
  std::vector<double> wsum;          // [ntrees] each staged set's weight sum (weighted datasets)
  const void* packed = nullptr;      // device: the packed sets (GradRowsetArgs)
  const int64_t* d_set_off = nullptr;
  const int32_t* d_set_m = nullptr;
};
// One chunk of a launch, on the host: program slot, first constant, the item it reports to and that
// item's tree (which names the row set where there is one).  A backend flattens it to its device list.
struct Chunk {
  int32_t slot, c0, item, tree;
  int32_t pos;  // its index in the pass as the items list it: the same on every rank, whatever the launch order
};
// One row-sharded call (srhip_eval_loss_grad_sharded / srhip_optimize_constants_sharded): its exchanges and what
// the call-start exchange gave -- the weight sum (or row count) over all ranks, and the decision inputs over all
// ranks' rows.  Every evaluation of the call divides by the one and decides from the other.
struct GradShardCall {
  const GradShardIO* io = nullptr;
  double wsum = 0.0;
  std::vector<double> tail;  // [per feature {column sum, non-finite count} | rows], the partials layout's tail
};
// What an evaluation does besides the plain one-device call (both null): a row shard's exchange, or the raw
// records of srhip_eval_loss_grad_partials -- sums undivided, no decision, every tree's statistic to raw_chk[tree]
struct GradExtra {
  const GradShardCall* sh = nullptr;
  double* raw_chk = nullptr;
};
// The two passes of an evaluation (gradient chunks of kt tangents, then value-only chunks: kt = 0)
struct GradPass {
  int kt;
  std::vector<Chunk> chunks;    // in launch order once the backend has prepared the pass
  const double* red = nullptr;  // the reduced records, (kt + 2) doubles per chunk by position (pinned staging)
};
// eval_grad_items' backends supply what differs between "every item on the view's rows" and "every item on
// its tree's own row set":
//   prepare(pass)           launch order of both passes' chunks, device buffers sized for both before the
//                           first launch (no reallocation under a queued kernel)
//   launch(pi, ps, ev0)     the pass's chunk list and kernels on the stream, its records written to
//                           ctx->h_gred[pi]; ev0 (nullable) recorded in front of the kernels
//   host_records()          the launch writes its records to ctx->h_gred[pi] (false: collect() sets each pass's red)
//   collect(pass)           the one host wait of the evaluation; every pass's red is readable after it
//   wsum(it)                the weight sum the item's records are divided by
//   decide(it, chk)         the item's status (0 ok, 1 fail, 2 undecided) from its check statistic
//   settle(items, und, ok)  the precise pass for the undecided items `und`: ok[u] for items[und[u]]

// Every item on the view's rows (srhip_grad.hip): row blocks x chunk groups, reduced by a second kernel.
// With a row shard's exchange (ex.sh) the view is this rank's rows: the reduction is the shard form, into the
// exchange's device buffer; collect is the exchange (its stream waits for the kernels through an event, the host
// waits once, for the reduced copy); the weight sum and the decision inputs are the call's global ones; settle
// sums the precise pass's per-operator sums over the ranks before the verdict.  Every rank builds the same
// passes -- the items are a function of the reduced values alone -- and a chunk's place in the exchange is its
// Chunk::pos, not its place in this rank's launch order.
struct ViewBackend {
  srhip_ctx* ctx;
  const srhip_dataset* ds;
  srhip_program* P;
  LossSel loss;  // built-in kind, or an expression program
  const View& v;
  GradExtra ex = {};
  LaunchPlan L[2] = {};
  std::vector<double> sums;  // decision inputs: only the feature statistics and the row count are read
  // a row shard's round: the exchange's device buffer, each pass's segments in it (in doubles), and the
  // reduced records put back into (kt + 2) doubles per chunk by launch position
  double* xbuf = nullptr;
  GradShardLayout xl;
  size_t sum_off[2] = {0, 0}, chk_off[2] = {0, 0};
  std::vector<double> xred[2];

  int prepare(GradPass (&pass)[2]) {
    sums.assign(sums_len(P->ntrees, ds->nfeat), 0.0);
    if (ex.sh) std::copy(ex.sh->tail.begin(), ex.sh->tail.end(), sums.begin() + 2 * (size_t)P->ntrees);
    else fill_decide_inputs(sums.data(), P->ntrees, ds->nfeat, v.stats, v.m);
    if (ex.sh) {
      const size_t n0 = pass[0].chunks.size(), n1 = pass[1].chunks.size();
      sum_off[0] = 0;
      sum_off[1] = n0 * (pass[0].kt + 1);
      xl.dtype = P->dtype;
      xl.nsum = sum_off[1] + n1 * (pass[1].kt + 1);
      chk_off[0] = xl.nsum;
      chk_off[1] = xl.nsum + n0;
      xl.nchk = n0 + n1;
      void* d = nullptr;
      const int rc = ex.sh->io->buffer(xl.bytes(), &d);
      if (rc) return rc;
      xbuf = (double*)d;
    }
    size_t slab_n = 0, red_n = 0, chunk_n = 0;
    for (int pi = 0; pi < 2; ++pi) {
      GradPass& ps = pass[pi];
      const int nch = (int)ps.chunks.size();
      if (nch == 0) continue;
      L[pi] = grad_plan(ctx, v.m, nch);
      // launch order: descending estimated cost, dealt round-robin over the tree groups (each group's
      // range stays contiguous), so every group gets the same cost mix and its waves -- which claim
      // chunks dynamically -- start with the longest ones.  Records are read back by position.
      if (nch > 1) {
        std::vector<int32_t> by(nch);
        std::iota(by.begin(), by.end(), 0);
        std::stable_sort(by.begin(), by.end(), [&](int32_t x, int32_t y) {
          return P->ginfo[ps.chunks[x].slot].cost > P->ginfo[ps.chunks[y].slot].cost;
        });
        const int G = L[pi].groups, tpg = L[pi].tpg;
        std::vector<int32_t> fill(G, 0);
        std::vector<Chunk> dealt(nch);
        int g = 0;
        for (int32_t k : by) {
          while (fill[g] >= std::min(tpg, nch - g * tpg)) g = (g + 1) % G;
          dealt[g * tpg + fill[g]++] = ps.chunks[k];
          g = (g + 1) % G;
        }
        ps.chunks.swap(dealt);
      }
      slab_n = std::max(slab_n, (size_t)nch * L[pi].nrb * (ps.kt + 2));
      red_n = std::max(red_n, (size_t)nch * (ps.kt + 2));
      chunk_n = std::max(chunk_n, (size_t)(ex.sh ? 3 : 2) * nch);  // (a shard: the exchange positions behind the list)
    }
    HIP_TRY(ctx->g_chunks.ensure(chunk_n * sizeof(int32_t)));
    HIP_TRY(ctx->g_slab.ensure(slab_n * sizeof(double)));
    if (!ex.sh) HIP_TRY(ctx->g_red.ensure(red_n * sizeof(double)));  // (a shard's records go to the exchange's buffer)
    return SRHIP_OK;
  }

  int launch(int pi, const GradPass& ps, hipEvent_t ev0) {
    const int dtype = P->dtype;
    const bool weighted = ds->weighted;
    const int nch = (int)ps.chunks.size();
    const LaunchPlan& Lp = L[pi];
    const int K = P->gkmax <= 2 ? 2 : (P->gkmax <= 4 ? 4 : 8);  // stack slots of the kernel variant
    GradArgs a{};
    // SRHIP_GRAD_INLINE_MAX (0: always copy the list), read per pass through the environment cache
    // so a test can compare both forms in one process
    // (a shard always copies: its list carries every chunk's exchange position behind the (slot, c0) pairs)
    const bool inl = !ex.sh && nch <= std::max(0, std::min(env_int("SRHIP_GRAD_INLINE_MAX", GRAD_INLINE), GRAD_INLINE));
    // the device list, (slot, c0) per chunk: in the kernel arguments, or through pinned staging (a pageable
    // source makes the runtime stage the copy through its own buffer, synchronously); stream order: the
    // copy follows the previous pass's kernel, which has read its chunk list
    const size_t list_bytes = (size_t)(ex.sh ? 3 : 2) * nch * sizeof(int32_t);
    if (!inl) HIP_TRY(ctx->h_gchunks[pi].ensure(list_bytes));
    int32_t* const list = inl ? a.inl : (int32_t*)ctx->h_gchunks[pi].p;
    for (int c = 0; c < nch; ++c) {
      list[2 * c] = ps.chunks[c].slot;
      list[2 * c + 1] = ps.chunks[c].c0;
      if (ex.sh) list[2 * nch + c] = ps.chunks[c].pos;
    }
    if (!inl) HIP_TRY(hipMemcpyAsync(ctx->g_chunks.p, list, list_bytes, hipMemcpyHostToDevice, ctx->stream));
    a.code = (const Ins*)P->d_gcode.p;
    a.prog_off = (const int32_t*)P->d_goff.p;
    a.chunks = inl ? nullptr : (const int32_t*)ctx->g_chunks.p;
    a.X = v.X;
    a.y = v.y;
    a.w = weighted ? v.w : nullptr;
    a.slab = (double*)ctx->g_slab.p;
    a.ld = v.ld;
    a.nvalid = v.m;
    a.nchunks = nch;
    a.nfeat = v.nfeat_x >= 0 ? v.nfeat_x : (int32_t)ds->nfeat;
    a.gd_nd = v.nd_x;
    a.rb_rows = Lp.rb_rows;
    a.nrb = Lp.nrb;
    a.chunks_per_group = Lp.tpg;
    a.loss_kind = loss.kind ? loss.kind->kind : 0;  // (an expression: its program travels beside these arguments)
    a.loss_p0 = loss.kind ? loss.kind->p0 : 0.0;
    a.weighted = weighted ? 1 : 0;
    a.max_steps = P->gmax_len;
    // the kernel by the loss selector: grad_kernel, or grad_lossx_kernel with the same arguments and grid
    auto launch_k = [&](int kt, const GradArgs& ga, dim3 grid) {
      return loss.expr ? launch_grad_lossx(dtype, K, kt, ga, *loss.expr, grid, ctx->stream)
                       : launch_grad(dtype, K, kt, ga, grid, ctx->stream);
    };
    if (ev0) HIP_TRY(hipEventRecord(ev0, ctx->stream));  // srhip_last_kernel_ms: the gradient kernels
    // value-only screening (SRHIP_GRAD_SCREEN = the fewest value-only chunks screened; default 0 =
    // off): row block 0 of every chunk first, in a launch of its own, then the other blocks, where a
    // chunk whose block-0 check statistic is already non-finite is skipped.  Records of evaluated
    // blocks are the same computation as in one launch, so losses and decisions are bit-identical
    // (test_value_only_screening_is_exact).  C4 (~40 % of its trial points overflow), same box:
    // off 173.6-177.9 ms, every pass 190-193, passes of >= 16 chunks 176.8-179.6 -- the extra launch
    // costs what the skipped blocks save at 100k rows.
    // (ignored on a row shard: which chunks a rank screens out depends on its own rows)
    const int screen_min = ex.sh ? 0 : env_int("SRHIP_GRAD_SCREEN", 0);
    if (ps.kt == 0 && screen_min > 0 && nch >= screen_min && Lp.nrb > 1) {
      GradArgs sa = a;
      const int tpg_s = 2 * GRAD_WAVES;
      sa.chunks_per_group = tpg_s;
      HIP_TRY(launch_k(0, sa, dim3(1, (nch + tpg_s - 1) / tpg_s)));
      a.block0 = 1;
      a.screened = 1;
      HIP_TRY(launch_k(0, a, dim3(Lp.nrb - 1, Lp.groups)));
    } else {
      HIP_TRY(launch_k(ps.kt, a, dim3(Lp.nrb, Lp.groups)));
    }
    if (ex.sh) {  // a row shard: the same fold, into the exchange's device buffer at the chunks' exchange positions
      HIP_TRY(launch_grad_reduce_shard(dtype, ps.kt, (const double*)ctx->g_slab.p, Lp.nrb, nch,
                                       (const int32_t*)ctx->g_chunks.p + 2 * nch, xbuf + sum_off[pi], xbuf + chk_off[pi],
                                       ctx->stream));
      return SRHIP_OK;
    }
    // the reduction writes the records straight into coherent pinned host memory (no copy on the stream)
    HIP_TRY(launch_grad_reduce(dtype, ps.kt, (const double*)ctx->g_slab.p, Lp.nrb, nch, (double*)ctx->h_gred[pi].p,
                               ctx->stream));
    return SRHIP_OK;
  }

  bool host_records() const { return !ex.sh; }

  int collect(GradPass (&pass)[2]) {
    if (!ex.sh) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      return SRHIP_OK;
    }
    // the exchange: no host wait in front of it, one behind it; then each pass's records back in the
    // (kt + 2)-per-chunk layout, by launch position
    const void* red = nullptr;
    const int rc = ex.sh->io->reduce(xl, ctx->stream, &red);
    if (rc) return rc;
    const double* const r = (const double*)red;
    for (int pi = 0; pi < 2; ++pi) {
      GradPass& ps = pass[pi];
      const size_t nch = ps.chunks.size(), w = (size_t)ps.kt + 2;
      if (nch == 0) continue;
      xred[pi].resize(nch * w);
      for (size_t c = 0; c < nch; ++c) {
        const size_t at = (size_t)ps.chunks[c].pos;
        std::copy(r + sum_off[pi] + at * (w - 1), r + sum_off[pi] + (at + 1) * (w - 1), xred[pi].begin() + c * w);
        xred[pi][c * w + w - 1] = r[chk_off[pi] + at];
      }
      ps.red = xred[pi].data();
    }
    return SRHIP_OK;
  }

  double wsum(const GradItem&) const {
    if (ex.raw_chk) return 1.0;  // (the raw sums: x / 1.0 is x)
    if (ex.sh) return ex.sh->wsum;
    return ds->weighted ? v.sum_w : (double)v.m;
  }
  int decide(const GradItem& it, double chk) {
    if (ex.raw_chk) {
      ex.raw_chk[it.tree] = chk;
      return 0;
    }
    return decide_tree(P->ginfo[it.slot], *P, ds->nfeat, sums.data(), chk);
  }

  // near-overflow sums: the exact per-operator-node pass on the gradient program decides, so the
  // objective is eval_loss's (L(Inf) exactly where did_succeed fails); one batched pass over the view
  // (a row shard: over this rank's rows, the per-operator sums summed over the ranks before the verdict)
  int settle(const std::vector<GradItem>& items, const std::vector<int32_t>& und, uint8_t* ok) {
    std::vector<int32_t> slots;
    for (int32_t ui : und) slots.push_back(items[ui].slot);
    return precise_decide(ctx, ds, P, v, slots.data(), (int32_t)slots.size(), true, ok,
                          ex.sh ? &ex.sh->io->reduce_host : nullptr);
  }
};

// Every item on its tree's own row set (srhip_grad_rowsets.hip).  One single-wave workgroup per chunk
// (slot, c0, set); the waves write the final (kt + 2) records straight into the pinned staging, so a pass
// is one launch.  Each item is decided on its own set's statistics (feature sums, non-finite counts, rows,
// weight sum); an undecided item (a near-overflow sum) is settled by the precise pass over a view gathered
// from its set.
struct RowsetBackend {
  srhip_ctx* ctx;
  const srhip_dataset* ds;
  srhip_program* P;
  LossSel loss;  // built-in kind, or an expression program
  const RowsetBatch& rb;
  int max_ld[2] = {0, 0};
  std::vector<double> sums;

  int prepare(GradPass (&pass)[2]) {
    sums.assign(sums_len(P->ntrees, ds->nfeat), 0.0);
    size_t chunk_n = 0;
    for (int pi = 0; pi < 2; ++pi) {
      GradPass& ps = pass[pi];
      for (const Chunk& c : ps.chunks) {
        if (!rb.staged[c.tree]) return fail(SRHIP_ERR_INVALID, "tree %d: its row set is not staged", (int)c.tree);
        max_ld[pi] = std::max(max_ld[pi], (rb.m[c.tree] + GRAD_ROWSET_RB - 1) / GRAD_ROWSET_RB * GRAD_ROWSET_RB);
      }
      // launch order: descending set length x tree cost
      auto weight = [&](const Chunk& c) { return (double)rb.m[c.tree] * P->ginfo[c.slot].cost; };
      std::stable_sort(ps.chunks.begin(), ps.chunks.end(),
                       [&](const Chunk& x, const Chunk& y) { return weight(x) > weight(y); });
      chunk_n = std::max(chunk_n, (size_t)3 * ps.chunks.size());
    }
    HIP_TRY(ctx->g_chunks.ensure(chunk_n * sizeof(int32_t)));
    return SRHIP_OK;
  }

  int launch(int pi, const GradPass& ps, hipEvent_t ev0) {
    const int nch = (int)ps.chunks.size();
    // the device list, (slot, c0, set) per chunk, through pinned staging; stream order: the copy follows
    // the previous pass's kernel, which has read its chunk list
    const size_t list_bytes = (size_t)3 * nch * sizeof(int32_t);
    HIP_TRY(ctx->h_gchunks[pi].ensure(list_bytes));
    int32_t* const list = (int32_t*)ctx->h_gchunks[pi].p;
    for (int c = 0; c < nch; ++c) {
      list[3 * c] = ps.chunks[c].slot;
      list[3 * c + 1] = ps.chunks[c].c0;
      list[3 * c + 2] = ps.chunks[c].tree;
    }
    HIP_TRY(hipMemcpyAsync(ctx->g_chunks.p, list, list_bytes, hipMemcpyHostToDevice, ctx->stream));
    GradRowsetArgs a{};
    a.code = (const Ins*)P->d_gcode.p;
    a.prog_off = (const int32_t*)P->d_goff.p;
    a.chunks = (const int32_t*)ctx->g_chunks.p;
    a.packed = rb.packed;
    a.set_off = rb.d_set_off;
    a.set_m = rb.d_set_m;
    a.out = (double*)ctx->h_gred[pi].p;
    a.ld = 0;
    a.nchunks = nch;
    a.nfeat = (int32_t)ds->nfeat;
    a.gd_nd = 0;
    a.loss_kind = loss.kind ? loss.kind->kind : 0;  // (an expression: its program travels beside these arguments)
    a.loss_p0 = loss.kind ? loss.kind->p0 : 0.0;
    a.weighted = ds->weighted ? 1 : 0;
    a.max_steps = P->gmax_len;
    if (ev0) HIP_TRY(hipEventRecord(ev0, ctx->stream));
    // the kernel by the loss selector, as ViewBackend: grad_rowsets_kernel, or grad_rowsets_lossx_kernel
    if (loss.expr) HIP_TRY(launch_grad_rowsets_lossx(P->dtype, ps.kt, a, *loss.expr, max_ld[pi], ctx->stream));
    else HIP_TRY(launch_grad_rowsets(P->dtype, ps.kt, a, max_ld[pi], ctx->stream));
    return SRHIP_OK;
  }

  bool host_records() const { return true; }

  int collect(GradPass (&)[2]) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SRHIP_OK;
  }

  double wsum(const GradItem& it) const { return ds->weighted ? rb.wsum[it.tree] : (double)rb.m[it.tree]; }
  int decide(const GradItem& it, double chk) {
    fill_decide_inputs(sums.data(), P->ntrees, ds->nfeat, rb.fstat.data() + (size_t)it.tree * ds->nfeat, rb.m[it.tree]);
    return decide_tree(P->ginfo[it.slot], *P, ds->nfeat, sums.data(), chk);
  }

  // (rare) the exact per-operator-node pass on a view made from each item's own set
  int settle(const std::vector<GradItem>& items, const std::vector<int32_t>& und, uint8_t* ok) {
    for (size_t u = 0; u < und.size(); ++u) {
      const GradItem& it = items[und[u]];
      View v{};
      int rc = make_view(ctx, ds, rb.rows + rb.row_off[it.tree], rb.m[it.tree], true, v);
      if (rc) return rc;
      rc = precise_decide(ctx, ds, P, v, &it.slot, 1, true, ok + u);
      if (rc) return rc;
    }
    return SRHIP_OK;
  }
};

// The evaluation primitive: every item's loss (+Inf where did_succeed fails), gradient and ok, in two
// passes on the stream (gradient chunks, then value-only chunks) and one synchronisation.
// timed: HIP events around the gradient kernels (srhip_last_kernel_ms).  The optimiser's launches go
// without: two timing events per launch cost C4 ~5 % (149-153 against 141-145 ms on one box).
template <class Backend>
static int eval_grad_items_on(srhip_ctx* ctx, srhip_program* P, Backend& be, const std::vector<GradItem>& items,
                              bool timed) {
  // tangent width of the gradient pass: a chunk carries the primal plus kt tangents, so trees with
  // few constants waste most of an 8-wide chunk; estimated cost per chunk ~ (3 + kt) (the primal's
  // transcendentals and derivative factors cost about three tangent updates).  Values and the
  // tangents of each constant do not depend on kt (independent components, same primal code; kt = 0
  // is the value-only pass).
  int64_t cost4 = 0, cost8 = 0;
  for (const GradItem& it : items) {
    if (P->ginfo[it.slot].static_fail || it.value_only) continue;
    const int nc = std::max(P->info[it.tree].nconst, 1);
    cost4 += (int64_t)((nc + 3) / 4) * (3 + 4);
    cost8 += (int64_t)((nc + GRAD_KT - 1) / GRAD_KT) * (3 + GRAD_KT);
  }
  const char* kte = env_get("SRHIP_GRAD_KT");  // tuning / tests: force 4 or 8
  int kt = cost4 < cost8 ? 4 : GRAD_KT;
  if (kte && (atoi(kte) == 4 || atoi(kte) == GRAD_KT)) kt = atoi(kte);
  GradPass pass[2];
  pass[0].kt = kt;
  pass[1].kt = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    const GradItem& it = items[i];
    *it.f = INFINITY;
    if (it.ok) *it.ok = 0;
    const int nc = P->info[it.tree].nconst;
    if (!it.value_only)
      for (int k = 0; k < nc; ++k) it.g[k] = 0.0;
    if (P->ginfo[it.slot].static_fail) continue;
    GradPass& ps = pass[it.value_only ? 1 : 0];
    const int span = it.value_only ? 1 : std::max(nc, 1);
    for (int c0 = 0; c0 < span; c0 += std::max(ps.kt, 1))
      ps.chunks.push_back(Chunk{it.slot, c0, (int32_t)i, it.tree, (int32_t)ps.chunks.size()});
  }
  if (pass[0].chunks.empty() && pass[1].chunks.empty()) {  // a patched gradient program may still be uploading from P->gcode
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SRHIP_OK;
  }
  int rc = be.prepare(pass);
  if (rc) return rc;
  bool first = true;
  for (int pi = 0; pi < 2; ++pi) {
    GradPass& ps = pass[pi];
    if (ps.chunks.empty()) continue;
    // the records' home: the context's coherent staging, which the reduction writes -- or, on a row shard,
    // the exchange's reduced copy, which collect() points ps.red at
    const bool staged = be.host_records();
    if (staged) HIP_TRY(ctx->h_gred[pi].ensure(ps.chunks.size() * (ps.kt + 2) * sizeof(double), hipHostMallocCoherent));
    rc = be.launch(pi, ps, first && timed ? ctx->ev0 : nullptr);
    if (rc) return rc;
    first = false;
    if (staged) ps.red = (const double*)ctx->h_gred[pi].p;
  }
  if (timed) HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = timed;
  ctx->last_ev0 = ctx->ev0;
  ctx->last_ev1 = ctx->ev1;
  rc = be.collect(pass);
  if (rc) return rc;
  std::vector<int32_t> undecided;  // items
  for (const GradPass& ps : pass) {
    const int nch = (int)ps.chunks.size();
    for (int c = 0; c < nch; ++c) {
      const Chunk& ch = ps.chunks[c];
      const GradItem& it = items[ch.item];
      const double* r = ps.red + (size_t)c * (ps.kt + 2);
      const int nc = P->info[it.tree].nconst;
      const double wsum = be.wsum(it);
      for (int j = 0; j < ps.kt && ch.c0 + j < nc; ++j) it.g[ch.c0 + j] = r[1 + j] / wsum;
      if (ch.c0 == 0) {
        const int st = be.decide(it, r[ps.kt + 1]);
        *it.f = st == 1 ? INFINITY : r[0] / wsum;
        if (it.ok) *it.ok = st != 1;
        if (st == 2) undecided.push_back(ch.item);
      }
    }
  }
  if (g_stats_on)
    for (const GradItem& it : items) {
      int64_t* c = g_items[it.value_only ? 1 : 0][items.size() > 64 ? 1 : 0];
      c[0] += 1;
      c[1] += !std::isfinite(*it.f);
    }
  if (!undecided.empty()) {
    std::vector<uint8_t> uok(undecided.size());
    rc = be.settle(items, undecided, uok.data());
    if (rc) return rc;
    for (size_t u = 0; u < undecided.size(); ++u)
      if (!uok[u]) {
        const GradItem& it = items[undecided[u]];
        *it.f = INFINITY;
        if (it.ok) *it.ok = 0;
      }
  }
  return SRHIP_OK;
}
// on the view's rows, or (rb given: it replaces the view) every item on its tree's own row set
static int eval_grad_items(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const LossSel& loss,
                           const View& v, const std::vector<GradItem>& items, bool timed, const RowsetBatch* rb,
                           const GradExtra& ex) {
  if (rb) {
    RowsetBackend be{ctx, ds, P, loss, *rb};
    return eval_grad_items_on(ctx, P, be, items, timed);
  }
  ViewBackend be{ctx, ds, P, loss, v, ex};
  return eval_grad_items_on(ctx, P, be, items, timed);
}

// Instructions [lo, hi) of P's gradient program to its device copy, on ctx's stream through the pinned
// buffer `stage` (a pageable source makes the runtime stage it synchronously).  Not synchronised: the
// caller leaves `stage` and gcode[lo, hi) alone until the stream has passed the copy.
static int upload_gcode(srhip_ctx* ctx, srhip_program& P, int64_t lo, int64_t hi, HostBuf& stage) {
  if (hi <= lo) return SRHIP_OK;
  const size_t nb = (size_t)(hi - lo) * sizeof(Ins);
  HIP_TRY(stage.ensure(nb));
  memcpy(stage.p, P.gcode.data() + lo, nb);
  HIP_TRY(hipMemcpyAsync((Ins*)P.d_gcode.p + lo, stage.p, nb, hipMemcpyHostToDevice, ctx->stream));
  return SRHIP_OK;
}

// The gradient program at P's current constants, on the device: compile_grad_host (srhip_compile.cpp)
// decides between patch and full compile and does either; this uploads what its GradEdit names.
static int compile_grad_program(srhip_program& P) {
  GradEdit edit;
  int rc = compile_grad_host(P, edit);
  if (rc || edit.kind == GradEdit::NONE) return rc;
  if (!P.ctx) return fail(SRHIP_ERR_INVALID, "host-only program");
  const double t_copy0 = now_s();
  HIP_TRY(hipSetDevice(P.ctx->device));
  if (edit.kind == GradEdit::PATCHED) {  // the device copy differs only in [lo, hi)
    rc = upload_gcode(P.ctx, P, edit.lo, edit.hi, P.ctx->h_gpatch);
    if (rc) return rc;
    // no synchronisation here: the gradient launch follows on the same stream, and eval_grad
    // synchronises before it returns, so the staging is not touched while this copy is in flight
    g_patch_copy_s += now_s() - t_copy0;
  } else {
    HIP_TRY(P.d_gcode.ensure(P.gcode.size() * sizeof(Ins)));
    HIP_TRY(P.d_goff.ensure(std::max<size_t>(1, P.gprog_off.size()) * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(P.d_gcode.p, P.gcode.data(), P.gcode.size() * sizeof(Ins), hipMemcpyHostToDevice, P.ctx->stream));
    if (!P.gprog_off.empty())
      HIP_TRY(hipMemcpyAsync(P.d_goff.p, P.gprog_off.data(), P.gprog_off.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                             P.ctx->stream));
    // the sources are the program's own vectors, which the next patch or speculative slot rewrites:
    // both copies are complete before this returns
    HIP_TRY(hipStreamSynchronize(P.ctx->stream));
  }
  P.grad_ready = true;
  return SRHIP_OK;
}

// Loss and gradient for `trees` at the program's current constants: f[t], g[coff[t] ..], ok[t]
// (nullable; did_succeed -- a tree can succeed with an overflowing loss: f = Inf, ok = 1), plus the
// items in `extra` (speculative slots, already instantiated; their instructions [spec_lo, spec_hi)
// are uploaded with the launch).
static int eval_grad(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const LossSel& loss, const View& v,
                     const std::vector<int32_t>& trees, const std::vector<int64_t>& coff, double* f, double* g,
                     uint8_t* ok = nullptr, const std::vector<GradItem>* extra = nullptr, int64_t spec_lo = 0,
                     int64_t spec_hi = -1, const uint8_t* value_only = nullptr, bool timed = true,
                     const RowsetBatch* rb = nullptr, const GradExtra& ex = GradExtra()) {
  const double t0 = now_s();
  int rc = compile_grad_program(*P);
  g_t_compile += now_s() - t0;
  g_n_launch += 1;
  if (rc) return rc;
  std::vector<GradItem> items;
  items.reserve(trees.size() + (extra ? extra->size() : 0));
  for (int32_t t : trees)
    items.push_back(GradItem{t, t, f + t, g + coff[t], ok ? ok + t : nullptr, value_only && value_only[t]});
  if (extra) items.insert(items.end(), extra->begin(), extra->end());
  auto body = [&]() -> int {
    // the speculative slots, through a staging buffer of their own: a patch's copy (compile_grad_program,
    // h_gpatch) can be in flight before the same launch; synchronised with the launch in eval_grad_items
    const int urc = upload_gcode(ctx, *P, spec_lo, spec_hi, ctx->h_gspec);
    if (urc) return urc;
    return eval_grad_items(ctx, ds, P, loss, v, items, timed, rb, ex);
  };
  rc = body();
  // a patched gradient program's upload (compile_grad_program) may still be in flight from P->gcode:
  // on an error return, drain the stream before the caller can destroy or recompile the program
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

namespace {

// The knobs of a run from the SRHIP_OPTIM_* switches, with their defaults and clamps (the state machine,
// srhip_bfgs.cpp, reads no environment)
BfgsKnobs bfgs_knobs(int iterations, double g_tol) {
  BfgsKnobs k;
  k.iterations = iterations;
  k.g_tol = g_tol;
  // value-only trial points (SRHIP_OPTIM_VALUE_TRIALS, default on)
  const char* vte = getenv("SRHIP_OPTIM_VALUE_TRIALS");
  k.value_trials = !(vte && *vte == '0');
  // SRHIP_OPTIM_SPEC, default 32 slots: a launch of a few trees is latency-bound (one tree x 100k rows fills
  // ~5 % of the wave slots), so a few dozen extra points cost little; more only adds mispredicted work
  const char* spe = getenv("SRHIP_OPTIM_SPEC");
  k.spec_slots = spe && *spe ? std::max(0, std::min(atoi(spe), 4096)) : 32;
  // speculate only in the pipeline's tail (SRHIP_OPTIM_SPEC_ACTIVE, default 64 active trees), at most
  // SRHIP_OPTIM_SPEC_DEPTH (default 64) points per tree and launch
  k.spec_max_active = std::max(0, env_int("SRHIP_OPTIM_SPEC_ACTIVE", 64));
  k.spec_max_depth = std::max(1, env_int("SRHIP_OPTIM_SPEC_DEPTH", 64));
  const char* tre = getenv("SRHIP_OPTIM_TRACE");  // SRHIP_OPTIM_TRACE=<tree>: every evaluation of one tree, stderr
  k.trace_tree = tre && *tre ? atoi(tre) : -1;
  k.stats_on = g_stats_on;  // SRHIP_OPTIM_TIMING=2 / 3, as the entry point read it for this thread
  return k;
}

// bfgs_run's evaluator on the device: each launch's points become the active trees' constants, the granted
// speculative points go to spare program slots (the tree's code with its constant immediates rewritten),
// and one eval_grad evaluates both (on the view's rows, or every tree on its own row set: rb)
struct DeviceEvaluator {
  srhip_ctx* ctx;
  const srhip_dataset* ds;
  srhip_program* P;
  const LossSel& loss;
  const View& v;
  const RowsetBatch* rb;
  GradExtra ex;  // a row shard's exchange: every evaluation of the run is one exchange
  std::vector<GradItem> sitems = {};
  int64_t spec_lo = INT64_MAX, spec_hi = -1;  // the instructions the launch's slots rewrote
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;

  int place(const BfgsBatch& b) {
    t0 = now_s();
    for (int32_t t : b.act) {  // only the active trees' constants change (get_constants order per tree)
      const double* c = b.xe.data() + b.coff[t];
      set_consts(P->nodes.data() + P->offsets[t], 0, c);
    }
    // the patch scans just the trees whose constants moved (a union if an earlier hint is pending;
    // no hint at all -- an unknown change -- keeps the full scan)
    if (P->grad_ready) P->ghint = b.act;
    else if (!P->ghint.empty()) P->ghint.insert(P->ghint.end(), b.act.begin(), b.act.end());
    P->grad_ready = false;
    spec_lo = INT64_MAX;
    spec_hi = -1;
    return SRHIP_OK;
  }
  // the slots are instantiated after the compile / patch: a full compile resets the slot region
  int slots(int* n) {
    const double tc = now_s();
    const int rc = compile_grad_program(*P);
    g_t_compile += now_s() - tc;
    *n = P->gspec_alloc;
    return rc;
  }
  bool grant(int32_t slot, int32_t t, const double* xs) {
    bool sfail = false;
    return spec_instantiate(*P, slot, t, xs, &sfail, spec_lo, spec_hi);
  }
  int evaluate(BfgsBatch& b) {
    sitems.clear();
    for (size_t i = 0; i < b.spec.size(); ++i)
      sitems.push_back(GradItem{P->ntrees + b.spec[i].slot, b.spec[i].t, &b.sf[i], b.sg.data() + b.spec[i].off, nullptr,
                                b.knobs.value_trials});
    t1 = now_s();
    const int rc = eval_grad(ctx, ds, P, loss, v, b.act, b.coff, b.fe.data(), b.ge.data(), nullptr, &sitems, spec_lo,
                             spec_hi, b.vonly.data(), /*timed=*/false, rb, ex);
    if (rc) return rc;
    if (loss.expr) {
      // an expression's loss is no failure where it is not finite (did_succeed is the tree's alone), so NaN and
      // -Inf reach here: they count as +Inf before the line search or the acceptance sees them (ls_update
      // compares with >, which a NaN would pass; BackTracking shrinks on !isfinite)
      for (int32_t t : b.act)
        if (!std::isfinite(b.fe[t])) b.fe[t] = INFINITY;
      for (double& sfv : b.sf)
        if (!std::isfinite(sfv)) sfv = INFINITY;
    }
    t2 = now_s();
    g_t_host += t1 - t0;
    g_t_eval += t2 - t1;
    return SRHIP_OK;
  }
  void launched(const BfgsBatch& b) {
    if (!g_launch_log) return;  // SRHIP_OPTIM_TIMING=3
    int nv = 0;
    for (int32_t t : b.act) nv += b.vonly[t];
    fprintf(stderr, "srhip launch: t %.3f act %zu trial %d vonly %d spec %zu used %lld host %.3f eval %.3f ms\n",
            1e3 * t2, b.act.size(), b.trials_pending(), nv, b.spec.size(), (long long)b.spec_used_last, 1e3 * (t1 - t0),
            1e3 * (t2 - t1));
  }
};

}  // namespace

// All restarts of all trees as one pipelined batch.  Every tree runs its own state machine
// (initial point -> [Hessian probes] -> line-search trials -> ... -> next restart: BfgsBatch,
// srhip_bfgs.cpp); each launch evaluates the one point every active tree needs next, so a tree never
// waits for a slower tree's line search or restart.  A tree's loss and gradient do not depend on which
// other trees share the launch (fixed row chunks, fixed reduction order), so each tree's trajectory --
// and the outcome -- is the one it would follow optimised alone (tests/test_gpu_optim.py checks this bit
// for bit).  Speculative trial points (SRHIP_OPTIM_SPEC slots, default 32, 0 = off): while few trees are
// active, the launch also evaluates, in spare program slots, the next points a failing line search would
// try; a result is consumed only where the line search really asks for exactly that point.
static int bfgs_pipelined(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const LossSel& loss,
                          const View& v, const std::vector<int32_t>& trees, const std::vector<int64_t>& coff,
                          int iterations, double g_tol, const std::vector<std::vector<double>>& starts,
                          std::vector<double>& best_x, std::vector<double>& best_f, std::vector<int64_t>& fcalls,
                          const RowsetBatch* rb = nullptr, const GradShardCall* sh = nullptr) {
  const BfgsKnobs knobs = bfgs_knobs(iterations, g_tol);
  BfgsBatch batch(P->ntrees, trees, coff, starts, knobs, best_x, best_f, fcalls);
  if (P->gspec_cap != knobs.spec_slots) {
    P->gspec_cap = knobs.spec_slots;  // the next gradient compile allocates the slots (a full compile)
    P->grad_ready = false;
  }
  DeviceEvaluator ev{ctx, ds, P, loss, v, rb, GradExtra{sh, nullptr}};
  const int rc = bfgs_run(batch, ev);
  g_nonfinite_trials += batch.stats.nonfinite_trials;
  g_spec_launched += batch.stats.spec_launched;
  g_spec_used += batch.stats.spec_used;
  for (int i = 0; i < 5; ++i) g_hist[i] += batch.stats.hist[i];
  if (rc) return rc;
  if (g_stats_on) {  // the trees with the most objective calls (the pipeline's tail)
    std::vector<int32_t> by(trees);
    std::sort(by.begin(), by.end(), [&](int32_t a, int32_t b) { return fcalls[a] > fcalls[b]; });
    for (size_t i = 0; i < by.size() && i < 4; ++i)
      fprintf(stderr, "srhip optim: tree %d: %lld objective calls, %d constants\n", by[i], (long long)fcalls[by[i]],
              (int)(coff[by[i] + 1] - coff[by[i]]));
  }
  return SRHIP_OK;
}

extern "C" {

int srhip_eval_loss_grad(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                         const int64_t* idx, int64_t nidx, double* out_loss, double* out_grad, uint8_t* out_ok) {
  if (!out_loss || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  int rc = check_eval_args(ctx, ds, P, MODE_LOSS, loss);
  if (rc) return rc;
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "constant gradients need Float32 / Float64");
  HIP_TRY(hipSetDevice(ctx->device));
  View v;
  rc = make_view(ctx, ds, idx, nidx, true, v);
  if (rc) return rc;
  if (idx && ds->weighted) {
    rc = gathered_weight_sum(ctx, ds, nidx, v);
    if (rc) return rc;
  }
  rc = derived_view(ctx, ds, P, v);
  if (rc) return rc;
  const std::vector<int64_t> coff = const_offsets(*P);
  std::vector<int32_t> all(P->ntrees);
  for (int32_t t = 0; t < P->ntrees; ++t) all[t] = t;
  // (diagnostic, scripts/grad_bench.py: SRHIP_GRAD_VALUE_ONLY=1 runs the line search's value-only pass
  // over every tree -- losses only, the gradients are left zero)
  const char* vo = env_get("SRHIP_GRAD_VALUE_ONLY");
  std::vector<uint8_t> value_only;
  if (vo && atoi(vo) == 1) value_only.assign(P->ntrees, 1);
  rc = eval_grad(ctx, ds, P, loss, v, all, coff, out_loss, out_grad, out_ok, nullptr, 0, -1,
                 value_only.empty() ? nullptr : value_only.data());
  if (rc) return rc;
  return SRHIP_OK;
}

int srhip_eval_grad_predict(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, int32_t wrt, int32_t direction,
                            const int64_t* idx, int64_t nidx, void* out_pred, void* out_grad, uint8_t* out_ok) {
  if (!out_pred || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  if (wrt != SRHIP_WRT_CONSTANTS && wrt != SRHIP_WRT_FEATURES) return fail(SRHIP_ERR_INVALID, "wrt %d", wrt);
  int rc = check_eval_args(ctx, ds, P, MODE_PRED, nullptr);
  if (rc) return rc;
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "derivatives need Float32 / Float64");
  if (direction < 0 || (direction > 0 && (wrt != SRHIP_WRT_FEATURES || direction > ds->nfeat)))
    return fail(SRHIP_ERR_INVALID, "direction %d (wrt %d, %lld features)", direction, wrt, (long long)ds->nfeat);
  // values and did_succeed: the evaluator itself (eval_tree_array semantics, bit-identical predictions)
  rc = run_eval(ctx, ds, P, MODE_PRED, nullptr, idx, nidx, nullptr, out_pred, out_ok);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  View v;
  rc = make_view(ctx, ds, idx, nidx, false, v);
  if (rc) return rc;
  P->g_want_derived = false;  // per-row derivatives (features: the operators' own) -- no derived columns
  rc = compile_grad_program(*P);
  if (rc) return rc;
  const int32_t nt = P->ntrees;
  const int64_t m = v.m;
  const size_t es = dtype_size(P->dtype);
  // derivative rows of each tree: nconst (constants), nfeatures, or 1 (one direction)
  std::vector<int64_t> row0(nt + 1, 0);
  for (int32_t t = 0; t < nt; ++t)
    row0[t + 1] = row0[t] + (wrt == SRHIP_WRT_CONSTANTS ? P->info[t].nconst : (direction > 0 ? 1 : ds->nfeat));
  const int64_t nrows_out = row0[nt];
  if (nrows_out == 0) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // a patched gradient program may still be uploading
    return SRHIP_OK;
  }
  std::vector<int32_t> chunks;
  for (int32_t t = 0; t < nt; ++t) {
    if (P->ginfo[t].static_fail) continue;
    const int64_t nc = row0[t + 1] - row0[t];
    const int32_t first = direction > 0 ? direction - 1 : 0, end = direction > 0 ? direction : (int32_t)nc;
    for (int32_t c0 = first; c0 < end; c0 += GRAD_ROW_KT) {
      chunks.push_back(t);
      chunks.push_back(c0);
      chunks.push_back(end);
      chunks.push_back((int32_t)(row0[t] + c0 - first));
    }
  }
  auto body = [&]() -> int {
    const int nch = (int)chunks.size() / 4;
    DevBuf der;
    HIP_TRY(der.ensure((size_t)nrows_out * m * es));
    if (nch > 0) {
      const LaunchPlan L = grad_plan(ctx, m, nch);
      HIP_TRY(ctx->g_chunks.ensure(chunks.size() * sizeof(int32_t)));
      HIP_TRY(hipMemcpyAsync(ctx->g_chunks.p, chunks.data(), chunks.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                             ctx->stream));
      GradArgs a{};
      a.code = (const Ins*)P->d_gcode.p;
      a.prog_off = (const int32_t*)P->d_goff.p;
      a.chunks = (const int32_t*)ctx->g_chunks.p;
      a.X = v.X;
      a.ld = v.ld;
      a.nvalid = m;
      a.nchunks = nch;
      a.nfeat = (int32_t)ds->nfeat;
      a.rb_rows = L.rb_rows;
      a.nrb = L.nrb;
      a.chunks_per_group = L.tpg;
      a.max_steps = P->gmax_len;
      a.out_der = der.p;
      HIP_TRY(launch_grad_rows(P->dtype, P->gkmax <= 4 ? 4 : 8, wrt == SRHIP_WRT_CONSTANTS ? GMODE_ROWC : GMODE_ROWF, a,
                               dim3(L.nrb, L.groups), ctx->stream));
    }
    HIP_TRY(hipMemcpyAsync(out_grad, der.p, (size_t)nrows_out * m * es, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SRHIP_OK;
  };
  rc = body();
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  // complete = did_succeed of the evaluation and every derivative finite; a static failure's rows NaN
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t n = (row0[t + 1] - row0[t]) * m;
    if (P->ginfo[t].static_fail || P->info[t].static_fail) {
      for (int64_t i = 0; i < n; ++i) {
        if (es == 8) ((double*)out_grad)[row0[t] * m + i] = NAN;
        else ((float*)out_grad)[row0[t] * m + i] = NAN;
      }
      out_ok[t] = 0;
      continue;
    }
    bool fin = true;
    for (int64_t i = 0; i < n && fin; ++i)
      fin = es == 8 ? std::isfinite(((const double*)out_grad)[row0[t] * m + i])
                    : std::isfinite(((const float*)out_grad)[row0[t] * m + i]);
    if (!fin) out_ok[t] = 0;
  }
  return SRHIP_OK;
}

}  // extern "C"

namespace {

// the context's first n auxiliary contexts (created on first use), or fewer if creation fails
std::vector<srhip_ctx*> aux_ctxs(srhip_ctx* ctx, int n) {
  std::lock_guard<std::mutex> g(ctx->aux_mu);
  while ((int)ctx->aux.size() < n) {
    srhip_ctx* a = nullptr;
    if (srhip_ctx_create(ctx->device, &a) != SRHIP_OK) break;
    ctx->aux.push_back(a);
  }
  return std::vector<srhip_ctx*>(ctx->aux.begin(), ctx->aux.begin() + std::min<size_t>(n, ctx->aux.size()));
}

// bfgs_pipelined over G groups of the trees at once (G = SRHIP_OPTIM_SPLIT, default 3; 1 = off;
// populations of fewer than 64 trees are not split): tree i goes to group i % G; group 0 runs on the
// caller's thread and context, group g > 0 as a program of its own on the context's auxiliary
// context g - 1 (own stream and buffers) from a host thread of its own.  Each launch's host
// turnaround (decisions, constant patches, synchronisation) then overlaps the other groups' kernels.
// A tree's trajectory does not depend on the trees that share its launches (fixed row blocks, fixed
// reduction order), so the outcome is the one bfgs_pipelined gives over all trees at once.
int optimize_split(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const LossSel& loss, const View& v,
                   const std::vector<int32_t>& trees, const std::vector<int64_t>& coff, int iterations, double g_tol,
                   const std::vector<std::vector<double>>& starts, std::vector<double>& best_x,
                   std::vector<double>& best_f, std::vector<int64_t>& fcalls) {
  const char* se = getenv("SRHIP_OPTIM_SPLIT");
  int G = se && *se ? std::max(1, std::min(atoi(se), 8)) : 3;
  if (trees.size() < 64) G = 1;
  const std::vector<srhip_ctx*> aux = G > 1 ? aux_ctxs(ctx, G - 1) : std::vector<srhip_ctx*>();
  G = 1 + (int)aux.size();
  if (G == 1) return bfgs_pipelined(ctx, ds, P, loss, v, trees, coff, iterations, g_tol, starts, best_x, best_f, fcalls);
  std::vector<std::vector<int32_t>> grp(G);
  for (size_t i = 0; i < trees.size(); ++i) grp[i % G].push_back(trees[i]);
  struct Part {
    srhip_program* P = nullptr;
    std::vector<int64_t> coff;
    std::vector<std::vector<double>> starts;
    std::vector<double> bx, bf;
    std::vector<int64_t> fc;
    std::vector<int32_t> all;
    int rc = SRHIP_OK;
    std::string err;
    Part() = default;
    Part(const Part&) = delete;  // owns P
    Part& operator=(const Part&) = delete;
    ~Part() { srhip_program_destroy(P); }
  };
  std::vector<Part> part(G);
  for (int gi = 1; gi < G; ++gi) {
    Part& q = part[gi];
    const std::vector<int32_t>& tb = grp[gi];
    const int32_t n2 = (int32_t)tb.size();
    const int rc = subprogram(aux[gi - 1], P, tb, &q.P);
    if (rc) return rc;
    // the caller's derived view serves every group: the same column numbering
    q.P->gdspec = P->gdspec;
    q.P->gdbase = P->gdbase;
    q.P->gdspec_done = P->gdspec_done;
    q.P->g_want_derived = P->g_want_derived;
    q.coff = const_offsets(*q.P);
    q.starts.assign(starts.size(), std::vector<double>(q.coff.back()));
    q.bx.resize(q.coff.back());
    q.bf.resize(n2);
    q.fc.resize(n2);
    q.all.resize(n2);
    for (int32_t j = 0; j < n2; ++j) {
      const int32_t t = tb[j];
      for (int64_t k = 0; k < q.coff[j + 1] - q.coff[j]; ++k) {
        for (size_t s = 0; s < starts.size(); ++s) q.starts[s][q.coff[j] + k] = starts[s][coff[t] + k];
        q.bx[q.coff[j] + k] = best_x[coff[t] + k];
      }
      q.bf[j] = best_f[t];
      q.fc[j] = fcalls[t];
      q.all[j] = j;
    }
  }
  std::vector<std::thread> th;
  for (int gi = 1; gi < G; ++gi)
    th.emplace_back([&, gi] {
      Part& q = part[gi];
      srhip_ctx* c = aux[gi - 1];
      (void)hipSetDevice(c->device);
      q.rc = bfgs_pipelined(c, ds, q.P, loss, v, q.all, q.coff, iterations, g_tol, q.starts, q.bx, q.bf, q.fc);
      if (q.rc) q.err = last_error();
    });
  const int rc = bfgs_pipelined(ctx, ds, P, loss, v, grp[0], coff, iterations, g_tol, starts, best_x, best_f, fcalls);
  for (std::thread& t : th) t.join();
  if (rc) return rc;
  for (int gi = 1; gi < G; ++gi) {
    Part& q = part[gi];
    if (q.rc) return fail(q.rc, "%s", q.err.c_str());
    for (int32_t j = 0; j < (int32_t)grp[gi].size(); ++j) {
      const int32_t t = grp[gi][j];
      for (int64_t k = 0; k < q.coff[j + 1] - q.coff[j]; ++k) best_x[coff[t] + k] = q.bx[q.coff[j] + k];
      best_f[t] = q.bf[j];
      fcalls[t] = q.fc[j];
    }
  }
  return SRHIP_OK;
}

// ---- the steps the optimiser's entry points share (each entry point keeps its own baseline, generator
// order, run and re-score) -------------------------------------------------------------------------
int check_optim_args(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss* loss,
                     const srhip_optim_options* opt) {
  if (opt->iterations < 0 || opt->nrestarts < 0) return fail(SRHIP_ERR_INVALID, "negative iterations / restarts");
  const int rc = check_eval_args(ctx, ds, P, MODE_LOSS, loss);
  if (rc) return rc;
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "constant optimisation needs Float32 / Float64");
  return SRHIP_OK;
}
// One perturbed start of the constant x0k (src/ConstantOptimization.jl:53-60: c * (1 + randn/2)).
// Float32 trees perturb in T as the reference does (node.val * (T(1) + T(1//2) * randn(T))): a Float32
// normal draw and Float32 arithmetic, the start rounded like the constant it replaces.  A caller-supplied
// start (given) replaces the draw -- the generator is not advanced; a Float32 program rounds it to Float32.
double perturbed_start(double x0k, std::mt19937_64& rng, std::normal_distribution<double>& randn, bool f32,
                       const double* given) {
  double xs;
  if (given) {
    xs = *given;
  } else if (f32) {
    const float r = (float)randn(rng);
    xs = (double)((float)x0k * (1.0f + 0.5f * r));
  } else {
    xs = x0k * (1.0 + 0.5 * randn(rng));
  }
  return f32 ? (double)(float)xs : xs;
}
// starts[1 ..] (the restarts; starts[0] is x0) to the caller's [nrestarts][sum nconst], if wanted
void copy_starts_out(const std::vector<std::vector<double>>& starts, double* starts_out) {
  if (!starts_out) return;
  for (size_t s = 1; s < starts.size(); ++s)
    std::copy(starts[s].begin(), starts[s].end(), starts_out + (s - 1) * starts[s].size());
}
// the thread's timing counters and statistics (SRHIP_OPTIM_TIMING), before an optimiser run
void reset_optim_counters(bool stats_on, bool launch_log) {
  g_t_compile = g_t_eval = g_t_host = 0.0;
  g_patch_scan_s = g_patch_copy_s = 0.0;
  g_n_launch = 0;
  g_stats_on = stats_on;
  g_launch_log = launch_log;
  for (int64_t& h : g_hist) h = 0;
  g_nonfinite_trials = 0;
  g_spec_launched = g_spec_used = 0;
  for (auto& a : g_items)
    for (auto& b : a) b[0] = b[1] = 0;
}
// after a failed run: the program back at the constants it came with
void restore_constants(srhip_program& P, const std::vector<double>& x0) {
  set_all_consts(P, x0.data());
  compile_program(P);
  upload_program(P);
}
// accept where the best minimum beats the baseline (src/ConstantOptimization.jl:70-78): out_improved[t],
// and the constants to return -- best_x of the accepted trees, x0 of the others
std::vector<double> accept_against_baseline(const std::vector<double>& x0, const std::vector<int64_t>& coff,
                                            const std::vector<double>& best_x, const std::vector<double>& best_f,
                                            const std::vector<double>& base, uint8_t* out_improved) {
  std::vector<double> final_x = x0;
  for (size_t t = 0; t < base.size(); ++t) {
    const bool better = best_f[t] < base[t];
    out_improved[t] = better ? 1 : 0;
    if (better)
      for (int64_t k = coff[t]; k < coff[t + 1]; ++k) final_x[k] = best_x[k];
  }
  return final_x;
}
int install_constants(srhip_program& P, const std::vector<double>& final_x) {
  set_all_consts(P, final_x.data());
  const int rc = compile_program(P);
  return rc ? rc : upload_program(P);
}
// num_evals bookkeeping (src/ConstantOptimization.jl:51,65,79): the objective calls of every start
// (result.f_calls), plus one for the re-score of an accepted tree; 0 for a tree left alone
void report_fcalls(const std::vector<int64_t>& fcalls, const uint8_t* out_improved, int64_t* out_fcalls) {
  if (!out_fcalls) return;
  for (size_t t = 0; t < fcalls.size(); ++t) out_fcalls[t] = fcalls[t] + out_improved[t];
}
// a failed step (status rc) whose call must leave the constants as they came: restored, the step's message kept
int restore_and_reraise(srhip_program& P, const std::vector<double>& x0, int rc) {
  const std::string msg = last_error();
  restore_constants(P, x0);
  return fail(rc, "%s", msg.c_str());
}
// The entry points' common end: install the accepted constants, re-score the returned trees with the call's
// evaluator (the reference re-scores accepted members), report the calls.  A failed re-score under a loss
// expression (expr) leaves the constants as they came.
template <class Score>
int install_and_rescore(srhip_program& P, bool expr, const std::vector<double>& x0, const std::vector<double>& final_x,
                        Score score, double* out_loss, const std::vector<int64_t>& fcalls, const uint8_t* out_improved,
                        int64_t* out_fcalls) {
  int rc = install_constants(P, final_x);
  if (rc) return rc;
  std::vector<uint8_t> ok(P.ntrees);
  rc = score(out_loss, ok.data());
  if (rc) return expr ? restore_and_reraise(P, x0, rc) : rc;
  report_fcalls(fcalls, out_improved, out_fcalls);
  return SRHIP_OK;
}

}  // namespace

// srhip_optimize_constants_starts / _expr after their argument checks: `score` is the evaluator of the loss
// (run_eval for a built-in kind, srhip_eval_loss_expr for an expression) for the baseline and the final
// re-score, `loss` the optimiser's objective.
template <class Score>
int optimize_starts(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const LossSel& loss, Score score,
                    const int64_t* idx, int64_t nidx, const srhip_optim_options* opt, const double* starts_in,
                    double* starts_out, double* out_loss, uint8_t* out_improved, int64_t* out_fcalls,
                    const GradShardCall* sh = nullptr) {
  int rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int32_t nt = P->ntrees;
  // baseline = f(tree) with the evaluator itself (src/ConstantOptimization.jl:49)
  std::vector<double> base(nt);
  std::vector<uint8_t> base_ok(nt);
  rc = score(base.data(), base_ok.data());
  if (rc) return rc;
  View v;
  rc = make_view(ctx, ds, idx, nidx, true, v);
  if (rc) return rc;
  if (idx && ds->weighted) {
    rc = gathered_weight_sum(ctx, ds, nidx, v);
    if (rc) return rc;
  }
  rc = derived_view(ctx, ds, P, v);
  if (rc) return rc;
  const std::vector<int64_t> coff = const_offsets(*P);
  const std::vector<double> x0 = get_all_consts(*P);
  const int64_t nall = (int64_t)x0.size();
  std::vector<int32_t> trees;  // trees with constants (nconst == 0: nothing to optimise, :35)
  for (int32_t t = 0; t < nt; ++t)
    if (P->info[t].nconst > 0 && !P->info[t].static_fail) trees.push_back(t);
  std::vector<double> best_x = x0, best_f(nt, INFINITY);
  std::vector<int64_t> fcalls(nt, 0);
  const double g_tol = opt->g_tol > 0 ? opt->g_tol : 1e-8;
  // the starting points: x0, then nrestarts perturbed copies drawn from one generator start-major, then
  // tree, then constant; caller-supplied starts (starts_in, [nrestarts][sum nconst]) replace the draws.
  // Trees without constants or failing statically keep x0.
  std::vector<std::vector<double>> starts(opt->nrestarts + 1, x0);
  std::mt19937_64 rng(opt->seed);
  std::normal_distribution<double> randn(0.0, 1.0);
  const bool f32 = P->dtype == SRHIP_F32;
  for (int start = 1; start <= opt->nrestarts; ++start)
    for (int32_t t : trees)
      for (int64_t k = coff[t]; k < coff[t + 1]; ++k)
        starts[start][k] = perturbed_start(x0[k], rng, randn, f32, starts_in ? starts_in + (int64_t)(start - 1) * nall + k : nullptr);
  copy_starts_out(starts, starts_out);
  if (!trees.empty()) {
    const double tb = now_s();
    const char* te = getenv("SRHIP_OPTIM_TIMING");
    reset_optim_counters(te && (*te == '2' || *te == '3'), te && *te == '3');
    // a row shard runs one group on the caller's context and thread: a communicator carries one exchange at a time
    rc = sh ? bfgs_pipelined(ctx, ds, P, loss, v, trees, coff, opt->iterations, g_tol, starts, best_x, best_f, fcalls,
                             nullptr, sh)
            : optimize_split(ctx, ds, P, loss, v, trees, coff, opt->iterations, g_tol, starts, best_x, best_f, fcalls);
    if (g_stats_on)
      fprintf(stderr, "srhip optim (the caller's group: 1 of SRHIP_OPTIM_SPLIT groups): launches by active trees: "
              "1: %lld, 2-4: %lld, 5-16: %lld, 17-64: %lld, >64: %lld; "
              "non-finite trial points %lld; speculative points %lld evaluated, %lld used\n", (long long)g_hist[0],
              (long long)g_hist[1], (long long)g_hist[2], (long long)g_hist[3], (long long)g_hist[4],
              (long long)g_nonfinite_trials, (long long)g_spec_launched, (long long)g_spec_used);
    if (g_stats_on)
      fprintf(stderr, "srhip optim: items (all / non-finite f): gradient small %lld/%lld big %lld/%lld; value-only "
              "small %lld/%lld big %lld/%lld\n", (long long)g_items[0][0][0], (long long)g_items[0][0][1],
              (long long)g_items[0][1][0], (long long)g_items[0][1][1], (long long)g_items[1][0][0],
              (long long)g_items[1][0][1], (long long)g_items[1][1][0], (long long)g_items[1][1][1]);
    if (te && (*te == '1' || *te == '2' || *te == '3'))
      fprintf(stderr,
              "srhip optim: %.1f ms total (all groups), caller's group: %lld launches, eval_grad %.1f ms (compile/patch "
              "%.1f ms: scan+recompile %.1f, "
              "snapshot+upload %.1f), set_consts %.1f ms\n",
              1e3 * (now_s() - tb), (long long)g_n_launch, 1e3 * g_t_eval, 1e3 * g_t_compile, 1e3 * g_patch_scan_s,
              1e3 * g_patch_copy_s, 1e3 * g_t_host);
    if (rc) {
      restore_constants(*P, x0);
      return rc;
    }
  }
  const std::vector<double> final_x = accept_against_baseline(x0, coff, best_x, best_f, base, out_improved);
  return install_and_rescore(*P, loss.expr != nullptr, x0, final_x, score, out_loss, fcalls, out_improved, out_fcalls);
}

extern "C" {

int srhip_optimize_constants_starts(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P,
                                    const srhip_loss* loss, const int64_t* idx, int64_t nidx,
                                    const srhip_optim_options* opt, const double* starts_in, double* starts_out,
                                    double* out_loss, uint8_t* out_improved, int64_t* out_fcalls) {
  if (!opt || !out_loss || !out_improved) return fail(SRHIP_ERR_INVALID, "null argument");
  const int rc = check_optim_args(ctx, ds, P, loss, opt);
  if (rc) return rc;
  auto score = [&](double* l, uint8_t* ok) { return run_eval(ctx, ds, P, MODE_LOSS, loss, idx, nidx, l, nullptr, ok); };
  return optimize_starts(ctx, ds, P, LossSel(loss), score, idx, nidx, opt, starts_in, starts_out, out_loss, out_improved,
                         out_fcalls);
}

// srhip_optimize_constants_starts under a loss expression: baseline and re-score by srhip_eval_loss_expr,
// the objective by grad_lossx_kernel
int srhip_optimize_constants_expr(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss_expr* e,
                                  const int64_t* idx, int64_t nidx, const srhip_optim_options* opt,
                                  const double* starts_in, double* starts_out, double* out_loss,
                                  uint8_t* out_improved, int64_t* out_fcalls) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!opt || !out_loss || !out_improved) return fail(SRHIP_ERR_INVALID, "null argument");
  if (opt->iterations < 0 || opt->nrestarts < 0) return fail(SRHIP_ERR_INVALID, "negative iterations / restarts");
  const int rc = check_loss_expr_args(ctx, ds, P, e);
  if (rc) return rc;
  auto score = [&](double* l, uint8_t* ok) { return srhip_eval_loss_expr(ctx, ds, P, e, idx, nidx, l, ok); };
  return optimize_starts(ctx, ds, P, LossSel(&e->prog), score, idx, nidx, opt, starts_in, starts_out, out_loss,
                         out_improved, out_fcalls);
}

// srhip_eval_loss_grad under a loss expression: the same view, decisions and reduction, the loss stage of
// every launch running the expression's program (srhip_grad_lossx.hip)
int srhip_eval_loss_grad_expr(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss_expr* e,
                              const int64_t* idx, int64_t nidx, double* out_loss, double* out_grad, uint8_t* out_ok) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!out_loss || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  int rc = check_loss_expr_args(ctx, ds, P, e);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  View v;
  rc = make_view(ctx, ds, idx, nidx, true, v);
  if (rc) return rc;
  if (idx && ds->weighted) {
    rc = gathered_weight_sum(ctx, ds, nidx, v);
    if (rc) return rc;
  }
  rc = derived_view(ctx, ds, P, v);
  if (rc) return rc;
  const std::vector<int64_t> coff = const_offsets(*P);
  std::vector<int32_t> all(P->ntrees);
  for (int32_t t = 0; t < P->ntrees; ++t) all[t] = t;
  rc = eval_grad(ctx, ds, P, LossSel(&e->prog), v, all, coff, out_loss, out_grad, out_ok);
  if (rc) return rc;
  for (int32_t t = 0; t < P->ntrees; ++t)  // a failed tree: +Inf and a zero slice, whatever its rows summed to
    if (!out_ok[t]) {
      out_loss[t] = INFINITY;
      std::fill(out_grad + coff[t], out_grad + coff[t + 1], 0.0);
    }
  return SRHIP_OK;
}

int srhip_optimize_constants(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                             const int64_t* idx, int64_t nidx, const srhip_optim_options* opt, double* out_loss,
                             uint8_t* out_improved, int64_t* out_fcalls) {
  return srhip_optimize_constants_starts(ctx, ds, P, loss, idx, nidx, opt, nullptr, nullptr, out_loss, out_improved,
                                         out_fcalls);
}

}  // extern "C"

// ---- row shards: srhip_eval_loss_grad_sharded / srhip_optimize_constants_sharded / the manual steps ---------
namespace {

// this rank's view of its own rows, as the one-device entry points make it
int shard_view(srhip_ctx* ctx, const srhip_dataset* ds, const int64_t* idx, int64_t nidx, View& v) {
  HIP_TRY(hipSetDevice(ctx->device));
  const int rc = make_view(ctx, ds, idx, nidx, true, v);
  if (rc) return rc;
  return idx && ds->weighted ? gathered_weight_sum(ctx, ds, nidx, v) : SRHIP_OK;
}

// The call-start exchange, one group: [weight sum or rows | per feature {column sum, non-finite count} | rows] by
// SUM and the call's signature [k_i, -k_i] by MAX.  Every rank returns SRHIP_ERR_INVALID naming the first field the
// ranks disagree on, before any per-round exchange: ranks that would build different launches fail at once
// instead of waiting out the communicator's timeout inside a collective.
int shard_call_start(const srhip_dataset* ds, const View& v, const GradShardIO& io, const double (&sig)[SIG_COUNT],
                     GradShardCall& sh) {
  const size_t nf = (size_t)ds->nfeat;
  std::vector<double> sum(2 + 2 * nf), mx(2 * (size_t)SIG_COUNT);
  sum[0] = ds->weighted ? v.sum_w : (double)v.m;
  for (size_t f = 0; f < nf; ++f) {
    sum[1 + 2 * f] = v.stats ? v.stats[f].sum : 0.0;
    sum[2 + 2 * f] = v.stats ? (double)v.stats[f].nonfinite : 0.0;
  }
  sum[1 + 2 * nf] = (double)v.m;
  for (int i = 0; i < SIG_COUNT; ++i) {
    mx[2 * i] = sig[i];
    mx[2 * i + 1] = -sig[i];
  }
  const int rc = io.start(sum.data(), sum.size(), mx.data(), mx.size());
  if (rc) return rc;
  const int bad = shard_sig_check(mx.data(), SIG_COUNT);
  if (bad >= 0)
    return fail(SRHIP_ERR_INVALID, "the ranks of a row-sharded call disagree on its %s (every rank calls with the same "
                                   "program, options, seed and SRHIP_* environment)", shard_sig_name(bad));
  sh.io = &io;
  sh.wsum = sum[0];
  sh.tail.assign(sum.begin() + 1, sum.end());
  return SRHIP_OK;
}

uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
  return h;
}
uint64_t f64_bits(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return b;
}

// the fields every sharded entry point shares
void shard_signature(const srhip_dataset* ds, const srhip_program* P, const srhip_loss* loss, int entry,
                     double (&sig)[SIG_COUNT]) {
  for (double& s : sig) s = 0.0;
  sig[SIG_ENTRY] = entry;
  sig[SIG_TREES] = P->ntrees;
  sig[SIG_CONSTS] = (double)const_offsets(*P).back();
  sig[SIG_DTYPE] = P->dtype;
  sig[SIG_WEIGHTED] = ds->weighted ? 1 : 0;
  sig[SIG_LOSS_KIND] = loss->kind;
  shard_sig_put64(sig, SIG_LOSS_P0_HI, f64_bits(loss->p0));
  shard_sig_put64(sig, SIG_LOSS_P1_HI, f64_bits(loss->p1));
  const char* kte = env_get("SRHIP_GRAD_KT");
  sig[SIG_GRAD_KT] = kte && (atoi(kte) == 4 || atoi(kte) == GRAD_KT) ? atoi(kte) : 0;
}

}  // namespace

int srhip::run_grad_sharded(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                            const int64_t* idx, int64_t nidx, const GradShardIO& gio, double* out_loss, double* out_grad,
                            uint8_t* out_ok) {
  if (!out_loss || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  int rc = check_eval_args(ctx, ds, P, MODE_LOSS, loss);
  if (rc) return rc;
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "constant gradients need Float32 / Float64");
  View v;
  rc = shard_view(ctx, ds, idx, nidx, v);
  if (rc) return rc;
  double sig[SIG_COUNT];
  shard_signature(ds, P, loss, 0, sig);
  GradShardCall sh;
  rc = shard_call_start(ds, v, gio, sig, sh);
  if (rc) return rc;
  rc = derived_view(ctx, ds, P, v);
  if (rc) return rc;
  const std::vector<int64_t> coff = const_offsets(*P);
  std::vector<int32_t> all(P->ntrees);
  std::iota(all.begin(), all.end(), 0);
  return eval_grad(ctx, ds, P, loss, v, all, coff, out_loss, out_grad, out_ok, nullptr, 0, -1, nullptr, true, nullptr,
                   GradExtra{&sh, nullptr});
}

int srhip::run_optimize_sharded(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                                const int64_t* idx, int64_t nidx, const srhip_optim_options* opt, const double* starts_in,
                                double* starts_out, const ShardIO& eio, const GradShardIO& gio, double* out_loss,
                                uint8_t* out_improved, int64_t* out_fcalls) {
  if (!opt || !out_loss || !out_improved) return fail(SRHIP_ERR_INVALID, "null argument");
  int rc = check_optim_args(ctx, ds, P, loss, opt);
  if (rc) return rc;
  GradShardCall sh;
  {
    // the call-start exchange on a view of its own, in front of the baseline: the signature is checked before
    // anything whose size depends on it is exchanged (optimize_starts makes the view again after its baseline,
    // whose evaluation gathers into the same buffers)
    View v;
    rc = shard_view(ctx, ds, idx, nidx, v);
    if (rc) return rc;
    double sig[SIG_COUNT];
    shard_signature(ds, P, loss, 1, sig);
    const BfgsKnobs k = bfgs_knobs(opt->iterations, opt->g_tol > 0 ? opt->g_tol : 1e-8);
    sig[SIG_ITERATIONS] = opt->iterations;
    sig[SIG_RESTARTS] = opt->nrestarts;
    shard_sig_put64(sig, SIG_SEED_HI, opt->seed);
    shard_sig_put64(sig, SIG_GTOL_HI, f64_bits(k.g_tol));
    const size_t nstart = (size_t)opt->nrestarts * (size_t)const_offsets(*P).back();
    shard_sig_put64(sig, SIG_STARTS_HI, starts_in && nstart ? fnv1a(starts_in, nstart * sizeof(double)) : 0);
    sig[SIG_VALUE_TRIALS] = k.value_trials ? 1 : 0;
    sig[SIG_SPEC_SLOTS] = k.spec_slots;
    sig[SIG_SPEC_ACTIVE] = k.spec_max_active;
    sig[SIG_SPEC_DEPTH] = k.spec_max_depth;
    rc = shard_call_start(ds, v, gio, sig, sh);
    if (rc) return rc;
  }
  auto score = [&](double* l, uint8_t* ok) { return run_eval_sharded(ctx, ds, P, loss, idx, nidx, eio, l, ok); };
  return optimize_starts(ctx, ds, P, LossSel(loss), score, idx, nidx, opt, starts_in, starts_out, out_loss, out_improved,
                         out_fcalls, &sh);
}

extern "C" {

int srhip_eval_loss_grad_partials(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                                  const int64_t* idx, int64_t nidx, double* sums, double* gsums, double* chk) {
  if (!sums || !chk) return fail(SRHIP_ERR_INVALID, "null output");
  int rc = check_eval_args(ctx, ds, P, MODE_LOSS, loss);
  if (rc) return rc;
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "constant gradients need Float32 / Float64");
  const std::vector<int64_t> coff = const_offsets(*P);
  if (!gsums && coff.back() > 0) return fail(SRHIP_ERR_INVALID, "null gradient sums");
  View v;
  rc = shard_view(ctx, ds, idx, nidx, v);
  if (rc) return rc;
  rc = derived_view(ctx, ds, P, v);
  if (rc) return rc;
  const int32_t nt = P->ntrees;
  std::vector<int32_t> all(nt);
  std::iota(all.begin(), all.end(), 0);
  std::vector<double> f(nt), g(std::max<int64_t>(1, coff.back()));
  for (int32_t t = 0; t < nt; ++t) chk[t] = 0.0;
  // the raw records: sums undivided (the backend divides by 1), no decision, each tree's statistic into chk
  rc = eval_grad(ctx, ds, P, loss, v, all, coff, f.data(), g.data(), nullptr, nullptr, 0, -1, nullptr, true, nullptr,
                 GradExtra{nullptr, chk});
  if (rc) return rc;
  const double wsum = ds->weighted ? v.sum_w : (double)v.m;
  for (int32_t t = 0; t < nt; ++t) {
    sums[2 * (size_t)t] = P->ginfo[t].static_fail ? 0.0 : f[t];  // (a static failure launches nothing: no sum)
    sums[2 * (size_t)t + 1] = wsum;
    // a non-finite Float32 statistic travels as +Inf: a MAX across shards need not keep a NaN
    if (P->dtype == SRHIP_F32 && !std::isfinite(chk[t])) chk[t] = INFINITY;
  }
  fill_decide_inputs(sums, nt, ds->nfeat, v.stats, v.m);
  std::copy(g.begin(), g.begin() + coff.back(), gsums);
  return SRHIP_OK;
}

}  // extern "C"

// ---- one row subset per tree: srhip_eval_loss_grad_rowsets / srhip_optimize_constants_rowsets ---------
namespace {

// The call's batch: the baseline through the rowsets evaluation (one launch; base_loss / base_ok), whose
// per-set records (feature statistics, weight sums) are kept on the host, and every set a wave can stage
// gathered once into the context's packed buffer.  Sets over the cap, statically failing trees (the
// evaluation took no statistics of their sets) and a non-default SRHIP_GRAD_RB stay unstaged: the
// single-idx path.
// The loss of a row-set call: a built-in kind or an expression (exactly one is set)
struct RowsetLoss {
  const srhip_loss* kind = nullptr;
  const srhip_loss_expr* expr = nullptr;
  LossSel sel() const { return expr ? LossSel(&expr->prog) : LossSel(kind); }
  // the call's evaluator: one rowsets launch
  int score(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const int64_t* row_offsets,
            const int64_t* rows, double* out_loss, uint8_t* out_ok) const {
    return expr ? srhip_eval_loss_expr_rowsets(ctx, ds, P, expr, row_offsets, rows, out_loss, out_ok)
                : srhip_eval_loss_rowsets(ctx, ds, P, kind, row_offsets, rows, out_loss, out_ok);
  }
};

int make_rowset_batch(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const RowsetLoss& loss,
                      const int64_t* row_offsets, const int64_t* rows, RowsetBatch& rb, double* base_loss,
                      uint8_t* base_ok) {
  const int32_t nt = P->ntrees;
  const int64_t nf = ds->nfeat;
  const bool weighted = ds->weighted;
  int rc = loss.score(ctx, ds, P, row_offsets, rows, base_loss, base_ok);
  if (rc) return rc;
  rb.row_off = row_offsets;
  rb.rows = rows;
  rb.staged.assign(nt, 0);
  rb.m.assign(nt, 0);
  rb.fstat.assign((size_t)nt * std::max<int64_t>(1, nf), FeatStat{});
  rb.wsum.assign(nt, 0.0);
  const int cap = grad_rowset_cap(P->dtype, nf, weighted);
  const bool pdec = P->dec.size() == (size_t)nt;
  const bool rb256 = grad_plan(ctx, 1, 1).rb_rows == GRAD_ROWSET_RB;
  const size_t fs_stride = (size_t)std::max<int64_t>(1, nf);
  const size_t fs_bytes = (size_t)nt * fs_stride * sizeof(FeatStat);
  const int64_t ncol = nf + 1 + (weighted ? 1 : 0);
  const int64_t total = row_offsets[nt];
  // [row_off | rows | set_off] int64, then set_m int32
  std::vector<int64_t> meta((size_t)nt + 1 + (size_t)total + (size_t)nt + ((size_t)nt + 1) / 2);
  int64_t* const h_set_off = meta.data() + nt + 1 + total;
  int32_t* const h_set_m = (int32_t*)(h_set_off + nt);
  memcpy(meta.data(), row_offsets, ((size_t)nt + 1) * sizeof(int64_t));
  memcpy(meta.data() + nt + 1, rows, (size_t)total * sizeof(int64_t));
  int64_t elems = 0;
  int32_t nstaged = 0;
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t m = row_offsets[t + 1] - row_offsets[t];
    const bool sfail = pdec ? P->dec[t].static_fail : P->info[t].static_fail;
    const bool st = rb256 && m <= cap && !sfail && !P->info[t].static_fail;
    rb.m[t] = (int32_t)std::min<int64_t>(m, INT32_MAX);
    h_set_m[t] = st ? (int32_t)m : 0;
    h_set_off[t] = st ? elems : -1;
    if (!st) continue;
    rb.staged[t] = 1;
    nstaged += 1;
    elems += ncol * ((m + GRAD_ROWSET_RB - 1) / GRAD_ROWSET_RB * GRAD_ROWSET_RB);
    // the rowsets evaluation's records of this set (it launched the tree: m <= its cap, no static failure)
    const FeatStat* fs = (const FeatStat*)ctx->h_rowsets.p + (size_t)t * fs_stride;
    for (int64_t f = 0; f < nf; ++f) rb.fstat[(size_t)t * nf + f] = fs[f];
    if (weighted) rb.wsum[t] = ((const double*)((const uint8_t*)ctx->h_rowsets.p + fs_bytes))[t];
  }
  if (nstaged == 0) return SRHIP_OK;
  const size_t es = dtype_size(P->dtype);
  HIP_TRY(ctx->g_rs_meta.ensure(meta.size() * sizeof(int64_t)));
  HIP_TRY(ctx->g_rs_packed.ensure((size_t)elems * es));
  HIP_TRY(hipMemcpyAsync(ctx->g_rs_meta.p, meta.data(), meta.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  const int64_t* d_meta = (const int64_t*)ctx->g_rs_meta.p;
  rb.packed = ctx->g_rs_packed.p;
  rb.d_set_off = d_meta + nt + 1 + total;
  rb.d_set_m = (const int32_t*)(rb.d_set_off + nt);
  HIP_TRY(launch_grad_rowsets_pack(P->dtype, ds->X.p, ds->y.p, weighted ? ds->w.p : nullptr, ds->ld, (int)nf, d_meta,
                                   d_meta + nt + 1, rb.d_set_off, nt, ctx->g_rs_packed.p, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // (meta is a local: its copy must be complete)
  return SRHIP_OK;
}

// srhip_eval_loss_grad_rowsets / srhip_eval_loss_grad_expr_rowsets after their argument checks
int grad_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const RowsetLoss& loss,
                 const int64_t* row_offsets, const int64_t* rows, double* out_loss, double* out_grad, uint8_t* out_ok) {
  const int32_t nt = P->ntrees;
  int rc = check_rowsets(ds, nt, row_offsets, rows);
  if (rc) return rc;
  ctx->rowsets_fallback = 0;
  if (nt == 0) return SRHIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  RowsetBatch rb;
  std::vector<double> base(nt);
  std::vector<uint8_t> base_ok(nt);
  rc = make_rowset_batch(ctx, ds, P, loss, row_offsets, rows, rb, base.data(), base_ok.data());
  if (rc) return rc;
  const std::vector<int64_t> coff = const_offsets(*P);
  // the unstaged sets first, each through the single-idx call on a one-tree program
  std::vector<int32_t> staged;
  int64_t nalone = 0;
  for (int32_t t = 0; t < nt; ++t) {
    if (rb.staged[t]) {
      staged.push_back(t);
      continue;
    }
    if (loss.expr && P->info[t].static_fail) {
      // srhip_eval_loss_grad_expr's answer for a tree that fails whatever the rows: +Inf, a zero slice, not ok
      out_loss[t] = INFINITY;
      std::fill(out_grad + coff[t], out_grad + coff[t + 1], 0.0);
      out_ok[t] = 0;
      continue;
    }
    srhip_program* Q = nullptr;
    rc = subprogram(ctx, P, {t}, &Q);
    if (rc) return rc;
    const int64_t* const set = rows + row_offsets[t];
    const int64_t m = row_offsets[t + 1] - row_offsets[t];
    rc = loss.expr ? srhip_eval_loss_grad_expr(ctx, ds, Q, loss.expr, set, m, out_loss + t, out_grad + coff[t], out_ok + t)
                   : srhip_eval_loss_grad(ctx, ds, Q, loss.kind, set, m, out_loss + t, out_grad + coff[t], out_ok + t);
    srhip_program_destroy(Q);
    if (rc) return rc;
    nalone += 1;
  }
  ctx->rowsets_fallback = nalone;
  if (staged.empty()) return SRHIP_OK;
  P->g_want_derived = false;  // (off below 8192 rows in the single-idx path too)
  const View none{};
  rc = eval_grad(ctx, ds, P, loss.sel(), none, staged, coff, out_loss, out_grad, out_ok, nullptr, 0, -1, nullptr, true, &rb);
  if (rc) return rc;
  if (loss.expr)
    for (int32_t t : staged)  // srhip_eval_loss_grad_expr: a failed tree is +Inf and a zero slice, whatever its rows summed to
      if (!out_ok[t]) {
        out_loss[t] = INFINITY;
        std::fill(out_grad + coff[t], out_grad + coff[t + 1], 0.0);
      }
  return SRHIP_OK;
}

// srhip_optimize_constants_rowsets / srhip_optimize_constants_expr_rowsets after their argument checks
int optimize_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const RowsetLoss& loss,
                     const int64_t* row_offsets, const int64_t* rows, const srhip_optim_options* opt,
                     const uint64_t* tree_seeds, const double* starts_in, double* starts_out, double* out_loss,
                     uint8_t* out_improved, int64_t* out_fcalls) {
  const int32_t nt = P->ntrees;
  int rc = check_rowsets(ds, nt, row_offsets, rows);
  if (rc) return rc;
  ctx->rowsets_fallback = 0;
  if (nt == 0) return SRHIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  // baseline = f(tree) with the evaluator itself (src/ConstantOptimization.jl:49), every tree on its own set
  RowsetBatch rb;
  std::vector<double> base(nt);
  std::vector<uint8_t> base_ok(nt);
  rc = make_rowset_batch(ctx, ds, P, loss, row_offsets, rows, rb, base.data(), base_ok.data());
  if (rc) return rc;
  P->g_want_derived = false;
  const std::vector<int64_t> coff = const_offsets(*P);
  const std::vector<double> x0 = get_all_consts(*P);
  const int64_t nall = (int64_t)x0.size();
  std::vector<int32_t> trees, alone;  // trees with constants, by path (nconst == 0: nothing to optimise, :35)
  for (int32_t t = 0; t < nt; ++t)
    if (P->info[t].nconst > 0 && !P->info[t].static_fail) (rb.staged[t] ? trees : alone).push_back(t);
  std::vector<double> best_x = x0, best_f(nt, INFINITY);
  std::vector<int64_t> fcalls(nt, 0);
  const double g_tol = opt->g_tol > 0 ? opt->g_tol : 1e-8;
  // the starting points: x0, then nrestarts perturbed copies; tree t draws from a generator of its own
  // (tree_seeds[t], or opt->seed + t) start-major, then constant by constant -- the sequence the one-tree
  // call draws (srhip_optimize_constants_starts).  Trees without constants or failing statically keep x0.
  std::vector<std::vector<double>> starts(opt->nrestarts + 1, x0);
  const bool f32 = P->dtype == SRHIP_F32;
  auto tree_seed = [&](int32_t t) { return tree_seeds ? tree_seeds[t] : opt->seed + (uint64_t)t; };
  for (int32_t t = 0; t < nt; ++t) {
    if (!(P->info[t].nconst > 0 && !P->info[t].static_fail)) continue;
    std::mt19937_64 rng(tree_seed(t));
    std::normal_distribution<double> randn(0.0, 1.0);
    for (int start = 1; start <= opt->nrestarts; ++start)
      for (int64_t k = coff[t]; k < coff[t + 1]; ++k)
        starts[start][k] = perturbed_start(x0[k], rng, randn, f32, starts_in ? starts_in + (int64_t)(start - 1) * nall + k : nullptr);
  }
  copy_starts_out(starts, starts_out);
  if (!trees.empty()) {
    const View none{};
    const double tb = now_s();
    reset_optim_counters(false, false);
    rc = bfgs_pipelined(ctx, ds, P, loss.sel(), none, trees, coff, opt->iterations, g_tol, starts, best_x, best_f, fcalls, &rb);
    const char* te = getenv("SRHIP_OPTIM_TIMING");  // the single-idx entry point's line, for this path
    if (te && *te && *te != '0')
      fprintf(stderr,
              "srhip optim rowsets: %.1f ms optimiser, %lld launches, eval_grad %.1f ms (compile/patch %.1f ms: "
              "scan+recompile %.1f, snapshot+upload %.1f), set_consts %.1f ms\n",
              1e3 * (now_s() - tb), (long long)g_n_launch, 1e3 * g_t_eval, 1e3 * g_t_compile, 1e3 * g_patch_scan_s,
              1e3 * g_patch_copy_s, 1e3 * g_t_host);
    if (rc) {
      restore_constants(*P, x0);
      return rc;
    }
  }
  std::vector<double> final_x = accept_against_baseline(x0, coff, best_x, best_f, base, out_improved);
  // the sets no wave can stage: the single-idx entry point on a one-tree program (its own view, baseline,
  // optimiser run and acceptance), seeded with the tree's seed and given the tree's starts.  (The tree is
  // still at x0: the optimiser above moved only the staged trees' constants.)
  for (int32_t t : alone) {
    const int64_t nc = coff[t + 1] - coff[t];
    std::vector<double> sin((size_t)opt->nrestarts * nc);
    for (int start = 1; start <= opt->nrestarts; ++start)
      for (int64_t k = 0; k < nc; ++k) sin[(size_t)(start - 1) * nc + k] = starts[start][coff[t] + k];
    srhip_program* Q = nullptr;
    rc = subprogram(ctx, P, {t}, &Q);
    if (rc == SRHIP_OK) {
      srhip_optim_options o1 = *opt;
      o1.seed = tree_seed(t);
      double l1 = 0.0;
      uint8_t imp = 0;
      int64_t fc = 0;
      const int64_t* const set = rows + row_offsets[t];
      const int64_t m = row_offsets[t + 1] - row_offsets[t];
      const double* const sp = opt->nrestarts > 0 ? sin.data() : nullptr;
      rc = loss.expr ? srhip_optimize_constants_expr(ctx, ds, Q, loss.expr, set, m, &o1, sp, nullptr, &l1, &imp, &fc)
                     : srhip_optimize_constants_starts(ctx, ds, Q, loss.kind, set, m, &o1, sp, nullptr, &l1, &imp, &fc);
      if (rc == SRHIP_OK) {
        double* cst = final_x.data() + coff[t];
        get_consts(Q->nodes.data(), 0, cst);
        out_improved[t] = imp;
        fcalls[t] = fc - imp;
      }
      srhip_program_destroy(Q);
    }
    if (rc) return restore_and_reraise(*P, x0, rc);
  }
  // the re-score: one rowsets launch
  auto score = [&](double* l, uint8_t* ok) { return loss.score(ctx, ds, P, row_offsets, rows, l, ok); };
  rc = install_and_rescore(*P, loss.expr != nullptr, x0, final_x, score, out_loss, fcalls, out_improved, out_fcalls);
  if (rc) return rc;
  ctx->rowsets_fallback = (int64_t)alone.size();
  return SRHIP_OK;
}

}  // namespace

extern "C" {

int srhip_eval_loss_grad_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                                 const int64_t* row_offsets, const int64_t* rows, double* out_loss, double* out_grad,
                                 uint8_t* out_ok) {
  if (!row_offsets || !rows || !out_loss || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null argument");
  const int rc = check_eval_args(ctx, ds, P, MODE_LOSS, loss);
  if (rc) return rc;
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "constant gradients need Float32 / Float64");
  return grad_rowsets(ctx, ds, P, RowsetLoss{loss, nullptr}, row_offsets, rows, out_loss, out_grad, out_ok);
}

int srhip_eval_loss_grad_expr_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss_expr* e,
                                      const int64_t* row_offsets, const int64_t* rows, double* out_loss,
                                      double* out_grad, uint8_t* out_ok) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!row_offsets || !rows || !out_loss || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null argument");
  const int rc = check_loss_expr_args(ctx, ds, P, e);
  if (rc) return rc;
  return grad_rowsets(ctx, ds, P, RowsetLoss{nullptr, e}, row_offsets, rows, out_loss, out_grad, out_ok);
}

int srhip_optimize_constants_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P, const srhip_loss* loss,
                                     const int64_t* row_offsets, const int64_t* rows, const srhip_optim_options* opt,
                                     const uint64_t* tree_seeds, const double* starts_in, double* starts_out,
                                     double* out_loss, uint8_t* out_improved, int64_t* out_fcalls) {
  if (!row_offsets || !rows || !opt || !out_loss || !out_improved) return fail(SRHIP_ERR_INVALID, "null argument");
  const int rc = check_optim_args(ctx, ds, P, loss, opt);
  if (rc) return rc;
  return optimize_rowsets(ctx, ds, P, RowsetLoss{loss, nullptr}, row_offsets, rows, opt, tree_seeds, starts_in, starts_out,
                          out_loss, out_improved, out_fcalls);
}

int srhip_optimize_constants_expr_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, srhip_program* P,
                                          const srhip_loss_expr* e, const int64_t* row_offsets, const int64_t* rows,
                                          const srhip_optim_options* opt, const uint64_t* tree_seeds,
                                          const double* starts_in, double* starts_out, double* out_loss,
                                          uint8_t* out_improved, int64_t* out_fcalls) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!row_offsets || !rows || !opt || !out_loss || !out_improved) return fail(SRHIP_ERR_INVALID, "null argument");
  if (opt->iterations < 0 || opt->nrestarts < 0) return fail(SRHIP_ERR_INVALID, "negative iterations / restarts");
  const int rc = check_loss_expr_args(ctx, ds, P, e);
  if (rc) return rc;
  return optimize_rowsets(ctx, ds, P, RowsetLoss{nullptr, e}, row_offsets, rows, opt, tree_seeds, starts_in, starts_out,
                          out_loss, out_improved, out_fcalls);
}

}  // extern "C"
