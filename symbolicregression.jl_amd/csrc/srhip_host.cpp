// srhip_host.cpp — host side of libsrhip.so: program upload, device datasets, the evaluation driver
// and the C ABI declared in include/srhip.h.  The tree compiler (Node{T} -> bytecode) is srhip_compile.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/srhip.h"
#include "srhip_internal.h"
#include "srhip_decide.h"
#include "srhip_isa.h"
#include "srhip_kernels.h"
#include "srhip_lossx.h"

using namespace srhip;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int srhip::fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
const char* srhip::last_error() { return g_err.c_str(); }

// Environment switches read per call (tests and the bench toggle them inside one process) through a
// per-thread cache: a getenv scans the whole environment (~1 us each, ~10 per evaluation); the cache
// is dropped whenever the environment's entry pointers change (every setenv / putenv / unsetenv
// replaces, adds or removes one), which a walk over those pointers detects in ~50 ns.
// (diagnostic) SRHIP_HOST_TIMING=1 timestamps: run_eval's wait and the end of eval_partials' tail
static thread_local std::chrono::steady_clock::time_point g_wait_begin, g_wait_done, g_tail_done;
extern "C" char** environ;
const char* srhip::env_get(const char* name) {
  struct Ent {
    const char* name;
    const char* val;
  };
  static thread_local uint64_t sig = 0;
  static thread_local std::vector<Ent> cache;
  uint64_t h = 1469598103934665603ull ^ (uint64_t)(uintptr_t)environ;
  for (char** e = environ; e && *e; ++e) h = (h ^ (uint64_t)(uintptr_t)*e) * 1099511628211ull;
  if (h != sig) {
    cache.clear();
    sig = h;
  }
  for (const Ent& c : cache)
    if (c.name == name || strcmp(c.name, name) == 0) return c.val;
  const char* v = getenv(name);
  cache.push_back(Ent{name, v});
  return v;
}

// ---------------------------------------------------------------------------------------------
// program upload (the compiler that fills the program's vectors: srhip_compile.cpp)
// ---------------------------------------------------------------------------------------------
// device pointers of the program's sections inside d_prog (blob_off layout)
static void set_prog_pointers(const srhip_program& P) {
  const uint8_t* d = (const uint8_t*)P.d_prog.p;
  const bool der = !P.dspec.empty();
  P.code_dev = (const Ins*)d;
  P.off_dev = (const int32_t*)(d + P.blob_off[0]);
  P.dcode_dev = der ? (const Ins*)(d + P.blob_off[1]) : nullptr;
  P.doff_dev = der ? (const int32_t*)(d + P.blob_off[2]) : nullptr;
  P.dspec_dev = der ? (const uint32_t*)(d + P.blob_off[3]) : nullptr;
  P.dmask_dev = der ? (const uint64_t*)(d + P.blob_off[4]) : nullptr;
  P.sbound_dev = P.sbound.empty() ? nullptr : (const float*)(d + P.blob_off[5]);
}

// The program's host image (upload_program built it) and, behind it, an order tail (nullable) into d_prog
// in one copy on stream st; the sections' device pointers, and ord_dev at the tail if there is one
static int push_program_image(const srhip_program& P, const std::vector<int32_t>* tail, hipStream_t st) {
  const size_t base = P.blob_off[6], bytes = tail ? tail->size() * sizeof(int32_t) : 0;
  if (tail) {
    P.blob.resize(base + bytes);
    memcpy(P.blob.data() + base, tail->data(), bytes);
  }
  HIP_TRY(P.d_prog.ensure(base + bytes));
  HIP_TRY(hipMemcpyAsync(P.d_prog.p, P.blob.data(), base + bytes, hipMemcpyHostToDevice, st));
  set_prog_pointers(P);
  P.upload_pending = false;
  if (tail) P.ord_dev = (const uint8_t*)P.d_prog.p + base;
  return SRHIP_OK;
}

int srhip::upload_program(srhip_program& P, bool sync, bool defer, hipStream_t stream) {
  HIP_TRY(hipSetDevice(P.ctx->device));
  // one host image and one copy (each hipMemcpyAsync costs a few us of API time and a blit on the
  // stream: the coalescer uploads a small program per flush)
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const bool der = !P.dspec.empty();
  const size_t n_code = P.code.size() * sizeof(Ins), n_off = P.prog_off.size() * sizeof(int32_t);
  const size_t n_dcode = der ? P.dcode.size() * sizeof(Ins) : 0, n_doff = der ? P.dprog_off.size() * sizeof(int32_t) : 0;
  const size_t n_dspec = der ? P.dspec.size() * sizeof(uint32_t) : 0, n_dmask = der ? P.dmask.size() * sizeof(uint64_t) : 0;
  const size_t o_off = al(n_code), o_dcode = o_off + al(n_off), o_doff = o_dcode + al(n_dcode);
  const size_t n_sb = P.sbound.size() * sizeof(float);
  const size_t o_dspec = o_doff + al(n_doff), o_dmask = o_dspec + al(n_dspec), o_sb = o_dmask + al(n_dmask);
  const size_t total = std::max<size_t>(16, o_sb + al(n_sb));
  P.blob.assign(total, 0);
  uint8_t* h = P.blob.data();
  if (n_code) memcpy(h, P.code.data(), n_code);
  if (n_off) memcpy(h + o_off, P.prog_off.data(), n_off);
  if (n_dcode) memcpy(h + o_dcode, P.dcode.data(), n_dcode);
  if (n_doff) memcpy(h + o_doff, P.dprog_off.data(), n_doff);
  if (n_dspec) memcpy(h + o_dspec, P.dspec.data(), n_dspec);
  if (n_dmask) memcpy(h + o_dmask, P.dmask.data(), n_dmask);
  if (n_sb) memcpy(h + o_sb, P.sbound.data(), n_sb);
  const size_t offs[7] = {o_off, o_dcode, o_doff, o_dspec, o_dmask, o_sb, total};
  memcpy(P.blob_off, offs, sizeof(offs));
  if (defer) {
    P.upload_pending = true;
    return SRHIP_OK;
  }
  // a launch order planned at creation (plan_persistent_order) travels in the same copy
  const bool with_order = !P.ord_host.empty() && P.ord_key[0] > 0;
  hipStream_t st = stream ? stream : P.ctx->stream;
  const int rc = push_program_image(P, with_order ? &P.ord_host : nullptr, st);
  if (rc) return rc;
  if (sync) HIP_TRY(hipStreamSynchronize(st));
  return SRHIP_OK;
}


// ---------------------------------------------------------------------------------------------
// evaluation driver
// ---------------------------------------------------------------------------------------------
int srhip::make_view(srhip_ctx* ctx, const srhip_dataset* ds, const int64_t* idx, int64_t nidx, bool need_y, View& v) {
  if (need_y && !ds->has_y) return fail(SRHIP_ERR_INVALID, "dataset has no y");
  if (!idx) {
    v.X = ds->X.p;
    v.y = ds->y.p;
    v.w = ds->weighted ? ds->w.p : nullptr;
    v.ld = ds->ld;
    v.m = ds->n;
    v.stats = ds->hstats.data();
    v.sum_w = ds->sum_w;
    return SRHIP_OK;
  }
  if (nidx <= 0) return fail(SRHIP_ERR_INVALID, "empty idx");
  for (int64_t i = 0; i < nidx; ++i)
    if (idx[i] < 0 || idx[i] >= ds->n) return fail(SRHIP_ERR_INVALID, "idx[%lld] = %lld out of range", (long long)i, (long long)idx[i]);
  const size_t es = dtype_size(ds->dtype);
  const int64_t ld = (nidx + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
  HIP_TRY(ctx->vX.ensure((size_t)std::max<int64_t>(1, ds->nfeat) * ld * es));
  HIP_TRY(ctx->vy.ensure((size_t)ld * es));
  HIP_TRY(ctx->vw.ensure((size_t)ld * es));
  HIP_TRY(ctx->vidx.ensure((size_t)nidx * sizeof(int64_t)));
  HIP_TRY(ctx->vstats.ensure(feature_stats_scratch(ds->nfeat) * sizeof(FeatStat)));
  HIP_TRY(ctx->h_stats.ensure((size_t)std::max<int64_t>(1, ds->nfeat) * sizeof(FeatStat)));
  HIP_TRY(hipMemcpyAsync(ctx->vidx.p, idx, (size_t)nidx * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_gather(ds->dtype, ds->X.p, ds->has_y ? ds->y.p : nullptr, ds->weighted ? ds->w.p : nullptr, ds->ld,
                        (int)ds->nfeat, (const int64_t*)ctx->vidx.p, nidx, ld, ctx->vX.p,
                        ds->has_y ? ctx->vy.p : nullptr, ds->weighted ? ctx->vw.p : nullptr, ctx->stream));
  HIP_TRY(launch_feature_stats(ds->dtype, ctx->vX.p, ld, nidx, (int)ds->nfeat, (FeatStat*)ctx->vstats.p, ctx->stream));
  if (ds->dtype != SRHIP_I32 && ds->nfeat > 0)
    HIP_TRY(hipMemcpyAsync(ctx->h_stats.p, ctx->vstats.p, (size_t)ds->nfeat * sizeof(FeatStat), hipMemcpyDeviceToHost,
                           ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  v.X = ctx->vX.p;
  v.y = ds->has_y ? ctx->vy.p : nullptr;
  v.w = ds->weighted ? ctx->vw.p : nullptr;
  v.ld = ld;
  v.m = nidx;
  v.stats = (const FeatStat*)ctx->h_stats.p;
  v.sum_w = 0.0;  // (gathered_weight_sum fills it for the callers that need it)
  return SRHIP_OK;
}

// ---- the device-allocation cache behind PoolBuf ----------------------------------------------
namespace {
struct DevPool {
  std::mutex mu;
  std::map<std::pair<int, size_t>, std::vector<void*>> free;  // (device, size class) -> blocks
  size_t cached = 0;
};
DevPool& devpool() {
  static DevPool* P = new DevPool();  // never destroyed: blocks outlive static destruction order
  return *P;
}
constexpr size_t DEVPOOL_MAX_CACHED = (size_t)512 << 20;
size_t devpool_class(size_t n) {
  size_t c = 4096;
  while (c < n) c <<= 1;
  return c;
}
}  // namespace

void* srhip::devpool_get(size_t bytes, size_t* cap) {
  const size_t c = devpool_class(bytes);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  {
    DevPool& P = devpool();
    std::lock_guard<std::mutex> g(P.mu);
    auto it = P.free.find({dev, c});
    if (it != P.free.end() && !it->second.empty()) {
      void* q = it->second.back();
      it->second.pop_back();
      P.cached -= c;
      *cap = c;
      return q;
    }
  }
  void* q = nullptr;
  if (hipMalloc(&q, c) != hipSuccess) return nullptr;
  *cap = c;
  return q;
}

void srhip::devpool_put(void* p, size_t cap, int device) {
  if (!p) return;
  DevPool& P = devpool();
  {
    std::lock_guard<std::mutex> g(P.mu);
    if (device >= 0 && P.cached + cap <= DEVPOOL_MAX_CACHED) {
      P.free[{device, cap}].push_back(p);
      P.cached += cap;
      return;
    }
  }
  (void)hipFree(p);
}

int srhip::next_fail_epoch(srhip_ctx* ctx, int64_t n, int32_t** flags, int32_t* epoch) {
  const size_t need = (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t);
  const bool fresh = !ctx->fail_flag.p || ctx->fail_flag.bytes < need;  // (a new buffer may reuse an address)
  HIP_TRY(ctx->fail_flag.ensure(need));
  if (fresh || ctx->epoch == INT32_MAX) {  // fresh buffer (or wrap): no stale epochs
    HIP_TRY(hipMemsetAsync(ctx->fail_flag.p, 0, ctx->fail_flag.bytes, ctx->stream));
    ctx->epoch = 0;
  }
  *flags = (int32_t*)ctx->fail_flag.p;
  *epoch = ++ctx->epoch;
  return SRHIP_OK;
}

int srhip::check_eval_args(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int mode,
                           const srhip_loss* loss) {
  if (!ctx || !ds || !P) return fail(SRHIP_ERR_INVALID, "null handle");
  if (!P->ctx) return fail(SRHIP_ERR_INVALID, "host-only program (created without a context) cannot be evaluated");
  if (ds->dtype != P->dtype) return fail(SRHIP_ERR_INVALID, "dataset dtype %d != program dtype %d", ds->dtype, P->dtype);
  // a dataset is read-only device memory after its (synchronised) upload: any context on its device
  // may evaluate over it (the coalescer's worker contexts share the caller's dataset)
  if (P->ctx != ctx) return fail(SRHIP_ERR_INVALID, "program belongs to a different context");
  if (ds->ctx != ctx && ds->device != ctx->device) return fail(SRHIP_ERR_INVALID, "dataset is on another device");
  if (P->maxfeat > ds->nfeat)
    return fail(SRHIP_ERR_INVALID, "tree uses feature %d but dataset has %lld features", (int)P->maxfeat, (long long)ds->nfeat);
  if (mode == MODE_LOSS) {
    if (!loss) return fail(SRHIP_ERR_INVALID, "null loss");
    if (P->dtype == SRHIP_I32 && loss->kind != SRHIP_LOSS_L2 && loss->kind != SRHIP_LOSS_L1)
      return fail(SRHIP_ERR_UNSUPPORTED, "Int32 datasets support L2/L1 losses only");
    if (loss->kind < SRHIP_LOSS_L2 || loss->kind > SRHIP_LOSS_DWD_MARGIN)
      return fail(SRHIP_ERR_UNSUPPORTED, "loss kind %d", loss->kind);
  }
  return SRHIP_OK;
}

// the argument checks the entry points that take a loss expression share (srhip_eval_loss_expr,
// srhip_eval_loss_grad_expr, srhip_optimize_constants_expr)
int srhip::check_loss_expr_args(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss_expr* e) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  const int rc = check_eval_args(ctx, ds, P, MODE_PRED, nullptr);
  if (rc) return rc;
  return check_loss_expr_data(ds, P->dtype, e);
}

int srhip::check_loss_expr_data(const srhip_dataset* ds, int dtype, const srhip_loss_expr* e) {
  if (!ds) return fail(SRHIP_ERR_INVALID, "null handle");
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "loss expressions are Float32 / Float64 only (Int32 program)");
  if (dtype != e->prog.dtype)
    return fail(SRHIP_ERR_INVALID, "loss expression dtype %d != program dtype %d", e->prog.dtype, dtype);
  if (!ds->has_y) return fail(SRHIP_ERR_INVALID, "dataset has no y");
  if (ds->weighted != (e->prog.nargs == 3))
    return fail(SRHIP_ERR_INVALID, "a%s dataset needs a loss expression of nargs = %d (this one has nargs = %d)",
                ds->weighted ? " weighted" : "n unweighted", ds->weighted ? 3 : 2, (int)e->prog.nargs);
  return SRHIP_OK;
}

// run_eval's device-decided precise pass: the reduction lists the trees whose overflow bound needs
// the precise pass, and the precise launch + its reduction follow on the stream before the one host
// synchronisation (no host round trip between the main launch and the precise pass); its output: PreciseOut
struct DevPrecise {
  bool used = false;
  int32_t count = 0;             // trees the device listed (may exceed DEV_PRECISE_MAX)
  int stride = 1;
  std::vector<int32_t> list;     // the first min(count, DEV_PRECISE_MAX) of them
  std::vector<double> opsums;    // [list.size()][stride]
};

// Device stage: one interpreter launch over the view + the per-tree reduction.  Fills the partials
// (sums layout above; chk[T]) and, in MODE_PRED, out_pred.  dp (nullable): also the device-decided
// precise pass (multi-block launches; single-block launches finish inside the interpreter and leave
// the precise pass to the caller).
// Row shards (run_eval_sharded): the reduction writes each tree's loss sum and check statistic into the
// exchange's device buffer instead of host memory (sums[2t] / chk stay to be filled from the all-reduced
// buffer); the rows each tree was evaluated on come back for the caller's lost-block check.
struct ShardDev {
  void* d_loss = nullptr;
  void* d_chk = nullptr;
  size_t zero_bytes = 0;  // [loss | chk] cleared before the launch (static-fail trees are never written)
};

// The device-listed precise pass, enqueued on the context's stream: the plain program over the trees
// of the device list ulist ([count, trees ...], count read by the launch, at most cap of them):
// one-tile row blocks and one-wave workgroups, G workgroups per row block, workgroup g taking the
// listed slots g, g + G, ... (G from the program's last count: an unused workgroup still costs its
// dispatch, and a count past G costs one launch longer, not another host round trip) -- K_MAX,
// global reads; then the double-double reduction of the per-block operator sums into the context's
// coherent h_pout ([count, list ..., sums]), which also clears the list.
// The precise pass's scratch (the per-block operator sums of the listed trees, their reduction's host
// output), ensured before the evaluation's main launch: a regrowth frees the old buffer, which
// synchronises the device -- after the launch that would wait for the whole evaluation.  Sized for
// a power-of-two operator count (32 at least: one size for every population of trees up to 33
// nodes) and at most 64 MB of per-block sums: the list's capacity (*cap, <= DEV_PRECISE_MAX) shrinks
// for very long row ranges (4 at least); trees past it take the host-written list.
constexpr size_t PRECISE_SLAB_MAX = (size_t)64 << 20;
constexpr int PRECISE_GRID_X = 2048;
static size_t precise_per_tree(const srhip_program* P, const View& v, int* sa_out = nullptr) {
  int sa = 32;
  while (sa < P->max_ops) sa <<= 1;
  if (sa_out) *sa_out = sa;
  const int rows = 64 * pick_rows_per_lane(P->dtype, K_MAX, MODE_PRECISE, v.m);
  const int64_t nrb = std::max<int64_t>(1, (v.m + rows - 1) / rows);
  return (size_t)sa * nrb * sizeof(double);
}
static int precise_cap(const srhip_program* P, const View& v, int cap) {
  return (int)std::max<int64_t>(std::min<int64_t>(cap, (int64_t)(PRECISE_SLAB_MAX / precise_per_tree(P, v))), 4);
}
static int ensure_dev_precise(srhip_ctx* ctx, const srhip_program* P, const View& v, int* cap, ResultSet* rs) {
  int sa = 32;
  const size_t per_tree = precise_per_tree(P, v, &sa);
  *cap = precise_cap(P, v, *cap);
  HIP_TRY(ctx->slab_prec.ensure((size_t)*cap * per_tree));
  HIP_TRY(rs->h_pout.ensure(PreciseOut::bytes(sa), hipHostMallocCoherent));
  return SRHIP_OK;
}
static int enqueue_dev_precise(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const View& v,
                               int32_t* ulist, int cap, int G, int* out_stride, ResultSet* rs) {
  const int dtype = P->dtype;
  const int stride = std::max(1, P->max_ops);
  const int Rp = pick_rows_per_lane(dtype, K_MAX, MODE_PRECISE, v.m);
  G = std::max(1, std::min(G, cap));
  LaunchPlan Lp = plan_launch(ctx->num_cu, dtype, ds->nfeat, false, false, v.m, G, 64 * Rp);
  Lp.rb_rows = 64 * Rp;
  Lp.nrb = (int)((v.m + Lp.rb_rows - 1) / Lp.rb_rows);
  {
    int c = cap;
    const int rc = ensure_dev_precise(ctx, P, v, &c, rs);
    if (rc) return rc;
    if (c < cap) return fail(SRHIP_ERR_INVALID, "precise list of %d trees past its capacity %d", cap, c);
  }
  EvalArgs q{};
  q.code = P->code_dev;
  q.prog_off = P->off_dev;
  q.order = ulist + 1;
  q.X = v.X;
  q.ld = v.ld;
  q.nvalid = v.m;
  q.ntrees = cap;
  q.grid_interleave = 1;  // grid.y = G workgroups share the list's slots interleaved
  q.nfeat = (int32_t)ds->nfeat;
  q.rb_rows = Lp.rb_rows;
  q.nrb = Lp.nrb;
  q.trees_per_group = 1;
  q.slab_prec = ctx->slab_prec.p;
  q.prec_stride = stride;
  q.max_steps = P->max_len;
  q.dev_count = ulist;
  q.wg_waves = 1;
  q.prec_assign = 1;  // one-tile row blocks
  // at most PRECISE_GRID_X workgroups per group, each striding over the row blocks: the launch runs
  // whether or not the list holds a tree, and with an empty list its cost is the workgroups'
  // dispatch (10M rows: 19532 x G one-wave workgroups, 41 us)
  q.block_stride = 1;
  HIP_TRY(launch_eval(dtype, q, Rp, K_MAX, MODE_PRECISE, false, dim3(std::min(Lp.nrb, PRECISE_GRID_X), G), 16,
                      ctx->stream));
  const PreciseOut out{rs->h_pout.p};
  HIP_TRY(launch_precise_reduce((const double*)ctx->slab_prec.p, Lp.nrb, stride, ulist, cap, G, DEV_PRECISE_MAX,
                                out.head(), out.sums(), ctx->stream));
  *out_stride = stride;
  return SRHIP_OK;
}

// An evaluation between its launches (eval_issue) and the reading of its records (eval_collect): what
// the second half needs of the first.  The launches of several jobs may be in flight on the context's
// stream at once (srhip_eval_loss_submit), each with its own result set.
struct EvalJob {
  ResultSet* rs = nullptr;
  bool launched = false, devp = false;
  int mode = 0, dtype = 0;
  int32_t nt = 0;
  EvalPlan pl{};  // the launch's plan (persistent, fused, expect_items)
  std::vector<int32_t> live;
  UndecidedList ul;
  DevBuf pred;  // MODE_PRED's device output (synchronous calls only)
  float fbound = 0.0f;  // Float32: the features' max |x| (feature_bound: the +/- bound's F)
  // the one-launch form of a loss expression (eval_issue_lossx; mode is MODE_PRED): the loss program, the
  // launch's order (tree of each slot: the result set's h_loss holds the loss sums by slot, then the weights'
  // sum), and the order's upload [order | identity | prog_off by slot] with its device copy
  const LossxProgram* lx = nullptr;
  std::vector<int32_t> lx_order, lx_tail;
  PoolBuf lx_dev;
};

// What plan_eval reads of a context and a program with nlive live trees (in EvalPlanIn's order): an
// unweighted, unsharded MODE_LOSS launch of loss kind 0 over WIDE_MIN_ROWS rows -- the launch
// plan_persistent_order assumes -- until the caller says otherwise.  A persistent launch's order always
// carries its slot records (eval_issue makes them).
static EvalPlanIn plan_input(const srhip_ctx* ctx, const srhip_program& P, int32_t nlive) {
  return EvalPlanIn{P.dtype, MODE_LOSS, nlive, WIDE_MIN_ROWS, P.maxfeat, (int32_t)P.dspec.size(), P.kmax, P.dkmax,
                    has_wide_ops(P.unaops), /*weighted*/ false, /*sharded*/ false, /*have_recs*/ true,
                    /*loss_kind*/ 0, ctx->num_cu, ctx->lds_max};
}

// What follows an evaluation's interpreter launch on the stream, for every launch form: the undecided list's
// set-up, the Float32 +/- bounds, the per-tree reduction of the launch's slabs into the result set's records
// (r.run: a fused single-block launch has written them itself) and the device-listed precise pass.
struct ReduceIn {
  bool run;
  const void* slab_loss;
  int nch, cpb;
  const void* slab_chk;
  int nrb, nslots;
  const int32_t* order;
  void* out_loss;
  void* out_chk;
  const int32_t* slab_rows;
  bool chk_inf;
  int32_t* items_done;
  int64_t* out_items;
};
static int issue_records(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const View& v, DevPrecise* dp,
                         EvalJob& J, bool devp, int ucap, const ReduceIn& r) {
  ResultSet* const rs = J.rs;
  UndecidedList& ul = J.ul;
  int ul_groups = 4;
  if (devp) {
    if (!ctx->d_ulist.p) {
      // [count, DEV_PRECISE_MAX trees, the precise reduction's finished-workgroup counter]
      HIP_TRY(ctx->d_ulist.ensure((2 + DEV_PRECISE_MAX) * sizeof(int32_t)));
      HIP_TRY(hipMemsetAsync(ctx->d_ulist.p, 0, ctx->d_ulist.bytes, ctx->stream));
    }
    ul.ulist = (int32_t*)ctx->d_ulist.p;
    // trees past the list's capacity are settled by the same pass over a host-written list (run_eval).
    // The precise launch's workgroups per row block: the program's last count plus two (4 at least)
    ul.umax = ucap;
    ul.rows = (double)v.m;
    ul_groups = std::min(ul.umax, std::max(4, P->und_hint + 2));
  }
  if (P->dtype == SRHIP_F32) {  // the reduction raises each tree's statistic to its +/- bound
    ul.sbound = P->sbound_dev;
    ul.fbound = J.fbound;
  }
  if (r.run)
    HIP_TRY(launch_reduce(P->dtype, r.slab_loss, r.nch, r.cpb, r.slab_chk, r.nrb, r.nslots, r.order, r.out_loss, r.out_chk,
                          ctx->stream, r.slab_rows, (int64_t*)rs->h_rows.p, ul, r.chk_inf, r.items_done, r.out_items));
  if (devp) {
    int stride = 1;
    const int rc = enqueue_dev_precise(ctx, ds, P, v, ul.ulist, ul.umax, ul_groups, &stride, rs);
    if (rc) return rc;
    dp->used = true;
    dp->stride = stride;
  }
  return SRHIP_OK;
}

// eval_issue for a loss expression in one launch (J.lx; srhip_eval_lossx.hip): the fused launch and its
// finishing sums, then what a MODE_PRED grid launch is followed by -- the reduction of the check statistics and
// rows evaluated into the result set's records, the device-listed precise pass -- so eval_collect and
// run_complete's settle read them as they read srhip_eval_predict's.
static int eval_issue_lossx(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const View& v, DevPrecise* dp,
                            EvalJob& J) {
  const int dtype = P->dtype;
  const int32_t nt = P->ntrees;
  ResultSet* const rs = J.rs;
  const int nl = (int)J.live.size();
  const bool weighted = ds->weighted;
  const LossxPlan lp = plan_eval_lossx(LossxPlanIn{dtype, nl, v.m, P->maxfeat, ctx->num_cu, ctx->lds_max});
  if (lp.nblocks > 0x7fffffffLL / std::max(1, lp.ngroups) || (int64_t)nl * lp.nblocks > 0x7fffffffLL)
    return fail(SRHIP_ERR_INVALID, "loss expression: %d trees x %lld row blocks is more than one launch indexes", nl,
                (long long)lp.nblocks);
  const int nblocks = (int)lp.nblocks;
  // what eval_collect reads of a plan: a grid launch whose reduction wrote the records
  J.pl = EvalPlan{};
  J.pl.kind = PLAN_GRID;
  J.pl.R = lp.R;
  J.pl.K = K_MAX;
  J.pl.L = LaunchPlan{lp.rb_rows, nblocks, lp.ngroups, lp.tpg, lp.xlds, lp.lds};
  // one group in descending cost: an item's trees cost alike, and the costliest items are dealt first
  J.lx_order = make_order(*P, J.live, std::vector<int32_t>{0, nl}, false);
  std::vector<int32_t>& tail = J.lx_tail;  // lives in the job: its copy is asynchronous
  tail.assign(J.lx_order.begin(), J.lx_order.end());
  tail.resize(3 * (size_t)nl);
  for (int sl = 0; sl < nl; ++sl) {
    tail[(size_t)nl + sl] = sl;
    tail[2 * (size_t)nl + sl] = P->prog_off[J.lx_order[sl]];
  }
  const int32_t* d_tail;
  {
    std::lock_guard<std::mutex> g(P->ord_mu);
    if (P->upload_pending) {  // deferred program upload (the coalescer's per-flush program): one copy
      const int rc = push_program_image(*P, &tail, ctx->stream);
      if (rc) return rc;
      d_tail = (const int32_t*)P->ord_dev;
      P->ord_key[0] = -1;  // what ord_dev holds is no plan_eval order
    } else {
      HIP_TRY(J.lx_dev.ensure(tail.size() * sizeof(int32_t)));
      HIP_TRY(hipMemcpyAsync(J.lx_dev.p, tail.data(), tail.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
      d_tail = (const int32_t*)J.lx_dev.p;
    }
  }
  const int nslots = nl + (weighted ? 1 : 0);
  HIP_TRY(ctx->slab_chk.ensure((size_t)nl * nblocks * 8));
  HIP_TRY(ctx->slab_rows.ensure((size_t)nl * nblocks * sizeof(int32_t)));
  HIP_TRY(ctx->lossx_pred.ensure(lp.scratch_bytes));
  HIP_TRY(ctx->lossx_part.ensure((size_t)nslots * nblocks * sizeof(double)));
  HIP_TRY(rs->h_loss.ensure((size_t)(nt + 1) * 8, hipHostMallocCoherent));  // by slot, then the weights' sum
  HIP_TRY(rs->h_chk.ensure((size_t)nt * 8, hipHostMallocCoherent));
  HIP_TRY(rs->h_rows.ensure((size_t)(nt + 1) * 8, hipHostMallocCoherent));
  if (dtype == SRHIP_F32) {
    if (!P->sbound_dev || P->sbound.size() != 4 * (size_t)P->ntrees)
      return fail(SRHIP_ERR_INVALID, "Float32 program without its +/- bounds");
    J.fbound = feature_bound(v.stats, ds->nfeat);
  }
  EvalLossxArgs q{};
  EvalArgs& a = q.e;
  a.code = P->code_dev;
  a.prog_off = d_tail + 2 * (size_t)nl;
  a.order = d_tail + nl;
  a.X = v.X;
  a.slab_chk = ctx->slab_chk.p;
  a.slab_rows = (int32_t*)ctx->slab_rows.p;
  a.ld = v.ld;
  a.nvalid = v.m;
  a.ntrees = nl;
  a.nfeat = P->maxfeat;
  a.rb_rows = lp.rb_rows;
  a.nrb = nblocks;
  a.trees_per_group = lp.tpg;
  a.max_steps = P->max_len;
  q.lx = *J.lx;
  q.y = v.y;
  q.w = weighted ? v.w : nullptr;
  q.pred = ctx->lossx_pred.p;
  q.partials = (double*)ctx->lossx_part.p;
  q.m = v.m;
  q.nblocks = nblocks;
  q.ngroups = lp.ngroups;
  const bool devp = dp && !env_flag("SRHIP_NO_DEVICE_PRECISE");
  int ucap = std::max(1, std::min(DEV_PRECISE_MAX, env_int("SRHIP_PRECISE_LIST", DEV_PRECISE_MAX)));
  if (devp) {
    const int rc = ensure_dev_precise(ctx, P, v, &ucap, rs);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(rs->ev0, ctx->stream));
  HIP_TRY(launch_eval_lossx(dtype, q, lp.xlds, lp.wgs, lp.lds, (double*)rs->h_loss.p, ctx->stream));
  HIP_TRY(hipEventRecord(rs->ev1, ctx->stream));
  J.launched = true;
  J.devp = devp;
  {
    const int rc = issue_records(ctx, ds, P, v, dp, J, devp, ucap,
                                 ReduceIn{true, nullptr, 0, 0, ctx->slab_chk.p, nblocks, nl, d_tail, nullptr, rs->h_chk.p,
                                          a.slab_rows, false, nullptr, nullptr});
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(rs->done, ctx->stream));
  return SRHIP_OK;
}

static int eval_issue(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int mode, const srhip_loss* loss,
                      const View& v, void* out_pred, double* sums, double* chk, DevPrecise* dp, ShardDev* sd,
                      EvalJob& J) {
  const int dtype = P->dtype;
  const int32_t nt = P->ntrees;
  ResultSet* const rs = J.rs;
  J.mode = mode;
  J.dtype = dtype;
  J.nt = nt;
  const int64_t nf = ds->nfeat;
  const bool weighted = ds->weighted && mode == MODE_LOSS;
  for (size_t i = 0; i < sums_len(nt, nf); ++i) sums[i] = 0.0;
  for (int32_t t = 0; t < nt; ++t) {
    chk[t] = 0.0;
    sums[2 * (size_t)t + 1] = weighted ? v.sum_w : (double)v.m;
  }
  for (int64_t f = 0; f < nf; ++f) {
    sums[2 * (size_t)nt + 2 * f] = v.stats[f].sum;
    sums[2 * (size_t)nt + 2 * f + 1] = (double)v.stats[f].nonfinite;
  }
  sums[2 * (size_t)nt + 2 * nf] = (double)v.m;
  std::vector<int32_t>& live = J.live;
  live.clear();
  live.reserve(nt);
  for (int32_t t = 0; t < nt; ++t)
    if (!tree_static_fail(*P, t)) live.push_back(t);
  if (live.empty()) return SRHIP_OK;
  if (J.lx) return eval_issue_lossx(ctx, ds, P, v, dp, J);
  const size_t es = dtype_size(dtype);
  const int nl = (int)live.size();
  // how the launch runs (srhip_plan.h): from here on the plan is only read
  EvalPlanIn in = plan_input(ctx, *P, nl);
  in.mode = mode;
  in.m = v.m;
  in.weighted = weighted;
  in.sharded = sd != nullptr;
  in.loss_kind = loss ? loss->kind : 0;
  const EvalPlan& pl = J.pl = plan_eval(in);
  const LaunchPlan& L = pl.L;
  const bool persistent = pl.kind == PLAN_PERSISTENT, use_d = pl.use_d;
  const int R = pl.R, K = pl.K, nch = pl.nch, cpb = pl.cpb, probe_blocks = pl.probe_blocks;
  const void* d_order;
  int rec_at = -1;  // the plan's slot records behind the order (int32 units), if it has them
  // persistent launches: one group, the order globally by descending cost (the probe's uniform
  // groups of one tree per wave are consecutive slots of it)
  const std::vector<int32_t> goff = persistent ? std::vector<int32_t>{0, nl} : shape_groups(L, nl, ctx->num_cu);
  {
    std::lock_guard<std::mutex> g(P->ord_mu);
    if (P->upload_pending || P->ord_key[0] != L.groups || P->ord_key[1] != L.tpg || P->ord_key[2] != (int)use_d ||
        P->ord_goff != goff || (persistent && P->ord_recs < 0)) {
      std::vector<int32_t>& order = P->ord_host;  // lives in the program: the copy below is asynchronous
      order = make_order(*P, live, goff, use_d);
      order.insert(order.end(), goff.begin(), goff.end());  // the group offsets follow the order
      P->ord_recs = persistent ? append_slot_records(*P, order, nl, use_d) : -1;  // ... and the slot records
      if (P->upload_pending) {  // deferred program upload: program and order in one copy
        const int rc = push_program_image(*P, &order, ctx->stream);
        if (rc) return rc;
      } else {
        HIP_TRY(P->d_order.ensure(order.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(P->d_order.p, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                               ctx->stream));
        P->ord_dev = P->d_order.p;
      }
      P->ord_key[0] = L.groups;
      P->ord_key[1] = L.tpg;
      P->ord_key[2] = (int)use_d;
      P->ord_goff = goff;
    }
    d_order = P->ord_dev;
    rec_at = P->ord_recs;
  }
  HIP_TRY(ctx->slab_loss.ensure((size_t)nl * L.nrb * cpb * 8));
  HIP_TRY(ctx->slab_chk.ensure((size_t)nl * L.nrb * 8));
  // the reduction writes the per-tree results straight into coherent pinned host memory (no
  // device-to-host copies on the stream)
  HIP_TRY(rs->h_loss.ensure((size_t)nt * 8, hipHostMallocCoherent));
  HIP_TRY(rs->h_chk.ensure((size_t)nt * 8, hipHostMallocCoherent));
  HIP_TRY(rs->h_rows.ensure((size_t)(nt + 1) * 8, hipHostMallocCoherent));  // [nt]: persistent items evaluated
  EvalArgs a{};
  a.code = use_d ? P->dcode_dev : P->code_dev;
  a.prog_off = use_d ? P->doff_dev : P->off_dev;
  a.order = (const int32_t*)d_order;
  a.nd = use_d ? in.nd : 0;
  a.dspec = use_d ? P->dspec_dev : nullptr;
  a.dmask = use_d ? P->dmask_dev : nullptr;
  if (dtype == SRHIP_F32) {
    // (every Float32 program carries its trees' +/- bounds: the interpreter folds no +/-)
    if (!P->sbound_dev || P->sbound.size() != 4 * (size_t)P->ntrees)
      return fail(SRHIP_ERR_INVALID, "Float32 program without its +/- bounds");
    J.fbound = feature_bound(v.stats, ds->nfeat);
  }
  a.X = v.X;
  a.y = v.y;
  a.w = weighted ? v.w : nullptr;
  a.slab_loss = ctx->slab_loss.p;
  a.slab_chk = ctx->slab_chk.p;
  a.ld = v.ld;
  a.nvalid = v.m;
  a.ntrees = nl;
  a.nfeat = P->maxfeat;  // staged feature columns
  a.rb_rows = L.rb_rows;
  a.nrb = L.nrb;
  a.nch = nch;
  a.cpb = cpb;
  a.trees_per_group = L.tpg;
  a.group_off = (const int32_t*)d_order + nl;
  a.loss_kind = loss ? loss->kind : 0;
  a.loss_p0 = loss ? loss->p0 : 0.0;
  a.weighted = weighted ? 1 : 0;
  a.has_y = mode == MODE_LOSS ? 1 : 0;
  a.max_steps = use_d ? P->dmax_len : P->max_len;
  a.debug_stop = debug_stop();
  a.wg_waves = pl.wg_waves;
  if (pl.fused) {  // one row block: the waves finish the per-tree reduction themselves
    a.fused = 1;
    a.fused_loss = mode == MODE_LOSS ? rs->h_loss.p : nullptr;
    a.fused_chk = dtype == SRHIP_I32 ? nullptr : rs->h_chk.p;
    a.fused_rows = (int64_t*)rs->h_rows.p;
  } else {
    HIP_TRY(ctx->slab_rows.ensure((size_t)nl * L.nrb * sizeof(int32_t)));
    a.slab_rows = (int32_t*)ctx->slab_rows.p;
  }
  const bool devp = dp && !a.fused && dtype != SRHIP_I32 && !env_flag("SRHIP_NO_DEVICE_PRECISE");
  // the device list's capacity: DEV_PRECISE_MAX (SRHIP_PRECISE_LIST: smaller, read per call -- the
  // tests' way to the overflow path), less for very long row ranges (ensure_dev_precise)
  int ucap = std::max(1, std::min(DEV_PRECISE_MAX, env_int("SRHIP_PRECISE_LIST", DEV_PRECISE_MAX)));
  if (devp) {
    const int rc = ensure_dev_precise(ctx, P, v, &ucap, rs);
    if (rc) return rc;
  }
  a.early_exit = mode == MODE_LOSS && early_exit_on() ? 1 : 0;
  if (a.early_exit) {
    const int rc = next_fail_epoch(ctx, nl, &a.fail_flag, &a.epoch);
    if (rc) return rc;
  }
  if (trace_on()) {
    HIP_TRY(ctx->h_dbg.ensure(64 * sizeof(int32_t), hipHostMallocCoherent));
    memset(ctx->h_dbg.p, 0xff, 64 * sizeof(int32_t));
    a.dbg = (int32_t*)ctx->h_dbg.p;
  }
  DevBuf& pred = J.pred;
  if (mode == MODE_PRED) {
    HIP_TRY(pred.ensure((size_t)nt * v.m * es));
    a.out_pred = pred.p;
  }
  dim3 grid(L.nrb, (unsigned)goff.size() - 1);
  // a probe with tile claims zeroes the counter itself, so a launch still in flight (an earlier
  // submitted evaluation, not yet seen to drain) needs no fill in front of this one
  if (persistent && (!ctx->block_ctr.p || (ctx->block_ctr_dirty && !pl.probe_tile_claims))) {
    // zeroed once: every persistent launch that drains its claims leaves it at zero (its last claim
    // resets it); again after a launch that was never seen to complete (an error return between the
    // launch and its synchronisation, or a lost row block below)
    // [claim counter, items evaluated]
    HIP_TRY(ctx->block_ctr.ensure(2 * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(ctx->block_ctr.p, 0, 2 * sizeof(int32_t), ctx->stream));
    ctx->block_ctr_dirty = false;
  }
  if (persistent) ctx->block_ctr_dirty = true;  // until the launch is seen to have drained
  if (sd) HIP_TRY(hipMemsetAsync(sd->d_loss, 0, sd->zero_bytes, ctx->stream));
  HIP_TRY(hipEventRecord(rs->ev0, ctx->stream));
  if (persistent) {
    if (probe_blocks > 0) {
      // leading row blocks, one tree per wave (uniform groups of consecutive slots), with the plain
      // program: a probe workgroup serves 16 trees, too few to pay for deriving columns (the values,
      // partials and slots are the same either way)
      // workgroup (b, g) of the probe takes slots g, g + G, g + 2G, ... (grid_interleave): each CU
      // gets one of the most expensive trees and cheap ones, not 16 of the most expensive (which
      // four waves per SIMD would share)
      EvalArgs q = a;
      q.group_off = nullptr;
      q.trees_per_group = eval_waves(R, K);
      q.grid_interleave = 1;
      // one (tree, tile) per claim: the costliest tree's two tiles run on two waves at once (the
      // probe's duration is that tree's); chk / rows of the probe blocks combine by atomics from 0
      // (the probe's workgroups zero their own combining entries and the persistent launch's block
      // counter: no memset launches on the stream)
      if (pl.probe_tile_claims) {
        q.tile_claims = 1;
        q.zero_ctr = (int32_t*)ctx->block_ctr.p;
      }
      q.code = P->code_dev;
      q.prog_off = P->off_dev;
      q.max_steps = P->max_len;
      q.nd = 0;
      q.dspec = nullptr;
      q.dmask = nullptr;
      const size_t qlds = (size_t)(P->maxfeat + 1 + (weighted ? 1 : 0)) * L.rb_rows * es + 16;
      const dim3 pgrid(probe_blocks, (unsigned)((nl + q.trees_per_group - 1) / q.trees_per_group));
      HIP_TRY(launch_eval(dtype, q, R, K, mode, true, pgrid, qlds, ctx->stream));
    }
    a.persistent = 1;
    a.block0 = probe_blocks;
    a.block_ctr = (int32_t*)ctx->block_ctr.p;
    // (diagnostic, tests only) a counter left non-zero when the main launch starts (after the probe,
    // which zeroes it): the launch skips that many row blocks, which the lost-block check after it must
    // report
    if (const int seed = env_int("SRHIP_DEBUG_BLOCK_CTR", 0)) {
      const int32_t h = (int32_t)seed;
      HIP_TRY(hipMemcpyAsync(ctx->block_ctr.p, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    a.tail_slices = pl.tail_slices;  // the last round in equal shares (plan_eval)
    a.tail_blocks = pl.tail_blocks;
    a.tail_shares = pl.tail_shares;
    if (pl.hot) a.recs = (const SlotRec*)((const int32_t*)d_order + rec_at);
    HIP_TRY(launch_eval(dtype, a, R, K, mode, true, dim3(pl.wgs, 1), L.lds, ctx->stream));
    if (a.recs) ++ctx->hot_launches;  // (counted once the launch is enqueued)
  } else {
    HIP_TRY(launch_eval(dtype, a, R, K, mode, L.xlds, grid, L.lds, ctx->stream));
  }
  HIP_TRY(hipEventRecord(rs->ev1, ctx->stream));
  J.launched = true;
  J.devp = devp;
  if (trace_on()) {  // poll the kernel's progress words for up to 10 s, then abort loudly
    const volatile int32_t* d = (const volatile int32_t*)ctx->h_dbg.p;
    int32_t last[16];
    for (int i = 0; i < 16; ++i) last[i] = -2;
    for (int it = 0; it < 10000; ++it) {
      hipError_t q = hipStreamQuery(ctx->stream);
      bool changed = false;
      for (int i = 0; i < 16; ++i) changed |= d[i] != last[i];
      if (changed) {
        for (int i = 0; i < 16; ++i) last[i] = d[i];
        fprintf(stderr, "[srhip] kernel progress: stage=%d tree=%d waves=%d,%d,%d,%d,%d,%d,%d,%d\n", last[0], last[1],
                last[8], last[9], last[10], last[11], last[12], last[13], last[14], last[15]);
        fflush(stderr);
      }
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) HIP_TRY(q);
      usleep(1000);
      if (it == 9999) {
        fprintf(stderr, "[srhip] kernel did not finish in 10 s; aborting\n");
        fflush(stderr);
        abort();
      }
    }
  }
  {
    const int rc = issue_records(
        ctx, ds, P, v, dp, J, devp, ucap,
        ReduceIn{!a.fused, mode == MODE_LOSS ? ctx->slab_loss.p : nullptr, nch, cpb,
                 dtype == SRHIP_I32 ? nullptr : ctx->slab_chk.p, L.nrb, nl, (const int32_t*)d_order,
                 mode == MODE_LOSS ? (sd ? sd->d_loss : rs->h_loss.p) : nullptr,
                 dtype == SRHIP_I32 ? nullptr : (sd ? sd->d_chk : rs->h_chk.p), a.slab_rows, sd != nullptr,
                 persistent ? (int32_t*)ctx->block_ctr.p + 1 : nullptr,
                 persistent ? (int64_t*)rs->h_rows.p + nt : nullptr});
    if (rc) return rc;
  }
  // (no host output asked for: srhip_eval_loss_expr reads the predictions where they are, J.pred)
  if (mode == MODE_PRED && out_pred)
    HIP_TRY(hipMemcpyAsync(out_pred, pred.p, (size_t)nt * v.m * es, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipEventRecord(rs->done, ctx->stream));
  return SRHIP_OK;
}

// The second half: the records of a job whose work has completed (the caller waited for its stream or
// its result set's completion event).
static int eval_collect(srhip_ctx* ctx, const srhip_program* P, const View& v, double* sums, double* chk,
                        DevPrecise* dp, ShardDev* sd, EvalJob& J) {
  ResultSet* const rs = J.rs;
  const int dtype = J.dtype, mode = J.mode;
  const int32_t nt = J.nt;
  const std::vector<int32_t>& live = J.live;
  const bool persistent = J.pl.kind == PLAN_PERSISTENT, devp = J.devp;
  const UndecidedList& ul = J.ul;
  ctx->last_ev0 = rs->ev0;
  ctx->last_ev1 = rs->ev1;
  ctx->timed = true;
  if (devp) {
    const PreciseOut out{rs->h_pout.p};
    dp->count = out.count();
    P->und_hint = dp->count;
    const int nu = std::min(dp->count, ul.umax);
    dp->list.assign(out.list(), out.list() + nu);
    dp->opsums.assign(out.sums(), out.sums() + (size_t)nu * dp->stride);
  }
  Records rec;
  rec.read(dtype, nt, mode == MODE_LOSS ? rs->h_loss.p : nullptr, rs->h_chk.p, rs->h_rows.p);
  for (int32_t t : live) {
    if (sd) break;  // the shard's loss sums and statistics are in the exchange's device buffer
    if (mode == MODE_LOSS) sums[2 * (size_t)t] = rec.loss_sum(t);
    // a single-block launch's records come straight from the interpreter: its +/- bound applied here
    const bool bound = dtype == SRHIP_F32 && J.pl.fused;
    chk[t] = bound ? skip_bound_apply((float)rec.chk_raw(t), P->sbound.data() + 4 * (size_t)t, J.fbound) : rec.chk_raw(t);
  }
  if (persistent) {
    // every row block was claimed exactly once: the workgroups' evaluated items add up to the launch's
    // item count (a counter left non-zero by a launch that never drained would make this one skip
    // blocks silently -- and leave the skipped blocks' stale partials in the slabs)
    const int64_t done = ((const int64_t*)rs->h_rows.p)[nt];
    if (done != J.pl.expect_items)
      return fail(SRHIP_ERR_DEVICE, "persistent launch evaluated %lld of %d row-block items (row-block counter "
                  "not at zero); the counter is reset for the next launch", (long long)done, J.pl.expect_items);
    ctx->block_ctr_dirty = false;
  }
  // the launch's work, counted on the device (rows each tree was evaluated on)
  for (int i = 0; i < 4; ++i) ctx->work[i] = 0;
  for (int32_t t : live) count_work(ctx->work, rec.rows_done(t), v.m, tree_size(*P, t));
  g_tail_done = std::chrono::steady_clock::now();
  return SRHIP_OK;
}

// Device stage, synchronous: the launches, the wait, the records (result set 0).
static int eval_partials(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int mode, const srhip_loss* loss,
                         const View& v, void* out_pred, double* sums, double* chk, DevPrecise* dp = nullptr,
                         ShardDev* sd = nullptr) {
  EvalJob J;
  J.rs = &ctx->rs[0];
  int rc = eval_issue(ctx, ds, P, mode, loss, v, out_pred, sums, chk, dp, sd, J);
  if (rc || !J.launched) return rc;
  rc = stream_wait(ctx);
  if (rc) return rc;
  return eval_collect(ctx, P, v, sums, chk, dp, sd, J);
}

// Precise stage: per-(tree, operator node) f64 sums over the view's rows for the selected trees;
// opsums[u * max(1, max_ops) + k].
static int eval_precise(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const View& v,
                        const int32_t* trees, int32_t nu, double* opsums, bool grad = false) {
  const int dtype = P->dtype;
  const int stride = std::max(1, grad ? P->gmax_ops : P->max_ops);
  for (size_t i = 0; i < (size_t)nu * stride; ++i) opsums[i] = 0.0;
  if (nu == 0 || dtype == SRHIP_I32) return SRHIP_OK;
  const int R = pick_rows_per_lane(dtype, K_MAX, MODE_PRECISE, v.m);
  LaunchPlan Lp = plan_launch(ctx->num_cu, dtype, ds->nfeat, false, false, v.m, nu, 64 * R);
  Lp.groups = 1;
  Lp.tpg = nu;
  const size_t slab_bytes = (size_t)nu * stride * Lp.nrb * sizeof(double);
  HIP_TRY(ctx->slab_prec.ensure(slab_bytes));
  HIP_TRY(hipMemsetAsync(ctx->slab_prec.p, 0, slab_bytes, ctx->stream));
  // the list [count | trees | the reduction's finished-workgroup counter] in one copy from pinned
  // staging: the precise launch reads the trees, precise_reduce_kernel the count and the counter
  HIP_TRY(ctx->h_plist.ensure((size_t)(nu + 2) * sizeof(int32_t)));
  int32_t* hlist = (int32_t*)ctx->h_plist.p;
  hlist[0] = nu;
  memcpy(hlist + 1, trees, (size_t)nu * sizeof(int32_t));
  hlist[1 + nu] = 0;
  HIP_TRY(ctx->order_prec.ensure((size_t)(nu + 2) * sizeof(int32_t)));
  HIP_TRY(hipMemcpyAsync(ctx->order_prec.p, hlist, (size_t)(nu + 2) * sizeof(int32_t), hipMemcpyHostToDevice,
                         ctx->stream));
  EvalArgs a{};
  a.code = grad ? (const Ins*)P->d_gcode.p : P->code_dev;
  a.prog_off = grad ? (const int32_t*)P->d_goff.p : P->off_dev;
  a.order = (const int32_t*)ctx->order_prec.p + 1;
  a.X = v.X;
  a.ld = v.ld;
  a.nvalid = v.m;
  a.ntrees = nu;
  a.nfeat = (int32_t)ds->nfeat;
  a.rb_rows = Lp.rb_rows;
  a.nrb = Lp.nrb;
  a.trees_per_group = nu;
  a.slab_prec = ctx->slab_prec.p;
  a.prec_stride = stride;
  a.max_steps = grad ? P->gmax_len : P->max_len;
  HIP_TRY(launch_eval(dtype, a, R, K_MAX, MODE_PRECISE, false, dim3(Lp.nrb, 1), 16, ctx->stream));
  // per-(tree, operator) sums over the row blocks on the device (precise_reduce_kernel: compensated
  // double-double in a fixed order, as the device-listed pass), into coherent host memory -- round 6:
  // the whole slab copied back and summed on the host in long double cost ~0.3 ms per tree at 10M rows
  // (row-shard steps)
  const size_t off = ((size_t)(nu + 1) * sizeof(int32_t) + 15) & ~(size_t)15;
  HIP_TRY(ctx->h_prec.ensure(off + (size_t)nu * stride * sizeof(double), hipHostMallocCoherent));
  HIP_TRY(launch_precise_reduce((const double*)ctx->slab_prec.p, Lp.nrb, stride, (int32_t*)ctx->order_prec.p, nu, nu,
                                nu, (int32_t*)ctx->h_prec.p, (double*)((uint8_t*)ctx->h_prec.p + off), ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(opsums, (const uint8_t*)ctx->h_prec.p + off, (size_t)nu * stride * sizeof(double));
  return SRHIP_OK;
}

int srhip::precise_decide(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const View& v,
                          const int32_t* trees, int32_t nu, bool grad, uint8_t* out_ok,
                          const std::function<int(double*, size_t)>* reduce_host) {
  if (nu <= 0) return SRHIP_OK;
  const int stride = std::max(1, grad ? P->gmax_ops : P->max_ops);
  std::vector<double> opsums((size_t)nu * stride);
  int rc = eval_precise(ctx, ds, P, v, trees, nu, opsums.data(), grad);
  if (rc) return rc;
  if (reduce_host) {
    rc = (*reduce_host)(opsums.data(), opsums.size());
    if (rc) return rc;
  }
  finalize_precise(*P, trees, nu, opsums.data(), stride, out_ok, grad);
  return SRHIP_OK;
}

int srhip::gathered_weight_sum(srhip_ctx* ctx, const srhip_dataset* ds, int64_t nidx, View& v) {
  std::vector<unsigned char> wbuf((size_t)nidx * dtype_size(ds->dtype));
  HIP_TRY(hipMemcpy(wbuf.data(), ctx->vw.p, wbuf.size(), hipMemcpyDeviceToHost));
  double s = 0.0;
  for (int64_t i = 0; i < nidx; ++i)
    s += ds->dtype == SRHIP_F64 ? ((double*)wbuf.data())[i] : (double)((float*)wbuf.data())[i];
  v.sum_w = s;
  return SRHIP_OK;
}

// (diagnostic) SRHIP_HOST_TIMING=1: run_eval's host time before the wait (argument checks, view,
// schedule, launches), in the wait, and after it (decisions), averaged over every 50 calls on stderr
int srhip::stream_wait(srhip_ctx* ctx) {
  g_wait_begin = std::chrono::steady_clock::now();
  static const bool spin = env_flag("SRHIP_SYNC_SPIN");
  if (!spin || !ctx->ev_sync) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    g_wait_done = std::chrono::steady_clock::now();
    return SRHIP_OK;
  }
  HIP_TRY(hipEventRecord(ctx->ev_sync, ctx->stream));
  for (;;) {
    const hipError_t q = hipEventQuery(ctx->ev_sync);
    if (q == hipSuccess) {
      g_wait_done = std::chrono::steady_clock::now();
      return SRHIP_OK;
    }
    if (q != hipErrorNotReady) HIP_TRY(q);
    __builtin_ia32_pause();
  }
}

// SRHIP_DECIDE_SLOW=1: every decision from the TreeInfo vectors, not the compact records (read once per
// call: the decide unit reads no environment and takes this flag)
static bool decide_fast_on() { return !env_flag("SRHIP_DECIDE_SLOW"); }

// An evaluation entry's preamble: the argument checks, the device, the view of the rows idx (all rows
// without) and a weighted gather's weight sum
static int open_view(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int mode, const srhip_loss* loss,
                     const int64_t* idx, int64_t nidx, View& v) {
  int rc = check_eval_args(ctx, ds, P, mode, loss);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  rc = make_view(ctx, ds, idx, nidx, mode == MODE_LOSS, v);
  if (rc) return rc;
  return idx && ds->weighted && mode == MODE_LOSS ? gathered_weight_sum(ctx, ds, nidx, v) : SRHIP_OK;
}

// The precise pass a host launches (eval_precise) over the undecided trees unc, as a stage of settle: their
// per-operator sums -- row shards: summed over the shards by reduce_host -- applied, none left undecided
static int settle_precise(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const View& v,
                          const double* sums, const std::function<int(double*, size_t)>* reduce_host, Verdict& V,
                          std::vector<int32_t>& unc) {
  const int stride = std::max(1, P->max_ops);
  std::vector<double> opsums(unc.size() * stride);
  int rc = eval_precise(ctx, ds, P, v, unc.data(), (int32_t)unc.size(), opsums.data());
  if (rc) return rc;
  if (reduce_host) {
    rc = (*reduce_host)(opsums.data(), opsums.size());
    if (rc) return rc;
  }
  V.apply_precise(*P, sums, unc.data(), (int32_t)unc.size(), opsums.data(), stride);
  unc.clear();
  return SRHIP_OK;
}

// Where every evaluation ends: the decision from its (possibly all-reduced) partials, then the caller's
// stages in their order while trees are undecided -- stage(V, unc) settles trees of unc through
// V.apply_precise and takes them off the list -- then the outputs (nullable).
template <typename... Stage>
static int settle(const srhip_program& P, int64_t nfeat, const double* sums, const double* chk, double* out_loss,
                  uint8_t* out_ok, Stage&&... stage) {
  Verdict V;
  std::vector<int32_t> unc = V.decide(P, nfeat, sums, chk, decide_fast_on());
  int rc = SRHIP_OK;
  ((rc = rc || unc.empty() ? rc : stage(V, unc)), ...);
  if (rc) return rc;
  for (int32_t t = 0; t < P.ntrees; ++t) {
    if (out_ok) out_ok[t] = V.ok[t];
    if (out_loss) out_loss[t] = V.loss[t];
  }
  return SRHIP_OK;
}

// Single-device evaluation: partials -> decision -> precise pass for undecided trees, as two halves --
// run_issue (arguments, view, launches) and run_complete (records, decisions, the precise passes the
// device did not settle, outputs) -- so that srhip_eval_loss_submit can return between them.
struct RunJob {
  EvalJob J;
  View v{};
  std::vector<double> sums, chk;
  DevPrecise dp;
  const srhip_dataset* ds = nullptr;
  const srhip_program* P = nullptr;
  int mode = 0;
  bool empty = false;  // no trees: nothing to decide
};
static int run_issue(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int mode, const srhip_loss* loss,
                     const int64_t* idx, int64_t nidx, void* out_pred, RunJob& R) {
  const int rc = open_view(ctx, ds, P, mode, loss, idx, nidx, R.v);
  if (rc) return rc;
  R.ds = ds;
  R.P = P;
  R.mode = mode;
  const int32_t nt = P->ntrees;
  if (nt == 0) {
    R.empty = true;
    return SRHIP_OK;
  }
  R.sums.assign(sums_len(nt, ds->nfeat), 0.0);
  R.chk.assign(nt, 0.0);
  return eval_issue(ctx, ds, P, mode, loss, R.v, out_pred, R.sums.data(), R.chk.data(), &R.dp, nullptr, R.J);
}
static int run_complete(srhip_ctx* ctx, RunJob& R, double* out_loss, uint8_t* out_ok) {
  if (R.empty) return SRHIP_OK;
  const srhip_dataset* ds = R.ds;
  const srhip_program* P = R.P;
  const View& v = R.v;
  std::vector<double>& sums = R.sums;
  DevPrecise& dp = R.dp;
  int rc = SRHIP_OK;
  if (R.J.launched) {
    rc = eval_collect(ctx, P, v, sums.data(), R.chk.data(), &dp, nullptr, R.J);
    if (rc) return rc;
  }
  // undecided trees the device's precise pass already covered (every undecided tree is listed by
  // the device: its test is the host's minus the host-only checks, so the list is a superset)
  const auto device_list = [&](Verdict& V, std::vector<int32_t>& unc) -> int {
    std::vector<int32_t> rest;
    for (int32_t t : unc) {
      const auto it = dp.used ? std::find(dp.list.begin(), dp.list.end(), t) : dp.list.end();
      if (it == dp.list.end()) rest.push_back(t);
      else V.apply_precise(*P, sums.data(), &t, 1, dp.opsums.data() + (size_t)(it - dp.list.begin()) * dp.stride, dp.stride);
    }
    unc.swap(rest);
    return SRHIP_OK;
  };
  // trees past the device list's capacity (a program's first evaluation lists at most 4): the same
  // device-listed pass over a host-written list, DEV_PRECISE_MAX trees at a time -- every undecided
  // tree of a device evaluation is then settled by one summation path (SRHIP_PRECISE_OVERFLOW_HOST=1:
  // the host-launched pass of eval_precise instead).  (A submitted evaluation reaches this after the
  // work queued behind it; its view is the whole dataset -- submits of row subsets complete at once --
  // and its results land in its own result set.)
  const auto overflow_batches = [&](Verdict& V, std::vector<int32_t>& unc) -> int {
    if (!dp.used || env_flag("SRHIP_PRECISE_OVERFLOW_HOST")) return SRHIP_OK;
    const PreciseOut out{R.J.rs->h_pout.p};
    const size_t bcap = (size_t)precise_cap(P, v, DEV_PRECISE_MAX);
    for (size_t b = 0; b < unc.size(); b += bcap) {
      const int32_t n = (int32_t)std::min<size_t>(bcap, unc.size() - b);
      std::vector<int32_t> lst(1 + n);
      lst[0] = n;
      std::copy(unc.begin() + b, unc.begin() + b + n, lst.begin() + 1);
      HIP_TRY(hipMemcpyAsync(ctx->d_ulist.p, lst.data(), lst.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                             ctx->stream));
      int stride = 1;
      int rc = enqueue_dev_precise(ctx, ds, P, v, (int32_t*)ctx->d_ulist.p, n, n, &stride, R.J.rs);
      if (rc) return rc;
      rc = stream_wait(ctx);
      if (rc) return rc;
      if (out.count() != n) return fail(SRHIP_ERR_DEVICE, "precise pass listed %d of %d trees", (int)out.count(), (int)n);
      V.apply_precise(*P, sums.data(), out.list(), n, out.sums(), stride);
    }
    unc.clear();
    return SRHIP_OK;
  };
  const auto host_pass = [&](Verdict& V, std::vector<int32_t>& unc) -> int {
    return settle_precise(ctx, ds, P, v, sums.data(), nullptr, V, unc);
  };
  if (!R.J.lx)
    return settle(*P, ds->nfeat, sums.data(), R.chk.data(), out_loss, out_ok, device_list, overflow_batches, host_pass);
  // a loss expression in one launch: srhip_eval_predict's decision, then each succeeded tree's loss from its
  // slot's sum -- the finishing kernel left them in the result set -- as srhip_eval_loss_expr divides it
  std::vector<uint8_t> ok(P->ntrees, 0);
  rc = settle(*P, ds->nfeat, sums.data(), R.chk.data(), nullptr, ok.data(), device_list, overflow_batches, host_pass);
  if (rc) return rc;
  const int32_t nl = (int32_t)R.J.lx_order.size();
  const double* hs = R.J.launched ? (const double*)R.J.rs->h_loss.p : nullptr;
  for (int32_t t = 0; t < P->ntrees; ++t) {
    if (out_loss) out_loss[t] = INFINITY;
    if (out_ok) out_ok[t] = ok[t];
  }
  if (out_loss && hs) {
    const double den = ds->weighted ? hs[nl] : (double)v.m;
    for (int32_t sl = 0; sl < nl; ++sl)
      if (ok[R.J.lx_order[sl]]) out_loss[R.J.lx_order[sl]] = hs[sl] / den;
  }
  return SRHIP_OK;
}

int srhip::run_eval(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int mode, const srhip_loss* loss,
                    const int64_t* idx, int64_t nidx, double* out_loss, void* out_pred, uint8_t* out_ok) {
  static const bool timing = env_flag("SRHIP_HOST_TIMING");
  const auto t_entry = std::chrono::steady_clock::now();
  struct Report {  // on every return path
    bool on;
    std::chrono::steady_clock::time_point t0;
    ~Report() {
      if (!on) return;
      static thread_local double acc[4];
      static thread_local int cnt;
      const auto t3 = std::chrono::steady_clock::now();
      acc[0] += std::chrono::duration<double>(g_wait_begin - t0).count();
      acc[1] += std::chrono::duration<double>(g_wait_done - g_wait_begin).count();
      acc[2] += std::chrono::duration<double>(g_tail_done - g_wait_done).count();
      acc[3] += std::chrono::duration<double>(t3 - g_tail_done).count();
      static const bool each = [] {  // SRHIP_HOST_TIMING=2: every call
        const char* e = getenv("SRHIP_HOST_TIMING");
        return e && atoi(e) >= 2;
      }();
      if (++cnt % (each ? 1 : 50) == 0) {
        fprintf(stderr, "[srhip host] run_eval: before wait %.1f us, wait %.1f us, records %.1f us, decisions %.1f us "
                "(mean of %d)\n", acc[0] / cnt * 1e6, acc[1] / cnt * 1e6, acc[2] / cnt * 1e6, acc[3] / cnt * 1e6, cnt);
        acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
        cnt = 0;
      }
    }
  } report{timing, t_entry};
  RunJob R;
  R.J.rs = &ctx->rs[0];
  int rc = run_issue(ctx, ds, P, mode, loss, idx, nidx, out_pred, R);
  if (rc) return rc;
  if (R.J.launched) {
    rc = stream_wait(ctx);
    if (rc) return rc;
  }
  return run_complete(ctx, R, out_loss, out_ok);
}

// Row-sharded evaluation (srhip_eval_loss_sharded): this shard's partials written by the reduction
// into the exchange's device buffer [loss | chk | aux], ONE all-reduce group of it in place (loss sums
// SUM, chk MAX for Float32 / SUM otherwise -- a non-finite statistic stored as +Inf -- and the aux
// entries SUM: the weight sum, the feature statistics, the row count), one copy to the host, and the
// decision every rank takes identically from the same reduced values; for undecided trees a precise pass
// over this shard with a SUM all-reduce of its per-operator sums.  The exchanges are the caller's
// (srhip_comm.cpp: RCCL on the device); nfeat is the dataset's feature count on every rank.
int srhip::run_eval_sharded(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss* loss,
                            const int64_t* idx, int64_t nidx, const ShardIO& io, double* out_loss, uint8_t* out_ok) {
  View v;
  int rc = open_view(ctx, ds, P, MODE_LOSS, loss, idx, nidx, v);
  if (rc) return rc;
  const int32_t nt = P->ntrees;
  if (nt == 0) return SRHIP_OK;
  const int64_t nf = ds->nfeat;
  const size_t ns = sums_len(nt, nf);
  ShardLayout SL;
  SL.dtype = P->dtype;
  SL.nt = (size_t)nt;
  SL.naux = 2 + 2 * (size_t)nf;  // [weight sum | feature stats (2F) | rows]
  void* dbuf = nullptr;
  rc = io.buffer(SL.bytes(), &dbuf);
  if (rc) return rc;
  ShardDev sd;
  sd.d_loss = dbuf;
  sd.d_chk = (uint8_t*)dbuf + SL.chk_off();
  sd.zero_bytes = SL.chk_off() + SL.nt * SL.chk_size();
  std::vector<double> sums(ns, 0.0), chk(nt, 0.0);
  rc = eval_partials(ctx, ds, P, MODE_LOSS, loss, v, nullptr, sums.data(), chk.data(), nullptr, &sd);
  if (rc) return rc;
  // the host-known entries (the same for every tree): weight sum, feature statistics, rows
  std::vector<double> aux(SL.naux);
  aux[0] = sums[1];
  for (size_t i = 0; i < 2 * (size_t)nf + 1; ++i) aux[1 + i] = sums[2 * (size_t)nt + i];
  const void* red = nullptr;
  rc = io.reduce(SL, aux.data(), &red);
  if (rc) return rc;
  const uint8_t* rb = (const uint8_t*)red;
  const double* raux = (const double*)(rb + SL.aux_off());
  for (int32_t t = 0; t < nt; ++t) {
    sums[2 * (size_t)t] = P->dtype == SRHIP_I32 ? (double)((const long long*)rb)[t] : ((const double*)rb)[t];
    sums[2 * (size_t)t + 1] = raux[0];
    if (P->dtype == SRHIP_F32) chk[t] = ((const float*)(rb + SL.chk_off()))[t];
    else if (P->dtype == SRHIP_F64) chk[t] = ((const double*)(rb + SL.chk_off()))[t];
  }
  for (size_t i = 0; i < 2 * (size_t)nf + 1; ++i) sums[2 * (size_t)nt + i] = raux[1 + i];
  // (this shard's persistent launch was checked to have evaluated every row block by eval_collect,
  // from its own item count -- not from the all-reduced statistic, which another shard's failures can
  // make non-finite: ADVICE r05)
  // every rank took the same decision from the same reduced partials: the undecided set agrees, and so
  // does whether the second exchange happens.  (The single-device path lists undecided trees on the
  // device; here the list depends on the all-reduced statistic, which the host already holds.)
  return settle(*P, nf, sums.data(), chk.data(), out_loss, out_ok, [&](Verdict& V, std::vector<int32_t>& unc) {
    return settle_precise(ctx, ds, P, v, sums.data(), &io.reduce_host, V, unc);
  });
}

// The launch order a fresh Float32 program's first large evaluation will use (eval_partials'
// persistent plan: one group, the live trees by descending cost, derived columns when they fit), made
// at creation -- on the thread that compiles, which in a pipeline overlaps the previous population's
// evaluation -- and uploaded with the program in its one copy, instead of sorting and copying it (a
// pageable-source copy the runtime stages synchronously) in front of the first launch.  Assumes an
// unweighted dataset of >= WIDE_MIN_ROWS rows; any other launch re-plans as before (the key differs).
static void plan_persistent_order(const srhip_ctx* ctx, srhip_program& P) {
  if (!ctx || P.ntrees == 0 || env_flag("SRHIP_NO_PREPLAN")) return;
  std::vector<int32_t> live;
  live.reserve(P.ntrees);
  for (int32_t t = 0; t < P.ntrees; ++t)
    if (!tree_static_fail(P, t)) live.push_back(t);
  if (live.empty()) return;
  const int nl = (int)live.size();
  const EvalPlan pl = plan_eval(plan_input(ctx, P, nl));
  if (pl.kind != PLAN_PERSISTENT) return;
  const std::vector<int32_t> goff{0, nl};
  std::lock_guard<std::mutex> g(P.ord_mu);
  P.ord_host = make_order(P, live, goff, pl.use_d);
  P.ord_host.insert(P.ord_host.end(), goff.begin(), goff.end());
  P.ord_recs = append_slot_records(P, P.ord_host, nl, pl.use_d);
  P.ord_key[0] = pl.L.groups;
  P.ord_key[1] = pl.L.tpg;
  P.ord_key[2] = (int)pl.use_d;
  P.ord_goff = goff;
}

// ---- deferred program teardown (srhip_program_destroy) -------------------------------------------
namespace {
struct Reaper {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<srhip_program*> q;
  bool started = false;
};
Reaper& reaper() {
  static Reaper* R = new Reaper();  // never destroyed: the thread may outlive static destruction
  return *R;
}
}  // namespace

static void reaper_push(srhip_program* P) {
  Reaper& R = reaper();
  std::lock_guard<std::mutex> g(R.mu);
  R.q.push_back(P);
  if (!R.started) {
    R.started = true;
    std::thread([&R] {
      for (;;) {
        std::vector<srhip_program*> batch;
        {
          std::unique_lock<std::mutex> lk(R.mu);
          R.cv.wait(lk, [&R] { return !R.q.empty(); });
          batch.swap(R.q);
        }
        for (srhip_program* p : batch) {
          if (p->device >= 0) (void)hipSetDevice(p->device);
          delete p;
        }
      }
    }).detach();
  }
  R.cv.notify_one();
}

template <typename T>
static void pack_column(const void* src, int64_t f, int64_t n, int64_t sf, int64_t sr, int64_t ld, T* dst) {
  const T* s = (const T*)src;
  for (int64_t j = 0; j < n; ++j) dst[j] = s[f * sf + j * sr];
  for (int64_t j = n; j < ld; ++j) dst[j] = dst[n - 1];
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

const char* srhip_last_error(void) { return srhip::last_error(); }
const char* srhip_version(void) { return "srhip 0.1.0 gfx950"; }

int srhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int srhip_ctx_create(int device, srhip_ctx** out) {
  if (!out) return fail(SRHIP_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SRHIP_ERR_DEVICE, "no HIP device available");
  if (device < 0 || device >= n) return fail(SRHIP_ERR_INVALID, "device %d out of range (%d devices)", device, n);
  std::unique_ptr<srhip_ctx> c(new srhip_ctx());
  c->device = device;
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  int lds_max = 0;
  if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds_max > 0)
    c->lds_max = lds_max;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SRHIP_ERR_UNSUPPORTED, "device %d is %s; libsrhip is built for gfx950 only", device, prop.gcnArchName);
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming));
  for (ResultSet& r : c->rs) {
    HIP_TRY(hipEventCreate(&r.ev0));
    HIP_TRY(hipEventCreate(&r.ev1));
    HIP_TRY(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  }
  HIP_TRY(hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
  *out = c.release();
  return SRHIP_OK;
}

void srhip_ctx_destroy(srhip_ctx* ctx) {
  if (!ctx) return;
  for (srhip_ctx* a : ctx->aux) srhip_ctx_destroy(a);
  ctx->aux.clear();
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev_sync) (void)hipEventDestroy(ctx->ev_sync);
  for (ResultSet& r : ctx->rs)
    for (hipEvent_t e : {r.ev0, r.ev1, r.done})
      if (e) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->up_stream) (void)hipStreamDestroy(ctx->up_stream);
  delete ctx;
  (void)hipGetLastError();
}

int srhip_ctx_synchronize(srhip_ctx* ctx) {
  if (!ctx) return fail(SRHIP_ERR_INVALID, "null ctx");
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return SRHIP_OK;
}

int srhip_dataset_create(srhip_ctx* ctx, int dtype, const void* X, int64_t nfeat, int64_t n, int64_t sf, int64_t sr,
                         const void* y, const void* w, srhip_dataset** out) {
  if (!ctx || !out) return fail(SRHIP_ERR_INVALID, "null argument");
  *out = nullptr;
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64 && dtype != SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (n <= 0) return fail(SRHIP_ERR_INVALID, "dataset needs n >= 1 rows");
  if (nfeat < 0 || nfeat > 65535) return fail(SRHIP_ERR_INVALID, "nfeatures %lld out of range", (long long)nfeat);
  if (nfeat > 0 && !X) return fail(SRHIP_ERR_INVALID, "null X");
  if (dtype == SRHIP_I32 && w) return fail(SRHIP_ERR_UNSUPPORTED, "weights on Int32 datasets");
  HIP_TRY(hipSetDevice(ctx->device));
  std::unique_ptr<srhip_dataset> d(new srhip_dataset());
  static std::atomic<uint64_t> g_ds_serial{0};
  d->serial = ++g_ds_serial;
  d->ctx = ctx;
  d->device = ctx->device;
  d->dtype = dtype;
  d->nfeat = nfeat;
  d->n = n;
  d->ld = (n + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
  d->has_y = y != nullptr;
  d->weighted = w != nullptr;
  const size_t es = dtype_size(dtype);
  const size_t colb = (size_t)d->ld * es;
  HIP_TRY(d->X.ensure(std::max<size_t>(1, (size_t)nfeat) * colb));
  HostBuf stage;
  HIP_TRY(stage.ensure(colb));
  for (int64_t f = 0; f < nfeat; ++f) {
    if (dtype == SRHIP_F64) pack_column<uint64_t>(X, f, n, sf, sr, d->ld, (uint64_t*)stage.p);
    else pack_column<uint32_t>(X, f, n, sf, sr, d->ld, (uint32_t*)stage.p);  // bit copy
    HIP_TRY(hipMemcpy((char*)d->X.p + f * colb, stage.p, colb, hipMemcpyHostToDevice));
  }
  if (y) {
    HIP_TRY(d->y.ensure(colb));
    if (dtype == SRHIP_F64) pack_column<uint64_t>(y, 0, n, 0, 1, d->ld, (uint64_t*)stage.p);
    else pack_column<uint32_t>(y, 0, n, 0, 1, d->ld, (uint32_t*)stage.p);
    HIP_TRY(hipMemcpy(d->y.p, stage.p, colb, hipMemcpyHostToDevice));
  }
  if (w) {
    HIP_TRY(d->w.ensure(colb));
    double s = 0.0;
    if (dtype == SRHIP_F64) {
      double* st = (double*)stage.p;
      for (int64_t j = 0; j < d->ld; ++j) st[j] = j < n ? ((const double*)w)[j] + 0.0 : pad_weight<double>();  // (-0.0 + 0.0 = +0.0)
      for (int64_t j = 0; j < n; ++j) s += st[j];
    } else {
      float* st = (float*)stage.p;
      for (int64_t j = 0; j < d->ld; ++j) st[j] = j < n ? ((const float*)w)[j] + 0.0f : pad_weight<float>();
      for (int64_t j = 0; j < n; ++j) s += st[j];
    }
    d->sum_w = s;
    HIP_TRY(hipMemcpy(d->w.p, stage.p, colb, hipMemcpyHostToDevice));
  }
  d->hstats.assign(std::max<int64_t>(1, nfeat), FeatStat{0.0, 0});
  if (dtype != SRHIP_I32 && nfeat > 0) {
    HIP_TRY(d->stats.ensure(feature_stats_scratch(nfeat) * sizeof(FeatStat)));
    HIP_TRY(launch_feature_stats(dtype, d->X.p, d->ld, n, (int)nfeat, (FeatStat*)d->stats.p, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d->hstats.data(), d->stats.p, (size_t)nfeat * sizeof(FeatStat), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  *out = d.release();
  return SRHIP_OK;
}

void srhip_dataset_destroy(srhip_dataset* ds) {
  if (!ds) return;
  (void)hipSetDevice(ds->device);
  delete ds;
  (void)hipGetLastError();  // no sticky error from the ignored calls above
}

int srhip_program_create(srhip_ctx* ctx, int dtype, const srhip_node* nodes, const int64_t* offsets, int32_t ntrees,
                         const srhip_operators* ops, srhip_program** out) {
  if (!out || !ops || (!offsets && ntrees > 0)) return fail(SRHIP_ERR_INVALID, "null argument");
  *out = nullptr;
  if (ntrees < 0) return fail(SRHIP_ERR_INVALID, "ntrees < 0");
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64 && dtype != SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "dtype %d", dtype);
  std::unique_ptr<srhip_program> P(new srhip_program());
  P->ctx = ctx;
  P->device = ctx ? ctx->device : -1;
  P->dtype = dtype;
  P->ntrees = ntrees;
  for (int i = 0; i < ops->nbin; ++i) {
    int sb, hb;
    if (!classify_binop(ops->binops[i], &sb, &hb)) return fail(SRHIP_ERR_UNSUPPORTED, "binary op code %d", ops->binops[i]);
    P->binops.push_back(ops->binops[i]);
  }
  for (int i = 0; i < ops->nuna; ++i) {
    if (classify_unop(ops->unaops[i]) < 0) return fail(SRHIP_ERR_UNSUPPORTED, "unary op code %d", ops->unaops[i]);
    P->unaops.push_back(ops->unaops[i]);
  }
  P->offsets.assign(offsets, offsets + ntrees + 1);
  if (ntrees > 0) {
    if (P->offsets[0] != 0) return fail(SRHIP_ERR_INVALID, "tree_offsets[0] must be 0");
    for (int32_t t = 0; t < ntrees; ++t)
      if (P->offsets[t + 1] <= P->offsets[t]) return fail(SRHIP_ERR_INVALID, "tree %d is empty", (int)t);
    P->nodes.assign(nodes, nodes + P->offsets[ntrees]);
  }
  int rc = compile_program(*P);
  if (rc) return rc;
  if (ctx) {  // ctx == NULL: host-only program (compile + did_succeed metadata, e.g. for finalize)
    plan_persistent_order(ctx, *P);
    rc = upload_program(*P, true, false, ctx->up_stream);
    if (rc) return rc;
  }
  *out = P.release();
  return SRHIP_OK;
}

void srhip_program_destroy(srhip_program* P) {
  if (!P) return;
  // a program's teardown is host work only (its device buffers go back to the allocation cache): a
  // background thread does it, so the caller -- e.g. a pipeline between two evaluations -- does not
  // wait for freeing a large population's per-tree metadata (~0.1 ms for 1024 trees)
  if (!env_flag("SRHIP_SYNC_DESTROY")) {
    reaper_push(P);
    return;
  }
  if (P->device >= 0) (void)hipSetDevice(P->device);
  delete P;
  (void)hipGetLastError();
}

int srhip_program_num_constants(const srhip_program* P, int32_t* out) {
  if (!P || !out) return fail(SRHIP_ERR_INVALID, "null argument");
  for (int32_t t = 0; t < P->ntrees; ++t) out[t] = P->info[t].nconst;
  return SRHIP_OK;
}

int srhip_program_get_constants(const srhip_program* P, double* consts) {
  if (!P || (!consts && P->ntrees > 0)) return fail(SRHIP_ERR_INVALID, "null argument");
  double* c = consts;
  for (int32_t t = 0; t < P->ntrees; ++t) get_consts(P->nodes.data() + P->offsets[t], 0, c);
  return SRHIP_OK;
}

int srhip_program_set_constants(srhip_program* P, const double* consts) {
  if (!P || (!consts && P->ntrees > 0)) return fail(SRHIP_ERR_INVALID, "null argument");
  const double* c = consts;
  for (int32_t t = 0; t < P->ntrees; ++t) set_consts(P->nodes.data() + P->offsets[t], 0, c);
  // new constants can change which trees fail statically (non-finite leaves): compile_program resets
  // the launch order, so the next evaluation plans it again
  int rc = compile_program(*P);
  if (rc) return rc;
  return P->ctx ? upload_program(*P) : SRHIP_OK;
}

int srhip_eval_loss(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const srhip_loss* loss,
                    const int64_t* idx, int64_t nidx, double* out_loss, uint8_t* out_ok) {
  if (!out_loss || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  return run_eval(ctx, ds, prog, MODE_LOSS, loss, idx, nidx, out_loss, nullptr, out_ok);
}

}  // extern "C"

int srhip::subprogram(srhip_ctx* ctx, const srhip_program* P, const std::vector<int32_t>& trees, srhip_program** Q) {
  const srhip_operators ops{(int32_t)P->binops.size(), (int32_t)P->unaops.size(), P->binops.data(), P->unaops.data()};
  std::vector<srhip_node> nodes;
  std::vector<int64_t> offs(1, 0);
  for (int32_t t : trees) {
    nodes.insert(nodes.end(), P->nodes.begin() + P->offsets[t], P->nodes.begin() + P->offsets[t + 1]);
    offs.push_back((int64_t)nodes.size());
  }
  return srhip_program_create(ctx, P->dtype, nodes.data(), offs.data(), (int32_t)trees.size(), &ops, Q);
}

int srhip::check_rowsets(const srhip_dataset* ds, int32_t nt, const int64_t* row_offsets, const int64_t* rows) {
  if (!ds->has_y) return fail(SRHIP_ERR_INVALID, "dataset has no y");
  if (row_offsets[0] != 0) return fail(SRHIP_ERR_INVALID, "row_offsets[0] must be 0");
  for (int32_t t = 0; t < nt; ++t) {
    if (row_offsets[t + 1] < row_offsets[t])
      return fail(SRHIP_ERR_INVALID, "row_offsets[%d] = %lld < row_offsets[%d] = %lld", (int)t + 1,
                  (long long)row_offsets[t + 1], (int)t, (long long)row_offsets[t]);
    if (row_offsets[t + 1] == row_offsets[t]) return fail(SRHIP_ERR_INVALID, "tree %d has an empty row set", (int)t);
    for (int64_t p = row_offsets[t]; p < row_offsets[t + 1]; ++p)
      if (rows[p] < 0 || rows[p] >= ds->n)
        return fail(SRHIP_ERR_INVALID, "tree %d: rows[%lld] (position %lld of its set) = %lld out of range [0, %lld)", (int)t,
                    (long long)p, (long long)(p - row_offsets[t]), (long long)rows[p], (long long)ds->n);
  }
  return SRHIP_OK;
}

extern "C" {

// ---- srhip_eval_loss_rowsets: one row subset per tree, one launch (srhip_rowsets.hip) ----------------
// Tree t of P alone on its set through the single-subset path (a one-tree program): the sets no wave
// can stage, and the rare trees the fast bound leaves undecided (the precise pass lives there).
static int rowset_single(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int32_t t, const srhip_loss* loss,
                         const int64_t* rows, int64_t m, double* out_loss, uint8_t* out_ok) {
  srhip_program* Q = nullptr;
  int rc = subprogram(ctx, P, {t}, &Q);
  if (rc) return rc;
  rc = run_eval(ctx, ds, Q, MODE_LOSS, loss, rows, m, out_loss, nullptr, out_ok);
  srhip_program_destroy(Q);
  return rc;
}

// The same tree under a loss expression: srhip_eval_loss_expr on the one-tree program
static int rowset_single_expr(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, int32_t t,
                              const srhip_loss_expr* e, const int64_t* rows, int64_t m, double* out_loss, uint8_t* out_ok) {
  srhip_program* Q = nullptr;
  int rc = subprogram(ctx, P, {t}, &Q);
  if (rc) return rc;
  rc = srhip_eval_loss_expr(ctx, ds, Q, e, rows, m, out_loss, out_ok);
  srhip_program_destroy(Q);
  return rc;
}

// srhip_eval_loss_rowsets (loss) and srhip_eval_loss_expr_rowsets (e) after their argument checks: exactly one
// of loss / e is set.  Under an expression the launch is rowsets_lossx_kernel (the interpreter in its prediction
// mode, then the loss program in the same wave) and the weighted mean divides by the weight sum taken in
// lossx_kernel's order; staging, statistics, records and decisions are one code path.
static int eval_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss* loss,
                        const srhip_loss_expr* e, const int64_t* row_offsets, const int64_t* rows, double* out_loss,
                        uint8_t* out_ok) {
  int rc;
  const int32_t nt = P->ntrees;
  ctx->rowsets_fallback = 0;
  if (nt == 0) return SRHIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int dtype = P->dtype;
  const int64_t nf = ds->nfeat;
  const bool weighted = ds->weighted;
  if (dtype == SRHIP_F32 && (P->sbound.size() != 4 * (size_t)nt))
    return fail(SRHIP_ERR_INVALID, "Float32 program without its +/- bounds");
  // the sets a wave can stage go into the launch, longest and costliest first; the others run alone
  const int cap = e ? rowset_lossx_cap(dtype, nf, weighted) : rowset_cap(dtype, nf, weighted), tile = 64 * rows_per_lane(dtype);
  std::vector<int32_t> live, alone;
  int64_t longest = 0;
  for (int32_t t = 0; t < nt; ++t) {
    if (tree_static_fail(*P, t)) continue;  // decided without a launch
    const int64_t m = row_offsets[t + 1] - row_offsets[t];
    if (m > cap) {
      alone.push_back(t);
    } else {
      live.push_back(t);
      longest = std::max(longest, m);
    }
  }
  std::stable_sort(live.begin(), live.end(), [&](int32_t a, int32_t b) {
    return (double)(row_offsets[a + 1] - row_offsets[a]) * P->info[a].cost > (double)(row_offsets[b + 1] - row_offsets[b]) * P->info[b].cost;
  });
  const int nl = (int)live.size();
  ResultSet* const rs = &ctx->rs[0];
  const FeatStat* fstat = nullptr;
  const double* wsum = nullptr;  // the mean's denominator of a weighted dataset
  static thread_local std::vector<uint64_t> r_fs;
  Records rec;
  if (nl > 0) {
    const int ld_lds = (int)((longest + tile - 1) / tile * tile);
    const int cpb = std::max(1, (ld_lds + loss_chunk(dtype) - 1) / loss_chunk(dtype));
    const int64_t total = row_offsets[nt];
    // [row_off | rows | order] in one copy
    std::vector<int64_t> up((size_t)nt + 1 + (size_t)total + ((size_t)nl + 1) / 2);
    memcpy(up.data(), row_offsets, ((size_t)nt + 1) * sizeof(int64_t));
    memcpy(up.data() + nt + 1, rows, (size_t)total * sizeof(int64_t));
    memcpy(up.data() + nt + 1 + total, live.data(), (size_t)nl * sizeof(int32_t));
    HIP_TRY(ctx->vidx.ensure(up.size() * sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(ctx->vidx.p, up.data(), up.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (P->upload_pending) {  // the coalescer's deferred program image: uploaded here, no cached order survives
      std::lock_guard<std::mutex> g(P->ord_mu);
      rc = push_program_image(*P, nullptr, ctx->stream);
      if (rc) return rc;
      P->ord_key[0] = P->ord_key[1] = P->ord_key[2] = -1;
      P->ord_goff.clear();
    }
    HIP_TRY(ctx->slab_loss.ensure((size_t)nl * cpb * 8));
    HIP_TRY(ctx->slab_chk.ensure((size_t)nl * 8));
    HIP_TRY(rs->h_loss.ensure((size_t)nt * 8, hipHostMallocCoherent));
    HIP_TRY(rs->h_chk.ensure((size_t)nt * 8, hipHostMallocCoherent));
    HIP_TRY(rs->h_rows.ensure((size_t)(nt + 1) * 8, hipHostMallocCoherent));
    const size_t fs_bytes = (size_t)nt * std::max<int64_t>(1, nf) * sizeof(FeatStat);
    // [feature statistics | position-order weight sums | (expression) weight sums in the loss pass's order]
    const size_t rs_bytes = fs_bytes + (size_t)nt * sizeof(double) * (e ? 2 : 1);
    HIP_TRY(ctx->h_rowsets.ensure(rs_bytes, hipHostMallocCoherent));
    if (e) HIP_TRY(ctx->lossx_work.ensure((size_t)nl * ld_lds * dtype_size(dtype)));  // the waves' predictions
    RowsetArgs a{};
    a.e.code = P->code_dev;
    a.e.prog_off = P->off_dev;
    a.e.order = (const int32_t*)((const int64_t*)ctx->vidx.p + nt + 1 + total);
    a.e.X = ds->X.p;
    a.e.y = ds->y.p;
    a.e.w = weighted ? ds->w.p : nullptr;
    a.e.slab_loss = ctx->slab_loss.p;
    a.e.slab_chk = ctx->slab_chk.p;
    a.e.ld = ld_lds;
    a.e.ntrees = nl;
    a.e.nfeat = P->maxfeat;
    a.e.rb_rows = ld_lds;
    a.e.nrb = 1;
    a.e.nch = cpb;
    a.e.cpb = cpb;
    a.e.trees_per_group = 1;
    a.e.loss_kind = loss ? loss->kind : 0;
    a.e.loss_p0 = loss ? loss->p0 : 0.0;
    a.e.weighted = weighted ? 1 : 0;
    a.e.has_y = e ? 0 : 1;
    a.e.max_steps = P->max_len;
    a.e.fused = 1;
    a.e.fused_loss = e ? nullptr : rs->h_loss.p;
    a.e.fused_chk = dtype == SRHIP_I32 ? nullptr : rs->h_chk.p;
    a.e.fused_rows = (int64_t*)rs->h_rows.p;
    a.row_off = (const int64_t*)ctx->vidx.p;
    a.rows = (const int64_t*)ctx->vidx.p + nt + 1;
    a.src_ld = ds->ld;
    a.nstage = (int32_t)nf;
    a.ld_lds = ld_lds;
    a.fstat = (FeatStat*)ctx->h_rowsets.p;
    a.wsum = weighted ? (double*)((uint8_t*)ctx->h_rowsets.p + fs_bytes) : nullptr;
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (e)
      HIP_TRY(launch_rowsets_lossx(dtype, a, e->prog, ctx->lossx_work.p, (double*)rs->h_loss.p,
                                   weighted ? (double*)((uint8_t*)ctx->h_rowsets.p + fs_bytes) + nt : nullptr, nl, ctx->stream));
    else
      HIP_TRY(launch_rowsets(dtype, a, nl, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    rc = stream_wait(ctx);  // the call's one synchronisation
    if (rc) return rc;
    // the records, out of the device-written (coherent) buffers in bulk copies
    rec.read(dtype, nt, rs->h_loss.p, rs->h_chk.p, rs->h_rows.p);
    r_fs.resize(rs_bytes / 8);
    memcpy(r_fs.data(), ctx->h_rowsets.p, r_fs.size() * 8);
    fstat = (const FeatStat*)r_fs.data();
    wsum = weighted ? (const double*)((const uint8_t*)r_fs.data() + fs_bytes) + (e ? nt : 0) : nullptr;
  }
  // every launched tree decided on its own record: its set's rows, feature statistics and +/- bound
  int64_t work[4] = {0, 0, 0, 0};
  std::vector<double> sums(sums_len(nt, nf), 0.0);
  std::vector<int32_t> undecided;
  const bool fast = decide_fast_on();
  for (int32_t t = 0; t < nt; ++t) {  // statically failing trees, and defaults
    out_loss[t] = INFINITY;
    out_ok[t] = 0;
  }
  for (int32_t t : live) {
    const int64_t m = row_offsets[t + 1] - row_offsets[t];
    const int st = decide_rowset(*P, t, nf, m, fstat + (size_t)t * nf, rec.chk_raw(t), fast, sums.data());
    if (st == 2) undecided.push_back(t);
    out_ok[t] = st == 0 ? 1 : 0;
    out_loss[t] = verdict_loss(st == 0, rec.loss_sum(t), weighted ? wsum[t] : (double)m);
    count_work(work, rec.rows_done(t), m, tree_size(*P, t));
  }
  alone.insert(alone.end(), undecided.begin(), undecided.end());
  for (int32_t t : alone) {
    const int64_t* const set = rows + row_offsets[t];
    const int64_t m = row_offsets[t + 1] - row_offsets[t];
    rc = e ? rowset_single_expr(ctx, ds, P, t, e, set, m, out_loss + t, out_ok + t)
           : rowset_single(ctx, ds, P, t, loss, set, m, out_loss + t, out_ok + t);
    if (rc) return rc;
    if (std::find(undecided.begin(), undecided.end(), t) == undecided.end())
      for (int i = 0; i < 4; ++i) work[i] += ctx->work[i];
  }
  for (int i = 0; i < 4; ++i) ctx->work[i] = work[i];
  if (nl > 0) {
    ctx->last_ev0 = ctx->ev0;
    ctx->last_ev1 = ctx->ev1;
    ctx->timed = true;
  }
  ctx->rowsets_fallback = (int64_t)alone.size();
  return SRHIP_OK;
}

int srhip_eval_loss_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss* loss,
                            const int64_t* row_offsets, const int64_t* rows, double* out_loss, uint8_t* out_ok) {
  if (!row_offsets || !rows || !out_loss || !out_ok) return fail(SRHIP_ERR_INVALID, "null argument");
  int rc = check_eval_args(ctx, ds, P, MODE_LOSS, loss);
  if (rc) return rc;
  rc = check_rowsets(ds, P->ntrees, row_offsets, rows);
  if (rc) return rc;
  return eval_rowsets(ctx, ds, P, loss, nullptr, row_offsets, rows, out_loss, out_ok);
}

int srhip_eval_loss_expr_rowsets(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss_expr* e,
                                 const int64_t* row_offsets, const int64_t* rows, double* out_loss, uint8_t* out_ok) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!row_offsets || !rows || !out_loss || !out_ok) return fail(SRHIP_ERR_INVALID, "null argument");
  int rc = check_loss_expr_args(ctx, ds, P, e);
  if (rc) return rc;
  rc = check_rowsets(ds, P->ntrees, row_offsets, rows);
  if (rc) return rc;
  return eval_rowsets(ctx, ds, P, nullptr, e, row_offsets, rows, out_loss, out_ok);
}

int64_t srhip_rowsets_fallback_trees(const srhip_ctx* ctx) { return ctx ? ctx->rowsets_fallback : -1; }

// srhip_eval_loss_submit / _wait: an evaluation whose launches return at once (queued on the context's
// stream behind whatever is in flight there) and whose records, decisions and outputs are taken at wait.
struct srhip_eval_ticket {
  srhip_ctx* ctx = nullptr;
  RunJob R;
  bool done = false;  // evaluated at submit (row subsets)
  std::vector<double> loss;
  std::vector<uint8_t> ok;
};

// the two submits: a built-in loss, or (e) a loss expression in its one-launch form
static int submit_eval(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const srhip_loss* loss,
                       const srhip_loss_expr* e, const int64_t* idx, int64_t nidx, srhip_eval_ticket** out) {
  if (!out) return fail(SRHIP_ERR_INVALID, "null ticket output");
  *out = nullptr;
  if (!ctx || !prog) return fail(SRHIP_ERR_INVALID, "null argument");
  std::unique_ptr<srhip_eval_ticket> t(new srhip_eval_ticket());
  t->ctx = ctx;
  if (idx) {
    // a row subset's gather synchronises the stream and its buffers are the context's: evaluated here
    t->loss.resize(prog->ntrees);
    t->ok.resize(prog->ntrees);
    const int rc = e ? srhip_eval_loss_expr_fused(ctx, ds, prog, e, idx, nidx, t->loss.data(), t->ok.data())
                     : run_eval(ctx, ds, prog, MODE_LOSS, loss, idx, nidx, t->loss.data(), nullptr, t->ok.data());
    if (rc) return rc;
    t->done = true;
    *out = t.release();
    return SRHIP_OK;
  }
  int k = -1;
  for (int i = 1; i < RESULT_SETS && k < 0; ++i)
    if (!ctx->rs[i].busy) k = i;
  if (k < 0) return fail(SRHIP_ERR_INVALID, "%d evaluations already in flight on this context", RESULT_SETS - 1);
  t->R.J.rs = &ctx->rs[k];
  if (e) t->R.J.lx = &e->prog;
  const int rc = run_issue(ctx, ds, prog, e ? MODE_PRED : MODE_LOSS, loss, nullptr, 0, nullptr, t->R);
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);  // launches may have been queued before the failure
    return rc;
  }
  ctx->rs[k].busy = true;
  *out = t.release();
  return SRHIP_OK;
}

int srhip_eval_loss_submit(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const srhip_loss* loss,
                           const int64_t* idx, int64_t nidx, srhip_eval_ticket** out) {
  return submit_eval(ctx, ds, prog, loss, nullptr, idx, nidx, out);
}

int srhip_eval_loss_expr_submit(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const srhip_loss_expr* e,
                                const int64_t* idx, int64_t nidx, srhip_eval_ticket** out) {
  if (out) *out = nullptr;
  const int rc = check_loss_expr_args(ctx, ds, prog, e);
  if (rc) return rc;
  return submit_eval(ctx, ds, prog, nullptr, e, idx, nidx, out);
}

int srhip_eval_loss_wait(srhip_eval_ticket* ticket, double* out_loss, uint8_t* out_ok) {
  if (!ticket) return fail(SRHIP_ERR_INVALID, "null ticket");
  std::unique_ptr<srhip_eval_ticket> t(ticket);
  if (t->done) {
    for (size_t i = 0; i < t->loss.size(); ++i) {
      if (out_loss) out_loss[i] = t->loss[i];
      if (out_ok) out_ok[i] = t->ok[i];
    }
    return SRHIP_OK;
  }
  srhip_ctx* ctx = t->ctx;
  ResultSet* rs = t->R.J.rs;
  struct Release {  // the result set is free again on every path
    ResultSet* r;
    ~Release() { r->busy = false; }
  } release{rs};
  HIP_TRY(hipSetDevice(ctx->device));
  if (t->R.J.launched) HIP_TRY(hipEventSynchronize(rs->done));
  return run_complete(ctx, t->R, out_loss, out_ok);
}

int srhip_eval_predict(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const int64_t* idx,
                       int64_t nidx, void* out_pred, uint8_t* out_ok) {
  if (!out_pred || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  return run_eval(ctx, ds, prog, MODE_PRED, nullptr, idx, nidx, nullptr, out_pred, out_ok);
}

// srhip_eval_loss with the loss given as an expression: the prediction evaluation of srhip_eval_predict
// with its output left on the device (the job's EvalJob::pred, alive until this function returns), the
// did_succeed decisions as they are, then the loss pass (srhip_lossx.hip) over the trees that succeeded.
int srhip_eval_loss_expr(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const srhip_loss_expr* e,
                         const int64_t* idx, int64_t nidx, double* out_loss, uint8_t* out_ok) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!out_loss || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  int rc = check_loss_expr_args(ctx, ds, prog, e);
  if (rc) return rc;
  const int32_t nt = prog->ntrees;
  const int64_t m = idx ? nidx : ds->n;
  // the whole population's predictions stay resident for the loss pass
  long long cap = 8LL << 30;
  if (const char* c = env_get("SRHIP_LOSSX_MAX_BYTES"))
    if (*c) cap = atoll(c);
  const long double need = (long double)nt * (long double)std::max<int64_t>(m, 0) * (long double)dtype_size(prog->dtype);
  if (need > (long double)cap)
    return fail(SRHIP_ERR_NOMEM, "loss expression: the prediction buffer needs %.0Lf bytes (%d trees x %lld rows), above the cap "
                "SRHIP_LOSSX_MAX_BYTES = %lld bytes; evaluate the population in parts", need, (int)nt, (long long)m, cap);
  RunJob R;
  R.J.rs = &ctx->rs[0];
  rc = run_issue(ctx, ds, prog, MODE_PRED, nullptr, idx, nidx, nullptr, R);
  if (rc) return rc;
  if (R.J.launched) {
    rc = stream_wait(ctx);
    if (rc) return rc;
  }
  rc = run_complete(ctx, R, nullptr, out_ok);
  if (rc) return rc;
  ctx->timed = false;  // srhip_last_kernel_ms reports the loss pass; none: < 0
  std::vector<int32_t> live;
  for (int32_t t = 0; t < nt; ++t) {
    out_loss[t] = INFINITY;
    if (out_ok[t]) live.push_back(t);
  }
  if (live.empty()) return SRHIP_OK;
  const View& v = R.v;
  const int32_t nl = (int32_t)live.size(), nslots = nl + (ds->weighted ? 1 : 0);
  const int64_t nblocks = lossx_blocks(v.m);
  // [partials | out | list]
  const size_t o_out = (size_t)nslots * nblocks * sizeof(double), o_list = o_out + (size_t)nslots * sizeof(double);
  HIP_TRY(ctx->lossx_work.ensure(o_list + (size_t)nl * sizeof(int32_t)));
  uint8_t* const wp = (uint8_t*)ctx->lossx_work.p;
  HIP_TRY(hipMemcpyAsync(wp + o_list, live.data(), (size_t)nl * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  HIP_TRY(launch_lossx(e->prog, R.J.pred.p, v.y, ds->weighted ? v.w : nullptr, v.m, (const int32_t*)(wp + o_list), nl,
                       (double*)wp, (double*)(wp + o_out), ctx->stream));
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  std::vector<double> sums(nslots);
  HIP_TRY(hipMemcpyAsync(sums.data(), wp + o_out, (size_t)nslots * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  rc = stream_wait(ctx);
  if (rc) return rc;
  ctx->last_ev0 = ctx->ev0;
  ctx->last_ev1 = ctx->ev1;
  ctx->timed = true;
  const double den = ds->weighted ? sums[nl] : (double)v.m;
  for (int32_t s = 0; s < nl; ++s) out_loss[live[s]] = sums[s] / den;
  return SRHIP_OK;
}

// srhip_eval_loss_expr in one launch (srhip_eval_lossx.hip): no prediction buffer, no residency cap, no host
// round trip between the evaluation and the loss; the same decision stages, the same summation order.
int srhip_eval_loss_expr_fused(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* prog, const srhip_loss_expr* e,
                               const int64_t* idx, int64_t nidx, double* out_loss, uint8_t* out_ok) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (!out_loss || !out_ok) return fail(SRHIP_ERR_INVALID, "null output");
  int rc = check_loss_expr_args(ctx, ds, prog, e);
  if (rc) return rc;
  RunJob R;
  R.J.rs = &ctx->rs[0];
  R.J.lx = &e->prog;
  rc = run_issue(ctx, ds, prog, MODE_PRED, nullptr, idx, nidx, nullptr, R);
  if (rc) return rc;
  if (R.J.launched) {
    rc = stream_wait(ctx);
    if (rc) return rc;
  } else {
    ctx->timed = false;  // every tree failed statically: no launch
  }
  return run_complete(ctx, R, out_loss, out_ok);
}

int srhip_eval_loss_batch(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_node* nodes, const int64_t* offsets,
                          int32_t ntrees, const srhip_operators* ops, const srhip_loss* loss, const int64_t* idx,
                          int64_t nidx, double* out_loss, uint8_t* out_ok) {
  if (!ds) return fail(SRHIP_ERR_INVALID, "null dataset");
  srhip_program* P = nullptr;
  int rc = srhip_program_create(ctx, ds->dtype, nodes, offsets, ntrees, ops, &P);
  if (rc) return rc;
  rc = srhip_eval_loss(ctx, ds, P, loss, idx, nidx, out_loss, out_ok);
  srhip_program_destroy(P);
  return rc;
}

int srhip_eval_loss_partials(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const srhip_loss* loss,
                             const int64_t* idx, int64_t nidx, double* sums, double* chk) {
  if (!sums || !chk) return fail(SRHIP_ERR_INVALID, "null output");
  View v;
  const int rc = open_view(ctx, ds, P, MODE_LOSS, loss, idx, nidx, v);
  if (rc) return rc;
  return eval_partials(ctx, ds, P, MODE_LOSS, loss, v, nullptr, sums, chk);
}

int srhip_partials_finalize(const srhip_program* P, int64_t nfeatures, const double* sums, const double* chk,
                            double* out_loss, uint8_t* out_ok, uint8_t* out_status) {
  if (!P || !sums || (!chk && P->dtype != SRHIP_I32)) return fail(SRHIP_ERR_INVALID, "null argument");
  if (nfeatures < 0) return fail(SRHIP_ERR_INVALID, "nfeatures < 0");
  for (const TreeInfo& I : P->info)
    for (int f : I.feat_checks)
      if (f >= nfeatures) return fail(SRHIP_ERR_INVALID, "tree checks feature %d of %lld", f + 1, (long long)nfeatures);
  finalize(*P, nfeatures, sums, chk, decide_fast_on(), out_loss, out_ok, out_status);
  return SRHIP_OK;
}

int srhip_eval_precise_partials(srhip_ctx* ctx, const srhip_dataset* ds, const srhip_program* P, const int64_t* idx,
                                int64_t nidx, const int32_t* trees, int32_t ntrees_sel, double* opsums) {
  if (!opsums || (!trees && ntrees_sel > 0) || ntrees_sel < 0) return fail(SRHIP_ERR_INVALID, "null argument");
  int rc = check_eval_args(ctx, ds, P, MODE_PRED, nullptr);
  if (rc) return rc;
  for (int32_t u = 0; u < ntrees_sel; ++u)
    if (trees[u] < 0 || trees[u] >= P->ntrees) return fail(SRHIP_ERR_INVALID, "tree index %d out of range", trees[u]);
  HIP_TRY(hipSetDevice(ctx->device));
  View v;
  rc = make_view(ctx, ds, idx, nidx, false, v);
  if (rc) return rc;
  return eval_precise(ctx, ds, P, v, trees, ntrees_sel, opsums);
}

int srhip_precise_finalize(const srhip_program* P, const int32_t* trees, int32_t ntrees_sel, const double* opsums,
                           uint8_t* out_ok) {
  if (!P || !opsums || !out_ok || (!trees && ntrees_sel > 0)) return fail(SRHIP_ERR_INVALID, "null argument");
  for (int32_t u = 0; u < ntrees_sel; ++u)
    if (trees[u] < 0 || trees[u] >= P->ntrees) return fail(SRHIP_ERR_INVALID, "tree index %d out of range", trees[u]);
  finalize_precise(*P, trees, ntrees_sel, opsums, std::max(1, P->max_ops), out_ok);
  return SRHIP_OK;
}

int srhip_decide_rowset(const srhip_program* P, int32_t tree, int64_t nfeatures, int64_t rows, const double* feat_stats,
                        double chk_raw, uint8_t* out_status, double* out_chk) {
  if (!P || !out_status || (!feat_stats && nfeatures > 0)) return fail(SRHIP_ERR_INVALID, "null argument");
  if (tree < 0 || tree >= P->ntrees) return fail(SRHIP_ERR_INVALID, "tree index %d out of range", tree);
  if (nfeatures < 0 || rows < 1) return fail(SRHIP_ERR_INVALID, "nfeatures < 0 or rows < 1");
  for (int f : P->info[tree].feat_checks)
    if (f >= nfeatures) return fail(SRHIP_ERR_INVALID, "tree checks feature %d of %lld", f + 1, (long long)nfeatures);
  if (P->dtype == SRHIP_F32 && P->sbound.size() != 4 * (size_t)P->ntrees)
    return fail(SRHIP_ERR_INVALID, "Float32 program without its +/- bounds");
  std::vector<FeatStat> st((size_t)nfeatures);
  for (int64_t f = 0; f < nfeatures; ++f)
    st[f] = FeatStat{feat_stats[3 * f], feat_stats[3 * f + 1] > 0.0 ? 1 : 0, feat_stats[3 * f + 2]};
  std::vector<double> sums(sums_len(P->ntrees, nfeatures), 0.0);
  *out_status = (uint8_t)decide_rowset(*P, tree, nfeatures, rows, st.data(), chk_raw, decide_fast_on(), sums.data(), out_chk);
  return SRHIP_OK;
}

int srhip_chk_reduce_op(int dtype) { return dtype == SRHIP_F32 ? 0 : 1; }

int32_t srhip_program_max_ops(const srhip_program* P) { return P ? std::max(1, P->max_ops) : 0; }

double srhip_last_kernel_ms(const srhip_ctx* ctx) {
  if (!ctx || !ctx->timed || !ctx->last_ev0 || !ctx->last_ev1) return -1.0;
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, ctx->last_ev0, ctx->last_ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

int srhip_tail_share_parts(int32_t blocks, int32_t units, int32_t nshares, int32_t share, int32_t* out) {
  if (!out || blocks < 1 || units < 1 || nshares < blocks || share < 0 || share >= nshares ||
      (int64_t)blocks * units * nshares >= ((int64_t)1 << 31))
    return -1;
  TailPart part[2];
  const int n = tail_share_parts(blocks, units, nshares, share, part);
  for (int i = 0; i < n; ++i) {
    out[3 * i] = part[i].block;
    out[3 * i + 1] = part[i].u0;
    out[3 * i + 2] = part[i].u1;
  }
  return n;
}

int srhip_last_work(const srhip_ctx* ctx, int64_t* out) {
  if (!ctx || !out) return fail(SRHIP_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = ctx->work[i];
  return SRHIP_OK;
}

int64_t srhip_hot_form_launches(const srhip_ctx* ctx) { return ctx ? ctx->hot_launches : -1; }

int srhip_program_stats(const srhip_program* P, int64_t* total_nodes, int64_t* total_opnodes, int32_t* max_stack) {
  if (!P) return fail(SRHIP_ERR_INVALID, "null program");
  if (total_nodes) *total_nodes = P->total_nodes;
  if (total_opnodes) *total_opnodes = P->total_ops;
  if (max_stack) *max_stack = P->kmax;
  return SRHIP_OK;
}

int srhip_program_derived(const srhip_program* P, int32_t* count, uint32_t* spec, int32_t cap) {
  if (!P) return fail(SRHIP_ERR_INVALID, "null program");
  if (count) *count = (int32_t)P->dspec.size();
  for (int32_t d = 0; spec && d < cap && d < (int32_t)P->dspec.size(); ++d) spec[d] = P->dspec[d];
  return SRHIP_OK;
}

}  // extern "C"
