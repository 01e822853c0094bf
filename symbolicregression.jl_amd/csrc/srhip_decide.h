// srhip_decide.h — the did_succeed decision, device-free (srhip_decide.cpp: host arithmetic, no HIP
// runtime call, no environment read): from an evaluation's records to every tree's status, ok and loss.
//
// Partials layout (the C ABI's srhip_eval_loss_partials): sums[2t] = sum of (w *) l over the rows,
// sums[2t+1] = sum of w (unweighted: the row count); sums[2T + 2f] = feature f column sum (Float64
// data: sum of x * 2^-64), sums[2T + 2f + 1] = its non-finite count; sums[2T + 2F] = rows.  Every
// entry combines across row shards by addition; chk[t] (the operator-output check statistic)
// combines by max for Float32 (max |v|) and by addition for Float64 (sum of |v| 2^-512).
#pragma once
#include "srhip_internal.h"

namespace srhip {

// overflow thresholds of an exact sum rounded to T: 2^128 - 2^103 and 2^1024 - 2^970
// (computed once: an ldexpl call per use cost ~1 us per 25 trees in the host decisions)
inline long double ovf_threshold(int dtype) {
  static const long double f64 = ldexpl(1.0L, 1024) - ldexpl(1.0L, 970), f32 = ldexpl(1.0L, 128) - ldexpl(1.0L, 103);
  return dtype == SRHIP_F64 ? f64 : f32;
}

// The partials layout's length, and the decision inputs of one view or row set written into it -- (sum,
// non-finite count) per feature (zeros without stats: Int32 data), then the row count.  The per-tree
// entries in front are left alone.
inline size_t sums_len(int32_t ntrees, int64_t nfeat) { return 2 * (size_t)ntrees + 2 * (size_t)nfeat + 1; }
inline void fill_decide_inputs(double* sums, int32_t ntrees, int64_t nfeat, const FeatStat* stats, int64_t rows) {
  double* const tail = sums + 2 * (size_t)ntrees;
  for (int64_t f = 0; f < nfeat; ++f) {
    tail[2 * f] = stats ? stats[f].sum : 0.0;
    tail[2 * f + 1] = stats ? (double)stats[f].nonfinite : 0.0;
  }
  tail[2 * nfeat] = (double)rows;
}

// A tree's evaluation-time metadata from the compact records (TreeDecide) where the program has them
inline bool tree_static_fail(const srhip_program& P, int32_t t) {
  return P.dec.size() == (size_t)P.ntrees ? P.dec[t].static_fail != 0 : P.info[t].static_fail;
}
struct TreeSize { int64_t nnodes, nops; };
inline TreeSize tree_size(const srhip_program& P, int32_t t) {
  if (P.dec.size() == (size_t)P.ntrees) return {P.dec[t].nnodes, P.dec[t].nops};
  return {P.info[t].nnodes, P.info[t].nops};
}
// srhip_last_work's four counters (evaluated node-rows, nominal node-rows, evaluated operator-node rows,
// evaluated tree-rows), one live tree added: the rows it was evaluated on, the rows asked for
inline void count_work(int64_t work[4], int64_t done, int64_t asked, const TreeSize& s) {
  work[0] += done * s.nnodes;
  work[1] += asked * s.nnodes;
  work[2] += done * s.nops;
  work[3] += done;
}

// did_succeed decision of one tree from partials in the layout above: 0 ok, 1 fail, 2 undecided (needs
// the precise pass; only the sums' feature / row-count entries are read)
int decide_tree(const TreeInfo& I, const srhip_program& P, int64_t nfeat, const double* sums, double chk);
// ... of every tree of P (fast: from the compact records where the program has them; the same answers);
// every output nullable
void finalize(const srhip_program& P, int64_t nfeat, const double* sums, const double* chk, bool fast, double* out_loss,
              uint8_t* out_ok, uint8_t* out_status);
// The precise pass's verdict: opsums[u * stride + k] = exact-ish (f64) sum over all rows of operator output k
// of tree trees[u] of the evaluation program (grad: of the gradient program); out_ok[u]
void finalize_precise(const srhip_program& P, const int32_t* trees, int32_t nsel, const double* opsums, int stride,
                      uint8_t* out_ok, bool grad = false);
// a decided tree's loss: the mean, or +Inf for a tree that did not succeed
inline double verdict_loss(bool ok, double sum, double den) { return ok ? sum / den : INFINITY; }

// The statuses, ok mask and losses of one evaluation
struct Verdict {
  std::vector<uint8_t> status, ok;
  std::vector<double> loss;
  // finalize; returns the undecided trees (status 2), ascending
  std::vector<int32_t> decide(const srhip_program& P, int64_t nfeat, const double* sums, const double* chk, bool fast);
  // the one place a precise result (finalize_precise's inputs) becomes ok[t] and loss[t] of the n trees
  void apply_precise(const srhip_program& P, const double* sums, const int32_t* trees, int32_t n, const double* opsums,
                     int stride);
};

// ---- row-sharded constant gradients (srhip_eval_loss_grad_partials -> all-reduce -> here) ------------------
// Loss, gradient, ok and status of every tree of P from combined partials: sums in the layout above, gsums[sum
// nconst] the gradient sums in get_constants order, chk[T] the gradient program's check statistic.  The decision is
// decide_tree on the gradient program's metadata (P.ginfo, which the caller has made current); loss and gradient
// are the sums over sums[2t + 1]; a failing tree (status 1) is +Inf with a zero slice; an undecided one (status 2)
// reports its sums' quotients and ok = 1 until the precise pass has settled it.
void finalize_grad(const srhip_program& P, int64_t nfeat, const double* sums, const double* gsums, const double* chk,
                   double* out_loss, double* out_grad, uint8_t* out_ok, uint8_t* out_status);

// The signature of a row-sharded gradient / optimiser call: what every rank must agree on for the ranks to build
// the same launches.  Each field is a double holding an integer below 2^53 (64-bit values travel as two halves);
// the call-start exchange all-reduces [k_i, -k_i] by MAX, and the ranks agree on field i iff max(k_i) == -max(-k_i).
enum ShardSigField {
  SIG_ENTRY = 0,  // 0: srhip_eval_loss_grad_sharded, 1: srhip_optimize_constants_sharded
  SIG_TREES, SIG_CONSTS, SIG_DTYPE, SIG_WEIGHTED, SIG_LOSS_KIND, SIG_LOSS_P0_HI, SIG_LOSS_P0_LO, SIG_LOSS_P1_HI,
  SIG_LOSS_P1_LO, SIG_ITERATIONS, SIG_RESTARTS, SIG_SEED_HI, SIG_SEED_LO, SIG_GTOL_HI, SIG_GTOL_LO, SIG_STARTS_HI,
  SIG_STARTS_LO, SIG_VALUE_TRIALS, SIG_SPEC_SLOTS, SIG_SPEC_ACTIVE, SIG_SPEC_DEPTH, SIG_GRAD_KT, SIG_COUNT
};
const char* shard_sig_name(int field);
// reduced[2 * nfields] = the MAX-reduced [k_i, -k_i] pairs: the first field the ranks disagree on, or -1
int shard_sig_check(const double* reduced, int nfields);
inline void shard_sig_put64(double* k, int hi_field, uint64_t bits) {
  k[hi_field] = (double)(uint32_t)(bits >> 32);
  k[hi_field + 1] = (double)(uint32_t)bits;
}

// the features' max |x| over a view's or row set's rows (+Inf if any entry is non-finite, or without
// statistics), rounded up to Float32: the F of the Float32 interpreter's +/- bound (EvalArgs::fbound)
float feature_bound(const FeatStat* stats, int64_t nfeat);
// The decision of tree t of P evaluated alone on a row set of its own: rows and stats ([nfeat]) of the set,
// chk_raw the interpreter's statistic (Float32: raised here to the tree's +/- bound over the set's own
// feature_bound).  sums: scratch of sums_len(P.ntrees, nfeat).  Returns the status; *chk_out (nullable):
// the statistic decided on
int decide_rowset(const srhip_program& P, int32_t t, int64_t nfeat, int64_t rows, const FeatStat* stats, double chk_raw,
                  bool fast, double* sums, double* chk_out = nullptr);

// The reduction's per-tree records, out of the device-written (coherent) host buffers in bulk copies:
// line-sized reads, not one uncached access per tree.  The copies are the thread's: one reader at a time
// (h_loss nullable: a launch without losses; Int32 data has no statistics)
class Records {
 public:
  void read(int dtype, int32_t nt, const void* h_loss, const void* h_chk, const void* h_rows);
  double loss_sum(int32_t t) const { return dtype_ == SRHIP_I32 ? (double)((const long long*)loss_)[t] : ((const double*)loss_)[t]; }
  double chk_raw(int32_t t) const {
    return dtype_ == SRHIP_F32 ? (double)((const float*)chk_)[t] : dtype_ == SRHIP_F64 ? ((const double*)chk_)[t] : 0.0;
  }
  int64_t rows_done(int32_t t) const { return ((const int64_t*)rows_)[t]; }

 private:
  int dtype_ = 0;
  const void *loss_ = nullptr, *chk_ = nullptr, *rows_ = nullptr;
};

// The device-listed precise pass's output in coherent host memory, h_pout = [count, list (DEV_PRECISE_MAX) |
// pad to 8 bytes | per-operator sums (double)]: the sums start on an 8-byte boundary (they followed the 65
// ints directly, at byte 260: misaligned double stores on the device and loads on the host -- UBSan's
// report from tools/host_stress, round 6)
constexpr int32_t DEV_PRECISE_MAX = 64;
struct PreciseOut {
  void* p;
  static constexpr size_t PREC_SUMS_OFF = ((size_t)(1 + DEV_PRECISE_MAX) * sizeof(int32_t) + 7) & ~(size_t)7;
  static size_t bytes(int ops_per_tree) { return PREC_SUMS_OFF + (size_t)DEV_PRECISE_MAX * ops_per_tree * sizeof(double); }
  int32_t* head() const { return (int32_t*)p; }  // [count, list ...], as the reduction writes it
  int32_t count() const { return head()[0]; }    // trees the device listed (may exceed the list's capacity)
  const int32_t* list() const { return head() + 1; }
  double* sums() const { return (double*)((uint8_t*)p + PREC_SUMS_OFF); }  // [listed tree][stride]
};

}  // namespace srhip
