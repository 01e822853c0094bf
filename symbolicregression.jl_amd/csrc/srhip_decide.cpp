// srhip_decide.cpp — the did_succeed decision (srhip_decide.h): host arithmetic, no HIP runtime call.
#include "srhip_decide.h"

#include <algorithm>
#include <cmath>

namespace srhip {
namespace {

// One feature's column check (tail = the sums' feature entries): true = the tree fails
inline bool column_fails(int dtype, const double* tail, int f, long double ovf) {
  const double fsum = tail[2 * (size_t)f], fbad = tail[2 * (size_t)f + 1];
  if (fbad > 0) return true;
  const long double sum = dtype == SRHIP_F64 ? (long double)fsum * 0x1p64L : (long double)fsum;
  return !isfinite(fsum) || fabsl(sum) >= ovf;
}
// The operator statistic of a tree that passed its constant and column checks, over m rows -> 0 / 1 / 2
inline int op_stat_status(int dtype, double chk, long double m, long double ovf) {
  if (!isfinite(chk)) return 1;  // a NaN / Inf operator output
  long double bound;
  if (dtype == SRHIP_F64) bound = (long double)chk * 0x1p512L;  // sum |v|
  else bound = (long double)chk * m;                              // m * max |v|
  if (bound * 2.0L >= ovf) return 2;
  return 0;
}

// Returns 0 ok, 1 fail, 2 undecided (needs the precise pass).
int decide_info(const TreeInfo& I, int dtype, int32_t T, int64_t nfeat, const double* sums, double chk) {
  if (I.static_fail) return 1;
  if (dtype == SRHIP_I32) return 0;
  const double* const tail = sums + 2 * (size_t)T;
  const long double m = (long double)tail[2 * (size_t)nfeat];
  const long double ovf = ovf_threshold(dtype);
  for (double c : I.fill_consts)
    if ((long double)fabs(c) * m >= ovf) return 1;
  for (int f : I.feat_checks)
    if (column_fails(dtype, tail, f, ovf)) return 1;
  if (I.op_sumcheck.empty()) return 0;
  return op_stat_status(dtype, chk, m, ovf);
}

// decide_info on the compact record: the same answer (fill constants: |c| m >= OVF is monotone in
// |c|, so the largest decides; NaN never fails; the feature checks in any order)
inline int decide_fast(const srhip_program& P, int32_t t, int64_t nfeat, const double* sums, double chk) {
  const TreeDecide& d = P.dec[t];
  if (d.slow) return decide_info(P.info[t], P.dtype, P.ntrees, nfeat, sums, chk);
  if (d.static_fail) return 1;
  const int dtype = P.dtype;
  if (dtype == SRHIP_I32) return 0;
  const double* const tail = sums + 2 * (size_t)P.ntrees;
  const long double m = (long double)tail[2 * (size_t)nfeat];
  const long double ovf = ovf_threshold(dtype);
  if (d.maxc >= 0.0 && (long double)d.maxc * m >= ovf) return 1;
  for (uint64_t fm = d.feat_mask; fm; fm &= fm - 1)
    if (column_fails(dtype, tail, __builtin_ctzll(fm), ovf)) return 1;
  if (!d.has_op) return 0;
  return op_stat_status(dtype, chk, m, ovf);
}

inline int decide_one(const srhip_program& P, int32_t t, int64_t nfeat, const double* sums, double chk, bool fast) {
  return fast ? decide_fast(P, t, nfeat, sums, chk) : decide_info(P.info[t], P.dtype, P.ntrees, nfeat, sums, chk);
}

}  // namespace

int decide_tree(const TreeInfo& I, const srhip_program& P, int64_t nfeat, const double* sums, double chk) {
  return decide_info(I, P.dtype, P.ntrees, nfeat, sums, chk);
}

void finalize(const srhip_program& P, int64_t nfeat, const double* sums, const double* chk, bool fast, double* out_loss,
              uint8_t* out_ok, uint8_t* out_status) {
  fast = fast && P.dec.size() == (size_t)P.ntrees;
  for (int32_t t = 0; t < P.ntrees; ++t) {
    const int st = decide_one(P, t, nfeat, sums, chk ? chk[t] : 0.0, fast);
    if (out_status) out_status[t] = (uint8_t)st;
    if (out_ok) out_ok[t] = st == 0 ? 1 : 0;
    if (out_loss) out_loss[t] = verdict_loss(st == 0, sums[2 * (size_t)t], sums[2 * (size_t)t + 1]);
  }
}

void finalize_precise(const srhip_program& P, const int32_t* trees, int32_t nsel, const double* opsums, int stride,
                      uint8_t* out_ok, bool grad) {
  const long double ovf = ovf_threshold(P.dtype);
  for (int u = 0; u < nsel; ++u) {
    const TreeInfo& I = grad ? P.ginfo[trees[u]] : P.info[trees[u]];
    int st = I.static_fail ? 1 : 0;
    for (size_t k = 0; k < I.op_sumcheck.size() && !st; ++k) {
      const double s = opsums[(size_t)u * stride + k];
      if (!isfinite(s)) st = 1;
      else if (I.op_sumcheck[k]) {
        const long double S = P.dtype == SRHIP_F64 ? (long double)s * 0x1p64L : (long double)s;
        if (fabsl(S) >= ovf) st = 1;
      }
    }
    out_ok[u] = st == 0 ? 1 : 0;
  }
}

void finalize_grad(const srhip_program& P, int64_t nfeat, const double* sums, const double* gsums, const double* chk,
                   double* out_loss, double* out_grad, uint8_t* out_ok, uint8_t* out_status) {
  size_t g0 = 0;
  for (int32_t t = 0; t < P.ntrees; ++t) {
    const int nc = P.info[t].nconst;
    const int st = decide_tree(P.ginfo[t], P, nfeat, sums, chk[t]);
    const double den = sums[2 * (size_t)t + 1];
    if (out_status) out_status[t] = (uint8_t)st;
    if (out_ok) out_ok[t] = st != 1;
    if (out_loss) out_loss[t] = st == 1 ? INFINITY : sums[2 * (size_t)t] / den;
    for (int k = 0; out_grad && k < nc; ++k) out_grad[g0 + k] = st == 1 ? 0.0 : gsums[g0 + k] / den;
    g0 += (size_t)nc;
  }
}

const char* shard_sig_name(int field) {
  static const char* const names[SIG_COUNT] = {
      "entry point", "trees", "total constants", "dtype", "weighted", "loss kind", "loss parameter 0 (high bits)",
      "loss parameter 0 (low bits)", "loss parameter 1 (high bits)", "loss parameter 1 (low bits)", "iterations",
      "restarts", "seed (high bits)", "seed (low bits)", "g_tol (high bits)", "g_tol (low bits)",
      "starts_in hash (high bits)", "starts_in hash (low bits)", "SRHIP_OPTIM_VALUE_TRIALS", "SRHIP_OPTIM_SPEC",
      "SRHIP_OPTIM_SPEC_ACTIVE", "SRHIP_OPTIM_SPEC_DEPTH", "SRHIP_GRAD_KT"};
  return field >= 0 && field < SIG_COUNT ? names[field] : "?";
}

int shard_sig_check(const double* reduced, int nfields) {
  for (int i = 0; i < nfields; ++i)
    if (!(reduced[2 * i] == -reduced[2 * i + 1])) return i;  // (a NaN disagrees)
  return -1;
}

std::vector<int32_t> Verdict::decide(const srhip_program& P, int64_t nfeat, const double* sums, const double* chk,
                                     bool fast) {
  const int32_t nt = P.ntrees;
  status.resize(nt);
  ok.resize(nt);
  loss.resize(nt);
  finalize(P, nfeat, sums, chk, fast, loss.data(), ok.data(), status.data());
  std::vector<int32_t> unc;
  for (int32_t t = 0; t < nt; ++t)
    if (status[t] == 2) unc.push_back(t);
  return unc;
}

void Verdict::apply_precise(const srhip_program& P, const double* sums, const int32_t* trees, int32_t n,
                            const double* opsums, int stride) {
  for (int32_t u = 0; u < n; ++u) {
    const int32_t t = trees[u];
    finalize_precise(P, &t, 1, opsums + (size_t)u * stride, stride, &ok[t]);
    loss[t] = verdict_loss(ok[t] != 0, sums[2 * (size_t)t], sums[2 * (size_t)t + 1]);
  }
}

float feature_bound(const FeatStat* stats, int64_t nfeat) {
  double F = 0.0;
  for (int64_t f = 0; stats && f < nfeat; ++f) {
    if (stats[f].nonfinite > 0 || !(stats[f].maxabs < INFINITY)) return INFINITY;
    F = std::max(F, stats[f].maxabs);
  }
  if (!stats && nfeat > 0) return INFINITY;
  const float r = (float)F;
  return (double)r >= F ? r : std::nextafter(r, INFINITY);
}

int decide_rowset(const srhip_program& P, int32_t t, int64_t nfeat, int64_t rows, const FeatStat* stats, double chk_raw,
                  bool fast, double* sums, double* chk_out) {
  const int dtype = P.dtype;
  fill_decide_inputs(sums, P.ntrees, nfeat, dtype == SRHIP_I32 ? nullptr : stats, rows);  // (Int32 data: zeros)
  double chk = 0.0;
  if (dtype == SRHIP_F32)
    chk = skip_bound_apply((float)chk_raw, P.sbound.data() + 4 * (size_t)t, feature_bound(stats, nfeat));
  else if (dtype == SRHIP_F64)
    chk = chk_raw;
  if (chk_out) *chk_out = chk;
  return decide_one(P, t, nfeat, sums, chk, fast && P.dec.size() == (size_t)P.ntrees);
}

void Records::read(int dtype, int32_t nt, const void* h_loss, const void* h_chk, const void* h_rows) {
  dtype_ = dtype;
  static thread_local std::vector<uint64_t> r_loss, r_chk, r_rows;
  r_loss.resize(nt);
  r_chk.resize(nt);
  r_rows.resize(nt);
  if (h_loss) memcpy(r_loss.data(), h_loss, (size_t)nt * 8);
  if (dtype != SRHIP_I32) memcpy(r_chk.data(), h_chk, (size_t)nt * (dtype == SRHIP_F32 ? 4 : 8));
  memcpy(r_rows.data(), h_rows, (size_t)nt * 8);
  loss_ = r_loss.data();
  chk_ = r_chk.data();
  rows_ = r_rows.data();
}

}  // namespace srhip

using namespace srhip;

extern "C" {

// The gradient program's metadata must describe the program's current constants: a device program has it from
// srhip_eval_loss_grad_partials (the step before this one); a host-only program is compiled here (no device).
int srhip_grad_partials_finalize(srhip_program* P, int64_t nfeatures, const double* sums, const double* gsums,
                                 const double* chk, double* out_loss, double* out_grad, uint8_t* out_ok,
                                 uint8_t* out_status) {
  if (!P || !sums || !chk || !out_loss || !out_grad || !out_ok) return fail(SRHIP_ERR_INVALID, "null argument");
  if (P->dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "constant gradients need Float32 / Float64");
  if (nfeatures < 0) return fail(SRHIP_ERR_INVALID, "nfeatures < 0");
  int64_t nall = 0;
  for (int32_t t = 0; t < P->ntrees; ++t) nall += P->info[t].nconst;
  if (!gsums && nall > 0) return fail(SRHIP_ERR_INVALID, "null gradient sums");
  if (!P->ctx) {
    GradEdit edit;
    const int rc = compile_grad_host(*P, edit);
    if (rc) return rc;
  } else if (!P->grad_ready) {
    return fail(SRHIP_ERR_INVALID, "the gradient program is not compiled at the program's current constants: "
                                   "srhip_eval_loss_grad_partials comes first");
  }
  if (P->ginfo.size() < (size_t)P->ntrees) return fail(SRHIP_ERR_INVALID, "program without a gradient program");
  for (int32_t t = 0; t < P->ntrees; ++t)
    for (int f : P->ginfo[t].feat_checks)
      if (f >= nfeatures) return fail(SRHIP_ERR_INVALID, "tree checks feature %d of %lld", f + 1, (long long)nfeatures);
  finalize_grad(*P, nfeatures, sums, gsums, chk, out_loss, out_grad, out_ok, out_status);
  return SRHIP_OK;
}

int32_t srhip_shard_signature_fields(void) { return (int32_t)SIG_COUNT; }

const char* srhip_shard_signature_field_name(int32_t field) {
  return field >= 0 && field < SIG_COUNT ? shard_sig_name(field) : nullptr;
}

int32_t srhip_shard_signature_check(const double* reduced, int32_t nfields) {
  if (!reduced || nfields < 0) return -2;
  return (int32_t)shard_sig_check(reduced, nfields);
}

}  // extern "C"
