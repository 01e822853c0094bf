// srhip_bfgs.cpp — the constant optimiser's state machine (srhip_bfgs.h) and srhip_bfgs_host, the same
// machine over a C callback.  Host arithmetic only: no HIP runtime call, no environment read.  Every
// floating-point expression keeps the order of Optim.jl / LineSearches.jl (oracle/optim.py restates them in
// the same order; tests/test_bfgs_host.py compares the two bit for bit).
//
// BFGS (nconst >= 2): Optim's BFGS -- inverse-Hessian approximation from the identity, direction
//   s = -H g (steepest descent if that is not a descent direction), update skipped unless
//   dx'dg > 0.
// Newton (nconst == 1, src/ConstantOptimization.jl:27-31): direction s = -g / |h| (Optim's
//   cholesky!(Positive, H) of a 1x1 Hessian flips a negative curvature and replaces a zero one by
//   1), h = (g(c + e) - g(c - e)) / 2e with e = cbrt(eps) max(1, |c|): two extra gradient launches
//   per iteration ("Hessian probes", not counted as objective calls, as Optim counts h_calls apart).
// Both: BackTracking line search from alpha = 1 (InitialStatic), stop on |g|_inf <= g_tol, on an
//   unchanged objective (f_reltol = x_abstol = 0) or after `iterations` iterations.
#include "srhip_bfgs.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "srhip_internal.h"

namespace srhip {

double backtrack_step(LineSearch& s) {
  const double rho_hi = 0.5, rho_lo = 0.1;
  double a_tmp;
  // LineSearches.jl's expressions with Julia's association (x^2 = x*x, x^3 = x*x*x as literal powers)
  if (s.iter == 1) {
    a_tmp = -(s.dphi0 * (s.a2 * s.a2)) / (2.0 * (s.phix1 - s.phi0 - s.dphi0 * s.a2));
  } else {
    const double a1sq = s.a1 * s.a1, a2sq = s.a2 * s.a2;
    const double div = 1.0 / (a1sq * a2sq * (s.a2 - s.a1));
    const double e1 = s.phix1 - s.phi0 - s.dphi0 * s.a2, e0 = s.phix0 - s.phi0 - s.dphi0 * s.a1;
    const double a = (a1sq * e1 - a2sq * e0) * div;
    const double b = (-(s.a1 * s.a1 * s.a1) * e1 + (s.a2 * s.a2 * s.a2) * e0) * div;
    if (fabs(a) <= 2.220446049250313e-16) a_tmp = s.dphi0 / (2.0 * b);
    else a_tmp = (-b + sqrt(std::max(b * b - 3.0 * a * s.dphi0, 0.0))) / (3.0 * a);
  }
  s.a1 = s.a2;
  a_tmp = std::isnan(a_tmp) ? s.a2 * rho_hi : std::min(a_tmp, s.a2 * rho_hi);  // NaNMath.min
  return std::max(a_tmp, s.a2 * rho_lo);
}

int ls_update(LineSearch& L, double phi) {
  L.phix1 = phi;
  if (!L.armijo) {
    if (!std::isfinite(phi) && L.iterfinite < LS_ITERFINITEMAX) {  // hard-coded halving until finite
      L.iterfinite += 1;
      L.a1 = L.a2;
      L.a2 = L.a1 / 2.0;
      return LS_CONTINUE;
    }
    L.armijo = true;
  }
  if (phi > L.phi0 + 1e-4 * L.a2 * L.dphi0) {  // sufficient decrease not met (or phi = Inf)
    if (L.dphi0 == -INFINITY) return LS_FAIL_NEGINF;
    if (++L.iter > LS_ITERATIONS) return LS_FAIL;
    const double a2 = backtrack_step(L);
    L.phix0 = L.phix1;
    L.a2 = a2;
    return LS_CONTINUE;
  }
  return LS_ACCEPT;
}

BfgsBatch::BfgsBatch(int32_t ntrees, const std::vector<int32_t>& trees, const std::vector<int64_t>& coff,
                     const std::vector<std::vector<double>>& starts, const BfgsKnobs& knobs, std::vector<double>& best_x,
                     std::vector<double>& best_f, std::vector<int64_t>& fcalls)
    : coff(coff), xe(best_x), vonly(ntrees, 0), fe(ntrees), ge(best_x.size()), knobs(knobs), trees(trees), starts(starts),
      best_x(best_x), best_f(best_f), fcalls(fcalls), x(best_x.size()), g(best_x.size()), s(best_x.size()),
      f(ntrees, INFINITY), hstep(ntrees, 0.0), gplus(ntrees, 0.0), hcurv(ntrees, 1.0), hoff(ntrees + 1, 0),
      phase(ntrees, DONE), start(ntrees, 0), iter(ntrees, 0), ls(ntrees), nfstreak(ntrees, 0), lsgen(ntrees, 0),
      hist(ntrees), sdepth(ntrees, 4), xacc(best_x.size()), phiacc(ntrees, 0.0) {
  for (int32_t t = 0; t < ntrees; ++t) {
    const int64_t n = coff[t + 1] - coff[t];
    hoff[t + 1] = hoff[t] + n * n;
  }
  H.assign(hoff.back(), 0.0);
  for (int32_t t : trees) begin_start(t);
}

double BfgsBatch::gnorm(int32_t t, const std::vector<double>& gg) const {
  double m = 0.0;
  for (int64_t k = coff[t]; k < coff[t + 1]; ++k) m = std::max(m, fabs(gg[k]));
  return m;
}

void BfgsBatch::begin_start(int32_t t) {
  const int64_t n = coff[t + 1] - coff[t], o = coff[t];
  for (int64_t k = o; k < o + n; ++k) x[k] = starts[start[t]][k];
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) H[hoff[t] + i * n + j] = i == j ? 1.0 : 0.0;
  phase[t] = INIT;
}

void BfgsBatch::finish_start(int32_t t) {
  // the first start is `result` unconditionally (:50); a restart replaces it only if strictly
  // better (:65-67)
  if (start[t] == 0 || f[t] < best_f[t]) {
    best_f[t] = f[t];
    for (int64_t k = coff[t]; k < coff[t + 1]; ++k) best_x[k] = x[k];
  }
  if (++start[t] < (int)starts.size()) begin_start(t);
  else phase[t] = DONE;
}

// Newton: probe the gradient at c + e and c - e for the curvature at the current point
void BfgsBatch::begin_hess(int32_t t) {
  hstep[t] = 6.055454452393343e-06 * std::max(1.0, fabs(x[coff[t]]));  // cbrt(eps(Float64))
  phase[t] = HESS_P;
}

// next iteration of t from (x, f, g): search direction and a fresh line search
void BfgsBatch::begin_iter(int32_t t) {
  if (iter[t] >= knobs.iterations) {
    finish_start(t);
    return;
  }
  const int64_t n = coff[t + 1] - coff[t], o = coff[t];
  double dphi = 0.0;
  if (newton(t)) {
    s[o] = -g[o] / hcurv[t];
    dphi = g[o] * s[o];
  } else {
    for (int64_t i = 0; i < n; ++i) {
      double acc = 0.0;
      for (int64_t j = 0; j < n; ++j) acc += H[hoff[t] + i * n + j] * g[o + j];
      s[o + i] = -acc;
      dphi += g[o + i] * s[o + i];
    }
    if (!(dphi < 0.0)) {
      dphi = 0.0;
      for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j < n; ++j) H[hoff[t] + i * n + j] = i == j ? 1.0 : 0.0;
        s[o + i] = -g[o + i];
        dphi -= g[o + i] * g[o + i];
      }
    }
  }
  LineSearch& L = ls[t];
  L = LineSearch();
  L.phi0 = f[t];
  L.dphi0 = dphi;
  L.a1 = L.a2 = 1.0;  // InitialStatic: alpha = 1
  L.phix0 = L.phix1 = f[t];
  phase[t] = TRIAL;
  nfstreak[t] = 0;
  lsgen[t] += 1;
  hist[t] = Hist();
}

void BfgsBatch::next_iter(int32_t t) {  // after an accepted step
  iter[t] += 1;
  if (newton(t) && iter[t] < knobs.iterations) begin_hess(t);
  else begin_iter(t);
}

// an accepted step to (xv, phi) with gradient gv there: BFGS update, then converge or iterate
void BfgsBatch::accept(int32_t t, double phi, const double* gv, const double* xv) {
  const int64_t o = coff[t], n = coff[t + 1] - coff[t];
  const LineSearch& L = ls[t];
  if (!newton(t)) {
    std::vector<double> dx(n), dg(n), u(n);
    double dxdg = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      dx[i] = L.a2 * s[o + i];
      dg[i] = gv[i] - g[o + i];
      dxdg += dx[i] * dg[i];
    }
    if (dxdg > 0.0) {
      double dgu = 0.0;
      for (int64_t i = 0; i < n; ++i) {
        double acc = 0.0;
        for (int64_t j = 0; j < n; ++j) acc += H[hoff[t] + i * n + j] * dg[j];
        u[i] = acc;
        dgu += dg[i] * acc;
      }
      const double c1 = (dxdg + dgu) / (dxdg * dxdg), c2 = 1.0 / dxdg;
      for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < n; ++j)
          H[hoff[t] + i * n + j] += c1 * dx[i] * dx[j] - c2 * (u[i] * dx[j] + dx[i] * u[j]);
    }
  }
  const double fold = f[t];
  for (int64_t k = 0; k < n; ++k) {
    x[o + k] = xv[k];
    g[o + k] = gv[k];
  }
  f[t] = phi;
  if (phi == fold || gnorm(t, g) <= knobs.g_tol) finish_start(t);  // converged
  else next_iter(t);
}

// one evaluation result of tree t at the point xv: loss phi, gradient gv (nullptr: value only)
void BfgsBatch::consume(int32_t t, double phi, const double* gv, const double* xv) {
  const int64_t o = coff[t], n = coff[t + 1] - coff[t];
  if (t == knobs.trace_tree) {  // every evaluation of one tree, stderr
    fprintf(stderr, "[srhip optim] tree %d start %d iter %d phase %d a %.17g f %.17g x", t, start[t], iter[t],
            phase[t], phase[t] == TRIAL ? ls[t].a2 : 0.0, phi);
    for (int64_t k = 0; k < n; ++k) fprintf(stderr, " %.17g", xv[k]);
    fprintf(stderr, " g");
    for (int64_t k = 0; k < n; ++k) fprintf(stderr, gv ? " %.17g" : " -", gv ? gv[k] : 0.0);
    fprintf(stderr, "\n");
  }
  if (phase[t] == GRADAT) {  // the gradient at an accepted value-only trial point
    accept(t, phiacc[t], gv, xacc.data() + o);
    return;
  }
  if (phase[t] == HESS_P) {
    gplus[t] = std::isfinite(phi) ? gv[0] : NAN;
    phase[t] = HESS_M;
    return;
  }
  if (phase[t] == HESS_M) {
    const double h = std::isfinite(phi) ? (gplus[t] - gv[0]) / (2.0 * hstep[t]) : NAN;
    hcurv[t] = (std::isfinite(h) && h != 0.0) ? fabs(h) : 1.0;  // cholesky!(Positive, [h])
    begin_iter(t);
    return;
  }
  fcalls[t] += 1;
  if (phase[t] == INIT) {
    f[t] = phi;
    for (int64_t k = 0; k < n; ++k) g[o + k] = gv[k];
    iter[t] = 0;
    if (!std::isfinite(f[t]) || gnorm(t, g) <= knobs.g_tol) finish_start(t);
    else if (newton(t) && knobs.iterations > 0) begin_hess(t);
    else begin_iter(t);
    return;
  }
  if (knobs.stats_on && !std::isfinite(phi)) stats.nonfinite_trials += 1;
  LineSearch& L = ls[t];
  if (std::isfinite(phi)) {
    Hist& h = hist[t];
    h.a[1] = h.a[0];
    h.f[1] = h.f[0];
    h.a[0] = L.a2;
    h.f[0] = phi;
    h.n = std::min(h.n + 1, 2);
  }
  switch (ls_update(L, phi)) {
    case LS_CONTINUE: nfstreak[t] = std::isfinite(phi) ? 0 : nfstreak[t] + 1; return;
    case LS_FAIL_NEGINF: fcalls[t] += LS_ITERATIONS - L.iter; finish_start(t); return;  // counted, not launched
    case LS_FAIL: finish_start(t); return;  // LineSearchException: the start ends at its last accepted point
    default: break;
  }
  if (!gv) {  // accepted without a gradient: fetch it at this point next launch
    for (int64_t k = 0; k < n; ++k) xacc[o + k] = xv[k];
    phiacc[t] = phi;
    phase[t] = GRADAT;
    return;
  }
  accept(t, phi, gv, xv);
}

bool BfgsBatch::next_points() {
  act.clear();
  spec.clear();
  for (int32_t t : trees) {
    if (phase[t] == DONE) continue;
    act.push_back(t);
    const int64_t o = coff[t], e = coff[t + 1];
    switch (phase[t]) {
      case INIT: for (int64_t k = o; k < e; ++k) xe[k] = x[k]; break;
      case TRIAL: for (int64_t k = o; k < e; ++k) xe[k] = x[k] + ls[t].a2 * s[k]; break;
      case HESS_P: xe[o] = x[o] + hstep[t]; break;
      case HESS_M: xe[o] = x[o] - hstep[t]; break;
      case GRADAT: for (int64_t k = o; k < e; ++k) xe[k] = xacc[k]; break;
      default: break;
    }
    // trials after a line search's first: loss only
    vonly[t] = knobs.value_trials && phase[t] == TRIAL && ls[t].iter + ls[t].iterfinite >= 1;
  }
  return !act.empty();
}

// Speculative trial points: a line search whose last trial was non-finite usually keeps failing for many
// trials (an overflowing direction halves alpha ~50 times, then shrinks it in the Armijo phase until
// x + a s rounds back to x -- hundreds of launches for one tree at the pipeline's tail).  While few trees
// are active, the launch also evaluates the next points the tree's BackTracking would try if every pending
// trial came back non-finite.  After the launch they are consumed in order for as long as the line search
// really asks for exactly that alpha (same line search, bitwise-equal alpha), so every consumed result is
// the one the sequential pipeline would have launched for: trajectories, outcomes and objective-call
// counts are unchanged.  A line search that has already failed twice is likely to keep backtracking.
bool BfgsBatch::speculating() const {
  if (knobs.spec_slots <= 0 || act.size() > (size_t)knobs.spec_max_active) return false;
  int ncand = 0;
  for (int32_t t : act) ncand += candidate(t);
  return ncand > 0;
}

void BfgsBatch::run_ahead(int slots) {
  int slot = 0;
  int64_t off = 0;
  for (int32_t t : act) {
    const int depth = std::min(std::min(sdepth[t], knobs.spec_max_depth), slots - slot);
    if (depth < 1 || !candidate(t)) continue;
    // the line search run ahead on predicted values: non-finite again after a non-finite
    // trial; otherwise phi(a) = phi0 + d (a / a_k)^q through the last two finite points (q = 2
    // from one).  Only the alphas matter, and BackTracking's steps are mostly its clamps
    // (0.5 or 0.1 of the last alpha), which a rough model reproduces bit for bit.
    const Hist& h = hist[t];
    const double phi0 = ls[t].phi0;
    double q = 2.0;
    if (h.n == 2 && h.f[0] > phi0 && h.f[1] > phi0 && h.a[0] != h.a[1] && h.a[0] > 0.0 && h.a[1] > 0.0)
      q = log((h.f[1] - phi0) / (h.f[0] - phi0)) / log(h.a[1] / h.a[0]);
    const bool model = nfstreak[t] == 0 && h.n > 0 && h.f[0] > phi0 && h.a[0] > 0.0 && std::isfinite(q);
    if (nfstreak[t] == 0 && !model) continue;
    LineSearch Ls = ls[t];
    for (int j = 0; j < depth; ++j) {
      const double phi_pred = model ? phi0 + (h.f[0] - phi0) * pow(Ls.a2 / h.a[0], q) : INFINITY;
      if (ls_update(Ls, phi_pred) != LS_CONTINUE) break;
      spec.push_back(BfgsSpec{t, slot++, lsgen[t], Ls.a2, off});
      off += coff[t + 1] - coff[t];
    }
  }
  sx.resize(off);
  sg.resize(off);
}

void BfgsBatch::consume() {
  const size_t na = act.size();
  if (knobs.stats_on) stats.hist[na <= 1 ? 0 : na <= 4 ? 1 : na <= 16 ? 2 : na <= 64 ? 3 : 4] += 1;  // launch sizes
  size_t si = 0;
  spec_used_last = 0;
  for (int32_t t : act) {
    const int64_t o = coff[t];
    consume(t, fe[t], vonly[t] ? nullptr : ge.data() + o, xe.data() + o);
    // then t's speculative points, in order, while its line search asks for exactly them
    int launched = 0, used = 0;
    bool hit = true;
    for (; si < spec.size() && spec[si].t == t; ++si) {
      const BfgsSpec& q = spec[si];
      launched += 1;
      hit = hit && phase[t] == TRIAL && lsgen[t] == q.gen && memcmp(&ls[t].a2, &q.alpha, sizeof(double)) == 0;
      if (!hit) continue;
      consume(t, sf[si], knobs.value_trials ? nullptr : sg.data() + q.off, sx.data() + q.off);
      used += 1;
    }
    spec_used_last += used;
    if (launched > 0) {
      stats.spec_used += used;
      // all used and still searching: go deeper; else keep what would have been used (+1)
      sdepth[t] = used == launched && phase[t] == TRIAL ? std::min(2 * sdepth[t], knobs.spec_max_depth)
                                                        : std::max(1, std::min(sdepth[t], used + 1));
    }
  }
}

int BfgsBatch::trials_pending() const {
  int n = 0;
  for (int32_t t : act) n += phase[t] == TRIAL;
  return n;
}

}  // namespace srhip

// ---- the machine over a C callback (include/srhip.h): no device ------------------------------------
namespace {

using namespace srhip;

// bfgs_run's evaluator: one callback call per launch, the active trees' points first, then the granted
// speculative points, packed into one x / g pair
struct CallbackEvaluator {
  srhip_bfgs_eval_fn eval;
  void* user;
  int nslots;
  int64_t nlaunches = 0;
  std::vector<int32_t> tree;
  std::vector<int64_t> xoff;
  std::vector<uint8_t> vo;
  std::vector<double> x, f, g;

  int place(const BfgsBatch&) { return 0; }
  int slots(int* n) {
    *n = nslots;
    return 0;
  }
  bool grant(int32_t slot, int32_t, const double*) const { return slot < nslots; }
  void launched(const BfgsBatch&) { nlaunches += 1; }
  int evaluate(BfgsBatch& b) {
    const std::vector<int64_t>& coff = b.coff;
    tree.clear(), xoff.clear(), vo.clear(), x.clear();
    auto add = [&](int32_t t, const double* p, bool value_only) {
      tree.push_back(t);
      xoff.push_back((int64_t)x.size());
      vo.push_back(value_only);
      x.insert(x.end(), p, p + (coff[t + 1] - coff[t]));
    };
    for (int32_t t : b.act) add(t, b.xe.data() + coff[t], b.vonly[t]);
    for (const BfgsSpec& q : b.spec) add(q.t, b.sx.data() + q.off, b.knobs.value_trials);
    f.assign(tree.size(), INFINITY);
    g.assign(x.size(), 0.0);
    const int rc = eval(user, (int32_t)tree.size(), tree.data(), xoff.data(), x.data(), vo.data(), f.data(), g.data());
    if (rc) return rc;
    const size_t nact = b.act.size();
    for (size_t i = 0; i < tree.size(); ++i) {
      const int32_t t = tree[i];
      (i < nact ? b.fe[t] : b.sf[i - nact]) = f[i];
      double* const gi = i < nact ? b.ge.data() + coff[t] : b.sg.data() + b.spec[i - nact].off;
      if (!vo[i]) std::copy(g.begin() + xoff[i], g.begin() + xoff[i] + (coff[t + 1] - coff[t]), gi);
    }
    return 0;
  }
};

}  // namespace

extern "C" int srhip_bfgs_host(const srhip_bfgs_query* q, srhip_bfgs_eval_fn eval, void* user, double* best_x,
                               double* best_f, int64_t* fcalls, int64_t* nlaunches) {
  if (!q || !eval || !best_x || !best_f || !fcalls || !q->const_offsets || !q->starts)
    return fail(SRHIP_ERR_INVALID, "null argument");
  if (q->ntrees < 0 || q->nstarts < 1 || q->iterations < 0 || q->spec_slots < 0 || q->spec_max_active < 0 ||
      q->spec_max_depth < 0 || q->const_offsets[0] != 0)
    return fail(SRHIP_ERR_INVALID, "srhip_bfgs_host: argument out of range");
  const std::vector<int64_t> coff(q->const_offsets, q->const_offsets + q->ntrees + 1);
  std::vector<int32_t> trees;  // trees with constants (nconst == 0: nothing to optimise)
  for (int32_t t = 0; t < q->ntrees; ++t) {
    if (coff[t + 1] < coff[t]) return fail(SRHIP_ERR_INVALID, "srhip_bfgs_host: constant offsets decrease at tree %d", t);
    if (coff[t + 1] > coff[t]) trees.push_back(t);
  }
  const int64_t nall = coff.back();
  std::vector<std::vector<double>> starts(q->nstarts);
  for (int32_t s = 0; s < q->nstarts; ++s) starts[s].assign(q->starts + s * nall, q->starts + (s + 1) * nall);
  BfgsKnobs knobs;
  knobs.iterations = q->iterations;
  knobs.g_tol = q->g_tol > 0 ? q->g_tol : 1e-8;
  knobs.value_trials = q->value_trials != 0;
  knobs.spec_slots = std::min(q->spec_slots, 4096);
  knobs.spec_max_active = q->spec_max_active;
  knobs.spec_max_depth = std::max(1, q->spec_max_depth);
  // the outputs are written only by a run that ends well
  std::vector<double> bx = starts[0], bf(q->ntrees, INFINITY);
  std::vector<int64_t> fc(q->ntrees, 0);
  BfgsBatch batch(q->ntrees, trees, coff, starts, knobs, bx, bf, fc);
  CallbackEvaluator ev{eval, user, knobs.spec_slots};
  const int rc = bfgs_run(batch, ev);
  if (rc) return rc;
  for (int32_t t : trees) {
    std::copy(bx.begin() + coff[t], bx.begin() + coff[t + 1], best_x + coff[t]);
    best_f[t] = bf[t];
    fcalls[t] = fc[t];
  }
  if (nlaunches) *nlaunches = ev.nlaunches;
  return SRHIP_OK;
}
