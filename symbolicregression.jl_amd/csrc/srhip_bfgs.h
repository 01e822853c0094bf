// srhip_bfgs.h — the constant optimiser's state machine, device-free (srhip_bfgs.cpp: host arithmetic, no
// HIP runtime call, no environment read).  Optim's BFGS and one-constant Newton over LineSearches'
// BackTracking for a batch of trees, each tree its own machine, plus the scheduling on top of it (value-only
// trials, the speculative run-ahead of a failing line search).  A launch is three steps -- next_points,
// speculate, consume -- and bfgs_run is the loop over them for any evaluator: the device's
// (srhip_optim.cpp) or a C callback (srhip_bfgs_host, include/srhip.h: the machine on any host).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace srhip {

// LineSearches.jl BackTracking (order 3) state of one tree: a finite-value phase (halve alpha while
// phi(alpha) is not finite, at most iterfinitemax = 52 times), then the sufficient-decrease phase
// (cubic / quadratic interpolation, alpha shrunk into [0.1, 0.5] of its last value, at most
// iterations = 1000 times; a non-finite phi there simply fails the test and is interpolated on).
struct LineSearch {
  double phi0, dphi0, a1, a2, phix0, phix1;
  int iter = 0, iterfinite = 0;
  bool armijo = false;  // the finite-value phase is over
};
constexpr int LS_ITERFINITEMAX = 52, LS_ITERATIONS = 1000;
// next trial step after phi(a2) = phix1 failed the sufficient-decrease test
double backtrack_step(LineSearch& s);
// one BackTracking step on phi(a2): LS_CONTINUE (next trial at the new a2), LS_ACCEPT, or a failure
// that ends the start: LS_FAIL (iterations exhausted, LineSearchException) or LS_FAIL_NEGINF (the
// slope overflowed to -Inf: phi0 + c1 a dphi0 = -Inf for every alpha > 0 the remaining iterations can
// reach, so every further trial fails and BackTracking throws after exactly LS_ITERATIONS of them)
enum { LS_CONTINUE = 0, LS_ACCEPT = 1, LS_FAIL = 2, LS_FAIL_NEGINF = 3 };
int ls_update(LineSearch& L, double phi);

struct BfgsKnobs {
  int iterations = 8;
  double g_tol = 1e-8;
  bool value_trials = true;  // a line search's trials after its first are evaluated without a gradient
  int spec_slots = 32;       // speculative points per launch (0: none) ...
  int spec_max_active = 64;  // ... only while at most this many trees are active (the pipeline's tail) ...
  int spec_max_depth = 64;   // ... and at most this many per tree
  int trace_tree = -1;       // every evaluation of this tree, one stderr line each
  bool stats_on = false;     // count non-finite trials and the launch-size histogram
};
struct BfgsStats {
  int64_t nonfinite_trials = 0, spec_launched = 0, spec_used = 0;
  int64_t hist[5] = {0, 0, 0, 0, 0};  // launches by active trees: 1, 2-4, 5-16, 17-64, > 64
};
// a granted speculative point: tree t in slot `slot` at x + alpha s, good while line search `gen` of the
// tree asks for exactly `alpha`; its point and gradient live at `off` of BfgsBatch::sx / sg
struct BfgsSpec {
  int32_t t, slot;
  int64_t gen;
  double alpha;
  int64_t off;
};

class BfgsBatch {
 public:
  // coff: [ntrees + 1] constant offsets; best_x / best_f / fcalls are the caller's, indexed like coff, and
  // only the entries of `trees` are touched.  The batch keeps references to all but the knobs.
  BfgsBatch(int32_t ntrees, const std::vector<int32_t>& trees, const std::vector<int64_t>& coff,
            const std::vector<std::vector<double>>& starts, const BfgsKnobs& knobs, std::vector<double>& best_x,
            std::vector<double>& best_f, std::vector<int64_t>& fcalls);
  // 1. the trees still running and the one point each needs next (false: every tree is done)
  bool next_points();
  // 2. whether a line search of this launch is worth running ahead, and the run-ahead into at most `slots`
  // points: grant(slot, tree, x) -> bool takes or refuses each; a refusal drops the rest of that tree's chain
  bool speculating() const;
  template <class Grant>
  void speculate(int slots, Grant&& grant) {
    run_ahead(slots);
    size_t keep = 0;
    int32_t dead = -1;  // a tree whose chain broke: drop its rest
    for (const BfgsSpec& q : spec) {
      if (q.t == dead) continue;
      const int64_t o = coff[q.t], n = coff[q.t + 1] - o;
      for (int64_t k = 0; k < n; ++k) sx[q.off + k] = x[o + k] + q.alpha * s[o + k];
      if (grant(q.slot, q.t, (const double*)sx.data() + q.off)) spec[keep++] = q;
      else dead = q.t;
    }
    spec.resize(keep);
    sf.resize(keep);
    stats.spec_launched += (int64_t)keep;
  }
  // 3. every active tree's result, then its speculative results for as long as its line search asks for
  // exactly them; adapts the tree's speculation depth
  void consume();

  // The launch, between next_points and consume.  An evaluator reads the points ...
  const std::vector<int64_t>& coff;
  std::vector<int32_t> act;     // the active trees
  std::vector<double> xe;       // tree t's point at coff[t]
  std::vector<uint8_t> vonly;   // [ntrees] loss only
  std::vector<BfgsSpec> spec;   // the granted speculative points, grouped by tree in act's order ...
  std::vector<double> sx;       // ... point i at spec[i].off; value-only where knobs.value_trials
  // ... and writes the results, every loss finite or +Inf: fe[t] and ge[coff[t] ..] of an active tree (no
  // gradient for a value-only one), sf[i] and sg[spec[i].off ..] of speculative point i
  std::vector<double> fe, ge, sf, sg;
  const BfgsKnobs knobs;
  BfgsStats stats;
  int64_t spec_used_last = 0;  // speculative results the last consume used
  int trials_pending() const;  // active trees of the last launch now in a line search

 private:
  enum { INIT = 0, TRIAL = 1, DONE = 2, HESS_P = 3, HESS_M = 4, GRADAT = 5 };
  // the last two finite trial points (alpha, phi) of the current line search, newest first: the
  // speculation's model of phi along the search direction
  struct Hist {
    int n = 0;
    double a[2], f[2];
  };
  bool newton(int32_t t) const { return coff[t + 1] - coff[t] == 1; }
  double gnorm(int32_t t, const std::vector<double>& gg) const;
  bool candidate(int32_t t) const { return phase[t] == TRIAL && ls[t].iter + ls[t].iterfinite >= 2; }
  void begin_start(int32_t t);
  void finish_start(int32_t t);
  void begin_hess(int32_t t);
  void begin_iter(int32_t t);
  void next_iter(int32_t t);
  void accept(int32_t t, double phi, const double* gv, const double* xv);
  void consume(int32_t t, double phi, const double* gv, const double* xv);
  void run_ahead(int slots);

  const std::vector<int32_t>& trees;
  const std::vector<std::vector<double>>& starts;
  std::vector<double>&best_x, &best_f;
  std::vector<int64_t>& fcalls;
  std::vector<double> x, g, s, f, hstep, gplus, hcurv, H;
  std::vector<int64_t> hoff;
  std::vector<int> phase, start, iter;
  std::vector<LineSearch> ls;
  // consecutive non-finite trials of the current line search, and a line-search generation counter
  std::vector<int> nfstreak;
  std::vector<int64_t> lsgen;
  std::vector<Hist> hist;
  // per-tree speculation depth: doubled while every speculative point of a launch is consumed,
  // cut back to what was consumed (+1) after a misprediction
  std::vector<int> sdepth;
  // an accepted value-only trial point is re-evaluated with its gradient (phase GRADAT: same point, same
  // loss bits, not an objective call)
  std::vector<double> xacc, phiacc;
};

// One pipelined run: each launch evaluates the one point every active tree needs next, plus the granted
// speculative points.  The evaluator offers
//   place(batch)          the launch's points are known (the device: the trees' constants are set)
//   slots(&n)             the speculative slots a launch may use (the device compiles first)
//   grant(slot, tree, x)  takes or refuses slot `slot` for tree `tree` at the point x
//   evaluate(batch)       the launch's losses and gradients into the batch
//   launched(batch)       after the results are consumed (counters, the launch log)
// place, slots and evaluate return a status; a non-zero one ends the run and is returned.
template <class Evaluator>
int bfgs_run(BfgsBatch& b, Evaluator& ev) {
  while (b.next_points()) {
    int rc = ev.place(b);
    if (rc) return rc;
    if (b.speculating()) {
      int slots = 0;
      rc = ev.slots(&slots);
      if (rc) return rc;
      b.speculate(slots, [&](int32_t slot, int32_t t, const double* xs) { return ev.grant(slot, t, xs); });
    }
    rc = ev.evaluate(b);
    if (rc) return rc;
    b.consume();
    ev.launched(b);
  }
  return 0;
}

}  // namespace srhip
