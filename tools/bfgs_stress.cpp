// bfgs_stress.cpp — memory / concurrency stress of the constant optimiser's state machine (srhip_bfgs.cpp)
// through the C ABI, for the sanitizer builds: `make -C tools asan` / `make -C tools tsan` link it against a
// libsrhip whose host objects are built with -fsanitize=address,undefined / -fsanitize=thread, the
// sanitizer runtime linked into this executable.  No GPU is needed and none is touched.
//
// THREADS threads each run ROUNDS batches of 64 trees through srhip_bfgs_host with speculation on, over the
// closed-form objectives of tests/test_bfgs_host.py (Rosenbrock, a quartic with an indefinite start at a scale
// where the BFGS update overflows, an overflowing exp, a log wall, a slope of -Inf, the one-constant Newton
// cases, converged and non-finite starts), two starts each, under varying knobs.  Every tree's result must
// equal, bit for bit, its result when it runs alone and sequentially; a callback error must come back as the
// call's status with the outputs untouched.
//
//   bfgs_stress [THREADS] [ROUNDS]     prints "bfgs_stress ok ..." and exits 0, or exits 1 on a mismatch
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/srhip.h"

static std::atomic<int> g_fail{0};
static std::atomic<long> g_items{0}, g_launches{0};
#define EXPECT(cond)                                                                   \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, srhip_last_error()); \
      g_fail = 1;                                                                      \
    }                                                                                  \
  } while (0)

struct Objective {
  int n;
  double x0[3];
  double (*f)(const double* x, double* g);  // value; the gradient into g
};
static double rosen(const double* x, double* g) {
  const double a = x[0], b = x[1];
  g[0] = -400.0 * a * (b - a * a) - 2.0 * (1.0 - a);
  g[1] = 200.0 * (b - a * a);
  return 100.0 * (b - a * a) * (b - a * a) + (1.0 - a) * (1.0 - a);
}
static double quartic3(const double* x, double* g) {
  static const double w[3] = {-1.1, 1.2, 0.3};
  double v = 0.0;
  for (int i = 0; i < 3; ++i) {
    g[i] = 4.0 * x[i] * x[i] * x[i] + 2.0 * 1e100 * w[i] * x[i];
    v += x[i] * x[i] * x[i] * x[i] + 1e100 * w[i] * x[i] * x[i];
  }
  return v;
}
static double exp_overflow(const double* x, double* g) {
  const double e = exp(20.0 * x[0] + 20.0 * x[1]);
  g[0] = g[1] = 20.0 * e - 1000.0;
  return e - 1000.0 * (x[0] + x[1]);
}
static double log_wall(const double* x, double* g) {
  const double r = x[0] + x[1], q = (r - 1.0) * (r - 3.0);
  g[0] = g[1] = 5.0 * (r - 2.5) - (2.0 * r - 4.0) / q;
  return 2.5 * (r - 2.5) * (r - 2.5) - log(q);
}
static double slope_neginf(const double* x, double* g) {
  for (int i = 0; i < 2; ++i) g[i] = 1e200 / (1.0 + (1e200 * x[i]) * (1e200 * x[i]));
  return atan(1e200 * x[0]) + atan(1e200 * x[1]);
}
static double negcurv(const double* x, double* g) {
  g[0] = 4.0 * x[0] * x[0] * x[0] - 4.0 * x[0];
  return x[0] * x[0] * x[0] * x[0] - 2.0 * x[0] * x[0];
}
static double linear(const double* x, double* g) {
  g[0] = 3.0;
  return 3.0 * x[0] + 1.0;
}
static double probe_wall(const double* x, double* g) {
  g[0] = 1.0 - 1.0 / x[0];
  return x[0] - log(x[0]);
}
static double bowl(const double* x, double* g) {
  g[0] = 2.0 * (x[0] - 1.0);
  g[1] = 2.0 * (x[1] + 2.0);
  return (x[0] - 1.0) * (x[0] - 1.0) + (x[1] + 2.0) * (x[1] + 2.0);
}
static double log_sum(const double* x, double* g) {
  g[0] = g[1] = 1.0 / (x[0] + x[1]);
  return log(x[0] + x[1]);
}
static const Objective OBJ[] = {
    {2, {-1.2, 1.0}, rosen},        {3, {-7.3e41, -1.2e43, -4e40}, quartic3}, {2, {0.0, 0.0}, exp_overflow},
    {2, {0.0, 0.0}, log_wall},      {2, {0.0, 0.0}, slope_neginf},            {1, {0.3}, negcurv},
    {1, {0.5}, linear},             {1, {1e-6}, probe_wall},                  {2, {1.0, -2.0}, bowl},
    {2, {-1.0, -1.0}, log_sum},
};
constexpr int NOBJ = sizeof(OBJ) / sizeof(OBJ[0]), NTREES = 64, NSTARTS = 2;

struct Batch {
  std::vector<int> obj;  // tree -> objective (-1: no constants)
  int fail_at = -1, calls = 0;
};
static int eval_cb(void* user, int32_t nitems, const int32_t* tree, const int64_t* x_off, const double* x,
                   const uint8_t* value_only, double* f, double* g) {
  Batch& b = *(Batch*)user;
  if (b.calls++ == b.fail_at) return 42;
  for (int32_t i = 0; i < nitems; ++i) {
    const Objective& o = OBJ[b.obj[tree[i]]];
    double gv[3];
    const double v = o.f(x + x_off[i], gv);
    f[i] = std::isfinite(v) ? v : INFINITY;  // the contract: finite or +Inf
    if (!value_only[i]) memcpy(g + x_off[i], gv, o.n * sizeof(double));
  }
  g_items += nitems;
  return 0;
}

struct Result {
  std::vector<double> x, f;
  std::vector<int64_t> fc;
  int rc;
  int64_t nl = 0;
};
static Result run(Batch& b, int vt, int slots, int active, int depth) {
  const int nt = (int)b.obj.size();
  std::vector<int64_t> coff(nt + 1, 0);
  for (int t = 0; t < nt; ++t) coff[t + 1] = coff[t] + (b.obj[t] < 0 ? 0 : OBJ[b.obj[t]].n);
  std::vector<double> starts((size_t)NSTARTS * coff[nt]);
  for (int s = 0; s < NSTARTS; ++s)
    for (int t = 0; t < nt; ++t)
      for (int64_t k = 0; k < coff[t + 1] - coff[t]; ++k)
        starts[(size_t)s * coff[nt] + coff[t] + k] = OBJ[b.obj[t]].x0[k] * (s == 0 ? 1.0 : 1.25) + (s == 0 ? 0.0 : 0.125);
  srhip_bfgs_query q{};
  q.ntrees = nt;
  q.nstarts = NSTARTS;
  q.const_offsets = coff.data();
  q.starts = starts.data();
  q.iterations = 8;
  q.value_trials = vt;
  q.spec_slots = slots;
  q.spec_max_active = active;
  q.spec_max_depth = depth;
  Result r{std::vector<double>(coff[nt], -77.0), std::vector<double>(nt, -77.0), std::vector<int64_t>(nt, -77), 0};
  b.calls = 0;
  r.rc = srhip_bfgs_host(&q, eval_cb, &b, r.x.data(), r.f.data(), r.fc.data(), &r.nl);
  return r;
}

static void worker(int id, int rounds) {
  // every objective alone and sequential: the reference of this thread
  std::vector<Result> alone;
  for (int o = 0; o < NOBJ; ++o) {
    Batch b{{o}};
    alone.push_back(run(b, 0, 0, 0, 1));
    EXPECT(alone.back().rc == 0);
  }
  for (int r = 0; r < rounds; ++r) {
    Batch b;
    for (int t = 0; t < NTREES; ++t) b.obj.push_back((t + r + id) % (NOBJ + 1) == NOBJ ? -1 : (t * 7 + r + id) % NOBJ);
    static const int SLOTS[] = {32, 4, 4096, 1}, DEPTH[] = {64, 1, 7};
    const Result got = run(b, (r + id) % 2, SLOTS[r % 4], 64, DEPTH[r % 3]);
    EXPECT(got.rc == 0);
    g_launches += got.nl;
    int64_t at = 0;
    for (int t = 0; t < NTREES; ++t) {
      if (b.obj[t] < 0) {
        EXPECT(got.f[t] == -77.0 && got.fc[t] == -77);
        continue;
      }
      const Result& a = alone[b.obj[t]];
      const int n = OBJ[b.obj[t]].n;
      EXPECT(memcmp(&got.f[t], &a.f[0], sizeof(double)) == 0 && got.fc[t] == a.fc[0]);
      EXPECT(memcmp(&got.x[at], a.x.data(), n * sizeof(double)) == 0);
      at += n;
    }
    b.fail_at = r % 5;  // the error path: the status comes back, the outputs stay as they were
    const Result bad = run(b, 1, 32, 64, 64);
    EXPECT(bad.rc == 42 && bad.nl == 0);
    for (double v : bad.x) EXPECT(v == -77.0);
    for (double v : bad.f) EXPECT(v == -77.0);
  }
  srhip_bfgs_query q{};
  EXPECT(srhip_bfgs_host(&q, eval_cb, nullptr, nullptr, nullptr, nullptr, nullptr) == SRHIP_ERR_INVALID);
  EXPECT(srhip_bfgs_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SRHIP_ERR_INVALID);
}

int main(int argc, char** argv) {
  const int threads = argc > 1 ? atoi(argv[1]) : 4, rounds = argc > 2 ? atoi(argv[2]) : 12;
  std::vector<std::thread> th;
  for (int i = 0; i < threads; ++i) th.emplace_back(worker, i, rounds);
  for (auto& t : th) t.join();
  if (g_fail) {
    fprintf(stderr, "bfgs_stress FAILED\n");
    return 1;
  }
  printf("bfgs_stress ok: %d threads x %d rounds of %d trees, %ld launches, %ld items\n", threads, rounds, NTREES,
         g_launches.load(), g_items.load());
  return 0;
}
