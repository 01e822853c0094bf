// lossx_stress.cpp — memory / concurrency stress of the loss-expression host unit (srhip_lossx_compile.cpp)
// through the C ABI, for the sanitizer builds: `make -C tools asan` / `make -C tools tsan` link it against a
// libsrhip whose host objects are built with -fsanitize=address,undefined / -fsanitize=thread, the
// sanitizer runtime linked into this executable.  No GPU is needed and none is touched.
//
// THREADS threads each create, evaluate (srhip_loss_expr_eval_host) and destroy ROUNDS random loss
// expressions -- chains, bushy trees, shared subtrees, both dtypes, two and three arguments -- and feed the
// rejected forms (too many nodes, too deep a stack, bad features, bad operator indices, child indices out of
// range, cycles, non-finite constants, Int32, null pointers), which must fail with their status and leave
// nothing behind.  Every accepted expression is checked against a direct evaluation of the same tree.
//
//   lossx_stress [THREADS] [ROUNDS]     prints "lossx_stress ok ..." and exits 0, or exits 1 on a mismatch
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../include/srhip.h"

static std::atomic<int> g_fail{0};
static std::atomic<long> g_ok{0}, g_rejected{0};
#define EXPECT(cond)                                                                   \
  do {                                                                                 \
    if (!(cond)) {                                                                     \
      fprintf(stderr, "FAIL %s:%d %s (%s)\n", __FILE__, __LINE__, #cond, srhip_last_error()); \
      g_fail = 1;                                                                      \
    }                                                                                  \
  } while (0)

// operators whose host values need no libm: the direct evaluation below restates them
static const int32_t BINOPS[] = {SRHIP_OP_ADD, SRHIP_OP_SUB, SRHIP_OP_MUL, SRHIP_OP_MAX};
static const int32_t UNAOPS[] = {SRHIP_OP_ABS, SRHIP_OP_SQUARE, SRHIP_OP_NEG};
static const srhip_operators OPS{4, 3, BINOPS, UNAOPS};

static srhip_node leaf_feature(int f) {
  srhip_node n{};
  n.feature = (uint16_t)f;
  n.l = n.r = -1;
  return n;
}
static srhip_node leaf_const(double v) {
  srhip_node n{};
  n.constant = 1;
  n.val = v;
  n.l = n.r = -1;
  return n;
}

// a random tree of at most `budget` nodes (root first), features 1..nargs
static int random_tree(std::mt19937_64& rng, int budget, int nargs, std::vector<srhip_node>& out) {
  const int me = (int)out.size();
  out.push_back(srhip_node{});
  const int pick = budget < 2 ? 0 : (budget < 3 ? (int)(rng() % 2) : (int)(rng() % 3));
  if (pick == 0) {
    out[me] = rng() % 4 == 0 ? leaf_const((double)(int)(rng() % 7) - 3.0) : leaf_feature(1 + (int)(rng() % nargs));
    return me;
  }
  srhip_node n{};
  n.degree = (uint8_t)pick;
  n.r = -1;
  if (pick == 1) {
    n.op = (uint16_t)(1 + rng() % 3);
    n.l = random_tree(rng, budget - 1, nargs, out);
  } else {
    n.op = (uint16_t)(1 + rng() % 4);
    const int lb = 1 + (int)(rng() % (budget - 2));
    n.l = random_tree(rng, lb, nargs, out);
    n.r = random_tree(rng, budget - 1 - lb, nargs, out);
  }
  out[me] = n;
  return me;
}

template <typename T>
static T direct(const std::vector<srhip_node>& nd, int i, const T* arg) {
  const srhip_node& n = nd[i];
  if (n.degree == 0) return n.constant ? (T)n.val : arg[n.feature - 1];
  const T a = direct<T>(nd, n.l, arg);
  if (n.degree == 1) {
    switch (UNAOPS[n.op - 1]) {
      case SRHIP_OP_ABS: return std::fabs(a);
      case SRHIP_OP_SQUARE: return a * a;
      default: return -a;
    }
  }
  const T b = direct<T>(nd, n.r, arg);
  switch (BINOPS[n.op - 1]) {
    case SRHIP_OP_ADD: return a + b;
    case SRHIP_OP_SUB: return a - b;
    case SRHIP_OP_MUL: return a * b;
    default: return (a != a || b != b) ? (T)NAN : (a > b ? a : b);
  }
}

template <typename T>
static void accepted(std::mt19937_64& rng, int dtype, const std::vector<srhip_node>& nd, int nargs) {
  srhip_loss_expr* e = nullptr;
  const int rc = srhip_loss_expr_create(dtype, nd.data(), (int64_t)nd.size(), &OPS, nargs, &e);
  if (rc == SRHIP_ERR_INVALID && !e) {  // (a bushy random tree may need more than 8 slots: a clean rejection)
    ++g_rejected;
    return;
  }
  EXPECT(rc == SRHIP_OK && e);
  if (!e) return;
  const int n = 1 + (int)(rng() % 97);
  std::vector<T> p(n), y(n), w(n), out(n, (T)-1);
  for (int i = 0; i < n; ++i) {
    p[i] = (T)((int)(rng() % 17) - 8);
    y[i] = (T)((int)(rng() % 17) - 8);
    w[i] = (T)(1 + rng() % 5);
  }
  EXPECT(srhip_loss_expr_eval_host(e, p.data(), y.data(), nargs == 3 ? w.data() : nullptr, n, out.data()) == SRHIP_OK);
  for (int i = 0; i < n; ++i) {
    const T arg[3] = {p[i], y[i], w[i]};
    const T want = direct<T>(nd, 0, arg);
    EXPECT(out[i] == want || (out[i] != out[i] && want != want));
  }
  srhip_loss_expr_destroy(e);
  ++g_ok;
}

static void rejected(int dtype, const std::vector<srhip_node>& nd, int64_t nnodes, const srhip_operators* ops, int nargs,
                     int want) {
  srhip_loss_expr* e = (srhip_loss_expr*)(uintptr_t)0x10;  // must be reset to NULL
  const int rc = srhip_loss_expr_create(dtype, nd.empty() ? nullptr : nd.data(), nnodes, ops, nargs, &e);
  EXPECT(rc == want);
  EXPECT(e == nullptr);
  EXPECT(strlen(srhip_last_error()) > 0);
  ++g_rejected;
}

static void worker(int id, int rounds) {
  std::mt19937_64 rng(1234 + 7919 * (uint64_t)id);
  for (int r = 0; r < rounds; ++r) {
    const int nargs = 2 + (int)(rng() % 2);
    std::vector<srhip_node> nd;
    random_tree(rng, 1 + (int)(rng() % 64), nargs, nd);
    if (rng() % 2) accepted<float>(rng, SRHIP_F32, nd, nargs);
    else accepted<double>(rng, SRHIP_F64, nd, nargs);
    // the rejected forms, one per round
    std::vector<srhip_node> bad;
    switch (r % 9) {
      case 0: {  // 65 nodes
        for (int i = 0; i < 64; ++i) {
          srhip_node n{};
          n.degree = 1;
          n.op = 1;
          n.l = i + 1;
          n.r = -1;
          bad.push_back(n);
        }
        bad.push_back(leaf_feature(1));
        rejected(SRHIP_F32, bad, 65, &OPS, 2, SRHIP_ERR_INVALID);
        break;
      }
      case 1: {  // nine stack slots: eight binary nodes sharing their one child
        for (int i = 0; i < 8; ++i) {
          srhip_node n{};
          n.degree = 2;
          n.op = 1;
          n.l = n.r = i + 1;
          bad.push_back(n);
        }
        bad.push_back(leaf_feature(2));
        rejected(SRHIP_F64, bad, 9, &OPS, 2, SRHIP_ERR_INVALID);
        break;
      }
      case 2:
        bad = {leaf_feature(nargs + 1)};
        rejected(SRHIP_F32, bad, 1, &OPS, nargs, SRHIP_ERR_INVALID);
        bad = {leaf_feature(0)};
        rejected(SRHIP_F32, bad, 1, &OPS, nargs, SRHIP_ERR_INVALID);
        break;
      case 3: {
        srhip_node n{};
        n.degree = 2;
        n.op = 5;  // four binary operators
        n.l = 1;
        n.r = 2;
        bad = {n, leaf_feature(1), leaf_feature(2)};
        rejected(SRHIP_F32, bad, 3, &OPS, 2, SRHIP_ERR_INVALID);
        break;
      }
      case 4: {
        srhip_node n{};
        n.degree = 2;
        n.op = 1;
        n.l = 1;
        n.r = 7;  // out of range
        bad = {n, leaf_feature(1), leaf_feature(2)};
        rejected(SRHIP_F64, bad, 3, &OPS, 2, SRHIP_ERR_INVALID);
        break;
      }
      case 5: {  // a cycle
        srhip_node a{}, b{};
        a.degree = b.degree = 1;
        a.op = b.op = 1;
        a.l = 1;
        b.l = 0;
        a.r = b.r = -1;
        bad = {a, b};
        rejected(SRHIP_F32, bad, 2, &OPS, 2, SRHIP_ERR_INVALID);
        break;
      }
      case 6:
        bad = {leaf_const(NAN)};
        rejected(SRHIP_F64, bad, 1, &OPS, 2, SRHIP_ERR_INVALID);
        bad = {leaf_const(1e300)};  // Inf in Float32
        rejected(SRHIP_F32, bad, 1, &OPS, 2, SRHIP_ERR_INVALID);
        break;
      case 7:
        bad = {leaf_feature(1)};
        rejected(SRHIP_I32, bad, 1, &OPS, 2, SRHIP_ERR_UNSUPPORTED);
        break;
      default:
        rejected(SRHIP_F32, bad, 1, &OPS, 2, SRHIP_ERR_INVALID);  // null nodes
        bad = {leaf_feature(1)};
        rejected(SRHIP_F32, bad, 1, nullptr, 2, SRHIP_ERR_INVALID);
        EXPECT(srhip_loss_expr_create(SRHIP_F32, bad.data(), 1, &OPS, 2, nullptr) == SRHIP_ERR_INVALID);
        EXPECT(srhip_loss_expr_eval_host(nullptr, nullptr, nullptr, nullptr, 1, nullptr) == SRHIP_ERR_INVALID);
        srhip_loss_expr_destroy(nullptr);
        break;
    }
  }
}

int main(int argc, char** argv) {
  const int threads = argc > 1 ? atoi(argv[1]) : 8, rounds = argc > 2 ? atoi(argv[2]) : 100;
  std::vector<std::thread> th;
  for (int i = 0; i < threads; ++i) th.emplace_back(worker, i, rounds);
  for (auto& t : th) t.join();
  if (g_fail) {
    fprintf(stderr, "lossx_stress FAILED\n");
    return 1;
  }
  printf("lossx_stress ok: %d threads x %d rounds, %ld expressions evaluated, %ld rejected\n", threads, rounds,
         g_ok.load(), g_rejected.load());
  return 0;
}
