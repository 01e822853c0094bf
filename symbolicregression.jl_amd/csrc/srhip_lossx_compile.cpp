// srhip_lossx_compile.cpp — elementwise losses given as expressions, host side and device-free: the
// validation of a loss tree, its compilation into a LossxProgram (srhip_lossx.h) and the host interpreter
// behind srhip_loss_expr_eval_host.  No HIP runtime call: the unit is part of the sanitizer library builds.
//
// Operator semantics are the device's (srhip_ops.h FOps<T>): ^ is safe_pow, log is safe_log, sqrt is
// safe_sqrt, ... -- a loss expression means what the same tree means as a member of the population.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/srhip.h"
#include "srhip_internal.h"
#include "srhip_isa.h"
#include "srhip_lossx.h"
#include "srhip_ops.h"

using namespace srhip;

namespace {

template <typename T> struct Bits;
template <> struct Bits<float> {
  static uint64_t of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
  static float from(uint64_t b) { const uint32_t u = (uint32_t)b; float v; memcpy(&v, &u, 4); return v; }
};
template <> struct Bits<double> {
  static uint64_t of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
  static double from(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }
};

struct LossCompiler {
  const srhip_node* nd;
  int64_t nn;
  const srhip_operators* ops;
  int dtype;
  int32_t nargs;
  std::vector<int16_t> need_memo;
  std::vector<int32_t> size_memo;  // nodes of the expanded tree (a shared subtree once per use), capped
  LossxProgram* out;

  int opcode(int64_t i) const { return nd[i].degree == 2 ? ops->binops[nd[i].op - 1] : ops->unaops[nd[i].op - 1]; }

  // every node on its own: fields in range (children, operator, feature, constant)
  int check_nodes() const {
    for (int64_t i = 0; i < nn; ++i) {
      const srhip_node& n = nd[i];
      if (n.degree > 2) return fail(SRHIP_ERR_INVALID, "loss expression: node %lld has degree %d", (long long)i, (int)n.degree);
      if (n.degree == 0) {
        if (n.constant) {
          const bool fin = dtype == SRHIP_F32 ? m_isfinite((float)n.val) : m_isfinite(n.val);
          if (!fin)
            return fail(SRHIP_ERR_INVALID, "loss expression: node %lld is a non-finite constant (%g)", (long long)i, n.val);
        } else if (n.feature < 1 || n.feature > nargs) {
          return fail(SRHIP_ERR_INVALID, "loss expression: node %lld reads feature index %d, outside 1..nargs = 1..%d "
                      "(1 = prediction, 2 = target, 3 = weight)", (long long)i, (int)n.feature, (int)nargs);
        }
        continue;
      }
      const int32_t nop = n.degree == 2 ? ops->nbin : ops->nuna;
      if (n.op < 1 || n.op > nop)
        return fail(SRHIP_ERR_INVALID, "loss expression: node %lld has %s operator index %d, outside 1..%d", (long long)i,
                    n.degree == 2 ? "binary" : "unary", (int)n.op, (int)nop);
      int sb, hb;
      const bool known = n.degree == 2 ? classify_binop(opcode(i), &sb, &hb) : classify_unop(opcode(i)) >= 0;
      if (!known) return fail(SRHIP_ERR_UNSUPPORTED, "loss expression: node %lld has unknown operator code %d", (long long)i, opcode(i));
      if (n.l < 0 || n.l >= nn || (n.degree == 2 && (n.r < 0 || n.r >= nn)))
        return fail(SRHIP_ERR_INVALID, "loss expression: node %lld has a child index out of range", (long long)i);
    }
    return SRHIP_OK;
  }

  // the nodes reachable from the root form no cycle (children may be shared); children before parents in
  // `order`
  int topo(std::vector<int32_t>& order) const {
    std::vector<uint8_t> state(nn, 0);  // 0 unseen, 1 open, 2 done
    std::vector<std::pair<int32_t, int>> st;
    st.push_back({0, 0});
    state[0] = 1;
    while (!st.empty()) {
      auto& [i, k] = st.back();
      const srhip_node& n = nd[i];
      if (k >= n.degree) {
        state[i] = 2;
        order.push_back(i);
        st.pop_back();
        continue;
      }
      const int32_t c = k == 0 ? n.l : n.r;
      ++k;
      if (state[c] == 1) return fail(SRHIP_ERR_INVALID, "loss expression: node %d is its own descendant", (int)c);
      if (state[c] == 0) {
        state[c] = 1;
        st.push_back({c, 0});
      }
    }
    return SRHIP_OK;
  }

  void emit_ins(uint32_t op, int dst, int a, int b, uint64_t imm) {
    LossxIns& I = out->ins[out->n++];
    I = LossxIns{};
    I.op = (uint16_t)op;
    I.dst = (uint8_t)dst;
    I.a = (uint8_t)a;
    I.b = (uint8_t)b;
    I.imm = imm;
  }
  // node i's value into slot base, using slots base .. base + need(i) - 1
  void emit(int64_t i, int base) {
    const srhip_node& n = nd[i];
    if (n.degree == 0) {
      if (n.constant)
        emit_ins(LX_LOAD_CONST, base, 0, 0, dtype == SRHIP_F32 ? Bits<float>::of((float)n.val) : Bits<double>::of(n.val));
      else
        emit_ins(n.feature == 1 ? LX_LOAD_PRED : (n.feature == 2 ? LX_LOAD_Y : LX_LOAD_W), base, 0, 0, 0);
      return;
    }
    if (n.degree == 1) {
      emit(n.l, base);
      emit_ins((uint32_t)opcode(i), base, base, 0, 0);
      return;
    }
    // the child of greater need first (srhip_compile.cpp need_: equal needs cost one slot more)
    if (need_memo[n.l] >= need_memo[n.r]) {
      emit(n.l, base);
      emit(n.r, base + 1);
      emit_ins((uint32_t)opcode(i), base, base, base + 1, 0);
    } else {
      emit(n.r, base);
      emit(n.l, base + 1);
      emit_ins((uint32_t)opcode(i), base, base + 1, base, 0);
    }
  }

  int run() {
    int rc = check_nodes();
    if (rc) return rc;
    std::vector<int32_t> order;
    rc = topo(order);
    if (rc) return rc;
    need_memo.assign(nn, 0);
    size_memo.assign(nn, 0);
    constexpr int32_t SIZE_CAP = 1 << 20;
    for (int32_t i : order) {
      const srhip_node& n = nd[i];
      if (n.degree == 0) {
        need_memo[i] = 1;
        size_memo[i] = 1;
      } else if (n.degree == 1) {
        need_memo[i] = need_memo[n.l];
        size_memo[i] = std::min(SIZE_CAP, 1 + size_memo[n.l]);
      } else {
        const int a = need_memo[n.l], b = need_memo[n.r];
        need_memo[i] = (int16_t)(a == b ? a + 1 : std::max(a, b));
        size_memo[i] = std::min(SIZE_CAP, 1 + size_memo[n.l] + size_memo[n.r]);
      }
    }
    if (need_memo[0] > LOSSX_MAX_STACK)
      return fail(SRHIP_ERR_INVALID, "loss expression needs %d stack slots; the stack need is at most %d", (int)need_memo[0],
                  LOSSX_MAX_STACK);
    if (size_memo[0] > LOSSX_MAX_NODES)
      return fail(SRHIP_ERR_INVALID, "loss expression with its shared subtrees written out has %s%d nodes; an expression "
                  "has at most %d nodes", size_memo[0] >= SIZE_CAP ? "over " : "", (int)size_memo[0], LOSSX_MAX_NODES);
    out->n = 0;
    out->nargs = nargs;
    out->dtype = dtype;
    out->need = need_memo[0];
    emit(0, 0);
    return SRHIP_OK;
  }
};

// one row of the program on the host: the operator bodies of srhip_ops.h
template <typename T>
T run_row(const LossxProgram& P, T pred, T y, T w) {
  using O = FOps<T>;
  T s[LOSSX_MAX_STACK] = {};
  for (int32_t pc = 0; pc < P.n; ++pc) {
    const LossxIns& I = P.ins[pc];
    const T a = s[I.a], b = s[I.b];
    T v;
    switch (I.op) {
      case LX_LOAD_PRED: v = pred; break;
      case LX_LOAD_Y: v = y; break;
      case LX_LOAD_W: v = w; break;
      case LX_LOAD_CONST: v = Bits<T>::from(I.imm); break;
#define X_(NAME, FN) case SRHIP_OP_##NAME: v = O::FN(a, b); break;
      SRHIP_SPEC_BINOPS(X_)
      SRHIP_HEAVY_BINOPS(X_)
#undef X_
#define X_(NAME, FN) case SRHIP_OP_##NAME: v = O::FN(a); break;
      SRHIP_UNOPS(X_)
#undef X_
      default: v = FP<T>::nan(); break;
    }
    s[I.dst] = v;
  }
  return s[0];
}

template <typename T>
void run_rows(const LossxProgram& P, const void* pred, const void* y, const void* w, int64_t n, void* out) {
  const T* p = (const T*)pred;
  const T* yy = (const T*)y;
  const T* ww = (const T*)w;
  T* o = (T*)out;
  for (int64_t i = 0; i < n; ++i) o[i] = run_row<T>(P, p[i], yy[i], ww ? ww[i] : T(0));
}

}  // namespace

extern "C" {

int srhip_loss_expr_create(int dtype, const srhip_node* nodes, int64_t nnodes, const srhip_operators* ops, int32_t nargs,
                           srhip_loss_expr** out) {
  if (!out) return fail(SRHIP_ERR_INVALID, "loss expression: null output");
  *out = nullptr;
  if (!nodes || !ops) return fail(SRHIP_ERR_INVALID, "loss expression: null nodes or operators");
  if ((ops->nbin > 0 && !ops->binops) || (ops->nuna > 0 && !ops->unaops) || ops->nbin < 0 || ops->nuna < 0)
    return fail(SRHIP_ERR_INVALID, "loss expression: null operator table");
  if (dtype == SRHIP_I32) return fail(SRHIP_ERR_UNSUPPORTED, "loss expressions are Float32 / Float64 only (Int32 asked)");
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) return fail(SRHIP_ERR_INVALID, "loss expression: unknown dtype %d", dtype);
  if (nargs != 2 && nargs != 3) return fail(SRHIP_ERR_INVALID, "loss expression: nargs = %d, not 2 or 3", (int)nargs);
  if (nnodes < 1) return fail(SRHIP_ERR_INVALID, "loss expression: no nodes");
  if (nnodes > LOSSX_MAX_NODES)
    return fail(SRHIP_ERR_INVALID, "loss expression has %lld nodes; an expression has at most %d nodes", (long long)nnodes,
                LOSSX_MAX_NODES);
  std::unique_ptr<srhip_loss_expr> e(new srhip_loss_expr());
  LossCompiler C{nodes, nnodes, ops, dtype, nargs, {}, {}, &e->prog};
  const int rc = C.run();
  if (rc) return rc;
  *out = e.release();
  return SRHIP_OK;
}

void srhip_loss_expr_destroy(srhip_loss_expr* e) { delete e; }

int srhip_loss_expr_eval_host(const srhip_loss_expr* e, const void* pred, const void* y, const void* w, int64_t n,
                              void* out) {
  if (!e) return fail(SRHIP_ERR_INVALID, "null loss expression");
  if (n < 0) return fail(SRHIP_ERR_INVALID, "loss expression: n < 0");
  if (n > 0 && (!pred || !y || !out)) return fail(SRHIP_ERR_INVALID, "loss expression: null pred, y or out");
  if (n > 0 && e->prog.nargs == 3 && !w) return fail(SRHIP_ERR_INVALID, "loss expression of 3 arguments: null weights");
  if (e->prog.dtype == SRHIP_F32) run_rows<float>(e->prog, pred, y, e->prog.nargs == 3 ? w : nullptr, n, out);
  else run_rows<double>(e->prog, pred, y, e->prog.nargs == 3 ? w : nullptr, n, out);
  return SRHIP_OK;
}

int32_t srhip_lossx_block_rows(void) { return LOSSX_BLOCK_ROWS; }

int srhip_loss_expr_instructions(const srhip_loss_expr* e, uint32_t* op, int32_t* dst, int32_t* a, int32_t* b, uint64_t* imm,
                                 int32_t cap, int32_t* count, int32_t* need) {
  if (!e || !count) return fail(SRHIP_ERR_INVALID, "loss expression instructions: null expression or count");
  if (cap < 0) return fail(SRHIP_ERR_INVALID, "loss expression instructions: cap < 0");
  *count = e->prog.n;
  if (need) *need = e->prog.need;
  for (int32_t i = 0; i < std::min(cap, e->prog.n); ++i) {
    const LossxIns& I = e->prog.ins[i];
    if (op) op[i] = I.op;
    if (dst) dst[i] = I.dst;
    if (a) a[i] = I.a;
    if (b) b[i] = I.b;
    if (imm) imm[i] = I.imm;
  }
  return SRHIP_OK;
}

}  // extern "C"
