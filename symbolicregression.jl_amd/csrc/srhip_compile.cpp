// srhip_compile.cpp — the tree compiler of libsrhip.so (srhip_compile.h): Node{T} -> bytecode for the
// evaluation program, its derived-column program and the constant-gradient program, the per-tree code
// cache, and the ABI entries that only read the compiler's output.  Host arithmetic on srhip_program's
// vectors: nothing here calls the HIP runtime (uploads: srhip_host.cpp upload_program, srhip_optim.cpp).
//
// The compiler restates, per tree, the host-decidable half of DynamicExpressions v0.16's
// eval_tree_array (external dependency; behaviour pinned by the reference's
// test/test_evaluation.jl, test/test_nan_detection.jl):
//   * constant subtrees are evaluated once as scalars (_eval_constant_tree): any non-finite
//     operator output => did_succeed = false; the folded value c is then a fill(c, n) array whose
//     isfinite(sum) is checked by its parent (or by the final root check);
//   * a non-finite constant leaf under a non-constant parent fails (@return_on_check);
//   * a feature leaf evaluated as a child array (child of a non-fused unary node, or the root)
//     gets its column's isfinite(sum) checked;
//   * every remaining operator node is emitted as bytecode; the device checks its outputs.
#include "srhip_compile.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <sys/resource.h>
#include <sys/syscall.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/srhip.h"
#include "srhip_internal.h"
#include "srhip_isa.h"
#include "srhip_ops.h"

using namespace srhip;

#ifndef SRHIP_COS_NC
// cos / sin of an operator output without their check fold (srhip_isa.h UN_NC_FLAG; 0: the checked form;
// C2 same box: 1.263 against 1.267 ms, profiles/r05_c2_scratch_g23/)
#define SRHIP_COS_NC 1
#endif

// ---------------------------------------------------------------------------------------------
// tree compiler
// ---------------------------------------------------------------------------------------------
namespace {

template <typename T> struct HostVal {
  static T from(double v) { return (T)v; }
  static uint64_t bits(T v) {
    if constexpr (sizeof(T) == 8) {
      uint64_t b;
      memcpy(&b, &v, 8);
      return b;
    } else {
      uint32_t b;
      memcpy(&b, &v, 4);
      return b;
    }
  }
};

// A derived column's key (srhip_isa.h; srhip_program::dspec, gdspec): the unary operator's class over
// the 0-based feature column it is applied to.
inline uint32_t derived_key(int unary_class, int32_t feature_1based) {
  return ((uint32_t)unary_class << 16) | (uint32_t)(feature_1based - 1);
}
// the derived column that key names in spec, or -1 (a spec holds distinct keys)
inline int32_t find_derived(const std::vector<uint32_t>& spec, uint32_t key) {
  for (size_t d = 0; d < spec.size(); ++d)
    if (spec[d] == key) return (int32_t)d;
  return -1;
}

static double op_cost(uint32_t h) {
  if (h == H_END) return 0.0;
  if (h < H_BIN0) return 1.0;
  if (h < H_HEAVY0) {
    const int sb = (h - H_BIN0) / SPEC_STRIDE;
    return sb == SB_DIV ? 10.0 : 2.0;
  }
  if (h < H_UN0) return 120.0;
  const int u = h - H_UN0;
  switch (u) {
    case UN_NEG: case UN_SQUARE: case UN_CUBE: case UN_ABS: case UN_RELU: case UN_SIGN:
    case UN_ROUND: case UN_FLOOR: case UN_CEIL:
      return 2.0;
    case UN_EXP: case UN_EXP2: case UN_SQRT: case UN_LOG: case UN_LOG2: case UN_LOG10:
      return 14.0;
    case UN_COS: case UN_SIN:
      return 30.0;
    default:
      return 60.0;
  }
}

template <typename T> class TreeCompiler {
 public:
  // grad = true: the constant-gradient program: constant subtrees are NOT folded (their
  // constants need tangents) and every constant leaf carries its get_constants index (0-based,
  // depth-first left-to-right) in the instruction's operand field.
  TreeCompiler(const srhip_node* nodes, int64_t nn, const srhip_program& prog, int nfeat_hint, bool grad = false)
      : nd_(nodes), nn_(nn), prog_(prog), nfeat_hint_(nfeat_hint), grad_(grad) {}
  // point a compiler (and its scratch vectors' capacity) at another tree
  void rebind(const srhip_node* nodes, int64_t nn) {
    nd_ = nodes;
    nn_ = nn;
    dmask_ = 0;
  }

  // returns SRHIP_OK or an error (last_error set); fills info and appends to code
  int compile(TreeInfo& info, std::vector<Ins>& code) { return compile_pair(info, code, nullptr, nullptr); }
  // The program of the tree (derived columns as set by set_derived) and, when dinfo is given, its
  // derived program too (derived columns dspec at dbase, set_derived's meaning) from the same
  // analysis: validation, counts, constant numbering and the host-decided checks do not depend on the
  // derived columns, so they run once.  Only code_begin / code_len / need / cost / static_fail of
  // *dinfo are filled (what a population's derived program keeps).
  int compile_pair(TreeInfo& info, std::vector<Ins>& code, TreeInfo* dinfo, std::vector<Ins>* dcode,
                   const std::vector<uint32_t>* dspec = nullptr, int dbase = 0) {
    info = TreeInfo();
    if (nn_ <= 0) return fail(SRHIP_ERR_INVALID, "empty tree");
    memo_const_.assign(nn_, -1);
    state_.assign(nn_, 0);
    int rc = validate(0, 0);
    if (rc) return rc;
    cidx_.assign(nn_, -1);
    tally(0, info);
    // host-decided checks (reference semantics, see header comment)
    static_checks(0, -1, info);
    if (std::is_same<T, float>::value && !grad_ && !info.static_fail) skip_bounds(info);
    rc = emit_program(info, code);
    if (rc || !dinfo) return rc;
    if (!grad_ && !reads_derived(dspec)) {
      // no U(X[f]) node of this tree is a derived column: the derived program is the plain one, byte
      // for byte (every emit decision is the same without a derived column), copied instead of emitted
      dinfo->static_fail = info.static_fail;
      dinfo->need = info.need;
      dinfo->cost = info.cost;
      dinfo->code_begin = (int32_t)dcode->size();
      dinfo->code_len = info.code_len;
      dcode->insert(dcode->end(), code.begin() + info.code_begin, code.begin() + info.code_begin + info.code_len);
      return SRHIP_OK;
    }
    const std::vector<uint32_t>* ds0 = dspec_;
    const int db0 = dbase_;
    set_derived(dspec, dbase);
    scratch_.op_sumcheck.clear();
    scratch_.static_fail = info.static_fail;
    scratch_.need = 0;
    scratch_.cost = 0.0;
    rc = emit_program(scratch_, *dcode);
    set_derived(ds0, db0);
    dinfo->static_fail = scratch_.static_fail;
    dinfo->need = scratch_.need;
    dinfo->cost = scratch_.cost;
    dinfo->code_begin = scratch_.code_begin;
    dinfo->code_len = scratch_.code_len;
    return rc;
  }

 private:
  const srhip_node* nd_;
  int64_t nn_;
  const srhip_program& prog_;
  int nfeat_hint_;
  bool grad_;
  std::vector<int32_t> cidx_;
  std::vector<int8_t> memo_const_;
  std::vector<int16_t> memo_need_;
  std::vector<int32_t> dcolv_;  // derived column per node, or -1
  std::vector<uint8_t> state_;
  std::vector<Ins>* code_ = nullptr;
  TreeInfo* info_ = nullptr;
  const std::vector<uint32_t>* dspec_ = nullptr;  // derived columns (nullptr: plain program)
  int dbase_ = 0;                                 // LDS column of derived column 0
  uint64_t dmask_ = 0;

 public:
  // compile U(X[f]) nodes listed in dspec as reads of LDS column dbase + d (srhip_isa.h)
  void set_derived(const std::vector<uint32_t>* dspec, int dbase) {
    dspec_ = dspec;
    dbase_ = dbase;
  }
  uint64_t dmask() const { return dmask_; }
  // does some U(X[f]) node of the tree read one of the derived columns dspec lists
  bool reads_derived(const std::vector<uint32_t>* dspec) const {
    if (!dspec || dspec->empty()) return false;
    for (int64_t i = 0; i < nn_; ++i) {
      const srhip_node& n = nd_[i];
      if (n.degree != 1 || !leaf_is_feature(n.l)) continue;
      if (find_derived(*dspec, derived_key(classify_unop(unaop(i)), nd_[n.l].feature)) >= 0) return true;
    }
    return false;
  }
  // the value-dependent did_succeed metadata alone (static_fail, fill_consts, feat_checks) of a tree
  // compiled before with other constant values: the gradient program's code does not depend on them
  void static_info(TreeInfo& info) {
    info = TreeInfo();
    memo_const_.assign(nn_, -1);
    static_checks(0, -1, info);
  }

 private:
  TreeInfo scratch_;  // compile_pair's derived-program info (its op_sumcheck's capacity reused)

  // code for the analysed tree (validate, tally and static_checks done) under the current derived
  // columns, appended to code; fills info's need, cost, code_begin and code_len
  int emit_program(TreeInfo& info, std::vector<Ins>& code) {
    dcolv_.assign(dspec_ && !grad_ ? nn_ : 0, -1);
    for (int64_t i = 0; i < (int64_t)dcolv_.size(); ++i) {
      const srhip_node& n = nd_[i];
      if (n.degree != 1 || !leaf_is_feature(n.l)) continue;
      dcolv_[i] = find_derived(*dspec_, derived_key(classify_unop(unaop(i)), nd_[n.l].feature));
    }
    memo_need_.assign(nn_, -1);
    info.code_begin = (int32_t)code.size();
    if (!info.static_fail) {
      info.need = need(0);
      if (info.need > K_MAX)
        return fail(SRHIP_ERR_UNSUPPORTED, "tree needs %d stack slots (> %d)", info.need, K_MAX);
      code_ = &code;
      info_ = &info;
      emit(0, 0, -1);
      if (super_ && (!grad_ || SRHIP_GRAD_SUPER_LEVEL >= 1)) fuse_push_loads(code, info.code_begin);
      Ins end{H_END, 0, 0};
      code.push_back(end);
      for (int64_t i = info.code_begin; i < (int64_t)code.size(); ++i) info.cost += op_cost(code[i].h);
    } else {
      Ins end{H_END, 0, 0};
      code.push_back(end);
    }
    info.code_len = (int32_t)code.size() - info.code_begin;
    return SRHIP_OK;
  }

  // one depth-first pass: node, operator-node and constant counts (count_nodes walks, shared
  // subtrees counted per use) and the get_constants numbering of the constant leaves
  void tally(int64_t i, TreeInfo& info) {
    const srhip_node& n = nd_[i];
    ++info.nnodes;
    if (n.degree == 0) {
      if (n.constant) cidx_[i] = info.nconst++;
      return;
    }
    ++info.nops;
    tally(n.l, info);
    if (n.degree == 2) tally(n.r, info);
  }

  int validate(int64_t i, int depth) {
    if (i < 0 || i >= nn_) return fail(SRHIP_ERR_INVALID, "child index %lld out of range", (long long)i);
    if (depth > 100000) return fail(SRHIP_ERR_INVALID, "tree too deep");
    if (state_[i] == 1) return fail(SRHIP_ERR_INVALID, "cycle in tree at node %lld", (long long)i);
    if (state_[i] == 2) return SRHIP_OK;  // shared subtree (GraphNode) already validated
    state_[i] = 1;
    const srhip_node& n = nd_[i];
    int rc = SRHIP_OK;
    if (n.degree == 0) {
      if (!n.constant) {
        if (n.feature < 1) rc = fail(SRHIP_ERR_INVALID, "feature index %d < 1", (int)n.feature);
        else if (nfeat_hint_ > 0 && n.feature > nfeat_hint_)
          rc = fail(SRHIP_ERR_INVALID, "feature index %d > nfeatures %d", (int)n.feature, nfeat_hint_);
      }
    } else if (n.degree == 1) {
      if (n.op < 1 || n.op > prog_.unaops.size())
        rc = fail(SRHIP_ERR_INVALID, "unary op index %d out of range", (int)n.op);
      else if (std::is_same<T, int32_t>::value && !int_unop_ok(unaop(i)))
        rc = fail(SRHIP_ERR_UNSUPPORTED, "unary op code %d is not defined for Int32", unaop(i));
      else rc = validate(n.l, depth + 1);
    } else if (n.degree == 2) {
      if (n.op < 1 || n.op > prog_.binops.size())
        rc = fail(SRHIP_ERR_INVALID, "binary op index %d out of range", (int)n.op);
      else if (std::is_same<T, int32_t>::value && !int_binop_ok(binop(i)))
        rc = fail(SRHIP_ERR_UNSUPPORTED, "binary op code %d is not defined for Int32", binop(i));
      else {
        rc = validate(n.l, depth + 1);
        if (!rc) rc = validate(n.r, depth + 1);
      }
    } else {
      rc = fail(SRHIP_ERR_INVALID, "bad degree %d", (int)n.degree);
    }
    state_[i] = 2;
    return rc;
  }

  bool is_const(int64_t i) {
    if (memo_const_[i] >= 0) return memo_const_[i];
    const srhip_node& n = nd_[i];
    bool c;
    if (n.degree == 0) c = n.constant;
    else if (n.degree == 1) c = is_const(n.l);
    else c = is_const(n.l) && is_const(n.r);
    memo_const_[i] = c;
    return c;
  }
  // Float32 evaluation programs fold no check statistic for + and -, nor for * by a constant
  // (srhip_eval_impl.h bin_rows_chk).  skip_bounds sets info.sb = (cM, cF, c0) with every such output
  // of the tree within cM M + cF F + c0,
  // M the tree's statistic of the folded values and F the features' max |x|: a folded operator output
  // is within M (a division the in-range path leaves unfolded is within 2^80: + 2^80), a cos / sin
  // within 1, a feature within F, a constant (subtree) its |value|, a +/- within the sum of its
  // operands' bounds and c * x within |c| times x's -- the reduction raises the statistic to that
  // bound, which only ever moves a tree
  // from decided to undecided (the precise pass then decides it exactly); never rounded down
  struct SkipB {
    double m = 0.0, f = 0.0, k = 0.0;
  };
  SkipB skip_bound(int64_t i, SkipB& mx) {
    SkipB b;
    const srhip_node& n = nd_[i];
    if (is_const(i)) {
      T v{};
      if (n.degree == 0) v = HostVal<T>::from(n.val);
      else eval_const(i, &v);
      const double a = fabs((double)v);
      b.k = a == a && a < INFINITY ? a : INFINITY;
      return b;
    }
    if (n.degree == 0) {
      b.f = 1.0;
      return b;
    }
    if (n.degree == 1) {
      (void)skip_bound(n.l, mx);
      const int u = classify_unop(unaop(i));
      if (u == UN_COS || u == UN_SIN) b.k = 1.0;
      else b.m = 1.0;
      return b;
    }
    const SkipB l = skip_bound(n.l, mx), r = skip_bound(n.r, mx);
    int sb, hb;
    classify_binop(binop(i), &sb, &hb);
    if (sb == SB_ADD || sb == SB_SUB) {
      b.m = l.m + r.m;
      b.f = l.f + r.f;
      b.k = l.k + r.k;
      mx.m = std::max(mx.m, b.m);
      mx.f = std::max(mx.f, b.f);
      mx.k = std::max(mx.k, b.k);
      return b;
    }
    if (sb == SB_MUL && (is_const(n.l) || is_const(n.r))) {
      // a product with a constant (the AC / CA / FC / CF forms): |c| times the other operand's bound,
      // never a zero factor -- 0 * Inf is NaN: an operand bound that is infinite (a non-finite feature)
      // must leave the product's bound infinite
      const SkipB& o = is_const(n.l) ? r : l;
      const double a = std::max(is_const(n.l) ? l.k : r.k, 0x1p-126);
      b.m = a * o.m;
      b.f = a * o.f;
      b.k = a * o.k;
      mx.m = std::max(mx.m, b.m);
      mx.f = std::max(mx.f, b.f);
      mx.k = std::max(mx.k, b.k);
      return b;
    }
    b.m = 1.0;
    if (sb == SB_DIV) b.k = 0x1p80;
    return b;
  }
  static float round_up_f(double x) {
    const float f = (float)x;
    return (double)f >= x ? f : std::nextafter(f, INFINITY);
  }
  void skip_bounds(TreeInfo& info) {
    SkipB mx;
    (void)skip_bound(0, mx);
    info.sb[0] = round_up_f(mx.m);
    info.sb[1] = round_up_f(mx.f);
    info.sb[2] = round_up_f(mx.k);
  }
  bool is_leaf(int64_t i) const { return nd_[i].degree == 0; }
  bool leafish(int64_t i) { return is_leaf(i) || (!grad_ && is_const(i)) || dcol(i) >= 0; }
  // derived column of node i (a listed U applied to a feature leaf), or -1
  int dcol(int64_t i) const { return dcolv_.empty() ? -1 : dcolv_[i]; }
  // column a leaf-like operand is read from (feature or derived), or -1 for constants
  int leaf_col(int64_t i) {
    if (leaf_is_feature(i)) return nd_[i].feature - 1;
    const int d = dcol(i);
    if (d < 0) return -1;
    dmask_ |= 1ull << d;
    return dbase_ + d;
  }
  // operand field of an instruction that consumes constant leaf i (gradient program only)
  uint32_t cop(int64_t i) const { return grad_ && cidx_[i] >= 0 ? (uint32_t)cidx_[i] : 0u; }
  int binop(int64_t i) const { return prog_.binops[nd_[i].op - 1]; }
  int unaop(int64_t i) const { return prog_.unaops[nd_[i].op - 1]; }

  // scalar semantics for constant folding (DynamicExpressions _eval_constant_tree)
  static T apply_bin(int code, T a, T b) {
    if constexpr (std::is_same<T, int32_t>::value) {
      switch (code) {
        case SRHIP_OP_ADD: return IOps::add(a, b);
        case SRHIP_OP_SUB: return IOps::sub(a, b);
        case SRHIP_OP_MUL: return IOps::mul(a, b);
        case SRHIP_OP_GREATER: return IOps::greater(a, b);
        case SRHIP_OP_COND: return IOps::cond(a, b);
        case SRHIP_OP_LOGICAL_OR: return IOps::logical_or(a, b);
        case SRHIP_OP_LOGICAL_AND: return IOps::logical_and(a, b);
        case SRHIP_OP_MAX: return IOps::max(a, b);
        case SRHIP_OP_MIN: return IOps::min(a, b);
        default: return 0;
      }
    } else {
      using O = FOps<T>;
      switch (code) {
#define X_(NAME, FN) case SRHIP_OP_##NAME: return O::FN(a, b);
        SRHIP_SPEC_BINOPS(X_)
        SRHIP_HEAVY_BINOPS(X_)
#undef X_
        default: return FP<T>::nan();
      }
    }
  }
  static T apply_un(int code, T a) {
    if constexpr (std::is_same<T, int32_t>::value) {
      switch (code) {
        case SRHIP_OP_NEG: return IOps::neg(a);
        case SRHIP_OP_SQUARE: return IOps::square(a);
        case SRHIP_OP_CUBE: return IOps::cube(a);
        case SRHIP_OP_ABS: return IOps::abs(a);
        case SRHIP_OP_RELU: return IOps::relu(a);
        case SRHIP_OP_SIGN: return IOps::sign(a);
        default: return 0;
      }
    } else {
      using O = FOps<T>;
      switch (code) {
#define X_(NAME, FN) case SRHIP_OP_##NAME: return O::FN(a);
        SRHIP_UNOPS(X_)
#undef X_
        default: return FP<T>::nan();
      }
    }
  }
  // returns ok; value in *v
  bool eval_const(int64_t i, T* v) {
    const srhip_node& n = nd_[i];
    if (n.degree == 0) {  // deg0_eval_constant: no check on the leaf itself
      *v = HostVal<T>::from(n.val);
      return true;
    }
    if (n.degree == 1) {
      T a;
      if (!eval_const(n.l, &a)) return false;
      *v = apply_un(unaop(i), a);
      return m_isfinite(*v);
    }
    T a, b;
    if (!eval_const(n.l, &a)) return false;
    if (!eval_const(n.r, &b)) return false;
    *v = apply_bin(binop(i), a, b);
    return m_isfinite(*v);
  }

  // Reference fusion: node C is evaluated inline (per element, no isfinite(sum)) by its deg-1
  // parent in DynamicExpressions' deg1_l2_ll0_lr0 / deg1_l1_ll0 kernels.
  bool fused_inner(int64_t c, int64_t parent) const {
    if (parent < 0 || nd_[parent].degree != 1) return false;
    const srhip_node& n = nd_[c];
    if (n.degree == 2) return is_leaf(n.l) && is_leaf(n.r);
    if (n.degree == 1) return is_leaf(n.l);
    return false;
  }

  void static_checks(int64_t i, int64_t parent, TreeInfo& info) {
    const srhip_node& n = nd_[i];
    const bool root = parent < 0;
    if (is_const(i)) {
      // constant subtree (or constant leaf): scalar path, fill(c, n) array then checked
      if (n.degree == 0) {
        if (root) info.fill_consts.push_back(n.val);
        else if (!m_isfinite(HostVal<T>::from(n.val))) info.static_fail = true;  // @return_on_check
        return;
      }
      T v;
      if (!eval_const(i, &v)) {
        info.static_fail = true;
        return;
      }
      info.fill_consts.push_back((double)v);
      return;
    }
    if (n.degree == 0) {  // feature leaf
      if (root) info.feat_checks.push_back(n.feature - 1);
      return;
    }
    if (n.degree == 1) {
      const int64_t c = n.l;
      // a feature leaf under a non-fused unary node is evaluated as an array and checked
      if (is_leaf(c) && !nd_[c].constant && !fused_inner(i, parent)) info.feat_checks.push_back(nd_[c].feature - 1);
      static_checks(c, i, info);
      return;
    }
    static_checks(n.l, i, info);
    static_checks(n.r, i, info);
  }

  int need(int64_t i) {
    if (memo_need_[i] < 0) memo_need_[i] = (int16_t)need_(i);
    return memo_need_[i];
  }
  int need_(int64_t i) {
    if (leafish(i)) return 0;
    const srhip_node& n = nd_[i];
    if (n.degree == 1) return need(n.l);
    const bool ll = leafish(n.l), rl = leafish(n.r);
    int sb, hb;
    classify_binop(binop(i), &sb, &hb);
    const int leaf_slot = hb >= 0 ? 1 : 0;  // a heavy op's leaf operand is loaded into a slot
    if (ll && rl) return leaf_slot;
    if (rl) return std::max(need(n.l), leaf_slot);
    if (ll) return std::max(need(n.r), leaf_slot);
    const int a = need(n.l), b = need(n.r);
    return a == b ? a + 1 : std::max(a, b);
  }

  void push_ins(uint32_t h, uint32_t a, uint64_t imm) { code_->push_back(Ins{h, a, imm}); }
  // operator instruction: a = (op ordinal + 1) << 16 | operand -- or, in a gradient program's
  // leaf-constant superinstructions (FC / CF), hi = the constant's index in the upper half (the
  // interpreter's precise pass counts operator ordinals in execution order: srhip_eval_impl.h
  // precise_hook; only a derived-column load needs its ordinal field, to mark it an operator)
  void push_op(uint32_t h, uint32_t operand, uint64_t imm, int64_t node, int64_t parent, int64_t hi = -1) {
    // the gradient program evaluates constant subtrees per row (their constants need tangents); the
    // reference evaluates them as scalars (_eval_constant_tree): finiteness only, no isfinite(sum)
    const bool scalar = grad_ && is_const(node);
    info_->op_sumcheck.push_back((!scalar && (parent < 0 || !fused_inner(node, parent))) ? 1 : 0);
    const uint32_t ord = (uint32_t)info_->op_sumcheck.size();
    push_ins(h, ((hi >= 0 ? (uint32_t)hi : ord) << 16) | (operand & 0xffff), imm);
  }
  uint64_t leaf_imm(int64_t i) {
    if (nd_[i].degree == 0) return HostVal<T>::bits(HostVal<T>::from(nd_[i].val));
    T v;
    eval_const(i, &v);  // folded constant subtree (ok: checked in static_checks)
    return HostVal<T>::bits(v);
  }
  bool leaf_is_feature(int64_t i) const { return nd_[i].degree == 0 && !nd_[i].constant; }

  // Superinstructions (SRHIP_NO_SUPER=1 turns them off; gradient programs as far as the build's
  // SRHIP_GRAD_SUPER_LEVEL allows -- none by default -- and SRHIP_GRAD_NO_SUPER=1 turns those off): the
  // leaf-leaf operand forms (emit) and a push fused with the leaf load that
  // follows it: one dispatch instead of two.  In a gradient program a leaf-constant form carries the
  // constant's index in its upper half (push_op's hi) and a push fuses with a plain feature or constant
  // load only (a derived-column load is an operator of its own).
  const bool super_ = grad_ ? grad_super_env() : super_env();

 public:
  static bool super_env() {
    const char* e = env_get("SRHIP_NO_SUPER");
    return !(e && *e && *e != '0');
  }
  static bool grad_super_env() {
    const char* e = env_get("SRHIP_GRAD_NO_SUPER");
    return super_env() && !(e && *e && *e != '0');
  }
  static bool grad_uniform_env() {
    const char* e = env_get("SRHIP_GRAD_UNIFORM");
    return !(e && *e == '0');
  }

 private:
  static void fuse_push_loads(std::vector<Ins>& code, int32_t begin) {
    size_t w = (size_t)begin;
    for (size_t r = (size_t)begin; r < code.size(); ++r) {
      const Ins& a = code[r];
      if (a.h >= H_PUSH0 && a.h < H_PUSH0 + K_MAX && r + 1 < code.size() &&
          ((code[r + 1].h == H_LOADF && (code[r + 1].a >> 16) == 0) || code[r + 1].h == H_LOADC)) {
        const Ins& b = code[r + 1];
        const uint32_t k = a.h - H_PUSH0;
        code[w++] = Ins{(b.h == H_LOADF ? H_PUSHLF0 : H_PUSHLC0) + k, b.a, b.imm};
        ++r;
        continue;
      }
      code[w++] = a;
    }
    code.resize(w);
  }

  void emit_leaf(int64_t i) {
    const int col = leaf_col(i);
    if (col >= 0) push_ins(H_LOADF, (uint32_t)col, 0);
    else push_ins(H_LOADC, cop(i), leaf_imm(i));
  }

  void emit(int64_t i, int base, int64_t parent) {
    if (leafish(i)) {
      emit_leaf(i);
      return;
    }
    const srhip_node& n = nd_[i];
    if (n.degree == 1) {
      if (grad_ && prog_.g_want_derived && leaf_is_feature(n.l)) {
        // a heavy operator of a feature in a constant-gradient program: its derived column (the
        // operator's value, no tangent), loaded with the operator's own ordinal -- its check fold and
        // precise sum stay where the operator's were
        const int32_t j = find_derived(prog_.gdspec, derived_key(classify_unop(unaop(i)), nd_[n.l].feature));
        if (j >= 0) {
          push_op(H_LOADF, (uint32_t)(prog_.gdbase + j), 0, i, parent);
          return;
        }
      }
      emit(n.l, base, i);
      const int u = classify_unop(unaop(i));
      // cos / sin of an operator output need no check fold of their own (srhip_isa.h UN_NC_FLAG); the
      // gradient program keeps every fold
      const bool nc = SRHIP_COS_NC && !grad_ && !leafish(n.l) && (u == UN_COS || u == UN_SIN);
      // gradient programs: an operator of a constant subtree (one value on every row) is evaluated
      // once per lane (SRHIP_GRAD_UNIFORM=0: per row)
      const bool uni = grad_ && is_const(n.l) && grad_uniform_env();
      push_op(h_un(u), (nc ? UN_NC_FLAG : 0) | (uni ? UN_UNIFORM_FLAG : 0), 0, i, parent);
      return;
    }
    int sb, hb;
    classify_binop(binop(i), &sb, &hb);
    const int64_t L = n.l, Rr = n.r;
    const bool ll = leafish(L), rl = leafish(Rr);
    if (sb >= 0) {
      // (a gradient program's two constant leaves keep the uniform constant form below)
      if (ll && rl && super_ && (!grad_ || SRHIP_GRAD_SUPER_LEVEL >= 2) && (leaf_col(L) >= 0 || leaf_col(Rr) >= 0)) {
        // deg2_l0_r0: both operands leaves (feature, derived column or constant) in one instruction
        const int cl = leaf_col(L), cr = leaf_col(Rr);
        if (cl >= 0 && cr >= 0) push_op(h_spec(sb, SPEC_FF), cl, (uint64_t)cr, i, parent);
        else if (cl >= 0) push_op(h_spec(sb, SPEC_FC), cl, leaf_imm(Rr), i, parent, grad_ ? (int64_t)cop(Rr) : -1);
        else push_op(h_spec(sb, SPEC_CF), cr, leaf_imm(L), i, parent, grad_ ? (int64_t)cop(L) : -1);
        return;
      }
      // gradient programs: an operator of two constant subtrees (one value on every row) is evaluated
      // once per lane (the forms whose operand field is a constant index or unused)
      const uint32_t uni = grad_ && is_const(i) && grad_uniform_env() ? UN_UNIFORM_FLAG : 0u;
      if (rl) {
        emit(L, base, i);
        if (leaf_col(Rr) >= 0) push_op(h_spec(sb, SPEC_AF), leaf_col(Rr), 0, i, parent);
        else push_op(h_spec(sb, SPEC_AC), cop(Rr) | uni, leaf_imm(Rr), i, parent);
      } else if (ll) {
        emit(Rr, base, i);
        if (leaf_col(L) >= 0) push_op(h_spec(sb, SPEC_FA), leaf_col(L), 0, i, parent);
        else push_op(h_spec(sb, SPEC_CA), cop(L) | uni, leaf_imm(L), i, parent);
      } else if (need(L) >= need(Rr)) {
        emit(L, base, i);
        push_ins(H_PUSH0 + base, 0, 0);
        emit(Rr, base + 1, i);
        push_op(h_spec(sb, SPEC_SA0 + base), uni, 0, i, parent);
      } else {
        emit(Rr, base, i);
        push_ins(H_PUSH0 + base, 0, 0);
        emit(L, base + 1, i);
        push_op(h_spec(sb, SPEC_AS0 + base), uni, 0, i, parent);
      }
      return;
    }
    // heavy binary op (pow, mod, atan2): the second operand lives in stack slot `base`
    if (rl) {
      emit(L, base, i);
      if (leaf_col(Rr) >= 0) push_ins(H_SLOADF0 + base, leaf_col(Rr), 0);
      else push_ins(H_SLOADC0 + base, cop(Rr), leaf_imm(Rr));
      push_op(h_heavy(hb, HEAVY_AS0 + base), 0, 0, i, parent);  // A = A op S[base]
    } else if (ll) {
      emit(Rr, base, i);
      if (leaf_col(L) >= 0) push_ins(H_SLOADF0 + base, leaf_col(L), 0);
      else push_ins(H_SLOADC0 + base, cop(L), leaf_imm(L));
      push_op(h_heavy(hb, HEAVY_SA0 + base), 0, 0, i, parent);  // A = S[base] op A
    } else if (need(L) >= need(Rr)) {
      emit(L, base, i);
      push_ins(H_PUSH0 + base, 0, 0);
      emit(Rr, base + 1, i);
      push_op(h_heavy(hb, HEAVY_SA0 + base), 0, 0, i, parent);  // A = S op A
    } else {
      emit(Rr, base, i);
      push_ins(H_PUSH0 + base, 0, 0);
      emit(L, base + 1, i);
      push_op(h_heavy(hb, HEAVY_AS0 + base), 0, 0, i, parent);  // A = A op S
    }
  }
};

// Host worker threads for the compiler: created once per process (a fork child makes its own) and
// parked on a condition variable between jobs, so a population compile pays no thread start-up.
// One job at a time; a caller that finds the pool busy (concurrent coalescer flushes) runs its items
// itself.  The process's pool is never destroyed: detached workers parked at exit are simply ended.
// Work items are claimed from one 64-bit counter holding (job generation << 32 | next index): a
// worker snapshots (generation, fn, n) under the mutex when it wakes, and a claim succeeds only by a
// compare-exchange on its own generation, so a worker delayed past the end of its job can never run
// an item of the next one (nor count it done).
class HostPool {
 public:
  static HostPool& get() {
    // lock-free, so that a fork taken while another thread is here cannot leave a held mutex behind;
    // the loser of a creation race shuts its own pool down (joins its threads) and deletes it
    static std::atomic<HostPool*> pool{nullptr};
    HostPool* p = pool.load();
    if (!p || p->pid_ != getpid()) {
      HostPool* q = new HostPool();
      if (pool.compare_exchange_strong(p, q)) {
        p = q;
      } else {
        q->shutdown();
        delete q;
      }
    }
    return *p;
  }
  int threads() const { return (int)nthr_ + 1; }
  // fn(0) .. fn(n - 1) on the pool's threads and the caller; false (nothing run) if busy
  bool run(int n, const std::function<void(int)>& fn) {
    std::unique_lock<std::mutex> busy(busy_mu_, std::try_to_lock);
    if (!busy.owns_lock()) return false;
    uint32_t g;
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn;
      n_ = n;
      done_ = 0;
      g = ++gen_;
      next_.store((uint64_t)g << 32);
    }
    cv_.notify_all();
    work(g, &fn, n);
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return done_ == n_; });
    fn_ = nullptr;
    return true;
  }

 private:
  HostPool() : pid_(getpid()) {
    // up to 15 workers + the caller: the CPU share a GPU process gets on the MI355X boxes (16);
    // hardware_concurrency there reports the whole machine
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    nthr_ = std::min(15u, hw - 1);
    // SRHIP_POOL_NICE = n > 0: the workers run at nice n, so a thread that is waiting for the device
    // (an evaluation beside a pipelined compile) gets its core back first when the device finishes
    const char* ne = getenv("SRHIP_POOL_NICE");
    const int nice_v = ne && *ne ? atoi(ne) : 0;
    for (unsigned i = 0; i < nthr_; ++i)
      threads_.emplace_back([this, nice_v] {
        if (nice_v > 0) (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), nice_v);
        loop();
      });
  }
  ~HostPool() {
    for (std::thread& t : threads_)
      if (t.joinable()) t.detach();
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
      ++gen_;
    }
    cv_.notify_all();
    for (std::thread& t : threads_)
      if (t.joinable()) t.join();
  }
  void loop() {
    uint32_t seen = 0;
    for (;;) {
      uint32_t g;
      const std::function<void(int)>* fn;
      int n;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = g = gen_;
        fn = fn_;
        n = n_;
      }
      if (fn) work(g, fn, n);
    }
  }
  void work(uint32_t g, const std::function<void(int)>* fn, int n) {
    for (;;) {
      uint64_t v = next_.load();
      if ((uint32_t)(v >> 32) != g || (int)(uint32_t)v >= n) return;
      if (!next_.compare_exchange_weak(v, v + 1)) continue;
      (*fn)((int)(uint32_t)v);
      std::lock_guard<std::mutex> lk(mu_);
      if (++done_ == n_) cv_done_.notify_all();
    }
  }
  const pid_t pid_;
  unsigned nthr_ = 0;
  std::vector<std::thread> threads_;
  std::mutex busy_mu_, mu_;
  std::condition_variable cv_, cv_done_;
  const std::function<void(int)>* fn_ = nullptr;
  int n_ = 0, done_ = 0;
  bool stop_ = false;
  std::atomic<uint64_t> next_{0};
  uint32_t gen_ = 0;
};

// Per-tree code cache: a tree's compiled code and metadata depend only on its node table (constant
// values included: folded constants are immediates), the operator tables and the element type, and
// its derived-program code also on which derived column each of its U(X[f]) nodes reads and where the
// derived columns start (the population's feature count).  Entries are keyed by a hash of the node
// bytes and operator tables and confirmed by comparing them in full, so a hit returns exactly the
// bytes a compile would produce.  Sharded by hash; a shard that grows past its share of
// CODE_CACHE_ENTRIES is emptied (the cache holds recent trees: the search's survivors, migrants and
// re-scored members).  SRHIP_NO_CODE_CACHE=1 bypasses it (read per compile).
// Entries are made on a tree's SECOND sighting: the first only records its hash in a lossy
// direct-mapped table of the shard (one 8-byte store), so a population of new trees -- every tree
// of a fresh population misses -- does not pay for copying ~10 vectors per tree into entries it will
// never hit (C2's 1024-tree compile, one thread: 7.6 -> ~4.6 ms).  A tree that recurs (survivors,
// migrants, re-scored members) is cached from its second compile and hits from its third.
// SRHIP_CODE_CACHE_EAGER=1 makes entries on the first sighting (read per compile).
constexpr int CODE_CACHE_SHARDS = 64;
constexpr size_t CODE_CACHE_ENTRIES = 1 << 15;
constexpr size_t CODE_CACHE_SEEN = 1 << 12;  // first-sighting hashes per shard
std::atomic<int64_t> g_cache_hits{0}, g_cache_misses{0}, g_cache_inserts{0};

inline uint64_t mix64(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  return h ^ (h >> 33);
}
inline uint64_t hash_words(const void* p, size_t bytes, uint64_t h) {
  const unsigned char* c = (const unsigned char*)p;
  size_t i = 0;
  for (; i + 8 <= bytes; i += 8) {
    uint64_t w;
    memcpy(&w, c + i, 8);
    h = mix64(h ^ w) + 0x9e3779b97f4a7c15ull;
  }
  for (; i < bytes; ++i) h = mix64(h ^ c[i]);
  return h;
}
inline uint64_t ops_hash(const srhip_program& P) {
  uint64_t h = hash_words(P.binops.data(), P.binops.size() * 4, 0x5eed ^ P.binops.size());
  return hash_words(P.unaops.data(), P.unaops.size() * 4, h ^ (P.unaops.size() << 20));
}

template <typename T> class CodeCache {
 public:
  struct Derived {
    int32_t dbase = -1;
    std::vector<int32_t> dsig;  // derived column of each U(X[f]) node, in node order (-1: none)
    std::vector<Ins> code;
    TreeInfo info;              // need, cost, code_len, static_fail
    uint64_t dmask = 0;
  };
  static CodeCache& get() {
    static CodeCache* c = new CodeCache();  // never destroyed (worker threads may outlive statics)
    return *c;
  }
  static bool enabled() {
    const char* e = env_get("SRHIP_NO_CODE_CACHE");
    return !(e && *e && *e != '0');
  }
  // derived column per U(X[f]) node of a valid tree (as TreeCompiler::emit_program assigns them)
  static void derived_sig(const srhip_node* nd, int64_t nn, const srhip_program& P, std::vector<int32_t>& sig) {
    sig.clear();
    for (int64_t i = 0; i < nn; ++i) {
      const srhip_node& n = nd[i];
      if (n.degree != 1 || nd[n.l].degree != 0 || nd[n.l].constant) continue;
      sig.push_back(find_derived(P.dspec, derived_key(classify_unop(P.unaops[n.op - 1]), nd[n.l].feature)));
    }
  }
  // On a hit, appends the plain code to code (and, with dcode, the derived code to dcode) exactly as
  // TreeCompiler::compile / compile_pair would, fills info / *dinfo / *dmask and returns true.
  // Returns LOOKUP_HIT (filled), LOOKUP_SEEN (a miss whose hash was seen before: compile and insert)
  // or LOOKUP_NEW (a first sighting, now recorded: compile, do not insert unless eager).
  enum { LOOKUP_NEW = 0, LOOKUP_HIT = 1, LOOKUP_SEEN = 2 };
  int lookup(uint64_t h, const srhip_node* nd, int64_t nn, const srhip_program& P, bool sup, TreeInfo& info,
             std::vector<Ins>& code, TreeInfo* dinfo, std::vector<Ins>* dcode, uint64_t* dmask,
             std::vector<int32_t>& sig) {
    Shard& s = shards_[h % CODE_CACHE_SHARDS];
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.map.find(h);
    if (it == s.map.end()) {
      const uint64_t hk = h ? h : 1;  // 0 marks an empty slot
      uint64_t& slot = s.seen[(h / CODE_CACHE_SHARDS) % CODE_CACHE_SEEN];
      if (slot == hk) return LOOKUP_SEEN;
      slot = hk;
      return LOOKUP_NEW;
    }
    const Entry& e = it->second;
    if (!same(e, nd, nn, P, sup)) return LOOKUP_SEEN;  // a hash collision with a cached tree
    if (dinfo) {
      derived_sig(nd, nn, P, sig);
      if (!e.d || e.d->dbase != P.maxfeat || e.d->dsig != sig) return LOOKUP_SEEN;
      dinfo->static_fail = e.d->info.static_fail;
      dinfo->need = e.d->info.need;
      dinfo->cost = e.d->info.cost;
      dinfo->code_len = e.d->info.code_len;
      dinfo->code_begin = (int32_t)dcode->size();
      dcode->insert(dcode->end(), e.d->code.begin(), e.d->code.end());
      *dmask = e.d->dmask;
    }
    info = e.info;
    info.code_begin = (int32_t)code.size();
    code.insert(code.end(), e.code.begin(), e.code.end());
    return LOOKUP_HIT;
  }
  void insert(uint64_t h, const srhip_node* nd, int64_t nn, const srhip_program& P, bool sup, const TreeInfo& info,
              const Ins* code, const TreeInfo* dinfo, const Ins* dcode, uint64_t dmask) {
    Entry e;
    e.nodes.assign(nd, nd + nn);
    e.binops = P.binops;
    e.unaops = P.unaops;
    e.super = sup;
    e.info = info;
    e.code.assign(code, code + info.code_len);
    if (dinfo) {
      e.d.reset(new Derived());
      e.d->dbase = P.maxfeat;
      derived_sig(nd, nn, P, e.d->dsig);
      e.d->info.static_fail = dinfo->static_fail;
      e.d->info.need = dinfo->need;
      e.d->info.cost = dinfo->cost;
      e.d->info.code_len = dinfo->code_len;
      e.d->code.assign(dcode, dcode + dinfo->code_len);
      e.d->dmask = dmask;
    }
    Shard& s = shards_[h % CODE_CACHE_SHARDS];
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.map.size() >= CODE_CACHE_ENTRIES / CODE_CACHE_SHARDS) s.map.clear();
    s.map[h] = std::move(e);
  }

 private:
  struct Entry {
    std::vector<srhip_node> nodes;
    std::vector<int32_t> binops, unaops;
    bool super = true;  // compiled with superinstructions (SRHIP_NO_SUPER unset)
    TreeInfo info;
    std::vector<Ins> code;
    std::unique_ptr<Derived> d;
  };
  struct Shard {
    std::mutex mu;
    std::unordered_map<uint64_t, Entry> map;
    std::vector<uint64_t> seen = std::vector<uint64_t>(CODE_CACHE_SEEN, 0);
  };
  static bool same(const Entry& e, const srhip_node* nd, int64_t nn, const srhip_program& P, bool sup) {
    return e.super == sup && (int64_t)e.nodes.size() == nn && memcmp(e.nodes.data(), nd, (size_t)nn * sizeof(srhip_node)) == 0 &&
           e.binops == P.binops && e.unaops == P.unaops;
  }
  Shard shards_[CODE_CACHE_SHARDS];
};

// The population's programs in one pass over the trees: the plain program and, when the population
// has derived columns (srhip_isa.h), the derived program, compiled tree by tree on the host pool
// (contiguous tree ranges; per-range code vectors concatenated in tree order: the same bytes as one
// sequential pass).  Derived columns: the heavy U(X[f]) nodes of the population's trees are counted
// first, the pairs used at least DERIVE_MIN_USES times kept (most used first, at most DERIVE_MAX).
// SRHIP_NO_DERIVE=1 disables them.
template <typename T>
void choose_derived_t(srhip_program& P) {
  P.dspec.clear();
  const char* env = env_get("SRHIP_NO_DERIVE");
  const bool off = env && *env && *env != '0';
  if (std::is_same<T, int32_t>::value || off) return;
  std::vector<std::pair<uint32_t, int>> cnt;  // (key, uses), in order of first use
  // uses counted in a dense (unary class, feature) table when it is small, else by search in cnt
  const int64_t nf = std::max<int32_t>(P.maxfeat, 1);
  const bool dense = (int64_t)NUM_UNOP * nf <= (1 << 16);
  std::vector<int32_t> slot(dense ? (size_t)(NUM_UNOP * nf) : 0, -1);  // index into cnt
  for (int32_t t = 0; t < P.ntrees; ++t) {
    // node tables are per tree with tree-relative child indices
    const int64_t b = P.offsets[t], e = P.offsets[t + 1];
    for (int64_t i = b; i < e; ++i) {
      const srhip_node& n = P.nodes[i];
      if (n.degree != 1) continue;
      // (this pass runs before the trees are validated: a malformed child or operator index is
      // skipped here and rejected by the compiler's validation with SRHIP_ERR_INVALID)
      if (n.l < 0 || n.l >= e - b) continue;
      if (n.op < 1 || (size_t)n.op > P.unaops.size()) continue;
      const srhip_node& c = P.nodes[b + n.l];
      if (c.degree != 0 || c.constant || c.feature < 1) continue;
      const int u = classify_unop(P.unaops[n.op - 1]);
      if (!un_derivable(u)) continue;
      const uint32_t key = derived_key(u, c.feature);
      int32_t* sl = dense && c.feature <= nf ? &slot[(size_t)u * nf + (c.feature - 1)] : nullptr;
      int32_t k = sl ? *sl : -1;
      if (!sl) {
        auto it = std::find_if(cnt.begin(), cnt.end(), [&](const std::pair<uint32_t, int>& q) { return q.first == key; });
        if (it != cnt.end()) k = (int32_t)(it - cnt.begin());
      }
      if (k < 0) {
        k = (int32_t)cnt.size();
        cnt.emplace_back(key, 0);
        if (sl) *sl = k;
      }
      ++cnt[k].second;
    }
  }
  std::stable_sort(cnt.begin(), cnt.end(), [](const std::pair<uint32_t, int>& a, const std::pair<uint32_t, int>& b) {
    return a.second > b.second;
  });
  static const int dmax_env = [] { const char* e = getenv("SRHIP_DERIVE_MAX"); return e ? atoi(e) : -1; }();
  const int dmax = dmax_env >= 0 ? std::min(dmax_env, DERIVE_MAX) : DERIVE_MAX;
  for (const auto& e : cnt)
    if (e.second >= DERIVE_MIN_USES && (int)P.dspec.size() < dmax) P.dspec.push_back(e.first);
}

static TreeDecide make_decide(const TreeInfo& I) {
  TreeDecide d;
  for (double c : I.fill_consts)
    if (!std::isnan(c)) d.maxc = std::max(d.maxc, fabs(c));
  for (int f : I.feat_checks) {
    if (f >= 0 && f < 64) d.feat_mask |= (uint64_t)1 << f;
    else d.slow = 1;
  }
  d.nnodes = I.nnodes;
  d.nops = I.nops;
  d.static_fail = I.static_fail;
  d.has_op = !I.op_sumcheck.empty();
  return d;
}
template <typename T>
int compile_program_t(srhip_program& P) {
  const int32_t n = P.ntrees;
  P.code.clear();
  P.prog_off.assign(n, 0);
  P.info.assign(n, TreeInfo());
  P.kmax = 0;
  P.max_ops = 0;
  P.max_len = 0;
  P.total_nodes = 0;
  P.total_ops = 0;
  P.dmask.assign(n, 0);
  P.dcode.clear();
  P.dprog_off.assign(n, 0);
  P.dcost.assign(n, 0.0);
  P.dec.assign(n, TreeDecide());
  P.sbound.clear();
  P.dkmax = P.dmax_len = 0;
  // operator-node count and the largest feature index, from the node tables
  P.maxfeat = 0;
  for (const srhip_node& nd : P.nodes) {
    P.total_ops += nd.degree > 0;
    if (nd.degree == 0 && !nd.constant) P.maxfeat = std::max<int32_t>(P.maxfeat, nd.feature);
  }
  choose_derived_t<T>(P);
  const bool der = !P.dspec.empty();
  std::vector<TreeInfo> dinfo(der ? n : 0);
  HostPool& pool = HostPool::get();
  // SRHIP_COMPILE_THREADS caps the threads one compile uses (read per compile; default: the pool)
  const int cap_env = env_int("SRHIP_COMPILE_THREADS", 0);
  const int wmax = cap_env > 0 ? std::min(cap_env, pool.threads()) : pool.threads();
  const int W = (int)std::max<int64_t>(1, std::min<int64_t>(wmax, (int64_t)n / 64));
  std::vector<std::vector<Ins>> part(W), dpart(W);
  std::vector<std::string> errs(W);
  std::vector<int> rcs(W, SRHIP_OK);
  CodeCache<T>* cache = CodeCache<T>::enabled() ? &CodeCache<T>::get() : nullptr;
  const bool sup = TreeCompiler<T>::super_env();
  const uint64_t oph = cache ? ops_hash(P) ^ (sup ? 0x5u : 0u) : 0;
  const bool eager = env_flag("SRHIP_CODE_CACHE_EAGER");
  const std::function<void(int)> range = [&](int w) {
    const int32_t t0 = (int32_t)((int64_t)n * w / W), t1 = (int32_t)((int64_t)n * (w + 1) / W);
    TreeCompiler<T> tc(nullptr, 0, P, 0);
    std::vector<int32_t> sig;
    int64_t nhit = 0, nmiss = 0, nins = 0;
    struct Count {  // the range's cache counters, added once at its end
      int64_t &a, &b, &c;
      ~Count() {
        g_cache_hits += a;
        g_cache_misses += b;
        g_cache_inserts += c;
      }
    } count{nhit, nmiss, nins};
    for (int32_t t = t0; t < t1 && !rcs[w]; ++t) {
      const int64_t b = P.offsets[t], e = P.offsets[t + 1];
      const srhip_node* tn = P.nodes.data() + b;
      uint64_t h = 0;
      bool keep = false;  // make a cache entry of this compile
      if (cache) {
        h = hash_words(tn, (size_t)(e - b) * sizeof(srhip_node), oph ^ (uint64_t)(e - b));
        const int lk = cache->lookup(h, tn, e - b, P, sup, P.info[t], part[w], der ? &dinfo[t] : nullptr,
                                     der ? &dpart[w] : nullptr, &P.dmask[t], sig);
        if (lk == CodeCache<T>::LOOKUP_HIT) {
          ++nhit;
          continue;
        }
        ++nmiss;
        keep = eager || lk == CodeCache<T>::LOOKUP_SEEN;
      }
      tc.rebind(tn, e - b);
      const int rc = der ? tc.compile_pair(P.info[t], part[w], &dinfo[t], &dpart[w], &P.dspec, P.maxfeat)
                         : tc.compile(P.info[t], part[w]);
      if (!rc && der) P.dmask[t] = tc.dmask();
      if (!rc && keep && cache) {
        ++nins;
        cache->insert(h, tn, e - b, P, sup, P.info[t], part[w].data() + P.info[t].code_begin, der ? &dinfo[t] : nullptr,
                      der ? dpart[w].data() + dinfo[t].code_begin : nullptr, P.dmask[t]);
      }
      if (rc) {
        errs[w] = "tree " + std::to_string(t) + ": " + last_error();
        rcs[w] = rc;
      }
    }
  };
  if (W == 1 || !pool.run(W, range))
    for (int w = 0; w < W; ++w) range(w);
  for (int w = 0; w < W; ++w)
    if (rcs[w]) return fail(rcs[w], "%s", errs[w].c_str());
  for (int w = 0; w < W; ++w) {
    const int32_t t0 = (int32_t)((int64_t)n * w / W), t1 = (int32_t)((int64_t)n * (w + 1) / W);
    const int32_t base = (int32_t)P.code.size(), dbase = (int32_t)P.dcode.size();
    for (int32_t t = t0; t < t1; ++t) {
      P.info[t].code_begin += base;
      if (der) dinfo[t].code_begin += dbase;
    }
    P.code.insert(P.code.end(), part[w].begin(), part[w].end());
    if (der) P.dcode.insert(P.dcode.end(), dpart[w].begin(), dpart[w].end());
  }
  for (int32_t t = 0; t < n; ++t) {
    P.prog_off[t] = P.info[t].code_begin;
    P.kmax = std::max(P.kmax, P.info[t].need);
    P.max_ops = std::max(P.max_ops, (int32_t)P.info[t].op_sumcheck.size());
    P.max_len = std::max(P.max_len, P.info[t].code_len);
    P.total_nodes += P.info[t].nnodes;
    P.dec[t] = make_decide(P.info[t]);
    if (std::is_same<T, float>::value) P.sbound.insert(P.sbound.end(), {P.info[t].sb[0], P.info[t].sb[1], P.info[t].sb[2], 0.0f});
    if (der) {
      const TreeInfo& ti = dinfo[t];
      P.dprog_off[t] = ti.code_begin;
      P.dcost[t] = ti.cost;
      P.dkmax = std::max(P.dkmax, ti.need);
      P.dmax_len = std::max(P.dmax_len, ti.code_len);
    }
  }
  // (diagnostic) SRHIP_DUMP_CODE=path: the derived (or plain) program's instructions as int32 (h, a,
  // imm low, imm high) records with a (-1, static_fail, need, cost) separator per tree, for
  // instruction-mix studies (scripts/code_stats.py) and the code-cache test; with derived columns the
  // plain program's go to path.plain
  if (const char* dump = env_get("SRHIP_DUMP_CODE")) {
    for (int pass = 0; pass < (der ? 2 : 1); ++pass) {
      const bool dd = der && pass == 0;
      FILE* f = fopen(pass ? (std::string(dump) + ".plain").c_str() : dump, "wb");
      if (!f) break;
      const std::vector<Ins>& code = dd ? P.dcode : P.code;
      for (int32_t t = 0; t < n; ++t) {
        const TreeInfo& ti = dd ? dinfo[t] : P.info[t];
        for (int32_t i = 0; i < ti.code_len; ++i) {
          const Ins& ins = code[(size_t)ti.code_begin + i];
          const int32_t rec[4] = {(int32_t)ins.h, (int32_t)ins.a, (int32_t)(uint32_t)ins.imm,
                                  (int32_t)(uint32_t)(ins.imm >> 32)};
          fwrite(rec, sizeof rec, 1, f);
        }
        const int32_t sep[4] = {-1, ti.static_fail ? 1 : 0, ti.need, (int32_t)ti.cost};
        fwrite(sep, sizeof sep, 1, f);
      }
      fclose(f);
    }
  }
  return SRHIP_OK;
}

template <typename T>
int compile_grad_t(srhip_program& P) {
  P.g_derived = P.g_want_derived && !P.gdspec.empty();
  if (!P.g_derived) P.g_want_derived = false;
  P.gcode.clear();
  P.gprog_off.assign(P.ntrees, 0);
  P.ginfo.assign(P.ntrees, TreeInfo());
  P.gkmax = 0;
  P.gmax_len = 0;
  P.gmax_ops = 0;
  for (int32_t t = 0; t < P.ntrees; ++t) {
    const int64_t b = P.offsets[t], e = P.offsets[t + 1];
    TreeCompiler<T> tc(P.nodes.data() + b, e - b, P, 0, true);
    TreeInfo& gi = P.ginfo[t];
    int rc = tc.compile(gi, P.gcode);
    if (rc) return fail(rc, "tree %d (gradient program): %s", (int)t, last_error());
    P.gprog_off[t] = gi.code_begin;
    P.gkmax = std::max(P.gkmax, gi.need);
    P.gmax_len = std::max(P.gmax_len, gi.code_len);
    P.gmax_ops = std::max(P.gmax_ops, (int32_t)gi.op_sumcheck.size());
  }
  // speculative slots: the constant-carrying instructions of every tree, and the region itself
  P.gci_off.assign(P.ntrees + 1, 0);
  P.gci.clear();
  P.gspec_ok.assign(P.ntrees, 0);
  P.gbase.assign(P.ntrees, TreeInfo());
  for (int32_t t = 0; t < P.ntrees; ++t) {
    const TreeInfo& gi = P.ginfo[t];
    if (!gi.static_fail) {
      int32_t nc = 0;
      for (int32_t i = 0; i < gi.code_len; ++i) {
        const Ins& ins = P.gcode[(size_t)gi.code_begin + i];
        bool carries = ins.h == H_LOADC || (ins.h >= H_SLOADC0 && ins.h < H_SLOADC0 + K_MAX) ||
                       (ins.h >= H_PUSHLC0 && ins.h < H_PUSHLC0 + K_MAX);
        bool hi = false;  // the constant index in the upper half (leaf-constant superinstructions)
        if (ins.h >= H_BIN0 && ins.h < H_HEAVY0) {
          const uint32_t form = (ins.h - H_BIN0) % SPEC_STRIDE;
          carries = form == SPEC_AC || form == SPEC_CA || form == SPEC_FC || form == SPEC_CF;
          hi = form == SPEC_FC || form == SPEC_CF;
        }
        if (!carries) continue;
        P.gci.push_back(i);
        P.gci.push_back((int32_t)(hi ? ins.a >> 16 : ins.a & 0xffff & ~UN_UNIFORM_FLAG));  // (the constant index)
        ++nc;
      }
      // every constant leaf is consumed by exactly one such instruction
      P.gspec_ok[t] = nc == gi.nconst;
      if (P.gspec_ok[t]) P.gbase[t] = gi;
      else P.gci.resize(P.gci_off[t]);
    }
    P.gci_off[t + 1] = (int32_t)P.gci.size();
  }
  P.gspec_alloc = P.gspec_cap;
  P.gspec_stride = std::max<int32_t>(1, P.gmax_len);
  P.gspec_base = (int64_t)P.gcode.size();
  P.gcode.resize(P.gcode.size() + (size_t)P.gspec_alloc * P.gspec_stride, Ins{H_END, 0, 0});
  for (int32_t sl = 0; sl < P.gspec_alloc; ++sl) {
    P.gprog_off.push_back((int32_t)(P.gspec_base + (int64_t)sl * P.gspec_stride));
    TreeInfo si;
    si.static_fail = true;
    si.code_begin = P.gprog_off.back();
    si.code_len = 1;
    P.ginfo.push_back(si);
  }
  return SRHIP_OK;
}

// A gspec_ok tree at other constants (srhip_internal.h gspec_ok): nd are its nodes holding them, c the
// same values in get_constants order.  `out` becomes the full compile's metadata (gbase) with the
// value-dependent part recomputed (static_fail, fill_consts: constant leaves' finiteness, constant
// subtrees folded) and code_begin = dst.  Unless the tree now fails statically, the base code stands at
// instruction dst of gcode (copied there when dst is not its own place) with the constant immediates
// rewritten, and [lo, hi) grows by it.  Returns false on a static failure: nothing is written at dst.
template <typename T>
bool rewrite_consts(srhip_program& P, int32_t t, const srhip_node* nd, const double* c, int64_t dst, TreeInfo& out,
                    int64_t& lo, int64_t& hi) {
  const TreeInfo& base = P.gbase[t];
  TreeInfo meta;
  TreeCompiler<T>(nd, P.offsets[t + 1] - P.offsets[t], P, 0, true).static_info(meta);
  out = base;
  out.static_fail = meta.static_fail;
  out.fill_consts = std::move(meta.fill_consts);
  out.code_begin = (int32_t)dst;
  if (out.static_fail) return false;
  if (dst != base.code_begin)
    std::copy(P.gcode.begin() + base.code_begin, P.gcode.begin() + base.code_begin + base.code_len, P.gcode.begin() + dst);
  for (int32_t j = P.gci_off[t]; j < P.gci_off[t + 1]; j += 2)
    P.gcode[(size_t)dst + P.gci[j]].imm = HostVal<T>::bits(HostVal<T>::from(c[P.gci[j + 1]]));
  lo = std::min<int64_t>(lo, dst);
  hi = std::max<int64_t>(hi, dst + base.code_len);
  return true;
}

template <typename T>
bool spec_instantiate_t(srhip_program& P, int32_t slot, int32_t t, const double* c, bool* static_fail, int64_t& lo,
                        int64_t& hi) {
  if (slot < 0 || slot >= P.gspec_alloc || t < 0 || t >= P.ntrees || P.gspec_ok.size() != (size_t)P.ntrees)
    return false;
  TreeInfo& si = P.ginfo[(size_t)P.ntrees + slot];
  const int64_t dst = P.gspec_base + (int64_t)slot * P.gspec_stride;
  // the tree's nodes at the constants c (get_constants order = pre-order over constant leaves)
  const int64_t b = P.offsets[t], e = P.offsets[t + 1];
  std::vector<srhip_node> nd(P.nodes.begin() + b, P.nodes.begin() + e);
  const double* cp = c;
  set_consts(nd.data(), 0, cp);
  if (!P.gspec_ok[t]) {  // the code's shape is not known to be value-independent: compile it
    TreeCompiler<T> tc(nd.data(), e - b, P, 0, true);
    std::vector<Ins> scratch;
    TreeInfo gi;
    if (tc.compile(gi, scratch)) return false;
    *static_fail = gi.static_fail;
    if (!gi.static_fail) {
      if (gi.code_len > P.gspec_stride || (size_t)gi.code_len != scratch.size()) return false;
      std::copy(scratch.begin(), scratch.end(), P.gcode.begin() + dst);
      lo = std::min<int64_t>(lo, dst);
      hi = std::max<int64_t>(hi, dst + gi.code_len);
    }
    si = std::move(gi);
    si.code_begin = (int32_t)dst;
    if (si.static_fail) si.code_len = 1;
    return true;
  }
  // the base code in the slot with the constant immediates rewritten
  if (P.gbase[t].code_len > P.gspec_stride) return false;
  *static_fail = !rewrite_consts<T>(P, t, nd.data(), c, dst, si, lo, hi);
  if (*static_fail) {  // @return_on_check: did_succeed = false, nothing to evaluate: a one-instruction failing entry
    si = TreeInfo();
    si.static_fail = true;
    si.code_begin = (int32_t)dst;
    si.code_len = 1;
  }
  return true;
}

void grad_snapshot(srhip_program& P) {
  P.gsnap.clear();
  P.gsnap_off.assign(P.ntrees + 1, 0);
  for (int32_t t = 0; t < P.ntrees; ++t) {
    for (int64_t i = P.offsets[t]; i < P.offsets[t + 1]; ++i)
      if (P.nodes[(size_t)i].degree == 0 && P.nodes[(size_t)i].constant) P.gsnap.push_back(P.nodes[(size_t)i].val);
    P.gsnap_off[t + 1] = (int64_t)P.gsnap.size();
  }
}

// Recompile in place only the trees whose constant values differ (bitwise) from the snapshot the
// gradient program was compiled with.  A tree's code depends on its own nodes only and is
// position-independent, so an unchanged length means the new code drops into the old slot; any
// other outcome (length change, no snapshot) returns patched = false and the caller recompiles all.
template <typename T>
int patch_grad_t(srhip_program& P, bool& patched, int64_t& lo, int64_t& hi) {
  patched = false;
  lo = INT64_MAX;
  hi = -1;
  const size_t nslots = (size_t)P.ntrees + P.gspec_alloc;
  if (P.gsnap.empty() || P.gprog_off.size() != nslots || P.ginfo.size() != nslots ||
      P.gsnap_off.size() != (size_t)P.ntrees + 1 || (size_t)P.gsnap_off[P.ntrees] != P.gsnap.size() ||
      P.gspec_cap != P.gspec_alloc || P.gspec_ok.size() != (size_t)P.ntrees || P.gci_off.size() != (size_t)P.ntrees + 1)
    return SRHIP_OK;
  std::vector<Ins> scratch;
  std::vector<double> cvals;
  // the trees the optimiser wrote constants of (P.ghint), or all of them
  std::vector<int32_t> all;
  if (P.ghint.empty()) {
    all.resize(P.ntrees);
    for (int32_t t = 0; t < P.ntrees; ++t) all[t] = t;
  }
  const std::vector<int32_t>& scan = P.ghint.empty() ? all : P.ghint;
  for (int32_t t : scan) {
    if (t < 0 || t >= P.ntrees) return SRHIP_OK;
    const int64_t b = P.offsets[t], e = P.offsets[t + 1];
    bool dirty = false;
    int64_t k = P.gsnap_off[t];
    for (int64_t i = b; i < e; ++i) {
      const srhip_node& n = P.nodes[(size_t)i];
      if (n.degree != 0 || !n.constant) continue;
      if (k >= P.gsnap_off[t + 1]) return SRHIP_OK;
      dirty |= memcmp(&n.val, &P.gsnap[k], sizeof(double)) != 0;
      P.gsnap[k++] = n.val;  // the snapshot follows the patch (this tree recompiles below if dirty)
    }
    if (!dirty) continue;
    if ((size_t)t < P.gspec_ok.size() && P.gspec_ok[t]) {
      // the code is the full compile's with new constant immediates; the did_succeed metadata is
      // recomputed from the new values (constant leaves' finiteness, constant subtrees folded)
      cvals.resize(P.info[t].nconst);
      double* cv = cvals.data();
      get_consts(P.nodes.data() + b, 0, cv);
      // in its own place; on a static failure the evaluation skips the tree and it keeps its code
      (void)rewrite_consts<T>(P, t, P.nodes.data() + b, cvals.data(), P.gbase[t].code_begin, P.ginfo[t], lo, hi);
      continue;
    }
    scratch.clear();
    TreeCompiler<T> tc(P.nodes.data() + b, e - b, P, 0, true);
    TreeInfo gi;
    int rc = tc.compile(gi, scratch);
    if (rc) return fail(rc, "tree %d (gradient program): %s", (int)t, last_error());
    TreeInfo& old = P.ginfo[t];
    if (gi.static_fail) {
      // a non-finite constant: eval_grad skips the tree, so its slot keeps the last code (and
      // length) and a later finite point patches into the same slot instead of forcing a full
      // recompile of the whole population (trial points of the line search do overflow)
      gi.code_begin = old.code_begin;
      gi.code_len = old.code_len;
      old = std::move(gi);
      continue;
    }
    if (gi.code_len != old.code_len) return SRHIP_OK;
    std::copy(scratch.begin(), scratch.end(), P.gcode.begin() + old.code_begin);
    lo = std::min<int64_t>(lo, old.code_begin);
    hi = std::max<int64_t>(hi, (int64_t)old.code_begin + old.code_len);
    gi.code_begin = old.code_begin;
    old = std::move(gi);
  }
  P.gkmax = 0;
  P.gmax_len = 0;
  P.gmax_ops = 0;
  for (const TreeInfo& gi : P.ginfo) {
    P.gkmax = std::max(P.gkmax, gi.need);
    P.gmax_len = std::max(P.gmax_len, gi.code_len);
    P.gmax_ops = std::max(P.gmax_ops, (int32_t)gi.op_sumcheck.size());
  }
  patched = true;
  return SRHIP_OK;
}

}  // namespace

thread_local double srhip::g_patch_scan_s = 0.0;
bool srhip::spec_instantiate(srhip_program& P, int32_t slot, int32_t t, const double* c, bool* static_fail,
                             int64_t& lo, int64_t& hi) {
  switch (P.dtype) {
    case SRHIP_F32: return spec_instantiate_t<float>(P, slot, t, c, static_fail, lo, hi);
    case SRHIP_F64: return spec_instantiate_t<double>(P, slot, t, c, static_fail, lo, hi);
    default: return false;
  }
}

// the derived columns a constant-gradient program can read: every heavy unary operator applied to a
// feature leaf, distinct (operator, column) pairs in order of first appearance, at most GD_MAX
constexpr size_t GD_MAX = 32;
void srhip::grad_derived_spec(srhip_program& P) {
  if (P.gdspec_done) return;
  P.gdspec_done = true;
  P.gdspec.clear();
  P.gdbase = P.maxfeat;
  for (int32_t t = 0; t < P.ntrees; ++t) {
    const int64_t b = P.offsets[t], e = P.offsets[t + 1];
    for (int64_t i = b; i < e; ++i) {
      const srhip_node& n = P.nodes[i];
      if (n.degree != 1 || n.l < 0 || b + n.l >= e) continue;
      const srhip_node& c = P.nodes[b + n.l];
      if (c.degree != 0 || c.constant || n.op < 1 || n.op > (int)P.unaops.size()) continue;
      const int u = classify_unop(P.unaops[n.op - 1]);
      if (u < 0 || un_grad_inline(u)) continue;
      const uint32_t key = derived_key(u, c.feature);
      if (find_derived(P.gdspec, key) < 0 && P.gdspec.size() < GD_MAX) P.gdspec.push_back(key);
    }
  }
}

int srhip::compile_grad_host(srhip_program& P, GradEdit& edit) {
  edit = GradEdit();
  // a program compiled for the other form (derived columns or not) is compiled again in full
  if (P.grad_ready && P.g_derived != (P.g_want_derived && !P.gdspec.empty())) P.grad_ready = false;
  if (P.grad_ready) return SRHIP_OK;
  const bool same_form = P.g_derived == (P.g_want_derived && !P.gdspec.empty());
  static const bool no_patch = [] { const char* e = getenv("SRHIP_NO_GRAD_PATCH"); return e && *e && *e != '0'; }();
  int rc;
  bool patched = false;
  const double t_patch0 = now_s();
  if (!no_patch && same_form && P.ctx && P.d_gcode.p) {  // a previous full compile is on the device
    switch (P.dtype) {
      case SRHIP_F32: rc = patch_grad_t<float>(P, patched, edit.lo, edit.hi); break;
      case SRHIP_F64: rc = patch_grad_t<double>(P, patched, edit.lo, edit.hi); break;
      default: rc = SRHIP_OK; break;
    }
    g_patch_scan_s += now_s() - t_patch0;
    if (rc) return rc;
  }
  P.ghint.clear();
  if (patched) {  // the device copy differs only in [lo, hi); the snapshot was updated by the patch
    edit.kind = GradEdit::PATCHED;
    return SRHIP_OK;
  }
  switch (P.dtype) {
    case SRHIP_F32: rc = compile_grad_t<float>(P); break;
    case SRHIP_F64: rc = compile_grad_t<double>(P); break;
    default: return fail(SRHIP_ERR_UNSUPPORTED, "constant gradients need a Float32 or Float64 program");
  }
  if (rc) return rc;
  grad_snapshot(P);
  edit.kind = GradEdit::FULL;
  return SRHIP_OK;
}

int srhip::compile_program(srhip_program& P) {
  P.grad_ready = false;
  P.ghint.clear();
  {
    std::lock_guard<std::mutex> g(P.ord_mu);  // costs and live trees change: new schedule
    P.ord_key[0] = P.ord_key[1] = P.ord_key[2] = -1;
    P.ord_goff.clear();
  }
  switch (P.dtype) {
    case SRHIP_F32: return compile_program_t<float>(P);
    case SRHIP_F64: return compile_program_t<double>(P);
    case SRHIP_I32: return compile_program_t<int32_t>(P);
    default: return fail(SRHIP_ERR_INVALID, "bad dtype %d", P.dtype);
  }
}

extern "C" {

int srhip_code_cache_stats(int64_t* hits, int64_t* misses, int64_t* inserts) {
  if (hits) *hits = g_cache_hits.load();
  if (misses) *misses = g_cache_misses.load();
  if (inserts) *inserts = g_cache_inserts.load();
  return SRHIP_OK;
}

// ---- the interpreter's handler ids, by name and by program (no device) -----------------------------
int32_t srhip_isa_handler_count(void) { return (int32_t)H_COUNT; }

int srhip_isa_handler_name(uint32_t h, char* buf, int32_t cap) {
  if (!buf || cap < 1) return fail(SRHIP_ERR_INVALID, "null or empty name buffer");
  if (h >= H_COUNT) return fail(SRHIP_ERR_INVALID, "handler id %u out of range (< %u)", h, H_COUNT);
  static const char* const spec_names[] = {
#define X_(n, f) #n,
      SRHIP_SPEC_BINOPS(X_)
#undef X_
  };
  static const char* const heavy_names[] = {
#define X_(n, f) #n,
      SRHIP_HEAVY_BINOPS(X_)
#undef X_
  };
  static const char* const un_names[] = {
#define X_(n, f) #f,
      SRHIP_UNOPS(X_)
#undef X_
  };
  static const char* const slot_names[] = {"SLOADF", "SLOADC", "PUSH", "PUSHLF", "PUSHLC"};
  static const char* const form_names[] = {"AF", "FA", "AC", "CA"};
  static const char* const leaf_forms[] = {"FF", "FC", "CF"};
  if (h == H_END) snprintf(buf, (size_t)cap, "END");
  else if (h == H_LOADF) snprintf(buf, (size_t)cap, "LOADF");
  else if (h == H_LOADC) snprintf(buf, (size_t)cap, "LOADC");
  else if (h < H_BIN0) snprintf(buf, (size_t)cap, "%s%u", slot_names[(h - H_SLOADF0) / K_MAX], (h - H_SLOADF0) % K_MAX);
  else if (h < H_HEAVY0) {
    const char* op = spec_names[(h - H_BIN0) / SPEC_STRIDE];
    const uint32_t form = (h - H_BIN0) % SPEC_STRIDE;
    if (form < SPEC_SA0) snprintf(buf, (size_t)cap, "%s.%s", op, form_names[form]);
    else if (form < SPEC_AS0) snprintf(buf, (size_t)cap, "%s.SA%u", op, form - SPEC_SA0);
    else if (form < SPEC_FF) snprintf(buf, (size_t)cap, "%s.AS%u", op, form - SPEC_AS0);
    else snprintf(buf, (size_t)cap, "%s.%s", op, leaf_forms[form - SPEC_FF]);
  } else if (h < H_UN0) {
    const char* op = heavy_names[(h - H_HEAVY0) / HEAVY_STRIDE];
    const uint32_t form = (h - H_HEAVY0) % HEAVY_STRIDE;
    snprintf(buf, (size_t)cap, "%s.%s%u", op, form < HEAVY_AS0 ? "SA" : "AS", form % K_MAX);
  } else {
    snprintf(buf, (size_t)cap, "UN.%s", un_names[h - H_UN0]);
  }
  return SRHIP_OK;
}

int srhip_isa_handler_ok(uint32_t h, int dtype) {
  if (h >= H_COUNT || (dtype != SRHIP_F32 && dtype != SRHIP_F64 && dtype != SRHIP_I32)) return -1;
  const bool is_int = dtype == SRHIP_I32;
  if (h < H_BIN0) return 1;
  if (h < H_HEAVY0) return isa_sb_ok(is_int, (int)((h - H_BIN0) / SPEC_STRIDE)) ? 1 : 0;
  if (h < H_UN0) return isa_hb_ok(is_int, (int)((h - H_HEAVY0) / HEAVY_STRIDE)) ? 1 : 0;
  return isa_un_ok(is_int, (int)(h - H_UN0)) ? 1 : 0;
}

int srhip_program_handlers(const srhip_program* P, int32_t tree, int32_t derived, uint32_t* out, int32_t cap,
                           int32_t* count) {
  if (!P || !count) return fail(SRHIP_ERR_INVALID, "null argument");
  if (tree < 0 || tree >= P->ntrees) return fail(SRHIP_ERR_INVALID, "tree %d out of range (%d trees)", (int)tree, (int)P->ntrees);
  const bool der = derived && !P->dspec.empty();
  const std::vector<Ins>& code = der ? P->dcode : P->code;
  size_t i = (size_t)(der ? P->dprog_off[tree] : P->prog_off[tree]);
  int32_t n = 0;
  for (; i < code.size(); ++i, ++n) {
    if (out && n < cap) out[n] = code[i].h;
    if (code[i].h == H_END) {
      ++n;
      break;
    }
  }
  *count = n;
  return SRHIP_OK;
}

}  // extern "C"
