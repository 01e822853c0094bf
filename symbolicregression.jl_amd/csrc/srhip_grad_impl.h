// srhip_grad_impl.h — device side of the dual-number interpreter shared by the constant-gradient kernels
// (srhip_grad.hip: row blocks of one view; srhip_grad_rowsets.hip: one row subset per chunk): operator values
// and partial derivatives, the dual-number type, the check statistic and the exact-bits lane exchange.
// The tile body itself is srhip_grad_tile.inc, included as text by every kernel that runs it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "srhip_grad.h"
#include "srhip_isa.h"
#include "srhip_kernels.h"
#include "srhip_ops.h"

#define UNR _Pragma("unroll")
#ifndef GRAD_R
#define GRAD_R 1  // 2 measured slower on C4 (2.60 -> 2.80 ms: 155 VGPRs, 3 waves per SIMD)
#endif
#define DI __device__ __attribute__((always_inline)) inline

namespace srhip {

#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) Ins GIns;  // bytecode through the scalar cache
#else
typedef const Ins GIns;
#endif

template <typename T> struct V2 { typedef T type __attribute__((ext_vector_type(2))); };
template <typename T> struct V4 { typedef T type __attribute__((ext_vector_type(4))); };

// ---- operator values and partial derivatives ------------------------------------------------
template <int U> constexpr bool dun_inline() { return un_grad_inline(U); }

// f(x) and f'(x) for a heavy unary operator U; D = false: the value alone (value-only passes: the
// derivative of cos is a sin, of log a division -- out of line the compiler cannot drop them), the
// same f.  Out of line per (T, U, D) (dual_un_heavy), and for value-only passes once per R rows
// (dual_un_heavy_rows: one call per node and tile instead of R, the same body per row)
template <typename T, int U, bool D> DI typename V2<T>::type dual_un_body(T x) {
  using O = FOps<T>;
  T f = T(0), df = T(0);
  switch (U) {
    case UN_COS:
      if constexpr (D && sizeof(T) == 8) {  // one Float64 reduction for both (srm_sincos: the same bits)
        double sn, cs;
        srm_sincos(x, &sn, &cs);
        f = cs;
        df = -sn;
      } else {
        f = O::cos(x);
        if constexpr (D) df = -O::sin(x);
      }
      break;
    case UN_SIN:
      if constexpr (D && sizeof(T) == 8) {
        double sn, cs;
        srm_sincos(x, &sn, &cs);
        f = sn;
        df = cs;
      } else {
        f = O::sin(x);
        if constexpr (D) df = O::cos(x);
      }
      break;
    case UN_TAN: f = O::tan(x); if constexpr (D) df = T(1) + f * f; break;
    case UN_EXP: f = O::exp(x); if constexpr (D) df = f; break;
    case UN_LOG: f = O::log(x); if constexpr (D) df = T(1) / x; break;
    case UN_LOG2: f = O::log2(x); if constexpr (D) df = T(1) / (x * T(0.69314718055994530942)); break;
    case UN_LOG10: f = O::log10(x); if constexpr (D) df = T(1) / (x * T(2.30258509299404568402)); break;
    case UN_LOG1P: f = O::log1p(x); if constexpr (D) df = T(1) / (T(1) + x); break;
    case UN_SQRT: f = O::sqrt(x); if constexpr (D) df = T(0.5) / f; break;
    case UN_ACOSH: f = O::acosh(x); if constexpr (D) df = T(1) / m_sqrt(x * x - T(1)); break;
    case UN_ATANH_CLIP: {
      f = O::atanh_clip(x);
      if constexpr (D) {
        const T u = O::mod(x + T(1), T(2)) - T(1);
        df = T(1) / (T(1) - u * u);
      }
      break;
    }
    case UN_SINH: f = O::sinh(x); if constexpr (D) df = O::cosh(x); break;
    case UN_COSH: f = O::cosh(x); if constexpr (D) df = O::sinh(x); break;
    case UN_TANH: f = O::tanh(x); if constexpr (D) df = T(1) - f * f; break;
    case UN_ASIN: f = O::asin(x); if constexpr (D) df = T(1) / m_sqrt(T(1) - x * x); break;
    case UN_ACOS: f = O::acos(x); if constexpr (D) df = -T(1) / m_sqrt(T(1) - x * x); break;
    case UN_ATAN: f = O::atan(x); if constexpr (D) df = T(1) / (T(1) + x * x); break;
    case UN_ASINH: f = O::asinh(x); if constexpr (D) df = T(1) / m_sqrt(x * x + T(1)); break;
    case UN_ERF: f = O::erf(x); if constexpr (D) df = T(1.12837916709551257390) * O::exp(-x * x); break;
    case UN_ERFC: f = O::erfc(x); if constexpr (D) df = -T(1.12837916709551257390) * O::exp(-x * x); break;
    case UN_GAMMA: f = O::gamma(x); if constexpr (D) df = FP<T>::nan(); break;  // no digamma: no gradient (optimizer keeps c)
    case UN_EXP2: f = O::exp2(x); if constexpr (D) df = f * T(0.69314718055994530942); break;
    case UN_EXPM1: f = O::expm1(x); if constexpr (D) df = f + T(1); break;
    case UN_CBRT: f = O::cbrt(x); if constexpr (D) df = T(1) / (T(3) * f * f); break;
    default: f = FP<T>::nan(); df = FP<T>::nan(); break;
  }
  typename V2<T>::type r;
  r[0] = f;
  r[1] = df;
  return r;
}
template <typename T, int U, bool D> __device__ __attribute__((noinline)) typename V2<T>::type dual_un_heavy(T x) {
  return dual_un_body<T, U, D>(x);
}
template <typename T, int R> struct VR { typedef T type __attribute__((ext_vector_type(R))); };
template <typename T> struct VR<T, 1> { typedef T type; };
#ifndef GRAD_ROWS_FENCE
#define GRAD_ROWS_FENCE 1  // rows of dual_un_heavy_rows one after another (no interleaving)
#endif
template <typename T, int U, int R>
__device__ __attribute__((noinline)) typename VR<T, R>::type dual_un_heavy_rows(typename VR<T, R>::type x) {
  if constexpr (R == 1) {
    return dual_un_body<T, U, false>(x)[0];
  } else {
    UNR for (int r = 0; r < R; ++r) {
      x[r] = dual_un_body<T, U, false>(x[r])[0];
      if (GRAD_ROWS_FENCE) __builtin_amdgcn_sched_barrier(0);
    }
    return x;
  }
}

template <typename T, int U, bool D = true> DI void dual_un(T x, T& f, T& df) {
  using O = FOps<T>;
  if constexpr (dun_inline<U>()) {
    switch (U) {
      case UN_NEG: f = O::neg(x); df = T(-1); break;
      case UN_SQUARE: f = O::square(x); df = T(2) * x; break;
      case UN_CUBE: f = O::cube(x); df = T(3) * x * x; break;
      case UN_ABS: f = O::abs(x); df = x > T(0) ? T(1) : (x < T(0) ? T(-1) : T(0)); break;
      case UN_RELU: f = O::relu(x); df = x > T(0) ? T(1) : T(0); break;
      case UN_SIGN: f = O::sign(x); df = T(0); break;
      case UN_ROUND: f = O::round(x); df = T(0); break;
      case UN_FLOOR: f = O::floor(x); df = T(0); break;
      case UN_CEIL: f = O::ceil(x); df = T(0); break;
      default: break;
    }
  } else {
    const typename V2<T>::type r = dual_un_heavy<T, U, D>(x);
    f = r[0];
    df = r[1];
  }
}

// f(a, b), df/da, df/db for a specialised (cheap) binary operator SB
template <typename T, int SB> DI void dual_spec(T a, T b, T& f, T& fa, T& fb) {
  using O = FOps<T>;
  switch (SB) {
    case SB_ADD: f = O::add(a, b); fa = T(1); fb = T(1); break;
    case SB_SUB: f = O::sub(a, b); fa = T(1); fb = T(-1); break;
    case SB_MUL: f = O::mul(a, b); fa = b; fb = a; break;
    case SB_DIV: { f = O::div(a, b); const T ib = T(1) / b; fa = ib; fb = -f * ib; break; }
    case SB_GREATER: f = O::greater(a, b); fa = T(0); fb = T(0); break;
    case SB_COND: f = O::cond(a, b); fa = T(0); fb = a > T(0) ? T(1) : T(0); break;
    case SB_LOGICAL_OR: f = O::logical_or(a, b); fa = T(0); fb = T(0); break;
    case SB_LOGICAL_AND: f = O::logical_and(a, b); fa = T(0); fb = T(0); break;
    case SB_MAX: f = O::max(a, b); fa = a > b ? T(1) : T(0); fb = a > b ? T(0) : T(1); break;
    case SB_MIN: f = O::min(a, b); fa = a < b ? T(1) : T(0); fb = a < b ? T(0) : T(1); break;
    default: f = FP<T>::nan(); fa = f; fb = f; break;
  }
}

// heavy binary (pow, mod, atan2): out of line; returns (f, df/da, df/db, -)
template <typename T, int HB, bool D> __device__ __attribute__((noinline)) typename V4<T>::type dual_heavy(T a, T b) {
  using O = FOps<T>;
  T f, fa = T(0), fb = T(0);
  switch (HB) {
    case HB_POW:
      f = O::pow(a, b);
      if constexpr (D) {
        fa = b * O::pow(a, b - T(1));
        fb = a > T(0) ? f * m_log(a) : T(0);
      }
      break;
    case HB_MOD: f = O::mod(a, b); if constexpr (D) { fa = T(1); fb = -m_floor(a / b); } break;
    case HB_ATAN2: {
      f = O::atan2(a, b);
      if constexpr (D) { const T r = T(1) / (a * a + b * b); fa = b * r; fb = -a * r; }
      break;
    }
    default: f = FP<T>::nan(); fa = f; fb = f; break;
  }
  typename V4<T>::type r;
  r[0] = f;
  r[1] = fa;
  r[2] = fb;
  r[3] = T(0);
  return r;
}

// d loss / d prediction for the distance losses of srhip_ops.h loss_elem (diff = pred - y)
template <typename T> DI T dloss_elem(int kind, T d, T p0) {
  const T sg = d > T(0) ? T(1) : (d < T(0) ? T(-1) : T(0));
  switch (kind) {
    case SRHIP_LOSS_L2: return T(2) * d;
    case SRHIP_LOSS_L1: return sg;
    case SRHIP_LOSS_LP: return p0 * m_pow(m_abs(d), p0 - T(1)) * sg;
    case SRHIP_LOSS_HUBER: return m_abs(d) <= p0 ? d : p0 * sg;
    case SRHIP_LOSS_L1_EPS_INS: return m_abs(d) > p0 ? sg : T(0);
    case SRHIP_LOSS_L2_EPS_INS: return T(2) * m_max(T(0), m_abs(d) - p0) * sg;
    case SRHIP_LOSS_LOGIT_DIST: { const T e = m_exp(d); return (e - T(1)) / (e + T(1)); }
    case SRHIP_LOSS_PERIODIC: {
      const T k = T(2) * T(3.14159265358979323846) / p0;
      return k * m_sin(d * k);
    }
    case SRHIP_LOSS_QUANTILE: return p0 - (d < T(0) ? T(1) : T(0));
    default: return FP<T>::nan();
  }
}

// (loss, d loss / d output) of the other distance losses, out of line: inline, their math bodies
// raised the kernel's register count for every loss kind
// d loss / d agreement of the margin losses of srhip_ops.h margin_loss (a = target * output)
template <typename T> DI T dmargin(int kind, T a, T p0) {
  switch (kind) {
    case SRHIP_LOSS_ZERO_ONE: return T(0);
    case SRHIP_LOSS_PERCEPTRON: return a >= T(0) ? T(0) : T(-1);
    case SRHIP_LOSS_LOGIT_MARGIN: return T(-1) / (T(1) + m_exp(a));
    case SRHIP_LOSS_L1_HINGE: return a >= T(1) ? T(0) : T(-1);
    case SRHIP_LOSS_L2_HINGE: return a >= T(1) ? T(0) : T(2) * (a - T(1));
    case SRHIP_LOSS_SMOOTHED_L1_HINGE: return a >= T(1) - p0 ? (a >= T(1) ? T(0) : (a - T(1)) / p0) : T(-1);
    case SRHIP_LOSS_MODIFIED_HUBER: return a >= T(-1) ? (a > T(1) ? T(0) : T(2) * a - T(2)) : T(-4);
    case SRHIP_LOSS_L2_MARGIN: return T(2) * (a - T(1));
    case SRHIP_LOSS_EXP: return -m_exp(-a);
    case SRHIP_LOSS_SIGMOID: { const T t = m_tanh(a); return -(T(1) - t * t); }
    case SRHIP_LOSS_DWD_MARGIN:
      return a <= p0 / (p0 + T(1)) ? T(-1) : -m_pow(p0 / (p0 + T(1)), p0 + T(1)) / m_pow(a, p0 + T(1));
    default: return FP<T>::nan();
  }
}
// (loss, d loss / d output) of one row for the kinds other than L2: distance losses of
// output - target, margin losses of target * output (chain rule: target * dL/da)
template <typename T>
__device__ __attribute__((noinline)) typename V2<T>::type loss_dloss_generic(int kind, T out, T y, T p0) {
  if (loss_is_margin(kind)) {
    const T a = y * out;
    return typename V2<T>::type{margin_loss<T>(kind, a, p0), y * dmargin<T>(kind, a, p0)};
  }
  const T d = out - y;
  return typename V2<T>::type{loss_elem<T>(kind, d, p0), dloss_elem<T>(kind, d, p0)};
}

// ---- the dual-number interpreter ----------------------------------------------------------------
template <typename T> DI T imm_bits(uint64_t b) {
  if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, b);
  else return __builtin_bit_cast(T, (uint32_t)b);
}

// KT = 0: values only (the line search's trial points): the primal code and its row-sum order are
// the same as with tangents, so a value-only loss is bit-identical to the loss of a gradient launch
template <typename T, int KT> struct Dual {
  T v;
  T d[KT > 0 ? KT : 1];
};

// leaves: tangents are seeded on the constants (GMODE_LOSS / GMODE_ROWC: rel = constant index - c0)
// or on the features (GMODE_ROWF: rel = feature index - c0)
template <int GM, typename T, int KT> DI void set_const(Dual<T, KT>& a, T c, int rel) {
  a.v = c;
  UNR for (int j = 0; j < KT; ++j) a.d[j] = (GM != GMODE_ROWF && rel == j) ? T(1) : T(0);
}
template <int GM, typename T, int KT> DI void set_feat(Dual<T, KT>& a, T x, int rel) {
  a.v = x;
  UNR for (int j = 0; j < KT; ++j) a.d[j] = (GM == GMODE_ROWF && rel == j) ? T(1) : T(0);
}
// out = f(l, r) with partials: out.d = fl * l.d + fr * r.d (out may alias l or r)
template <typename T, int KT>
DI void combine(Dual<T, KT>& out, const Dual<T, KT>& l, const Dual<T, KT>& r, T f, T fl, T fr) {
  T d[KT > 0 ? KT : 1];
  UNR for (int j = 0; j < KT; ++j) d[j] = fl * l.d[j] + fr * r.d[j];
  out.v = f;
  UNR for (int j = 0; j < KT; ++j) out.d[j] = d[j];
}

// check statistic, as in the evaluator: max |v| (Float32, NaN-propagating) / sum |v| 2^-512 (Float64)
DI void chk_fold(float& M, float v) { M = __builtin_elementwise_maximum(M, __builtin_fabsf(v)); }
DI void chk_fold(double& M, double v) { M = __builtin_fma(__builtin_fabs(v), 0x1p-512, M); }

// XLDS: the workgroup stages its row block of X (and y) into LDS once -- feature leaves then read
// LDS instead of issuing a dependent global load per leaf per tile (grad_lds_bytes: [nfeat + 1][rb_rows])
// R rows per lane: a tile is 64 R rows (row tile_base + 64 r + lane), one bytecode dispatch per tile.
// Every lane still folds its rows in ascending row order (tile-major, r inner), so losses and
// gradients are bit-identical for any R.
// The value of lane (lane ^ O) for the xor butterflies of the per-(chunk, row block) sums: DPP for
// O <= 8 (quad permutes; half-row / row mirrors composed with them), ds_swizzle for 16, ds_bpermute
// for 32 -- the partner's exact bits, so every sum is the one __shfl_xor gave, with four of the six
// levels off the LDS crossbar's latency.
template <int O> DI uint32_t xor_lane_u32(uint32_t v, int lane) {
  if constexpr (O == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);  // quad [1,0,3,2]
  else if constexpr (O == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);  // quad [2,3,0,1]
  else if constexpr (O == 4)  // half-row mirror (i ^ 7), then quad mirror (^ 3)
    return (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false), 0x1B, 0xF, 0xF, false);
  else if constexpr (O == 8)  // row mirror (i ^ 15), then half-row mirror (^ 7)
    return (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, false), 0x141, 0xF, 0xF, false);
  else if constexpr (O == 16)  // bitmask swizzle within 32 lanes: and 0x1f, or 0, xor 0x10
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);
  else
    return (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ O) << 2, (int)v);
}
template <int O> DI double xor_lane(double x, int lane) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const uint64_t r = (uint64_t)xor_lane_u32<O>((uint32_t)b, lane) | ((uint64_t)xor_lane_u32<O>((uint32_t)(b >> 32), lane) << 32);
  return __builtin_bit_cast(double, r);
}
template <int O> DI float xor_lane(float x, int lane) {
  return __builtin_bit_cast(float, xor_lane_u32<O>(__builtin_bit_cast(uint32_t, x), lane));
}

}  // namespace srhip
