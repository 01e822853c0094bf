// srhip_grad_lossx.hip — constant gradients under a loss given as an expression (srhip_loss_expr): the
// objective of srhip_eval_loss_grad_expr and srhip_optimize_constants_expr.
//
// grad_lossx_kernel is grad_kernel's GMODE_LOSS form (srhip_grad.hip) with another loss stage: the same
// geometry (grad_plan), LDS staging of the row block and dynamic chunk claiming, the same tile body for the
// tree (srhip_grad_tile.inc part 1: values, KT tangents, check statistic M), the same xor levels (part 3) and
// the same slab record [loss, KT gradient sums, M] per (chunk, row block), reduced by launch_grad_reduce.
// In place of part 2, the loss stage (srhip_grad_lossx_stage.inc, included as text here and by
// grad_rowsets_lossx_kernel) runs the expression's register program (LossxProgram, in the kernel
// arguments beside GradArgs) once per tile over dual numbers with one tangent, d / d prediction:
//   LX_LOAD_PRED loads (p, 1); target, weight and constants load with tangent 0;
//   an operator's value is FOps<T>'s and its partials are dual_un / dual_spec / dual_heavy's
//   (srhip_grad_impl.h, the rules the tree's own operators use); a binary operator's tangent is
//   fa * da + fb * db, a unary one's df * da, in T.
// Slot 0 then holds (l, dl) and the rows fold as part 2's do, per row in ascending row order:
//   lacc += (double)l;  gacc[j] += (double)(dl * A[r].d[j]);
// The stage does not multiply by the weight (a weighted loss names it) and its outputs are not folded into
// M: a non-finite l or dl is no failure, did_succeed stays the tree's alone.  KT = 0 runs the primal program
// (the D = false forms of the same functions): the same l bits as with tangents.
#include "srhip_grad_impl.h"
#include "srhip_grad_lossx.h"

namespace srhip {

#ifndef SRHIP_GRAD_WPE
#define SRHIP_GRAD_WPE 0  // srhip_grad.hip's build-level waves-per-SIMD target (0 leaves the allocator free)
#endif

template <typename T, int KT, int K, bool XLDS, int R>
__global__ __launch_bounds__(64 * GRAD_WAVES)
#if SRHIP_GRAD_WPE > 0
__attribute__((amdgpu_waves_per_eu(KT >= 4 ? SRHIP_GRAD_WPE : 1)))
#endif
void grad_lossx_kernel(const GradLossxArgs q) {
  constexpr int GM = GMODE_LOSS;
  constexpr bool DL = KT > 0;  // the loss program carries its tangent
  const GradArgs& p = q.g;
  const int lane = threadIdx.x & 63;
  const int rb = blockIdx.x + p.block0;
  const int64_t row_base = (int64_t)rb * p.rb_rows;
  const int ntiles = p.rb_rows / (64 * R);
  // valid rows of this block, block-relative: the row tests below are 32-bit (scalar for the tile test)
  const int nrel = __builtin_amdgcn_readfirstlane((int)min<int64_t>(max<int64_t>(p.nvalid - row_base, 0), (int64_t)p.rb_rows));
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int group_base = blockIdx.y * p.chunks_per_group;
  const int group_n = min(p.chunks_per_group, p.nchunks - group_base);
  const T* Xg = reinterpret_cast<const T*>(p.X);
  const T* Yg = reinterpret_cast<const T*>(p.y);
  const T* W = reinterpret_cast<const T*>(p.w);
  extern __shared__ __attribute__((aligned(16))) unsigned char grad_lossx_lds[];
  T* xs = reinterpret_cast<T*>(grad_lossx_lds);
  const int rbr = p.rb_rows;
  // chunks are claimed dynamically from an LDS counter, as in grad_kernel (wave w starts with chunk w)
  __shared__ int next_chunk;
  if (threadIdx.x == 0) next_chunk = GRAD_WAVES;
  if constexpr (XLDS) {
    const int nf = p.nfeat;
    const bool has_y = Yg != nullptr;
    for (int i = threadIdx.x; i < (nf + 1) * rbr; i += 64 * GRAD_WAVES) {
      const int f = i / rbr, r = i - f * rbr;
      const int64_t row = row_base + r;
      T v = T(0);
      if (row < p.ld) v = f < nf ? Xg[(int64_t)f * p.ld + row] : (has_y ? Yg[row] : T(0));
      xs[i] = v;
    }
  }
  __syncthreads();
  // feature f / target at block-relative row rr of this row block
  // (a derived view's derived columns, f >= nfeat, are read from global memory)
  auto xat = [&](int f, int rr) -> T {
    if constexpr (XLDS) {
      if (f < p.nfeat) return xs[f * rbr + rr];
    }
    return Xg[(int64_t)f * p.ld + row_base + rr];
  };
  auto yat = [&](int rr) -> T {
    if constexpr (XLDS) return xs[p.nfeat * rbr + rr];
    else return Yg[row_base + rr];
  };
  GIns* code = (GIns*)(uintptr_t)p.code;
  const int max_steps = __builtin_amdgcn_readfirstlane(p.max_steps);
  const int lx_n = __builtin_amdgcn_readfirstlane(min(q.lx.n, LOSSX_MAX_NODES));
  const bool lx_w = q.lx.nargs == 3 && W != nullptr;
  auto claim = [&]() {
    int c = 0;
    if (lane == 0) c = atomicAdd(&next_chunk, 1);
    return __builtin_amdgcn_readfirstlane(c);
  };
  for (int ci = wave; ci < group_n; ci = claim()) {
    const int chunk = group_base + ci;
    int tree, c0;
    if (!p.chunks) {  // the list in the kernel arguments
      tree = __builtin_amdgcn_readfirstlane(p.inl[2 * chunk]);
      c0 = __builtin_amdgcn_readfirstlane(p.inl[2 * chunk + 1]);
    } else {
      tree = __builtin_amdgcn_readfirstlane(p.chunks[2 * chunk]);
      c0 = __builtin_amdgcn_readfirstlane(p.chunks[2 * chunk + 1]);
    }
    if constexpr (KT == 0) {
      if (p.screened) {  // grad_kernel's value-only screening: block 0's record of this chunk decides
        const double m0 = p.slab[(int64_t)chunk * p.nrb * 2 + 1];  // [chunk][block 0][loss, chk]
        if (__builtin_amdgcn_readfirstlane((int)!__builtin_isfinite(m0))) continue;
      }
    }
    const int pc0 = __builtin_amdgcn_readfirstlane(p.prog_off[tree]);
    double lacc = 0.0;
    double gacc[KT > 0 ? KT : 1];
    UNR for (int j = 0; j < KT; ++j) gacc[j] = 0.0;
    T M = T(0);
    for (int tile = 0; tile < ntiles; ++tile) {
      const int tb = tile * 64 * R;  // block-relative first row of the tile
      if (tb >= nrel) break;
      // rows up to ld are finite replicas; masked at the loss
#define SRHIP_GRAD_PART 1
#include "srhip_grad_tile.inc"
#undef SRHIP_GRAD_PART
#define GLX_PROG q.lx
#include "srhip_grad_lossx_stage.inc"
#undef GLX_PROG
    }
    // wave reductions, one slab entry per (chunk, row block)
#define SRHIP_GRAD_PART 3
#include "srhip_grad_tile.inc"
#undef SRHIP_GRAD_PART
    if (lane == 0) {
      double* out = p.slab + ((int64_t)chunk * p.nrb + rb) * (KT + 2);
      out[0] = lacc;
      UNR for (int j = 0; j < KT; ++j) out[1 + j] = gacc[j];
      out[KT + 1] = (double)M;
    }
  }
}

// launch_grad's staging bound and rows per lane (srhip_grad.hip): K is a register budget, R does not change
// a bit of the result
constexpr size_t GLX_LDS_MAX = 48 * 1024;
template <int KT, int K> constexpr int glx_rows() {
  return KT == 0 ? 4 : (KT <= 4 && K <= 2 ? 2 : (KT <= 4 && K <= 4 ? GRAD_R : 1));
}

template <typename T, int KT, int K>
static hipError_t launch_glx_t(const GradLossxArgs& q, dim3 grid, hipStream_t s) {
  constexpr int R = glx_rows<KT, K>();
  if (q.g.rb_rows % (64 * R)) return hipErrorInvalidValue;
  const size_t lds = (size_t)(q.g.nfeat + 1) * (size_t)q.g.rb_rows * sizeof(T);
  if (lds <= GLX_LDS_MAX)
    hipLaunchKernelGGL((grad_lossx_kernel<T, KT, K, true, R>), grid, dim3(64 * GRAD_WAVES), lds, s, q);
  else
    hipLaunchKernelGGL((grad_lossx_kernel<T, KT, K, false, R>), grid, dim3(64 * GRAD_WAVES), 0, s, q);
  return hipGetLastError();
}

template <typename T, int KT> static hipError_t launch_glx_k(int K, const GradLossxArgs& q, dim3 grid, hipStream_t s) {
  if constexpr (sizeof(T) == 8) {  // K = 2 for shallow-stack populations, as launch_grad
    if (K <= 2) return launch_glx_t<T, KT, 2>(q, grid, s);
  }
  return K <= 4 ? launch_glx_t<T, KT, 4>(q, grid, s) : launch_glx_t<T, KT, 8>(q, grid, s);
}

hipError_t launch_grad_lossx(int dtype, int K, int kt, const GradArgs& a, const LossxProgram& lx, dim3 grid,
                             hipStream_t s) {
  if (kt != 0 && kt != 4 && kt != GRAD_KT) return hipErrorInvalidValue;
  if (lx.n < 1 || lx.n > LOSSX_MAX_NODES || lx.dtype != dtype) return hipErrorInvalidValue;
  for (int i = 0; i < lx.n; ++i)  // every slot index the kernel's switches see is one of the eight
    if (lx.ins[i].dst >= LOSSX_MAX_STACK || lx.ins[i].a >= LOSSX_MAX_STACK || lx.ins[i].b >= LOSSX_MAX_STACK)
      return hipErrorInvalidValue;
  GradLossxArgs q{};
  q.g = a;
  q.lx = lx;
  switch (dtype) {
    case SRHIP_F32:
      return kt == 0 ? launch_glx_k<float, 0>(K, q, grid, s)
           : kt == 4 ? launch_glx_k<float, 4>(K, q, grid, s) : launch_glx_k<float, GRAD_KT>(K, q, grid, s);
    case SRHIP_F64:
      return kt == 0 ? launch_glx_k<double, 0>(K, q, grid, s)
           : kt == 4 ? launch_glx_k<double, 4>(K, q, grid, s) : launch_glx_k<double, GRAD_KT>(K, q, grid, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace srhip
