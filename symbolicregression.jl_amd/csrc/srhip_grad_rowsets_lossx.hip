// srhip_grad_rowsets_lossx.hip — loss and constant gradients of many (program slot, row subset) pairs in one
// launch under a loss given as an expression: the objective of srhip_eval_loss_grad_expr_rowsets and
// srhip_optimize_constants_expr_rowsets.
//
// grad_rowsets_lossx_kernel is grad_rowsets_kernel (srhip_grad_rowsets.hip) with grad_lossx_kernel's loss
// stage in place of tile part 2.  From the former: one wavefront per chunk (slot, c0, set), the LDS copy of
// the set's packed columns, the 256-row block walk, parts 1 and 3 of srhip_grad_tile.inc, block b's record
// kept by lane b, grad_reduce_kernel's fold and the final (kt + 2) record in coherent host memory.  From the
// latter (srhip_grad_lossx_stage.inc, the same text): the stack zeroed at the stage's head, the expression's
// register program over dual numbers with one tangent, the fold
//   lacc += (double)l;  gacc[j] += (double)(dl * A[r].d[j]);   (the product in T)
// with no weight multiply and nothing folded into M.
// So a chunk's record has the bits of grad_lossx_kernel + grad_reduce_kernel over a view gathered from the
// set: the same rows per lane in the same order, the same block records, the same fold.
#include "srhip_grad_impl.h"
#include "srhip_grad_lossx.h"
#include "srhip_kernels.h"

namespace srhip {

template <typename T, int KT, int K, int R>
__global__ __launch_bounds__(64) void grad_rowsets_lossx_kernel(const GradRowsetLossxArgs q) {
  constexpr int GM = GMODE_LOSS;
  constexpr int RB = GRAD_ROWSET_RB;
  constexpr bool DL = KT > 0;  // the loss program carries its tangent
  const GradRowsetArgs& p = q.g;
  extern __shared__ __attribute__((aligned(16))) unsigned char grad_rsx_lds[];
  T* const region = reinterpret_cast<T*>(grad_rsx_lds);
  const int lane = (int)threadIdx.x;
  const int chunk = (int)blockIdx.x;
  const int slot = __builtin_amdgcn_readfirstlane(p.chunks[3 * chunk]);
  const int c0 = __builtin_amdgcn_readfirstlane(p.chunks[3 * chunk + 1]);
  const int set = __builtin_amdgcn_readfirstlane(p.chunks[3 * chunk + 2]);
  const int m = __builtin_amdgcn_readfirstlane(p.set_m[set]);  // 1 .. cap (host-checked)
  const int nb = (m + RB - 1) / RB;                             // row blocks of this set (<= 64)
  const int rbr = nb * RB;                                      // ld_t: the region's column stride
  const int ncol = p.nfeat + 1 + (p.weighted ? 1 : 0);
  // ---- 1. the set's packed columns into the wave's region (ncol * rbr elements: whole 16-byte units) ----
  {
    const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(p.packed) + p.set_off[set]);
    uint4* dst = reinterpret_cast<uint4*>(grad_rsx_lds);
    const int n16 = ncol * rbr * (int)sizeof(T) / 16;
    for (int i = lane; i < n16; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  const T* Xg = region;  // (the tile body's derived-column reads: never taken, gd_nd = 0)
  const int64_t row_base = 0;
  GIns* code = (GIns*)(uintptr_t)p.code;
  const int max_steps = __builtin_amdgcn_readfirstlane(p.max_steps);
  const int pc0 = __builtin_amdgcn_readfirstlane(p.prog_off[slot]);
  const int lx_n = __builtin_amdgcn_readfirstlane(min(q.lx.n, LOSSX_MAX_NODES));
  const bool lx_w = q.lx.nargs == 3 && p.weighted != 0;
  constexpr int ntiles = RB / (64 * R);
  // block b's record, kept by lane b
  double rec_l = 0.0, rec_g[KT > 0 ? KT : 1], rec_m = 0.0;
  UNR for (int j = 0; j < KT; ++j) rec_g[j] = 0.0;
  for (int b = 0; b < nb; ++b) {
    const T* xs = region + b * RB;                     // block-relative rows of every column
    const T* W = region + (p.nfeat + 1) * rbr + b * RB;  // (read only where lx_w: the weight column exists)
    const int nrel = min(m - b * RB, RB);              // valid rows of this block
    auto xat = [&](int f, int rr) -> T { return xs[f * rbr + rr]; };
    auto yat = [&](int rr) -> T { return xs[p.nfeat * rbr + rr]; };
    double lacc = 0.0;
    double gacc[KT > 0 ? KT : 1];
    UNR for (int j = 0; j < KT; ++j) gacc[j] = 0.0;
    T M = T(0);
    for (int tile = 0; tile < ntiles; ++tile) {
      const int tb = tile * 64 * R;
      if (tb >= nrel) break;
#define SRHIP_GRAD_PART 1
#include "srhip_grad_tile.inc"
#undef SRHIP_GRAD_PART
#define GLX_PROG q.lx
#include "srhip_grad_lossx_stage.inc"
#undef GLX_PROG
    }
#define SRHIP_GRAD_PART 3
#include "srhip_grad_tile.inc"
#undef SRHIP_GRAD_PART
    if (lane == b) {  // every lane holds the block's sums after the butterfly: lane b keeps them
      rec_l = lacc;
      UNR for (int j = 0; j < KT; ++j) rec_g[j] = gacc[j];
      rec_m = (double)M;
    }
  }
  // ---- 3. grad_reduce_kernel's fold over the set's blocks ----
  auto fold = [&](double v, bool is_max) -> double {
    double s = 0.0;
    if (lane < nb) s = is_max ? __builtin_elementwise_maximum(s, v) : s + v;
    UNR for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_xor(s, o);
      s = is_max ? __builtin_elementwise_maximum(s, t) : s + t;
    }
    return s;
  };
  double* out = p.out + (int64_t)chunk * (KT + 2);
  const double r0 = fold(rec_l, false);
  if (lane == 0) out[0] = r0;
  UNR for (int j = 0; j < KT; ++j) {
    const double rj = fold(rec_g[j], false);
    if (lane == 0) out[1 + j] = rj;
  }
  const double rm = fold(rec_m, sizeof(T) == 4);
  if (lane == 0) out[KT + 1] = rm;
}

template <typename T, int KT>
static hipError_t launch_grx_t(const GradRowsetLossxArgs& q, size_t lds, hipStream_t s) {
  constexpr int R = KT == 0 ? 4 : 1;  // launch_grad_rowsets_t's rows per lane (K = 8): R changes no bit
  auto kern = grad_rowsets_lossx_kernel<T, KT, 8, R>;
  hipLaunchKernelGGL(kern, dim3(q.g.nchunks), dim3(64), lds, s, q);
  return hipGetLastError();
}

hipError_t launch_grad_rowsets_lossx(int dtype, int kt, const GradRowsetArgs& a, const LossxProgram& lx, int max_ld,
                                     hipStream_t s) {
  if (a.nchunks <= 0) return hipSuccess;
  if (kt != 0 && kt != 4 && kt != GRAD_KT) return hipErrorInvalidValue;
  if (lx.n < 1 || lx.n > LOSSX_MAX_NODES || lx.dtype != dtype) return hipErrorInvalidValue;
  for (int i = 0; i < lx.n; ++i)  // every slot index the kernel's switches see is one of the eight
    if (lx.ins[i].dst >= LOSSX_MAX_STACK || lx.ins[i].a >= LOSSX_MAX_STACK || lx.ins[i].b >= LOSSX_MAX_STACK)
      return hipErrorInvalidValue;
  const size_t es = dtype == SRHIP_F64 ? 8 : 4;
  const size_t lds = (size_t)(a.nfeat + 1 + (a.weighted ? 1 : 0)) * (size_t)max_ld * es;
  if (max_ld <= 0 || max_ld % GRAD_ROWSET_RB != 0 || lds > (size_t)ROWSET_LDS_BUDGET || a.gd_nd != 0)
    return hipErrorInvalidValue;
  GradRowsetLossxArgs q{};
  q.g = a;
  q.lx = lx;
  switch (dtype) {
    case SRHIP_F32:
      return kt == 0 ? launch_grx_t<float, 0>(q, lds, s)
           : kt == 4 ? launch_grx_t<float, 4>(q, lds, s) : launch_grx_t<float, GRAD_KT>(q, lds, s);
    case SRHIP_F64:
      return kt == 0 ? launch_grx_t<double, 0>(q, lds, s)
           : kt == 4 ? launch_grx_t<double, 4>(q, lds, s) : launch_grx_t<double, GRAD_KT>(q, lds, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace srhip
