// srhip_grad_rowsets.hip — loss and constant gradients of many (program slot, row subset) pairs in one
// launch: the batching mode's per-member minibatch of optimize_constants (reference:
// src/ConstantOptimization.jl:14-17 batch_sample per member, :48 / :72 the member's idx in its objective).
//
// One wavefront owns one chunk = (program slot, first constant c0, tree whose set it reads).  Workgroups
// are single waves, one per chunk (grid.x = chunks, in descending set length x tree cost), so the
// hardware's workgroup dispatcher is the claim counter, as in rowsets_kernel.  The wave
//   1. copies its set's packed columns (features, y, w; [column][ld_t], ld_t = the set's length rounded
//      up to whole 256-row blocks, padded with replicas of the last row) from the call's packed buffer
//      into its own LDS region with 16-byte coalesced reads -- the sets were gathered by index once, at
//      the start of the call (grad_rowsets_pack_kernel), not on every launch;
//   2. walks the set in the 256-row blocks grad_plan fixes for the single-view kernel, running the same
//      tile body (srhip_grad_tile.inc, included as text) with the same rows per lane: lanes fold their
//      rows in ascending order, and each block's record is formed by the same six xor levels -- the
//      (chunk, row block) slab entry grad_kernel writes;
//   3. combines the block records in grad_reduce_kernel's order: block b's record sits in lane b, 0.0 in
//      the lanes that hold no block (it matters for -0.0), the xor butterfly 32 .. 1, the check statistic
//      by max (Float32) or sum (Float64); lane 0 writes the final (kt + 2) record to coherent host memory.
// So a chunk's record has the bits the single-view path (grad_kernel + grad_reduce_kernel over a view
// gathered from the set) produces, with no slab and no reduce launch.
//
// The derived view (columns of U(feature)) is off below 8192 rows, far above any set a wave can stage:
// gradient programs evaluated here are compiled without derived columns.
//
// Variants: tangent widths 0 (value-only trial points), 4 and 8 as launch_grad; the stack depth is always
// K = 8 (it holds every program; bits do not depend on K or on the rows per lane).  The launch is bound by
// latency, not occupancy: one wave per chunk, at most a few hundred chunks in flight.
#include "srhip_grad_impl.h"
#include "srhip_kernels.h"

namespace srhip {

template <typename T, int KT, int K, int R>
__global__ __launch_bounds__(64) void grad_rowsets_kernel(GradRowsetArgs p) {
  constexpr int GM = GMODE_LOSS;
  constexpr int RB = GRAD_ROWSET_RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char grad_rs_lds[];
  T* const region = reinterpret_cast<T*>(grad_rs_lds);
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
    uint4* dst = reinterpret_cast<uint4*>(grad_rs_lds);
    const int n16 = ncol * rbr * (int)sizeof(T) / 16;
    for (int i = lane; i < n16; i += 64) dst[i] = src[i];
  }
  __syncthreads();
  const T* Xg = region;  // (the tile body's derived-column reads: never taken, gd_nd = 0)
  const int64_t row_base = 0;
  GIns* code = (GIns*)(uintptr_t)p.code;
  const T p0 = (T)p.loss_p0;
  const int max_steps = __builtin_amdgcn_readfirstlane(p.max_steps);
  const int pc0 = __builtin_amdgcn_readfirstlane(p.prog_off[slot]);
  constexpr int ntiles = RB / (64 * R);
  // block b's record, kept by lane b
  double rec_l = 0.0, rec_g[KT > 0 ? KT : 1], rec_m = 0.0;
  UNR for (int j = 0; j < KT; ++j) rec_g[j] = 0.0;
  for (int b = 0; b < nb; ++b) {
    const T* xs = region + b * RB;                     // block-relative rows of every column
    const T* W = region + (p.nfeat + 1) * rbr + b * RB;
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
#define SRHIP_GRAD_PART 2
#include "srhip_grad_tile.inc"
#undef SRHIP_GRAD_PART
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

// The call's pack: workgroup t gathers set t by index, [column][ld_t], gather_kernel's padding rule
// (positions past the set's end replicate its last row, with the padding weight -0.0).  set_off[t] < 0: not packed
// (a set no wave can stage).
template <typename T>
__global__ __launch_bounds__(256) void grad_rowsets_pack_kernel(const T* __restrict__ X, const T* __restrict__ y,
                                                                const T* __restrict__ w, int64_t src_ld, int nfeat,
                                                                const int64_t* __restrict__ row_off,
                                                                const int64_t* __restrict__ rows,
                                                                const int64_t* __restrict__ set_off, T* __restrict__ packed) {
  const int t = (int)blockIdx.x;
  const int64_t off = set_off[t];
  if (off < 0) return;
  const int64_t r0 = row_off[t];
  const int m = (int)(row_off[t + 1] - r0);
  const int ld = (m + GRAD_ROWSET_RB - 1) / GRAD_ROWSET_RB * GRAD_ROWSET_RB;
  T* dst = packed + off;
  for (int pos = (int)threadIdx.x; pos < ld; pos += (int)blockDim.x) {
    const int64_t j = rows[r0 + min(pos, m - 1)];  // in [0, n): checked on the host
    for (int f = 0; f < nfeat; ++f) dst[(int64_t)f * ld + pos] = X[(int64_t)f * src_ld + j];
    dst[(int64_t)nfeat * ld + pos] = y[j];
    if (w) dst[(int64_t)(nfeat + 1) * ld + pos] = pos < m ? w[j] : pad_weight<T>();
  }
}

int grad_rowset_cap(int dtype, int64_t nfeat, bool weighted) {
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) return 0;
  // never above the evaluation's cap, so the baseline's per-set statistics cover every staged set
  return std::min(rowset_cap(dtype, nfeat, weighted), 64 * GRAD_ROWSET_RB) / GRAD_ROWSET_RB * GRAD_ROWSET_RB;
}

template <typename T, int KT>
static hipError_t launch_grad_rowsets_t(const GradRowsetArgs& a, size_t lds, hipStream_t s) {
  constexpr int R = KT == 0 ? 4 : 1;  // launch_grad's rows per lane at K = 8
  auto kern = grad_rowsets_kernel<T, KT, 8, R>;
  hipLaunchKernelGGL(kern, dim3(a.nchunks), dim3(64), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_grad_rowsets(int dtype, int kt, const GradRowsetArgs& a, int max_ld, hipStream_t s) {
  if (a.nchunks <= 0) return hipSuccess;
  if (kt != 0 && kt != 4 && kt != GRAD_KT) return hipErrorInvalidValue;
  const size_t es = dtype == SRHIP_F64 ? 8 : 4;
  const size_t lds = (size_t)(a.nfeat + 1 + (a.weighted ? 1 : 0)) * (size_t)max_ld * es;
  if (max_ld <= 0 || max_ld % GRAD_ROWSET_RB != 0 || lds > (size_t)ROWSET_LDS_BUDGET || a.gd_nd != 0)
    return hipErrorInvalidValue;
  switch (dtype) {
    case SRHIP_F32:
      return kt == 0 ? launch_grad_rowsets_t<float, 0>(a, lds, s)
           : kt == 4 ? launch_grad_rowsets_t<float, 4>(a, lds, s) : launch_grad_rowsets_t<float, GRAD_KT>(a, lds, s);
    case SRHIP_F64:
      return kt == 0 ? launch_grad_rowsets_t<double, 0>(a, lds, s)
           : kt == 4 ? launch_grad_rowsets_t<double, 4>(a, lds, s) : launch_grad_rowsets_t<double, GRAD_KT>(a, lds, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_grad_rowsets_pack(int dtype, const void* X, const void* y, const void* w, int64_t src_ld, int nfeat,
                                    const int64_t* row_off, const int64_t* rows, const int64_t* set_off, int ntrees,
                                    void* packed, hipStream_t s) {
  if (ntrees <= 0) return hipSuccess;
  if (dtype == SRHIP_F64)
    hipLaunchKernelGGL(grad_rowsets_pack_kernel<double>, dim3(ntrees), dim3(256), 0, s, (const double*)X, (const double*)y,
                       (const double*)w, src_ld, nfeat, row_off, rows, set_off, (double*)packed);
  else if (dtype == SRHIP_F32)
    hipLaunchKernelGGL(grad_rowsets_pack_kernel<float>, dim3(ntrees), dim3(256), 0, s, (const float*)X, (const float*)y,
                       (const float*)w, src_ld, nfeat, row_off, rows, set_off, (float*)packed);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace srhip
