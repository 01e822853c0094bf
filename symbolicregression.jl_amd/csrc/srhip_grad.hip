// srhip_grad.hip — batched forward-mode (dual-number) constant gradients for the constant optimizer.
//
// Replaces (reference): the objective of _optimize_constants (src/ConstantOptimization.jl:43-81),
// f(c) = eval_loss(tree(c), dataset, options; regularization=false), whose gradient Optim obtains
// by finite differences (no g! is passed, :50).  Here one launch returns, for every tree, the loss
// and its exact gradient with respect to the tree's constants (get_constants order,
// test/test_derivatives.jl:123-147), by carrying KT tangent components per value through the
// same bytecode interpreter as the evaluator (the "gradient program": constants not folded, each
// constant leaf tagged with its index).  A "chunk" is (tree, first constant c0): trees with more
// than KT constants take several chunks.  One lane owns one row (R = 1); values and tangents
// live in VGPRs.  Operator values are computed by the same functions as srhip_eval_impl.h, so the
// loss equals srhip_eval_loss's.
// The operator / dual-number device functions live in srhip_grad_impl.h and the tile body in
// srhip_grad_tile.inc (included as text below), shared with srhip_grad_rowsets.hip.
#include "srhip_grad_impl.h"

namespace srhip {

// SRHIP_GRAD_WPE = W > 0 (build level, A/B): the tangent-carrying variants (KT >= 4) are compiled for at
// least W waves per SIMD (the register allocator's target; 0 leaves it free)
#ifndef SRHIP_GRAD_WPE
#define SRHIP_GRAD_WPE 0
#endif
template <typename T, int KT, int K, int GM, bool XLDS, int R>
__global__ __launch_bounds__(64 * GRAD_WAVES)
#if SRHIP_GRAD_WPE > 0
__attribute__((amdgpu_waves_per_eu(KT >= 4 ? SRHIP_GRAD_WPE : 1)))
#endif
void grad_kernel(GradArgs p) {
  constexpr int CW = GM == GMODE_LOSS ? 2 : 4;  // ints per chunk record
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
  extern __shared__ __attribute__((aligned(16))) unsigned char grad_lds[];
  T* xs = reinterpret_cast<T*>(grad_lds);
  const int rbr = p.rb_rows;
  // chunks are claimed dynamically from an LDS counter (wave w starts with chunk w): the host orders
  // each group's chunks by descending cost, so the waves of a workgroup finish within about one cheap
  // chunk of each other (a static round-robin left the cost spread idle at every workgroup's end);
  // every (chunk, row block) record is computed by one wave as before, so the bits do not change
  __shared__ int next_chunk;
  if (threadIdx.x == 0) next_chunk = GRAD_WAVES;
  if constexpr (XLDS) {
    const int nf = p.nfeat;
    const bool has_y = GM == GMODE_LOSS && Yg != nullptr;
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
  const T p0 = (T)p.loss_p0;
  const int max_steps = __builtin_amdgcn_readfirstlane(p.max_steps);
  auto claim = [&]() {
    int c = 0;
    if (lane == 0) c = atomicAdd(&next_chunk, 1);
    return __builtin_amdgcn_readfirstlane(c);
  };
  for (int ci = wave; ci < group_n; ci = claim()) {
    const int chunk = group_base + ci;
    int tree, c0;
    if (GM == GMODE_LOSS && !p.chunks) {  // the list in the kernel arguments
      tree = __builtin_amdgcn_readfirstlane(p.inl[2 * chunk]);
      c0 = __builtin_amdgcn_readfirstlane(p.inl[2 * chunk + 1]);
    } else {
      tree = __builtin_amdgcn_readfirstlane(p.chunks[CW * chunk]);
      c0 = __builtin_amdgcn_readfirstlane(p.chunks[CW * chunk + 1]);
    }
    if constexpr (GM == GMODE_LOSS && KT == 0) {
      if (p.screened) {
        // the screen launch's record of row block 0 for this chunk: a non-finite check statistic (a
        // NaN / Inf operator output in its rows) fails the tree; the blocks left unwritten here only
        // ever reach the reduction's check statistic, which block 0 already makes non-finite
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
      if constexpr (GM != GMODE_LOSS) {
        // record: (tree, c0, end component, output row of component c0)
        const int cend = __builtin_amdgcn_readfirstlane(p.chunks[CW * chunk + 2]);
        const int orow = __builtin_amdgcn_readfirstlane(p.chunks[CW * chunk + 3]);
        UNR for (int r = 0; r < R; ++r) {
          const int64_t row = row_base + tb + 64 * r + lane;
          if (row < p.nvalid) {
            T* der = reinterpret_cast<T*>(p.out_der) + (int64_t)orow * p.nvalid + row;
            UNR for (int j = 0; j < KT; ++j)
              if (c0 + j < cend) der[(int64_t)j * p.nvalid] = A[r].d[j];
          }
        }
        continue;
      }
#define SRHIP_GRAD_PART 2
#include "srhip_grad_tile.inc"
#undef SRHIP_GRAD_PART
    }
    if constexpr (GM != GMODE_LOSS) continue;
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

// per-chunk fixed-order reduction over row blocks, one wave per chunk: the fold both reduction kernels share,
// so a row shard's record has the unsharded bits by construction.  Element e of the chunk's (KT + 2)-wide
// record (loss sum, KT gradient sums, the check statistic -- MAX for Float32, SUM for Float64) goes to
// write(e, value) on lane 0.
// (each lane folds its row blocks b = lane, lane + 64, ... in order -- the loads of a batch issued
// before its adds: a strided loop waited out one memory latency per block and element)
template <int KT, bool CHK_MAX, class Write>
__device__ __forceinline__ void grad_reduce_fold(const double* __restrict__ slab, int nrb, int chunk, int lane,
                                                 Write write) {
  constexpr int BB = 8;
  for (int e = 0; e < KT + 2; ++e) {
    const bool is_max = CHK_MAX && e == KT + 1;
    double s = 0.0;
    for (int b0 = lane; b0 < nrb; b0 += 64 * BB) {
      double v[BB];
      UNR for (int j = 0; j < BB; ++j) {
        const int b = b0 + 64 * j;
        v[j] = b < nrb ? slab[((int64_t)chunk * nrb + b) * (KT + 2) + e] : 0.0;
      }
      UNR for (int j = 0; j < BB; ++j) {
        if (b0 + 64 * j >= nrb) break;
        s = is_max ? __builtin_elementwise_maximum(s, v[j]) : s + v[j];
      }
    }
    UNR for (int o = 32; o > 0; o >>= 1) {
      const double t = __shfl_xor(s, o);
      s = is_max ? __builtin_elementwise_maximum(s, t) : s + t;
    }
    if (lane == 0) write(e, s);
  }
}

// ... into (KT + 2) doubles per chunk by launch position (coherent host memory)
template <int KT, bool CHK_MAX>
__global__ __launch_bounds__(256) void grad_reduce_kernel(const double* __restrict__ slab, int nrb, int nchunks,
                                                          double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;
  grad_reduce_fold<KT, CHK_MAX>(slab, nrb, chunk, lane,
                                [&](int e, double s) { out[(int64_t)chunk * (KT + 2) + e] = s; });
}

// ... for a row shard (srhip_optim.cpp, the sharded ViewBackend): into a device buffer the ranks all-reduce in
// place, split by reduction operator: sum[pos][KT + 1] (loss sum, gradient sums; SUM) and chk[pos] (MAX for
// Float32, SUM for Float64).  pos[chunk] is the chunk's position in the exchange (the launch order depends on
// the rank's row count, the exchange must not).  A non-finite Float32 statistic, NaN included, is stored as
// +Inf, as the evaluation's shard reduction stores it (reduce_finish, srhip_eval.hip): a MAX across ranks is
// not defined on NaN.
template <int KT, bool CHK_MAX>
__global__ __launch_bounds__(256) void grad_reduce_shard_kernel(const double* __restrict__ slab, int nrb, int nchunks,
                                                                const int32_t* __restrict__ pos,
                                                                double* __restrict__ sum, double* __restrict__ chk) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;
  const int at = pos ? pos[chunk] : chunk;
  grad_reduce_fold<KT, CHK_MAX>(slab, nrb, chunk, lane, [&](int e, double s) {
    if (e <= KT) sum[(int64_t)at * (KT + 1) + e] = s;
    else chk[at] = CHK_MAX && !__builtin_isfinite(s) ? (double)INFINITY : s;
  });
}

// LDS staging of the row block when it fits (few features): [nfeat + 1][rb_rows] elements
constexpr size_t GRAD_LDS_MAX = 48 * 1024;
template <typename T> static size_t grad_lds_bytes(const GradArgs& a) {
  return (size_t)(a.nfeat + 1) * (size_t)a.rb_rows * sizeof(T);
}

// rows per lane: value-only passes (no tangents) carry 4 rows per lane (one dispatch per 256-row
// block); with tangents the register budget decides (GRAD_R)
// (K = 2, the common shallow-stack population -- C4's size-20 trees all fit it -- leaves room for two
// rows per lane with 4 tangents: half the dispatches per row at the same waves per SIMD)
template <int KT, int K> constexpr int grad_rows() {
  return KT == 0 ? 4 : (KT <= 4 && K <= 2 ? 2 : (KT <= 4 && K <= 4 ? GRAD_R : 1));
}

template <typename T, int KT, int K, int GM = GMODE_LOSS>
static hipError_t launch_grad_t(const GradArgs& a, dim3 grid, hipStream_t s) {
  constexpr int R = grad_rows<KT, K>();
  if (a.rb_rows % (64 * R)) return hipErrorInvalidValue;
  const size_t lds = grad_lds_bytes<T>(a);
  if (lds <= GRAD_LDS_MAX)
    hipLaunchKernelGGL((grad_kernel<T, KT, K, GM, true, R>), grid, dim3(64 * GRAD_WAVES), lds, s, a);
  else
    hipLaunchKernelGGL((grad_kernel<T, KT, K, GM, false, R>), grid, dim3(64 * GRAD_WAVES), 0, s, a);
  return hipGetLastError();
}

template <typename T, int GM>
static hipError_t launch_grad_rows_t(int K, const GradArgs& a, dim3 grid, hipStream_t s) {
  return K <= 4 ? launch_grad_t<T, GRAD_ROW_KT, 4, GM>(a, grid, s) : launch_grad_t<T, GRAD_ROW_KT, 8, GM>(a, grid, s);
}

hipError_t launch_grad_rows(int dtype, int K, int gmode, const GradArgs& a, dim3 grid, hipStream_t s) {
  if (gmode != GMODE_ROWC && gmode != GMODE_ROWF) return hipErrorInvalidValue;
  switch (dtype) {
    case SRHIP_F32:
      return gmode == GMODE_ROWC ? launch_grad_rows_t<float, GMODE_ROWC>(K, a, grid, s)
                                 : launch_grad_rows_t<float, GMODE_ROWF>(K, a, grid, s);
    case SRHIP_F64:
      return gmode == GMODE_ROWC ? launch_grad_rows_t<double, GMODE_ROWC>(K, a, grid, s)
                                 : launch_grad_rows_t<double, GMODE_ROWF>(K, a, grid, s);
    default: return hipErrorInvalidValue;
  }
}


// A derived view's derived columns (srhip_optim.cpp derived_view): Xd[j][row] = U_j(X[f_j][row]) over
// the view's ld rows, with the gradient kernel's own value function (the bits the kernel computes in
// place), and after the nd of them the tangent-zero columns Xd[nd + j][row] = U_j'(x) * 0 -- what the
// kernel's tangents of U_j(feature) are (a feature's tangent is +0): +-0, or NaN where U_j' is not finite.
struct DeriveSpec {
  uint32_t key[32];  // u << 16 | feature column
};
template <typename T>
__global__ __launch_bounds__(256) void grad_derive_kernel(const T* __restrict__ X, T* __restrict__ Xd, int64_t ld,
                                                          DeriveSpec spec) {
  const int j = blockIdx.y;
  const int u = (int)(spec.key[j] >> 16), f = (int)(spec.key[j] & 0xffff);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += (int64_t)gridDim.x * blockDim.x) {
    const T x = X[(int64_t)f * ld + i];
    T v = x, dv = T(0), v1, dv1;
    switch (u) {
#define X_(NAME, FN) \
  case UN_##NAME: dual_un<T, UN_##NAME, false>(x, v, dv1); dual_un<T, UN_##NAME, true>(x, v1, dv); break;
      SRHIP_UNOPS(X_)
#undef X_
      default: break;
    }
    Xd[(int64_t)j * ld + i] = v;
    Xd[(int64_t)(gridDim.y + j) * ld + i] = dv * T(0);
  }
}
hipError_t launch_grad_derive(int dtype, const void* X, void* Xd, int64_t ld, const uint32_t* keys, int nd,
                              hipStream_t s) {
  if (nd <= 0) return hipSuccess;
  if (nd > 32) return hipErrorInvalidValue;
  DeriveSpec spec{};
  for (int j = 0; j < nd; ++j) spec.key[j] = keys[j];
  const dim3 grid((unsigned)std::min<int64_t>((ld + 255) / 256, 1024), (unsigned)nd);
  if (dtype == SRHIP_F64)
    hipLaunchKernelGGL(grad_derive_kernel<double>, grid, dim3(256), 0, s, (const double*)X, (double*)Xd, ld, spec);
  else
    hipLaunchKernelGGL(grad_derive_kernel<float>, grid, dim3(256), 0, s, (const float*)X, (float*)Xd, ld, spec);
  return hipGetLastError();
}
hipError_t launch_grad(int dtype, int K, int kt, const GradArgs& a, dim3 grid, hipStream_t s) {
  if (kt != 0 && kt != 4 && kt != GRAD_KT) return hipErrorInvalidValue;
  switch (dtype) {
    case SRHIP_F32:
      if (kt == 0) return K <= 4 ? launch_grad_t<float, 0, 4>(a, grid, s) : launch_grad_t<float, 0, 8>(a, grid, s);
      if (kt == 4) return K <= 4 ? launch_grad_t<float, 4, 4>(a, grid, s) : launch_grad_t<float, 4, 8>(a, grid, s);
      return K <= 4 ? launch_grad_t<float, GRAD_KT, 4>(a, grid, s) : launch_grad_t<float, GRAD_KT, 8>(a, grid, s);
    case SRHIP_F64:  // K = 2 variants for shallow-stack populations (fewer VGPRs: two rows per lane)
      if (kt == 0)
        return K <= 2 ? launch_grad_t<double, 0, 2>(a, grid, s)
             : K <= 4 ? launch_grad_t<double, 0, 4>(a, grid, s) : launch_grad_t<double, 0, 8>(a, grid, s);
      if (kt == 4)
        return K <= 2 ? launch_grad_t<double, 4, 2>(a, grid, s)
             : K <= 4 ? launch_grad_t<double, 4, 4>(a, grid, s) : launch_grad_t<double, 4, 8>(a, grid, s);
      return K <= 2 ? launch_grad_t<double, GRAD_KT, 2>(a, grid, s)
           : K <= 4 ? launch_grad_t<double, GRAD_KT, 4>(a, grid, s) : launch_grad_t<double, GRAD_KT, 8>(a, grid, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_grad_reduce(int dtype, int kt, const double* slab, int nrb, int nchunks, double* out, hipStream_t s) {
  if (kt != 0 && kt != 4 && kt != GRAD_KT) return hipErrorInvalidValue;
  dim3 grid((nchunks + 3) / 4), block(256);
  if (kt == 0) {
    if (dtype == SRHIP_F32) hipLaunchKernelGGL((grad_reduce_kernel<0, true>), grid, block, 0, s, slab, nrb, nchunks, out);
    else hipLaunchKernelGGL((grad_reduce_kernel<0, false>), grid, block, 0, s, slab, nrb, nchunks, out);
    return hipGetLastError();
  }
  if (dtype == SRHIP_F32) {
    if (kt == 4) hipLaunchKernelGGL((grad_reduce_kernel<4, true>), grid, block, 0, s, slab, nrb, nchunks, out);
    else hipLaunchKernelGGL((grad_reduce_kernel<GRAD_KT, true>), grid, block, 0, s, slab, nrb, nchunks, out);
  } else {
    if (kt == 4) hipLaunchKernelGGL((grad_reduce_kernel<4, false>), grid, block, 0, s, slab, nrb, nchunks, out);
    else hipLaunchKernelGGL((grad_reduce_kernel<GRAD_KT, false>), grid, block, 0, s, slab, nrb, nchunks, out);
  }
  return hipGetLastError();
}

hipError_t launch_grad_reduce_shard(int dtype, int kt, const double* slab, int nrb, int nchunks, const int32_t* pos,
                                    double* sum, double* chk, hipStream_t s) {
  if (kt != 0 && kt != 4 && kt != GRAD_KT) return hipErrorInvalidValue;
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) return hipErrorInvalidValue;
  if (nchunks <= 0) return hipSuccess;
  dim3 grid((nchunks + 3) / 4), block(256);
#define SRHIP_REDUCE_SHARD(KT_, MAX_) \
  hipLaunchKernelGGL((grad_reduce_shard_kernel<KT_, MAX_>), grid, block, 0, s, slab, nrb, nchunks, pos, sum, chk)
  if (dtype == SRHIP_F32) {
    if (kt == 0) SRHIP_REDUCE_SHARD(0, true);
    else if (kt == 4) SRHIP_REDUCE_SHARD(4, true);
    else SRHIP_REDUCE_SHARD(GRAD_KT, true);
  } else {
    if (kt == 0) SRHIP_REDUCE_SHARD(0, false);
    else if (kt == 4) SRHIP_REDUCE_SHARD(4, false);
    else SRHIP_REDUCE_SHARD(GRAD_KT, false);
  }
#undef SRHIP_REDUCE_SHARD
  return hipGetLastError();
}

}  // namespace srhip
