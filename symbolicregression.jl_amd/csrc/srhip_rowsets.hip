// srhip_rowsets.hip — one launch for many (tree, row subset) pairs: the batching mode's fresh
// minibatch per score (reference: src/LossFunctions.jl:114-127, src/Mutate.jl:96-98,268).
//
// One wavefront owns one tree.  Workgroups are single waves, one per launched tree (grid.x = trees, in
// descending set length x tree cost), so the hardware's workgroup dispatcher is the claim counter: a
// CU takes the next tree as soon as one of its waves retires.  The wave
//   1. stages its set's rows of every feature column, y and w BY INDEX from the resident dataset into
//      its own LDS region [column][ld_lds] -- gather_kernel's rule: the positions past the set's end up
//      to the end of its last tile replicate the set's last row, with the padding weight -0.0;
//   2. folds the set's per-feature statistics (f64 sum, non-finite count, max |x|) with the arithmetic
//      of feature_stats_kernel / feature_stats_final for a single row chunk (256 strided partial sums,
//      the same halving tree), and the weight sum in position order (gathered_weight_sum's loop);
//   3. runs the unchanged tile interpreter over that region: eval_block<T, R, K_MAX, MODE_LOSS, false>
//      on a per-wave copy of the launch's EvalArgs whose X / y / w are the LDS region and whose row
//      count is the set's length -- a fused single-row-block launch of one tree group per workgroup, so
//      the loss chunks (position p belongs to chunk p / loss_chunk) are summed by lane and combined in
//      reduce_kernel's order by the very code that serves srhip_eval_loss on a small view.
// Per-tree records (loss sum, check statistic, rows; feature statistics; weight sum) go to coherent
// host memory; the host decides every tree on its own record after the call's one synchronisation.
//
// LDS: a wave's region is (features + y [+ w]) x ld_lds elements, ld_lds = the launch's longest set
// rounded up to whole tiles; ROWSET_LDS_BUDGET bytes per wave at most (rowset_cap), which leaves four
// waves per CU (one per SIMD) at the cap and a dozen at the search's 50-row sets.
#include "srhip_eval_impl.h"

namespace srhip {

template <typename T, int R>
__global__ __launch_bounds__(64) void rowsets_kernel(RowsetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* lx = reinterpret_cast<T*>(smem);
  const int lane = (int)threadIdx.x;
  const int tree = __builtin_amdgcn_readfirstlane(a.e.order[blockIdx.x]);
  const int64_t r0 = a.row_off[tree];
  const int m = __builtin_amdgcn_readfirstlane((int)(a.row_off[tree + 1] - r0));  // 1 .. ld_lds (host-checked)
  constexpr int TILE = 64 * R;
  const int ld = a.ld_lds;
  const int staged = min(ld, (m + TILE - 1) / TILE * TILE);  // whole tiles of this set
  const int nx = a.nstage;
  const bool weighted = a.e.weighted != 0;
  const T* gX = reinterpret_cast<const T*>(a.e.X);
  const T* gy = reinterpret_cast<const T*>(a.e.y);
  const T* gw = reinterpret_cast<const T*>(a.e.w);
  T* ly = lx + (int64_t)nx * ld;
  T* lw = ly + ld;

  // ---- 1. stage by index ----
  for (int p = lane; p < staged; p += 64) {
    const int64_t j = a.rows[r0 + min(p, m - 1)];  // in [0, n): checked on the host before the launch
    for (int c = 0; c < nx; ++c) lx[(int64_t)c * ld + p] = gX[(int64_t)c * a.src_ld + j];
    ly[p] = gy[j];
    if (weighted) lw[p] = p < m ? gw[j] : pad_weight<T>();
  }
  __syncthreads();

  // ---- 2. the set's feature statistics and weight sum ----
  if constexpr (!kIsInt<T>) {
    for (int f = 0; f < nx; ++f) {
      const T* col = lx + (int64_t)f * ld;
      // feature_stats_kernel's thread v = lane + 64 j adds rows v, v + 256, ...
      double s[4] = {0.0, 0.0, 0.0, 0.0}, mx[4] = {0.0, 0.0, 0.0, 0.0};
      unsigned long long bad[4] = {0, 0, 0, 0};
      for (int base = 0; base < m; base += 256) {
        UNR for (int j = 0; j < 4; ++j) {
          const int p = base + 64 * j + lane;
          if (p < m) {
            const T v = col[p];
            if (!m_isfinite(v)) {
              bad[j]++;
            } else {
              s[j] += sizeof(T) == 8 ? (double)v * 0x1p-64 : (double)v;
              mx[j] = fmax(mx[j], fabs((double)v));
            }
          }
        }
      }
      // its halving tree: o = 128 (v += v + 128), o = 64, then the lanes
      s[0] += s[2];
      s[1] += s[3];
      s[0] += s[1];
      mx[0] = fmax(fmax(mx[0], mx[2]), fmax(mx[1], mx[3]));
      bad[0] += bad[2] + bad[1] + bad[3];
      double ss = s[0], sm = mx[0];
      unsigned long long sb = bad[0];
      UNR for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_down(ss, o);
        sm = fmax(sm, __shfl_down(sm, o));
        sb += __shfl_down(sb, o);
      }
      if (lane == 0) {  // feature_stats_final over the one chunk
        FeatStat* out = a.fstat + (int64_t)tree * nx + f;
        out->sum = 0.0 + ss;
        out->nonfinite = (long long)sb;
        out->maxabs = fmax(0.0, sm);
      }
    }
    if (weighted && lane == 0) {
      double s = 0.0;
      for (int p = 0; p < m; ++p) s += (double)lw[p];
      a.wsum[tree] = s;
    }
  }

  // ---- 3. the interpreter over the wave's region ----
  EvalArgs q = a.e;
  q.X = lx;
  q.y = ly;
  q.w = weighted ? lw : nullptr;
  q.nvalid = m;
  eval_block<T, R, K_MAX, MODE_LOSS, false>(q, smem, 0, (int)blockIdx.x);
}

template <typename T, int R>
static hipError_t launch_rowsets_t(const RowsetArgs& a, int nlaunch, size_t lds, hipStream_t s) {
  auto kern = rowsets_kernel<T, R>;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(nlaunch), dim3(64), lds, s, a);
  return hipGetLastError();
}

int rowset_cap(int dtype, int64_t nfeat, bool weighted) {
  const int64_t tile = 64 * (int64_t)rows_per_lane(dtype);
  const int64_t row_bytes = (nfeat + 1 + (weighted ? 1 : 0)) * (dtype == SRHIP_F64 ? 8 : 4);
  return (int)(ROWSET_LDS_BUDGET / row_bytes / tile * tile);
}

hipError_t launch_rowsets(int dtype, const RowsetArgs& a, int nlaunch, hipStream_t s) {
  if (nlaunch <= 0) return hipSuccess;
  const int tile = 64 * rows_per_lane(dtype);
  const size_t es = dtype == SRHIP_F64 ? 8 : 4;
  const size_t lds = (size_t)(a.nstage + 1 + (a.e.weighted ? 1 : 0)) * a.ld_lds * es;
  if (a.ld_lds <= 0 || a.ld_lds % tile != 0 || lds > (size_t)ROWSET_LDS_BUDGET || a.e.nfeat > a.nstage ||
      a.e.rb_rows != a.ld_lds || a.e.ld != a.ld_lds || !a.e.fused || a.e.nrb != 1 || a.e.trees_per_group != 1)
    return hipErrorInvalidValue;
  switch (dtype) {
    case SRHIP_F32: return launch_rowsets_t<float, R_F32>(a, nlaunch, lds, s);
    case SRHIP_F64: return launch_rowsets_t<double, R_F64>(a, nlaunch, lds, s);
    case SRHIP_I32: return launch_rowsets_t<int32_t, R_F32>(a, nlaunch, lds, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace srhip
