// srhip_rowsets_lossx.hip — one launch for many (tree, row subset) pairs under a loss given as an expression
// (srhip_loss_expr): srhip_eval_loss_expr_rowsets, the batching mode's fresh minibatch per score with a
// custom elementwise_loss.
//
// One wavefront owns one tree, as in rowsets_kernel (srhip_rowsets.hip): single-wave workgroups, one per
// launched tree, longest and costliest first.  The wave
//   1. stages its set's rows of every feature column, y and w by index into its own LDS region;
//   2. folds the set's feature statistics and the position-order weight sum (rowsets_kernel's step 2, the same
//      text: the gradient batch of the optimiser reads both);
//   3. runs the unchanged tile interpreter in its prediction mode, eval_block<T, R, K_MAX, MODE_PRED, false>,
//      as a fused single-row-block launch of one tree group: the check statistic and the rows evaluated go to
//      the per-tree host records srhip_eval_predict's decision reads, the predictions to the wave's own row of
//      a per-launch global scratch [launched tree][ld] (they are read back by other lanes of the same wave
//      after a workgroup barrier; LDS would take a column off every set's cap);
//   4. runs the loss program over those predictions and reduces in lossx_kernel's order restated for one wave:
//      lane l plays threads v = l, 64 + l, 128 + l, 192 + l of the 256-thread block; thread v of block b starts
//      from 0.0 and adds rows 4096 b + v + 256 i, i = 0 .. 15 ascending, as doubles; each of the four virtual
//      waves takes the xor butterfly 32 .. 1; they combine as ((w0 + w1) + w2) + w3; the blocks are added in
//      ascending order onto 0.0 (lossx_finish_kernel).  The weights of a weighted dataset are summed in the
//      same layout: srhip_eval_loss_expr divides by that sum.
// Lane 0 writes the tree's loss sum and weight sum to coherent host memory: one launch, one synchronisation,
// no atomics.  A (virtual wave, pass) none of whose rows lies in the set adds nothing in lossx_kernel and is
// skipped here.
#include "srhip_eval_impl.h"
#include "srhip_lossx.h"
#include "srhip_ops.h"

namespace srhip {
namespace {

template <typename T> __device__ __forceinline__ T imm_value(uint64_t imm);
template <> __device__ __forceinline__ float imm_value<float>(uint64_t imm) { return __uint_as_float((uint32_t)imm); }
template <> __device__ __forceinline__ double imm_value<double>(uint64_t imm) { return __longlong_as_double((long long)imm); }

__device__ __forceinline__ double wave_butterfly(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace

template <typename T, int RT>
__global__ __launch_bounds__(64) void rowsets_lossx_kernel(const RowsetLossxArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const RowsetArgs& a = q.r;
  T* lx = reinterpret_cast<T*>(smem);
  const int lane = (int)threadIdx.x;
  const int tree = __builtin_amdgcn_readfirstlane(a.e.order[blockIdx.x]);
  const int64_t r0 = a.row_off[tree];
  const int m = __builtin_amdgcn_readfirstlane((int)(a.row_off[tree + 1] - r0));  // 1 .. ld_lds (host-checked)
  constexpr int TILE = 64 * RT;
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

  // ---- 2. the set's feature statistics and position-order weight sum (rowsets_kernel's step 2) ----
  for (int f = 0; f < nx; ++f) {
    const T* col = lx + (int64_t)f * ld;
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
    if (lane == 0) {
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

  // ---- 3. the interpreter over the wave's region, predictions to the wave's scratch row ----
  T* const pred = reinterpret_cast<T*>(q.pred) + (int64_t)blockIdx.x * ld;
  EvalArgs e = a.e;
  e.X = lx;
  e.y = nullptr;
  e.w = nullptr;
  e.nvalid = m;
  e.out_pred = pred - (int64_t)tree * m;  // store_pred indexes [tree][nvalid]
  eval_block<T, RT, K_MAX, MODE_PRED, false>(e, smem, 0, (int)blockIdx.x);
  __syncthreads();  // the predictions are read back by other lanes

  // ---- 4. the loss program over the predictions, lossx_kernel's reduction for one wave ----
  using O = FOps<T>;
  constexpr int R = LOSSX_ROWS_PER_LANE;
  const bool lx_w = weighted && q.lx.nargs == 3;
  double total = 0.0, wtotal = 0.0;
  for (int row0 = 0; row0 < m; row0 += LOSSX_BLOCK_ROWS) {
    double blk = 0.0, wblk = 0.0;
    for (int k = 0; k < LOSSX_THREADS / 64; ++k) {  // virtual wave k: thread v = 64 k + lane
      const int v = 64 * k + lane;
      double acc = 0.0;
      for (int ps = 0; ps < LOSSX_PASSES; ++ps) {
        const int rq = row0 + ps * R * LOSSX_THREADS;
        if (rq + 64 * k >= m) break;  // (rq >= m: lossx_kernel's break; else no row of this wave's: nothing added)
        T vp[R], vy[R], vw[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int row = rq + j * LOSSX_THREADS + v;
          const bool in = row < m;
          vp[j] = in ? pred[row] : T(0);
          vy[j] = in ? ly[row] : T(0);
          vw[j] = (in && lx_w) ? lw[row] : T(0);
        }
#define LX_PROG q.lx
#include "srhip_lossx_run.inc"
#undef LX_PROG
        // ascending row order within the thread
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int row = rq + j * LOSSX_THREADS + v;
          if (row < m) acc += (double)s0[j];
        }
      }
      acc = wave_butterfly(acc);
      blk = k == 0 ? acc : blk + acc;
      if (weighted) {  // the weights' sum in the same layout
        double wacc = 0.0;
        for (int i = 0; i < LOSSX_PASSES * R; ++i) {
          const int row = row0 + i * LOSSX_THREADS + v;
          if (row < m) wacc += (double)lw[row];
        }
        wacc = wave_butterfly(wacc);
        wblk = k == 0 ? wacc : wblk + wacc;
      }
    }
    total += blk;
    wtotal += wblk;
  }
  if (lane == 0) {
    q.out_loss[tree] = total;
    if (weighted) q.out_wsum[tree] = wtotal;
  }
}

template <typename T, int RT>
static hipError_t launch_rowsets_lossx_t(const RowsetLossxArgs& q, int nlaunch, size_t lds, hipStream_t s) {
  auto kern = rowsets_lossx_kernel<T, RT>;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(nlaunch), dim3(64), lds, s, q);
  return hipGetLastError();
}

int rowset_lossx_cap(int dtype, int64_t nfeat, bool weighted) {
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) return 0;
  return rowset_cap(dtype, nfeat, weighted);  // the predictions live in global scratch: no column lost
}

hipError_t launch_rowsets_lossx(int dtype, const RowsetArgs& a, const LossxProgram& lx, void* pred, double* out_loss,
                                double* out_wsum, int nlaunch, hipStream_t s) {
  if (nlaunch <= 0) return hipSuccess;
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) return hipErrorInvalidValue;
  if (lx.n < 1 || lx.n > LOSSX_MAX_NODES || lx.dtype != dtype) return hipErrorInvalidValue;
  for (int i = 0; i < lx.n; ++i)  // every slot index the kernel's switches see is one of the eight
    if (lx.ins[i].dst >= LOSSX_MAX_STACK || lx.ins[i].a >= LOSSX_MAX_STACK || lx.ins[i].b >= LOSSX_MAX_STACK)
      return hipErrorInvalidValue;
  const int tile = 64 * rows_per_lane(dtype);
  const size_t es = dtype == SRHIP_F64 ? 8 : 4;
  const size_t lds = (size_t)(a.nstage + 1 + (a.e.weighted ? 1 : 0)) * a.ld_lds * es;
  if (a.ld_lds <= 0 || a.ld_lds % tile != 0 || lds > (size_t)ROWSET_LDS_BUDGET || a.e.nfeat > a.nstage ||
      a.e.rb_rows != a.ld_lds || a.e.ld != a.ld_lds || !a.e.fused || a.e.nrb != 1 || a.e.trees_per_group != 1 ||
      !pred || !out_loss || (a.e.weighted && (!out_wsum || !a.wsum)) || !a.fstat)
    return hipErrorInvalidValue;
  RowsetLossxArgs q{};
  q.r = a;
  q.lx = lx;
  q.pred = pred;
  q.out_loss = out_loss;
  q.out_wsum = out_wsum;
  switch (dtype) {
    case SRHIP_F32: return launch_rowsets_lossx_t<float, R_F32>(q, nlaunch, lds, s);
    default: return launch_rowsets_lossx_t<double, R_F64>(q, nlaunch, lds, s);
  }
}

}  // namespace srhip
