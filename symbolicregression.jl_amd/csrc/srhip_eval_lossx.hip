// srhip_eval_lossx.hip — a whole view under a loss given as an expression (srhip_loss_expr) in ONE launch:
// srhip_eval_loss_expr_fused, srhip_eval_loss_expr_submit and the expression coalescer's flushes.
//
// eval_lossx_kernel<T, RT, XLDS>: a persistent-style grid.  Workgroup g of G takes the items g, g + G, ... of
// the launch; an item is (tree group, loss block): trees_per_group consecutive order slots over the
// LOSSX_BLOCK_ROWS rows of one loss block.  For each item the workgroup
//   1. runs the unchanged tile interpreter in its prediction mode, eval_block<T, RT, K_MAX, MODE_PRED, XLDS>, as
//      row block 0 of a view that starts at the loss block's first row and holds its valid rows: the block's
//      feature columns are staged once for the group's trees (XLDS) or read from global memory, the waves claim
//      the group's trees, the check statistic and the rows evaluated go to the (block, slot) entries that
//      launch_reduce folds into the records srhip_eval_predict's decision reads, and the predictions go to the
//      workgroup's own slab of a global scratch, [tree of the group][valid rows of the block] -- the launch
//      relabels its trees by order slot (EvalLossxArgs), so store_pred's [tree][nvalid] is that packing;
//   2. after a workgroup barrier runs the loss program over those predictions, one wave per tree of the group,
//      and reduces in lossx_kernel's order restated for one wave as rowsets_lossx_kernel restates it: lane l
//      plays threads v = l, 64 + l, 128 + l, 192 + l of the 256-thread block; thread v starts from 0.0 and adds
//      rows v + 256 i, i = 0 .. 15 ascending, as doubles; each of the four virtual waves takes the xor butterfly
//      32 .. 1; they combine as ((w0 + w1) + w2) + w3; one double goes to partials[slot][block].  The weights of
//      a weighted view are one more slot in the same layout, written by the first group's item of each block.
// No atomics and no counter: an item's owner is a function of its index, every (slot, block) partial is written
// by one wave, and a tree's partials do not depend on what else the launch holds.
// lossx_finish then adds each slot's partials in ascending block order onto 0.0 (lossx_finish_kernel's text,
// which srhip_lossx.hip keeps to itself).
//
// The scratch is bounded by the launch geometry (plan_eval_lossx): workgroups x trees_per_group x
// LOSSX_BLOCK_ROWS x sizeof(T) bytes, whatever ntrees x m is.
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

template <typename T, int RT, bool XLDS>
__global__ __launch_bounds__(64 * eval_waves(RT, K_MAX)) void eval_lossx_kernel(const EvalLossxArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using CT = typename Chk<T>::type;
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int nwaves = (int)blockDim.x >> 6;
  const int tpg = q.e.trees_per_group;
  const int ntrees = q.e.ntrees;
  const int64_t nitems = (int64_t)q.ngroups * q.nblocks;
  const bool weighted = q.w != nullptr;
  const bool lx_w = weighted && q.lx.nargs == 3;
  T* const slab = reinterpret_cast<T*>(q.pred) + (int64_t)blockIdx.x * tpg * LOSSX_BLOCK_ROWS;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int grp = (int)(item / q.nblocks);
    const int blk = (int)(item - (int64_t)grp * q.nblocks);
    const int64_t row_base = (int64_t)blk * LOSSX_BLOCK_ROWS;
    const int nrel = (int)min<int64_t>(q.m - row_base, (int64_t)LOSSX_BLOCK_ROWS);  // 1 .. LOSSX_BLOCK_ROWS
    const int slot0 = grp * tpg;
    const int gn = min(tpg, ntrees - slot0);

    // ---- 1. the interpreter over the block, predictions to the workgroup's slab ----
    EvalArgs e = q.e;
    e.X = reinterpret_cast<const T*>(q.e.X) + row_base;
    e.nvalid = nrel;
    e.out_pred = slab - (int64_t)slot0 * nrel;  // store_pred indexes [slot][nvalid]
    e.slab_chk = reinterpret_cast<CT*>(q.e.slab_chk) + (int64_t)blk * ntrees;
    e.slab_rows = q.e.slab_rows + (int64_t)blk * ntrees;
    eval_block<T, RT, K_MAX, MODE_PRED, XLDS>(e, smem, 0, grp);
    __syncthreads();  // the predictions are read back by other waves

    // ---- 2. the loss program over the predictions, lossx_kernel's reduction one wave per tree ----
    using O = FOps<T>;
    constexpr int R = LOSSX_ROWS_PER_LANE;
    const T* const ly = reinterpret_cast<const T*>(q.y) + row_base;
    const T* const lw = reinterpret_cast<const T*>(q.w) + row_base;  // (read only when weighted)
    const int nunits = gn + ((weighted && grp == 0) ? 1 : 0);  // the group's trees, then the weights' slot
    for (int u = wave; u < nunits; u += nwaves) {
      double bsum = 0.0;
      if (u >= gn) {
        for (int k = 0; k < LOSSX_THREADS / 64; ++k) {  // the weights' sum in the same layout
          int v = 64 * k + lane;
          asm volatile("" : "+v"(v));  // (as below)
          double wacc = 0.0;
          for (int i = 0; i < LOSSX_PASSES * R; ++i) {
            const int row = i * LOSSX_THREADS + v;
            if (row < nrel) wacc += (double)lw[row];
          }
          wacc = wave_butterfly(wacc);
          bsum = k == 0 ? wacc : bsum + wacc;
        }
        if (lane == 0) q.partials[(int64_t)ntrees * q.nblocks + blk] = bsum;
        continue;
      }
      const T* const pred = slab + (int64_t)u * nrel;
      for (int k = 0; k < LOSSX_THREADS / 64; ++k) {  // virtual wave k: thread v = 64 k + lane
        // (opaque: left visible, the 64 row offsets of a block's (virtual wave, pass, row) triples are hoisted out
        // of the item loop and held -- 128 VGPRs -- across the interpreter)
        int v = 64 * k + lane;
        asm volatile("" : "+v"(v));
        double acc = 0.0;
        for (int ps = 0; ps < LOSSX_PASSES; ++ps) {
          const int rq = ps * R * LOSSX_THREADS;
          if (rq + 64 * k >= nrel) break;  // (rq >= nrel: lossx_kernel's break; else no row of this wave's: nothing added)
          T vp[R], vy[R], vw[R];
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const int row = rq + j * LOSSX_THREADS + v;
            const bool in = row < nrel;
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
            if (row < nrel) acc += (double)s0[j];
          }
        }
        acc = wave_butterfly(acc);
        bsum = k == 0 ? acc : bsum + acc;
      }
      if (lane == 0) q.partials[(int64_t)(slot0 + u) * q.nblocks + blk] = bsum;
    }
    __syncthreads();  // every wave is done with the slab and the staged block
  }
}

// lossx_finish_kernel's text (srhip_lossx.hip): one wave per slot adds the slot's partials in ascending block order
__global__ __launch_bounds__(64) void eval_lossx_finish_kernel(const double* __restrict__ partials, int64_t nblocks,
                                                               int32_t nslots, double* __restrict__ out) {
  const int32_t slot = blockIdx.x;
  if (slot >= nslots) return;
  const double* p = partials + (int64_t)slot * nblocks;
  const int lane = threadIdx.x;
  double acc = 0.0;  // the same in every lane
  for (int64_t base = 0; base < nblocks; base += 64) {
    const double v = base + lane < nblocks ? p[base + lane] : 0.0;
    const int cnt = (int)(nblocks - base < 64 ? nblocks - base : 64);
    for (int k = 0; k < cnt; ++k) acc += __shfl(v, k, 64);
  }
  if (lane == 0) out[slot] = acc;
}

template <typename T, int RT, bool XLDS>
static hipError_t launch_eval_lossx_t(const EvalLossxArgs& q, int wgs, size_t lds, hipStream_t s) {
  auto kern = eval_lossx_kernel<T, RT, XLDS>;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(wgs), dim3(64 * eval_waves(RT, K_MAX)), lds, s, q);
  return hipGetLastError();
}

hipError_t launch_eval_lossx(int dtype, const EvalLossxArgs& q, bool xlds, int wgs, size_t lds, double* out,
                             hipStream_t s) {
  if (dtype != SRHIP_F32 && dtype != SRHIP_F64) return hipErrorInvalidValue;
  const LossxProgram& lx = q.lx;
  if (lx.n < 1 || lx.n > LOSSX_MAX_NODES || lx.dtype != dtype) return hipErrorInvalidValue;
  for (int i = 0; i < lx.n; ++i)  // every slot index the kernel's switches see is one of the eight
    if (lx.ins[i].dst >= LOSSX_MAX_STACK || lx.ins[i].a >= LOSSX_MAX_STACK || lx.ins[i].b >= LOSSX_MAX_STACK)
      return hipErrorInvalidValue;
  const EvalArgs& a = q.e;
  const size_t es = dtype == SRHIP_F64 ? 8 : 4;
  if (a.ntrees <= 0 || q.m <= 0 || wgs <= 0 || a.trees_per_group <= 0 || a.rb_rows != LOSSX_BLOCK_ROWS ||
      q.nblocks != lossx_blocks(q.m) || q.ngroups != (a.ntrees + a.trees_per_group - 1) / a.trees_per_group ||
      (int64_t)wgs > (int64_t)q.nblocks * q.ngroups || a.ld < (int64_t)q.nblocks * LOSSX_BLOCK_ROWS || a.group_off ||
      a.fused || a.persistent || a.weighted || a.has_y || a.nd != 0 || a.early_exit || a.tile_claims ||
      !a.slab_chk || !a.slab_rows || !a.order || !a.prog_off || !a.code || !a.X || !q.y || !q.pred || !q.partials ||
      !out || (xlds && lds < (size_t)a.nfeat * LOSSX_BLOCK_ROWS * es))
    return hipErrorInvalidValue;
  hipError_t err;
  if (dtype == SRHIP_F32)
    err = xlds ? launch_eval_lossx_t<float, R_F32, true>(q, wgs, lds, s) : launch_eval_lossx_t<float, R_F32, false>(q, wgs, lds, s);
  else
    err = xlds ? launch_eval_lossx_t<double, R_F64, true>(q, wgs, lds, s) : launch_eval_lossx_t<double, R_F64, false>(q, wgs, lds, s);
  if (err != hipSuccess) return err;
  const int32_t nslots = a.ntrees + (q.w ? 1 : 0);
  hipLaunchKernelGGL(eval_lossx_finish_kernel, dim3((unsigned)nslots), dim3(64), 0, s, q.partials, (int64_t)q.nblocks, nslots,
                     out);
  return hipGetLastError();
}

}  // namespace srhip
