// srhip_lossx.hip — the loss pass of srhip_eval_loss_expr (gfx950): a loss expression evaluated per row
// over predictions that stay on the device, reduced to one double per tree.
//
//   lossx_kernel<T>        grid (row blocks, tree slots), 256 threads.  One workgroup takes one tree's block
//                          of LOSSX_BLOCK_ROWS rows: each lane holds LOSSX_ROWS_PER_LANE rows (stride 256:
//                          a wave's load is 256 contiguous bytes of Float32) through one run of the loss
//                          program, LOSSX_PASSES runs per block.  The program is the same for the whole
//                          launch and travels in the kernel arguments (one run: srhip_lossx_run.inc, included
//                          as text here and by rowsets_lossx_kernel); its instructions are read with
//                          scalar loads and dispatched by a wave-uniform switch onto FOps<T>; the value
//                          slots are registers (every slot index is resolved by a uniform switch to a
//                          constant).  A lane adds its rows' losses in double in ascending row order; the
//                          block combines its lanes by an xor butterfly (32, 16, ..., 1) and its four
//                          waves in wave order, and stores one double to partials[slot][block].
//   lossx_finish_kernel    one wave per slot adds the slot's partials in ascending block order.
//
// No atomics: a slot's result is a fixed-order sum of its own rows, whatever else the launch holds.  The
// weights' sum (weighted data) is one more slot reduced the same way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srhip_isa.h"
#include "srhip_lossx.h"
#include "srhip_ops.h"

namespace srhip {
namespace {

constexpr int R = LOSSX_ROWS_PER_LANE;

template <typename T> __device__ __forceinline__ T imm_value(uint64_t imm);
template <> __device__ __forceinline__ float imm_value<float>(uint64_t imm) { return __uint_as_float((uint32_t)imm); }
template <> __device__ __forceinline__ double imm_value<double>(uint64_t imm) { return __longlong_as_double((long long)imm); }

// the block's lanes combined in one fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return s;
}

template <typename T>
__global__ __launch_bounds__(LOSSX_THREADS) void lossx_kernel(const LossxProgram prog, const T* __restrict__ pred,
                                                              const T* __restrict__ y, const T* __restrict__ w,
                                                              int64_t m, const int32_t* __restrict__ list, int32_t nlive,
                                                              int32_t nslots, int64_t nblocks, double* __restrict__ partials) {
  using O = FOps<T>;
  __shared__ double lds[LOSSX_THREADS / 64];
  const int64_t block = blockIdx.x;
  const int64_t row0 = block * LOSSX_BLOCK_ROWS;
  for (int32_t slot = blockIdx.y; slot < nslots; slot += gridDim.y) {
    double acc = 0.0;
    if (slot >= nlive) {
      // the weights' sum, once per view
      for (int q = 0; q < LOSSX_PASSES * R; ++q) {
        const int64_t row = row0 + (int64_t)q * LOSSX_THREADS + threadIdx.x;
        if (row < m) acc += (double)w[row];
      }
    } else {
      const T* __restrict__ p = pred + (int64_t)list[slot] * m;
      for (int q = 0; q < LOSSX_PASSES; ++q) {
        const int64_t rq = row0 + (int64_t)q * R * LOSSX_THREADS;
        if (rq >= m) break;
        T vp[R], vy[R], vw[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int64_t row = rq + (int64_t)j * LOSSX_THREADS + threadIdx.x;
          const bool in = row < m;
          vp[j] = in ? p[row] : T(0);
          vy[j] = in ? y[row] : T(0);
          vw[j] = (in && w) ? w[row] : T(0);
        }
#define LX_PROG prog
#include "srhip_lossx_run.inc"
#undef LX_PROG
        // ascending row order within the lane
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int64_t row = rq + (int64_t)j * LOSSX_THREADS + threadIdx.x;
          if (row < m) acc += (double)s0[j];
        }
      }
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[(int64_t)slot * nblocks + block] = sum;
  }
}

__global__ __launch_bounds__(64) void lossx_finish_kernel(const double* __restrict__ partials, int64_t nblocks, int32_t nslots,
                                                          double* __restrict__ out) {
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

}  // namespace

hipError_t launch_lossx(const LossxProgram& prog, const void* pred, const void* y, const void* w, int64_t m,
                        const int32_t* list, int32_t nlive, double* partials, double* out, hipStream_t stream) {
  const int32_t nslots = nlive + (w ? 1 : 0);
  const int64_t nblocks = lossx_blocks(m);
  if (nslots <= 0 || nblocks <= 0) return hipSuccess;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nblocks, (unsigned)(nslots < 65535 ? nslots : 65535));
  if (prog.dtype == SRHIP_F64)
    hipLaunchKernelGGL(lossx_kernel<double>, grid, dim3(LOSSX_THREADS), 0, stream, prog, (const double*)pred, (const double*)y,
                       (const double*)w, m, list, nlive, nslots, nblocks, partials);
  else
    hipLaunchKernelGGL(lossx_kernel<float>, grid, dim3(LOSSX_THREADS), 0, stream, prog, (const float*)pred, (const float*)y,
                       (const float*)w, m, list, nlive, nslots, nblocks, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lossx_finish_kernel, dim3((unsigned)nslots), dim3(64), 0, stream, partials, nblocks, nslots, out);
  return hipGetLastError();
}

}  // namespace srhip
