// srhip_lossx.h — elementwise losses given as expressions (srhip_loss_expr): the compiled form shared by
// the host compiler and interpreter (srhip_lossx_compile.cpp, device-free), the evaluation driver
// (srhip_host.cpp srhip_eval_loss_expr) and the gfx950 loss pass (srhip_lossx.hip).
//
// A loss l(prediction, target[, weight]) compiles to a short register program over LOSSX_MAX_STACK value
// slots: every instruction names the slot it writes and the slots it reads, so neither interpreter keeps a
// stack pointer.  Slots are the positions of a postfix evaluation's operand stack, with the child of greater
// need evaluated first (the Sethi-Ullman order of srhip_compile.cpp need_); every leaf takes a slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srhip.h"

namespace srhip {

constexpr int LOSSX_MAX_NODES = 64;   // nodes of the tree, and instructions of its program
constexpr int LOSSX_MAX_STACK = 8;    // value slots
// rows of one workgroup's block: 256 threads x 16 rows.  Part of the reduction contract: a tree's sum is
// the sum of its blocks' partials, so the constant fixes the bits of every result.
constexpr int LOSSX_THREADS = 256;
constexpr int LOSSX_ROWS_PER_LANE = 4;     // rows a lane holds in registers through one run of the program
constexpr int LOSSX_PASSES = 4;            // runs of the program per block
constexpr int LOSSX_BLOCK_ROWS = LOSSX_THREADS * LOSSX_ROWS_PER_LANE * LOSSX_PASSES;

// opcodes: an SRHIP_OP_* code (binary: dst = op(slot a, slot b); unary: dst = op(slot a)), or a load
enum : uint32_t { LX_LOAD_PRED = 0x100, LX_LOAD_Y = 0x101, LX_LOAD_W = 0x102, LX_LOAD_CONST = 0x103 };

struct LossxIns {
  uint16_t op;
  uint8_t dst, a, b, pad[3];
  uint64_t imm;  // LX_LOAD_CONST: the constant's bits in T (Float32 in the low word)
};
static_assert(sizeof(LossxIns) == 16, "LossxIns must be 16 bytes");

// the whole program travels in the loss pass's kernel arguments (1040 bytes)
struct LossxProgram {
  int32_t n = 0;      // instructions; the result is in slot 0
  int32_t nargs = 2;  // 2: l(pred, y); 3: l(pred, y, w)
  int32_t dtype = SRHIP_F32;
  int32_t need = 0;   // slots used
  LossxIns ins[LOSSX_MAX_NODES];
};

// srhip_lossx.hip: partial sums of tree list[s]'s losses over each block of LOSSX_BLOCK_ROWS rows (and, for
// weighted data, of the weights as one more slot), then their sum per slot in ascending block order.
//   pred: T[ntrees][m]; y, w: T[m] (w may be null); list: int32[nlive] trees to reduce (device);
//   partials: double[(nlive + (w ? 1 : 0)) * nblocks] (device); out: double[nlive + (w ? 1 : 0)] (device).
hipError_t launch_lossx(const LossxProgram& prog, const void* pred, const void* y, const void* w, int64_t m,
                        const int32_t* list, int32_t nlive, double* partials, double* out, hipStream_t stream);
inline int64_t lossx_blocks(int64_t m) { return (m + LOSSX_BLOCK_ROWS - 1) / LOSSX_BLOCK_ROWS; }

}  // namespace srhip

// the opaque handle of include/srhip.h
struct srhip_loss_expr {
  srhip::LossxProgram prog;
};
