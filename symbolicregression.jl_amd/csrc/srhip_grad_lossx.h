// srhip_grad_lossx.h — constant gradients under a loss given as an expression (srhip_grad_lossx.hip): the
// loss selector the optimiser's host path carries, the kernel's argument block and its launcher.
#pragma once
#include "srhip_grad.h"
#include "srhip_lossx.h"

namespace srhip {

// Which loss a gradient evaluation applies: one of the built-in SRHIP_LOSS_* kinds (grad_kernel's loss
// stage), or an expression's register program (grad_lossx_kernel's).  Exactly one of the two is set.
struct LossSel {
  const srhip_loss* kind = nullptr;
  const LossxProgram* expr = nullptr;
  LossSel(const srhip_loss* k) : kind(k) {}
  explicit LossSel(const LossxProgram* e) : expr(e) {}
};

// grad_kernel's arguments as they are, and the loss program beside them
struct GradLossxArgs {
  GradArgs g;
  LossxProgram lx;
};
static_assert(sizeof(GradLossxArgs) <= 4096, "kernel arguments are limited to 4 KB");

// launch_grad's GMODE_LOSS launch with the loss stage running lx (a.loss_kind / loss_p0 / weighted are not
// read: a weighted loss names the weight itself); the slab layout is launch_grad's, reduced by
// launch_grad_reduce
hipError_t launch_grad_lossx(int dtype, int K, int kt, const GradArgs& a, const LossxProgram& lx, dim3 grid,
                             hipStream_t s);

// grad_rowsets_kernel's arguments as they are, and the loss program beside them (srhip_grad_rowsets_lossx.hip)
struct GradRowsetLossxArgs {
  GradRowsetArgs g;
  LossxProgram lx;
};
static_assert(sizeof(GradRowsetLossxArgs) <= 4096, "kernel arguments are limited to 4 KB");

// launch_grad_rowsets with the loss stage running lx (a.loss_kind / loss_p0 are not read; a.weighted only
// says whether the packed sets carry a weight column): the same chunks, packed sets and final records
hipError_t launch_grad_rowsets_lossx(int dtype, int kt, const GradRowsetArgs& a, const LossxProgram& lx, int max_ld,
                                     hipStream_t s);

}  // namespace srhip
