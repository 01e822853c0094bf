// srhip_compile.h — the tree compiler (srhip_compile.cpp: host arithmetic on srhip_program's vectors, no
// HIP runtime call, no device): what the other units of libsrhip.so call.  Uploading what it compiled
// is theirs (srhip_host.cpp upload_program, srhip_optim.cpp compile_grad_program).
#pragma once
#include <stdint.h>

struct srhip_program;

namespace srhip {

// the evaluation program (+ its derived-column program) from P's trees; invalidates the gradient
// program and the launch order
int compile_program(srhip_program& P);

// P.gdspec / gdbase from the trees (once)
void grad_derived_spec(srhip_program& P);

// What compile_grad_host did to the gradient program, for the upload that follows it.
struct GradEdit {
  enum Kind {
    NONE,     // the program was ready: nothing to upload
    PATCHED,  // instructions [lo, hi) of gcode changed in place (hi <= lo: none), the rest is as uploaded
    FULL      // gcode and gprog_off were compiled anew
  } kind = NONE;
  int64_t lo = 0, hi = 0;  // PATCHED only
};
// The gradient program at P's current constants, host side: the trees whose constants moved since the
// last compile patched in place when a previous full compile is on the device, everything compiled in
// full otherwise (always so for a host-only program).  grad_ready is the uploader's to set.
int compile_grad_host(srhip_program& P, GradEdit& edit);
extern thread_local double g_patch_scan_s;  // its patch scans' time (SRHIP_OPTIM_TIMING), per thread

// Speculative slot `slot` := tree t at constants c[0 .. nconst) (get_constants order), host side;
// false if the tree cannot be instantiated.  *static_fail: did_succeed is false before any row is
// evaluated (a non-finite constant leaf or constant subtree; no evaluation needed).  [lo, hi) grows by the instructions written.
bool spec_instantiate(srhip_program& P, int32_t slot, int32_t t, const double* c, bool* static_fail, int64_t& lo,
                      int64_t& hi);

}  // namespace srhip
