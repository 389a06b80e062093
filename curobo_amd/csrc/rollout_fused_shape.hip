// rollout_fused_shape.hip -- the instantiations of ONE compile-time shape of the fused trajectory launch and their launcher
// (fused_shapes.hpp).  curobo_amd/build.py compiles this file once per shape of the table (-DCUROBO_FUSED_SHAPE_TU=<id>, in
// parallel); curobo_amd/backends/fused_jit.py compiles it at run time for a shape given on the command line
// (-DCUROBO_FUSED_SHAPE_TU=99 -DCUROBO_FUSED_JIT_SHAPE=...).  The dispatch that calls the launchers is rollout_fused.hip.
#include "fused_device.hpp"

#if !defined(CUROBO_FUSED_SHAPE_TU) || !(CUROBO_FUSED_SHAPE_TU > 0)
#error "rollout_fused_shape.hip holds one shape: compile it with -DCUROBO_FUSED_SHAPE_TU=<shape id>"
#endif

namespace curobo_hip {

#define CUROBO_FUSED_CAT2(a, b) a##b
#define CUROBO_FUSED_CAT(a, b) CUROBO_FUSED_CAT2(a, b)
#define CUROBO_FUSED_CAT3_(a, b, c) a##b##c
#define CUROBO_FUSED_CAT3(a, b, c) CUROBO_FUSED_CAT3_(a, b, c)
int CUROBO_FUSED_CAT(fused_shape_launch_, CUROBO_FUSED_SHAPE_TU)(CUROBO_FUSED_SHAPE_LAUNCHER_PARAMS) {
  using SH = CUROBO_FUSED_CAT(CUROBO_FUSED_SHAPE_, CUROBO_FUSED_SHAPE_TU);
  if (!fused_shape_matches<SH>(a, threads)) return 0;
#define CUROBO_FUSED_SHAPE_KERNEL(DG, SW, KD, TM)                                                                      \
  if (deg == DG && sweep == SW && kinds == KD && terms == TM && (!(TM) || !SH::kPlain || fused_plain_terms(a))) {      \
    auto kfn = rollout_trajectory_fused_kernel<DG, SW, KD, TM, SH>;                                                    \
    if (batch <= 0) return 1; /* query only */                                                                         \
    *err = fused_launch(kfn, dim3((unsigned)batch), dim3(threads), lds, kFusedLdsUnasked, st, a);                      \
    return 1;                                                                                                          \
  }
  CUROBO_FUSED_CAT3(CUROBO_FUSED_SHAPE_, CUROBO_FUSED_SHAPE_TU, _KERNELS)(CUROBO_FUSED_SHAPE_KERNEL)
#undef CUROBO_FUSED_SHAPE_KERNEL
  return 0;
}
#ifdef CUROBO_FUSED_JIT_SHAPE
// entry points of a run-time compiled shape object (loaded by curobo_amd/backends/fused_jit.py, handed to
// curobo_hip_rollout_fused_register_shape): the launcher behind a C signature, and the size of the argument block so that an
// object built from other sources than the library's is refused
extern "C" __attribute__((visibility("default"))) int curobo_fused_jit_launch(const void *args, int deg, int sweep, int kinds, int terms,
                                                                               int batch, int threads, size_t lds, void *stream, int *err) {
  hipError_t e = hipSuccess;
  const int r = CUROBO_FUSED_CAT(fused_shape_launch_, CUROBO_FUSED_SHAPE_TU)(*static_cast<const FusedTrajArgs *>(args), deg, sweep, kinds,
                                                                             terms != 0, batch, threads, lds, (hipStream_t)stream, &e);
  *err = (int)e;
  return r;
}
extern "C" __attribute__((visibility("default"))) int curobo_fused_jit_args_bytes(void) { return (int)sizeof(FusedTrajArgs); }
#endif

}  // namespace curobo_hip
