// wave_fence.h -- where the lanes of ONE wavefront meet between two phases that hand data to each other through LDS or through the
// wavefront's own global writes: a wavefront barrier between wavefront-scope fences (no s_barrier: the other wavefronts of the workgroup
// are not waited for).  Shared by the evaluator (evalstate_device.h), K6 (trad_kernel.hip) and K8 (rave_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace gmk {

__device__ __forceinline__ void wave_phase_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace gmk
