// mgx_host.h -- what the launchers of every translation unit share on the host side (not part of include/mgx.h).
#ifndef MGX_HOST_H
#define MGX_HOST_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mgx.h"
#include "mgx_env_rows.h"      // misaligned(), cell_bytes(), log2_of(): no HIP needed

extern "C" void mgx_internal_set_hip_error(int e);      // mgx_kernels.hip: what mgx_last_hip_error() reports

namespace mgx {

// behind every kernel launch: the launch's error, read off HIP's sticky state (mgx_kernels.hip: hip_failed has the why)
inline int finish_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { mgx_internal_set_hip_error((int)e); return MGX_ERR_LAUNCH; }
    return MGX_OK;
}

}  // namespace mgx

#endif
