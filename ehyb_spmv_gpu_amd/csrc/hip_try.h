// HIP_TRY(expr): a failed HIP call records its error (set_error) and returns EHYB_ERR_NO_DEVICE or EHYB_ERR_HIP from the calling
// C-ABI function.  (ehyb_comm.hip maps errors its own way.)
#pragma once
#include <hip/hip_runtime.h>

#include "ehyb_internal.h"

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::ehyb::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorNoDevice ? EHYB_ERR_NO_DEVICE : EHYB_ERR_HIP;                \
        }                                                                                     \
    } while (0)
