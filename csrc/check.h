// Error-check macros for HIP and RCCL calls.
#pragma once

#include <c10/util/Exception.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#define CGX_HIP_CHECK(cmd)                                              \
  do {                                                                  \
    hipError_t e_ = (cmd);                                              \
    TORCH_CHECK(e_ == hipSuccess, "cgx HIP error: ", hipGetErrorString(e_)); \
  } while (0)

#define CGX_NCCL_CHECK(cmd)                                              \
  do {                                                                   \
    ncclResult_t r_ = (cmd);                                             \
    TORCH_CHECK(r_ == ncclSuccess, "cgx RCCL error: ", ncclGetErrorString(r_)); \
  } while (0)
