// The one declaration of the error setter api.hip defines: records "<where>: <what>" for mmpl_last_error() (thread-local), returns 1.
#pragma once
int mmpl_set_error(const char* where, const char* what);
// Leaves the calling entry point with that error when a HIP call fails.
#define MMPL_HIP_TRY(expr, where)                                                  \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess) return mmpl_set_error(where, hipGetErrorString(e__));   \
  } while (0)
