// jm_error.h -- error plumbing of the C ABI, shared by the translation units of a topology library: the thread-local
// message behind `jm_last_error`, `fail` and `HIP_TRY`.  The message is one object per library (a C++17 inline variable);
// it and `fail` are hidden, so that two topology libraries in one process never share them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/jiminy_hip.h"

__attribute__((visibility("hidden"))) inline thread_local std::string g_last_error;

__attribute__((visibility("hidden"))) inline int32_t fail(int32_t code, const std::string & msg)
{
    g_last_error = msg;
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do                                                                                             \
    {                                                                                              \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(JM_ERUNTIME, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)
