// dyn_lds.h -- the one place that raises a kernel's dynamic-LDS limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// A launch of fn with `bytes` of dynamic LDS: every kernel may use 64 KiB, above
// that the limit is raised first (up to the 160 KiB of a gfx950 workgroup).
// Returns a hipError_t as an int (HIPCHK takes it).
static inline int set_dyn_lds(const void* fn, size_t bytes) {
    if (bytes <= 64 * 1024) return (int)hipSuccess;
    return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
