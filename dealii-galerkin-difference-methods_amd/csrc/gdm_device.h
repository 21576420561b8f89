// gdm_device.h -- address-space typedefs and wait macros shared by the device
// code of the stencil, the face kernels and the mass inverse.
#pragma once
#include <hip/hip_runtime.h>

namespace gdmk {

#define GDM_WAIT_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")
#define GDM_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Coefficient tables are read-only for the whole launch and indexed by
// wave-uniform positions: read them through the constant address space so
// they become scalar (s_load) loads instead of vector loads.
typedef __attribute__((address_space(4))) const double cdouble;
__device__ __forceinline__ cdouble *cptr(const double *p) { return (cdouble *)(p); }

typedef __attribute__((address_space(3))) double ldouble;
typedef __attribute__((address_space(3))) unsigned int lu32;
typedef double dpair __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) dpair ldouble2;

}  // namespace gdmk
