// probe_lds_budget.hip -- up to how many bytes of LDS per workgroup do FIVE three-wave, 128-register workgroups share a CU?
// (diagnostic, not shipped; the fold gate kernel's budget, s5fxp_fast.hpp GATE_FOLD_LDS_5WG)
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_lds_budget.hip -o probe_lds_budget && ./probe_lds_budget
// Every workgroup spins for a fixed number of cycles; 5 x (number of CUs) workgroups are launched; where they all fit the launch
// takes one spin, otherwise two.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

__global__ __launch_bounds__(192) void k_spin(int *out, long long cycles)
{
    extern __shared__ int lds[];
    asm volatile("v_mov_b32 v127, 0" ::: "v127"); // 128 registers, as the gate kernel
    lds[threadIdx.x] = threadIdx.x;
    const long long t0 = __builtin_readcyclecounter();
    while (__builtin_readcyclecounter() - t0 < cycles) __builtin_amdgcn_s_sleep(8);
    if (lds[threadIdx.x] == -1) out[0] = 1;
}

int main()
{
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    int *out; CK(hipMalloc(&out, 64));
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_spin), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const long long cycles = 100000;
    const int sizes[] = {31328, 31712, 31744, 32000, 32004, 32256, 32768, 33280, 40960};
    printf("%d CUs, %d workgroups of 192 threads per launch\n", cus, 5 * cus);
    for (int bytes : sizes) {
        hipLaunchKernelGGL(k_spin, dim3(5 * cus), dim3(192), bytes, 0, out, cycles);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_spin, dim3(5 * cus), dim3(192), bytes, 0, out, cycles);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        printf("LDS %6d bytes per workgroup: %7.1f us\n", bytes, ms * 1e3);
    }
    return 0;
}
