// probe_resid_u16.hip -- the residual add's aligned sum as a uint16 (mfma_bn.hpp SumU16, resolve_u16) against the scalar
// add_cb_apply + ReLU (fxp_prims.hpp), exhaustively:
//   SUM      sum_u16_pair on all 65 536 z x all 32 768 skip >= 0 x the 31 operand shift pairs (shx, 0), shx = 0..15, and
//            (0, shy), shy = 1..15, plus shifts of 16 (the widest the plan admits), against max(sat16(z << shx) + sat16(skip << shy), 0) as
//            add_cb_apply forms it (post = 0, 32-bit result); the two halves of a pair carry different operands and each
//            half sees every (z, skip);
//   RESOLVE  resolve_u16 on all 65 536 U x post = -31..31 against relu(add_cb_apply) of an already aligned sum;
//   CHAIN    resolve_u16(sum_u16_pair(z, skip)) against relu(add_cb_apply(z, skip)) with 16-bit operands and result on all z x
//            346 skip values (every 95th and both rails) x the same 33 shift pairs x post = -31..15, the range the plan admits
//            (s5fxp_fast.hpp: res_exp >= 0).
// tests/test_resid_fold.py builds and runs it:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_resid_u16.hip -o tools/bin/probe_resid_u16
// Prints "<part> evaluations <n> mismatches <n>" per part; exit status 1 on any mismatch or a part that did not run.
#include "../sparsernns_amd/csrc/mfma_bn.hpp"
#include <cstdio>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)

using namespace s5;

constexpr int NPAIR = 33;
__device__ __forceinline__ void shift_pair(int i, int &shx, int &shy)
{
    shx = i < 16 ? i : 0;
    shy = i >= 16 && i < 31 ? i - 15 : 0;
    if (i == 31) shx = 16;
    if (i == 32) shy = 16;
}
__device__ __forceinline__ int32_t ref_sum(int32_t z, int32_t s, int shx, int shy)
{
    const int32_t t = add_cb_apply(z, 16, s, 16, AddCb{shx, shy, 0, 0}, 32);
    return t < 0 ? 0 : t;
}
__device__ __forceinline__ int32_t ref_h(int32_t z, int32_t s, int shx, int shy, int post)
{
    const int32_t t = add_cb_apply(z, 16, s, 16, AddCb{shx, shy, post, 0}, 16);
    return t < 0 ? 0 : t;
}

constexpr int SUM_CHUNKS = 64; // gridDim.y: 512 skip values each
__global__ __launch_bounds__(256) void k_sum(unsigned long long *count, unsigned long long *bad)
{
    const int z0 = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 32768; // every int16 value; the high half takes another one
    const int z1 = (int)(int16_t)(uint16_t)((z0 * 40503) ^ 0x5aa5);
    const uint32_t zp = ((uint32_t)z0 & 0xffffu) | ((uint32_t)z1 << 16);
    unsigned long long n = 0, b = 0;
    for (int ip = 0; ip < NPAIR; ++ip) {
        int shx, shy;
        shift_pair(ip, shx, shy);
        const SumU16 p = sum_u16_setup(shx, shy);
        const int s_lo = blockIdx.y * (32768 / SUM_CHUNKS);
        for (int s = s_lo; s < s_lo + 32768 / SUM_CHUNKS; ++s) {
            const int s1 = 32767 - s; // the high half walks the skip values from the other end: both halves see all of them
            const uint32_t got = sum_u16_pair(p, zp, (uint32_t)s | ((uint32_t)s1 << 16));
            b += (got & 0xffffu) != (uint32_t)ref_sum(z0, s, shx, shy);
            b += (got >> 16) != (uint32_t)ref_sum(z1, s1, shx, shy);
            n += 2;
        }
    }
    atomicAdd(count, n);
    if (b) atomicAdd(bad, b);
}

__global__ __launch_bounds__(256) void k_resolve(unsigned long long *count, unsigned long long *bad)
{
    const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x); // every uint16 value
    const SatB so = sat_bounds(16);
    unsigned long long n = 0, b = 0;
    for (int post = -31; post <= 31; ++post) {
        const int32_t got = resolve_u16(u, post > 0 ? post : 0, post < 0 ? -post : 0, so);
        const int32_t t = add_cb_apply(u, 16, 0, 16, AddCb{0, 0, post, 0}, 16); // shx = shy = 0: the operands are not clipped
        b += got != (t < 0 ? 0 : t);
        ++n;
    }
    atomicAdd(count, n);
    if (b) atomicAdd(bad, b);
}

constexpr int CHAIN_SKIPS = 346;
__global__ __launch_bounds__(256) void k_chain(unsigned long long *count, unsigned long long *bad)
{
    const int z = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 32768;
    const SatB so = sat_bounds(16);
    unsigned long long n = 0, b = 0;
    int shx, shy;
    shift_pair(blockIdx.y, shx, shy);
    const SumU16 p = sum_u16_setup(shx, shy);
    for (int is = 0; is < CHAIN_SKIPS; ++is) {
        const int s = is == CHAIN_SKIPS - 1 ? 32767 : 95 * is; // 0, 95, ..., 32 680, 32 767
        const int32_t u = (int32_t)(sum_u16_pair(p, (uint32_t)z & 0xffffu, (uint32_t)s) & 0xffffu);
        for (int post = -31; post <= 15; ++post) {
            b += resolve_u16(u, post > 0 ? post : 0, post < 0 ? -post : 0, so) != ref_h(z, s, shx, shy, post);
            ++n;
        }
    }
    atomicAdd(count, n);
    if (b) atomicAdd(bad, b);
}

int main()
{
    unsigned long long *dc;
    CK(hipMalloc(&dc, 48));
    CK(hipMemset(dc, 0, 48));
    hipLaunchKernelGGL(k_sum, dim3(256, SUM_CHUNKS), dim3(256), 0, 0, dc, dc + 3);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_resolve, dim3(256), dim3(256), 0, 0, dc + 1, dc + 4);
    CK(hipGetLastError());
    hipLaunchKernelGGL(k_chain, dim3(256, NPAIR), dim3(256), 0, 0, dc + 2, dc + 5);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    unsigned long long res[6];
    CK(hipMemcpy(res, dc, 48, hipMemcpyDeviceToHost));
    const char *names[3] = {"SUM", "RESOLVE", "CHAIN"};
    const unsigned long long want[3] = {2 * 65536ull * 32768 * NPAIR, 65536ull * 63, 65536ull * CHAIN_SKIPS * NPAIR * 47};
    int rc = 0;
    for (int a = 0; a < 3; ++a) {
        printf("%-8s evaluations %llu mismatches %llu\n", names[a], res[a], res[3 + a]);
        if (res[3 + a] || res[a] != want[a]) rc = 1;
    }
    return rc;
}
