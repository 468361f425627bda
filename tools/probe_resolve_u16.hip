// probe_resolve_u16.hip -- the packed resolve of the residual add's aligned sum (mfma_bn.hpp resolve_u16_pair)
// against the scalar resolve_u16, exhaustively:
//   PAIR     resolve_u16_pair<RES_GENERIC> on all 65 536 U x post = -31..15 (the range the plan admits: res_exp >= 0), both
//            halves of the pair, which carry different values of U;
//   RIGHT    resolve_u16_pair<RES_RIGHT> on all U x every post resolve_u16_setup gives that arm (-15..0), both halves; the
//            arm is also checked to be RES_RIGHT for exactly those shifts.
// tests/test_resid_lazy.py builds and runs it:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_resolve_u16.hip -o tools/bin/probe_resolve_u16
// Prints "<part> evaluations <n> mismatches <n>" per part; exit status 1 on any mismatch or a part that did not run.
#include "../sparsernns_amd/csrc/mfma_bn.hpp"
#include <cstdio>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)

using namespace s5;

__global__ __launch_bounds__(256) void k_pair(unsigned long long *count, unsigned long long *bad)
{
    const uint32_t u0 = blockIdx.x * blockDim.x + threadIdx.x; // every uint16 value; the high half takes another one
    const uint32_t u1 = ((u0 * 40503u) ^ 0x5aa5u) & 0xffffu;   // (an odd multiplier: a bijection of the 65 536 values)
    const SatB so = sat_bounds(16);
    unsigned long long n[2] = {0, 0}, b[2] = {0, 0};
    for (int post = -31; post <= 15; ++post) {
        const ResolveU16 p = resolve_u16_setup(post);
        const int lsh = post > 0 ? post : 0, rsh = post < 0 ? -post : 0;
        const uint32_t w0 = (uint32_t)resolve_u16((int32_t)u0, lsh, rsh, so), w1 = (uint32_t)resolve_u16((int32_t)u1, lsh, rsh, so);
        const uint32_t got = resolve_u16_pair<RES_GENERIC>(p, u0 | (u1 << 16));
        b[0] += (got & 0xffffu) != w0;
        b[0] += (got >> 16) != w1;
        n[0] += 2;
        const bool right = post <= 0 && post >= -15;
        b[1] += (p.arm == RES_RIGHT) != right; // (counted as a mismatch of the RIGHT part)
        if (p.arm == RES_RIGHT) {
            const uint32_t gr = resolve_u16_pair<RES_RIGHT>(p, u0 | (u1 << 16));
            b[1] += (gr & 0xffffu) != w0;
            b[1] += (gr >> 16) != w1;
            n[1] += 2;
        }
    }
    atomicAdd(count, n[0]);
    atomicAdd(count + 1, n[1]);
    if (b[0]) atomicAdd(bad, b[0]);
    if (b[1]) atomicAdd(bad + 1, b[1]);
}

int main()
{
    unsigned long long *dc;
    CK(hipMalloc(&dc, 32));
    CK(hipMemset(dc, 0, 32));
    hipLaunchKernelGGL(k_pair, dim3(256), dim3(256), 0, 0, dc, dc + 2);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    unsigned long long res[4];
    CK(hipMemcpy(res, dc, 32, hipMemcpyDeviceToHost));
    const char *names[2] = {"PAIR", "RIGHT"};
    const unsigned long long want[2] = {2 * 65536ull * 47, 2 * 65536ull * 16};
    int rc = 0;
    for (int a = 0; a < 2; ++a) {
        printf("%-8s evaluations %llu mismatches %llu\n", names[a], res[a], res[2 + a]);
        if (res[2 + a] || res[a] != want[a]) rc = 1;
    }
    return rc;
}
