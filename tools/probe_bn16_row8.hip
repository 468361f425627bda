// probe_bn16_row8.hip -- the row-layout BatchNorm chain (mfma_bn.hpp bn16_row8) against bn16_x4, exhaustively: all 65 536
// input values x every shift pattern an arm admits (shx1 0..14, r1 0..31, rs2 0..31, change_cfg by -15..14) x per-channel
// constants on both rails, at zero and in between, plus the boundary patterns the short arms must reject (other widths, a
// left shift of the sum, shifts one past the packed forms' reach), which must select ROW_GENERIC and still agree.
// tests/test_gate_urec.py builds and runs it:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe_bn16_row8.hip -o tools/bin/probe_bn16_row8
// Prints one line per arm "<arm> patterns <n> evaluations <n> mismatches <n>" and "rejections wrong: <n>"; exit status 1 on any
// mismatch, wrong selection or an arm that was never reached.
#include "../sparsernns_amd/csrc/mfma_bn.hpp"
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)

using namespace s5;

struct Pat {
    int8_t xb, b1, b2, cbits, shx1, post1, rs2, de;
};
constexpr int NCONST = 16; // (mean, isv) pairs: two row vectors of eight channels

__global__ __launch_bounds__(256) void k_probe(const Pat *pats, int npat, const int32_t *mean, const int32_t *isv, unsigned long long *count,
                                               unsigned long long *bad)
{
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 32768; // every int16 value
    unsigned long long n[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    for (int ip = blockIdx.y; ip < npat; ip += gridDim.y) {
        const Pat q = pats[ip];
        // an input stored within its bits, as the kernels find it
        const int32_t hi = (1 << (q.xb - 1)) - 1, xv = x > hi ? hi : (x < ~hi ? ~hi : x);
        Bn16 ref{};
        ref.m1 = mean; ref.isv = isv; ref.sc = mean; ref.b4 = mean;
        ref.shx1 = q.shx1; ref.l1 = q.post1 > 0 ? q.post1 : 0; ref.r1 = q.post1 < 0 ? -q.post1 : 0; ref.b1 = q.b1; ref.xb = q.xb;
        ref.rs2 = q.rs2; ref.b2 = q.b2;
        ref.cl = q.de > 0 ? q.de : 0; ref.cr = q.de < 0 ? -q.de : 0; ref.cbits = q.cbits;
        ref.sxb = sat_bounds(q.xb); ref.s1 = sat_bounds(q.b1); ref.s2 = sat_bounds(q.b2); ref.scb = sat_bounds(q.cbits);
        Bn16Row row;
        bn16_row_shifts(row, q.xb, 16, 16, q.b1, q.b2, q.cbits, q.shx1, q.post1, q.rs2, q.de);
        const uint32_t xp = ((uint32_t)xv & 0xffffu) * 0x10001u;
        const v4i xin = {(int)xp, (int)xp, (int)xp, (int)xp};
#pragma unroll
        for (int h0 = 0; h0 < NCONST; h0 += 8) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                row.m[k] = ((uint32_t)mean[h0 + 2 * k] & 0xffffu) | ((uint32_t)mean[h0 + 2 * k + 1] << 16);
                row.iv[k] = ((uint32_t)isv[h0 + 2 * k] & 0xffffu) | ((uint32_t)isv[h0 + 2 * k + 1] << 16);
            }
            v4i got;
            if (row.arm == ROW_PACKED) got = bn16_row8<ROW_PACKED>(row, xin);
            else if (row.arm == ROW_SHIFTED) got = bn16_row8<ROW_SHIFTED>(row, xin);
            else got = bn16_row8<ROW_GENERIC>(row, xin);
            const int32_t x4[4] = {xv, xv, xv, xv};
            int32_t t[4], u[8];
            bn16_x4(ref, x4, h0, t, reinterpret_cast<int32_t(&)[4]>(u[0]));
            bn16_x4(ref, x4, h0 + 4, t, reinterpret_cast<int32_t(&)[4]>(u[4]));
            const v2i p0 = pack4_i16(u[0], u[1], u[2], u[3]), p1 = pack4_i16(u[4], u[5], u[6], u[7]);
            n[row.arm] += 8;
            b[row.arm] += (got[0] != p0[0]) + (got[1] != p0[1]) + (got[2] != p1[0]) + (got[3] != p1[1]);
        }
    }
    for (int a = 0; a < 3; ++a) {
        if (n[a]) atomicAdd(count + a, n[a]);
        if (b[a]) atomicAdd(bad + a, b[a]);
    }
}

int main()
{
    std::vector<Pat> pats;
    unsigned long long npat[3] = {0, 0, 0};
    int wrong = 0;
    auto add = [&](int xb, int b1, int b2, int cbits, int shx1, int post1, int rs2, int de, int want) {
        const int l1 = post1 > 0 ? post1 : 0, r1 = post1 < 0 ? -post1 : 0, cl = de > 0 ? de : 0, cr = de < 0 ? -de : 0;
        const int arm = bn16_row_arm(xb, 16, 16, b1, b2, cbits, shx1, l1, r1, cl, cr);
        if (want >= 0 && arm != want) ++wrong;
        ++npat[arm];
        pats.push_back(Pat{(int8_t)xb, (int8_t)b1, (int8_t)b2, (int8_t)cbits, (int8_t)shx1, (int8_t)post1, (int8_t)rs2, (int8_t)de});
    };
    // everything the two short arms admit
    for (int shx1 = 0; shx1 <= 14; ++shx1)
        for (int r1 = 0; r1 <= 31; ++r1)
            for (int rs2 = 0; rs2 <= 31; ++rs2)
                for (int de = -15; de <= 14; ++de) add(16, 16, 16, 16, shx1, -r1, rs2, de, r1 ? ROW_SHIFTED : ROW_PACKED);
    // a narrower stored input is admitted unshifted only
    for (int xb : {8, 15})
        for (int r1 : {0, 1, 3})
            for (int rs2 : {0, 6, 14}) {
                for (int de : {-6, 0, 4}) add(xb, 16, 16, 16, 0, -r1, rs2, de, r1 ? ROW_SHIFTED : ROW_PACKED);
                add(xb, 16, 16, 16, 1, -r1, rs2, -1, ROW_GENERIC);
            }
    // the boundaries: one past each limit, and every other width
    for (int r1 : {0, 1, 2, 5})
        for (int rs2 : {0, 5, 9, 15, 31}) {
            add(16, 16, 16, 16, 15, -r1, rs2, -2, ROW_GENERIC);   // shx1 = 15: 2^15 is no positive int16 multiplier
            add(16, 16, 16, 16, 3, -r1, rs2, 15, ROW_GENERIC);    // cl = 15
            add(16, 16, 16, 16, 3, -r1, rs2, -16, ROW_GENERIC);   // cr = 16: beyond the packed shift
            add(16, 16, 16, 16, 3, -r1, rs2, -20, ROW_GENERIC);
            for (int w : {8, 12, 15}) {
                add(16, w, 16, 16, 2, -r1, rs2, -3, ROW_GENERIC);
                add(16, 16, w, 16, 2, -r1, rs2, 2, ROW_GENERIC);
                add(16, 16, 16, w, 2, -r1, rs2, 1, ROW_GENERIC);
                add(w, w, w, w, 0, -r1, rs2, 0, ROW_GENERIC);
            }
        }
    for (int l1 : {1, 2, 7, 14})   // a left shift of the sum
        for (int shx1 : {0, 1, 6})
            for (int rs2 : {0, 7, 13})
                for (int de : {-5, 0, 3}) add(16, 16, 16, 16, shx1, l1, rs2, de, ROW_GENERIC);

    const int32_t rails[4] = {-32768, 0, 32767, 1};
    std::vector<int32_t> mean(NCONST), isv(NCONST);
    for (int i = 0; i < NCONST; ++i) { mean[i] = rails[i & 3]; isv[i] = rails[i >> 2]; }
    // (the last row of the grid: typical operands instead of isv = 1 against every mean)
    const int32_t tm[4] = {-3277, 1234, -17, 20000}, ti[4] = {64, 91, 52, 23170};
    for (int i = 0; i < 4; ++i) { mean[12 + i] = tm[i]; isv[12 + i] = ti[i]; }

    Pat *dp; int32_t *dm, *di; unsigned long long *dc;
    CK(hipMalloc(&dp, pats.size() * sizeof(Pat))); CK(hipMalloc(&dm, NCONST * 4)); CK(hipMalloc(&di, NCONST * 4)); CK(hipMalloc(&dc, 48));
    CK(hipMemcpy(dp, pats.data(), pats.size() * sizeof(Pat), hipMemcpyHostToDevice));
    CK(hipMemcpy(dm, mean.data(), NCONST * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(di, isv.data(), NCONST * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dc, 0, 48));
    hipLaunchKernelGGL(k_probe, dim3(256, 32), dim3(256), 0, 0, dp, (int)pats.size(), dm, di, dc, dc + 3);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    unsigned long long res[6];
    CK(hipMemcpy(res, dc, 48, hipMemcpyDeviceToHost));
    const char *names[3] = {"ROW_GENERIC", "ROW_PACKED", "ROW_SHIFTED"};
    int rc = wrong ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        printf("%-12s patterns %llu evaluations %llu mismatches %llu\n", names[a], npat[a], res[a], res[3 + a]);
        if (res[3 + a] || !res[a]) rc = 1;
    }
    printf("rejections wrong: %d\n", wrong);
    return rc;
}
