// scan_fq.hpp -- the FLOAT model's recurrence with the integer model's per-step rounding.
//
// The integer recurrence (sparseRNNs fxpmodel.py:147-172) floors four products and the shifted Bu at every step.  On states
// that lie on the grid 2^-e that is, with F(v, e) = floor(v * 2^e) * 2^-e taken of the EXACT real v,
//   xr' = (F(ar * xr, er) - F(ai * xi, er)) + F(br, er)
//   xi' = (F(ar * xi, ei) + F(ai * xr, ei)) + F(bi, ei)
// which inside the domain (|x| * 2^e < 2^24, every v * 2^e a normal number or zero) is one exactly defined float32 function:
// the floored terms are grid values below 2^24 LSBs, so both sums are exact.  floatmodel.fq_scan states it in float64.
// The rounding makes the step non-associative, so this is a sequential scan: a lane owns one (sequence, state) pair for
// all its steps.
//
// Decomposition: lanes are the flattened (sequence, state) pairs, consecutive lanes consecutive states, so one step of a
// wave is 512 contiguous bytes of a row (at P = 32 of two sequences' rows).  One wave per workgroup spreads the few waves
// there are over the CUs (32 sequences at P = 64: 32 waves); no LDS, no barrier.  The chain of a lane is dependent from
// step to step, so HBM latency must not sit on it: Bu is loaded in register blocks of FQS_BLK steps and the next block is
// requested before the current block's chain starts.
//
// Addresses: bu and xs share one layout, so one 32-bit byte offset per lane and step-in-block serves both, against a scalar
// base that moves with the block; a full block costs no vector address arithmetic.  The entry refuses shapes whose offsets
// would not fit 32 bits (fqs_span_ok).  The last block of a lane clamps its load rows to the lane's last row and predicates
// its stores, so nothing past clamp(lens[b], 0, L) rows is read or written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace s5 {

struct ScanFqArgs {
    const float2 *lambda; // (P) complex64
    const float2 *bu;     // (B,L,P) complex64
    float2 *xs;           // (B,L,P)
    const float2 *x0;     // (B,P) state before the first step, or nullptr (zeros)
    float2 *x_last;       // (B,P) state after the last step, or nullptr
    const int32_t *lens;  // (B) device, or nullptr: every sequence runs L steps
    int32_t B, L, P;
    float sr, isr, si, isi; // 2^exp_re, 2^-exp_re, 2^exp_im, 2^-exp_im
};

constexpr int FQS_BLK = 16; // steps per register block: 16 float2 in flight behind the 16 the chain works on

// The lanes of a wave span at most 64 / P + 2 sequences; their byte offsets, relative to the wave's first sequence, must
// fit 32 bits.
inline bool fqs_span_ok(long long L, long long P)
{
    return (unsigned __int128)(64 / P + 2) * L * P * sizeof(float2) < ((unsigned __int128)1 << 32); // L * P alone may pass 2^62
}

// The translation unit is built with the compiler's default contraction, under which __fmul_rn is a plain product that the
// back end may fuse into the sum that consumes it.  An empty asm statement that claims to modify the value costs no
// instruction and ends that: a floored term is rounded as a product before it enters a sum.
__device__ __forceinline__ float fqs_pin(float v)
{
    asm("" : "+v"(v));
    return v;
}

// F(a * b, e) of the exact product: p is the rounded product, r its exact residual (a * b = p + r), and only the sign of r
// is used: floor(p * 2^e) is the floor of the exact product unless p * 2^e is an integer and the exact product lies below it.
__device__ __forceinline__ float fqs_floor_prod(float a, float b, float s, float is)
{
#pragma clang fp contract(off)
    const float p = __fmul_rn(a, b);
    const float r = __fmaf_rn(a, b, -p);
    const float t = __fmul_rn(p, s);
    float fl = floorf(t);
    if (fl == t && r < 0.f) fl = __fsub_rn(fl, 1.f);
    return fqs_pin(__fmul_rn(fl, is));
}

__device__ __forceinline__ float fqs_floor(float v, float s, float is)
{
#pragma clang fp contract(off)
    return fqs_pin(__fmul_rn(floorf(__fmul_rn(v, s)), is));
}

// The loads of one block.  fqs_load_full: all FQS_BLK rows are the lane's own.  fqs_load_clamped: the first n in 1..FQS_BLK
// are; a row past them re-reads the lane's last one, so there is no branch around a single load and no register array
// indexed by a variable.  fqs_load picks between them by a WAVE-UNIFORM test and predicates the clamped form as a whole:
// two per-lane alternatives that write the same registers would be serialised by the compiler, with a wait for every
// outstanding load between them -- which puts the memory latency of the block just requested in front of the chain.
__device__ __forceinline__ void fqs_load_full(float2 (&u)[FQS_BLK], const char *base, const uint32_t (&off)[FQS_BLK])
{
#pragma unroll
    for (int k = 0; k < FQS_BLK; ++k) u[k] = *reinterpret_cast<const float2 *>(base + off[k]);
}

__device__ __forceinline__ void fqs_load_clamped(float2 (&u)[FQS_BLK], const char *base, uint32_t off0, int n, uint32_t rowb)
{
#pragma unroll
    for (int k = 0; k < FQS_BLK; ++k) u[k] = *reinterpret_cast<const float2 *>(base + (off0 + (uint32_t)(k < n ? k : n - 1) * rowb));
}

// rows: how many rows from the block's first one on are the lane's own (<= 0: none, the lane loads nothing)
__device__ __forceinline__ void fqs_load(float2 (&u)[FQS_BLK], const char *base, const uint32_t (&off)[FQS_BLK], int rows,
                                         uint32_t rowb)
{
    if (__all(rows >= FQS_BLK)) fqs_load_full(u, base, off);
    else if (rows > 0) fqs_load_clamped(u, base, off[0], rows < FQS_BLK ? rows : FQS_BLK, rowb);
}

__device__ __forceinline__ void fqs_copy(float2 (&d)[FQS_BLK], const float2 (&u)[FQS_BLK])
{
#pragma unroll
    for (int k = 0; k < FQS_BLK; ++k) d[k] = u[k];
}

// One block of the chain.  !FULL: only the first n steps are the lane's own; the steps behind them are computed and dropped
// (straight-line code over the register block: no loop that would index it by a variable).
template <bool FULL>
__device__ __forceinline__ void fqs_chain(const float2 (&u)[FQS_BLK], char *base, const uint32_t (&off)[FQS_BLK], int n,
                                          float ar, float ai, float &xr, float &xi, const ScanFqArgs &a)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < FQS_BLK; ++k) {
        const float br = fqs_floor(u[k].x, a.sr, a.isr), bi = fqs_floor(u[k].y, a.si, a.isi);
        const float nr = __fadd_rn(__fsub_rn(fqs_floor_prod(ar, xr, a.sr, a.isr), fqs_floor_prod(ai, xi, a.sr, a.isr)), br);
        const float ni = __fadd_rn(__fadd_rn(fqs_floor_prod(ar, xi, a.si, a.isi), fqs_floor_prod(ai, xr, a.si, a.isi)), bi);
        if (FULL || k < n) {
            xr = nr;
            xi = ni;
            *reinterpret_cast<float2 *>(base + off[k]) = make_float2(xr, xi);
        }
    }
}

__global__ __launch_bounds__(64) void k_scan_fq_c64(ScanFqArgs a)
{
    const long long pairs = (long long)a.B * a.P;
    const long long g0 = (long long)blockIdx.x * 64, g = g0 + threadIdx.x;
    if (g >= pairs) return;
    const int b0 = (int)(g0 / a.P); // the wave's first sequence: uniform
    const int b = (int)(g / a.P), p = (int)(g - (long long)b * a.P);
    int len = a.L;
    if (a.lens) {
        const int raw = a.lens[b];
        len = raw < 0 ? 0 : raw > a.L ? a.L : raw;
    }
    const float ar = a.lambda[p].x, ai = a.lambda[p].y;
    float xr = 0.f, xi = 0.f;
    if (a.x0) {
        const float2 v = a.x0[(size_t)b * a.P + p];
        xr = v.x; xi = v.y;
    }
    const uint32_t rowb = (uint32_t)a.P * (uint32_t)sizeof(float2);
    const size_t seq0 = (size_t)b0 * a.L * a.P * sizeof(float2); // byte offset of the wave's first sequence
    const uint32_t lane_off = (uint32_t)(b - b0) * (uint32_t)a.L * rowb + (uint32_t)p * (uint32_t)sizeof(float2);
    uint32_t off[FQS_BLK];
#pragma unroll
    for (int k = 0; k < FQS_BLK; ++k) off[k] = lane_off + (uint32_t)k * rowb;
    const char *src = reinterpret_cast<const char *>(a.bu) + seq0;
    char *dst = reinterpret_cast<char *>(a.xs) + seq0;

    if (len == 0) { // nothing to run: the carry passes through
        if (a.x_last) a.x_last[(size_t)b * a.P + p] = make_float2(xr, xi);
        return;
    }
    float2 cur[FQS_BLK], nxt[FQS_BLK];
    fqs_load(cur, src, off, len, rowb);
    for (int t0 = 0; t0 < len; t0 += FQS_BLK) {
        const int tu = __builtin_amdgcn_readfirstlane(t0); // the same in every lane still in the loop: scalar block bases
        const char *ld = src + (size_t)(tu + FQS_BLK) * rowb;
        char *sd = dst + (size_t)tu * rowb;
        const int left = len - t0, ahead = left - FQS_BLK; // rows of this block and behind it
        fqs_load(nxt, ld, off, ahead, rowb); // request the next block before this block's chain starts
        // wave-uniform as well, and the hand-over of the next block inside either form: in the full form every store is
        // unconditional, so the wait for the next block's loads can count the 16 stores issued behind them and need not
        // wait for their acknowledgements
        if (__all(left >= FQS_BLK)) {
            fqs_chain<true>(cur, sd, off, FQS_BLK, ar, ai, xr, xi, a);
            if (ahead > 0) fqs_copy(cur, nxt);
        } else {
            fqs_chain<false>(cur, sd, off, left < FQS_BLK ? left : FQS_BLK, ar, ai, xr, xi, a);
            if (ahead > 0) fqs_copy(cur, nxt);
        }
    }
    if (a.x_last) a.x_last[(size_t)b * a.P + p] = make_float2(xr, xi);
}

} // namespace s5
