// float_model.hpp -- the FLOAT model's forward (synth.float_forward, calibrate_bn=False) as four tile kernels around the
// existing complex64 scan (scan_assoc.hpp): encoder, per layer B projection -> scan -> gate, decoder.  DESIGN.md §4r.
//
// Every contraction runs on v_mfma_f32_16x16x4_f32: exact float32, bit for bit a k-ordered fmaf chain.  A workgroup is four
// waves and walks 32-frame tiles (grid-stride); its slice of the weight matrix is loaded ONCE into registers as MFMA B operands
// (lane l holds W[4*ks + (l >> 4)][16*t + (l & 15)] for k-step ks of column tile t; wave w owns the column tiles w, w + 4, ...),
// the frame tile is staged through LDS and read as the A operand (lane l: row l & 15, k = 4*ks + (l >> 4)).  Two row tiles x NT
// column tiles give every wave at least two independent accumulators.  C/D layout: col = lane & 15, row = 4 * (lane >> 4) + reg.
//
// Observers: every kernel keeps a running max of |v| per lane as the value's bits with the sign cleared (non-negative floats
// order like their bits, and NaN bits lie above infinity's, so a NaN reaches the observer as np.abs(v).max() would give it),
// reduces it through the wave (shuffles) and the workgroup (LDS) and issues ONE atomicMax per observer per workgroup.  The
// array is only ever raised; a NULL array switches the observers off.  Rows beyond N and padded columns never enter.
//
// TRACE additionally stores the planes nothing downstream reads (u; y, g_in, g).  It changes no arithmetic: outputs and
// observers are bit-identical in the two modes.
//
// HIST (the k_*_hist kernels) additionally counts every value that enters an observer into that observer's
// histogram over the float32 exponent field: bin = clamp(E - 87, 0, 63), E = (bits >> 23) & 0xff, at the very statement where
// the value enters the observer, under the same masks.  Counts accumulate in LDS as 32-bit words, FM_HIST_COPIES private
// copies per workgroup chosen by the lane (a plane really uses two or three bins, so one copy would serialise a wave's
// 64 atomics on them; with 16 copies laid out [bin][copy] at most four lanes meet on a word and the copies of a bin lie in
// 16 different banks).  At the end of the kernel the copies are summed in 64 bits and every NON-ZERO sum is added to the
// global array with one 64-bit atomicAdd.  Wrap rule: a workgroup sees at most ceil(tiles / grid) * 32 rows * 272 values of
// one observer; the entry refuses (S5FXP_EBADARG) an N at which that reaches 2^32 (fm_hist_rows_ok), so no flush is needed
// before the end.
//
// CLIPS (the k_*_clips and k_*_clips_hist kernels) run n clips of different lengths, padded to Lmax rows each, in
// one launch: a tile belongs to one clip (FClipMap), holds the rows the clip has there and is skipped when it has none, so
// every clip gets bit for bit what the rectangular kernels give it alone and no padding row is read, written or observed.
//
// FQ (the k_*_fq and k_*_clips_fq kernels) fake-quantise chosen observed tensors: a site that is on replaces the
// value, right after it entered its observer, by q(v) = clamp(R(v 2^exp), lo, hi) 2^-exp (fm_fq: four VALU operations, none
// of which can be contracted).  The sites reach a kernel as one more by-value parameter, FFq<n>, so that no argument struct of
// the existing kernels grows.  Built without the histogram.
//
// The four kernels are written once, in float_model_kernels.inc, which this header includes once per form, six times: plain
// (k_fenc, k_fbproj, k_fgate, k_fdec), _hist, _clips, _clips_hist, _fq and _clips_fq.  A form is three preprocessor flags
// (FM_HIST, FM_CLIPS, FM_FAKEQ) and a name suffix; the .inc derives everything else from them and cleans up after itself.
// With all flags 0 the text is token for token the kernels as they were before any other form existed, so their instruction
// streams do not move.  The flags are preprocessor ones and not template parameters because both alternatives change the
// existing kernels: a template parameter changes their mangled names (and their kernarg layout, if the argument struct
// grows), and a shared __device__ body behind thin __global__ wrappers compiles to different code than the same text inside
// the kernel (measured: tools/disasm_compare.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace s5 {

typedef float fm_f32x4 __attribute__((ext_vector_type(4)));

constexpr int FM_FT = 32;       // frames per tile: two 16-row MFMA tiles
constexpr int FM_WAVES = 4;     // waves per workgroup
constexpr int FM_DIN = 257;     // encoder rows / decoder columns of the N-DNS recipe
constexpr int FM_KENC = 260;    // 257 zero-padded to a multiple of the MFMA's k = 4
constexpr int FM_MDEC = 272;    // 257 zero-padded to 17 column tiles
constexpr int FM_DEC_TILES = 17;

__device__ inline unsigned fm_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ inline unsigned fm_umax(unsigned a, unsigned b) { return a > b ? a : b; }
// np.maximum(v, 0): a NaN stays a NaN
__device__ inline float fm_relu(float v) { return v < 0.f ? 0.f : v; }
// the prenorm BatchNorm; explicit roundings, so that the B projection and the gate kernel rebuild the same bits
__device__ inline float fm_bn(float h, float mean, float istd, float sc, float bi)
{
    return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(h, mean), istd), sc), bi);
}

// one fake-quantisation site, prepared on the host: scale = 2^exp, inv_scale = 2^-exp, lo = -2^(bits-1), hi = 2^(bits-1) - 1
constexpr unsigned FM_FQF_ON = 1u, FM_FQF_NEAREST = 2u, FM_FQF_SATURATE = 4u;
struct FqSite {
    float scale, inv_scale, lo, hi;
    unsigned flags; // 0: the site is off
};
template <int N>
struct FFq {
    FqSite s[N];
};
// flags is a kernel argument, so the three tests are scalar branches.  The clamp is two compare-and-selects and not
// fmin / fmax / med3, which would swallow a NaN: both comparisons are false for one, so it passes.
__device__ inline float fm_fq(float v, const FqSite &s)
{
    if (!(s.flags & FM_FQF_ON)) return v;
    float t = __fmul_rn(v, s.scale);
    t = (s.flags & FM_FQF_NEAREST) ? rintf(t) : floorf(t);
    if (s.flags & FM_FQF_SATURATE) t = t < s.lo ? s.lo : t > s.hi ? s.hi : t;
    return __fmul_rn(t, s.inv_scale);
}

constexpr int FM_HIST_BINS = 64;   // S5FXP_FLOAT_HIST_BINS
constexpr int FM_HIST_EMIN = -40;  // S5FXP_FLOAT_HIST_EMIN: bin b in 1..62 holds 2^(b + EMIN) <= |v| < 2^(b + EMIN + 1)
#ifndef S5_FM_HIST_COPIES
#define S5_FM_HIST_COPIES 16       // -DS5_FM_HIST_COPIES=1 builds the single-copy arm of tools/bench_float_hist.py
#endif
constexpr int FM_HIST_COPIES = S5_FM_HIST_COPIES; // a power of two, at most 64
constexpr int fm_hist_words(int planes) { return planes * FM_HIST_BINS * FM_HIST_COPIES; }
// the most rows a launch of `grid` workgroups may walk with 32-bit LDS counters
constexpr bool fm_hist_rows_ok(long long tiles, long long grid)
{
    return (tiles + grid - 1) / grid <= 0xffffffffll / (FM_FT * FM_MDEC);
}
__device__ inline int fm_hist_bin(float v)
{
    const int e = (int)((__float_as_uint(v) >> 23) & 0xffu) - (127 + FM_HIST_EMIN);
    return e < 0 ? 0 : e > FM_HIST_BINS - 1 ? FM_HIST_BINS - 1 : e;
}
// one value into LDS plane `plane` of the workgroup's histograms
__device__ inline void fm_hist_add(unsigned *sh, int plane, float v)
{
    atomicAdd(sh + (plane * FM_HIST_BINS + fm_hist_bin(v)) * FM_HIST_COPIES + (threadIdx.x & (FM_HIST_COPIES - 1)), 1u);
}
// the workgroup's histograms: static LDS of the kernels that count, none in the others
template <int PLANES>
__device__ inline unsigned *fm_hist_lds()
{
    __shared__ unsigned sh[fm_hist_words(PLANES)];
    return sh;
}
template <int PLANES>
__device__ inline void fm_hist_zero(unsigned *sh)
{
    for (int i = threadIdx.x; i < fm_hist_words(PLANES); i += 256) sh[i] = 0u;
    __syncthreads();
}
// LDS plane i goes to row i of `hist`, or to row i + 1 from DUP_ROW on; plane DUP_SRC is added to row DUP_ROW as well
// (gate.l repeats out2.inp).  Only non-zero sums touch global memory.
template <int PLANES, int DUP_SRC = -1, int DUP_ROW = -1>
__device__ inline void fm_hist_flush(const unsigned *sh, unsigned long long *hist)
{
    __syncthreads();
    for (int i = threadIdx.x; i < PLANES * FM_HIST_BINS; i += 256) {
        unsigned long long n = 0;
#pragma unroll
        for (int c = 0; c < FM_HIST_COPIES; ++c) n += sh[i * FM_HIST_COPIES + c];
        if (n == 0) continue;
        const int plane = i / FM_HIST_BINS, bin = i - plane * FM_HIST_BINS;
        const int row = DUP_ROW >= 0 && plane >= DUP_ROW ? plane + 1 : plane;
        atomicAdd(hist + row * FM_HIST_BINS + bin, n);
        if (plane == DUP_SRC) atomicAdd(hist + DUP_ROW * FM_HIST_BINS + bin, n);
    }
}
constexpr int fm_lda(int K) { return (K + 31) / 32 * 32 + 4; } // row stride of an LDS tile: 16 rows x 4 k spread over the banks

// the wave's B operands: W is (4*KS, ldw) row-major, zero-padded, tiles = column tiles that exist
template <int KS, int NT>
__device__ inline void fm_load_w(float (&b)[NT][KS], const float *__restrict__ W, int ldw, int tiles)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = wave + FM_WAVES * nt;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            b[nt][ks] = t < tiles ? W[(size_t)(4 * ks + (lane >> 4)) * ldw + t * 16 + (lane & 15)] : 0.f;
    }
}

// acc[rt][nt] += A(rows 16*rt .. 16*rt+15 of the LDS tile) x the wave's column tile nt
template <int KS, int NT>
__device__ inline void fm_mma(fm_f32x4 (&acc)[2][NT], const float *A, int lda, const float (&b)[NT][KS], int tiles)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *a0 = A + (lane & 15) * lda + (lane >> 4);
    const float *a1 = a0 + 16 * lda;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[rt][nt] = fm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const float x0 = a0[4 * ks], x1 = a1[4 * ks];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            if (wave + FM_WAVES * nt < tiles) { // wave-uniform
                acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, b[nt][ks], acc[0][nt], 0, 0, 0);
                acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, b[nt][ks], acc[1][nt], 0, 0, 0);
            }
    }
}

// lanes -> waves -> workgroup -> one atomicMax per observer.  slots: FM_WAVES * NOBS words of LDS.
template <int NOBS>
__device__ inline void fm_obs_flush(const unsigned (&m)[NOBS], unsigned *slots, unsigned *stats)
{
    if (!stats) return; // uniform: a kernel argument
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NOBS; ++i) {
        unsigned v = m[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fm_umax(v, (unsigned)__shfl_xor((int)v, off));
        if (lane == 0) slots[wave * NOBS + i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NOBS) {
        unsigned v = slots[threadIdx.x];
#pragma unroll
        for (int w = 1; w < FM_WAVES; ++w) v = fm_umax(v, slots[w * NOBS + threadIdx.x]);
        atomicMax(stats + threadIdx.x, v);
    }
}

// the kernels' arguments (float_model_kernels.inc says what each kernel computes)
struct FEncArgs {
    const float *x;  // (N,257)
    const float *w;  // (260,H), rows 257..259 zero
    const float *b;  // (H)
    float *h;        // (N,H)
    unsigned *stats; // 2 words or NULL
    long long N;
};
struct FNormArgs {
    const float *mean, *istd, *scale, *bias; // (H) each; scale = 1 / bias = 0 where the model has none (exact)
};
struct FBprojArgs {
    const float *h; // (N,H) layer input
    FNormArgs nm;
    const float *bcat; // (H,2P)
    float *bu;         // (N,2P)
    float *u_trace;    // (N,H), TRACE only
    unsigned *stats;   // 3 words or NULL
    long long N;
};
struct FGateArgs {
    const float *xs; // (N,2P) raw states, complex64
    const float *h;  // (N,H) layer input
    FNormArgs nm;
    const float *ccat; // (2P,H)
    const float *D;    // (H)
    const float *w2;   // (H,H)
    const float *b2;   // (H)
    float *hout;       // (N,H)
    float *y_trace, *gin_trace, *g_trace; // (N,H) each, TRACE only
    unsigned *stats;   // 7 words or NULL
    long long N;
};
struct FDecArgs {
    const float *h;  // (N,H)
    const float *w;  // (H,272), columns 257..271 zero
    const float *b;  // (272)
    float *out;      // (N,257)
    unsigned *stats; // 2 words or NULL
    long long N;
};

// a clip-form launch: tile i of n * tpc belongs to clip i / tpc at t0 = 32 * (i % tpc), so no tile straddles two clips
struct FClipMap {
    const int *lens; // (n) device; clamped to 0..Lmax where it is read
    int Lmax, tpc;   // rows per clip of every plane; tpc = ceil(Lmax / 32)
    long long tiles; // n * tpc
};

// The six forms of the four kernels.  An inclusion states its three flags and its kernel-name suffix and nothing else; what
// follows from them is defined at the head of float_model_kernels.inc and undefined, the flags included, at its foot.
#define FM_HIST 0
#define FM_CLIPS 0
#define FM_FAKEQ 0
#define FM_KERNEL(name) name
#include "float_model_kernels.inc"

#define FM_HIST 1
#define FM_CLIPS 0
#define FM_FAKEQ 0
#define FM_KERNEL(name) name##_hist
#include "float_model_kernels.inc"

#define FM_HIST 0
#define FM_CLIPS 1
#define FM_FAKEQ 0
#define FM_KERNEL(name) name##_clips
#include "float_model_kernels.inc"

#define FM_HIST 1
#define FM_CLIPS 1
#define FM_FAKEQ 0
#define FM_KERNEL(name) name##_clips_hist
#include "float_model_kernels.inc"

#define FM_HIST 0
#define FM_CLIPS 0
#define FM_FAKEQ 1
#define FM_KERNEL(name) name##_fq
#include "float_model_kernels.inc"

#define FM_HIST 0
#define FM_CLIPS 1
#define FM_FAKEQ 1
#define FM_KERNEL(name) name##_clips_fq
#include "float_model_kernels.inc"

} // namespace s5
