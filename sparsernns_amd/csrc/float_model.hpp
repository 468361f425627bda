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

// ------------------------------------------------------------------------------------------------------------------
// encoder: h = relu(x W + b); observers [0] encoder.inp, [1] encoder.out (before the ReLU)
// ------------------------------------------------------------------------------------------------------------------
struct FEncArgs {
    const float *x;  // (N,257)
    const float *w;  // (260,H), rows 257..259 zero
    const float *b;  // (H)
    float *h;        // (N,H)
    unsigned *stats; // 2 words or NULL
    long long N;
};

template <int DS>
__global__ __launch_bounds__(256) void k_fenc(FEncArgs a)
{
    constexpr int H = 48 * DS, HT = 3 * DS, NT = (HT + 3) / 4, KS = FM_KENC / 4, LDA = fm_lda(FM_KENC);
    __shared__ float sx[FM_FT * LDA];
    __shared__ unsigned sobs[FM_WAVES * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float breg[NT][KS];
    fm_load_w<KS, NT>(breg, a.w, H, HT);
    float bias[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = wave + FM_WAVES * nt;
        bias[nt] = t < HT ? a.b[t * 16 + (lane & 15)] : 0.f;
    }
    unsigned om[2] = {0u, 0u};
    const long long tiles = (a.N + FM_FT - 1) / FM_FT;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r0 = tile * FM_FT;
        const int rows = (int)(a.N - r0 < FM_FT ? a.N - r0 : FM_FT);
        // rows are 257 floats: dword loads, all of a thread's issued before the first is used.  Addresses are clamped into the
        // tile's valid rows and columns, so no load is conditional; what lies outside is replaced by zero afterwards.
        const float *src = a.x + (size_t)r0 * FM_DIN;
        constexpr int PER = (FM_FT * FM_KENC + 255) / 256;
        float v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + 256 * j, r = i / FM_KENC, c = i - r * FM_KENC;
            const int rc = r < rows ? r : rows - 1, cc = c < FM_DIN ? c : FM_DIN - 1;
            v[j] = src[(size_t)rc * FM_DIN + cc];
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + 256 * j, r = i / FM_KENC, c = i - r * FM_KENC;
            if (i >= FM_FT * FM_KENC) continue; // the last round is partial: 8320 = 32.5 x 256
            const bool ok = r < rows && c < FM_DIN;
            const float w = ok ? v[j] : 0.f;
            if (ok) om[0] = fm_umax(om[0], fm_absbits(w));
            sx[r * LDA + c] = w;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS, NT>(acc, sx, LDA, breg, HT);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= HT) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows) continue;
                    const float v = __fadd_rn(acc[rt][nt][r], bias[nt]);
                    om[1] = fm_umax(om[1], fm_absbits(v));
                    a.h[(size_t)(r0 + row) * H + t * 16 + (lane & 15)] = fm_relu(v);
                }
            }
        __syncthreads();
    }
    fm_obs_flush<2>(om, sobs, a.stats);
}

// ------------------------------------------------------------------------------------------------------------------
// B projection: u = BatchNorm(h); Bu = u B_bar^T as ONE real product against bcat (H, 2P) whose columns interleave re and
// im, so the result is the (N,P) complex64 plane the scan takes.  Observers [0] u, [1] Bu_re, [2] Bu_im.
// ------------------------------------------------------------------------------------------------------------------
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

template <int DS, bool TRACE>
__global__ __launch_bounds__(256) void k_fbproj(FBprojArgs a)
{
    constexpr int H = 48 * DS, P2 = 64 * DS, PT = 4 * DS, NT = DS, KS = H / 4, LDA = fm_lda(H);
    __shared__ float su[FM_FT * LDA];
    __shared__ float snm[4 * H];
    __shared__ unsigned sobs[FM_WAVES * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float breg[NT][KS];
    fm_load_w<KS, NT>(breg, a.bcat, P2, PT);
    for (int i = threadIdx.x; i < H; i += 256) {
        snm[i] = a.nm.mean[i]; snm[H + i] = a.nm.istd[i]; snm[2 * H + i] = a.nm.scale[i]; snm[3 * H + i] = a.nm.bias[i];
    }
    __syncthreads();
    unsigned om_u = 0u, om_bu = 0u; // a lane's Bu columns all have the lane's parity: even = re, odd = im
    const long long tiles = (a.N + FM_FT - 1) / FM_FT;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r0 = tile * FM_FT;
        const int rows = (int)(a.N - r0 < FM_FT ? a.N - r0 : FM_FT);
        for (int i = threadIdx.x; i < FM_FT * (H / 4); i += 256) {
            const int r = i / (H / 4), c = (i - r * (H / 4)) * 4;
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) {
                const float4 h = *reinterpret_cast<const float4 *>(a.h + (size_t)(r0 + r) * H + c);
                u.x = fm_bn(h.x, snm[c], snm[H + c], snm[2 * H + c], snm[3 * H + c]);
                u.y = fm_bn(h.y, snm[c + 1], snm[H + c + 1], snm[2 * H + c + 1], snm[3 * H + c + 1]);
                u.z = fm_bn(h.z, snm[c + 2], snm[H + c + 2], snm[2 * H + c + 2], snm[3 * H + c + 2]);
                u.w = fm_bn(h.w, snm[c + 3], snm[H + c + 3], snm[2 * H + c + 3], snm[3 * H + c + 3]);
                om_u = fm_umax(fm_umax(fm_umax(om_u, fm_absbits(u.x)), fm_umax(fm_absbits(u.y), fm_absbits(u.z))), fm_absbits(u.w));
                if (TRACE) *reinterpret_cast<float4 *>(a.u_trace + (size_t)(r0 + r) * H + c) = u;
            }
            *reinterpret_cast<float4 *>(su + r * LDA + c) = u;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS, NT>(acc, su, LDA, breg, PT);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt; // < PT always: PT = 4 * NT
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows) continue;
                    const float v = acc[rt][nt][r];
                    om_bu = fm_umax(om_bu, fm_absbits(v));
                    a.bu[(size_t)(r0 + row) * P2 + t * 16 + (lane & 15)] = v;
                }
            }
        __syncthreads();
    }
    const unsigned om[3] = {om_u, (lane & 1) ? 0u : om_bu, (lane & 1) ? om_bu : 0u};
    fm_obs_flush<3>(om, sobs, a.stats);
}

// ------------------------------------------------------------------------------------------------------------------
// gate: complex ReLU on the raw states, y = 2 (x_re C_re^T - x_im C_im^T) + D u as ONE real product of the interleaved
// rectified states against ccat (2P,H) = rows (C_re^T, -C_im^T) interleaved, with u rebuilt from the layer input;
// x1 = relu(y), g_in = x1 W2 + b2, g = sigmoid(g_in), h' = relu(x1 g + h).
// Observers [0] x_re, [1] x_im (raw states), [2] y, [3] out2.inp, [4] out2.out, [5] gate.l (= out2.inp), [6] gate.r.
// ------------------------------------------------------------------------------------------------------------------
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

template <int DS, bool TRACE>
__global__ __launch_bounds__(256) void k_fgate(FGateArgs a)
{
    constexpr int H = 48 * DS, P = 32 * DS, P2 = 64 * DS, HT = 3 * DS, NT = (HT + 3) / 4, KS1 = P2 / 4, KS2 = H / 4;
    constexpr int LD1 = fm_lda(P2), LDH = fm_lda(H);
    __shared__ float sxs[FM_FT * LD1];
    __shared__ float sh[FM_FT * LDH];
    __shared__ float sx1[FM_FT * LDH];
    __shared__ float spar[6 * H]; // mean, istd, scale, bias, D, b2
    __shared__ unsigned sobs[FM_WAVES * 7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float bc[NT][KS1], bw[NT][KS2];
    fm_load_w<KS1, NT>(bc, a.ccat, H, HT);
    fm_load_w<KS2, NT>(bw, a.w2, H, HT);
    for (int i = threadIdx.x; i < H; i += 256) {
        spar[i] = a.nm.mean[i]; spar[H + i] = a.nm.istd[i]; spar[2 * H + i] = a.nm.scale[i]; spar[3 * H + i] = a.nm.bias[i];
        spar[4 * H + i] = a.D[i]; spar[5 * H + i] = a.b2[i];
    }
    __syncthreads();
    unsigned o_xre = 0u, o_xim = 0u, o_y = 0u, o_x1 = 0u, o_gin = 0u, o_g = 0u;
    const long long tiles = (a.N + FM_FT - 1) / FM_FT;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r0 = tile * FM_FT;
        const int rows = (int)(a.N - r0 < FM_FT ? a.N - r0 : FM_FT);
        for (int i = threadIdx.x; i < FM_FT * P; i += 256) {
            const int r = i / P, p = i - r * P;
            float2 v = make_float2(0.f, 0.f);
            if (r < rows) {
                v = *reinterpret_cast<const float2 *>(a.xs + (size_t)(r0 + r) * P2 + 2 * p);
                o_xre = fm_umax(o_xre, fm_absbits(v.x));
                o_xim = fm_umax(o_xim, fm_absbits(v.y));
                const bool keep = v.x > 0.f || (v.x == 0.f && v.y > 0.f);
                if (!keep) v = make_float2(0.f, 0.f);
            }
            *reinterpret_cast<float2 *>(sxs + r * LD1 + 2 * p) = v;
        }
        for (int i = threadIdx.x; i < FM_FT * (H / 4); i += 256) {
            const int r = i / (H / 4), c = (i - r * (H / 4)) * 4;
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) h = *reinterpret_cast<const float4 *>(a.h + (size_t)(r0 + r) * H + c);
            *reinterpret_cast<float4 *>(sh + r * LDH + c) = h;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS1, NT>(acc, sxs, LD1, bc, HT);
        float x1v[2][NT][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= HT) continue;
                const int col = t * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    const float u = fm_bn(sh[row * LDH + col], spar[col], spar[H + col], spar[2 * H + col], spar[3 * H + col]);
                    const float y = __fadd_rn(__fmul_rn(2.f, acc[rt][nt][r]), __fmul_rn(spar[4 * H + col], u));
                    const float x1 = fm_relu(y);
                    x1v[rt][nt][r] = x1;
                    sx1[row * LDH + col] = x1;
                    if (row < rows) {
                        o_y = fm_umax(o_y, fm_absbits(y));
                        o_x1 = fm_umax(o_x1, fm_absbits(x1));
                        if (TRACE) a.y_trace[(size_t)(r0 + row) * H + col] = y;
                    }
                }
            }
        __syncthreads();
        fm_mma<KS2, NT>(acc, sx1, LDH, bw, HT);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= HT) continue;
                const int col = t * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows) continue;
                    const float gin = __fadd_rn(acc[rt][nt][r], spar[5 * H + col]);
                    const float g = 1.f / (1.f + expf(-gin));
                    o_gin = fm_umax(o_gin, fm_absbits(gin));
                    o_g = fm_umax(o_g, fm_absbits(g));
                    const size_t o = (size_t)(r0 + row) * H + col;
                    a.hout[o] = fm_relu(__fadd_rn(__fmul_rn(x1v[rt][nt][r], g), sh[row * LDH + col]));
                    if (TRACE) {
                        a.gin_trace[o] = gin;
                        a.g_trace[o] = g;
                    }
                }
            }
        __syncthreads();
    }
    const unsigned om[7] = {o_xre, o_xim, o_y, o_x1, o_gin, o_x1, o_g};
    fm_obs_flush<7>(om, sobs, a.stats);
}

// ------------------------------------------------------------------------------------------------------------------
// decoder: out = h Wd + bd; observers [0] decoder.inp, [1] decoder.out.  The 257 columns leave a masked last tile.
// ------------------------------------------------------------------------------------------------------------------
struct FDecArgs {
    const float *h;  // (N,H)
    const float *w;  // (H,272), columns 257..271 zero
    const float *b;  // (272)
    float *out;      // (N,257)
    unsigned *stats; // 2 words or NULL
    long long N;
};

template <int DS>
__global__ __launch_bounds__(256) void k_fdec(FDecArgs a)
{
    constexpr int H = 48 * DS, NT = (FM_DEC_TILES + 3) / 4, KS = H / 4, LDA = fm_lda(H);
    __shared__ float sh[FM_FT * LDA];
    __shared__ unsigned sobs[FM_WAVES * 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float breg[NT][KS];
    fm_load_w<KS, NT>(breg, a.w, FM_MDEC, FM_DEC_TILES);
    float bias[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = wave + FM_WAVES * nt;
        bias[nt] = t < FM_DEC_TILES ? a.b[t * 16 + (lane & 15)] : 0.f;
    }
    unsigned om[2] = {0u, 0u};
    const long long tiles = (a.N + FM_FT - 1) / FM_FT;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r0 = tile * FM_FT;
        const int rows = (int)(a.N - r0 < FM_FT ? a.N - r0 : FM_FT);
        for (int i = threadIdx.x; i < FM_FT * (H / 4); i += 256) {
            const int r = i / (H / 4), c = (i - r * (H / 4)) * 4;
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) {
                h = *reinterpret_cast<const float4 *>(a.h + (size_t)(r0 + r) * H + c);
                om[0] = fm_umax(fm_umax(fm_umax(om[0], fm_absbits(h.x)), fm_umax(fm_absbits(h.y), fm_absbits(h.z))), fm_absbits(h.w));
            }
            *reinterpret_cast<float4 *>(sh + r * LDA + c) = h;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS, NT>(acc, sh, LDA, breg, FM_DEC_TILES);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= FM_DEC_TILES) continue;
                const int col = t * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows || col >= FM_DIN) continue;
                    const float v = __fadd_rn(acc[rt][nt][r], bias[nt]);
                    om[1] = fm_umax(om[1], fm_absbits(v));
                    a.out[(size_t)(r0 + row) * FM_DIN + col] = v;
                }
            }
        __syncthreads();
    }
    fm_obs_flush<2>(om, sobs, a.stats);
}

} // namespace s5
