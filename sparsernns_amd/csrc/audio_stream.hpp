// audio_stream.hpp -- the framing of audio_stft.hpp for a live signal: whole hops of 128 samples in, cleaned hops out, with a
// small per-stream state between calls.  Two kernels either side of the step kernel (s5fxp_step.hpp), which is not touched:
//
//   k_stream_stft        new audio (S,c*128) + state -> x = |Z| - sub of the F frames the push completes, (S,F,257)
//   k_stream_mask_istft  mask (S,F,257) + state -> O cleaned hops (S,O*128) [+ cleaned_mag = |Z| * (1 + mask), (S,F,257)]
//
// With h hops received before a push of c (1..32): frame k of the batch framing covers audio hops k-2 .. k+1, so the push
// completes frames h-1 .. h+c-2 (frame -1 does not exist: F = c - (h == 0)); output hop o is the sum over q = 0..3 of slice
// 128(3-q) of the inverse transforms of frames o-1+q, so the push yields hops max(0,h-3) .. h+c-4, and with `final` -- the
// caller has pushed scipy's trailing zeros -- also hop h+c-3, whose fourth frame does not exist.
//
// State of one stream, STATE_FLOATS floats, all-zero bytes = a fresh stream:
//   aud[35][128]  the last 35 hops received, newest last.  The front kernel shifts the push in, so the window of a push -- its
//                 three hops of history and its c new hops, W = aud[32-c .. 35) -- is contiguous for the back kernel, which
//                 has no audio argument and rebuilds the spectrum from W as k_mask_istft does from the clip.
//   seg[3][512]   the inverse transforms of the last three frames (what later output hops still need of them).
// Only the front kernel writes aud and only the back kernel writes seg.  Nothing on the device counts hops.
//
// One 256-thread workgroup per stream walks the push in tiles of 16 frames, so the in-place update has no second writer.
// Every transform goes through audio_stft.hpp (forward_transform, bin_from_packed, cabs, inverse_tile, the same twiddles,
// contraction off), a frame's arithmetic does not depend on its place in a tile, and a hop is `acc = 0; acc += seg[q]` for
// q = 0..3 over the same four segments (one that does not exist adds a zero, which leaves acc's bits alone) divided by the
// same cover: x, cleaned_mag and the audio are bit for bit what k_stft_mag / k_mask_istft give for the whole signal.
#pragma once
#include "audio_stft.hpp"

namespace s5 {
namespace stft {

constexpr int STREAM_MAX_HOPS = 32;
constexpr int HIST = 3;                                  // hops of history a frame reaches back
constexpr int AUD_HOPS = STREAM_MAX_HOPS + HIST;
constexpr int SEG_FLOATS = HIST * NFFT;
constexpr int STATE_FLOATS = AUD_HOPS * HOP + SEG_FLOATS;
static_assert(STATE_FLOATS % 4 == 0, "per-stream state is a multiple of 16 bytes");

// Stages hops w0 .. w0+18 of a window of nw hops, zeros from hop nw on, in plane B as forward_tile does; load(w, n) is sample
// n of hop w.  Ends with a barrier.
template <class Load> __device__ __forceinline__ void stage_window(Smem &sm, int nw, int w0, Load load)
{
    float *stage = reinterpret_cast<float *>(sm.b);
#pragma unroll
    for (int j = 0; j < (NHOP * HOP + 255) / 256; ++j) {
        const int i = threadIdx.x + 256 * j;
        const int w = w0 + (i >> 7), n = i & 127;
        const float a = (i < NHOP * HOP && w < nw) ? load(w, n) : 0.0f;
        if (i < NHOP * HOP) stage[(i >> 7) * HSTR + n] = a;
    }
    __syncthreads();
}

// grid = S.  f0 = 1 for the first push of a stream (hops_before == 0), else 0: frame i of the window (i = f0 .. c-1, hops
// i .. i+3 of it) is row i - f0 of x.
__global__ __launch_bounds__(256) void k_stream_stft(const float *__restrict__ audio, int c, int f0, float sub, float *state,
                                                     float *__restrict__ x)
{
#pragma clang fp contract(off)
    __shared__ Smem sm;
    const int64_t s = blockIdx.x;
    float *aud = state + s * STATE_FLOATS;
    const float *hist = aud + STREAM_MAX_HOPS * HOP;
    const float *fresh = audio ? audio + s * c * HOP : nullptr;
    const int F = c - f0;
    // this thread's part of the history, kept for the shift at the end
    const float keep0 = hist[threadIdx.x], keep1 = threadIdx.x < HIST * HOP - 256 ? hist[256 + threadIdx.x] : 0.0f;
    if (F > 0) {
        make_twiddles(sm);
#pragma unroll 1
        for (int i0 = 0; i0 < c; i0 += FR) {
            stage_window(sm, c + HIST, i0, [&](int w, int n) {
                return w < HIST ? hist[w * HOP + n] : fresh ? fresh[(w - HIST) * HOP + n] : 0.0f;
            });
            forward_transform(sm);
            const int lo = i0 < f0 ? f0 : i0, hi = i0 + FR < c ? i0 + FR : c;
            const int64_t base = (s * F + (lo - f0)) * NBIN;
            for (int i = threadIdx.x; i < (hi - lo) * NBIN; i += 256) {
                const int fr = i / NBIN, k = i - fr * NBIN;
                const float2 z = bin_from_packed(sm.b + (lo - i0 + fr) * FSTR, sm.tw, k);
                x[base + i] = cabs(z) - sub;
            }
            __syncthreads();  // plane B is the next tile's stage
        }
    }
    // every read of the history is behind a barrier: shift the window in
    __syncthreads();
    float *dst = aud + (STREAM_MAX_HOPS - c) * HOP;
    for (int i = threadIdx.x; i < (c + HIST) * HOP; i += 256)
        dst[i] = i < 256 ? keep0 : i < HIST * HOP ? keep1 : fresh ? fresh[i - HIST * HOP] : 0.0f;
}

// grid = S.  h4 = min(hops_before, 4).  Segment list of a push: the three carried ones, then frames i = 0 .. c-1 of the
// window (frame 0 of a first push is a zero), then with `final` a zero; row r (output hop hops_before - 3 + r) sums entries
// r .. r+3 of it.  Rows below rmin = max(0, 3 - hops_before) lie before the signal and are not written.
__global__ __launch_bounds__(256) void k_stream_mask_istft(const float *__restrict__ mask, int c, int h4, int final, float *state,
                                                           float *__restrict__ out, float *__restrict__ cleaned_mag)
{
#pragma clang fp contract(off)
    __shared__ Smem sm;
    __shared__ float prev[SEG_FLOATS];  // the three segments in front of the tile
    const int64_t s = blockIdx.x;
    float *st = state + s * STATE_FLOATS;
    const float *W = st + (STREAM_MAX_HOPS - c) * HOP;
    float *carry = st + AUD_HOPS * HOP;
    const int f0 = h4 == 0 ? 1 : 0, F = c - f0, rmin = h4 < 3 ? 3 - h4 : 0;
    const int O = (c > rmin ? c - rmin : 0) + (final ? 1 : 0);
    for (int i = threadIdx.x; i < SEG_FLOATS; i += 256) prev[i] = carry[i];
    make_twiddles(sm);
    constexpr int NJ = (FR * NBIN + 255) / 256;  // elements threadIdx.x + 256 j of the tile's 16 x 257
    const float *seg = reinterpret_cast<const float *>(sm.a);
#pragma unroll 1
    for (int i0 = 0; i0 < c; i0 += FR) {
        const int nf = c - i0 < FR ? c - i0 : FR;
        const int64_t base = (s * F + (i0 - f0)) * NBIN;
        stage_window(sm, c + HIST, i0, [&](int w, int n) { return W[w * HOP + n]; });
        forward_transform(sm);
        // Z' = Z * (1 + mask) into plane A.  Not unrolled further and the mask is read here, not ahead of the transform: kept
        // in registers across it, the 17 factors and the unrolled loop took the kernel past 256 registers
#pragma unroll 4
        for (int j = 0; j < NJ; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i >= FR * NBIN) break;
            const int fr = i / NBIN, k = i - fr * NBIN;
            const int fi = i0 + fr;
            float2 z = make_float2(0.0f, 0.0f);
            if (fi >= f0 && fi < c) {
                const float fj = mask ? 1.0f + mask[base + i] : 1.0f;
                z = bin_from_packed(sm.b + fr * FSTR, sm.tw, k);
                if (cleaned_mag) cleaned_mag[base + i] = cabs(z) * fj;
                z = make_float2(z.x * fj, z.y * fj);
            }
            sm.a[fr * FSTR + k] = z;
        }
        __syncthreads();
        inverse_tile(sm);
        // rows i0 .. i0+nf-1: the newest of their four segments is in this tile
        for (int i = threadIdx.x; i < nf * HOP; i += 256) {
            const int t = i >> 7, n = i & 127, r = i0 + t;
            if (r < rmin) continue;
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = t + q;
                acc += m < HIST ? prev[m * NFFT + HOP * (3 - q) + n] : seg[(m - HIST) * (2 * FSTR) + HOP * (3 - q) + n];
            }
            const float cover = 4.0f - (h4 - 3 + r == 0 ? 1.0f : 0.0f);
            out[(s * O + (r - rmin)) * HOP + n] = acc / cover;
        }
        // the last three segments of prev ++ tile are the next tile's prev
        float nx[SEG_FLOATS / 256];
#pragma unroll
        for (int j = 0; j < SEG_FLOATS / 256; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int m = (i >> 9) + nf, e = i & (NFFT - 1);
            nx[j] = m < HIST ? prev[m * NFFT + e] : seg[(m - HIST) * (2 * FSTR) + e];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SEG_FLOATS / 256; ++j) prev[threadIdx.x + 256 * j] = nx[j];
        __syncthreads();
    }
    if (final) {
        // row c: three carried segments and a frame that does not exist
        for (int n = threadIdx.x; n < HOP; n += 256) {
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) acc += prev[q * NFFT + HOP * (3 - q) + n];
            out[(s * O + (c - rmin)) * HOP + n] = acc / 3.0f;
        }
    }
    for (int i = threadIdx.x; i < SEG_FLOATS; i += 256) carry[i] = prev[i];
}

} // namespace stft
} // namespace s5
