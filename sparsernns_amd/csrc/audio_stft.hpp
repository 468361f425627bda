// audio_stft.hpp -- the two steps either side of the model in the reference's N-DNS validation loop as HIP kernels:
// sparseRNNs/train_helpers.py:1382-1412 (stft_splitter / stft_mixer = scipy.signal.stft / istft with nperseg = nfft = 512,
// hop 128, boxcar window, one-sided, boundary="zeros", padded=True, scaling="spectrum") and fxprun.py:63-78
// (mag - 0.0007 in front of the model, noisy_mag * (1 + mask) -> stft_mixer behind it).
//
//   k_stft_mag     audio (B,T) -> x = |Z| - sub, (B,n_seg,257) frame-major [+ the complex spectrum Z]
//   k_mask_istft   audio (B,T), mask (B,n_seg,257) -> cleaned audio (B,(n_seg-1)*128) [+ cleaned_mag = |Z| * (1 + mask)]
//   k_stft_mag_i16 / k_mask_istft_i16: the same two with the model's int16 boundary (s5fxp_model_forward_i16): x leaves as
//                  fromfp(|Z| - sub, FLOOR) at (x_bits, x_exp), the mask arrives as int16 at mask_exp -- 2 bytes per value, and
//                  the same audio bit for bit, since both conversions restate 16-bit integers.  The bodies are shared as text
//                  (audio_stft_mag_body.inc, audio_mask_istft_body.inc) with the boundary type as a compile-time constant, as
//                  the encoder's and decoder's are (proj_p.hpp): the float kernels keep their instruction streams.
//   k_stft_mag_clips / k_mask_istft_clips: the same two bodies for n clips of different lengths in one launch (at the end).
//
// Framing.  With p the signal between 256 zeros on each side and zero-filled up to a whole hop, frame k is p[128k .. 128k+511]
// (hops k..k+3 of p), n_seg = ceil(T/128) + 1.  Output hop o of the inverse (samples 128o .. 128o+127, hop o+2 of p) is the
// sum of position 128(3-q) + s of the inverse transforms of frames o-1+q, q = 0..3, divided by the number of those frames
// that exist: 4, or 3 in the first and the last hop.  A fixed order of four adds: no atomics, no normaliser tensor.
//
// One 256-thread workgroup takes 16 consecutive frames: 19 hops of audio are staged in LDS (zeros outside [0,T)), 16 lanes
// work on one frame.  A frame's 512 real samples are 256 complex numbers z[n] = x[2n] + i x[2n+1]; their 256-point
// transform is two rounds of 16-point transforms in registers (radix 4 x 4) with one exchange through LDS between them, and
// the one-sided 257 bins follow from Y[k] and Y[256-k].  The inverse kernel rebuilds the spectrum from the audio in the same
// way (same device functions: its |Z| is bit for bit k_stft_mag's), multiplies the complex value by 1 + mask -- equal to
// polar(|Z| * (1 + mask), angle(Z)), negative factors included, without angle or polar -- and walks the same steps back.  Its
// tile of 16 frames yields 13 output hops, so neighbouring tiles overlap by three frames (16/13 of the transforms).
//
// Twiddles: a table of the 512th roots of unity in LDS, from sincospif.  Floating-point contraction is off in every function
// here and fused multiply-adds are written out, so the shared functions round identically in both kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fxp_prims.hpp"

namespace s5 {
namespace stft {

constexpr int NFFT = 512, HOP = 128, NBIN = 257;
constexpr int FR = 16;             // frames per workgroup (4 waves x 4 frames, 16 lanes each)
constexpr int OH = FR - 3;         // output hops per workgroup of the inverse
constexpr int NHOP = FR + 3;       // hops of audio a workgroup stages
constexpr int HSTR = HOP + 32;     // staged hop stride in floats (padded; bank conflicts not profiled)
constexpr int FSTR = 272;          // frame stride of an exchange plane in float2 (16 rows of 17; >= 257)
static_assert(NHOP * HSTR <= 2 * FR * FSTR, "the staged audio lives in plane B");

struct Smem {
    float2 tw[512];       // tw[j] = exp(-2 pi i j / 512)
    float2 a[FR * FSTR];  // plane A
    float2 b[FR * FSTR];  // plane B (first the staged audio)
};

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a * w, or a * conj(w)
template <bool CONJ> __device__ __forceinline__ float2 cmul(float2 a, float2 w)
{
#pragma clang fp contract(off)
    const float wy = CONJ ? -w.y : w.y;
    return make_float2(__builtin_fmaf(a.x, w.x, -(a.y * wy)), __builtin_fmaf(a.x, wy, a.y * w.x));
}

// 4-point transform in place; INV: exp(+...).
template <bool INV> __device__ __forceinline__ void fft4(float2 &a, float2 &b, float2 &c, float2 &d)
{
#pragma clang fp contract(off)
    const float2 t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), t3 = csub(b, d);
    // -i * t3 = (t3.y, -t3.x)
    const float2 r = INV ? make_float2(-t3.y, t3.x) : make_float2(t3.y, -t3.x);
    a = cadd(t0, t2);
    b = cadd(t1, r);
    c = csub(t0, t2);
    d = csub(t1, r);
}

// 16-point transform in place.  Bin k is left in v[pos16(k)].
__host__ __device__ constexpr int pos16(int k) { return 4 * (k & 3) + (k >> 2); }
template <bool INV> __device__ __forceinline__ void fft16(float2 (&v)[16])
{
#pragma clang fp contract(off)
    // exp(-2 pi i j / 16), j = 0..9
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, R = 0.70710678118654752f;
    constexpr float WX[10] = {1.f, C1, R, S1, 0.f, -S1, -R, -C1, -1.f, -C1};
    constexpr float WY[10] = {0.f, -S1, -R, -C1, -1.f, -C1, -R, -S1, 0.f, S1};
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) fft4<INV>(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
#pragma unroll
    for (int k1 = 1; k1 < 4; ++k1)
#pragma unroll
        for (int n2 = 1; n2 < 4; ++n2) v[4 * k1 + n2] = cmul<INV>(v[4 * k1 + n2], make_float2(WX[n2 * k1], WY[n2 * k1]));
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) fft4<INV>(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
}

// Second half of a 256-point transform whose first half (16-point transforms over the slow index, in v) is done:
// twiddle by exp(-+2 pi i l c / 256), exchange through plane `ex` (rows of 17), transform over the lanes' index.
// On return lane c of the frame holds bin c + 16 d in v[pos16(d)].  Ends without a barrier after its reads of `ex`.
template <bool INV> __device__ __forceinline__ void fft256_finish(float2 (&v)[16], float2 *ex, const float2 *tw, int l)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float2 t = v[pos16(c)];
        if (c) t = cmul<INV>(t, tw[(2 * l * c) & 511]);
        ex[c * 17 + l] = t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = ex[l * 17 + j];
    fft16<INV>(v);
}

__device__ __forceinline__ void make_twiddles(Smem &sm)
{
    for (int j = threadIdx.x; j < 512; j += 256) {
        float s, c;
        sincospif((float)j * (1.0f / 256.0f), &s, &c);
        sm.tw[j] = make_float2(c, -s);
    }
}

// With 19 hops staged in plane B (hop stride HSTR) and a barrier behind them: leaves, for the 16 frames that start at those
// hops, Y = the 256-point transform of z[n] = x[2n] + i x[2n+1] in plane B (natural order, frame stride FSTR).  Ends with a
// barrier.
__device__ __forceinline__ void forward_transform(Smem &sm)
{
#pragma clang fp contract(off)
    const float *stage = reinterpret_cast<const float *>(sm.b);
    const int fr = threadIdx.x >> 4, l = threadIdx.x & 15;
    float2 v[16];
#pragma unroll
    for (int n1 = 0; n1 < 16; ++n1)
        v[n1] = *reinterpret_cast<const float2 *>(stage + (fr + (n1 >> 2)) * HSTR + 32 * (n1 & 3) + 2 * l);
    fft16<false>(v);
    fft256_finish<false>(v, sm.a + fr * FSTR, sm.tw, l);
    // every lane has taken its samples out of the stage before the exchange's barrier: plane B is free
#pragma unroll
    for (int d = 0; d < 16; ++d) sm.b[fr * FSTR + l + 16 * d] = v[pos16(d)];
    __syncthreads();
}

// Stages hops h0 .. h0+18 of the padded signal of one sequence and runs forward_transform on them.
__device__ __forceinline__ void forward_tile(Smem &sm, const float *__restrict__ audio, int64_t T, int64_t h0)
{
    float *stage = reinterpret_cast<float *>(sm.b);
    // unrolled: the loads of all ten rounds are in flight together
#pragma unroll
    for (int j = 0; j < (NHOP * HOP + 255) / 256; ++j) {
        const int i = threadIdx.x + 256 * j;
        const int64_t t = (h0 + (i >> 7)) * HOP + (i & 127) - NFFT / 2;
        const float a = (i < NHOP * HOP && t >= 0 && t < T) ? audio[t] : 0.0f;
        if (i < NHOP * HOP) stage[(i >> 7) * HSTR + (i & 127)] = a;
    }
    __syncthreads();
    forward_transform(sm);
}

// Bin k (0..256) of the 512-point real transform, scaled by 1/512, from the 256-point Y of the packed signal.
__device__ __forceinline__ float2 bin_from_packed(const float2 *__restrict__ Y, const float2 *__restrict__ tw, int k)
{
#pragma clang fp contract(off)
    const float2 a = Y[k & 255], b = Y[(256 - k) & 255], w = tw[k];
    const float dx = a.x - b.x, dy = a.y + b.y;
    const float re = (a.x + b.x) + __builtin_fmaf(w.x, dy, w.y * dx);
    const float im = (a.y - b.y) + __builtin_fmaf(w.y, dy, -(w.x * dx));
    return make_float2(re * (1.0f / 1024.0f), im * (1.0f / 1024.0f));
}

__device__ __forceinline__ float cabs(float2 z)
{
#pragma clang fp contract(off)
    return __builtin_sqrtf(z.x * z.x + z.y * z.y);
}

// With the one-sided spectra Z' of the tile's 16 frames in plane A (bins 0..256, frame stride FSTR) and a barrier behind them:
// leaves their 512 real samples in plane A (floats, frame stride 2 * FSTR).  Uses plane B.  Ends with a barrier.
__device__ __forceinline__ void inverse_tile(Smem &sm)
{
#pragma clang fp contract(off)
    const int fr = threadIdx.x >> 4, l = threadIdx.x & 15;
    float2 v[16];
    {
        const float2 *Z = sm.a + fr * FSTR;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            // Y'[k] = Xe + i Xo, Xe = (p + conj q) / 2, Xo = (p - conj q) / 2 * conj(w^k); the halves and the 512 of
            // irfft(512 Z') cancel against the 1/256 of the packed inverse
            const int k = 16 * a + l;
            const float2 p = Z[k], q = Z[256 - k], w = sm.tw[k];
            const float ex = p.x - q.x, ey = p.y + q.y;
            const float gx = __builtin_fmaf(ex, w.x, ey * w.y), gy = __builtin_fmaf(ey, w.x, -(ex * w.y));
            v[a] = make_float2((p.x + q.x) - gy, (p.y - q.y) + gx);
        }
    }
    fft16<true>(v);
    fft256_finish<true>(v, sm.b + fr * FSTR, sm.tw, l);
    // lane l holds z'[l + 16 d] = (x'[2l + 32d], x'[2l + 32d + 1]); plane A was last read before the exchange's barrier
#pragma unroll
    for (int d = 0; d < 16; ++d) sm.a[fr * FSTR + l + 16 * d] = v[pos16(d)];
    __syncthreads();
}

// grid = B * tiles, tiles = ceil(n_seg / 16)
__global__ __launch_bounds__(256) void k_stft_mag(const float *__restrict__ audio, int64_t T, int64_t n_seg, int tiles, float sub,
                                                  float *__restrict__ x, float2 *__restrict__ spec)
{
#pragma clang fp contract(off)
    constexpr bool I16 = false;
    [[maybe_unused]] constexpr int x_bits = 0, x_exp = 0;
    const int64_t a_pitch = T, f_pitch = n_seg;
#include "audio_stft_mag_body.inc"
}

// x = fxp_from_fp(|Z| - sub, FLOOR) at (x_bits <= 16, x_exp) of the very float k_stft_mag stores (fxp_prims.hpp fromfp)
__global__ __launch_bounds__(256) void k_stft_mag_i16(const float *__restrict__ audio, int64_t T, int64_t n_seg, int tiles, float sub,
                                                      int x_bits, int x_exp, int16_t *__restrict__ x, float2 *__restrict__ spec)
{
#pragma clang fp contract(off)
    constexpr bool I16 = true;
    const int64_t a_pitch = T, f_pitch = n_seg;
#include "audio_stft_mag_body.inc"
}

// grid = B * tiles, tiles = ceil((n_seg - 1) / 13); workgroup (b, o0 / 13) writes output hops o0 .. o0+12 from frames
// o0-1 .. o0+14
__global__ __launch_bounds__(256) void k_mask_istft(const float *__restrict__ audio, const float *__restrict__ mask, int64_t T,
                                                    int64_t n_seg, int tiles, float *__restrict__ out,
                                                    float *__restrict__ cleaned_mag)
{
#pragma clang fp contract(off)
    constexpr bool I16 = false;
    [[maybe_unused]] constexpr int mask_exp = 0;
    const int64_t a_pitch = T, f_pitch = n_seg;
#include "audio_mask_istft_body.inc"
}

// the mask as the decoder leaves it (int16 at mask_exp): 1 + to_float(mask) is the float route's factor
__global__ __launch_bounds__(256) void k_mask_istft_i16(const float *__restrict__ audio, const int16_t *__restrict__ mask, int mask_exp,
                                                        int64_t T, int64_t n_seg, int tiles, float *__restrict__ out,
                                                        float *__restrict__ cleaned_mag)
{
#pragma clang fp contract(off)
    constexpr bool I16 = true;
    const int64_t a_pitch = T, f_pitch = n_seg;
#include "audio_mask_istft_body.inc"
}

// Clips: n sequences of DIFFERENT lengths in one launch, the bodies above with each clip's geometry read from `samples`.  Clip e
// is row e of audio (n, a_pitch = Tmax) with T = clamp(samples[e], 0, Tmax) samples and n_seg = ceil(T / 128) + 1 frames (0 below
// 512 samples) in row e of tensors padded to f_pitch = Lmax = frames(Tmax) rows, the layout s5fxp_model_clips_f32 takes.  The grid
// is cut for the longest clip; a workgroup whose tile lies behind its clip's end leaves before the first barrier and LDS write (the
// test depends on blockIdx and samples[e] only, so a whole workgroup goes or stays).  A frame's transform and an output hop's sum
// do not depend on the tile that computes them: every clip gets the bits of k_stft_mag / k_mask_istft at B = 1, T = T_e.
__device__ __forceinline__ int64_t clip_samples(const int32_t *__restrict__ samples, int e, int64_t Tmax)
{
    const int64_t s = samples[e];
    return s < 0 ? 0 : s > Tmax ? Tmax : s;
}
__device__ __forceinline__ int64_t clip_frames(int64_t T) { return T < NFFT ? 0 : (T + HOP - 1) / HOP + 1; }

// grid = n * tiles, tiles = ceil(Lmax / 16); lens: NULL or (n), lens[e] = n_seg of clip e for s5fxp_model_clips
__global__ __launch_bounds__(256) void k_stft_mag_clips(const float *__restrict__ audio, int64_t a_pitch, int64_t f_pitch, int tiles,
                                                        const int32_t *__restrict__ samples, float sub, float *__restrict__ x,
                                                        float2 *__restrict__ spec, int32_t *__restrict__ lens)
{
#pragma clang fp contract(off)
    constexpr bool I16 = false;
    [[maybe_unused]] constexpr int x_bits = 0, x_exp = 0;
    const int64_t T = clip_samples(samples, blockIdx.x / tiles, a_pitch), n_seg = clip_frames(T);
    if (lens && blockIdx.x % tiles == 0 && threadIdx.x == 0) lens[blockIdx.x / tiles] = (int32_t)n_seg;
    if ((int64_t)(blockIdx.x % tiles) * FR >= n_seg) return;
#include "audio_stft_mag_body.inc"
}

// grid = n * tiles, tiles = ceil((Lmax - 1) / 13); clip e writes the first (n_seg - 1) * 128 samples of its row of out
// (n, (Lmax - 1) * 128)
__global__ __launch_bounds__(256) void k_mask_istft_clips(const float *__restrict__ audio, const float *__restrict__ mask, int64_t a_pitch,
                                                          int64_t f_pitch, int tiles, const int32_t *__restrict__ samples,
                                                          float *__restrict__ out, float *__restrict__ cleaned_mag)
{
#pragma clang fp contract(off)
    constexpr bool I16 = false;
    [[maybe_unused]] constexpr int mask_exp = 0;
    const int64_t T = clip_samples(samples, blockIdx.x / tiles, a_pitch), n_seg = clip_frames(T);
    if ((int64_t)(blockIdx.x % tiles) * OH >= n_seg - 1) return;
#include "audio_mask_istft_body.inc"
}

} // namespace stft
} // namespace s5
