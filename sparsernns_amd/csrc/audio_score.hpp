// audio_score.hpp -- the last stage of the reference's N-DNS validation step (sparseRNNs/fxprun.py:79-88) on the device:
// si_snr(cleaned, clean) (train_helpers.py:15-53) and loss = lam * mean((cleaned_mag - clean_mag)^2) + (100 - si_snr), from
// the noisy clip, the clean clip and the model's mask in two launches.  Neither the cleaned audio nor a magnitude plane has
// to exist in HBM.
//
//   k_mask_istft_score[_i16]  everything k_mask_istft[_i16] does (audio_stft.hpp; out and cleaned_mag optional), plus six sums
//                             per tile: the clean clip's 19 hops go through the same forward transform first (its |Z| is bit
//                             for bit what k_stft_mag stores with sub = 0), stay in registers next to 1 + mask, and meet
//                             |Z| * (1 + mask) of the noisy clip where that is formed; every cleaned sample meets its clean
//                             sample (a second read of the clean hops, from the L2) where it would be stored.
//   k_score_finalize          grid = B: the tile sums of a sequence in index order, then the three scores.
//   k_mask_istft_score_clips / k_score_finalize_clips: the two for n clips of different lengths (at the end).
//
// Ownership.  Neighbouring tiles overlap by three frames; a tile counts the frames it reports in cleaned_mag -- its frames
// 1..13, the last tile of a sequence also what lies beyond them -- so every frame 0..n_seg-1 is counted once.  Output hops
// belong to one tile each; samples at or beyond T (the zero padding up to (n_seg-1)*128) are not counted.
//
// Moments.  With t the float32 the kernel would store in out and e the clean sample, over the N = T samples:
//   |s_t|^2 = St2 - St^2/N, |s_e|^2 = Se2 - Se^2/N, dot = Ste - St Se/N, P = dot^2/|s_t|^2 = sum(proj^2),
//   sum((s_e - proj)^2) = |s_e|^2 - P (clamped at 0), si_snr = 10 log10(P / (that + 1e-8) + 1e-8).
// These subtract nearly equal numbers: everything is accumulated and combined in double (products of two float32 are exact
// there), which is what makes the form usable at 30-40 dB.  No atomics: lanes by shuffles, waves through LDS, tiles by the
// second kernel, each in a fixed order, so two calls give identical bits.
#pragma once
#include "audio_stft.hpp"

namespace s5 {
namespace stft {

constexpr int NSUM = 6; // St, Se, St2, Se2, Ste, Sd2 (d = cleaned_mag - clean_mag)

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v; // lane 0 holds the wave's sum
}

// grid as k_mask_istft; partials: (B, tiles, NSUM) double
__global__ __launch_bounds__(256) void k_mask_istft_score(const float *__restrict__ audio, const float *__restrict__ clean,
                                                          const float *__restrict__ mask, int64_t T, int64_t n_seg, int tiles,
                                                          float *__restrict__ out, float *__restrict__ cleaned_mag,
                                                          double *__restrict__ partials)
{
#pragma clang fp contract(off)
    constexpr bool I16 = false;
    [[maybe_unused]] constexpr int mask_exp = 0;
    const int64_t a_pitch = T, f_pitch = n_seg;
#include "audio_mask_istft_score_body.inc"
}

__global__ __launch_bounds__(256) void k_mask_istft_score_i16(const float *__restrict__ audio, const float *__restrict__ clean,
                                                              const int16_t *__restrict__ mask, int mask_exp, int64_t T,
                                                              int64_t n_seg, int tiles, float *__restrict__ out,
                                                              float *__restrict__ cleaned_mag, double *__restrict__ partials)
{
#pragma clang fp contract(off)
    constexpr bool I16 = true;
    const int64_t a_pitch = T, f_pitch = n_seg;
#include "audio_mask_istft_score_body.inc"
}

// grid = B, one wave: lane c < NSUM adds sum c of the sequence's tiles in index order, lane 0 forms the scores.
// mag_mse and loss may be NULL.
__global__ __launch_bounds__(64) void k_score_finalize(const double *__restrict__ partials, int tiles, int64_t T, int64_t n_seg,
                                                       float lam, float *__restrict__ si_snr, float *__restrict__ mag_mse,
                                                       float *__restrict__ loss)
{
#pragma clang fp contract(off)
    const int pitch = tiles;
#include "audio_score_finalize_body.inc"
}

// Clips: n sequences of DIFFERENT lengths in two launches, the layout and the geometry of k_mask_istft_clips (audio_stft.hpp);
// clean is (n, Tmax), padded like audio, and clip e is scored over its own T_e samples and len_e frames.  A tile's six sums depend
// on that tile's frames and on the clip's own T and n_seg only, and the finalize adds the clip's own tiles in the same order with
// the same expressions: every score, and every plane, has the bits of k_mask_istft_score / k_score_finalize at B = 1, T = T_e.
//
// grid = n * tiles, tiles = ceil((Lmax - 1) / 13); partials: (n, tiles, NSUM) double.  A workgroup whose tile lies behind its
// clip's end leaves before the first barrier and LDS write and writes no partial.
__global__ __launch_bounds__(256) void k_mask_istft_score_clips(const float *__restrict__ audio, const float *__restrict__ clean,
                                                                const float *__restrict__ mask, int64_t a_pitch, int64_t f_pitch,
                                                                int tiles, const int32_t *__restrict__ samples,
                                                                float *__restrict__ out, float *__restrict__ cleaned_mag,
                                                                double *__restrict__ partials)
{
#pragma clang fp contract(off)
    constexpr bool I16 = false;
    [[maybe_unused]] constexpr int mask_exp = 0;
    const int64_t T = clip_samples(samples, blockIdx.x / tiles, a_pitch), n_seg = clip_frames(T);
    if ((int64_t)(blockIdx.x % tiles) * OH >= n_seg - 1) return;
#include "audio_mask_istft_score_body.inc"
}

// grid = n, one wave; pitch: the tiles of the grid above.  Only the tiles whose workgroups stayed, 0 .. ceil((len_e - 1) / 13) - 1, are
// read.  A clip without frames gets a quiet NaN in all three scores.
__global__ __launch_bounds__(64) void k_score_finalize_clips(const double *__restrict__ partials, int pitch, int64_t Tmax,
                                                             const int32_t *__restrict__ samples, float lam,
                                                             float *__restrict__ si_snr, float *__restrict__ mag_mse,
                                                             float *__restrict__ loss)
{
#pragma clang fp contract(off)
    const int64_t T = clip_samples(samples, blockIdx.x, Tmax), n_seg = clip_frames(T);
    if (n_seg == 0) {
        if (threadIdx.x == 0) {
            const float nan = __builtin_nanf("");
            si_snr[blockIdx.x] = nan;
            if (mag_mse) mag_mse[blockIdx.x] = nan;
            if (loss) loss[blockIdx.x] = nan;
        }
        return;
    }
    const int tiles = (int)((n_seg - 1 + OH - 1) / OH);
#include "audio_score_finalize_body.inc"
}

} // namespace stft
} // namespace s5
