// audio_stream.hpp -- the framing of audio_stft.hpp for a live signal: whole hops of 128 samples in, cleaned hops out, with a
// small per-stream state between calls.  Two kernels either side of the step kernel (s5fxp_step.hpp), which is not touched:
//
//   k_stream_stft        new audio (S,c*128) + state -> x = |Z| - sub of the F frames the push completes, (S,F,257)
//   k_stream_mask_istft  mask (S,F,257) + state -> O cleaned hops (S,O*128) [+ cleaned_mag = |Z| * (1 + mask), (S,F,257)]
//
// and their ragged forms k_stream_stft_ragged / k_stream_mask_istft_ragged (the same bodies, audio_stream_*_body.inc): one
// workgroup per ENTRY of a descriptor array, each with its own c, h4, flags and state slot (include/s5fxp.h s5fxp_push_desc).
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
#define STREAM_RAGGED 0
#include "audio_stream_stft_body.inc"
#undef STREAM_RAGGED
}

// grid = S.  h4 = min(hops_before, 4).  Segment list of a push: the three carried ones, then frames i = 0 .. c-1 of the
// window (frame 0 of a first push is a zero), then with `final` a zero; row r (output hop hops_before - 3 + r) sums entries
// r .. r+3 of it.  Rows below rmin = max(0, 3 - hops_before) lie before the signal and are not written.
__global__ __launch_bounds__(256) void k_stream_mask_istft(const float *__restrict__ mask, int c, int h4, int final, float *state,
                                                           float *__restrict__ out, float *__restrict__ cleaned_mag)
{
#define STREAM_RAGGED 0
#include "audio_stream_mask_istft_body.inc"
#undef STREAM_RAGGED
}

// The two kernels with per-workgroup c, h4, flags and state slot (include/s5fxp.h s5fxp_push_desc): grid = n entries.  O in
// the back kernel still counts the entry's output hops; the padded row of `out` holds cmax + 1.
__global__ __launch_bounds__(256) void k_stream_stft_ragged(const float *__restrict__ audio, int cmax,
                                                            const s5fxp_push_desc *__restrict__ desc, float sub, float *state,
                                                            float *__restrict__ x)
{
#define STREAM_RAGGED 1
#include "audio_stream_stft_body.inc"
#undef STREAM_RAGGED
}

__global__ __launch_bounds__(256) void k_stream_mask_istft_ragged(const float *__restrict__ mask, int cmax,
                                                                  const s5fxp_push_desc *__restrict__ desc, float *state,
                                                                  float *__restrict__ out, float *__restrict__ cleaned_mag)
{
#define STREAM_RAGGED 1
#include "audio_stream_mask_istft_body.inc"
#undef STREAM_RAGGED
}

} // namespace stft
} // namespace s5
