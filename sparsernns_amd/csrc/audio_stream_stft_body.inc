// audio_stream_stft_body.inc -- the body of the streaming STFT kernel, included by audio_stream.hpp once per kernel:
//   STREAM_RAGGED 0  k_stream_stft: c and f0 are kernel arguments, stream s = blockIdx.x owns state s and rows s * F ..
//   STREAM_RAGGED 1  k_stream_stft_ragged: entry e = blockIdx.x reads c, h4, its flags and its state's slot from desc[e]; its
//                    audio and rows sit at the front of padded rows of cmax hops / cmax frames.
#pragma clang fp contract(off)
    __shared__ Smem sm;
    const int64_t s = blockIdx.x;
#if STREAM_RAGGED
    const s5fxp_push_desc *pd = desc + s;
    const int c = pd->hops, f0 = pd->h4 == 0 ? 1 : 0, flags = pd->flags;
    const bool zst = (flags & S5FXP_PUSH_FRESH) != 0;  // the slot's state reads as all-zero bytes
    float *aud = state + (int64_t)pd->slot * STATE_FLOATS;
    const float *hist = aud + STREAM_MAX_HOPS * HOP;
    const float *fresh = audio && !(flags & S5FXP_PUSH_ZEROS) ? audio + s * cmax * HOP : nullptr;
    const int F = c - f0;
    const float keep0 = zst ? 0.0f : hist[threadIdx.x];
    const float keep1 = !zst && threadIdx.x < HIST * HOP - 256 ? hist[256 + threadIdx.x] : 0.0f;
#else
    float *aud = state + s * STATE_FLOATS;
    const float *hist = aud + STREAM_MAX_HOPS * HOP;
    const float *fresh = audio ? audio + s * c * HOP : nullptr;
    const int F = c - f0;
    // this thread's part of the history, kept for the shift at the end
    const float keep0 = hist[threadIdx.x], keep1 = threadIdx.x < HIST * HOP - 256 ? hist[256 + threadIdx.x] : 0.0f;
#endif
    if (F > 0) {
        make_twiddles(sm);
#pragma unroll 1
        for (int i0 = 0; i0 < c; i0 += FR) {
            stage_window(sm, c + HIST, i0, [&](int w, int n) {
#if STREAM_RAGGED
                return w < HIST ? (zst ? 0.0f : hist[w * HOP + n]) : fresh ? fresh[(w - HIST) * HOP + n] : 0.0f;
#else
                return w < HIST ? hist[w * HOP + n] : fresh ? fresh[(w - HIST) * HOP + n] : 0.0f;
#endif
            });
            forward_transform(sm);
            const int lo = i0 < f0 ? f0 : i0, hi = i0 + FR < c ? i0 + FR : c;
#if STREAM_RAGGED
            const int64_t base = (s * cmax + (lo - f0)) * NBIN;
#else
            const int64_t base = (s * F + (lo - f0)) * NBIN;
#endif
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
