// audio_stream_mask_istft_body.inc -- the body of the streaming masked iSTFT kernel, included by audio_stream.hpp once per
// kernel:
//   STREAM_RAGGED 0  k_stream_mask_istft: c, h4 and final are kernel arguments, stream s = blockIdx.x owns state s
//   STREAM_RAGGED 1  k_stream_mask_istft_ragged: entry e = blockIdx.x reads them and its state's slot from desc[e]; its rows and
//                    output hops sit at the front of padded rows of cmax frames / cmax + 1 hops.
#pragma clang fp contract(off)
    __shared__ Smem sm;
    __shared__ float prev[SEG_FLOATS];  // the three segments in front of the tile
    const int64_t s = blockIdx.x;
#if STREAM_RAGGED
    const s5fxp_push_desc *pd = desc + s;
    const int c = pd->hops, h4 = pd->h4, flags = pd->flags, final = flags & S5FXP_PUSH_FINAL;
    const bool zst = (flags & S5FXP_PUSH_FRESH) != 0;  // the carried segments read as zeros (the window is the front kernel's)
    float *st = state + (int64_t)pd->slot * STATE_FLOATS;
#else
    float *st = state + s * STATE_FLOATS;
#endif
    const float *W = st + (STREAM_MAX_HOPS - c) * HOP;
    float *carry = st + AUD_HOPS * HOP;
    const int f0 = h4 == 0 ? 1 : 0, F = c - f0, rmin = h4 < 3 ? 3 - h4 : 0;
    const int O = (c > rmin ? c - rmin : 0) + (final ? 1 : 0);
#if STREAM_RAGGED
    for (int i = threadIdx.x; i < SEG_FLOATS; i += 256) prev[i] = zst ? 0.0f : carry[i];
#else
    for (int i = threadIdx.x; i < SEG_FLOATS; i += 256) prev[i] = carry[i];
#endif
    make_twiddles(sm);
    constexpr int NJ = (FR * NBIN + 255) / 256;  // elements threadIdx.x + 256 j of the tile's 16 x 257
    const float *seg = reinterpret_cast<const float *>(sm.a);
#pragma unroll 1
    for (int i0 = 0; i0 < c; i0 += FR) {
        const int nf = c - i0 < FR ? c - i0 : FR;
#if STREAM_RAGGED
        const int64_t base = (s * cmax + (i0 - f0)) * NBIN;
#else
        const int64_t base = (s * F + (i0 - f0)) * NBIN;
#endif
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
#if STREAM_RAGGED
            out[(s * (cmax + 1) + (r - rmin)) * HOP + n] = acc / cover;
#else
            out[(s * O + (r - rmin)) * HOP + n] = acc / cover;
#endif
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
#if STREAM_RAGGED
            out[(s * (cmax + 1) + (c - rmin)) * HOP + n] = acc / 3.0f;
#else
            out[(s * O + (c - rmin)) * HOP + n] = acc / 3.0f;
#endif
        }
    }
    for (int i = threadIdx.x; i < SEG_FLOATS; i += 256) carry[i] = prev[i];
