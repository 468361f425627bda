// audio_mask_istft_score_body.inc -- the body of k_mask_istft_score, k_mask_istft_score_i16 and k_mask_istft_score_clips
// (audio_score.hpp), included with I16 = false / true: audio_mask_istft_body.inc with the clean clip's transform in front and the
// sums folded in.  T, n_seg, a_pitch and f_pitch as in audio_stft_mag_body.inc (clean is pitched like audio); the tile sums go to
// partials at pitch `tiles`, the grid's.
    __shared__ Smem sm;
    const int64_t b = blockIdx.x / tiles, o0 = (int64_t)(blockIdx.x % tiles) * OH, k0 = o0 - 1;
    constexpr int NJ = (FR * NBIN + 255) / 256;
    const int64_t base = (b * f_pitch + k0) * NBIN;
    // of the tile's frames fr = 0..15 (frame k0 + fr of the sequence) fr_lo..fr_hi exist; the tile owns 1..own_hi of them, as
    // audio_mask_istft_body.inc reports them in cleaned_mag: its frames 1..13, the last tile of a sequence also what lies beyond
    const int fr_lo = k0 < 0 ? 1 : 0, fr_hi = (int)(n_seg - 1 - k0 < FR - 1 ? n_seg - 1 - k0 : FR - 1);
    const int own_hi = o0 + OH >= n_seg - 1 ? fr_hi : OH;
    // the clean clip first, in the planes the noisy tile will take: |Z_clean| of this thread's elements (threadIdx.x + 256 j of
    // the tile's 16 x 257) stays in registers
    make_twiddles(sm);
    forward_tile(sm, clean + b * a_pitch, T, k0);
    float cm[NJ];
    // this phase's lane masks are computed from a thread index the compiler cannot match with the later loops', or it keeps
    // 17 of them in scalar registers across both transforms and spills
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = tid + 256 * j;
        const int fr = i / NBIN, k = i - fr * NBIN;
        cm[j] = (fr >= fr_lo && fr <= fr_hi) ? cabs(bin_from_packed(sm.b + fr * FSTR, sm.tw, k)) : 0.0f;
    }
    __syncthreads(); // plane B is staged again
    // from here on k_mask_istft's steps; a frame that does not exist contributes nothing
    float f[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = threadIdx.x + 256 * j, fr = i / NBIN;
        if constexpr (I16) f[j] = (mask && fr >= fr_lo && fr <= fr_hi) ? 1.0f + tofloat(mask[base + i], mask_exp) : 1.0f;
        else f[j] = (mask && fr >= fr_lo && fr <= fr_hi) ? 1.0f + mask[base + i] : 1.0f;
    }
    forward_tile(sm, audio + b * a_pitch, T, k0);
    double sum[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // Z' = Z * (1 + mask) into plane A
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = threadIdx.x + 256 * j;
        if (i >= FR * NBIN) break;
        const int fr = i / NBIN, k = i - fr * NBIN;
        float2 z = make_float2(0.0f, 0.0f);
        if (fr >= fr_lo && fr <= fr_hi) {
            z = bin_from_packed(sm.b + fr * FSTR, sm.tw, k);
            const bool own = fr >= 1 && fr <= own_hi;
            const float m = cabs(z) * f[j];
            if (cleaned_mag && own) cleaned_mag[base + i] = m;
            const double d = own ? (double)m - (double)cm[j] : 0.0; // a zero leaves the sum's bits alone
            sum[5] += d * d;
            z = make_float2(z.x * f[j], z.y * f[j]);
        }
        sm.a[fr * FSTR + k] = z;
    }
    __syncthreads();
    inverse_tile(sm);
    const int64_t n_out = n_seg - 1;
    const int noh = (int)(n_out - o0 < OH ? n_out - o0 : OH);
    const float *seg = reinterpret_cast<const float *>(sm.a);
    float *dst = out ? out + b * (f_pitch - 1) * HOP + o0 * HOP : nullptr;
    const float *ref = clean + b * a_pitch;
    for (int i = threadIdx.x; i < noh * HOP; i += 256) {
        const int j = i >> 7, s = i & 127;
        const int64_t o = o0 + j, g = o0 * HOP + i;
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += seg[(j + q) * (2 * FSTR) + HOP * (3 - q) + s];
        const float cover = 4.0f - (o == 0 ? 1.0f : 0.0f) - (o == n_out - 1 ? 1.0f : 0.0f);
        const float t = acc / cover;
        if (dst) dst[i] = t;
        // samples of the clean clip's length count (zeros otherwise); its hops are in the L2 from the staging above
        const double td = g < T ? (double)t : 0.0, ed = g < T ? (double)ref[g] : 0.0;
        sum[0] += td;
        sum[1] += ed;
        sum[2] += td * td;
        sum[3] += ed * ed;
        sum[4] += td * ed;
    }
    // lanes, then waves in index order; plane B was last read before inverse_tile's closing barrier
    double *red = reinterpret_cast<double *>(sm.b);
#pragma unroll
    for (int c = 0; c < NSUM; ++c) {
        const double w = wave_sum(sum[c]);
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * NSUM + c] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *p = partials + (int64_t)blockIdx.x * NSUM; // blockIdx.x = b * tiles + tile
#pragma unroll
        for (int c = 0; c < NSUM; ++c) p[c] = ((red[c] + red[NSUM + c]) + red[2 * NSUM + c]) + red[3 * NSUM + c];
    }
