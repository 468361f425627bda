// audio_mask_istft_body.inc -- the body of k_mask_istft, k_mask_istft_i16 and k_mask_istft_clips (audio_stft.hpp), included with
// I16 = false / true.  T, n_seg, a_pitch and f_pitch as in audio_stft_mag_body.inc; a row of `out` is f_pitch - 1 hops.
    __shared__ Smem sm;
    const int64_t b = blockIdx.x / tiles, o0 = (int64_t)(blockIdx.x % tiles) * OH, k0 = o0 - 1;
    // this thread's 1 + mask values (elements threadIdx.x + 256 j of the tile's 16 x 257), asked for before the forward
    // transform so that they arrive behind it; a frame outside 0..n_seg-1 contributes nothing
    constexpr int NJ = (FR * NBIN + 255) / 256;
    const int64_t base = (b * f_pitch + k0) * NBIN;
    float f[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = threadIdx.x + 256 * j;
        const int64_t kf = k0 + i / NBIN;
        if constexpr (I16) f[j] = (mask && i < FR * NBIN && kf >= 0 && kf < n_seg) ? 1.0f + tofloat(mask[base + i], mask_exp) : 1.0f;
        else f[j] = (mask && i < FR * NBIN && kf >= 0 && kf < n_seg) ? 1.0f + mask[base + i] : 1.0f;
    }
    make_twiddles(sm);
    forward_tile(sm, audio + b * a_pitch, T, k0);
    // Z' = Z * (1 + mask) into plane A
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = threadIdx.x + 256 * j;
        if (i >= FR * NBIN) break;
        const int fr = i / NBIN, k = i - fr * NBIN;
        const int64_t kf = k0 + fr;
        float2 z = make_float2(0.0f, 0.0f);
        if (kf >= 0 && kf < n_seg) {
            z = bin_from_packed(sm.b + fr * FSTR, sm.tw, k);
            // frames 0, 14 and 15 of a tile are frames 13, 1 and 2 of its neighbours: a tile reports its frames 1..13, the
            // last tile of a sequence also what lies beyond them
            if (cleaned_mag && fr >= 1 && (fr <= OH || o0 + OH >= n_seg - 1)) cleaned_mag[base + i] = cabs(z) * f[j];
            z = make_float2(z.x * f[j], z.y * f[j]);
        }
        sm.a[fr * FSTR + k] = z;
    }
    __syncthreads();
    inverse_tile(sm);
    const int64_t n_out = n_seg - 1;
    const int noh = (int)(n_out - o0 < OH ? n_out - o0 : OH);
    const float *seg = reinterpret_cast<const float *>(sm.a);
    float *dst = out + b * (f_pitch - 1) * HOP + o0 * HOP;
    for (int i = threadIdx.x; i < noh * HOP; i += 256) {
        const int j = i >> 7, s = i & 127;
        const int64_t o = o0 + j;
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += seg[(j + q) * (2 * FSTR) + HOP * (3 - q) + s];
        const float cover = 4.0f - (o == 0 ? 1.0f : 0.0f) - (o == n_out - 1 ? 1.0f : 0.0f);
        dst[i] = acc / cover;
    }
