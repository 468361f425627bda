// audio_stft_mag_body.inc -- the body of k_stft_mag, k_stft_mag_i16 and k_stft_mag_clips (audio_stft.hpp), included with I16 = false /
// true.  The including kernel names the sequence's own T and n_seg and the row pitches of its tensors: a_pitch samples per audio
// row, f_pitch frames per row of x / spec (the batch kernels: T and n_seg themselves).
    __shared__ Smem sm;
    [[maybe_unused]] const float sc = I16 ? ldexpf(1.f, x_exp) : 0.f; // the quantisation scale of an int16 x
    const int64_t b = blockIdx.x / tiles, k0 = (int64_t)(blockIdx.x % tiles) * FR;
    make_twiddles(sm);
    forward_tile(sm, audio + b * a_pitch, T, k0);
    const int nfr = (int)(n_seg - k0 < FR ? n_seg - k0 : FR);
    const int64_t base = (b * f_pitch + k0) * NBIN;
    for (int i = threadIdx.x; i < nfr * NBIN; i += 256) {
        const int fr = i / NBIN, k = i - fr * NBIN;
        const float2 z = bin_from_packed(sm.b + fr * FSTR, sm.tw, k);
        if constexpr (I16) x[base + i] = (int16_t)fromfp(cabs(z) - sub, sc, x_bits);
        else x[base + i] = cabs(z) - sub;
        if (spec) spec[base + i] = z;
    }
