// audio_score_finalize_body.inc -- the body of k_score_finalize and k_score_finalize_clips (audio_score.hpp).  The including kernel
// names the sequence's own T, n_seg and tiles, and `pitch`, the tiles per row of partials (the batch kernel: tiles itself).
    const int c = threadIdx.x;
    double s = 0.0;
    if (c < NSUM) {
        const double *p = partials + (int64_t)blockIdx.x * pitch * NSUM + c;
#pragma unroll 8
        for (int t = 0; t < tiles; ++t) s += p[(int64_t)t * NSUM];
    }
    const double st = __shfl(s, 0), se = __shfl(s, 1), st2 = __shfl(s, 2), se2 = __shfl(s, 3), ste = __shfl(s, 4),
                 sd2 = __shfl(s, 5);
    if (c) return;
    const double N = (double)T;
    const double nt = st2 - st * st / N, ne = se2 - se * se / N, dot = ste - st * se / N;
    const double P = dot * dot / nt;
    const double nz = ne - P > 0.0 ? ne - P : 0.0;
    const double score = 10.0 * log10(P / (nz + 1e-8) + 1e-8);
    const double mse = sd2 / ((double)n_seg * NBIN);
    si_snr[blockIdx.x] = (float)score;
    if (mag_mse) mag_mse[blockIdx.x] = (float)mse;
    if (loss) loss[blockIdx.x] = (float)((double)lam * mse + (100.0 - score));
