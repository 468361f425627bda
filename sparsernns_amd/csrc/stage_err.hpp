// stage_err.hpp -- compare pairs of planes where they lie: the error statistics of the verification report
// (fxpreporter.compute_error) for up to 4096 pairs of strided 3-D boxes in two launches.
//
//   k_stage_err           grid (wgs, pairs): workgroup x of pair y walks elements [x * share, (x + 1) * share) of the box in
//                         row-major order (consecutive lanes on consecutive columns), keeps its sums per thread in double,
//                         its counts per thread in 32 bits and its two exponent histograms in 32-bit LDS words, reduces them
//                         once and stores ONE partial record.  A workgroup without elements stores a zero record.
//   k_stage_err_finalize  grid = pairs: word w of the record is added (maxima: compared) over the pair's partials in index
//                         order by one thread.
//
// Arithmetic, per element (the statement of verify.stage_errors_host): va = (double)a * 2^-a_exp (exact for any int32) or
// (double)a for a float32 a; vb = (double)b; an element whose raw a or b is not finite is counted in n_nonfinite and enters
// nothing else; with RELU_A a negative va becomes +0; e = |va - vb| (one rounding); where vb != 0, rel = e / |vb| (one
// rounding: the division is the correctly rounded one).  sum_sq adds the ROUNDED e * e (contraction is off), sum_ref_sq adds
// vb * vb, which is exact.  The histograms bin (float)e and (float)rel by fm_hist_bin, the rule of the float model's k_*_hist
// kernels.
//
// No floating-point atomics and no global atomics at all: lanes by shuffles, waves through LDS, workgroups by the second
// kernel, each in a fixed order; the LDS atomics add integers.  Two calls give identical bits.
//
// Wrap rule: a thread counts at most share / 256 elements and a histogram word at most share, so the entry refuses a pair
// whose share at the call's cap of workgroups (stage_wgs_cap) could reach 2^32.
#pragma once
#include "float_model.hpp"

namespace s5 {
namespace stage {

constexpr int TPB = 256;           // threads per workgroup
constexpr int UNROLL = 4;          // elements in flight per thread
constexpr int COPIES = 8;          // private copies of a histogram bin, chosen by the lane: [plane][bin][copy]
constexpr int MAX_WGS = 512;       // workgroups per pair, at most
constexpr int WG_BUDGET = 16384;   // workgroups per launch, at most (and partial records in the workspace)
constexpr int64_t WG_MIN_ELEMS = (int64_t)TPB * 16; // a pair below this many elements per workgroup gets fewer workgroups
constexpr int REC_WORDS = 10 + 2 * FM_HIST_BINS;    // s5fxp_stage_err_rec in 8-byte words
constexpr int W_NFIN = 1, W_NEQ = 2, W_NNZ = 3, W_SUM_ABS = 4, W_SUM_SQ = 5, W_MAX_ABS = 6, W_SUM_REF = 7, W_SUM_REL = 8,
              W_MAX_REL = 9, W_HIST = 10;

// the most workgroups per pair a call of n_pairs pairs uses; the workspace holds n_pairs * stage_wgs_cap(n_pairs) partials
constexpr int stage_wgs_cap(int n_pairs)
{
    const int c = WG_BUDGET / (n_pairs < 1 ? 1 : n_pairs);
    return c < 1 ? 1 : c > MAX_WGS ? MAX_WGS : c;
}
// elements per workgroup, a multiple of TPB
constexpr uint64_t stage_share(uint64_t n, int wgs) { return ((n + wgs - 1) / wgs + TPB - 1) / TPB * TPB; }

struct DevPair {
    const uint32_t *a; // int32 or float32, by kind
    const float *b;
    int64_t as[3], bs[3]; // element strides: batch, row, column
    uint64_t n;           // nb * rows * cols
    double scale;         // 2^-a_exp
    uint32_t rows, cols;
    int32_t f32, relu;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const double o = __shfl_down(v, off);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// partials: (pairs, gridDim.x, REC_WORDS) 8-byte words
__global__ __launch_bounds__(TPB) void k_stage_err(const DevPair *__restrict__ pairs, unsigned long long *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ unsigned sh_hist[2 * FM_HIST_BINS * COPIES];
    __shared__ double sh_d[TPB / 64][6];
    __shared__ unsigned sh_c[TPB / 64][3];
    const int tid = threadIdx.x;
    const DevPair p = pairs[blockIdx.y];
    for (int i = tid; i < 2 * FM_HIST_BINS * COPIES; i += TPB) sh_hist[i] = 0;
    __syncthreads();

    const uint64_t share = stage_share(p.n, (int)gridDim.x);
    const uint64_t lo = (uint64_t)blockIdx.x * share;
    const uint64_t begin = lo < p.n ? lo : p.n, end = begin + share < p.n ? begin + share : p.n;
    const uint32_t count = (uint32_t)(end - begin); // below 2^32 by the wrap rule
    const uint32_t iters = (uint32_t)tid < count ? (count - tid + TPB - 1) / TPB : 0;

    double sum_abs = 0, sum_sq = 0, max_abs = 0, sum_ref = 0, sum_rel = 0, max_rel = 0;
    unsigned n_nonfin = 0, n_equal = 0, n_nz = 0;

    if (iters) {
        // this thread's first element, and what TPB elements further on means for (row, column) and the two offsets
        const uint64_t e0 = begin + tid, r0 = e0 / p.cols, b0 = r0 / p.rows;
        uint32_t c = (uint32_t)(e0 - r0 * p.cols), row = (uint32_t)(r0 - b0 * p.rows);
        int64_t oa = (int64_t)b0 * p.as[0] + (int64_t)row * p.as[1] + (int64_t)c * p.as[2];
        int64_t ob = (int64_t)b0 * p.bs[0] + (int64_t)row * p.bs[1] + (int64_t)c * p.bs[2];
        const uint32_t step_r = TPB / p.cols, step_c = TPB - step_r * p.cols;
        const uint32_t step_b = step_r / p.rows, step_rr = step_r - step_b * p.rows;
        const int64_t da = (int64_t)step_b * p.as[0] + (int64_t)step_rr * p.as[1] + (int64_t)step_c * p.as[2];
        const int64_t db = (int64_t)step_b * p.bs[0] + (int64_t)step_rr * p.bs[1] + (int64_t)step_c * p.bs[2];
        const int64_t da_c = p.as[1] - (int64_t)p.cols * p.as[2], db_c = p.bs[1] - (int64_t)p.cols * p.bs[2]; // column wrap
        const int64_t da_r = p.as[0] - (int64_t)p.rows * p.as[1], db_r = p.bs[0] - (int64_t)p.rows * p.bs[1]; // row wrap
        unsigned *const h_abs = sh_hist + (tid & (COPIES - 1)), *const h_rel = h_abs + FM_HIST_BINS * COPIES;

        for (uint32_t k = 0; k < iters; k += UNROLL) {
            uint32_t ua[UNROLL];
            float fb[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                if (k + j < iters) {
                    ua[j] = p.a[oa];
                    fb[j] = p.b[ob];
                }
                c += step_c, row += step_rr, oa += da, ob += db;
                if (c >= p.cols) c -= p.cols, ++row, oa += da_c, ob += db_c;
                if (row >= p.rows) row -= p.rows, oa += da_r, ob += db_r;
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                if (k + j >= iters) break;
                double va;
                bool finite = true;
                if (p.f32) {
                    const float af = __uint_as_float(ua[j]);
                    finite = (ua[j] & 0x7f800000u) != 0x7f800000u;
                    va = (double)af;
                } else {
                    va = (double)(int32_t)ua[j] * p.scale;
                }
                if ((__float_as_uint(fb[j]) & 0x7f800000u) == 0x7f800000u) finite = false;
                if (!finite) {
                    ++n_nonfin;
                    continue;
                }
                if (p.relu && va < 0.0) va = 0.0;
                const double vb = (double)fb[j];
                const double e = fabs(va - vb);
                sum_abs += e;
                sum_sq += e * e;
                sum_ref += vb * vb;
                max_abs = e > max_abs ? e : max_abs;
                n_equal += e == 0.0;
                atomicAdd(h_abs + fm_hist_bin((float)e) * COPIES, 1u);
                if (vb != 0.0) {
                    const double rel = e / fabs(vb);
                    ++n_nz;
                    sum_rel += rel;
                    max_rel = rel > max_rel ? rel : max_rel;
                    atomicAdd(h_rel + fm_hist_bin((float)rel) * COPIES, 1u);
                }
            }
        }
    }

    // lanes by shuffles, waves through LDS, in index order
    const int wave = tid >> 6, lane = tid & 63;
    const double d[6] = {wave_sum(sum_abs), wave_sum(sum_sq), wave_max(max_abs), wave_sum(sum_ref), wave_sum(sum_rel), wave_max(max_rel)};
    const unsigned cn[3] = {wave_sum(n_nonfin), wave_sum(n_equal), wave_sum(n_nz)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) sh_d[wave][i] = d[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) sh_c[wave][i] = cn[i];
    }
    __syncthreads();
    unsigned long long *out = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * REC_WORDS;
    if (tid < 2 * FM_HIST_BINS) { // hist_abs then hist_rel, as the LDS planes lie
        unsigned long long n = 0;
#pragma unroll
        for (int cpy = 0; cpy < COPIES; ++cpy) n += sh_hist[tid * COPIES + cpy];
        out[W_HIST + tid] = n;
    } else if (tid < 2 * FM_HIST_BINS + 6) {
        const int i = tid - 2 * FM_HIST_BINS;
        double v = sh_d[0][i];
        const bool is_max = i == 2 || i == 5;
        for (int w = 1; w < TPB / 64; ++w) v = is_max ? (sh_d[w][i] > v ? sh_d[w][i] : v) : v + sh_d[w][i];
        out[W_SUM_ABS + i] = (unsigned long long)__double_as_longlong(v);
    } else if (tid < 2 * FM_HIST_BINS + 9) {
        const int i = tid - (2 * FM_HIST_BINS + 6);
        unsigned long long v = 0;
        for (int w = 0; w < TPB / 64; ++w) v += sh_c[w][i];
        out[W_NFIN + i] = v;
    } else if (tid == 2 * FM_HIST_BINS + 9) {
        out[0] = count;
    }
}

// ---- clips: the same comparison over a padded box of which clip b holds lens[b] frames ----
//
//   k_stage_err_clips     k_stage_err's grid, shares and reductions over the PADDED box (nb = clips, rows, cols): a workgroup
//                         walks its share of the padded index space and compares element (b, r, c) iff row0 + r < lens[b];
//                         an element outside is never read and belongs to no count, so word 0 of a partial is the number of
//                         elements inside.  With a_exp_dev the integer side of clip b has the exponent
//                         a_exp_dev[b * a_exp_stride], read on the device; an exponent outside 0..40 sends the clip's elements to
//                         n and n_nonfinite and to nothing else.  Finalised by k_stage_err_finalize.
struct DevPairClips {
    DevPair box;
    const int32_t *lens;      // nb, device memory
    const int32_t *a_exp_dev; // or nullptr: box.scale
    int64_t a_exp_stride;
    int32_t row0, pad;
};

__global__ __launch_bounds__(TPB) void k_stage_err_clips(const DevPairClips *__restrict__ pairs, unsigned long long *__restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ unsigned sh_hist[2 * FM_HIST_BINS * COPIES];
    __shared__ double sh_d[TPB / 64][6];
    __shared__ unsigned sh_c[TPB / 64][4];
    const int tid = threadIdx.x;
    const DevPairClips pc = pairs[blockIdx.y];
    const DevPair &p = pc.box;
    for (int i = tid; i < 2 * FM_HIST_BINS * COPIES; i += TPB) sh_hist[i] = 0;
    __syncthreads();

    const uint64_t share = stage_share(p.n, (int)gridDim.x);
    const uint64_t lo = (uint64_t)blockIdx.x * share;
    const uint64_t begin = lo < p.n ? lo : p.n, end = begin + share < p.n ? begin + share : p.n;
    const uint32_t count = (uint32_t)(end - begin); // of the padded box; below 2^32 by the wrap rule
    const uint32_t iters = (uint32_t)tid < count ? (count - tid + TPB - 1) / TPB : 0;

    double sum_abs = 0, sum_sq = 0, max_abs = 0, sum_ref = 0, sum_rel = 0, max_rel = 0;
    unsigned n_in = 0, n_nonfin = 0, n_equal = 0, n_nz = 0;

    if (iters) {
        // k_stage_err's walk, with the clip index carried along
        const uint64_t e0 = begin + tid, r0 = e0 / p.cols, b0 = r0 / p.rows;
        uint32_t c = (uint32_t)(e0 - r0 * p.cols), row = (uint32_t)(r0 - b0 * p.rows), b = (uint32_t)b0;
        int64_t oa = (int64_t)b0 * p.as[0] + (int64_t)row * p.as[1] + (int64_t)c * p.as[2];
        int64_t ob = (int64_t)b0 * p.bs[0] + (int64_t)row * p.bs[1] + (int64_t)c * p.bs[2];
        const uint32_t step_r = TPB / p.cols, step_c = TPB - step_r * p.cols;
        const uint32_t step_b = step_r / p.rows, step_rr = step_r - step_b * p.rows;
        const int64_t da = (int64_t)step_b * p.as[0] + (int64_t)step_rr * p.as[1] + (int64_t)step_c * p.as[2];
        const int64_t db = (int64_t)step_b * p.bs[0] + (int64_t)step_rr * p.bs[1] + (int64_t)step_c * p.bs[2];
        const int64_t da_c = p.as[1] - (int64_t)p.cols * p.as[2], db_c = p.bs[1] - (int64_t)p.cols * p.bs[2]; // column wrap
        const int64_t da_r = p.as[0] - (int64_t)p.rows * p.as[1], db_r = p.bs[0] - (int64_t)p.rows * p.bs[1]; // row wrap
        unsigned *const h_abs = sh_hist + (tid & (COPIES - 1)), *const h_rel = h_abs + FM_HIST_BINS * COPIES;

        for (uint32_t k = 0; k < iters; k += UNROLL) {
            uint32_t ua[UNROLL];
            float fb[UNROLL];
            double sc[UNROLL]; // the clip's 2^-exponent; < 0: outside 0..40
            bool in[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                in[j] = false;
                if (k + j < iters) {
                    // row0 + row < 2^32: both are below 2^31
                    const int32_t len = pc.lens[b];
                    in[j] = len > 0 && (uint32_t)pc.row0 + row < (uint32_t)len;
                    if (in[j]) {
                        ua[j] = p.a[oa];
                        fb[j] = p.b[ob];
                        sc[j] = p.scale;
                        if (pc.a_exp_dev && !p.f32) {
                            const int32_t ex = pc.a_exp_dev[(int64_t)b * pc.a_exp_stride];
                            sc[j] = ex < 0 || ex > 40 ? -1.0 : __longlong_as_double((long long)(1023 - ex) << 52);
                        }
                    }
                }
                c += step_c, row += step_rr, b += step_b, oa += da, ob += db;
                if (c >= p.cols) c -= p.cols, ++row, oa += da_c, ob += db_c;
                if (row >= p.rows) row -= p.rows, ++b, oa += da_r, ob += db_r;
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                if (!in[j]) continue;
                ++n_in;
                double va;
                bool finite = sc[j] >= 0.0;
                if (p.f32) {
                    const float af = __uint_as_float(ua[j]);
                    finite = (ua[j] & 0x7f800000u) != 0x7f800000u;
                    va = (double)af;
                } else {
                    va = (double)(int32_t)ua[j] * sc[j];
                }
                if ((__float_as_uint(fb[j]) & 0x7f800000u) == 0x7f800000u) finite = false;
                if (!finite) {
                    ++n_nonfin;
                    continue;
                }
                if (p.relu && va < 0.0) va = 0.0;
                const double vb = (double)fb[j];
                const double e = fabs(va - vb);
                sum_abs += e;
                sum_sq += e * e;
                sum_ref += vb * vb;
                max_abs = e > max_abs ? e : max_abs;
                n_equal += e == 0.0;
                atomicAdd(h_abs + fm_hist_bin((float)e) * COPIES, 1u);
                if (vb != 0.0) {
                    const double rel = e / fabs(vb);
                    ++n_nz;
                    sum_rel += rel;
                    max_rel = rel > max_rel ? rel : max_rel;
                    atomicAdd(h_rel + fm_hist_bin((float)rel) * COPIES, 1u);
                }
            }
        }
    }

    // lanes by shuffles, waves through LDS, in index order
    const int wave = tid >> 6, lane = tid & 63;
    const double d[6] = {wave_sum(sum_abs), wave_sum(sum_sq), wave_max(max_abs), wave_sum(sum_ref), wave_sum(sum_rel), wave_max(max_rel)};
    const unsigned cn[4] = {wave_sum(n_in), wave_sum(n_nonfin), wave_sum(n_equal), wave_sum(n_nz)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) sh_d[wave][i] = d[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) sh_c[wave][i] = cn[i];
    }
    __syncthreads();
    unsigned long long *out = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * REC_WORDS;
    if (tid < 2 * FM_HIST_BINS) { // hist_abs then hist_rel, as the LDS planes lie
        unsigned long long n = 0;
#pragma unroll
        for (int cpy = 0; cpy < COPIES; ++cpy) n += sh_hist[tid * COPIES + cpy];
        out[W_HIST + tid] = n;
    } else if (tid < 2 * FM_HIST_BINS + 6) {
        const int i = tid - 2 * FM_HIST_BINS;
        double v = sh_d[0][i];
        const bool is_max = i == 2 || i == 5;
        for (int w = 1; w < TPB / 64; ++w) v = is_max ? (sh_d[w][i] > v ? sh_d[w][i] : v) : v + sh_d[w][i];
        out[W_SUM_ABS + i] = (unsigned long long)__double_as_longlong(v);
    } else if (tid < 2 * FM_HIST_BINS + 10) { // n, n_nonfinite, n_equal, n_ref_nonzero: words 0..3
        const int i = tid - (2 * FM_HIST_BINS + 6);
        unsigned long long v = 0;
        for (int w = 0; w < TPB / 64; ++w) v += sh_c[w][i];
        out[i] = v;
    }
}

// grid = pairs, REC_WORDS threads at least: thread w folds word w of the pair's `wgs` partials in index order
__global__ __launch_bounds__(TPB) void k_stage_err_finalize(const unsigned long long *__restrict__ partials, int wgs,
                                                            unsigned long long *__restrict__ out)
{
#pragma clang fp contract(off)
    const int w = threadIdx.x;
    if (w >= REC_WORDS) return;
    const unsigned long long *src = partials + (size_t)blockIdx.x * wgs * REC_WORDS + w;
    unsigned long long r;
    if (w >= W_SUM_ABS && w < W_HIST) {
        double v = __longlong_as_double((long long)src[0]);
        const bool is_max = w == W_MAX_ABS || w == W_MAX_REL;
        for (int i = 1; i < wgs; ++i) {
            const double o = __longlong_as_double((long long)src[(size_t)i * REC_WORDS]);
            v = is_max ? (o > v ? o : v) : v + o;
        }
        r = (unsigned long long)__double_as_longlong(v);
    } else {
        r = 0;
        for (int i = 0; i < wgs; ++i) r += src[(size_t)i * REC_WORDS];
    }
    out[(size_t)blockIdx.x * REC_WORDS + w] = r;
}

} // namespace stage
} // namespace s5
