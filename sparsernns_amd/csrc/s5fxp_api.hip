// s5fxp_api.hip -- host side of libs5fxp.so: the C ABI declared in include/s5fxp.h.
//
// Everything here only validates arguments, packs parameters and enqueues kernels on the
// caller's stream.  No device allocation, no synchronisation, no global mutable state.
#include "../../include/s5fxp.h"
#include "s5fxp_kernels.hpp"
#include "mfma_fused.hpp"
#include "scan_assoc.hpp"
#include "scan_fq.hpp"
#include "audio_stft.hpp"
#include "audio_stream.hpp"
#include "audio_score.hpp"
#include "float_model.hpp"
#include "stage_err.hpp"

#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

using namespace s5;

namespace {

inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }
inline int hip_rc(hipError_t e) { return e == hipSuccess ? S5FXP_OK : S5FXP_EHIP; }
inline int launch_rc() { return hip_rc(hipGetLastError()); }
inline unsigned ew_grid(int64_t n)
{
    int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
inline bool shift_ok(int s) { return s >= 0 && s <= 31; }
// tiles * n workgroups fit a grid's x extent (tiles >= 0, n >= 1; the product itself may not fit 64 bits)
inline bool grid_fits(int64_t tiles, int64_t n) { return tiles <= 0x7fffffffll / n; }

// Workspace sizes are formed in 128 bits, where no product of three ints and a few small factors can wrap, and narrowed once:
// a size that does not fit a size_t becomes 0, which every size query returns for "no such workspace" and every entry refuses
using wide_t = unsigned __int128;
inline wide_t wide_al256(wide_t v) { return (v + 255) & ~(wide_t)255; }
inline size_t fit_size(wide_t v) { return v > (wide_t)SIZE_MAX ? 0 : (size_t)v; }
// time blocks (4 steps each) of an L-frame sequence, padded to a multiple of depth; L + 3 itself may not fit an int
inline int64_t time_blocks(int L, int depth) { return (((int64_t)L + 3) / 4 + depth - 1) / depth * depth; }

// column split of the frame-tiled matmul: 4 waves x mw columns, mw % 4 == 0
inline int mw_for(int M) { return ((M + 3) / 4 + 3) / 4 * 4; }
constexpr int MW_LIMIT = 68;

// dispatch on the compile-time column budget
#define S5_DISPATCH_MW(mw, X24, KERNEL, grid, stream, args)                                                   \
    do {                                                                                                      \
        if ((mw) <= 4) hipLaunchKernelGGL((KERNEL<4, X24>), dim3(grid), dim3(256), 0, stream, args);          \
        else if ((mw) <= 8) hipLaunchKernelGGL((KERNEL<8, X24>), dim3(grid), dim3(256), 0, stream, args);     \
        else if ((mw) <= 16) hipLaunchKernelGGL((KERNEL<16, X24>), dim3(grid), dim3(256), 0, stream, args);   \
        else if ((mw) <= 24) hipLaunchKernelGGL((KERNEL<24, X24>), dim3(grid), dim3(256), 0, stream, args);   \
        else if ((mw) <= 32) hipLaunchKernelGGL((KERNEL<32, X24>), dim3(grid), dim3(256), 0, stream, args);   \
        else if ((mw) <= 48) hipLaunchKernelGGL((KERNEL<48, X24>), dim3(grid), dim3(256), 0, stream, args);   \
        else if ((mw) <= 64) hipLaunchKernelGGL((KERNEL<64, X24>), dim3(grid), dim3(256), 0, stream, args);   \
        else hipLaunchKernelGGL((KERNEL<68, X24>), dim3(grid), dim3(256), 0, stream, args);                   \
    } while (0)

// k_cproj keeps two output tiles in LDS; its column budget stops at 48 (H <= 192)
#define S5_DISPATCH_MW_C(mw, X24, PASS, AT, grid, stream, args)                                                         \
    do {                                                                                                      \
        if ((mw) <= 4) hipLaunchKernelGGL((k_cproj<4, X24, PASS, AT>), dim3(grid), dim3(256), 0, stream, args);         \
        else if ((mw) <= 8) hipLaunchKernelGGL((k_cproj<8, X24, PASS, AT>), dim3(grid), dim3(256), 0, stream, args);    \
        else if ((mw) <= 16) hipLaunchKernelGGL((k_cproj<16, X24, PASS, AT>), dim3(grid), dim3(256), 0, stream, args);  \
        else if ((mw) <= 24) hipLaunchKernelGGL((k_cproj<24, X24, PASS, AT>), dim3(grid), dim3(256), 0, stream, args);  \
        else if ((mw) <= 32) hipLaunchKernelGGL((k_cproj<32, X24, PASS, AT>), dim3(grid), dim3(256), 0, stream, args);  \
        else hipLaunchKernelGGL((k_cproj<48, X24, PASS, AT>), dim3(grid), dim3(256), 0, stream, args);                  \
    } while (0)
constexpr int MW_LIMIT_C = 48;

bool fits24(const int32_t *p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (p[i] < -(1 << 23) || p[i] >= (1 << 23)) return false;
    return true;
}

} // namespace

// -----------------------------------------------------------------------------------------------
extern "C" int s5fxp_version(void) { return S5FXP_VERSION; }

extern "C" const char *s5fxp_strerror(int code)
{
    switch (code) {
    case S5FXP_OK: return "ok";
    case S5FXP_EBADARG: return "bad argument";
    case S5FXP_ENEGSHIFT: return "negative or out-of-range shift (invalid result_exp)";
    case S5FXP_EUNSUPPORTED: return "unsupported configuration";
    case S5FXP_EHIP: return "HIP runtime error";
    case S5FXP_EWORKSPACE: return "workspace or blob too small";
    default: return "unknown error";
    }
}

// -----------------------------------------------------------------------------------------------
// op level
// -----------------------------------------------------------------------------------------------
extern "C" int s5fxp_from_fp(const float *x, int32_t *y, int64_t n, int bits, int exp, int round_mode, void *stream)
{
    if (!x || !y || n < 0 || bits < 1 || bits > 32 || exp < 0 || exp > 31 || round_mode < 0 || round_mode > 2)
        return S5FXP_EBADARG;
    if (n == 0) return S5FXP_OK;
    hipLaunchKernelGGL(k_from_fp, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, n, bits, exp, round_mode);
    return launch_rc();
}

extern "C" int s5fxp_to_float(const int32_t *x, float *y, int64_t n, int exp, void *stream)
{
    if (!x || !y || n < 0 || exp < 0 || exp > 31) return S5FXP_EBADARG;
    if (n == 0) return S5FXP_OK;
    hipLaunchKernelGGL(k_to_float, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, n, exp);
    return launch_rc();
}

extern "C" int s5fxp_change_cfg(const int32_t *x, int32_t *y, int64_t n, int bits, int exp, int new_bits, int new_exp,
                                void *stream)
{
    if (!x || !y || n < 0 || bits < 1 || bits > 32 || new_bits < 1 || new_bits > 32) return S5FXP_EBADARG;
    if (!shift_ok(exp > new_exp ? exp - new_exp : new_exp - exp)) return S5FXP_ENEGSHIFT;
    if (n == 0) return S5FXP_OK;
    hipLaunchKernelGGL(k_change_cfg, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, n, bits, exp, new_bits, new_exp);
    return launch_rc();
}

extern "C" int s5fxp_dense(const int32_t *x, const int32_t *w, const int32_t *bias, int32_t *y, int64_t N, int K, int M,
                           int x_exp, int w_exp, int b_bits, int b_exp, int out_bits, int out_exp, int flags,
                           void *stream)
{
    if (!x || !w || !y || N < 0 || K < 1 || M < 1 || out_bits < 1 || out_bits > 32) return S5FXP_EBADARG;
    if (mw_for(M) > MW_LIMIT) return S5FXP_EUNSUPPORTED;
    if (!shift_ok(x_exp + w_exp - out_exp)) return S5FXP_ENEGSHIFT;
    if (bias && !shift_ok(b_exp > out_exp ? b_exp - out_exp : out_exp - b_exp)) return S5FXP_ENEGSHIFT;
    if (N == 0) return S5FXP_OK;
    DenseArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.N = N; a.K = K; a.M = M; a.mw = mw_for(M);
    a.xb = 32; a.xe = DynExp{x_exp, nullptr}; a.check_inp = 0;
    a.w_exp = w_exp; a.b_bits = b_bits; a.b_exp = b_exp; a.out_bits = out_bits; a.out_exp = out_exp;
    a.relu = flags & 1; a.check24 = 0; a.status = nullptr;
    const unsigned grid = (unsigned)((N + TN - 1) / TN);
    S5_DISPATCH_MW(a.mw, false, k_dense, grid, S(stream), a);
    return launch_rc();
}

extern "C" int s5fxp_dense_csr(const int32_t *x, const int32_t *rowptr, const int32_t *colidx, const int32_t *val,
                               const int32_t *bias, int32_t *y, int64_t N, int K, int M, int x_exp, int w_exp, int b_bits,
                               int b_exp, int out_bits, int out_exp, int flags, void *stream)
{
    if (!x || !rowptr || !y || N < 0 || K < 1 || M < 1 || out_bits < 1 || out_bits > 32) return S5FXP_EBADARG;
    if (!colidx || !val) return S5FXP_EBADARG;
    const size_t smem = (size_t)(64 * (K | 1) + 64 * 65) * 4;
    if (smem > 160 * 1024) return S5FXP_EUNSUPPORTED; // K <= 574: the input tile must fit one CU's LDS
    if (!shift_ok(x_exp + w_exp - out_exp)) return S5FXP_ENEGSHIFT;
    if (bias && !shift_ok(b_exp > out_exp ? b_exp - out_exp : out_exp - b_exp)) return S5FXP_ENEGSHIFT;
    if (N == 0) return S5FXP_OK;
    DenseCsrArgs a{};
    a.x = x; a.rowptr = rowptr; a.colidx = colidx; a.val = val; a.bias = bias; a.y = y; a.N = N; a.K = K; a.M = M;
    a.rs = x_exp + w_exp - out_exp; a.b_bits = b_bits; a.b_exp = b_exp; a.out_bits = out_bits; a.out_exp = out_exp;
    a.relu = flags & 1;
    if (smem > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_dense_csr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL(k_dense_csr, dim3((unsigned)((N + 63) / 64)), dim3(256), smem, S(stream), a);
    return launch_rc();
}

extern "C" int s5fxp_add(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_bits,
                         int x_exp, int y_bits, int y_exp, int out_bits, int out_exp, int negate_y, void *stream)
{
    if (!x || !y || !out || n < 0 || y_len < 1 || (n % y_len) != 0) return S5FXP_EBADARG;
    if (!shift_ok(x_exp > out_exp ? x_exp - out_exp : out_exp - x_exp) ||
        !shift_ok(y_exp > out_exp ? y_exp - out_exp : out_exp - y_exp))
        return S5FXP_ENEGSHIFT;
    if (n == 0) return S5FXP_OK;
    hipLaunchKernelGGL(k_add, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, out, n, y_len, x_bits, x_exp, y_bits,
                       y_exp, out_bits, out_exp, negate_y);
    return launch_rc();
}

extern "C" int s5fxp_mul(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_exp,
                         int y_exp, int out_bits, int out_exp, void *stream)
{
    if (!x || !y || !out || n < 0 || y_len < 1 || (n % y_len) != 0) return S5FXP_EBADARG;
    const int rs = x_exp + y_exp - out_exp;
    if (!shift_ok(rs)) return S5FXP_ENEGSHIFT; // fxparray.py:619-621
    if (n == 0) return S5FXP_OK;
    hipLaunchKernelGGL(k_mul, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, out, n, y_len, rs, out_bits);
    return launch_rc();
}

static int cb_common(bool is_mul, const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len,
                     int x_bits, int x_exp, int y_bits, int y_exp, int out_bits, int32_t *out_exp_dev, void *scratch,
                     void *stream)
{
    if (!x || !y || !out || !out_exp_dev || !scratch || n < 1 || y_len < 1 || (n % y_len) != 0) return S5FXP_EBADARG;
    uint32_t *sc = reinterpret_cast<uint32_t *>(scratch);
    int rc = hip_rc(hipMemsetAsync(sc, 0, 32, S(stream)));
    if (rc) return rc;
    if (is_mul) {
        hipLaunchKernelGGL(k_cb_reduce<true>, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, n, y_len, x_exp, y_exp, sc);
        hipLaunchKernelGGL(k_cb_finalize, dim3(1), dim3(64), 0, S(stream), sc, x_exp, y_exp, out_bits, 1, out_exp_dev);
        hipLaunchKernelGGL(k_cb_apply<true>, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, out, n, y_len, x_bits,
                           y_bits, out_bits, sc);
    } else {
        hipLaunchKernelGGL(k_cb_reduce<false>, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, n, y_len, x_exp, y_exp, sc);
        hipLaunchKernelGGL(k_cb_finalize, dim3(1), dim3(64), 0, S(stream), sc, x_exp, y_exp, out_bits, 0, out_exp_dev);
        hipLaunchKernelGGL(k_cb_apply<false>, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, out, n, y_len, x_bits,
                           y_bits, out_bits, sc);
    }
    return launch_rc();
}

extern "C" int s5fxp_add_cb(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_bits,
                            int x_exp, int y_bits, int y_exp, int out_bits, int32_t *out_exp_dev, void *scratch,
                            void *stream)
{
    return cb_common(false, x, y, out, n, y_len, x_bits, x_exp, y_bits, y_exp, out_bits, out_exp_dev, scratch, stream);
}

extern "C" int s5fxp_mul_cb(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_exp,
                            int y_exp, int out_bits, int32_t *out_exp_dev, void *scratch, void *stream)
{
    return cb_common(true, x, y, out, n, y_len, 32, x_exp, 32, y_exp, out_bits, out_exp_dev, scratch, stream);
}

extern "C" int s5fxp_relu(const int32_t *re, const int32_t *im, int32_t *out_re, int32_t *out_im, int64_t n,
                          void *stream)
{
    if (!re || !out_re || n < 0 || (im && !out_im)) return S5FXP_EBADARG;
    if (n == 0) return S5FXP_OK;
    hipLaunchKernelGGL(k_relu, dim3(ew_grid(n)), dim3(256), 0, S(stream), re, im, out_re, out_im, n);
    return launch_rc();
}

extern "C" int s5fxp_sigmoid(const int32_t *x, int32_t *y, int64_t n, int x_bits, int x_exp, int sig_x_exp,
                             int sig_y_exp, const int32_t *lut_host, void *stream)
{
    if (!x || !y || !lut_host || n < 0 || sig_x_exp < 0 || sig_x_exp > 15 || sig_y_exp < 1 || sig_y_exp > 30)
        return S5FXP_EBADARG;
    if (!shift_ok(x_exp > sig_x_exp ? x_exp - sig_x_exp : sig_x_exp - x_exp)) return S5FXP_ENEGSHIFT;
    if (n == 0) return S5FXP_OK;
    Lut8 l;
    for (int i = 0; i < 8; ++i) l.v[i] = lut_host[i];
    hipLaunchKernelGGL(k_sigmoid, dim3(ew_grid(n)), dim3(256), 0, S(stream), x, y, n, x_bits, x_exp, sig_x_exp,
                       sig_y_exp, l);
    return launch_rc();
}

static int launch_scan(ScanArgs &a, hipStream_t st)
{
    const int64_t total = (int64_t)a.B * a.P;
    const unsigned grid = (unsigned)((total + 63) / 64);
    hipLaunchKernelGGL(k_scan_lane<8>, dim3(grid), dim3(64), 0, st, a);
    return launch_rc();
}

extern "C" int s5fxp_scan(const int32_t *bu_re, const int32_t *bu_im, const int32_t *a_re, const int32_t *a_im,
                          int32_t *xs_re, int32_t *xs_im, int B, int L, int P, int a_re_exp, int a_im_exp,
                          int bu_re_exp, int bu_im_exp, int x_re_exp, int x_im_exp, int flags, void *stream)
{
    if (!bu_re || !bu_im || !a_re || !a_im || !xs_re || !xs_im || B < 0 || L < 0 || P < 1) return S5FXP_EBADARG;
    const int sr = bu_re_exp - x_re_exp, si = bu_im_exp - x_im_exp;
    if (!shift_ok(a_re_exp) || !shift_ok(a_im_exp) || !shift_ok(sr < 0 ? -sr : sr) || !shift_ok(si < 0 ? -si : si))
        return S5FXP_ENEGSHIFT;
    if (B == 0 || L == 0) return S5FXP_OK;
    ScanArgs a{};
    a.bu_re = bu_re; a.bu_im = bu_im; a.a_re = a_re; a.a_im = a_im; a.out_re = xs_re; a.out_im = xs_im;
    a.B = B; a.L = L; a.P = P; a.TB = 0; a.ea_re = a_re_exp; a.ea_im = a_im_exp; a.sh_re = sr; a.sh_im = si;
    a.relu = flags & 1; a.run_if = nullptr;
    return launch_scan(a, S(stream));
}

extern "C" int s5fxp_assoc_scan_c64(const float *lambda, const float *bu, float *xs, const float *x0, float *x_last, int B,
                                    int L, int P, int reverse, void *stream)
{
    if (!lambda || !bu || !xs || B < 0 || L < 0 || P < 1) return S5FXP_EBADARG;
    if (B == 0 || L == 0) return S5FXP_OK;
    const int64_t grid = (int64_t)B * (((int64_t)P + ASSOC_PT - 1) / ASSOC_PT);
    if (grid > 0x7fffffffll) return S5FXP_EBADARG;
    ScanAssocArgs a{};
    a.lambda = reinterpret_cast<const float2 *>(lambda); a.bu = reinterpret_cast<const float2 *>(bu);
    a.xs = reinterpret_cast<float2 *>(xs); a.x0 = reinterpret_cast<const float2 *>(x0);
    a.x_last = reinterpret_cast<float2 *>(x_last); a.B = B; a.L = L; a.P = P; a.reverse = reverse ? 1 : 0;
    hipLaunchKernelGGL(k_scan_assoc_c64, dim3((unsigned)grid), dim3(64 * ASSOC_WAVES), 0, S(stream), a);
    return launch_rc();
}

extern "C" int s5fxp_fq_scan_c64(const float *lambda, const float *bu, float *xs, const float *x0, float *x_last,
                                 const int32_t *lens, int B, int L, int P, int exp_re, int exp_im, void *stream)
{
    if (!lambda || !bu || !xs || B < 1 || L < 1 || P < 1) return S5FXP_EBADARG;
    if (exp_re < -24 || exp_re > 40 || exp_im < -24 || exp_im > 40) return S5FXP_EBADARG;
    const int64_t grid = ((int64_t)B * P + 63) / 64; // one wave per workgroup
    if (grid > 0x7fffffffll || !fqs_span_ok(L, P)) return S5FXP_EBADARG;
    ScanFqArgs a{};
    a.lambda = reinterpret_cast<const float2 *>(lambda); a.bu = reinterpret_cast<const float2 *>(bu);
    a.xs = reinterpret_cast<float2 *>(xs); a.x0 = reinterpret_cast<const float2 *>(x0);
    a.x_last = reinterpret_cast<float2 *>(x_last); a.lens = lens; a.B = B; a.L = L; a.P = P;
    a.sr = ldexpf(1.f, exp_re); a.isr = ldexpf(1.f, -exp_re); a.si = ldexpf(1.f, exp_im); a.isi = ldexpf(1.f, -exp_im);
    hipLaunchKernelGGL(k_scan_fq_c64, dim3((unsigned)grid), dim3(64), 0, S(stream), a);
    return launch_rc();
}

// The audio steps either side of the model (audio_stft.hpp).  n_seg = ceil(T / 128) + 1 frames for T >= 512.
extern "C" int64_t s5fxp_stft_frames(int64_t T) { return T < stft::NFFT ? -1 : T / stft::HOP + (T % stft::HOP != 0) + 1; }

// One checked launch per direction: the arguments and the tile arithmetic the float and the int16 entry share.  extra_ok: the
// boundary's own argument checks; launch(grid, n_seg, tiles) enqueues its kernel.
namespace {
template <class Launch>
int stft_mag_entry(const float *audio, const void *x, int B, int64_t T, bool extra_ok, Launch launch)
{
    if (!audio || !x || B < 1 || !extra_ok) return S5FXP_EBADARG;
    if (T < stft::NFFT) return S5FXP_EUNSUPPORTED;
    const int64_t n_seg = s5fxp_stft_frames(T), tiles = (n_seg + stft::FR - 1) / stft::FR;
    if (!grid_fits(tiles, B)) return S5FXP_EUNSUPPORTED;
    launch(dim3((unsigned)(tiles * B)), n_seg, (int)tiles);
    return launch_rc();
}

template <class Launch>
int mask_istft_entry(const float *audio, const float *out, int B, int64_t T, bool extra_ok, Launch launch)
{
    if (!audio || !out || B < 1 || !extra_ok) return S5FXP_EBADARG;
    if (T < stft::NFFT) return S5FXP_EUNSUPPORTED;
    const int64_t n_seg = s5fxp_stft_frames(T), tiles = (n_seg - 1 + stft::OH - 1) / stft::OH;
    if (!grid_fits(tiles, B)) return S5FXP_EUNSUPPORTED;
    launch(dim3((unsigned)(tiles * B)), n_seg, (int)tiles);
    return launch_rc();
}
} // namespace

extern "C" int s5fxp_stft_mag(const float *audio, int B, int64_t T, float sub, float *x, float *spec, void *stream)
{
    return stft_mag_entry(audio, x, B, T, true, [&](dim3 grid, int64_t n_seg, int tiles) {
        hipLaunchKernelGGL(stft::k_stft_mag, grid, dim3(256), 0, S(stream), audio, T, n_seg, tiles, sub, x, reinterpret_cast<float2 *>(spec));
    });
}

extern "C" int s5fxp_mask_istft(const float *audio, const float *mask, int B, int64_t T, float *out, float *cleaned_mag,
                                void *stream)
{
    return mask_istft_entry(audio, out, B, T, true, [&](dim3 grid, int64_t n_seg, int tiles) {
        hipLaunchKernelGGL(stft::k_mask_istft, grid, dim3(256), 0, S(stream), audio, mask, T, n_seg, tiles, out, cleaned_mag);
    });
}

// ... with the model's int16 boundary (s5fxp_model_forward_i16) on the model's side of both
extern "C" int s5fxp_stft_mag_i16(const float *audio, int B, int64_t T, float sub, int x_bits, int x_exp, int16_t *x, float *spec,
                                  void *stream)
{
    return stft_mag_entry(audio, x, B, T, x_bits >= 1 && x_bits <= 16 && shift_ok(x_exp), [&](dim3 grid, int64_t n_seg, int tiles) {
        hipLaunchKernelGGL(stft::k_stft_mag_i16, grid, dim3(256), 0, S(stream), audio, T, n_seg, tiles, sub, x_bits, x_exp, x,
                           reinterpret_cast<float2 *>(spec));
    });
}

extern "C" int s5fxp_mask_istft_i16(const float *audio, const int16_t *mask, int mask_exp, int B, int64_t T, float *out,
                                    float *cleaned_mag, void *stream)
{
    return mask_istft_entry(audio, out, B, T, shift_ok(mask_exp), [&](dim3 grid, int64_t n_seg, int tiles) {
        hipLaunchKernelGGL(stft::k_mask_istft_i16, grid, dim3(256), 0, S(stream), audio, mask, mask_exp, T, n_seg, tiles, out, cleaned_mag);
    });
}

// ... for n clips of different lengths in one launch each (k_stft_mag_clips / k_mask_istft_clips): the rows are padded to Tmax
// samples and Lmax = frames(Tmax) frames, the clip's own length comes from `samples` on the device
namespace {
int clips_audio_args(const void *audio, const void *samples, const void *io, int n, int64_t Tmax)
{
    if (!audio || !samples || !io || n < 1 || Tmax > ((1ll << 20) - 1) * stft::HOP) return S5FXP_EBADARG;
    return Tmax < stft::NFFT ? S5FXP_EUNSUPPORTED : S5FXP_OK;
}
} // namespace

extern "C" int s5fxp_stft_mag_clips(const float *audio, int n, int64_t Tmax, const int32_t *samples, float sub, float *x, float *spec,
                                    int32_t *lens, void *stream)
{
    if (const int rc = clips_audio_args(audio, samples, x, n, Tmax)) return rc;
    const int64_t Lmax = s5fxp_stft_frames(Tmax), tiles = (Lmax + stft::FR - 1) / stft::FR;
    if (tiles * n > 0x7fffffffll) return S5FXP_EUNSUPPORTED;
    hipLaunchKernelGGL(stft::k_stft_mag_clips, dim3((unsigned)(tiles * n)), dim3(256), 0, S(stream), audio, Tmax, Lmax, (int)tiles,
                       samples, sub, x, reinterpret_cast<float2 *>(spec), lens);
    return launch_rc();
}

extern "C" int s5fxp_mask_istft_clips(const float *audio, const float *mask, int n, int64_t Tmax, const int32_t *samples, float *out,
                                      float *cleaned_mag, void *stream)
{
    if (const int rc = clips_audio_args(audio, samples, out, n, Tmax)) return rc;
    const int64_t Lmax = s5fxp_stft_frames(Tmax), tiles = (Lmax - 1 + stft::OH - 1) / stft::OH;
    if (tiles * n > 0x7fffffffll) return S5FXP_EUNSUPPORTED;
    hipLaunchKernelGGL(stft::k_mask_istft_clips, dim3((unsigned)(tiles * n)), dim3(256), 0, S(stream), audio, mask, Tmax, Lmax,
                       (int)tiles, samples, out, cleaned_mag);
    return launch_rc();
}

// The masked inverse with the validation step's scores (audio_score.hpp): the tile sums go through `workspace`, a second small
// launch forms si_snr, mag_mse and loss per sequence.
extern "C" size_t s5fxp_score_workspace_bytes(int B, int64_t T)
{
    if (B < 1 || T < stft::NFFT) return 0;
    const int64_t tiles = (s5fxp_stft_frames(T) - 1 + stft::OH - 1) / stft::OH;
    if (!grid_fits(tiles, B)) return 0; // s5fxp_mask_istft_score refuses it; the size would not fit a size_t either
    return (size_t)B * (size_t)tiles * stft::NSUM * sizeof(double);
}

namespace {
template <class Launch>
int score_entry(const float *audio, const float *clean, int B, int64_t T, float lam, const void *workspace, size_t workspace_bytes,
                float *si_snr, float *mag_mse, float *loss, bool extra_ok, void *stream, Launch launch)
{
    if (!audio || !clean || !workspace || !si_snr || B < 1 || !extra_ok) return S5FXP_EBADARG;
    if (T < stft::NFFT) return S5FXP_EUNSUPPORTED;
    const int64_t n_seg = s5fxp_stft_frames(T), tiles = (n_seg - 1 + stft::OH - 1) / stft::OH;
    if (!grid_fits(tiles, B)) return S5FXP_EUNSUPPORTED;
    if (workspace_bytes < s5fxp_score_workspace_bytes(B, T)) return S5FXP_EWORKSPACE;
    launch(dim3((unsigned)(tiles * B)), n_seg, (int)tiles);
    hipLaunchKernelGGL(stft::k_score_finalize, dim3((unsigned)B), dim3(64), 0, S(stream), static_cast<const double *>(workspace),
                       (int)tiles, T, n_seg, lam, si_snr, mag_mse, loss);
    return launch_rc();
}
} // namespace

extern "C" int s5fxp_mask_istft_score(const float *audio, const float *clean, const float *mask, int B, int64_t T, float lam,
                                      float *out, float *cleaned_mag, void *workspace, size_t workspace_bytes, float *si_snr,
                                      float *mag_mse, float *loss, void *stream)
{
    return score_entry(audio, clean, B, T, lam, workspace, workspace_bytes, si_snr, mag_mse, loss, true, stream,
                       [&](dim3 grid, int64_t n_seg, int tiles) {
        hipLaunchKernelGGL(stft::k_mask_istft_score, grid, dim3(256), 0, S(stream), audio, clean, mask, T, n_seg, tiles, out, cleaned_mag,
                           static_cast<double *>(workspace));
    });
}

extern "C" int s5fxp_mask_istft_score_i16(const float *audio, const float *clean, const int16_t *mask, int mask_exp, int B, int64_t T,
                                          float lam, float *out, float *cleaned_mag, void *workspace, size_t workspace_bytes,
                                          float *si_snr, float *mag_mse, float *loss, void *stream)
{
    return score_entry(audio, clean, B, T, lam, workspace, workspace_bytes, si_snr, mag_mse, loss, shift_ok(mask_exp), stream,
                       [&](dim3 grid, int64_t n_seg, int tiles) {
        hipLaunchKernelGGL(stft::k_mask_istft_score_i16, grid, dim3(256), 0, S(stream), audio, clean, mask, mask_exp, T, n_seg, tiles, out,
                           cleaned_mag, static_cast<double *>(workspace));
    });
}

// ... for n clips of different lengths (k_mask_istft_score_clips / k_score_finalize_clips): the layouts of s5fxp_mask_istft_clips,
// clean padded like audio, one score per clip over its own length
extern "C" size_t s5fxp_score_clips_workspace_bytes(int n, int64_t Tmax)
{
    if (n < 1 || Tmax < stft::NFFT || Tmax > ((1ll << 20) - 1) * stft::HOP) return 0;
    const int64_t tiles = (s5fxp_stft_frames(Tmax) - 1 + stft::OH - 1) / stft::OH;
    return (size_t)n * (size_t)tiles * stft::NSUM * sizeof(double);
}

extern "C" int s5fxp_mask_istft_score_clips(const float *audio, const float *clean, const float *mask, int n, int64_t Tmax,
                                            const int32_t *samples, float lam, float *out, float *cleaned_mag, void *workspace,
                                            size_t workspace_bytes, float *si_snr, float *mag_mse, float *loss, void *stream)
{
    if (!clean || !workspace) return S5FXP_EBADARG;
    if (const int rc = clips_audio_args(audio, samples, si_snr, n, Tmax)) return rc;
    const int64_t Lmax = s5fxp_stft_frames(Tmax), tiles = (Lmax - 1 + stft::OH - 1) / stft::OH;
    if (tiles * n > 0x7fffffffll) return S5FXP_EUNSUPPORTED;
    if (workspace_bytes < s5fxp_score_clips_workspace_bytes(n, Tmax)) return S5FXP_EWORKSPACE;
    hipLaunchKernelGGL(stft::k_mask_istft_score_clips, dim3((unsigned)(tiles * n)), dim3(256), 0, S(stream), audio, clean, mask, Tmax,
                       Lmax, (int)tiles, samples, out, cleaned_mag, static_cast<double *>(workspace));
    hipLaunchKernelGGL(stft::k_score_finalize_clips, dim3((unsigned)n), dim3(64), 0, S(stream), static_cast<const double *>(workspace),
                       (int)tiles, Tmax, samples, lam, si_snr, mag_mse, loss);
    return launch_rc();
}

// The same framing for a live signal (audio_stream.hpp): whole hops in, cleaned hops out, the caller's state between calls.
extern "C" size_t s5fxp_stream_audio_state_bytes(void) { return stft::STATE_FLOATS * sizeof(float); }

extern "C" int64_t s5fxp_stream_frames(int64_t hops_before, int c)
{
    if (hops_before < 0 || c < 1 || c > stft::STREAM_MAX_HOPS) return -1;
    return c - (hops_before == 0 ? 1 : 0);
}

extern "C" int64_t s5fxp_stream_out_hops(int64_t hops_before, int c, int final)
{
    if (hops_before < 0 || c < 1 || c > stft::STREAM_MAX_HOPS) return -1;
    const int64_t ready = hops_before >= 3 ? c : hops_before + c - 3; // min(c, .): hops_before + c may not fit
    return (ready < 0 ? 0 : ready) + (final ? 1 : 0);
}

extern "C" int s5fxp_stream_stft(const float *audio, int n, int c, int64_t hops_before, float sub, void *state, float *x,
                                 void *stream)
{
    if (!state || n < 1 || s5fxp_stream_frames(hops_before, c) < 0) return S5FXP_EBADARG;
    if (!x && s5fxp_stream_frames(hops_before, c) > 0) return S5FXP_EBADARG;
    hipLaunchKernelGGL(stft::k_stream_stft, dim3((unsigned)n), dim3(256), 0, S(stream), audio, c, hops_before == 0 ? 1 : 0, sub,
                       static_cast<float *>(state), x);
    return launch_rc();
}

extern "C" int s5fxp_stream_mask_istft(const float *mask, int n, int c, int64_t hops_before, int final, void *state, float *out,
                                       float *cleaned_mag, void *stream)
{
    if (!state || n < 1 || s5fxp_stream_frames(hops_before, c) < 0) return S5FXP_EBADARG;
    if (!out && s5fxp_stream_out_hops(hops_before, c, final) > 0) return S5FXP_EBADARG;
    if (final && hops_before < 4) return S5FXP_EUNSUPPORTED;
    hipLaunchKernelGGL(stft::k_stream_mask_istft, dim3((unsigned)n), dim3(256), 0, S(stream), mask, c,
                       (int)(hops_before < 4 ? hops_before : 4), final ? 1 : 0, static_cast<float *>(state), out, cleaned_mag);
    return launch_rc();
}

// The two with per-entry c, h4, flags and state slot, read from a device array of descriptors (audio_stream.hpp)
extern "C" int s5fxp_stream_stft_ragged(const float *audio, int n, int cmax, const s5fxp_push_desc *desc, float sub, void *state,
                                        int n_slots, float *x, void *stream)
{
    if (!desc || !state || !x || n < 1 || n_slots < 1 || cmax < 1 || cmax > stft::STREAM_MAX_HOPS) return S5FXP_EBADARG;
    hipLaunchKernelGGL(stft::k_stream_stft_ragged, dim3((unsigned)n), dim3(256), 0, S(stream), audio, cmax, desc, sub,
                       static_cast<float *>(state), x);
    return launch_rc();
}

extern "C" int s5fxp_stream_mask_istft_ragged(const float *mask, int n, int cmax, const s5fxp_push_desc *desc, void *state,
                                              int n_slots, float *out, float *cleaned_mag, void *stream)
{
    if (!desc || !state || !out || n < 1 || n_slots < 1 || cmax < 1 || cmax > stft::STREAM_MAX_HOPS) return S5FXP_EBADARG;
    hipLaunchKernelGGL(stft::k_stream_mask_istft_ragged, dim3((unsigned)n), dim3(256), 0, S(stream), mask, cmax, desc,
                       static_cast<float *>(state), out, cleaned_mag);
    return launch_rc();
}

// -----------------------------------------------------------------------------------------------
// model level
// -----------------------------------------------------------------------------------------------
struct DenseDev {
    int K = 0, M = 0;
    const int32_t *w = nullptr, *bias = nullptr;
    int w_exp = 0, b_bits = 0, b_exp = 0, inp_bits = 0, inp_exp = 0, out_bits = 0, out_exp = 0;
    bool x24 = false;
};

struct LayerDev {
    // norm
    const int32_t *mm = nullptr, *isv = nullptr, *scale = nullptr, *nbias = nullptr;
    s5fxp_norm_desc nd{};
    // ssm
    const int32_t *a_re = nullptr, *a_im = nullptr, *bcat = nullptr, *c_re_t = nullptr, *c_im_t = nullptr, *D = nullptr;
    s5fxp_ssm_desc sd{};
    bool b24 = false, c24 = false;
    bool quad_ok = false; // quad recurrence kernel applicable (P % 16 == 0, coefficients fit 24 bits)
    int32_t quad_xmax = 0; // its exactness bound on |state|
    bool pair_ok = false;  // pair recurrence kernel applicable (scan_quad.hpp k_scan_pair_asm)
    int32_t pair_xmax = 0; // its exactness bound on |state|
    DenseDev out2;
    int l_bits, l_exp, r_bits, r_exp, res_bits, res_exp, sig_x, sig_y;
    int32_t lut[8];
};

struct FastModel; // int8-MFMA path (s5fxp_fast.hpp); nullptr when the model is not eligible

// Experiment / test switches.  They are read from the environment ONCE, in s5fxp_model_create, and live in the handle:
// a forward never consults the environment, so s5fxp_model_recurrence_kernel always reports what s5fxp_model_forward
// runs and two handles with different switches can be used side by side (include/s5fxp.h, "Environment").
struct ModelCfg {
    bool debug_sync = false;  // S5FXP_DEBUG_SYNC: synchronise + check after every stage of the fused forward
    bool no_bn_ext = false;   // S5FXP_NO_BN_EXT: four full BatchNorm reductions instead of the per-channel extremes
    bool no_pair = false;     // S5FXP_NO_PAIR: never the pair recurrence kernel
    bool pair_global = false; // S5FXP_PAIR_GLOBAL: pair kernel fed from an int32 K stream in global memory (no helper wave)
    bool no_pk16 = false;     // S5FXP_NO_PK16: unpacked epilogues in the gate kernel
    bool no_compact = false;  // S5FXP_NO_COMPACT: never run a layer on its live states only (s5fxp_fast.hpp FastLayer)
    bool no_live_lanes = false; // S5FXP_NO_LIVE_LANES: the recurrence streams of a compacted layer keep their padding slots
    // S5FXP_GATE_BN: where the gate kernel takes the SSM input u = BatchNorm(layer input) from.  Unset: the 32-frame kernel rebuilds
    // it in its tile staging (k_cgate_p<.., UREC>); =0: it is read from memory and the B projection stores it (the kernels before
    // UREC: the A/B partner); any other value: the first experiment, 64-frame tiles with the BatchNorm in the first epilogue
    // (k_cgate_p<.., GBN>; measured slower: DESIGN.md 4a).  =2 leaves the gate kernel at its default and takes the same row chain
    // out of the B projection instead: its phase A keeps bn16_x4 on every layer (the kernels before k_bproj_p<.., ROW>: the A/B
    // partner of that change.  A value of this switch, not a name of its own: both select where bn16_row8 runs)
    bool gate_bn = false, no_gate_urec = false, no_bproj_row = false;
    bool cgate_ft64 = false;   // S5FXP_CGATE_FT64: the packed-epilogue gate kernel on 64-frame tiles with six-wave workgroups (the form before
                               // the 32-frame / three-wave one became the default at dim_scale 0.5)
    int64_t cap_cgate32 = 1280; // S5FXP_WGS_CGATE32: workgroups per launch of the 32-frame gate kernel (5 per CU: all resident)
    bool no_dec_resid = false; // S5FXP_NO_DEC_RESID: the last layer's residual pass as its own launch (proj_p.hpp k_dec_p<.., RESID>)
    int pairl_blocks = 32;    // S5FXP_PAIRL_BLOCKS=16: 16 time blocks per LDS buffer of the LDS-fed pair kernel
    size_t plane_skew = 0;    // S5FXP_PLANE_SKEW=<bytes, multiple of 256>: extra distance between the workspace's planes (experiments)
    int64_t cap_enc = 512, cap_dec = 512, cap_cgate = 512, cap_bproj = 1024, cap_resid = 512; // S5FXP_WGS_ENC|DEC|CGATE|BPROJ|RESID: workgroups per launch
    static ModelCfg from_env()
    {
        ModelCfg c;
        auto on = [](const char *n) { return std::getenv(n) != nullptr; };
        auto cap = [](const char *n, int64_t dflt) {
            const char *e = std::getenv(n);
            const int v = e ? std::atoi(e) : 0;
            return (int64_t)(v > 0 ? v : dflt);
        };
        c.debug_sync = on("S5FXP_DEBUG_SYNC"); c.no_bn_ext = on("S5FXP_NO_BN_EXT"); c.no_pair = on("S5FXP_NO_PAIR");
        c.pair_global = on("S5FXP_PAIR_GLOBAL"); c.no_pk16 = on("S5FXP_NO_PK16"); c.no_compact = on("S5FXP_NO_COMPACT"); c.no_dec_resid = on("S5FXP_NO_DEC_RESID"); c.no_live_lanes = on("S5FXP_NO_LIVE_LANES"); c.cgate_ft64 = on("S5FXP_CGATE_FT64"); c.cap_cgate32 = cap("S5FXP_WGS_CGATE32", c.cap_cgate32);
        {
            const char *e = std::getenv("S5FXP_GATE_BN");
            c.no_gate_urec = e && std::strcmp(e, "0") == 0; c.no_bproj_row = e && std::strcmp(e, "2") == 0;
            c.gate_bn = e && !c.no_gate_urec && !c.no_bproj_row;
        }
        { const char *e = std::getenv("S5FXP_PAIRL_BLOCKS"); c.pairl_blocks = e && std::atoi(e) == 16 ? 16 : 32; }
        { const char *e = std::getenv("S5FXP_PLANE_SKEW"); c.plane_skew = e ? ((size_t)std::atoll(e) & ~(size_t)255) : 0; }
        c.cap_enc = cap("S5FXP_WGS_ENC", c.cap_enc); c.cap_dec = cap("S5FXP_WGS_DEC", c.cap_dec);
        c.cap_cgate = cap("S5FXP_WGS_CGATE", c.cap_cgate); c.cap_bproj = cap("S5FXP_WGS_BPROJ", c.cap_bproj);
        c.cap_resid = cap("S5FXP_WGS_RESID", c.cap_resid);
        return c;
    }
};

struct s5fxp_model {
    int n_layers = 0, d_in = 0, H = 0, P = 0, d_out = 0;
    DenseDev enc, dec;
    std::vector<LayerDev> layers;
    int flags = 0;
    ModelCfg cfg;
    FastModel *fast = nullptr; // owned
    s5fxp_model() = default;
    s5fxp_model(const s5fxp_model &) = delete;
    s5fxp_model &operator=(const s5fxp_model &) = delete;
    ~s5fxp_model(); // behind s5fxp_fast.hpp, where FastModel is complete
};

namespace {

struct Packer {
    size_t off = 0;
    char *host = nullptr; // nullptr: size pass
    char *dev = nullptr;  // nullptr: size pass, the addresses handed out are null
    const char *addr() const { return dev ? dev + off : nullptr; }
    const int32_t *put(const int32_t *src, size_t n)
    {
        const size_t bytes = n * sizeof(int32_t);
        const int32_t *d = reinterpret_cast<const int32_t *>(addr());
        if (host) std::memcpy(host + off, src, bytes);
        off = (off + bytes + 255) & ~(size_t)255;
        return d;
    }
};

bool dense_ok(const s5fxp_dense_desc &d) { return d.weight && d.bias && d.K > 0 && d.M > 0; }

void pack_dense(Packer &p, const s5fxp_dense_desc &d, DenseDev &o, bool allow24)
{
    o.K = d.K; o.M = d.M;
    o.w = p.put(d.weight, (size_t)d.K * d.M);
    o.bias = p.put(d.bias, (size_t)d.M);
    o.w_exp = d.w_exp; o.b_bits = d.b_bits; o.b_exp = d.b_exp; o.inp_bits = d.inp_bits; o.inp_exp = d.inp_exp;
    o.out_bits = d.out_bits; o.out_exp = d.out_exp;
    o.x24 = allow24 && fits24(d.weight, (size_t)d.K * d.M);
}

// Exactness bounds of the fast recurrence kernels (scan_quad.hpp) over the states idx[0..n) of a layer that runs on P_slots
// state slots (all P states, or the live ones of a compacted layer: a dead state's coefficients never meet a non-zero state).
struct ScanBounds {
    bool quad_ok = false, pair_ok = false;
    int32_t quad_xmax = 0, pair_xmax = 0;
};
ScanBounds scan_bounds(const s5fxp_ssm_desc &ssm, const int *idx, int n, int P_slots, bool allow24)
{
    ScanBounds o;
    // scaled coefficients c = A * 2^(16-e) must fit 24 signed bits; |c*x| + 2^16 < 2^31 bounds the state
    const int sre = 16 - ssm.A_re_exp, sim = 16 - ssm.A_im_exp;
    int64_t cmax = 1;
    for (int j = 0; j < n; ++j) {
        const int q = idx[j];
        const int64_t ar = std::llabs((long long)ssm.A_re[q]), ai = std::llabs((long long)ssm.A_im[q]);
        const int smax = sre > sim ? sre : sim;
        if (smax >= 0 && smax < 24) {
            cmax = std::max(cmax, ar << smax);
            cmax = std::max(cmax, ai << smax);
        }
    }
    o.quad_ok = allow24 && (P_slots % 16 == 0) && sre >= 0 && sim >= 0 && sre < 16 && sim < 16 && cmax < (1 << 23);
    o.quad_xmax = (int32_t)std::min<int64_t>(((int64_t(1) << 31) - 1 - 65536) / cmax, (1 << 23) - 1);
    // pair kernel: Bu is folded into the addend of the own product (always an Ai product), so
    //   |Ai| * 2^(16-e) * |x| + 2^16 * (bmax + 1) <= 2^31 - 1   and   |Ar| * 2^(16-e) * |x| <= 2^31 - 1
    // with bmax = the largest |Bu| after the shift to the state exponent (static: its bits minus the shift)
    const int sh_re = ssm.Bu_re_exp - ssm.x_re_exp, sh_im = ssm.Bu_im_exp - ssm.x_im_exp;
    const int bb_re = ssm.Bu_re_bits - sh_re, bb_im = ssm.Bu_im_bits - sh_im; // bits of the shifted Bu
    if (o.quad_ok && P_slots % 32 == 0 && bb_re >= 1 && bb_re <= 16 && bb_im >= 1 && bb_im <= 16) {
        const int64_t lim = (int64_t(1) << 31) - 1;
        int64_t xm = 32766;
        for (int j = 0; j < n; ++j) {
            const int q = idx[j];
            const int64_t ar = std::llabs((long long)ssm.A_re[q]), ai = std::llabs((long long)ssm.A_im[q]);
            const int64_t room_re = lim - 65536 * ((int64_t(1) << (bb_re - 1)) + 1), room_im = lim - 65536 * ((int64_t(1) << (bb_im - 1)) + 1);
            if (ai) xm = std::min({xm, room_re / (ai << sre), room_im / (ai << sim)});
            if (ar) xm = std::min({xm, lim / (ar << sre), lim / (ar << sim)});
        }
        o.pair_xmax = (int32_t)xm;
        o.pair_ok = xm >= 16384; // below that the quad kernel (bound 32767) is the better optimistic choice
    }
    return o;
}

void pack_layer(Packer &p, const s5fxp_layer_desc &l, LayerDev &o, bool allow24)
{
    const int H = l.ssm.H, P = l.ssm.P;
    o.nd = l.norm;
    o.mm = p.put(l.norm.minus_mean, H);
    o.isv = p.put(l.norm.invsq_var, H);
    o.scale = l.norm.scale ? p.put(l.norm.scale, H) : nullptr;
    o.nbias = l.norm.bias ? p.put(l.norm.bias, H) : nullptr;
    o.sd = l.ssm;
    o.a_re = p.put(l.ssm.A_re, P);
    o.a_im = p.put(l.ssm.A_im, P);
    std::vector<int32_t> tmp((size_t)H * 2 * P);
    for (int h = 0; h < H; ++h)
        for (int q = 0; q < P; ++q) {
            tmp[(size_t)h * 2 * P + q] = l.ssm.B_re[(size_t)q * H + h];
            tmp[(size_t)h * 2 * P + P + q] = l.ssm.B_im[(size_t)q * H + h];
        }
    o.bcat = p.put(tmp.data(), tmp.size());
    o.b24 = allow24 && fits24(tmp.data(), tmp.size());
    std::vector<int32_t> t2((size_t)P * H), t3((size_t)P * H);
    for (int h = 0; h < H; ++h)
        for (int q = 0; q < P; ++q) {
            t2[(size_t)q * H + h] = l.ssm.C_re[(size_t)h * P + q];
            t3[(size_t)q * H + h] = l.ssm.C_im[(size_t)h * P + q];
        }
    o.c_re_t = p.put(t2.data(), t2.size());
    o.c_im_t = p.put(t3.data(), t3.size());
    o.c24 = allow24 && fits24(t2.data(), t2.size()) && fits24(t3.data(), t3.size());
    o.D = p.put(l.ssm.D, H);
    {
        std::vector<int> all(P);
        for (int q = 0; q < P; ++q) all[q] = q;
        const ScanBounds sb = scan_bounds(l.ssm, all.data(), P, P, allow24);
        o.quad_ok = sb.quad_ok; o.quad_xmax = sb.quad_xmax; o.pair_ok = sb.pair_ok; o.pair_xmax = sb.pair_xmax;
    }
    pack_dense(p, l.out2, o.out2, allow24);
    o.l_bits = l.l_bits; o.l_exp = l.l_exp; o.r_bits = l.r_bits; o.r_exp = l.r_exp; o.res_bits = l.res_bits;
    o.res_exp = l.res_exp; o.sig_x = l.sig_x_exp; o.sig_y = l.sig_y_exp;
    std::memcpy(o.lut, l.lut, sizeof(o.lut));
}

int validate(const s5fxp_model_desc *d)
{
    if (!d || d->n_layers < 0 || (d->n_layers > 0 && !d->layers) || !dense_ok(d->encoder) || !dense_ok(d->decoder))
        return S5FXP_EBADARG;
    const int H = d->encoder.M;
    if (d->decoder.K != H) return S5FXP_EBADARG;
    if (mw_for(H) > MW_LIMIT_C || mw_for(d->decoder.M) > MW_LIMIT) return S5FXP_EUNSUPPORTED;
    if (8 + 8 * d->n_layers > S5FXP_STATUS_WORDS) return S5FXP_EUNSUPPORTED;
    for (int i = 0; i < d->n_layers; ++i) {
        const s5fxp_layer_desc &l = d->layers[i];
        const s5fxp_ssm_desc &s = l.ssm;
        if (s.H != H || s.P < 1 || !s.A_re || !s.A_im || !s.B_re || !s.B_im || !s.C_re || !s.C_im || !s.D ||
            !l.norm.minus_mean || !l.norm.invsq_var || !dense_ok(l.out2) || l.out2.K != H || l.out2.M != H)
            return S5FXP_EBADARG;
        if (mw_for(2 * s.P) > MW_LIMIT) return S5FXP_EUNSUPPORTED;
        // static shifts: a negative one is a ValueError (fxp_mul) or an undefined XLA shift (fxp_matmul)
        const int sh[] = {s.u_exp + s.B_re_exp - s.Bu_re_exp, s.u_exp + s.B_im_exp - s.Bu_im_exp,
                          s.x_re_exp + s.C_re_exp - s.y_exp,  s.x_im_exp + s.C_im_exp - s.y_exp,
                          s.D_exp + s.u_exp - s.y_exp,        l.l_exp + l.r_exp - l.res_exp,
                          s.A_re_exp,                         s.A_im_exp};
        for (int v : sh)
            if (!shift_ok(v)) return S5FXP_ENEGSHIFT;
        const int d1 = s.Bu_re_exp - s.x_re_exp, d2 = s.Bu_im_exp - s.x_im_exp;
        if (!shift_ok(d1 < 0 ? -d1 : d1) || !shift_ok(d2 < 0 ? -d2 : d2)) return S5FXP_ENEGSHIFT;
        if (l.sig_x_exp < 0 || l.sig_x_exp > 15 || l.sig_y_exp < 1 || l.sig_y_exp > 30) return S5FXP_EUNSUPPORTED;
    }
    return S5FXP_OK;
}

// time blocks (4 steps each) the recurrence kernels keep in flight: streams are padded to a multiple of it and followed by
// that many blocks of readable padding (the pair kernel's ring, the deepest, prefetches that far beyond its run)
constexpr int SCAN_DEPTH = S5_SCANP_ASM_DEPTH;
static_assert(S5_SCANP_ASM_DEPTH % S5_SCAN_ASM_DEPTH == 0, "one padding rule for all recurrence kernels");

// the recurrence kernels address one (sequence, state group) run of a stream through a 32-bit buffer extent
inline bool stream_extent_ok(const s5fxp_model *m, int L)
{
    return (((int64_t)L + 3) / 4 + 2 * SCAN_DEPTH) * (m->P ? m->P : 1) * 32 < 0xffffffffll;
}

// BatchNorm arguments of layer l, whose input has hb_in bits and the (device) exponent he_in
BnArgs make_bn(const LayerDev &l, int hb_in, DynExp he_in, LayerDyn *d)
{
    const s5fxp_ssm_desc &s = l.sd;
    auto mx = [](int a, int b) { return a > b ? a : b; };
    BnArgs bn{};
    bn.mm = l.mm; bn.isv = l.isv; bn.scale = l.scale; bn.bias = l.nbias;
    bn.xb = hb_in; bn.xe = he_in;
    bn.mb = l.nd.mean_bits; bn.me = l.nd.mean_exp; bn.b1 = mx(hb_in, bn.mb);
    bn.ib = l.nd.invsq_var_bits; bn.ie = l.nd.invsq_var_exp; bn.b2 = mx(bn.b1, bn.ib);
    bn.sb = l.nd.scale_bits; bn.se = l.nd.scale_exp; bn.b3 = l.scale ? mx(bn.b2, bn.sb) : bn.b2;
    bn.bb = l.nd.bias_bits; bn.be = l.nd.bias_exp; bn.b4 = l.nbias ? mx(bn.b3, bn.bb) : bn.b3;
    bn.ub = s.u_bits; bn.ue = s.u_exp; bn.out_bits = bn.b4; bn.dyn = d;
    return bn;
}

// BatchNorm exponents by full reductions, one compute_best op after the other: reduce -> (cross-rank max) -> finalize.
// reduce(std::integral_constant<int, OP>) launches the reduce kernel of op 1..4 over the layer input (k_bn_reduce on the
// generic path's int32 planes, k_bn_reduce16 on the fused path's int16 ones).
template <class Reduce>
int bn_exponent_ops(Reduce reduce, const BnArgs &bn, LayerDyn *d, int32_t *status, int32_t *st_exps, const s5fxp_forward_opts *opts,
                    hipStream_t st)
{
    const s5fxp_allreduce_max_fn allreduce = opts ? opts->allreduce : nullptr;
    auto op = [&](auto k, int slot, int n) {
        reduce(k);
        if (allreduce && allreduce(opts->allreduce_ctx, reinterpret_cast<float *>(d->mx + slot), n, (void *)st)) return false;
        hipLaunchKernelGGL(k_bn_finalize<decltype(k)::value>, dim3(1), dim3(64), 0, st, bn, d, status, st_exps);
        return true;
    };
    const bool ok = op(std::integral_constant<int, 1>{}, 0, 3) && op(std::integral_constant<int, 2>{}, 3, 1) &&
                    (!bn.scale || op(std::integral_constant<int, 3>{}, 4, 1)) && (!bn.bias || op(std::integral_constant<int, 4>{}, 5, 3));
    return ok ? S5FXP_OK : S5FXP_EHIP;
}

} // namespace

#include "s5fxp_fast.hpp"
#include "s5fxp_step.hpp"
#include "s5fxp_clip.hpp"

s5fxp_model::~s5fxp_model() { delete fast; }

namespace {

// m == nullptr: size pass (an upper bound: it includes the MFMA-path tensors whenever the model is eligible)
size_t pack_all(const s5fxp_model_desc *d, Packer &p, s5fxp_model *m, bool allow24)
{
    DenseDev tmp_e, tmp_d;
    pack_dense(p, d->encoder, m ? m->enc : tmp_e, allow24);
    for (int i = 0; i < d->n_layers; ++i) {
        LayerDev tmp;
        pack_layer(p, d->layers[i], m ? m->layers[i] : tmp, allow24);
    }
    pack_dense(p, d->decoder, m ? m->dec : tmp_d, allow24);
    if ((allow24 || !m) && fast_eligible(d)) {
        if (m) m->fast = new FastModel();
        pack_fast(p, d, m ? m->fast : nullptr);
        // appended last: the parameter block of s5fxp_model_step, built from the addresses handed out above
        StepParams sp;
        if (m) fill_step_params(m, sp);
        const void *dev = put_raw(p, &sp, sizeof(sp));
        if (m) m->fast->step = reinterpret_cast<const StepParams *>(dev);
    }
    return p.off;
}

} // namespace

extern "C" size_t s5fxp_model_blob_bytes(const s5fxp_model_desc *desc)
{
    if (validate(desc) != S5FXP_OK) return 0;
    Packer p;
    return pack_all(desc, p, nullptr, false);
}

extern "C" int s5fxp_model_create(const s5fxp_model_desc *desc, void *dev_blob, size_t blob_bytes, int flags,
                                  void *stream, s5fxp_model **out)
{
    if (!out || !dev_blob) return S5FXP_EBADARG;
    *out = nullptr;
    if (flags & S5FXP_MODEL_FORCE_CSR) return S5FXP_EUNSUPPORTED; // see include/s5fxp.h: op level only
    int rc = validate(desc);
    if (rc) return rc;
    const size_t need = s5fxp_model_blob_bytes(desc);
    if (blob_bytes < need) return S5FXP_EWORKSPACE;
    s5fxp_model *m = new (std::nothrow) s5fxp_model();
    if (!m) return S5FXP_EBADARG;
    m->n_layers = desc->n_layers;
    m->d_in = desc->encoder.K;
    m->H = desc->encoder.M;
    m->P = desc->n_layers ? desc->layers[0].ssm.P : 0;
    m->d_out = desc->decoder.M;
    m->flags = flags;
    m->cfg = ModelCfg::from_env();
    m->layers.resize(desc->n_layers);
    std::vector<char> host(need);
    Packer p;
    p.host = host.data();
    p.dev = reinterpret_cast<char *>(dev_blob);
    pack_all(desc, p, m, !(flags & S5FXP_MODEL_FORCE_GENERIC));
    // pageable-memory async copies are staged by the runtime before returning, so `host` may go
    rc = hip_rc(hipMemcpyAsync(dev_blob, host.data(), need, hipMemcpyHostToDevice, S(stream)));
    if (rc) {
        delete m;
        return rc;
    }
    rc = hip_rc(hipStreamSynchronize(S(stream))); // creation is not on the hot path
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return S5FXP_OK;
}

extern "C" void s5fxp_model_destroy(s5fxp_model *m) { delete m; }
extern "C" int s5fxp_model_out_exp(const s5fxp_model *m) { return m ? m->dec.out_exp : 0; }
extern "C" int s5fxp_model_out_bits(const s5fxp_model *m) { return m ? m->dec.out_bits : 0; }
/* 1 if the int8-MFMA path was packed for this model (it also needs L % 4 == 0 at run time) */
extern "C" int s5fxp_model_is_fast(const s5fxp_model *m) { return m && m->fast ? 1 : 0; }
extern "C" int s5fxp_model_recurrence_xmax(const s5fxp_model *m, int layer)
{
    const int k = s5fxp_model_recurrence_kernel(m, layer);
    if (k < 0) return -1;
    const LayerDev &l = m->layers[layer];
    // the fused path: a plain forward of a compactable layer runs on its live states, and their bounds apply
    const int32_t bound = m->fast ? plain_plan(m, layer).bound : l.quad_xmax;
    if (k >= 3) return bound;
    if (k == 2) return bound < 32766 ? bound : 32766;
    return l.quad_ok ? bound : 0;
}

extern "C" int s5fxp_model_recurrence_kernel(const s5fxp_model *m, int layer)
{
    if (!m || layer < 0 || layer >= m->n_layers) return -1;
    const LayerDev &l = m->layers[layer];
    if (!m->fast) return l.quad_ok && !(m->flags & S5FXP_MODEL_FORCE_GENERIC) ? 1 : 0;
    // the fused path: the plan of a plain forward (reported in status word [8 + 8*layer + 5])
    const int code = plain_plan(m, layer).rung.code;
    return code == RK_EXACT ? 1 : code; // no fast rung applies: a quad kernel all the same, the 32-bit chain
}

namespace {

struct WsLayout {
    size_t hA, hB, bq, xs, x1, z, dyn, total;
    int TB; // time blocks per sequence in the scan-native streams (padded to a multiple of SCAN_DEPTH)
};
WsLayout ws_layout(const s5fxp_model *m, int B, int L)
{
    WsLayout w{};
    w.TB = (int)time_blocks(L, SCAN_DEPTH);
    // the planes' sizes in 128 bits; a layout whose end does not fit a size_t has total == 0 and no meaningful offsets
    const wide_t nh_w = wide_al256((wide_t)B * L * m->H * 4);
    // + SCAN_DEPTH blocks of padding: the recurrence kernel's ring buffer reads ahead of the last block
    const wide_t ns_w = wide_al256(((wide_t)B * w.TB + SCAN_DEPTH) * (m->P ? m->P : 1) * 8 * 4);
    const size_t dyn_b = (size_t)wide_al256(sizeof(LayerDyn) * (size_t)(m->n_layers ? m->n_layers : 1));
    if (!fit_size(4 * nh_w + 2 * ns_w + dyn_b)) return w;
    const size_t nh = (size_t)nh_w, ns = (size_t)ns_w;
    size_t off = 0;
    w.hA = off; off += nh;
    w.hB = off; off += nh;
    w.bq = off; off += ns;
    w.xs = off; off += ns;
    w.x1 = off; off += nh;
    w.z = off; off += nh;
    w.dyn = off; off += dyn_b;
    w.total = off;
    return w;
}
} // namespace

extern "C" size_t s5fxp_workspace_bytes(const s5fxp_model *m, int B, int L)
{
    if (!m || B < 1 || L < 1) return 0;
    const size_t g = ws_layout(m, B, L).total;
    if (!g) return 0; // it does not fit a size_t
    if (!m->fast) return g;
    const size_t f = fast_ws(m, B, L).total;
    if (!f) return 0;
    return g > f ? g : f;
}

namespace {

// FxpSequenceLayer.forward (fxpmodel.py:1110-1161) x [first, last) on the generic int32 kernels: BatchNorm exponents
// (reduce -> cross-rank max -> finalize per compute_best op), B projection, recurrence, C projection (+ exact re-run),
// out2 / sigmoid / gate, residual.  h: the first layer's input (read only), hn / h: the ping-pong pair the outputs go to;
// on return h points at the last layer's output and (hb, he) are its configuration.
struct GenericRun {
    const s5fxp_model *m;
    int B, L;
    WsLayout w;
    char *ws;
    LayerDyn *dyn;
    int32_t *status;
    const s5fxp_layer_trace *traces; // indexed by layer - trace_base
    int trace_base;
    const s5fxp_forward_opts *opts;
    hipStream_t st;
    void *stream;

    const s5fxp_allreduce_max_fn allreduce = opts ? opts->allreduce : nullptr;
    void *const allreduce_ctx = opts ? opts->allreduce_ctx : nullptr;
    void **const scan_events = opts ? opts->scan_events : nullptr;
    const int32_t *const state_in = opts ? opts->state_in : nullptr;
    int32_t *const state_out = opts ? opts->state_out : nullptr;

    int layers(int first, int last, int32_t *&h, int32_t *&hn, int &hb, DynExp &he) const;
};

int GenericRun::layers(int first, int last, int32_t *&h, int32_t *&hn, int &hb, DynExp &he) const
{
    auto I = [&](size_t off) { return reinterpret_cast<int32_t *>(ws + off); };
    const int64_t N = (int64_t)B * L;
    const int H = m->H, P = m->P;
    const int64_t NH = N * H;
    const unsigned tiles = (unsigned)((N + TN - 1) / TN);
    int rc;
    for (int li = first; li < last; ++li) {
        const LayerDev &l = m->layers[li];
        const s5fxp_layer_trace *tr = traces ? &traces[li - trace_base] : nullptr;
        LayerDyn *d = dyn + li;
        int32_t *st_exps = status + 8 + 8 * li;
        const s5fxp_ssm_desc &s = l.sd;
        const BnArgs bn = make_bn(l, hb, he, d);

        // ---- BatchNorm exponents: reduce -> (cross-rank max) -> finalize, per compute_best op
        const unsigned rg = ew_grid(NH) > 2048 ? 2048 : ew_grid(NH);
        if ((rc = bn_exponent_ops([&](auto op) {
                 hipLaunchKernelGGL(k_bn_reduce<decltype(op)::value>, dim3(rg), dim3(256), 0, st, bn, h, NH, H, d);
             }, bn, d, status, st_exps, opts, st)))
            return rc;

        // ---- B projection (fused BatchNorm apply + change_cfg), writes the scan-native stream
        const int sh_re = s.Bu_re_exp - s.x_re_exp, sh_im = s.Bu_im_exp - s.x_im_exp;
        {
            BprojArgs a{};
            a.bn = bn; a.x = h; a.w = l.bcat; a.bq = I(w.bq);
            a.tr_bu_re = tr ? tr->Bu_re : nullptr; a.tr_bu_im = tr ? tr->Bu_im : nullptr;
            a.tr_pre_s5 = tr ? tr->pre_s5 : nullptr; a.tr_u = tr ? tr->u : nullptr;
            a.N = N; a.L = L; a.TB = w.TB; a.H = H; a.P = P; a.mw = mw_for(2 * P);
            a.rs_re = s.u_exp + s.B_re_exp - s.Bu_re_exp; a.rs_im = s.u_exp + s.B_im_exp - s.Bu_im_exp;
            a.bre_bits = s.Bu_re_bits; a.bim_bits = s.Bu_im_bits; a.sh_re = sh_re; a.sh_im = sh_im;
            if (l.b24 && s.u_bits <= 24 && bn.out_bits <= 24) S5_DISPATCH_MW(a.mw, true, k_bproj, tiles, st, a);
            else S5_DISPATCH_MW(a.mw, false, k_bproj, tiles, st, a);
        }
        // ---- recurrence.  Fast: quad kernel (3 dependent VALU ops / step), exact while |x| <= xmax; the C
        //      projection checks that bound on every state, the quad kernel on the carry it starts from, and if
        //      either fails, the exact 32-bit kernels re-run.
        ScanArgs sl{};
        sl.bu_re = I(w.bq); sl.a_re = l.a_re; sl.a_im = l.a_im; sl.out_re = I(w.xs);
        sl.B = B; sl.L = L; sl.P = P; sl.TB = w.TB; sl.ea_re = s.A_re_exp; sl.ea_im = s.A_im_exp;
        const size_t plane = (size_t)B * P;
        sl.x0_re = state_in ? state_in + (size_t)li * 2 * plane : nullptr;
        sl.x0_im = state_in ? sl.x0_re + plane : nullptr;
        const unsigned lane_grid = (unsigned)(((int64_t)B * P + 63) / 64);
        int32_t xmax = (1 << 23) - 1; // the 24-bit C projection's own limit
        const bool quad = l.quad_ok && !(m->flags & S5FXP_MODEL_FORCE_GENERIC);
        if (scan_events && scan_events[2 * li] && (rc = hip_rc(hipEventRecord((hipEvent_t)scan_events[2 * li], st)))) return rc;
        if (quad) {
            ScanQuadArgs q{};
            q.bq = I(w.bq); q.xs = I(w.xs); q.a_re = l.a_re; q.a_im = l.a_im; q.B = B; q.TB = w.TB; q.P = P;
            q.ea_re = s.A_re_exp; q.ea_im = s.A_im_exp; q.x0_re = sl.x0_re; q.x0_im = sl.x0_im;
            // the carry is no stored state: the quad kernel checks it against its bound itself (scan_quad.hpp CarryCheck)
            if (state_in) q.cc = CarryCheck{l.quad_xmax, ST_WIDE_STATE, &d->redo, status};
            hipLaunchKernelGGL(k_scan_quad_asm, dim3((unsigned)((int64_t)B * P / 16)), dim3(64), 0, st, q, GroupOff{});
            xmax = l.quad_xmax;
        } else {
            sl.run_if = nullptr;
            hipLaunchKernelGGL(k_scan_lane_native, dim3(lane_grid), dim3(64), 0, st, sl);
        }
        if (scan_events && scan_events[2 * li + 1] && (rc = hip_rc(hipEventRecord((hipEvent_t)scan_events[2 * li + 1], st)))) return rc;
        // ---- C projection + D*u + ReLU: pass 0 (24-bit multiplies, range check), then the exact re-run
        {
            CprojArgs a{};
            a.bn = bn; a.x = h; a.xs = I(w.xs); a.w_re = l.c_re_t; a.w_im = l.c_im_t; a.D = l.D;
            a.x1 = I(w.x1); a.tr_ys = tr ? tr->ys : nullptr; a.N = N; a.L = L; a.TB = w.TB; a.H = H; a.P = P;
            a.mw = mw_for(H);
            a.rs_re = s.x_re_exp + s.C_re_exp - s.y_exp; a.rs_im = s.x_im_exp + s.C_im_exp - s.y_exp;
            a.rs_d = s.D_exp + s.u_exp - s.y_exp; a.y_bits = s.y_bits; a.xmax = xmax; a.dynw = d; a.status = status;
            const bool c24 = l.c24 && !(m->flags & S5FXP_MODEL_FORCE_GENERIC);
            if (c24) S5_DISPATCH_MW_C(a.mw, true, 0, int32_t, tiles, st, a);
            else hipMemsetAsync(&d->redo, 0xff, 4, st); // no 24-bit variant: the exact pass does all the work
            if (quad) {
                sl.run_if = &d->redo;
                hipLaunchKernelGGL(k_scan_lane_native, dim3(lane_grid), dim3(64), 0, st, sl);
            }
            S5_DISPATCH_MW_C(a.mw, false, 1, int32_t, tiles, st, a);
            if (state_out) // the raw states are still in the stream (either pass): carry out = state after frame L-1
                hipLaunchKernelGGL(k_state_out, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, (const void *)I(w.xs), 0,
                                   (const int32_t *)nullptr, B, L, P, w.TB, state_out + (size_t)li * 2 * plane,
                                   state_out + (size_t)li * 2 * plane + plane, GroupOff{});
            if (tr && (tr->xs_re || tr->xs_im))
                hipLaunchKernelGGL(k_unpack_native, dim3(ew_grid(N * P)), dim3(256), 0, st, (const int32_t *)I(w.xs),
                                   tr->xs_re, tr->xs_im, B, L, P, w.TB);
        }
        // ---- out2 + sigmoid + gate + residual maxima
        {
            const DenseDev &o = l.out2;
            GateArgs a{};
            a.x1 = I(w.x1); a.w = o.w; a.bias = o.bias; a.skip = h; a.z = I(w.z);
            a.tr_out2 = tr ? tr->out2 : nullptr; a.tr_sig = tr ? tr->out2_sigmoid : nullptr;
            a.N = N; a.H = H; a.mw = mw_for(H); a.y_bits = s.y_bits; a.y_exp = s.y_exp;
            a.inp_bits = o.inp_bits; a.inp_exp = o.inp_exp; a.w_exp = o.w_exp; a.b_bits = o.b_bits; a.b_exp = o.b_exp;
            a.out_bits = o.out_bits; a.out_exp = o.out_exp; a.sig_x = l.sig_x; a.sig_y = l.sig_y;
            std::memcpy(a.lut, l.lut, sizeof(a.lut));
            a.l_bits = l.l_bits; a.l_exp = l.l_exp; a.r_bits = l.r_bits; a.r_exp = l.r_exp; a.res_bits = l.res_bits;
            a.res_exp = l.res_exp; a.rs_gate = l.l_exp + l.r_exp - l.res_exp;
            a.skip_bits = hb; a.skip_e = he; a.dynw = d; a.status = status;
            // exponent sanity that the reference would hit as a ValueError / undefined shift
            const bool conv = s.y_bits > o.inp_bits || s.y_exp > o.inp_exp;
            if (!shift_ok((conv ? o.inp_exp : s.y_exp) + o.w_exp - o.out_exp)) return S5FXP_ENEGSHIFT;
            if (o.x24 && s.y_bits <= 24) S5_DISPATCH_MW(a.mw, true, k_out2gate, tiles, st, a);
            else S5_DISPATCH_MW(a.mw, false, k_out2gate, tiles, st, a);
            if (tr && tr->post_GLU) hipMemcpyAsync(tr->post_GLU, a.z, (size_t)NH * 4, hipMemcpyDeviceToDevice, st);
        }
        if (allreduce && allreduce(allreduce_ctx, reinterpret_cast<float *>(d->mx + 8), 3, stream)) return S5FXP_EHIP;
        hipLaunchKernelGGL(k_res_finalize, dim3(1), dim3(64), 0, st, d, l.res_exp, he, l.res_bits, status, st_exps, 8);
        hipLaunchKernelGGL(k_resid, dim3(ew_grid(NH)), dim3(256), 0, st, (const int32_t *)I(w.z), (const int32_t *)h, hn,
                           tr ? tr->residadd : nullptr, NH, l.res_bits, hb, (const LayerDyn *)d);
        int32_t *sw = h; h = hn; hn = sw;
        hb = l.res_bits;
        he = DynExp{0, &d->res.eo};
    }

    return S5FXP_OK;
}

// the status words of a generic forward over layers [first, last) start from zero except the path and, per layer, the
// recurrence kernel, the state slots and the slots the streams hold
void clear_status_generic(const s5fxp_model *m, int first, int last, int32_t *status, hipStream_t st)
{
    StatusInit si{};
    si.path = S5FXP_PATH_GENERIC;
    for (int li = first; li < last; ++li) {
        si.rk[li] = m->layers[li].quad_ok && !(m->flags & S5FXP_MODEL_FORCE_GENERIC) ? 1 : 0;
        si.slots[li] = m->P;
        si.stream[li] = m->P;
    }
    hipLaunchKernelGGL(k_clear2, dim3(1), dim3(256), 0, st, status, (int)S5FXP_STATUS_WORDS, (int32_t *)nullptr, 0, si, m->n_layers, GroupOff{});
}

// encoder and decoder of the generic forward: one frame-tiled k_dense each
void launch_dense(const DenseDev &e, const int32_t *x, int xb, DynExp xe, int32_t *y, int64_t N, bool first, int32_t *status, hipStream_t st)
{
    DenseArgs a{};
    a.x = x; a.w = e.w; a.bias = e.bias; a.y = y; a.N = N; a.K = e.K; a.M = e.M; a.mw = mw_for(e.M);
    a.xb = xb; a.xe = xe; a.inp_bits = e.inp_bits; a.inp_exp = e.inp_exp; a.check_inp = 1;
    a.w_exp = e.w_exp; a.b_bits = e.b_bits; a.b_exp = e.b_exp; a.out_bits = e.out_bits; a.out_exp = e.out_exp;
    a.relu = first; a.check24 = first; a.status = status; // the encoder: ReLU, and the 24-bit check of the model's input
    const unsigned tiles = (unsigned)((N + TN - 1) / TN);
    if (e.x24 && (first || xb <= 24)) S5_DISPATCH_MW(a.mw, true, k_dense, tiles, st, a);
    else S5_DISPATCH_MW(a.mw, false, k_dense, tiles, st, a);
}

// The forward on the generic int32 kernels (arguments checked by forward_entry): encoder, the layers, decoder
int forward_generic(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int B, int L, int32_t *y, void *workspace,
                    int32_t *status, const s5fxp_layer_trace *traces, const s5fxp_forward_opts *opts, void *stream)
{
    const WsLayout w = ws_layout(m, B, L);
    hipStream_t st = S(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    LayerDyn *dyn = reinterpret_cast<LayerDyn *>(ws + w.dyn);
    const int64_t N = (int64_t)B * L;
    int rc;
    clear_status_generic(m, 0, m->n_layers, status, st);
    if ((rc = hip_rc(hipMemsetAsync(dyn, 0, sizeof(LayerDyn) * (size_t)(m->n_layers ? m->n_layers : 1), st)))) return rc;

    // ---- encoder + ReLU (fxpmodel.py:1263-1266)
    int32_t *h = reinterpret_cast<int32_t *>(ws + w.hA), *hn = reinterpret_cast<int32_t *>(ws + w.hB);
    const DenseDev &e = m->enc;
    const bool conv = x_bits > e.inp_bits || x_exp > e.inp_exp;
    if (!shift_ok((conv ? e.inp_exp : x_exp) + e.w_exp - e.out_exp)) return S5FXP_ENEGSHIFT;
    launch_dense(e, x, x_bits, DynExp{x_exp, nullptr}, h, N, true, status, st);
    int hb = e.out_bits;
    DynExp he{e.out_exp, nullptr};

    const GenericRun g{m, B, L, w, ws, dyn, status, traces, 0, opts, st, stream};
    if ((rc = g.layers(0, m->n_layers, h, hn, hb, he))) return rc;

    // ---- decoder (fxpmodel.py:1437): its input exponent is the last residual's
    launch_dense(m->dec, h, hb, he, y, N, false, status, st);
    return launch_rc();
}

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// The one forward entry behind s5fxp_model_forward (io = IO_I32: int32 x and y), s5fxp_model_forward_f32 (IO_F32: float32) and
// s5fxp_model_forward_i16 (IO_I16: int16; the constants of proj_p.hpp).  A fused model converts inside its encoder and decoder
// kernels (k_enc_pf / k_dec_pf, k_enc_ps / k_dec_ps) on the int forward's workspace; a generic one stages int32 copies of x and y
// behind the int forward's workspace and converts before and after it: k_from_fp / k_to_float (the float-in, float-out forward
// of fxprun.py:63-88) or k_widen_i16 / k_narrow_i16.  The checks come in this order: arguments, what the model supports, the
// workspace, the stream extent.
// pinned: the _at entries (stated exponents).  Their own checks follow the namesake's, all before the device is
// touched: a null exps, traces, s5fxp_model_exps_check (which refuses a generic model).  A fused model that takes the
// four-reduction route unpinned (fast_bn_ext false) runs the same pinned plan on the two-plane residual (k_resid16).
int forward_entry(const s5fxp_model *m, int io, const void *x, int x_bits, int x_exp, int B, int L, void *y, void *workspace,
                  size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces, const s5fxp_forward_opts *opts,
                  void *stream, bool pinned = false, const int32_t *exps = nullptr)
{
    if (!m || !x || !y || !workspace || !status || B < 1 || L < 1 || x_bits < 1 || x_bits > (io == IO_I16 ? 16 : 32) ||
        (io == IO_F32 && !shift_ok(x_exp)))
        return S5FXP_EBADARG;
    if (io == IO_F32 && !shift_ok(m->dec.out_exp)) return S5FXP_EUNSUPPORTED; // the range s5fxp_to_float takes
    if (io == IO_I16 && m->dec.out_bits > 16) return S5FXP_EUNSUPPORTED;       // the narrowing of y would lose bits
    const int G = opts && opts->groups > 1 ? opts->groups : 1;
    const size_t ws_one = io == IO_I32   ? s5fxp_workspace_bytes(m, B, L)
                          : io == IO_F32 ? s5fxp_workspace_bytes_f32(m, B, L)
                                         : s5fxp_workspace_bytes_i16(m, B, L);
    // no workspace can hold it: one forward's size does not fit a size_t (the query's 0), or the G-fold of it does not
    if (!ws_one || ws_one > SIZE_MAX / (size_t)G) return S5FXP_EWORKSPACE;
    if (workspace_bytes < (size_t)G * ws_one) return S5FXP_EWORKSPACE;
    if (pinned) {
        if (!stream_extent_ok(m, L) || !exps) return S5FXP_EBADARG;
        if (traces) return S5FXP_EUNSUPPORTED;
        if (const int rc = exps_check(m, exps)) return rc;
    }
    const size_t N = (size_t)B * L;
    if (G > 1) {
        // Grouped call: G independent reference batches of B sequences each.  The fused kernels take them in ONE set of
        // launches (gridDim.y = G) when nothing couples the groups on the host; otherwise one (fused or generic) forward per group.
        // (a pinned forward takes its groups one by one: its kernels read LayerDyn from memory, a mode no grouped launch has run in)
        if (m->fast && !traces && !opts->allreduce && fast_bn_ext(m) && stream_extent_ok(m, L) && !pinned)
            return forward_fast(m, x, x_bits, x_exp, B, L, y, workspace, status, traces, opts, S(stream), G, ws_one, io);
        const size_t esz = io == IO_I16 ? 2 : 4, plane = (size_t)m->n_layers * 2 * B * (m->P ? m->P : 1);
        for (int g = 0; g < G; ++g) {
            s5fxp_forward_opts o = *opts;
            o.groups = 1;
            if (o.state_in) o.state_in += g * plane;
            if (o.state_out) o.state_out += g * plane;
            const int rc = forward_entry(m, io, static_cast<const char *>(x) + g * N * m->d_in * esz, x_bits, x_exp, B, L,
                                         static_cast<char *>(y) + g * N * m->d_out * esz, static_cast<char *>(workspace) + g * ws_one,
                                         ws_one, status + (size_t)g * S5FXP_STATUS_WORDS,
                                         traces ? traces + (size_t)g * m->n_layers : nullptr, &o, stream, pinned, exps);
            if (rc) return rc;
        }
        return S5FXP_OK;
    }
    if (!stream_extent_ok(m, L)) return S5FXP_EBADARG;
    if (m->fast) return forward_fast(m, x, x_bits, x_exp, B, L, y, workspace, status, traces, opts, S(stream), 1, 0, io, pinned ? exps : nullptr);
    if (io == IO_I32)
        return forward_generic(m, static_cast<const int32_t *>(x), x_bits, x_exp, B, L, static_cast<int32_t *>(y), workspace, status,
                               traces, opts, stream);
    // generic, float32 or int16: convert, the int forward, convert back, on int32 copies staged behind the int forward's workspace
    int32_t *xi = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + s5fxp_workspace_bytes(m, B, L));
    int32_t *yi = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(xi) + al256(N * m->d_in * 4));
    const int64_t nx = (int64_t)N * m->d_in, ny = (int64_t)N * m->d_out;
    int rc;
    if (io == IO_F32) {
        if ((rc = s5fxp_from_fp(static_cast<const float *>(x), xi, nx, x_bits, x_exp, S5FXP_FLOOR, stream))) return rc;
    } else {
        hipLaunchKernelGGL(k_widen_i16, dim3(ew_grid(nx)), dim3(256), 0, S(stream), static_cast<const int16_t *>(x), xi, nx);
    }
    if ((rc = forward_generic(m, xi, x_bits, x_exp, B, L, yi, workspace, status, traces, opts, stream))) return rc;
    if (io == IO_F32) return s5fxp_to_float(yi, static_cast<float *>(y), ny, m->dec.out_exp, stream);
    hipLaunchKernelGGL(k_narrow_i16, dim3(ew_grid(ny)), dim3(256), 0, S(stream), (const int32_t *)yi, static_cast<int16_t *>(y), ny);
    return launch_rc();
}

} // namespace

extern "C" int s5fxp_model_forward(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int B, int L,
                                   int32_t *y, void *workspace, size_t workspace_bytes, int32_t *status,
                                   const s5fxp_layer_trace *traces, const s5fxp_forward_opts *opts, void *stream)
{
    return forward_entry(m, IO_I32, x, x_bits, x_exp, B, L, y, workspace, workspace_bytes, status, traces, opts, stream);
}

// A generic model's float32 / int16 forward stages 4 bytes per element of both tensors behind the int forward's workspace; a
// fused one needs no more than an int forward (forward_entry)
extern "C" size_t s5fxp_workspace_bytes_f32(const s5fxp_model *m, int B, int L)
{
    const size_t ws = s5fxp_workspace_bytes(m, B, L);
    if (!ws || m->fast) return ws;
    const wide_t N = (wide_t)B * L;
    return fit_size(ws + wide_al256(N * m->d_in * 4) + wide_al256(N * m->d_out * 4));
}

extern "C" int s5fxp_model_forward_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int B, int L, float *y,
                                       void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                                       const s5fxp_forward_opts *opts, void *stream)
{
    return forward_entry(m, IO_F32, x, x_bits, x_exp, B, L, y, workspace, workspace_bytes, status, traces, opts, stream);
}

extern "C" size_t s5fxp_workspace_bytes_i16(const s5fxp_model *m, int B, int L)
{
    return s5fxp_workspace_bytes_f32(m, B, L); // the same staging: 4 bytes per element of both tensors on the generic path
}

extern "C" int s5fxp_model_forward_i16(const s5fxp_model *m, const int16_t *x, int x_bits, int x_exp, int B, int L, int16_t *y,
                                       void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                                       const s5fxp_forward_opts *opts, void *stream)
{
    return forward_entry(m, IO_I16, x, x_bits, x_exp, B, L, y, workspace, workspace_bytes, status, traces, opts, stream);
}

// The three forwards at stated exponents (include/s5fxp.h)
extern "C" int s5fxp_model_forward_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int B, int L, int32_t *y,
                                      void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                                      const s5fxp_forward_opts *opts, const int32_t *exps, void *stream)
{
    return forward_entry(m, IO_I32, x, x_bits, x_exp, B, L, y, workspace, workspace_bytes, status, traces, opts, stream, true, exps);
}

extern "C" int s5fxp_model_forward_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int B, int L, float *y,
                                          void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                                          const s5fxp_forward_opts *opts, const int32_t *exps, void *stream)
{
    return forward_entry(m, IO_F32, x, x_bits, x_exp, B, L, y, workspace, workspace_bytes, status, traces, opts, stream, true, exps);
}

extern "C" int s5fxp_model_forward_at_i16(const s5fxp_model *m, const int16_t *x, int x_bits, int x_exp, int B, int L, int16_t *y,
                                          void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                                          const s5fxp_forward_opts *opts, const int32_t *exps, void *stream)
{
    return forward_entry(m, IO_I16, x, x_bits, x_exp, B, L, y, workspace, workspace_bytes, status, traces, opts, stream, true, exps);
}

// FxpSequenceLayer.forward for ONE layer of a created model (fxpmodel.py:1110-1161): BatchNorm -> SSM -> ReLU -> out2 ->
// sigmoid -> gate -> residual compute_best add -> ReLU, on the generic int32 kernels (exact for any int32 operands; the
// fused kernels exist for whole forwards, where the int16 inter-kernel planes pay off).
extern "C" int s5fxp_layer_forward(const s5fxp_model *m, int layer, const int32_t *x, int x_bits, int x_exp, int B, int L,
                                   int32_t *y, int32_t *y_exp_dev, void *workspace, size_t workspace_bytes, int32_t *status,
                                   const s5fxp_layer_trace *trace, const s5fxp_forward_opts *opts, void *stream)
{
    if (!m || !x || !y || !workspace || !status || layer < 0 || layer >= m->n_layers || B < 1 || L < 1 || x_bits < 1 || x_bits > 32)
        return S5FXP_EBADARG;
    if (opts && opts->groups > 1) return S5FXP_EUNSUPPORTED;
    if (!stream_extent_ok(m, L)) return S5FXP_EBADARG;
    const WsLayout w = ws_layout(m, B, L);
    if (!w.total || workspace_bytes < w.total) return S5FXP_EWORKSPACE; // 0: the size does not fit a size_t
    hipStream_t st = S(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    LayerDyn *dyn = reinterpret_cast<LayerDyn *>(ws + w.dyn);
    int rc;
    clear_status_generic(m, layer, layer + 1, status, st);
    if ((rc = hip_rc(hipMemsetAsync(dyn, 0, sizeof(LayerDyn) * (size_t)m->n_layers, st)))) return rc;
    // streaming carry of a single layer: the arrays are [1][2][B][P] here
    s5fxp_forward_opts o{};
    if (opts) o = *opts;
    const size_t plane2 = (size_t)2 * B * (m->P ? m->P : 1);
    if (o.state_in) o.state_in -= (size_t)layer * plane2;   // GenericRun::layers indexes the carry by layer
    if (o.state_out) o.state_out -= (size_t)layer * plane2;
    int32_t *h = const_cast<int32_t *>(x), *hn = y; // h is only read
    int hb = x_bits;
    DynExp he{x_exp, nullptr};
    const GenericRun g{m, B, L, w, ws, dyn, status, trace, layer, &o, st, stream};
    if ((rc = g.layers(layer, layer + 1, h, hn, hb, he))) return rc;
    if (y_exp_dev && (rc = hip_rc(hipMemcpyAsync(y_exp_dev, he.dyn, sizeof(int32_t), hipMemcpyDeviceToDevice, st)))) return rc;
    return launch_rc();
}
extern "C" int s5fxp_model_live_states(const s5fxp_model *m, int layer)
{
    if (!m || layer < 0 || layer >= m->n_layers) return -1;
    if (m->fast) return m->fast->layers[layer].n_live;
    return m->P;
}
extern "C" int s5fxp_model_layer_out_bits(const s5fxp_model *m, int layer)
{
    return m && layer >= 0 && layer < m->n_layers ? m->layers[layer].res_bits : -1;
}

// -----------------------------------------------------------------------------------------------
// the float model (float_model.hpp)
// -----------------------------------------------------------------------------------------------
struct s5fxp_float_model {
    int n_layers = 0, H = 0, P = 0, DS = 0;
    const float *enc_w = nullptr, *enc_b = nullptr, *dec_w = nullptr, *dec_b = nullptr;
    struct Layer {
        FNormArgs nm{};
        const float *lam = nullptr, *bcat = nullptr, *ccat = nullptr, *D = nullptr, *w2 = nullptr, *b2 = nullptr;
    };
    std::vector<Layer> layers;
};

namespace {

int float_validate(const s5fxp_float_model_desc *d)
{
    if (!d || d->n_layers < 1 || d->n_layers > 64 || !d->layers || !d->enc_w || !d->enc_b || !d->dec_w || !d->dec_b) return S5FXP_EBADARG;
    if (d->d_in < 1 || d->d_out < 1 || d->H < 1 || d->P < 1) return S5FXP_EBADARG;
    for (int i = 0; i < d->n_layers; ++i) {
        const s5fxp_float_layer_desc &l = d->layers[i];
        if (!l.mean || !l.var || !l.lambda_bar || !l.B_bar || !l.C || !l.D || !l.w2 || !l.b2) return S5FXP_EBADARG;
    }
    const int DS = d->H / 48;
    if (d->d_in != FM_DIN || d->d_out != FM_DIN || DS < 1 || DS > 4 || d->H != 48 * DS || d->P != 32 * DS) return S5FXP_EUNSUPPORTED;
    return S5FXP_OK;
}

// One pass lays the blob out (host == nullptr: sizes only).  Every tensor starts on a 256-byte boundary; pads are zero.
struct FloatPacker {
    size_t off = 0; // in floats
    float *host = nullptr;
    const float *dev = nullptr; // nullptr: size pass, the addresses handed out are null
    float *take(size_t n, const float *&d)
    {
        float *h = host ? host + off : nullptr;
        d = dev ? dev + off : nullptr;
        off = (off + n + 63) & ~(size_t)63;
        return h;
    }
};

size_t float_pack(const s5fxp_float_model_desc *d, FloatPacker &p, s5fxp_float_model *m)
{
    const int H = d->H, P = d->P;
    s5fxp_float_model tmp;
    s5fxp_float_model &o = m ? *m : tmp;
    o.layers.resize(d->n_layers);
    if (float *w = p.take((size_t)FM_KENC * H, o.enc_w)) std::memcpy(w, d->enc_w, (size_t)FM_DIN * H * sizeof(float));
    if (float *b = p.take(H, o.enc_b)) std::memcpy(b, d->enc_b, H * sizeof(float));
    for (int i = 0; i < d->n_layers; ++i) {
        const s5fxp_float_layer_desc &l = d->layers[i];
        s5fxp_float_model::Layer &L = o.layers[i];
        if (float *v = p.take(H, L.nm.mean)) std::memcpy(v, l.mean, H * sizeof(float));
        if (float *v = p.take(H, L.nm.istd))
            for (int h = 0; h < H; ++h) v[h] = 1.0f / sqrtf(l.var[h] + 1e-5f);
        if (float *v = p.take(H, L.nm.scale))
            for (int h = 0; h < H; ++h) v[h] = l.scale ? l.scale[h] : 1.0f;
        if (float *v = p.take(H, L.nm.bias))
            for (int h = 0; h < H; ++h) v[h] = l.bias ? l.bias[h] : 0.0f;
        if (float *v = p.take(2 * P, L.lam)) std::memcpy(v, l.lambda_bar, 2 * P * sizeof(float));
        if (float *v = p.take((size_t)H * 2 * P, L.bcat)) // (H,2P): [h][2p + c] = B_bar[p][h].c
            for (int q = 0; q < P; ++q)
                for (int h = 0; h < H; ++h)
                    for (int c = 0; c < 2; ++c) v[(size_t)h * 2 * P + 2 * q + c] = l.B_bar[((size_t)q * H + h) * 2 + c];
        if (float *v = p.take((size_t)2 * P * H, L.ccat)) // (2P,H): [2p][h] = C_re[h][p], [2p+1][h] = -C_im[h][p]
            for (int h = 0; h < H; ++h)
                for (int q = 0; q < P; ++q) {
                    v[(size_t)(2 * q) * H + h] = l.C[((size_t)h * P + q) * 2];
                    v[(size_t)(2 * q + 1) * H + h] = -l.C[((size_t)h * P + q) * 2 + 1];
                }
        if (float *v = p.take(H, L.D)) std::memcpy(v, l.D, H * sizeof(float));
        if (float *v = p.take((size_t)H * H, L.w2)) std::memcpy(v, l.w2, (size_t)H * H * sizeof(float));
        if (float *v = p.take(H, L.b2)) std::memcpy(v, l.b2, H * sizeof(float));
    }
    if (float *w = p.take((size_t)H * FM_MDEC, o.dec_w))
        for (int h = 0; h < H; ++h) std::memcpy(w + (size_t)h * FM_MDEC, d->dec_w + (size_t)h * FM_DIN, FM_DIN * sizeof(float));
    if (float *b = p.take(FM_MDEC, o.dec_b)) std::memcpy(b, d->dec_b, FM_DIN * sizeof(float));
    return p.off * sizeof(float);
}

constexpr long long FM_GRID_CAP = 512; // workgroups per launch: the weights are loaded into registers once per workgroup

// Local to float_forward<CLIPS> (they use its m, trace and CLIPS) and undefined behind it.  FM_AT_DS: the kernel template k at
// dim_scale ds; what follows are k's template arguments after DS.  FM_K / FM_K_TRACE: the stage kernel of the launch that
// runs, at the model's DS -- `rect` or `clip`, FM_K_TRACE: k<DS, trace>; FM_K_TRACE_HIST: the same for the histogram forms,
// whose clip kernels have no traced instantiation (clip<DS, false>: s5fxp_float_model_clips_traced offers no histogram).  The
// other one sits in a discarded statement, so float_forward<true> names no traced clip histogram kernel, which would create
// it.  The code object lays kernels out in the order the host code first names them: DS 1..4, traced before untraced.
#define FM_AT_DS(ds, k, ...) \
    ((ds) <= 2 ? ((ds) == 1 ? k<1, ##__VA_ARGS__> : k<2, ##__VA_ARGS__>) : ((ds) == 3 ? k<3, ##__VA_ARGS__> : k<4, ##__VA_ARGS__>))
#define FM_RECT_OR_CLIP(rect, clip)       \
    [&] {                                 \
        if constexpr (CLIPS) return clip; \
        else return rect;                 \
    }()
#define FM_K(rect, clip) FM_RECT_OR_CLIP(FM_AT_DS(m->DS, rect), FM_AT_DS(m->DS, clip))
#define FM_K_TRACE(rect, clip)                                                                          \
    FM_RECT_OR_CLIP((trace ? FM_AT_DS(m->DS, rect, true) : FM_AT_DS(m->DS, rect, false)), \
                    (trace ? FM_AT_DS(m->DS, clip, true) : FM_AT_DS(m->DS, clip, false)))
#define FM_K_TRACE_HIST(rect, clip) \
    FM_RECT_OR_CLIP((trace ? FM_AT_DS(m->DS, rect, true) : FM_AT_DS(m->DS, rect, false)), FM_AT_DS(m->DS, clip, false))

// What the rectangular launch (B sequences of L rows) and the clip launch (B clips padded to L rows, lens[e] of them real)
// differ in
struct FmTiling {
    long long N, tiles;
    unsigned grid;
    FClipMap cm; // clips only
};

FmTiling fm_tiling(int B, int L, bool clips, const int32_t *lens)
{
    const int tpc = (int)(((long long)L + FM_FT - 1) / FM_FT);
    FmTiling t{};
    t.N = (long long)B * L;
    t.tiles = clips ? (long long)B * tpc : (t.N + FM_FT - 1) / FM_FT;
    t.grid = (unsigned)(t.tiles < FM_GRID_CAP ? t.tiles : FM_GRID_CAP);
    // A stride that shares a factor with tpc ties a workgroup to few tile positions: at 512 and tpc = 16 it would see the same
    // position of every clip it visits, the workgroups of the early positions all the work and those of the late ones next to
    // none.  A stride coprime to tpc walks every workgroup through all positions.
    if (clips && t.tiles > t.grid)
        while (std::gcd(t.grid, (unsigned)tpc) != 1) --t.grid;
    t.cm = FClipMap{lens, L, tpc, t.tiles};
    return t;
}

// One tile-kernel launch: k(a, [the FClipMap,] what k's form takes behind that: nothing, the histogram rows or the FFq<n> sites)
template <bool CLIPS, class K, class Args, class... Extra>
void fm_launch(const FmTiling &t, hipStream_t st, K k, const Args &a, Extra... extra)
{
    if constexpr (CLIPS) hipLaunchKernelGGL(k, dim3(t.grid), dim3(256), 0, st, a, t.cm, extra...);
    else hipLaunchKernelGGL(k, dim3(t.grid), dim3(256), 0, st, a, extra...);
}

static_assert(FM_HIST_BINS == S5FXP_FLOAT_HIST_BINS && FM_HIST_EMIN == S5FXP_FLOAT_HIST_EMIN, "include/s5fxp.h and float_model.hpp");

// The sites of a fake-quantised forward, checked and prepared on the host: in stats order, 2 for the encoder,
// per layer u, Bu_re, Bu_im, x_re, x_im, y, out2.inp, out2.out, gate.l, gate.r, 2 for the decoder.
struct FqPlan {
    bool any = false;
    std::vector<FqSite> s;
    std::vector<int> step_re, step_im; // per layer: the exponents of its state sites in step mode, or INT_MIN (scan mode)
    bool step(int i) const { return !step_re.empty() && step_re[i] != INT_MIN; }
    FFq<2> enc() const { return {{s[0], s[1]}}; }
    FFq<3> bproj(int i) const { const FqSite *l = &s[2 + 10 * i]; return {{l[0], l[1], l[2]}}; }
    FFq<8> gate(int i) const // u, then the gate kernel's seven observers
    {
        const FqSite *l = &s[2 + 10 * i];
        return {{l[0], l[3], l[4], l[5], l[6], l[7], l[8], l[9]}};
    }
    FFq<2> dec() const { return {{s[s.size() - 2], s[s.size() - 1]}}; }
};

// S5FXP_EBADARG for a site the kernels do not serve; fq == nullptr or every site off leaves plan.any false
int fq_plan(const s5fxp_float_fq_site *fq, int n_layers, FqPlan &plan)
{
    if (!fq) return S5FXP_OK;
    const int n = 4 + 10 * n_layers;
    plan.s.assign(n, FqSite{1.f, 1.f, 0.f, 0.f, 0u});
    plan.step_re.assign(n_layers, INT_MIN);
    plan.step_im.assign(n_layers, INT_MIN);
    for (int j = 0; j < n; ++j) {
        const s5fxp_float_fq_site &q = fq[j];
        if (q.bits == 0) continue;
        const int k = j >= 2 && j < n - 2 ? (j - 2) % 10 : -1;
        const bool state = k == 3 || k == 4; // x_re, x_im: the integer model wraps its state
        if (q.bits < 2 || q.bits > 24 || q.exp < -24 || q.exp > 40 || q.mode > S5FXP_FQ_STEP || q.saturate > 1 ||
            (state && q.saturate) || (q.mode == S5FXP_FQ_STEP && !state))
            return S5FXP_EBADARG;
        if (q.mode == S5FXP_FQ_STEP) { // the recurrence rounds (s5fxp_fq_scan_c64); the gate kernel's site stays off
            (k == 3 ? plan.step_re : plan.step_im)[(j - 2) / 10] = q.exp;
            plan.any = true;
            continue;
        }
        const float half = ldexpf(1.f, q.bits - 1);
        plan.s[j] = FqSite{ldexpf(1.f, q.exp), ldexpf(1.f, -q.exp), -half, half - 1.f,
                           FM_FQF_ON | (q.mode == S5FXP_FQ_NEAREST ? FM_FQF_NEAREST : 0u) | (q.saturate ? FM_FQF_SATURATE : 0u)};
        plan.any = true;
    }
    for (int i = 0; i < n_layers; ++i) // both state sites of a layer step together
        if ((plan.step_re[i] == INT_MIN) != (plan.step_im[i] == INT_MIN)) return S5FXP_EBADARG;
    return S5FXP_OK;
}

// The one forward of the five entries, rectangular (B sequences of L rows) or, with CLIPS, B clips padded to L rows of which
// lens[e] are real (trace planes: 4x, padded like y, never together with hist).  hist == nullptr launches exactly the kernels without the histogram, and
// fq == nullptr or all off exactly those without fake quantisation (the two are never given together).  A layer whose state
// sites are in step mode runs k_scan_fq_c64 in place of the associative scan; every other launch is unchanged.
template <bool CLIPS>
int float_forward(const s5fxp_float_model *m, const float *x, int B, int L, const int32_t *lens, float *y, float *stats,
                  unsigned long long *hist, const s5fxp_float_fq_site *fq, float *trace, void *workspace, size_t workspace_bytes,
                  void *stream)
{
    if (!m || !x || !y || (CLIPS && !lens) || !workspace || B < 1 || L < 1) return S5FXP_EBADARG;
    if (reinterpret_cast<uintptr_t>(hist) % sizeof(unsigned long long)) return S5FXP_EBADARG;
    if (CLIPS && hist && trace) return S5FXP_EBADARG; // the clip histogram kernels have no traced form
    FqPlan qp;
    if (fq_plan(fq, m->n_layers, qp)) return S5FXP_EBADARG;
    const FmTiling t = fm_tiling(B, L, CLIPS, lens);
    if (hist && !fm_hist_rows_ok(t.tiles, t.grid)) return S5FXP_EBADARG; // a 32-bit LDS counter could wrap
    const size_t ws_need = s5fxp_float_workspace_bytes(m, B, L, trace != nullptr);
    if (!ws_need || workspace_bytes < ws_need) return S5FXP_EWORKSPACE; // 0: the size does not fit a size_t
    const int64_t scan_grid = (int64_t)B * ((m->P + ASSOC_PT - 1) / ASSOC_PT); // of the clip scan
    if (CLIPS && scan_grid > 0x7fffffffll) return S5FXP_EBADARG;
    for (int i = 0; i < m->n_layers; ++i) // what s5fxp_fq_scan_c64 would refuse, before anything is launched
        if (qp.step(i) && (((int64_t)B * m->P + 63) / 64 > 0x7fffffffll || !fqs_span_ok(L, m->P))) return S5FXP_EBADARG;
    const long long N = t.N;
    const size_t NH = (size_t)N * m->H, NP2 = (size_t)N * 2 * m->P;
    hipStream_t st = S(stream);
    unsigned *obs = reinterpret_cast<unsigned *>(stats);
    float *ws = static_cast<float *>(workspace);
    float *hbuf[2] = {ws, ws + NH};
    float *planes = ws + 2 * NH; // per layer (trace) or shared: Bu, xs
    int rc;

    float *h = hbuf[0];
    FEncArgs ea{x, m->enc_w, m->enc_b, h, obs, N};
    if (qp.any) fm_launch<CLIPS>(t, st, FM_K(k_fenc_fq, k_fenc_clips_fq), ea, qp.enc());
    else if (hist) fm_launch<CLIPS>(t, st, FM_K(k_fenc_hist, k_fenc_clips_hist), ea, hist);
    else fm_launch<CLIPS>(t, st, FM_K(k_fenc, k_fenc_clips), ea);
    if ((rc = launch_rc())) return rc;
    for (int i = 0; i < m->n_layers; ++i) {
        const s5fxp_float_model::Layer &l = m->layers[i];
        float *bu = planes + (trace ? (size_t)i * 2 * NP2 : 0), *xs = bu + NP2;
        float *tr = trace ? trace + (size_t)i * 5 * NH : nullptr; // u, y, g_in, g, h'
        float *hout = trace ? tr + 4 * NH : hbuf[(i + 1) & 1];
        unsigned *lo = obs ? obs + 2 + 10 * i : nullptr;
        unsigned long long *lh = hist ? hist + (size_t)(2 + 10 * i) * FM_HIST_BINS : nullptr;
        FBprojArgs ba{h, l.nm, l.bcat, bu, tr, lo, N};
        if (qp.any) fm_launch<CLIPS>(t, st, FM_K_TRACE(k_fbproj_fq, k_fbproj_clips_fq), ba, qp.bproj(i));
        else if (hist) fm_launch<CLIPS>(t, st, FM_K_TRACE_HIST(k_fbproj_hist, k_fbproj_clips_hist), ba, lh);
        else fm_launch<CLIPS>(t, st, FM_K_TRACE(k_fbproj, k_fbproj_clips), ba);
        if ((rc = launch_rc())) return rc;
        if (qp.step(i)) {
            rc = s5fxp_fq_scan_c64(l.lam, bu, xs, nullptr, nullptr, lens, B, L, m->P, qp.step_re[i], qp.step_im[i], stream);
        } else if constexpr (CLIPS) {
            ScanAssocClipsArgs sa{reinterpret_cast<const float2 *>(l.lam), reinterpret_cast<const float2 *>(bu),
                                  reinterpret_cast<float2 *>(xs), lens, B, L, m->P};
            hipLaunchKernelGGL(k_scan_assoc_c64_clips, dim3((unsigned)scan_grid), dim3(64 * ASSOC_WAVES), 0, st, sa);
            rc = launch_rc();
        } else {
            rc = s5fxp_assoc_scan_c64(l.lam, bu, xs, nullptr, nullptr, B, L, m->P, 0, stream);
        }
        if (rc) return rc;
        FGateArgs ga{xs, h, l.nm, l.ccat, l.D, l.w2, l.b2, hout, tr ? tr + NH : nullptr, tr ? tr + 2 * NH : nullptr,
                     tr ? tr + 3 * NH : nullptr, lo ? lo + 3 : nullptr, N};
        unsigned long long *gh = lh ? lh + 3 * FM_HIST_BINS : nullptr;
        if (qp.any) fm_launch<CLIPS>(t, st, FM_K_TRACE(k_fgate_fq, k_fgate_clips_fq), ga, qp.gate(i));
        else if (hist) fm_launch<CLIPS>(t, st, FM_K_TRACE_HIST(k_fgate_hist, k_fgate_clips_hist), ga, gh);
        else fm_launch<CLIPS>(t, st, FM_K_TRACE(k_fgate, k_fgate_clips), ga);
        if ((rc = launch_rc())) return rc;
        h = hout;
    }
    FDecArgs da{h, m->dec_w, m->dec_b, y, obs ? obs + 2 + 10 * m->n_layers : nullptr, N};
    unsigned long long *dh = hist ? hist + (size_t)(2 + 10 * m->n_layers) * FM_HIST_BINS : nullptr;
    if (qp.any) fm_launch<CLIPS>(t, st, FM_K(k_fdec_fq, k_fdec_clips_fq), da, qp.dec());
    else if (hist) fm_launch<CLIPS>(t, st, FM_K(k_fdec_hist, k_fdec_clips_hist), da, dh);
    else fm_launch<CLIPS>(t, st, FM_K(k_fdec, k_fdec_clips), da);
    return launch_rc();
}
#undef FM_AT_DS
#undef FM_RECT_OR_CLIP
#undef FM_K
#undef FM_K_TRACE
#undef FM_K_TRACE_HIST

} // namespace

extern "C" size_t s5fxp_float_model_blob_bytes(const s5fxp_float_model_desc *desc)
{
    if (float_validate(desc) != S5FXP_OK) return 0;
    FloatPacker p;
    return float_pack(desc, p, nullptr);
}

extern "C" int s5fxp_float_model_pack(const s5fxp_float_model_desc *desc, void *host_blob, size_t blob_bytes)
{
    if (!host_blob) return S5FXP_EBADARG;
    int rc = float_validate(desc);
    if (rc) return rc;
    const size_t need = s5fxp_float_model_blob_bytes(desc);
    if (blob_bytes < need) return S5FXP_EWORKSPACE;
    std::memset(host_blob, 0, need);
    FloatPacker p;
    p.host = static_cast<float *>(host_blob);
    p.dev = p.host;
    float_pack(desc, p, nullptr);
    return S5FXP_OK;
}

extern "C" int s5fxp_float_model_create(const s5fxp_float_model_desc *desc, void *dev_blob, size_t blob_bytes, void *stream,
                                        s5fxp_float_model **out)
{
    if (!out || !dev_blob) return S5FXP_EBADARG;
    *out = nullptr;
    int rc = float_validate(desc);
    if (rc) return rc;
    const size_t need = s5fxp_float_model_blob_bytes(desc);
    if (blob_bytes < need) return S5FXP_EWORKSPACE;
    s5fxp_float_model *m = new (std::nothrow) s5fxp_float_model();
    if (!m) return S5FXP_EBADARG;
    m->n_layers = desc->n_layers; m->H = desc->H; m->P = desc->P; m->DS = desc->H / 48;
    std::vector<float> host(need / sizeof(float), 0.0f);
    FloatPacker p;
    p.host = host.data();
    p.dev = static_cast<const float *>(dev_blob);
    float_pack(desc, p, m);
    // pageable-memory async copies are staged by the runtime before returning, so `host` may go
    rc = hip_rc(hipMemcpyAsync(dev_blob, host.data(), need, hipMemcpyHostToDevice, S(stream)));
    if (!rc) rc = hip_rc(hipStreamSynchronize(S(stream))); // creation is not on the hot path
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return S5FXP_OK;
}

extern "C" void s5fxp_float_model_destroy(s5fxp_float_model *m) { delete m; }

extern "C" size_t s5fxp_float_workspace_bytes(const s5fxp_float_model *m, int B, int L, int trace)
{
    if (!m || B < 1 || L < 1) return 0;
    const wide_t N = (wide_t)B * L;
    return fit_size((2 * N * m->H + (wide_t)(trace ? m->n_layers : 1) * 2 * N * 2 * m->P) * sizeof(float));
}

extern "C" size_t s5fxp_float_trace_bytes(const s5fxp_float_model *m, int B, int L)
{
    if (!m || B < 1 || L < 1) return 0;
    return (size_t)m->n_layers * 5 * (size_t)B * L * m->H * sizeof(float);
}

extern "C" int s5fxp_float_model_forward(const s5fxp_float_model *m, const float *x, int B, int L, float *y, float *stats,
                                         float *trace, void *workspace, size_t workspace_bytes, void *stream)
{
    return float_forward<false>(m, x, B, L, nullptr, y, stats, nullptr, nullptr, trace, workspace, workspace_bytes, stream);
}

extern "C" int s5fxp_float_model_forward_hist(const s5fxp_float_model *m, const float *x, int B, int L, float *y, float *stats,
                                              unsigned long long *hist, float *trace, void *workspace, size_t workspace_bytes,
                                              void *stream)
{
    return float_forward<false>(m, x, B, L, nullptr, y, stats, hist, nullptr, trace, workspace, workspace_bytes, stream);
}

extern "C" int s5fxp_float_model_forward_fq(const s5fxp_float_model *m, const float *x, int B, int L, float *y, float *stats,
                                            const s5fxp_float_fq_site *fq, float *trace, void *workspace, size_t workspace_bytes,
                                            void *stream)
{
    return float_forward<false>(m, x, B, L, nullptr, y, stats, nullptr, fq, trace, workspace, workspace_bytes, stream);
}

extern "C" int s5fxp_float_model_clips(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens, float *y,
                                       float *stats, unsigned long long *hist, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    return float_forward<true>(m, x, n, Lmax, lens, y, stats, hist, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int s5fxp_float_model_clips_fq(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens, float *y,
                                          float *stats, const s5fxp_float_fq_site *fq, void *workspace, size_t workspace_bytes,
                                          void *stream)
{
    return float_forward<true>(m, x, n, Lmax, lens, y, stats, nullptr, fq, nullptr, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// Stage errors (stage_err.hpp): up to 4096 pairs of strided boxes compared in two launches.  The workspace holds
// the device form of the descriptors (one stream-ordered copy), then one partial record per workgroup.
namespace {
constexpr size_t stage_desc_bytes(int n_pairs) { return ((size_t)n_pairs * sizeof(stage::DevPair) + 255) / 256 * 256; }
static_assert(sizeof(s5fxp_stage_err_rec) == stage::REC_WORDS * 8, "s5fxp_stage_err_rec is REC_WORDS 8-byte words");
} // namespace

extern "C" size_t s5fxp_stage_err_workspace_bytes(int n_pairs)
{
    if (n_pairs < 1 || n_pairs > 4096) return 0;
    return stage_desc_bytes(n_pairs) + (size_t)n_pairs * stage::stage_wgs_cap(n_pairs) * sizeof(s5fxp_stage_err_rec);
}

extern "C" int s5fxp_stage_err(const s5fxp_stage_pair *pairs_host, int n_pairs, s5fxp_stage_err_rec *out_dev, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!pairs_host || !out_dev || !workspace || n_pairs < 1 || n_pairs > 4096) return S5FXP_EBADARG;
    const int cap = stage::stage_wgs_cap(n_pairs);
    std::vector<stage::DevPair> dev((size_t)n_pairs);
    uint64_t n_max = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const s5fxp_stage_pair &p = pairs_host[i];
        if (p.a_kind != S5FXP_STAGE_I32 && p.a_kind != S5FXP_STAGE_F32) return S5FXP_EBADARG;
        if (p.flags & ~S5FXP_STAGE_RELU_A) return S5FXP_EBADARG;
        if (p.a_kind == S5FXP_STAGE_I32 && (p.a_exp < 0 || p.a_exp > 40)) return S5FXP_EBADARG;
        if (p.nb < 0 || p.rows < 0 || p.cols < 0) return S5FXP_EBADARG;
        const unsigned __int128 n = (unsigned __int128)p.nb * (unsigned)p.rows * (unsigned)p.cols;
        if (n && (!p.a || !p.b)) return S5FXP_EBADARG;
        // the wrap rule: a workgroup's share of the pair, at the most workgroups this call can use, stays below 2^32
        if (n > (unsigned __int128)cap * 0xffffff00ull) return S5FXP_EBADARG;
        stage::DevPair &d = dev[i];
        d.a = static_cast<const uint32_t *>(p.a), d.b = p.b;
        for (int k = 0; k < 3; ++k) d.as[k] = p.a_stride[k], d.bs[k] = p.b_stride[k];
        d.n = (uint64_t)n;
        d.scale = p.a_kind == S5FXP_STAGE_I32 ? std::ldexp(1.0, -p.a_exp) : 1.0;
        d.rows = (uint32_t)p.rows, d.cols = (uint32_t)p.cols;
        d.f32 = p.a_kind == S5FXP_STAGE_F32, d.relu = (p.flags & S5FXP_STAGE_RELU_A) != 0;
        n_max = std::max(n_max, d.n);
    }
    if (workspace_bytes < s5fxp_stage_err_workspace_bytes(n_pairs)) return S5FXP_EWORKSPACE;
    // workgroups per pair from the largest pair: fewer than `cap` only while every share is WG_MIN_ELEMS at most
    const uint64_t want = (n_max + stage::WG_MIN_ELEMS - 1) / stage::WG_MIN_ELEMS;
    const int wgs = (int)std::min<uint64_t>((uint64_t)cap, std::max<uint64_t>(want, 1));
    char *ws = static_cast<char *>(workspace);
    auto *partials = reinterpret_cast<unsigned long long *>(ws + stage_desc_bytes(n_pairs));
    // pageable-memory async copies are staged by the runtime before returning, so `dev` may go
    if (const int rc = hip_rc(hipMemcpyAsync(ws, dev.data(), dev.size() * sizeof(stage::DevPair), hipMemcpyHostToDevice, S(stream))))
        return rc;
    hipLaunchKernelGGL(stage::k_stage_err, dim3((unsigned)wgs, (unsigned)n_pairs), dim3(stage::TPB), 0, S(stream),
                       reinterpret_cast<const stage::DevPair *>(ws), partials);
    hipLaunchKernelGGL(stage::k_stage_err_finalize, dim3((unsigned)n_pairs), dim3(stage::TPB), 0, S(stream), partials, wgs,
                       reinterpret_cast<unsigned long long *>(out_dev));
    return launch_rc();
}

// The ragged form: the same two launches over padded boxes, masked by the clips' lengths on the device.
namespace {
constexpr size_t stage_clips_desc_bytes(int n_pairs) { return ((size_t)n_pairs * sizeof(stage::DevPairClips) + 255) / 256 * 256; }
static_assert(sizeof(s5fxp_stage_pair_clips) == 120, "s5fxp_stage_pair_clips is 120 bytes (include/s5fxp.h, verify.StagePairClips)");
} // namespace

extern "C" size_t s5fxp_stage_err_clips_workspace_bytes(int n_pairs)
{
    if (n_pairs < 1 || n_pairs > 4096) return 0;
    return stage_clips_desc_bytes(n_pairs) + (size_t)n_pairs * stage::stage_wgs_cap(n_pairs) * sizeof(s5fxp_stage_err_rec);
}

extern "C" int s5fxp_stage_err_clips(const s5fxp_stage_pair_clips *pairs_host, int n_pairs, s5fxp_stage_err_rec *out_dev,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    if (!pairs_host || !out_dev || !workspace || n_pairs < 1 || n_pairs > 4096) return S5FXP_EBADARG;
    const int cap = stage::stage_wgs_cap(n_pairs);
    std::vector<stage::DevPairClips> dev((size_t)n_pairs);
    uint64_t n_max = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const s5fxp_stage_pair_clips &pc = pairs_host[i];
        const s5fxp_stage_pair &p = pc.box;
        if (p.a_kind != S5FXP_STAGE_I32 && p.a_kind != S5FXP_STAGE_F32) return S5FXP_EBADARG;
        if (p.flags & ~S5FXP_STAGE_RELU_A) return S5FXP_EBADARG;
        if (p.a_kind == S5FXP_STAGE_I32 && !pc.a_exp_dev && (p.a_exp < 0 || p.a_exp > 40)) return S5FXP_EBADARG;
        if (p.nb < 0 || p.rows < 0 || p.cols < 0 || pc.row0 < 0 || pc.reserved) return S5FXP_EBADARG;
        const unsigned __int128 n = (unsigned __int128)p.nb * (unsigned)p.rows * (unsigned)p.cols;
        if (n && (!p.a || !p.b || !pc.lens)) return S5FXP_EBADARG;
        // the wrap rule of s5fxp_stage_err, on the padded box
        if (n > (unsigned __int128)cap * 0xffffff00ull) return S5FXP_EBADARG;
        stage::DevPairClips &dc = dev[i];
        stage::DevPair &d = dc.box;
        d.a = static_cast<const uint32_t *>(p.a), d.b = p.b;
        for (int k = 0; k < 3; ++k) d.as[k] = p.a_stride[k], d.bs[k] = p.b_stride[k];
        d.n = (uint64_t)n;
        d.scale = p.a_kind == S5FXP_STAGE_I32 && !pc.a_exp_dev ? std::ldexp(1.0, -p.a_exp) : 1.0;
        d.rows = (uint32_t)p.rows, d.cols = (uint32_t)p.cols;
        d.f32 = p.a_kind == S5FXP_STAGE_F32, d.relu = (p.flags & S5FXP_STAGE_RELU_A) != 0;
        dc.lens = pc.lens, dc.a_exp_dev = pc.a_exp_dev, dc.a_exp_stride = pc.a_exp_stride, dc.row0 = pc.row0, dc.pad = 0;
        n_max = std::max(n_max, d.n);
    }
    if (workspace_bytes < s5fxp_stage_err_clips_workspace_bytes(n_pairs)) return S5FXP_EWORKSPACE;
    const uint64_t want = (n_max + stage::WG_MIN_ELEMS - 1) / stage::WG_MIN_ELEMS;
    const int wgs = (int)std::min<uint64_t>((uint64_t)cap, std::max<uint64_t>(want, 1));
    char *ws = static_cast<char *>(workspace);
    auto *partials = reinterpret_cast<unsigned long long *>(ws + stage_clips_desc_bytes(n_pairs));
    // pageable-memory async copies are staged by the runtime before returning, so `dev` may go
    if (const int rc = hip_rc(hipMemcpyAsync(ws, dev.data(), dev.size() * sizeof(stage::DevPairClips), hipMemcpyHostToDevice, S(stream))))
        return rc;
    hipLaunchKernelGGL(stage::k_stage_err_clips, dim3((unsigned)wgs, (unsigned)n_pairs), dim3(stage::TPB), 0, S(stream),
                       reinterpret_cast<const stage::DevPairClips *>(ws), partials);
    hipLaunchKernelGGL(stage::k_stage_err_finalize, dim3((unsigned)n_pairs), dim3(stage::TPB), 0, S(stream), partials, wgs,
                       reinterpret_cast<unsigned long long *>(out_dev));
    return launch_rc();
}

// The clip forward with trace planes: the TRACE instantiations of k_fbproj_clips[_fq] / k_fgate_clips[_fq]; Bu
// and xs of every layer stay in the workspace, as in the rectangular traced forward.
extern "C" int s5fxp_float_model_clips_traced(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens,
                                              float *y, float *stats, const s5fxp_float_fq_site *fq, float *trace, void *workspace,
                                              size_t workspace_bytes, void *stream)
{
    if (!trace) return S5FXP_EBADARG;
    return float_forward<true>(m, x, n, Lmax, lens, y, stats, nullptr, fq, trace, workspace, workspace_bytes, stream);
}

#ifdef S5_PHASE_PROF
// tools/prof_phases.py only (a -DS5_PHASE_PROF build): the accumulated phase clocks of k_enc_p
extern "C" int s5fxp_debug_phase_prof(long long *host_out, int n)
{
    return hip_rc(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_phase_prof), (size_t)n * sizeof(long long)));
}
#endif
