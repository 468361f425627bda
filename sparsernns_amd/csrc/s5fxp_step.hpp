// s5fxp_step.hpp -- the one-launch streaming step (include/s5fxp.h s5fxp_model_step): a whole forward of the fixed-point
// S5 model, encoder to decoder, for R = B * L <= 32 rows in ONE workgroup; G independent groups are G workgroups of one
// launch.  Included by s5fxp_api.hip after s5fxp_fast.hpp (it reads FastModel's packed int8 weight rows).
//
// Why one workgroup can do it: every tensor-wide maximum the model needs (the four BatchNorm compute_best exponents,
// the residual add's exponent, the width of the states) is over R x H <= 32 x 192 values -- a workgroup reduction.  The
// batch path (s5fxp_fast.hpp) needs a kernel boundary for each of them; here they are __syncthreads().
//
// Arithmetic: exactly the generic kernels' (s5fxp_kernels.hpp), op for op -- bn_chain, finalize_add_cb / finalize_mul_cb,
// scan_step, crelu, sigmoid_lut, add_cb_apply -- with the int32 contractions on the int8 matrix cores as mfma_proj.hpp
// describes: a 16-bit activation is two signed byte planes, an int32 state four, one v_mfma_i32_32x32x32_i8 pass per
// plane, the partial sums recombined modulo 2^32 (fxparray.py:662 sums in int32 with wrap, so any split is exact).
//   * rows R..31 of the 32-row MFMA tile are padding: their A-operand lanes re-read row R-1 (defined memory) and their
//     results are dropped by the epilogues' row < R test -- they reach no maximum, check, carry or store;
//   * k columns beyond a projection's K meet zero weights (pack_mfma pads with zeros), so their plane bytes are free;
//   * the recurrence is the plain 32-bit chain of fxpmodel.py:147-172 (scan_step), one thread per (sequence, state),
//     L <= 32 steps: no pair / quad rung, no range bound, no redo;
//   * the C projection is exact for int32 states of any width: when every state of the layer (after the complex ReLU)
//     fits 16 bits -- a workgroup-uniform test -- two byte planes run, otherwise four.
// Two kernels share the body (s5fxp_step_body.inc): k_model_step, every group B x L rows and carry g, and k_model_step_ragged,
// every group its own row count and carry slot from a descriptor (s5fxp_model_step_ragged), x and y padded to Lmax frames.
// The clip kernel (s5fxp_clip.hpp) repeats the body's stages over 32-row tiles.  One stage is a function both call,
// step_bn_exps below (the four BatchNorm exponent reductions); the others are still text in both and have to be kept
// equal by hand (DESIGN.md 4o says why they stayed).  The three entries share one launcher, step_launch.
// Each of the three also has a form at STATED exponents (the _at entries): k_model_step_at,
// k_model_step_ragged_at and k_model_clips_at are the same bodies with STEP_PINNED / CLIP_PINNED, in which step_bn_pinned
// stands for step_bn_exps and no maximum is gathered or reduced.
// LDS (dynamic, sized by R): [PLA: encoder-input / state planes][PLB: u / out2-input / decoder-input planes]
//   [h int16 R x H][x1 int16 R x H][z int16 R x H][bq int32 2 x R x P].  R = 32 at H = 192: 120 KB; R = 1: 3.4 KB.
#pragma once
#include "pinned_exps.hpp"

namespace s5 {

constexpr int STEP_MAX_ROWS = 32;
constexpr int STEP_CUS = 256;          // MI355X
constexpr size_t STEP_STATIC_LDS = 2048; // the kernel's static LDS (status words, reduction slots, LayerDyn, LUT), rounded up
constexpr int STEP_MAX_WAVES = 8; // workgroups of 512, 256 or 128 threads (step_entry chooses)

struct StepDense {
    MfmaW w;
    const int32_t *bias_eff;
    int32_t K, M, inp_bits, inp_exp, w_exp, out_bits, out_exp;
};

struct StepLayer {
    BnArgs bn; // xe and dyn are filled in by the kernel (the layer input's exponent is chosen on the device)
    MfmaW bproj, cre, cim, out2;
    const int32_t *o2_bias_eff, *Dpad, *a_re, *a_im;
    int32_t rs_bre, rs_bim, bre_bits, bim_bits, sh_re, sh_im, ea_re, ea_im;
    int32_t rs_cre, rs_cim, rs_d, y_bits, y_exp;
    int32_t o2_conv, o2_inp_bits, o2_inp_exp, rs_o2, o2_out_bits, o2_out_exp, sig_x, sig_y;
    int32_t lut[8];
    int32_t l_bits, l_exp, r_bits, r_exp, res_bits, res_exp, rs_gate;
};

// Appended to the model blob by s5fxp_model_create (device memory; every pointer inside is a device address)
struct StepParams {
    int32_t n_layers, H, P, hp, d_in, d_out;
    StepDense enc, dec;
    StepLayer layers[15]; // 8 + 8 * n_layers <= S5FXP_STATUS_WORDS
};

struct StepArgs {
    const StepParams *sp;
    const void *x;          // (G,B,L,d_in) int32, or float32 with f32
    void *y;                // (G,B,L,d_out) int32 / float32
    const int32_t *state_in; // [G][n_layers][2][B][P] or nullptr (zeros)
    int32_t *state_out;      // the same layout or nullptr; may alias state_in
    int32_t *status;         // G x S5FXP_STATUS_WORDS
    int32_t B, L, x_bits, x_exp, f32;
};

// LDS extents of one group of R rows (bytes; every region 16-byte aligned)
struct StepLds {
    int kpa_enc, kpa_st, kpb; // row strides of the byte planes: encoder input, states, u / out2 input / decoder input
    size_t pla, plb, hb, x1, z, bq, total;
};
__host__ __device__ inline StepLds step_lds(int R, int H, int P, int hp, int d_in)
{
    StepLds l{};
    auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
    l.kpa_enc = (d_in + 31) / 32 * 32 + 16;
    l.kpa_st = P + 16;
    l.kpb = hp + 16;
    const size_t enc = 2 * (size_t)R * l.kpa_enc, st = 8 * (size_t)R * l.kpa_st;
    size_t off = 0;
    l.pla = off; off += al(enc > st ? enc : st);
    l.plb = off; off += al(2 * (size_t)R * l.kpb);
    l.hb = off; off += al(2 * (size_t)R * H);
    l.x1 = off; off += al(2 * (size_t)R * H);
    l.z = off; off += al(2 * (size_t)R * H);
    l.bq = off; off += al(8 * (size_t)R * P);
    l.total = off;
    return l;
}

// 16-bit value -> two byte planes [lo ^ 0x80][hi]; int32 value -> four [b0 ^ 0x80][b1 ^ 0x80][b2 ^ 0x80][b3] (mfma_proj.hpp)
__device__ __forceinline__ void step_put2(int8_t *pl, int pstride, int off, int32_t v)
{
    pl[off] = (int8_t)((v & 0xff) ^ 0x80);
    pl[pstride + off] = (int8_t)(v >> 8);
}
__device__ __forceinline__ void step_put4(int8_t *pl, int pstride, int off, int32_t v)
{
    pl[off] = (int8_t)((v & 0xff) ^ 0x80);
    pl[pstride + off] = (int8_t)(((v >> 8) & 0xff) ^ 0x80);
    pl[2 * pstride + off] = (int8_t)(((v >> 16) & 0xff) ^ 0x80);
    pl[3 * pstride + off] = (int8_t)(v >> 24);
}

// One 32 x 32 output tile: rows = the group's rows (A operand: NPL byte planes [plane][row][KP] in LDS), columns =
// channels 32 * tile .. + 31 (B operand: the channel's int8 weight row, 16 bytes per k-step and lane half, from the blob).
// Two planes accumulate side by side (independent MFMA chains); four planes are two such pairs.  Lane (r = lane & 31,
// h = lane >> 5) receives column 32 * tile + r of rows (i & 3) + 8 * (i >> 2) + 4 * h, i = 0..15.
template <int NPL>
__device__ __forceinline__ v16i step_mm(const int8_t *pl, int pstride, int KP, int arow, int h, const MfmaW &w, int col, int nks)
{
    static_assert(NPL == 2 || NPL == 4, "byte planes of a 16- or 32-bit operand");
    const int8_t *wrow = as_global(w.wt) + (size_t)col * w.Kp + 16 * h;
    const int8_t *xrow = pl + arow * KP + 16 * h;
    const int32_t cs128 = as_global(w.cs128)[col];
    v16i total;
#pragma unroll
    for (int i = 0; i < 16; ++i) total[i] = 0;
#pragma unroll
    for (int pp = NPL - 2; pp >= 0; pp -= 2) {
        v16i a0, a1;
#pragma unroll
        for (int i = 0; i < 16; ++i) a0[i] = a1[i] = 0;
        for (int ks = 0; ks < nks; ++ks) {
            const v4i b = *reinterpret_cast<const v4i *>(wrow + 32 * ks);
            const v4i x1 = *reinterpret_cast<const v4i *>(xrow + (pp + 1) * pstride + 32 * ks);
            const v4i x0 = *reinterpret_cast<const v4i *>(xrow + pp * pstride + 32 * ks);
            a1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(x1, b, a1, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(x0, b, a0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) total[i] = wadd(wadd(wshl(total[i], 16), wshl(a1[i], 8)), a0[i]);
    }
    // the +128 offsets of the lower planes: 128 * sum(w) once per lower plane at that plane's weight
    const int32_t cs = wmul(cs128, NPL == 2 ? 1 : 65793);
#pragma unroll
    for (int i = 0; i < 16; ++i) total[i] = wadd(total[i], cs);
    return total;
}

// maxima of NV non-negative floats over the workgroup; every thread receives them
template <int NV, int STEP_WAVES>
__device__ __forceinline__ void step_wg_max(float (&v)[NV], float (*red)[STEP_MAX_WAVES])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float x = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
        if (lane == 0) red[i][wave] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float x = red[i][0];
#pragma unroll
        for (int w = 1; w < STEP_WAVES; ++w) x = fmaxf(x, red[i][w]);
        v[i] = x;
    }
    __syncthreads();
}

// ---- the four BatchNorm compute_best exponents (fxpmodel.py:892-933): full reductions over the n values of h, the rule of
// k_bn_reduce / k_bn_finalize.  One function for the step kernels (h in LDS, n = R * H) and the clip kernel (h in the
// workgroup's scratch, n = len * H): it is inlined, so h keeps the address space its kernel gave it.  Each reduction ends
// behind a barrier; after the last one s_d is complete for every thread.
template <int STEP_THREADS>
__device__ __forceinline__ void step_bn_exps(const int16_t *hsrc, int n, int H, const BnArgs &bn, int he, LayerDyn &s_d,
                                             int32_t *s_status, int32_t *st_exps, float (*s_red)[STEP_MAX_WAVES])
{
    constexpr int STEP_WAVES = STEP_THREADS / 64;
    const int tid = threadIdx.x;
    {
        float v[3] = {0.f, 0.f, 0.f};
        for (int i = tid; i < n; i += STEP_THREADS) {
            const int c = i % H;
            const float fx = tofloat(hsrc[i], he), fm = tofloat(bn.mm[c], bn.me);
            v[0] = fmaxf(v[0], fabsf(__fadd_rn(fx, fm)));
            v[1] = fmaxf(v[1], fabsf(fx));
            v[2] = fmaxf(v[2], fabsf(fm));
        }
        step_wg_max<3, STEP_WAVES>(v, s_red);
        if (tid == 0) {
            const uint32_t m3[3] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
            s_d.bn1 = finalize_add_cb(m3, he, bn.me, bn.b1, s_status);
            st_exps[0] = s_d.bn1.eo;
            s_d.bn_e = s_d.bn1.eo;
        }
        __syncthreads();
    }
    {
        LayerDyn d = s_d;
        float v[1] = {0.f};
        for (int i = tid; i < n; i += STEP_THREADS) {
            const int c = i % H;
            const int32_t t = bn_chain<1>(bn, d, hsrc[i], c);
            v[0] = fmaxf(v[0], fabsf(__fmul_rn(tofloat(t, d.bn1.eo), tofloat(bn.isv[c], bn.ie))));
        }
        step_wg_max<1, STEP_WAVES>(v, s_red);
        if (tid == 0) {
            finalize_mul_cb(__float_as_uint(v[0]), s_d.bn1.eo, bn.ie, bn.b2, s_d.rs2, s_d.e2, s_status);
            st_exps[1] = s_d.e2;
            s_d.bn_e = s_d.e2;
        }
        __syncthreads();
    }
    if (bn.scale) {
        LayerDyn d = s_d;
        float v[1] = {0.f};
        for (int i = tid; i < n; i += STEP_THREADS) {
            const int c = i % H;
            const int32_t t = bn_chain<2>(bn, d, hsrc[i], c);
            v[0] = fmaxf(v[0], fabsf(__fmul_rn(tofloat(t, d.e2), tofloat(bn.scale[c], bn.se))));
        }
        step_wg_max<1, STEP_WAVES>(v, s_red);
        if (tid == 0) {
            finalize_mul_cb(__float_as_uint(v[0]), s_d.e2, bn.se, bn.b3, s_d.rs3, s_d.e3, s_status);
            st_exps[2] = s_d.e3;
            s_d.bn_e = s_d.e3;
        }
        __syncthreads();
    }
    if (bn.bias) {
        LayerDyn d = s_d;
        float v[3] = {0.f, 0.f, 0.f};
        for (int i = tid; i < n; i += STEP_THREADS) {
            const int c = i % H;
            const int32_t t = bn_chain<3>(bn, d, hsrc[i], c);
            const float ft = tofloat(t, bn.scale ? d.e3 : d.e2), fb = tofloat(bn.bias[c], bn.be);
            v[0] = fmaxf(v[0], fabsf(__fadd_rn(ft, fb)));
            v[1] = fmaxf(v[1], fabsf(ft));
            v[2] = fmaxf(v[2], fabsf(fb));
        }
        step_wg_max<3, STEP_WAVES>(v, s_red);
        if (tid == 0) {
            const uint32_t m3[3] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
            s_d.bn4 = finalize_add_cb(m3, bn.scale ? s_d.e3 : s_d.e2, bn.be, bn.b4, s_status);
            st_exps[3] = s_d.bn4.eo;
            s_d.bn_e = s_d.bn4.eo;
        }
        __syncthreads();
    }
}

// ---- stated exponents (the _at entries): PinExps, pinned_add_cb and step_bn_pinned are in pinned_exps.hpp, which the
// batch forward's head shares (s5fxp_fast.hpp)

// STEP_THREADS: 512 when the groups are at most one per CU (eight waves shorten one group's chain of stages); 256 or 128
// when there are more groups than CUs and several fit a CU (the kernel needs up to 256 registers per lane, so a CU holds
// eight waves of it: one, two or four workgroups)
template <int STEP_THREADS>
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_step(StepArgs a)
{
#define STEP_RAGGED 0
#define STEP_PINNED 0
#include "s5fxp_step_body.inc"
#undef STEP_PINNED
#undef STEP_RAGGED
}

// The same body at stated exponents (s5fxp_model_step_at): an argument struct of its own, so StepArgs keeps its layout
struct StepPinArgs {
    StepArgs c;
    PinExps pin;
};

template <int STEP_THREADS>
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_step_at(StepPinArgs pa)
{
    const StepArgs &a = pa.c;
    const PinExps &pin = pa.pin;
#define STEP_RAGGED 0
#define STEP_PINNED 1
#include "s5fxp_step_body.inc"
#undef STEP_PINNED
#undef STEP_RAGGED
}

// The same body with per-workgroup rows and an indirection into the carry (include/s5fxp.h s5fxp_model_step_ragged)
struct StepRaggedArgs {
    const StepParams *sp;
    const void *x;                // (n,B,Lmax,d_in) int32, or float32 with f32
    void *y;                      // (n,B,Lmax,d_out) int32 / float32
    const s5fxp_push_desc *desc;  // n entries, device memory
    int32_t *state;               // [n_slots][n_layers][2][B][P], entry e updates slot desc[e].slot in place
    int32_t *status;              // n x S5FXP_STATUS_WORDS
    int32_t B, Lmax, x_bits, x_exp, f32;
};

template <int STEP_THREADS>
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_step_ragged(StepRaggedArgs a)
{
#define STEP_RAGGED 1
#define STEP_PINNED 0
#include "s5fxp_step_body.inc"
#undef STEP_PINNED
#undef STEP_RAGGED
}

struct StepRaggedPinArgs {
    StepRaggedArgs c;
    PinExps pin;
};

template <int STEP_THREADS>
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_step_ragged_at(StepRaggedPinArgs pa)
{
    const StepRaggedArgs &a = pa.c;
    const PinExps &pin = pa.pin;
#define STEP_RAGGED 1
#define STEP_PINNED 1
#include "s5fxp_step_body.inc"
#undef STEP_PINNED
#undef STEP_RAGGED
}

} // namespace s5

namespace {

// The step's parameter block for a model on the fused path, with the device addresses pack_all handed out.
void fill_step_params(const s5fxp_model *m, StepParams &sp)
{
    std::memset(&sp, 0, sizeof(sp));
    const FastModel &F = *m->fast;
    sp.n_layers = m->n_layers; sp.H = m->H; sp.P = m->P; sp.hp = fast_shape(m->H, m->P).hp; sp.d_in = m->d_in; sp.d_out = m->d_out;
    auto dense = [](const DenseDev &e, const MfmaWDev &w) {
        StepDense o{};
        o.w = w.w; o.bias_eff = w.bias_eff; o.K = e.K; o.M = e.M; o.inp_bits = e.inp_bits; o.inp_exp = e.inp_exp; o.w_exp = e.w_exp;
        o.out_bits = e.out_bits; o.out_exp = e.out_exp;
        return o;
    };
    sp.enc = dense(m->enc, F.enc);
    sp.dec = dense(m->dec, F.dec);
    int hb = m->enc.out_bits;
    for (int li = 0; li < m->n_layers; ++li) {
        const LayerDev &l = m->layers[li];
        const FastLayer &fl = F.layers[li];
        const s5fxp_ssm_desc &s = l.sd;
        const DenseDev &o = l.out2;
        StepLayer &q = sp.layers[li];
        q.bn = make_bn(l, hb, DynExp{0, nullptr}, nullptr);
        q.bproj = fl.bproj.w; q.cre = fl.cre.w; q.cim = fl.cim.w; q.out2 = fl.out2.w;
        q.o2_bias_eff = fl.out2.bias_eff; q.Dpad = fl.Dpad; q.a_re = l.a_re; q.a_im = l.a_im;
        q.rs_bre = s.u_exp + s.B_re_exp - s.Bu_re_exp; q.rs_bim = s.u_exp + s.B_im_exp - s.Bu_im_exp;
        q.bre_bits = s.Bu_re_bits; q.bim_bits = s.Bu_im_bits; q.sh_re = s.Bu_re_exp - s.x_re_exp; q.sh_im = s.Bu_im_exp - s.x_im_exp;
        q.ea_re = s.A_re_exp; q.ea_im = s.A_im_exp;
        q.rs_cre = s.x_re_exp + s.C_re_exp - s.y_exp; q.rs_cim = s.x_im_exp + s.C_im_exp - s.y_exp;
        q.rs_d = s.D_exp + s.u_exp - s.y_exp; q.y_bits = s.y_bits; q.y_exp = s.y_exp;
        q.o2_conv = (s.y_bits > o.inp_bits || s.y_exp > o.inp_exp) ? 1 : 0; q.o2_inp_bits = o.inp_bits; q.o2_inp_exp = o.inp_exp;
        q.rs_o2 = (q.o2_conv ? o.inp_exp : s.y_exp) + o.w_exp - o.out_exp; // checked per call (step_entry)
        q.o2_out_bits = o.out_bits; q.o2_out_exp = o.out_exp; q.sig_x = l.sig_x; q.sig_y = l.sig_y;
        std::memcpy(q.lut, l.lut, sizeof(q.lut));
        q.l_bits = l.l_bits; q.l_exp = l.l_exp; q.r_bits = l.r_bits; q.r_exp = l.r_exp; q.res_bits = l.res_bits; q.res_exp = l.res_exp;
        q.rs_gate = l.l_exp + l.r_exp - l.res_exp;
        hb = l.res_bits;
    }
}

// What both step entries check before the device is touched: arguments, then the model, then the static shifts.
int step_checks(const s5fxp_model *m, const void *x, int x_bits, int x_exp, int G, int B, int L, void *y, int32_t *status, bool f32)
{
    if (!m || !x || !y || !status || G < 1 || B < 1 || L < 1 || (int64_t)B * L > STEP_MAX_ROWS || x_bits < 1 || x_bits > 32)
        return S5FXP_EBADARG;
    if (f32 && (x_exp < 0 || x_exp > 31)) return S5FXP_EBADARG;
    if (!m->fast || !m->fast->step) return S5FXP_EUNSUPPORTED;
    if (f32 && (m->dec.out_exp < 0 || m->dec.out_exp > 31)) return S5FXP_EUNSUPPORTED; // the range s5fxp_to_float takes
    // the static shifts a batch forward checks while it enqueues (encoder, out2)
    const DenseDev &e = m->enc;
    const bool conv = x_bits > e.inp_bits || x_exp > e.inp_exp;
    if (!shift_ok((conv ? e.inp_exp : x_exp) + e.w_exp - e.out_exp)) return S5FXP_ENEGSHIFT;
    for (int li = 0; li < m->n_layers; ++li) {
        const s5fxp_ssm_desc &s = m->layers[li].sd;
        const DenseDev &o = m->layers[li].out2;
        const bool c2 = s.y_bits > o.inp_bits || s.y_exp > o.inp_exp;
        if (!shift_ok((c2 ? o.inp_exp : s.y_exp) + o.w_exp - o.out_exp)) return S5FXP_ENEGSHIFT;
    }
    return S5FXP_OK;
}

// Threads of a workgroup for G groups with `smem` bytes of dynamic LDS each.  Workgroups of one CU: eight waves by registers,
// 160 KB of LDS
int step_threads(int G, size_t smem)
{
    const size_t fit = (160 * 1024) / (smem + STEP_STATIC_LDS);
    if (G <= STEP_CUS || fit < 2) return 512;
    if (G <= 2 * STEP_CUS || fit < 4) return 256;
    return 128;
}

// One launch of G workgroups with `smem` bytes of dynamic LDS each, on the instantiation step_threads chooses.  What the step,
// the ragged step and the clip entries share behind their argument checks.
template <class Args>
int step_launch(int G, size_t smem, const Args &a, void (*k512)(Args), void (*k256)(Args), void (*k128)(Args), void *stream)
{
    const int threads = step_threads(G, smem);
    void (*kernel)(Args) = threads == 512 ? k512 : (threads == 256 ? k256 : k128);
    if (smem > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL(kernel, dim3((unsigned)G), dim3((unsigned)threads), smem, S(stream), a);
    return launch_rc();
}

// The largest exponent op k of a layer can take: its result bits - 1 (intbits >= 0); -1: the layer has no such op
int exp_max_of(const s5fxp_model *m, int layer, int k)
{
    if (!m || layer < 0 || layer >= m->n_layers || k < 0 || k > 4) return -1;
    const LayerDev &l = m->layers[layer];
    const BnArgs bn = make_bn(l, layer ? m->layers[layer - 1].res_bits : m->enc.out_bits, DynExp{0, nullptr}, nullptr);
    if ((k == 2 && !l.scale) || (k == 3 && !l.nbias)) return -1;
    const int bits[5] = {bn.b1, bn.b2, bn.b3, bn.b4, l.res_bits};
    return bits[k] - 1;
}

// What the host can say about a set of stated exponents (include/s5fxp.h s5fxp_model_exps_check): with every exponent
// stated, every shift of the forward is static.
int exps_check(const s5fxp_model *m, const int32_t *e)
{
    if (!m || !e) return S5FXP_EBADARG;
    if (!m->fast || !m->fast->step || m->n_layers > PIN_MAX_LAYERS) return S5FXP_EUNSUPPORTED;
    for (int li = 0; li < m->n_layers; ++li)
        for (int k = 0; k < 5; ++k) {
            const int mx = exp_max_of(m, li, k);
            if (mx >= 0 && (e[5 * li + k] < 0 || e[5 * li + k] > mx)) return S5FXP_EBADARG;
        }
    // finalize_add_cb's test: both operand shifts and the result's shift
    auto add_ok = [](int eo, int xe, int ye) {
        const int ea = xe > ye ? xe : ye, post = eo - ea;
        return ea - xe <= 31 && ea - ye <= 31 && post <= 31 && post >= -31;
    };
    auto dist_ok = [](int a, int b) { return shift_ok(a > b ? a - b : b - a); }; // the two shifts of a change_cfg
    int hb = m->enc.out_bits, he = m->enc.out_exp;
    for (int li = 0; li < m->n_layers; ++li) {
        const LayerDev &l = m->layers[li];
        const int32_t *pe = e + 5 * li;
        if (!add_ok(pe[0], he, l.nd.mean_exp)) return S5FXP_ENEGSHIFT;
        if (!shift_ok(pe[0] + l.nd.invsq_var_exp - pe[1])) return S5FXP_ENEGSHIFT;
        int be = pe[1];
        if (l.scale) {
            if (!shift_ok(be + l.nd.scale_exp - pe[2])) return S5FXP_ENEGSHIFT;
            be = pe[2];
        }
        if (l.nbias) {
            if (!add_ok(pe[3], be, l.nd.bias_exp)) return S5FXP_ENEGSHIFT;
            be = pe[3];
        }
        if (!dist_ok(be, l.sd.u_exp)) return S5FXP_ENEGSHIFT; // bn_chain's change_cfg to the SSM input
        if (!add_ok(pe[4], l.res_exp, he)) return S5FXP_ENEGSHIFT;
        hb = l.res_bits;
        he = pe[4];
    }
    const DenseDev &d = m->dec;
    const bool conv = hb > d.inp_bits || he > d.inp_exp;
    if (conv && !dist_ok(he, d.inp_exp)) return S5FXP_ENEGSHIFT;
    if (!shift_ok((conv ? d.inp_exp : he) + d.w_exp - d.out_exp)) return S5FXP_ENEGSHIFT;
    return S5FXP_OK;
}

// The kernel-argument copy of a checked host array
PinExps pin_exps(const s5fxp_model *m, const int32_t *e)
{
    PinExps p{};
    std::memcpy(p.e, e, sizeof(int32_t) * 5 * (size_t)m->n_layers);
    return p;
}

// exps == nullptr: the entry as it always was; pinned: the _at form, which refuses a null exps
int step_entry(const s5fxp_model *m, const void *x, int x_bits, int x_exp, int G, int B, int L, void *y, const int32_t *state_in,
               int32_t *state_out, int32_t *status, void *stream, bool f32, bool pinned = false, const int32_t *exps = nullptr)
{
    if (pinned && !exps) return S5FXP_EBADARG;
    if (const int rc = step_checks(m, x, x_bits, x_exp, G, B, L, y, status, f32)) return rc;
    if (pinned)
        if (const int rc = exps_check(m, exps)) return rc;
    const size_t smem = step_lds(B * L, m->H, m->P, fast_shape(m->H, m->P).hp, m->d_in).total;
    StepArgs a{};
    a.sp = m->fast->step; a.x = x; a.y = y; a.state_in = state_in; a.state_out = state_out; a.status = status;
    a.B = B; a.L = L; a.x_bits = x_bits; a.x_exp = x_exp; a.f32 = f32 ? 1 : 0;
    if (pinned) {
        StepPinArgs pa{a, pin_exps(m, exps)};
        return step_launch(G, smem, pa, k_model_step_at<512>, k_model_step_at<256>, k_model_step_at<128>, stream);
    }
    return step_launch(G, smem, a, k_model_step<512>, k_model_step<256>, k_model_step<128>, stream);
}

// The ragged form: the same checks at (B, Lmax), the dynamic LDS of B * Lmax rows, the same rule on n for the workgroup size.
int step_ragged_entry(const s5fxp_model *m, const void *x, int x_bits, int x_exp, int n, int B, int Lmax, void *y,
                      const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, void *stream, bool f32,
                      bool pinned = false, const int32_t *exps = nullptr)
{
    if (!desc || !state || n_slots < 1 || (pinned && !exps)) return S5FXP_EBADARG;
    if (const int rc = step_checks(m, x, x_bits, x_exp, n, B, Lmax, y, status, f32)) return rc;
    if (pinned)
        if (const int rc = exps_check(m, exps)) return rc;
    const size_t smem = step_lds(B * Lmax, m->H, m->P, fast_shape(m->H, m->P).hp, m->d_in).total;
    StepRaggedArgs a{};
    a.sp = m->fast->step; a.x = x; a.y = y; a.desc = desc; a.state = state; a.status = status;
    a.B = B; a.Lmax = Lmax; a.x_bits = x_bits; a.x_exp = x_exp; a.f32 = f32 ? 1 : 0;
    if (pinned) {
        StepRaggedPinArgs pa{a, pin_exps(m, exps)};
        return step_launch(n, smem, pa, k_model_step_ragged_at<512>, k_model_step_ragged_at<256>, k_model_step_ragged_at<128>, stream);
    }
    return step_launch(n, smem, a, k_model_step_ragged<512>, k_model_step_ragged<256>, k_model_step_ragged<128>, stream);
}

} // namespace

extern "C" int s5fxp_model_step_ok(const s5fxp_model *m, int B, int L)
{
    if (!m || B < 1 || L < 1) return -1;
    return m->fast && m->fast->step && (int64_t)B * L <= STEP_MAX_ROWS ? 1 : 0;
}

extern "C" int s5fxp_model_step(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int G, int B, int L, int32_t *y,
                                const int32_t *state_in, int32_t *state_out, int32_t *status, void *stream)
{
    return step_entry(m, x, x_bits, x_exp, G, B, L, y, state_in, state_out, status, stream, false);
}

extern "C" int s5fxp_model_step_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int G, int B, int L, float *y,
                                    const int32_t *state_in, int32_t *state_out, int32_t *status, void *stream)
{
    return step_entry(m, x, x_bits, x_exp, G, B, L, y, state_in, state_out, status, stream, true);
}

extern "C" int s5fxp_model_step_ragged(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int B, int Lmax, int32_t *y,
                                       const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, void *stream)
{
    return step_ragged_entry(m, x, x_bits, x_exp, n, B, Lmax, y, desc, state, n_slots, status, stream, false);
}

extern "C" int s5fxp_model_step_ragged_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int B, int Lmax, float *y,
                                           const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, void *stream)
{
    return step_ragged_entry(m, x, x_bits, x_exp, n, B, Lmax, y, desc, state, n_slots, status, stream, true);
}

// ---- the same four entries at stated exponents, and what the host can say about a set of them (include/s5fxp.h)
extern "C" int s5fxp_model_exp_max(const s5fxp_model *m, int layer, int k) { return exp_max_of(m, layer, k); }

extern "C" int s5fxp_model_exps_check(const s5fxp_model *m, const int32_t *exps_host) { return exps_check(m, exps_host); }

extern "C" int s5fxp_model_step_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int G, int B, int L, int32_t *y,
                                   const int32_t *state_in, int32_t *state_out, int32_t *status, const int32_t *exps, void *stream)
{
    return step_entry(m, x, x_bits, x_exp, G, B, L, y, state_in, state_out, status, stream, false, true, exps);
}

extern "C" int s5fxp_model_step_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int G, int B, int L, float *y,
                                       const int32_t *state_in, int32_t *state_out, int32_t *status, const int32_t *exps, void *stream)
{
    return step_entry(m, x, x_bits, x_exp, G, B, L, y, state_in, state_out, status, stream, true, true, exps);
}

extern "C" int s5fxp_model_step_ragged_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int B, int Lmax,
                                          int32_t *y, const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status,
                                          const int32_t *exps, void *stream)
{
    return step_ragged_entry(m, x, x_bits, x_exp, n, B, Lmax, y, desc, state, n_slots, status, stream, false, true, exps);
}

extern "C" int s5fxp_model_step_ragged_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int B, int Lmax,
                                              float *y, const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status,
                                              const int32_t *exps, void *stream)
{
    return step_ragged_entry(m, x, x_bits, x_exp, n, B, Lmax, y, desc, state, n_slots, status, stream, true, true, exps);
}

// Host-only validation of a descriptor array (include/s5fxp.h): the kernels trust what they read.
extern "C" int s5fxp_push_desc_check(const s5fxp_push_desc *d, int n, int n_slots, int Lmax, int cmax, int audio)
{
    if (!d || n < 1 || n_slots < 1 || Lmax < 0) return S5FXP_EBADARG;
    if (audio && (cmax < 1 || cmax > S5FXP_STREAM_MAX_HOPS)) return S5FXP_EBADARG;
    const int known = S5FXP_PUSH_FRESH | S5FXP_PUSH_ZEROS | S5FXP_PUSH_FINAL;
    std::vector<bool> seen((size_t)n_slots, false);
    bool short_final = false;
    for (int e = 0; e < n; ++e) {
        const s5fxp_push_desc &p = d[e];
        if (p.slot < 0 || p.slot >= n_slots || seen[(size_t)p.slot]) return S5FXP_EBADARG;
        seen[(size_t)p.slot] = true;
        if (p.rows < 0 || p.rows > Lmax || (p.flags & ~known) || p.reserved[0] || p.reserved[1] || p.reserved[2]) return S5FXP_EBADARG;
        if (!audio) continue;
        if (p.hops < 1 || p.hops > cmax || p.h4 < 0 || p.h4 > 4) return S5FXP_EBADARG;
        if ((p.flags & S5FXP_PUSH_FRESH) && p.h4 != 0) return S5FXP_EBADARG;
        if (p.rows != p.hops - (p.h4 == 0 ? 1 : 0)) return S5FXP_EBADARG;
        if ((p.flags & S5FXP_PUSH_FINAL) && p.h4 < 4) short_final = true;
    }
    return short_final ? S5FXP_EUNSUPPORTED : S5FXP_OK;
}
