// s5fxp_fast.hpp -- host side of the int8-MFMA forward (included by s5fxp_api.hip after Packer,
// s5fxp_model, WsLayout-independent helpers).  Packs the weights for mfma_proj.hpp and enqueues the
// w8a16 fast path:  encoder -> [BN maxima -> B proj -> recurrence -> C proj -> out2/gate -> residual] x L
// -> decoder, with int16 activations and int32 recurrence streams.
#pragma once
#include "pinned_exps.hpp"

namespace s5 {
struct StepParams; // s5fxp_step.hpp
}

struct MfmaWDev {
    MfmaW w{};
    const int32_t *bias_eff = nullptr; // [Np], bias moved to out_exp (dense layers only)
};

struct FastLayer {
    MfmaWDev bproj, cre, cim, out2;
    MfmaWDev bproj_pair; // the same weights with re / im of a state 16 columns apart inside one 32-column tile
    const int32_t *Dpad = nullptr; // [Np]
    const int32_t *sigtab = nullptr; // [2][7 << sig_x] (mfma_fused.hpp k_cgate_p)
    const int16_t *sigdir = nullptr; // [1 << sigdir_bits] when the sigmoid input has <= 12 bits (DIRECT)
    int sigdir_bits = 0;
    bool bias16 = false; // every out2 bias, moved to out_exp, fits 16 bits (a condition of the gate kernel's PK16 epilogues)
    // Live-state compaction.  A state whose rows of B_bar_re and B_bar_im are all zero (8-bit B_bar with ONE exponent per matrix
    // rounds the rows of slow states away: 43-46 of 64 on the N-DNS recipe at dim_scale 0.5, profiles/r03_sparsity_census.log)
    // receives Bu = 0 at every step, so from a zero carry it stays (0, 0) for ever: asr(A * 0) = 0, the complex ReLU keeps
    // (0, 0), and its column of C multiplies zeros (fxpmodel.py:147-172, :740-763).  When at most half of a layer's states
    // are live, the layer is ALSO packed over c_slots state slots -- the live states in their order, then zero slots -- and
    // forwards that neither trace the states nor carry them in or out run every kernel of the layer on that half: half the
    // bytes of both recurrence streams, half the recurrence waves, half the gate kernel's phase A.  Bit-identical by the
    // argument above (the dropped terms are exact zeros of int32 sums).
    bool compact_ok = false;
    int n_live = 0;
    int c_slots = 0; // state slots of the compacted layer: n_live rounded up to a multiple of 32 (when that is <= P / 2)
    MfmaWDev c_bproj, c_bproj_pair, c_cre, c_cim;
    ScanBounds c_bounds; // the recurrence kernels' exactness bounds over the live states only
    const int32_t *c_a_re = nullptr, *c_a_im = nullptr; // (c_slots) Lambda_bar of the slots (0 for the empty ones)
};

struct FastModel {
    MfmaWDev enc, dec;
    std::vector<FastLayer> layers;
    const s5::StepParams *step = nullptr; // the one-launch step's parameter block, appended to the blob (s5fxp_step.hpp)
};

namespace {

inline const void *put_raw(Packer &p, const void *src, size_t bytes)
{
    const void *d = p.addr();
    if (p.host) std::memcpy(p.host + p.off, src, bytes);
    p.off = (p.off + bytes + 255) & ~(size_t)255;
    return d;
}

inline bool fits_bits(const int32_t *v, size_t n, int bits)
{
    const int32_t hi = (1 << (bits - 1)) - 1, lo = -hi - 1;
    for (size_t i = 0; i < n; ++i)
        if (v[i] < lo || v[i] > hi) return false;
    return true;
}

// The shape class of a fused forward: everything its stages derive from the model's (H, P).  The tile kernels are instantiated
// for the four N-DNS shapes (recipes/ndns.json at dim_scale 0.25, 0.5, 0.75, 1.0): H = 48, 96, 144, 192 on nt = 2, 3, 5, 6
// 32-channel tiles, P = 2 H / 3 states.  48 and 144 leave the last tile half empty: rows stay dense in memory and the kernels
// mask the pad lanes (proj_p.hpp shape_channels).  This is the one place that knows the shapes: the stages take tile counts,
// thread counts and LDS extents from here, and nt_kernel / ks_kernel below turn nt and a layer's ks into template arguments.
struct FastShape {
    int nt = 0;        // 32-channel tiles of H (0: not a fused shape)
    int hp = 0;        // 32 * nt: the extent of the kernels' LDS tables and byte planes
    int bproj_waves;   // waves of k_bproj_p: one per 32-column tile of [B_re | B_im] = 2 P / 32
    int gate_threads;  // k_cgate_p on 64-frame tiles: one wave per (32-frame half, channel tile)
    bool gate32;       // the 32-frame, GBN and UREC forms of the packed-epilogue gate kernel exist (tuned for H = 96 only)
    bool wide;         // H >= 144: half the B projection's workgroups per CU
};
inline FastShape fast_shape(int H, int P)
{
    FastShape s{};
    if (!(H == 48 || H == 96 || H == 144 || H == 192) || 3 * P != 2 * H) return s;
    s.nt = (H + 31) / 32;
    s.hp = 32 * s.nt;
    s.bproj_waves = 2 * P / 32;
    s.gate_threads = 128 * s.nt;
    s.gate32 = s.nt == 3;
    s.wide = s.nt >= 5;
    return s;
}
// kernel(std::integral_constant<int, NT>) for the shape's tile count
template <class Kernel> auto nt_kernel(int nt, Kernel kernel)
{
    return nt == 2 ? kernel(std::integral_constant<int, 2>{}) : nt == 3 ? kernel(std::integral_constant<int, 3>{})
         : nt == 5 ? kernel(std::integral_constant<int, 5>{}) : kernel(std::integral_constant<int, 6>{});
}
// Shapes whose B projection has the row-chain instantiations (proj_p.hpp k_bproj_p<.., ROW>): H = 96, the shape it was measured
// at.  (The other three compile without scratch and to fewer registers than their bn16_x4 kernels as well -- DESIGN.md 4a has
// the table -- but nobody has timed them: they keep the old kernels.)
constexpr bool bproj_row_shape(int nt) { return nt == 3; }

// The MFMA path runs the N-DNS shapes (FastShape) with <= 8-bit weights and <= 16-bit activations; everything else runs
// the generic kernels.
bool fast_eligible(const s5fxp_model_desc *d)
{
    if (d->n_layers < 1) return false;
    const int H = d->encoder.M, K = d->encoder.K, M = d->decoder.M, P = d->layers[0].ssm.P;
    if (!fast_shape(H, P).nt) return false;
    if (K <= 256 || K > 288 || M > 288 || M < 1) return false;
    auto dense16 = [](const s5fxp_dense_desc &e) { return e.inp_bits <= 16 && e.out_bits <= 16 && e.b_bits <= 32; };
    if (!dense16(d->encoder) || d->decoder.inp_bits > 16 || d->decoder.out_bits > 32) return false;
    if (!fits_bits(d->encoder.weight, (size_t)K * H, 8) || !fits_bits(d->decoder.weight, (size_t)H * M, 8)) return false;
    for (int i = 0; i < d->n_layers; ++i) {
        const s5fxp_layer_desc &l = d->layers[i];
        const s5fxp_ssm_desc &s = l.ssm;
        if (s.P != P) return false;
        const s5fxp_norm_desc &n = l.norm;
        if (n.mean_bits > 16 || n.invsq_var_bits > 16 || (n.scale && n.scale_bits > 16) || (n.bias && n.bias_bits > 16))
            return false;
        if (s.u_bits > 16 || s.y_bits > 16 || s.Bu_re_bits > 32 || s.Bu_im_bits > 32) return false;
        if (!dense16(l.out2) || l.l_bits > 16 || l.r_bits > 16 || l.res_bits > 16) return false;
        if (!fits_bits(s.B_re, (size_t)P * H, 8) || !fits_bits(s.B_im, (size_t)P * H, 8) ||
            !fits_bits(s.C_re, (size_t)H * P, 8) || !fits_bits(s.C_im, (size_t)H * P, 8) ||
            !fits_bits(l.out2.weight, (size_t)H * H, 8) || !fits_bits(s.D, (size_t)H, 16))
            return false;
        for (int i8 = 0; i8 < 8; ++i8) // the fused gate kernel keeps two LUT entries per 32-bit word
            if (l.lut[i8] < 0 || l.lut[i8] > 65535) return false;
        if (l.sig_x_exp > 6) return false; // the reference's rule is min(out2.out_exp, 6) (fxpmodel.py:1097-1104); the r table assumes it
    }
    return true;
}

// get(k, ch) -> weight; result rows are channels, padded and strided for conflict-free 16-byte LDS reads
// min_np: rows the consuming kernel loads whatever M is (zero rows beyond M; the per-channel arrays sized by Np follow)
template <class Get>
void pack_mfma(Packer &p, Get get, int K, int M, MfmaWDev &o, int min_np = 0)
{
    const int Kpad = (K + 31) / 32 * 32;
    const int Kp = ((Kpad / 16) % 2 == 0) ? Kpad + 16 : Kpad;
    const int Np = std::max((M + 31) / 32 * 32, min_np);
    std::vector<int8_t> wt((size_t)Np * Kp, 0);
    std::vector<int32_t> cs(Np, 0);
    for (int ch = 0; ch < M; ++ch) {
        uint32_t sum = 0;
        for (int k = 0; k < K; ++k) {
            const int32_t v = get(k, ch);
            wt[(size_t)ch * Kp + k] = (int8_t)v;
            sum += (uint32_t)v;
        }
        cs[ch] = (int32_t)(sum * 128u);
    }
    o.w.wt = reinterpret_cast<const int8_t *>(put_raw(p, wt.data(), wt.size()));
    o.w.cs128 = reinterpret_cast<const int32_t *>(put_raw(p, cs.data(), cs.size() * 4));
    o.w.Kp = Kp;
    o.w.Np = Np;
}

void pack_bias_eff(Packer &p, const s5fxp_dense_desc &e, int Np, MfmaWDev &o)
{
    std::vector<int32_t> b(Np, 0);
    for (int ch = 0; ch < e.M; ++ch) b[ch] = fxp::chexp(e.bias[ch], e.b_bits, e.b_exp, e.out_exp);
    o.bias_eff = reinterpret_cast<const int32_t *>(put_raw(p, b.data(), b.size() * 4));
}

void pack_fast(Packer &p, const s5fxp_model_desc *d, FastModel *f)
{
    FastModel tmp;
    if (!f) f = &tmp;
    f->layers.resize(d->n_layers);
    const s5fxp_dense_desc &e = d->encoder;
    pack_mfma(p, [&](int k, int ch) { return e.weight[(size_t)k * e.M + ch]; }, e.K, e.M, f->enc);
    pack_bias_eff(p, e, f->enc.w.Np, f->enc);
    for (int i = 0; i < d->n_layers; ++i) {
        const s5fxp_layer_desc &l = d->layers[i];
        const s5fxp_ssm_desc &s = l.ssm;
        FastLayer &o = f->layers[i];
        const int H = s.H, P = s.P;
        pack_mfma(p, [&](int k, int ch) { return ch < P ? s.B_re[(size_t)ch * H + k] : s.B_im[(size_t)(ch - P) * H + k]; }, H,
                  2 * P, o.bproj);
        pack_mfma(p, [&](int k, int ch) {
                      const int st = 16 * (ch / 32) + (ch & 15);
                      return (ch & 16) ? s.B_im[(size_t)st * H + k] : s.B_re[(size_t)st * H + k];
                  }, H, 2 * P, o.bproj_pair);
        pack_mfma(p, [&](int k, int ch) { return s.C_re[(size_t)ch * P + k]; }, P, H, o.cre);
        pack_mfma(p, [&](int k, int ch) { return s.C_im[(size_t)ch * P + k]; }, P, H, o.cim);
        pack_mfma(p, [&](int k, int ch) { return l.out2.weight[(size_t)k * l.out2.M + ch]; }, H, H, o.out2);
        pack_bias_eff(p, l.out2, o.out2.w.Np, o.out2);
        o.bias16 = true;
        for (int ch = 0; ch < l.out2.M; ++ch) {
            const int32_t v = fxp::chexp(l.out2.bias[ch], l.out2.b_bits, l.out2.b_exp, l.out2.out_exp);
            o.bias16 = o.bias16 && v >= -32768 && v <= 32767;
        }
        {
            std::vector<int> idx;
            for (int q = 0; q < P; ++q) {
                bool live = false;
                for (int k = 0; k < H && !live; ++k) live = s.B_re[(size_t)q * H + k] != 0 || s.B_im[(size_t)q * H + k] != 0;
                if (live) idx.push_back(q);
            }
            o.n_live = (int)idx.size();
            // the fewest 32-state groups that hold the live states, if that is at most half of the layer's
            const int Pc = o.n_live <= 32 ? 32 : (o.n_live + 31) / 32 * 32;
            o.compact_ok = P % 64 == 0 && Pc <= P / 2;
            o.c_slots = o.compact_ok ? Pc : P;
            if (o.compact_ok) {
                o.c_bounds = scan_bounds(s, idx.data(), o.n_live, Pc, true);
                idx.resize(Pc, -1);
                auto bre = [&](int st, int k) { return idx[st] < 0 ? 0 : s.B_re[(size_t)idx[st] * H + k]; };
                auto bim = [&](int st, int k) { return idx[st] < 0 ? 0 : s.B_im[(size_t)idx[st] * H + k]; };
                pack_mfma(p, [&](int k, int ch) { return ch < Pc ? bre(ch, k) : bim(ch - Pc, k); }, H, 2 * Pc, o.c_bproj);
                pack_mfma(p, [&](int k, int ch) {
                              const int st = 16 * (ch / 32) + (ch & 15);
                              return (ch & 16) ? bim(st, k) : bre(st, k);
                          }, H, 2 * Pc, o.c_bproj_pair);
                pack_mfma(p, [&](int k, int ch) { return idx[k] < 0 ? 0 : s.C_re[(size_t)ch * P + idx[k]]; }, Pc, H, o.c_cre);
                pack_mfma(p, [&](int k, int ch) { return idx[k] < 0 ? 0 : s.C_im[(size_t)ch * P + idx[k]]; }, Pc, H, o.c_cim);
                std::vector<int32_t> ar(Pc, 0), ai(Pc, 0);
                for (int st = 0; st < Pc; ++st)
                    if (idx[st] >= 0) {
                        ar[st] = s.A_re[idx[st]];
                        ai[st] = s.A_im[idx[st]];
                    }
                o.c_a_re = reinterpret_cast<const int32_t *>(put_raw(p, ar.data(), ar.size() * 4));
                o.c_a_im = reinterpret_cast<const int32_t *>(put_raw(p, ai.data(), ai.size() * 4));
            }
        }
        std::vector<int32_t> Dp(o.cre.w.Np, 0);
        for (int h = 0; h < H; ++h) Dp[h] = s.D[h];
        o.Dpad = reinterpret_cast<const int32_t *>(put_raw(p, Dp.data(), Dp.size() * 4));
        // gate operand r = change_cfg(sigmoid(xx)) for every (sign, min(|xx| >> sx, 6), |xx| mod 2^sx): fxpmodel.py:97-144
        // + :1075-1093, the same integer formula as fxp_prims.hpp sigmoid_lut
        const int sx = l.sig_x_exp, S = 1 << sx, sy = l.sig_y_exp;
        std::vector<int32_t> tab((size_t)14 * S);
        for (int pos = 0; pos < 2; ++pos)
            for (int i = 0; i < 7 * S; ++i) {
                const int ind = i >> sx, mu = i & (S - 1);
                const int32_t half = wadd(asr(wmul(S - mu, l.lut[ind]), sx), asr(wmul(mu, l.lut[ind + 1]), sx));
                const int32_t sg = wadd(1 << (sy - 1), pos ? half : wsub(0, half));
                tab[(size_t)pos * 7 * S + i] = chcfg(sg, l.out2.out_bits, sy, l.r_bits, l.r_exp);
            }
        o.sigtab = reinterpret_cast<const int32_t *>(put_raw(p, tab.data(), tab.size() * 4));
        // the sigmoid input is xx = gq >> (out_exp - sx): when that leaves <= 12 bits, r is tabulated over xx itself
        const int nb = l.out2.out_bits - (l.out2.out_exp - sx);
        if (l.out2.out_exp >= sx && nb >= 2 && nb <= SIGDIR_MAX_BITS && l.r_bits <= 16) {
            std::vector<int16_t> dir((size_t)1 << nb);
            for (int i = 0; i < (1 << nb); ++i) {
                const int32_t xx = i - (1 << (nb - 1)), ax = xx < 0 ? -xx : xx;
                const int ind = (ax >> sx) > 6 ? 6 : (ax >> sx), mu = ax & (S - 1);
                const int32_t half = wadd(asr(wmul(S - mu, l.lut[ind]), sx), asr(wmul(mu, l.lut[ind + 1]), sx));
                const int32_t sg = wadd(1 << (sy - 1), xx > 0 ? half : wsub(0, half));
                dir[i] = (int16_t)chcfg(sg, l.out2.out_bits, sy, l.r_bits, l.r_exp);
            }
            o.sigdir = reinterpret_cast<const int16_t *>(put_raw(p, dir.data(), dir.size() * 2));
            o.sigdir_bits = nb;
        }
    }
    const s5fxp_dense_desc &dd = d->decoder;
    // the decoder kernels (proj_p.hpp k_dec_p: six waves x three column tiles) load the weight rows, cs128 and bias_eff of all
    // 288 columns they can serve and mask only the stores: a narrower decoder (d_out = 1 packs 32 rows) is padded with zero
    // rows, or those loads would run up to 28 KB past the packed arrays -- past the end of the blob, where they were appended last
    pack_mfma(p, [&](int k, int ch) { return dd.weight[(size_t)k * dd.M + ch]; }, dd.K, dd.M, f->dec, 288);
    pack_bias_eff(p, dd, f->dec.w.Np, f->dec);
}

struct FastWs {
    // x1: no fused kernel uses it; it stays until a change of the workspace size (s5fxp_workspace_bytes) is wanted
    size_t hA, hB, x1, z, u, bq, xs, dyn, ext, dyn_bytes, total;
    int TB;
};

FastWs fast_ws(const s5fxp_model *m, int B, int L)
{
    FastWs w{};
    w.TB = (int)time_blocks(L, SCAN_DEPTH);
    // the planes' sizes in 128 bits; a layout whose end does not fit a size_t has total == 0 and no meaningful offsets
    const wide_t nh_w = wide_al256((wide_t)B * L * m->H * 2 + 64) + m->cfg.plane_skew; // int16 (+ slack for the 32-byte fragment loads of clamped tail lanes)
    const wide_t ns_w = wide_al256(((wide_t)B * w.TB + SCAN_DEPTH) * m->P * 8 * 4) + m->cfg.plane_skew;
    const size_t dyn_b = (size_t)wide_al256(sizeof(LayerDyn) * (size_t)m->n_layers);
    const size_t ext_b = (size_t)wide_al256(sizeof(float) * 2 * (size_t)m->H * (size_t)m->n_layers * EXT_REPS);
    if (!fit_size(5 * nh_w + 2 * ns_w + dyn_b + ext_b)) return w;
    const size_t nh = (size_t)nh_w, ns = (size_t)ns_w;
    size_t off = 0;
    w.hA = off; off += nh;
    w.hB = off; off += nh;
    w.x1 = off; off += nh;
    w.z = off; off += nh;
    w.u = off; off += nh;
    w.bq = off; off += ns;
    w.xs = off; off += ns;
    // per-layer device state and per-channel extremes: contiguous, zeroed by one memset per forward
    w.dyn = off; off += dyn_b;
    w.ext = off; off += ext_b;
    w.dyn_bytes = off - w.dyn;
    w.total = off;
    return w;
}

// Which recurrence kernel a fused forward with these S5FXP_FWD_* flags runs for layer li.  Codes 1..4 as
// s5fxp_model_recurrence_kernel (include/s5fxp.h); RK_EXACT = the exact 32-bit chain (k_scan_quad32_asm).  Only plan_layer
// calls it: forward_fast launches by the plan, the status words report it, the queries answer from it.
enum { RK_LANE = 0, RK_QUAD32 = 1, RK_QUAD16 = 2, RK_PAIR = 3, RK_PAIRL = 4, RK_EXACT = 5 };
struct Rung {
    bool exact, defer, quad, s16, pair, pairl;
    int code;
};
Rung select_rung(const s5fxp_model *m, int li, int fwd_flags, bool traced, bool compact)
{
    const LayerDev &l = m->layers[li];
    const bool quad_ok = compact ? m->fast->layers[li].c_bounds.quad_ok : l.quad_ok;
    const bool pair_ok = compact ? m->fast->layers[li].c_bounds.pair_ok : l.pair_ok;
    const s5fxp_ssm_desc &s = l.sd;
    Rung r{};
    r.exact = (fwd_flags & S5FXP_FWD_EXACT) != 0;
    r.defer = (fwd_flags & S5FXP_FWD_DEFER_REDO) && !r.exact;
    r.quad = quad_ok && !r.exact;
    const int sh_re = s.Bu_re_exp - s.x_re_exp, sh_im = s.Bu_im_exp - s.x_im_exp;
    // optimistic forwards (the caller repeats with S5FXP_FWD_EXACT if the range check fires) keep both recurrence
    // streams as int16 when every Bu value, shifted to the state exponent, provably fits: half the bytes of the
    // B projection's output, of both sides of the recurrence and of the gate kernel's state input
    r.s16 = r.defer && r.quad && !traced && s.Bu_re_bits - sh_re <= 16 && s.Bu_im_bits - sh_im <= 16;
    // ... and, where the layer's coefficients leave room for Bu in the multiply's addend, the pair kernel (two lanes
    // per state, four instructions per step), fed either from an int16 Bu stream through LDS by a helper wave (default:
    // the HBM bytes of the quad16 path) or from an int32 K stream in global memory (ModelCfg::pair_global)
    r.pair = r.s16 && pair_ok && !m->cfg.no_pair && !(fwd_flags & S5FXP_FWD_NO_PAIR);
    r.pairl = r.pair && !m->cfg.pair_global;
    r.code = r.pairl ? RK_PAIRL : r.pair ? RK_PAIR : r.quad ? (r.s16 ? RK_QUAD16 : RK_QUAD32) : RK_EXACT;
    return r;
}

// State slots a compacted layer keeps in its two recurrence streams, or 0 = all of them: on the two int16 rungs (LDS-fed pair
// kernel, quad16) the padding slots are neither stored nor loaded -- whole state pairs, so that the pair kernel keeps whole
// lane quads (scan_quad.hpp ScanPairLArgs::live_slots; producers k_bproj_p<.., SM = 3 / 1>, consumer k_cgate_p<.., S16>).
int stream_live_slots(const s5fxp_model *m, int li, const Rung &rung, bool compact)
{
    const FastLayer &fl = m->fast->layers[li];
    const bool int16_rung = rung.pairl || (rung.quad && rung.s16 && !rung.pair);
    if (!(compact && int16_rung) || rung.exact || m->cfg.no_live_lanes) return 0;
    int n = 2 * ((fl.n_live + 1) / 2);
    n = n < 2 ? 2 : n;
    return n >= fl.c_slots ? 0 : n;
}

bool fast_bn_ext(const s5fxp_model *m)
{
    // BatchNorm exponents from per-channel extremes need every BN operand to be <= 16 bit with exponents in
    // [0,15] (no int32 wrap -> every stage monotone, mfma_bn.hpp); otherwise the four full reductions run.
    // ModelCfg::no_bn_ext (tests): take the four-reduction path even when the extremes method applies
    bool bn_ext = !m->cfg.no_bn_ext && m->enc.out_bits <= 16 && m->enc.out_exp >= 0 && m->enc.out_exp <= 15;
    for (int li = 0; li < m->n_layers; ++li) {
        const s5fxp_norm_desc &n = m->layers[li].nd;
        auto ok = [](int bits, int e) { return bits <= 16 && e >= 0 && e <= 15; };
        bn_ext = bn_ext && ok(n.mean_bits, n.mean_exp) && ok(n.invsq_var_bits, n.invsq_var_exp) &&
                 (!m->layers[li].scale || ok(n.scale_bits, n.scale_exp)) && (!m->layers[li].nbias || ok(n.bias_bits, n.bias_exp)) &&
                 m->layers[li].res_bits <= 16;
    }
    return bn_ext;
}

// The form of a layer's gate kernel (mfma_fused.hpp k_cgate_p): traced; 64-frame tiles; the packed-epilogue kernel on
// 32-frame tiles with three-wave workgroups; the packed-epilogue kernel that recomputes u (GBN).
enum GateForm { GATE_TRACED, GATE_FT64, GATE_FT32, GATE_GBN };

// Everything a fused forward decides about layer li before it enqueues anything.
struct LayerPlan {
    bool compact;     // live-state compaction (FastLayer): the layer's kernels run on c_slots state slots
    Rung rung;
    int P;            // state slots the layer's kernels run on: m->P, or c_slots when compacted
    int ks;           // P / 32: the KS of k_cgate_p and half the NC of k_bproj_p
    int live_slots;   // state slots the recurrence streams hold, 0 = every one (stream_live_slots)
    int stream_slots; // status word [8 + 8l + 7]
    int32_t bound;    // the recurrence kernel's exactness bound on |state| (pair or quad, over the slots it runs on)
    int32_t xmax;     // the bound the gate kernel checks on every state: <= 32767 (the C projection's 16-bit planes)
    bool direct;      // the sigmoid input has a direct table (FastLayer::sigdir)
    bool pk16;        // packed int16 epilogues of the gate kernel (mfma_fused.hpp PK16)
    bool gate_bn;     // the gate kernel recomputes u (S5FXP_GATE_BN)
    bool gate_urec;   // the 32-frame gate kernel rebuilds u in its tile staging (k_cgate_p<.., UREC>; off: S5FXP_GATE_BN=0)
    bool bproj_row;   // the B projection's phase A runs the same row chain (k_bproj_p<.., ROW>; off: S5FXP_GATE_BN=2)
    bool resid_fold;  // the gate kernel stores the residual add's aligned sum U, its consumer reads that one plane (FusedForward::plan_layers)
    bool resid_lazy;  // ... and between this layer and the next nobody stores the shifted sum: the U plane is the next layer's input
    bool gate_ext;    // ... and the gate kernel gathers the extremes of U itself: the residual pass between the two is its head alone
    GateForm gate;
    const MfmaW *w_bproj, *w_cre, *w_cim; // full or compacted; w_bproj: the pair-ordered packing on the pair rungs
    const int32_t *a_re, *a_im;           // Lambda_bar of the slots
};

LayerPlan plan_layer(const s5fxp_model *m, int li, int fwd_flags, bool traced, bool carry, bool fold)
{
    const LayerDev &l = m->layers[li];
    const FastLayer &fl = m->fast->layers[li];
    const s5fxp_ssm_desc &s = l.sd;
    const FastShape sh = fast_shape(m->H, m->P);
    LayerPlan p{};
    p.compact = fl.compact_ok && !m->cfg.no_compact && !traced && !carry;
    p.rung = select_rung(m, li, fwd_flags, traced, p.compact);
    const Rung &r = p.rung;
    p.P = p.compact ? fl.c_slots : m->P;
    p.ks = p.P / 32;
    // on the int16 rungs a compacted layer keeps only its live slots in the two recurrence streams (whole lane quads = state
    // pairs; scan_quad.hpp ScanPairLArgs::live_slots)
    p.live_slots = stream_live_slots(m, li, r, p.compact);
    p.stream_slots = p.live_slots ? p.live_slots : p.P;
    const ScanBounds &cb = fl.c_bounds;
    p.bound = r.pair ? (p.compact ? cb.pair_xmax : l.pair_xmax) : (p.compact ? cb.quad_xmax : l.quad_xmax);
    p.xmax = 32767;
    if (r.quad) p.xmax = std::min(p.bound, p.xmax); // the pair bound is <= 32766: a saturated int16 state fails the check
    if (r.quad && r.s16 && !r.pair) p.xmax = std::min(p.xmax, 32766); // a saturated int16 state must fail the check
    // packed int16 epilogues of the gate kernel (mfma_fused.hpp PK16): every width they touch is 16, no out2 input conversion
    const bool out2_conv = s.y_bits > l.out2.inp_bits || s.y_exp > l.out2.inp_exp;
    p.direct = r.s16 && fl.sigdir_bits > 0;
    p.pk16 = p.direct && !traced && !m->cfg.no_pk16 && fl.bias16 && s.y_bits == 16 && l.out2.out_bits == 16 && l.res_bits == 16 &&
             l.l_bits == 16 && !out2_conv && l.l_exp - s.y_exp <= 14;
    // ... and on that kernel the SSM input u CAN be recomputed from the layer input instead of travelling through memory (the
    // exponents are the ones this layer's B projection publishes in its prologue).  The first form of it (k_cgate_p<.., GBN>,
    // S5FXP_GATE_BN=1: 64-frame tiles, bn16_x4 in the first epilogue, operands from an LDS table) lost: gate kernel 207 -> 250 us
    // per 8-batch launch, B projection 104 -> 90, 3 % slower overall.  Kept as the record; what ships is gate_urec below.
    p.gate_bn = p.pk16 && fold && sh.gate32 && m->cfg.gate_bn;
    // 32-frame tiles, three-wave workgroups: with the sigmoid table sized exactly FIVE of them fit a CU's LDS and registers --
    // 15 waves instead of the 12 of two six-wave workgroups, for a kernel whose waves wait two thirds of their cycles.  The
    // grid is exactly what is resident at once (5 x 256 CUs): 170 us per 8-batch launch against 190 (tools/ab_cgate_ft32.sh;
    // 1024 or 1536 workgroups: 189 / 209).  (Without PK16 they were tried as well: 39 vs 36 us.)
    p.gate = traced ? GATE_TRACED : p.gate_bn ? GATE_GBN : (sh.gate32 && p.pk16 && !m->cfg.cgate_ft64) ? GATE_FT32 : GATE_FT64;
    // The 32-frame form rebuilds u in its tile staging, where a thread holds whole 16-byte rows of the layer input and no
    // accumulator is live, from operands in eight registers and in 4.5-6 instructions per element chosen by the layer's shifts
    // (mfma_fused.hpp UREC, mfma_bn.hpp bn16_row8): by default wherever the B projection publishes the exponents (fold) and the
    // BatchNorm has no scale / bias stage (those models keep reading u).  -50 MB per layer and batch, +5 % frames/s against the
    // kernels that move u through memory, which S5FXP_GATE_BN=0 restores (profiles/r05_gate_urec_*).
    p.gate_urec = p.gate == GATE_FT32 && fold && !l.scale && !l.nbias && !m->cfg.no_gate_urec;
    // The B projection builds the same u from the same rows, so its phase A runs the same chain (proj_p.hpp k_bproj_p<.., ROW>):
    // every untraced layer whose BatchNorm has no scale / bias stage, at the shapes that have the instantiations (bproj_row_shape).
    // It takes its exponents from its own prologue, so it does not need `fold`.  S5FXP_GATE_BN=2 restores bn16_x4 everywhere.
    p.bproj_row = !traced && bproj_row_shape(sh.nt) && !l.scale && !l.nbias && !m->cfg.no_bproj_row;
    p.w_bproj = r.pair ? &(p.compact ? fl.c_bproj_pair : fl.bproj_pair).w : &(p.compact ? fl.c_bproj : fl.bproj).w;
    p.w_cre = &(p.compact ? fl.c_cre : fl.cre).w;
    p.w_cim = &(p.compact ? fl.c_cim : fl.cim).w;
    p.a_re = p.compact ? fl.c_a_re : l.a_re;
    p.a_im = p.compact ? fl.c_a_im : l.a_im;
    return p;
}

// What s5fxp_model_recurrence_kernel / _xmax report: a plain forward (no traces, no carry) under S5FXP_FWD_DEFER_REDO
LayerPlan plain_plan(const s5fxp_model *m, int li) { return plan_layer(m, li, S5FXP_FWD_DEFER_REDO, false, false, fast_bn_ext(m)); }

// kernel(std::integral_constant<int, KS>) for a layer's KS = state slots / 32: 1 (NT = 2), 2 (NT = 3), 3 (NT = 5) or 4 (NT = 6);
// at NT = 3 and 6 halved or quartered for a compacted layer (the 32 and 96 states of NT = 2 and 5 are never compacted:
// FastLayer::compact_ok).  The one KS helper of the fused path: it instantiates no KS that cannot run.
template <int NT, class Kernel> auto ks_kernel(int ks, Kernel kernel)
{
    if constexpr (NT == 2) return kernel(std::integral_constant<int, 1>{});
    else if constexpr (NT == 5) return kernel(std::integral_constant<int, 3>{});
    else {
        if constexpr (NT == 6)
            if (ks == 4) return kernel(std::integral_constant<int, 4>{});
        return ks == 1 ? kernel(std::integral_constant<int, 1>{}) : kernel(std::integral_constant<int, 2>{});
    }
}
// waves of the B projection for NT channel tiles (FastShape::bproj_waves as a template argument)
template <int NT> constexpr int bproj_waves_of() { return NT == 2 ? 2 : NT == 3 ? 4 : NT == 5 ? 6 : 8; }

// k_bproj_p of an untraced layer: SM = the stream its recurrence rung wants (proj_p.hpp), NC = 2 KS column tiles, ROW = the
// row chain in phase A (LayerPlan::bproj_row; only the shapes of bproj_row_shape have those kernels)
template <int SM, bool ROW = false> auto bproj_kernel(const FastShape &sh, int ks)
{
    return nt_kernel(sh.nt, [&](auto n) {
        constexpr int NT = decltype(n)::value;
        return ks_kernel<NT>(ks, [](auto k) { return k_bproj_p<NT, bproj_waves_of<NT>(), false, SM, 2 * decltype(k)::value, ROW && bproj_row_shape(NT)>; });
    });
}
template <int SM> auto bproj_kernel(const FastShape &sh, int ks, bool row) { return row ? bproj_kernel<SM, true>(sh, ks) : bproj_kernel<SM>(sh, ks); }
// ... and of a traced one (every state slot, int32 stream)
inline auto bproj_traced_kernel(const FastShape &sh)
{
    return nt_kernel(sh.nt, [](auto n) { constexpr int NT = decltype(n)::value; return k_bproj_p<NT, bproj_waves_of<NT>(), true>; });
}

// k_cgate_p<KS, NT, false, S16, DIRECT, FTP, false, PAIR, PK16, GBN, UREC> of an untraced, inexact layer in its gate form: the
// 32-frame (with or without UREC) and GBN forms exist for the packed epilogues (PK16) at H = 96 only (FastShape::gate32)
// (k_cgate_p has two overloads, told apart by the argument block: the pointer type names the one that is meant)
using GateKernel = void (*)(const CGateArgs, GroupOff);
using GateFoldKernel = void (*)(const CGateFoldArgs, GroupOff);
constexpr size_t GATE_FOLD_LDS_5WG = 32000; // LDS bytes per workgroup up to which five 192-thread workgroups share a CU (see gate())
// (k_resid_minmax16 likewise: the storing pass and the read-only one of a lazy layer, mfma_bn.hpp ResidLazyArgs)
using ResidKernel = void (*)(const int16_t *, const int16_t *, int16_t *, int32_t *, int64_t, int, int64_t, int, int, ResidHead, float *, int,
                             int32_t *, GroupOff);
using ResidLazyKernel = void (*)(ResidLazyArgs, GroupOff);
template <bool S16, bool DIR, bool PAIR, bool PK16> GateKernel cgate_kernel(const LayerPlan &p, const FastShape &sh)
{
    return nt_kernel(sh.nt, [&](auto n) -> GateKernel {
        constexpr int NT = decltype(n)::value;
        if constexpr (PK16 && NT == 3) {
            if (p.gate == GATE_FT32 && p.gate_urec)
                return ks_kernel<3>(p.ks, [](auto k) -> GateKernel { return k_cgate_p<decltype(k)::value, 3, false, S16, DIR, 32, false, PAIR, true, false, true>; });
            if (p.gate == GATE_FT32)
                return ks_kernel<3>(p.ks, [](auto k) -> GateKernel { return k_cgate_p<decltype(k)::value, 3, false, S16, DIR, 32, false, PAIR, true>; });
            if (p.gate == GATE_GBN)
                return ks_kernel<3>(p.ks, [](auto k) -> GateKernel { return k_cgate_p<decltype(k)::value, 3, false, S16, DIR, 64, false, PAIR, true, true>; });
        }
        return ks_kernel<NT>(p.ks, [](auto k) -> GateKernel { return k_cgate_p<decltype(k)::value, NT, false, S16, DIR, 64, false, PAIR, PK16>; });
    });
}
// the UREC kernel that stores the aligned sum (mfma_fused.hpp FOLD): gate_urec implies H = 96, PK16 and with it S16 and DIRECT
inline GateFoldKernel gate_fold_kernel(const LayerPlan &p)
{
    if (p.rung.pair)
        return ks_kernel<3>(p.ks, [](auto k) -> GateFoldKernel { return k_cgate_p<decltype(k)::value, 3, false, true, true, 32, false, true, true, false, true>; });
    return ks_kernel<3>(p.ks, [](auto k) -> GateFoldKernel { return k_cgate_p<decltype(k)::value, 3, false, true, true, 32, false, false, true, false, true>; });
}
// ... for the seven (S16, DIRECT, PAIR, PK16) a plan can hold (PK16 needs DIRECT; DIRECT and PAIR need S16)
GateKernel gate_kernel(const LayerPlan &p, const FastShape &sh)
{
    const bool pair = p.rung.pair;
    return p.pk16 && pair   ? cgate_kernel<true, true, true, true>(p, sh)
           : p.pk16         ? cgate_kernel<true, true, false, true>(p, sh)
           : p.direct && pair ? cgate_kernel<true, true, true, false>(p, sh)
           : pair           ? cgate_kernel<true, false, true, false>(p, sh)
           : p.direct       ? cgate_kernel<true, true, false, false>(p, sh)
           : p.rung.s16     ? cgate_kernel<true, false, false, false>(p, sh)
                            : cgate_kernel<false, false, false, false>(p, sh);
}
// the exact gate kernel (k_cgate_p<.., WIDE>): the in-forward re-run and S5FXP_FWD_EXACT; traced: every state slot
inline GateKernel gate_exact_kernel(const LayerPlan &p, const FastShape &sh, bool traced)
{
    return nt_kernel(sh.nt, [&](auto n) -> GateKernel {
        constexpr int NT = decltype(n)::value;
        constexpr int KSF = NT == 2 ? 1 : NT == 3 ? 2 : NT == 5 ? 3 : 4; // all of the shape's states
        if (traced) return k_cgate_p<KSF, NT, true, false, false, 64, true>;
        return ks_kernel<NT>(p.ks, [](auto k) -> GateKernel { return k_cgate_p<decltype(k)::value, NT, false, false, false, 64, true>; });
    });
}
inline GateKernel gate_traced_kernel(const FastShape &sh)
{
    return nt_kernel(sh.nt, [](auto n) -> GateKernel {
        constexpr int NT = decltype(n)::value;
        constexpr int KSF = NT == 2 ? 1 : NT == 3 ? 2 : NT == 5 ? 3 : 4;
        return k_cgate_p<KSF, NT, true>;
    });
}

// Workgroups of a launch over `tiles` tiles, at most `cap` of them (persistent loops over the tiles)
inline unsigned grid_for(int64_t tiles, int64_t cap)
{
    const int64_t per = (tiles + cap - 1) / cap;
    return (unsigned)((tiles + per - 1) / per);
}

// One fused forward: the plan and the stages that enqueue it.
// G > 1: a grouped launch (include/s5fxp.h s5fxp_forward_opts::groups): x, y, workspace, status and the carry arrays hold G
// consecutive copies of what one forward uses; every kernel runs with gridDim.y = G (scan_quad.hpp GroupOff).  The caller
// (s5fxp_model_forward) sends only hook-free, trace-free forwards here with G > 1.
struct FusedForward {
    const s5fxp_model *m;
    const s5fxp_forward_opts *opts;
    const s5fxp_layer_trace *traces;
    int32_t *status;
    hipStream_t st;
    int G, B, L;
    char *ws;
    size_t ws_stride; // bytes between the groups' workspaces (0: this forward's size)
    int io = IO_I32;  // the model boundary (proj_p.hpp): IO_F32 (s5fxp_model_forward_f32) and IO_I16 (s5fxp_model_forward_i16) convert inside
                      // the encoder and the decoder
    // Stated exponents (s5fxp_model_forward_at): 5 * n_layers checked host values (s5fxp_model_exps_check), or
    // nullptr.  A pinned forward runs the plan of the multi-rank mode -- every kernel reads its layer's LayerDyn from memory,
    // none derives it (fold is off) -- without that mode's finalize kernels and exchanges: the head launch (k_clear2_at) has
    // filled every layer's LayerDyn and exponent status words from `exps` before the encoder starts.
    const int32_t *exps = nullptr;
    const bool pinned = exps != nullptr;

    const FastModel &F = *m->fast;
    const ModelCfg &cfg = m->cfg;
    const int H = m->H, fwd_flags = opts ? opts->flags : 0;
    const int64_t N = (int64_t)B * L, NH = N * H;
    const FastShape sh = fast_shape(m->H, m->P);
    const bool exact = (fwd_flags & S5FXP_FWD_EXACT) != 0, defer = (fwd_flags & S5FXP_FWD_DEFER_REDO) && !exact;
    const s5fxp_allreduce_max_fn allreduce = opts && !pinned ? opts->allreduce : nullptr; // (pinned: nothing to exchange)
    const int32_t *state_in = opts ? opts->state_in : nullptr;
    int32_t *state_out = opts ? opts->state_out : nullptr;
    const FastWs w = fast_ws(m, B, L);
    LayerDyn *dyn = reinterpret_cast<LayerDyn *>(ws + w.dyn);
    const int64_t carry_stride = (int64_t)m->n_layers * 2 * B * (m->P ? m->P : 1) * 4;
    const GroupOff go{N * m->d_in * (io == IO_I16 ? 2 : 4), N * m->d_out * (io == IO_I16 ? 2 : 4), (int64_t)(ws_stride ? ws_stride : w.total), 4 * S5FXP_STATUS_WORDS,
                      carry_stride, carry_stride};

    // ---- the plan
    const bool bn_ext = fast_bn_ext(m);
    // single-rank mode folds the two one-workgroup "finalize" kernels of every layer into the residual pass
    // (mfma_bn.hpp k_resid_minmax16); with a multi-rank hook the maxima are exchanged in between, so they stay
    const bool fold = bn_ext && !allreduce && !pinned;
    const std::array<LayerPlan, 15> layer = plan_layers(); // validate: 8 + 8 * n_layers <= S5FXP_STATUS_WORDS
    // the layer whose residual pass rides on the decoder (proj_p.hpp k_dec_p<.., RESID>), or -1
    const int dec_resid = bn_ext && fold && !traces && !cfg.no_dec_resid ? m->n_layers - 1 : -1;
    // workgroups per launch (persistent loops over tiles): tuned per kernel on MI355X (256 CUs); ModelCfg (S5FXP_WGS_* at
    // model creation) overrides them
    // A grouped launch shares the caps between its groups (every workgroup pays its prologue once -- weights into registers,
    // tables into LDS, the exponent derivation -- and G x 512 workgroups of 4 tiles each pay it 4 times as often as 512
    // workgroups of 16 tiles: tools/sweep_groups.sh, +4 % at G = 4), down to a floor that still fills the chip with G groups
    int64_t per_group(int64_t cap, int64_t floor_) const { return G > 1 ? std::max<int64_t>(cap / G, floor_) : cap; }
    // six-wave phase-split kernels (proj_p.hpp, mfma_fused.hpp): 64-frame tiles; the per-layer ones tile each sequence
    const int64_t tiles64 = (N + 63) / 64, seq_tiles64 = (int64_t)B * ((L + 63) / 64);
    const unsigned grid_enc = grid_for(tiles64, per_group(cfg.cap_enc, 64)), grid_dec = grid_for(tiles64, per_group(cfg.cap_dec, 64));
    // the B projection: up to 4 (H <= 96) / 2 (H >= 144) workgroups per CU
    const int64_t cap_bproj = per_group(cfg.cap_bproj, 128);
    const unsigned grid_bproj = grid_for(seq_tiles64, sh.wide ? std::max<int64_t>(cap_bproj / 2, 1) : cap_bproj);
    const unsigned grid_gate = grid_for(seq_tiles64, per_group(cfg.cap_cgate, 64)), grid_gate_exact = grid_for(seq_tiles64, 512);
    const unsigned grid_gate32 = grid_for((int64_t)B * ((L + 31) / 32), std::max<int64_t>(cfg.cap_cgate32 / G, 1));
    // residual / extremes pass: a workgroup owns rm_span consecutive frames, a multiple of its 4 x R frame step
    const int64_t rm_step = 4 * (RESID_THREADS / (H / 8)), rm_iters = (N + rm_step - 1) / rm_step;
    // (the kernel addresses a workgroup's span with 32-bit byte offsets: at most 2^31 bytes of one (N,H) int16 tensor per workgroup)
    const int64_t rm_per = std::min(std::max<int64_t>(1, ((int64_t(1) << 31) / (2 * H)) / rm_step),
                                    (rm_iters + per_group(cfg.cap_resid, 64) - 1) / per_group(cfg.cap_resid, 64));
    const int64_t rm_span = rm_per * rm_step;
    const unsigned rm_grid = (unsigned)((rm_iters + rm_per - 1) / rm_per);

    // the current layer input: its plane, the other one of the ping-pong pair, its bits and (device) exponent
    int16_t *h = I16(w.hA), *hn = I16(w.hB);
    // the plane the gate kernel writes (z, or the aligned sum U).  Behind a lazy layer (LayerPlan::resid_lazy) that plane IS the
    // next layer input -- uint16, shifted on load with *h_lazy, the LayerDyn of the layer that produced it -- and the plane
    // that held the layer input until then, dead once the gate kernel has run, takes the next gate kernel's output
    int16_t *zp = I16(w.z);
    const LayerDyn *h_lazy = nullptr;
    int hb = m->enc.out_bits;
    DynExp he{m->enc.out_exp, nullptr};

    std::array<LayerPlan, 15> plan_layers() const
    {
        std::array<LayerPlan, 15> p{};
        for (int li = 0; li < m->n_layers; ++li) {
            p[li] = plan_layer(m, li, fwd_flags, traces != nullptr, state_in || state_out, fold);
            // resid_fold: of the residual add h = relu(z + skip), a compute_best op, only the result shift waits
            // for the batch-wide maximum; the operand shifts follow from res_exp and the layer input's exponent, which the gate
            // kernel reads anyway.  Where it rebuilds u in its staging (gate_urec) it holds z(t) and skip(t) side by side when z
            // leaves the tile, and stores U = max(sat16(z << shx) + sat16(skip << shy), 0) in z's place (mfma_bn.hpp SumU16): a
            // uint16 that loses nothing when both operands are 16 bit and skip >= 0 (the layer input is a ReLU output).  The
            // residual pass (k_resid_minmax16<true, true>) or the decoder's fused residual then read ONE plane and shift it.
            // Conditions: a deferred forward (the in-forward exact re-run would store a plain z), no traces and no multi-rank
            // hook (both implied by gate_urec: pk16 needs !traced, fold needs !allreduce), 0 <= res_exp <= 16 (then post <= 15,
            // so a negative sum cannot wrap to a positive value in the result shift, and the operand shifts are <= 16, so
            // the reference's int32 shift of a 16-bit operand does not wrap either).  A model created with S5FXP_MODEL_NO_RESID_FOLD keeps the
            // two-plane kernels (the A/B partner).
            const int in_bits = li ? m->layers[li - 1].res_bits : m->enc.out_bits;
            p[li].resid_fold = p[li].gate_urec && defer && !traces && fold && m->layers[li].res_bits == 16 && in_bits == 16 &&
                               m->layers[li].res_exp >= 0 && m->layers[li].res_exp <= 16 && !(m->flags & S5FXP_MODEL_NO_RESID_FOLD);
        }
        // resid_lazy: U -> h is one shift and one clip (mfma_bn.hpp resolve_u16), and only the shift is late --
        // the residual pass publishes it in LayerDyn::res before either reader of h starts.  So between two layers that both
        // fold, the pass stores nothing (it still gathers the extremes: the map is monotone, the extremes of h are the resolved
        // extremes of U) and the next layer's B projection and gate kernel shift U as they load it.  The next layer must be one
        // whose kernels can: the MFMA B projection that derives its exponents from the extremes and the gate kernel that
        // rebuilds u -- what gives it its own resid_fold.  The last layer's U goes to the decoder as before.  A model created
        // with S5FXP_MODEL_NO_RESID_LAZY keeps the storing pass (the A/B partner).
        for (int li = 0; li + 1 < m->n_layers; ++li)
            p[li].resid_lazy = p[li].resid_fold && p[li + 1].resid_fold && !(m->flags & S5FXP_MODEL_NO_RESID_LAZY);
        // gate_ext: the lazy pass reads the U plane only for its per-channel extremes, and the gate kernel held
        // every U it stored in registers a moment earlier.  So the gate kernel keeps packed running extremes and leaves them in
        // the next layer's block of extremes, in U units (mfma_fused.hpp CGateFoldArgs::ext_next); the pass shrinks to one
        // workgroup per group that derives the result shift as before and resolves the block in place (mfma_bn.hpp
        // ResidLazyArgs::head_only).  The block is zeroed by clear_status() at the head of the forward, ahead of every gate
        // kernel.  A model created with S5FXP_MODEL_NO_GATE_EXT keeps the reading pass (the A/B partner).
        for (int li = 0; li + 1 < m->n_layers; ++li) p[li].gate_ext = p[li].resid_lazy && !(m->flags & S5FXP_MODEL_NO_GATE_EXT);
        return p;
    }
    int16_t *I16(size_t off) const { return reinterpret_cast<int16_t *>(ws + off); }
    int32_t *I32(size_t off) const { return reinterpret_cast<int32_t *>(ws + off); }
    const s5fxp_layer_trace *trace(int li) const { return traces ? &traces[li] : nullptr; }
    float *ext(int li) const { return reinterpret_cast<float *>(ws + w.ext) + (size_t)li * 2 * H * EXT_REPS; }
    int32_t *status_exps(int li) const { return status + 8 + 8 * li; }
    // one event of the pair s5fxp_forward_opts::scan_events / gate_events attaches to layer li's launch (measurement only)
    static hipEvent_t event(void **evs, int li, int k) { return evs ? (hipEvent_t)evs[2 * li + k] : nullptr; }

    // Every launch with gridDim.y = G: the dynamic-LDS attribute where a kernel needs more than the default 64 KB (the
    // dim_scale 1.0 tiles; a host-side table update), and the kernel's own start / stop time stamps when a pair of events is
    // attached (what rocprofv3's kernel trace reports), not events recorded around it
    template <class K, class... A>
    void launch(K kernel, unsigned grid, unsigned block, size_t smem, hipEvent_t ev0, hipEvent_t ev1, const A &...args) const
    {
        if (smem > 65536)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (ev0 && ev1) hipExtLaunchKernelGGL(kernel, dim3(grid, G), dim3(block), smem, st, ev0, ev1, 0, args..., go);
        else hipLaunchKernelGGL(kernel, dim3(grid, G), dim3(block), smem, st, args..., go);
    }

    // ModelCfg::debug_sync: synchronise and check for launch / execution errors after every stage (names the stage that
    // failed); off by default -- a forward has no host synchronisation, and launch errors are collected once at the end
    bool stage_ok(const char *what, int li) const
    {
        if (!cfg.debug_sync) return true;
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) std::fprintf(stderr, "[s5fxp] %s (layer %d): %s\n", what, li, hipGetErrorString(e));
        return e == hipSuccess;
    }

    // the status words start from zero except what the host already knows: which path runs ([2]) and, per layer, the
    // recurrence kernel ([8 + 8l + 5]), the state slots ([6]) and the slots the streams hold ([7]); the per-layer device state
    // and extremes are zeroed by the same launch
    void clear_status() const
    {
        StatusInit si{};
        si.path = S5FXP_PATH_FUSED;
        for (int li = 0; li < m->n_layers; ++li) {
            si.rk[li] = layer[li].rung.code;
            si.slots[li] = layer[li].P;
            si.stream[li] = layer[li].stream_slots;
        }
        if (pinned) {
            // the same words, every layer's LayerDyn and its exponent words (pinned_exps.hpp); the block of extremes stays as it is
            static_assert(PIN_STATUS_WORDS == S5FXP_STATUS_WORDS, "k_clear2_at builds the status block in LDS");
            PinHeadArgs pa{};
            pa.si = si;
            std::memcpy(pa.pin.e, exps, sizeof(int32_t) * 5 * (size_t)m->n_layers);
            for (int li = 0; li < m->n_layers; ++li) {
                pa.bn[li] = make_bn(m->layers[li], li ? m->layers[li - 1].res_bits : m->enc.out_bits, DynExp{0, nullptr}, nullptr);
                pa.res_exp[li] = m->layers[li].res_exp;
            }
            pa.enc_exp = m->enc.out_exp; pa.n_layers = m->n_layers;
            launch(k_clear2_at, 1, 256, 0, nullptr, nullptr, status, dyn, pa);
            return;
        }
        launch(k_clear2, 8, 256, 0, nullptr, nullptr, status, (int)S5FXP_STATUS_WORDS, reinterpret_cast<int32_t *>(dyn),
               (int)(w.dyn_bytes / 4), si, m->n_layers);
    }

    // ---- encoder + ReLU
    int encoder(const void *x, int x_bits, int x_exp) const
    {
        const DenseDev &e = m->enc;
        EncArgs a{};
        // IO_F32: float rows, read as their bits by k_enc_pf; IO_I16: int16 rows, read by k_enc_ps
        a.x = reinterpret_cast<const int32_t *>(x); a.y = h; a.w = F.enc.w; a.bias_eff = F.enc.bias_eff; a.N = N; a.K = e.K; a.M = e.M;
        a.xb = x_bits; a.xe = x_exp; a.inp_bits = e.inp_bits; a.inp_exp = e.inp_exp;
        a.conv = (x_bits > e.inp_bits || x_exp > e.inp_exp) ? 1 : 0;
        a.rs = (a.conv ? e.inp_exp : x_exp) + e.w_exp - e.out_exp;
        if (!shift_ok(a.rs)) return S5FXP_ENEGSHIFT;
        a.out_bits = e.out_bits; a.status = status;
        const size_t smem = 4 * (size_t)sh.hp * 4 + 2 * 64 * 304; // cs128 + bias_eff + byte planes + extremes
        // the extremes of the output (layer 0's BatchNorm operand) are gathered on the way; single-rank mode also
        // lets the last workgroup derive layer 0's BatchNorm exponents (mfma_bn.hpp ResidTail)
        float *ext0 = bn_ext && !pinned ? ext(0) : nullptr; // (pinned: nobody derives an exponent from them)
        const int ext_reps = (ext0 && !allreduce) ? EXT_REPS : 1; // the consumer (k_bproj_p's prologue) folds the replicas
        auto kernel = nt_kernel(sh.nt, [&](auto n) { return io == IO_F32 ? k_enc_pf<decltype(n)::value> : io == IO_I16 ? k_enc_ps<decltype(n)::value> : k_enc_p<decltype(n)::value>; });
        launch(kernel, grid_enc, 384, smem, nullptr, nullptr, a, ext0, ext_reps);
        return S5FXP_OK;
    }

    // ---- BatchNorm exponents of layer li: from the extremes the previous stage left (layer 0: the encoder; later layers:
    // the previous layer's residual pass), or the four full reductions
    int bn_exponents(int li, const BnArgs &bn) const
    {
        LayerDyn *d = dyn + li;
        if (pinned) return S5FXP_OK; // the head launch wrote them
        if (!bn_ext) {
            const unsigned rg = std::min(ew_grid(NH / 4), 2048u);
            return bn_exponent_ops([&](auto op) {
                hipLaunchKernelGGL(k_bn_reduce16<decltype(op)::value>, dim3(rg), dim3(256), 0, st, bn, (const int16_t *)h, NH, H, d);
            }, bn, d, status, status_exps(li), opts, st);
        }
        if (!fold) { // (fold: the B projection's prologue derives them)
            // mode A: the extremes (positive floats) are what the ranks exchange -- one MAX over 2H values
            if (allreduce && allreduce(opts->allreduce_ctx, ext(li), 2 * H, (void *)st)) return S5FXP_EHIP;
            hipLaunchKernelGGL(k_bn_finalize_mm, dim3(1), dim3(256), 0, st, bn, (const float *)ext(li), H, d, status, status_exps(li));
        }
        return S5FXP_OK;
    }

    // ---- B projection -> scan-native stream (+ u for the gate kernel)
    void bproj(int li, const BnArgs &bn) const
    {
        const LayerPlan &p = layer[li];
        const s5fxp_ssm_desc &s = m->layers[li].sd;
        const s5fxp_layer_trace *tr = trace(li);
        BprojM2Args a{};
        a.bn = bn; a.x = h; a.w = *p.w_bproj; a.bq = I32(w.bq); a.u = I16(w.u);
        a.tr_bu_re = tr ? tr->Bu_re : nullptr; a.tr_bu_im = tr ? tr->Bu_im : nullptr;
        a.tr_pre_s5 = tr ? tr->pre_s5 : nullptr; a.tr_u = tr ? tr->u : nullptr;
        a.N = N; a.L = L; a.TB = w.TB; a.H = H; a.P = p.P;
        a.rs_re = s.u_exp + s.B_re_exp - s.Bu_re_exp; a.rs_im = s.u_exp + s.B_im_exp - s.Bu_im_exp;
        a.bre_bits = s.Bu_re_bits; a.bim_bits = s.Bu_im_bits; a.sh_re = s.Bu_re_exp - s.x_re_exp; a.sh_im = s.Bu_im_exp - s.x_im_exp;
        a.k_re = 65536 - (1 << (16 - s.A_re_exp));
        a.live_slots = p.live_slots;
        // u is not stored when the gate kernel rebuilds it -- and nothing else reads it: the in-forward exact re-run
        // (k_cgate_p<.., WIDE>, enqueued when !defer) takes u from memory.  (Today pk16 implies the int16 rungs and those imply
        // defer; the rule is stated here so that it does not rest on that.)
        a.no_u = (p.gate_bn || p.gate_urec) && defer ? 1 : 0;
        if (fold) {
            a.ext = ext(li);
            a.ext_reps = EXT_REPS; a.status = status; a.status_exps = status_exps(li);
        }
        a.lazy = h_lazy;
        a.t_lo = 0; a.t_len = L;
        const size_t smem = 16 * (size_t)sh.hp + 4 * 64 * (size_t)(sh.hp + 16); // BN operands + double-buffered byte planes
        // phase-split kernel (proj_p.hpp), one wave per 32-column tile of [B_re | B_im]; SM: the stream the recurrence rung
        // wants; a compacted layer has fewer column tiles (NC)
        const Rung &r = p.rung;
        auto kernel = tr ? bproj_traced_kernel(sh)
                         : r.pairl ? bproj_kernel<3>(sh, p.ks, p.bproj_row) : r.pair ? bproj_kernel<2>(sh, p.ks, p.bproj_row)
                         : r.s16 ? bproj_kernel<1>(sh, p.ks, p.bproj_row) : bproj_kernel<0>(sh, p.ks, p.bproj_row);
        launch(kernel, grid_bproj, 64 * sh.bproj_waves, smem, nullptr, nullptr, a);
    }
    // the recurrence's arguments on the quad layout (the fast quad kernels, the exact chain and its gated re-run)
    ScanQuadArgs quad_args(int li, const int32_t *run_if) const
    {
        const LayerPlan &p = layer[li];
        const s5fxp_ssm_desc &s = m->layers[li].sd;
        ScanQuadArgs q{};
        q.bq = I32(w.bq); q.xs = I32(w.xs); q.a_re = p.a_re; q.a_im = p.a_im; q.B = B; q.TB = w.TB; q.P = p.P;
        q.ea_re = s.A_re_exp; q.ea_im = s.A_im_exp; q.run_if = run_if; q.x0_re = x0(li, 0); q.x0_im = x0(li, 1);
        q.live_slots = p.live_slots;
        if (!run_if) q.cc = carry_check(li); // the fast kernels; the gated exact chain takes a carry of any width
        return q;
    }
    // the fast recurrence kernels' range check of the carry in (scan_quad.hpp CarryCheck): the bound and the bits the gate
    // kernel uses for the stored states.  Without state_in, and on the exact rung, there is nothing to check.
    CarryCheck carry_check(int li) const
    {
        const LayerPlan &p = layer[li];
        CarryCheck c{};
        if (!state_in || !p.rung.quad) return c;
        c.xmax = p.xmax; c.bad_bits = ST_WIDE_STATE | (defer ? ST_REDO : 0); c.redo = &dyn[li].redo; c.status = status;
        return c;
    }
    // the carry in of layer li, part c (0 = re, 1 = im), or nullptr
    const int32_t *x0(int li, int c) const
    {
        const size_t plane = (size_t)B * layer[li].P;
        return state_in ? state_in + (size_t)li * 2 * plane + c * plane : nullptr;
    }

    // ---- recurrence: the first launch of the layer carries the scan events on every rung
    void recurrence(int li) const
    {
        const LayerPlan &p = layer[li];
        const Rung &r = p.rung;
        const s5fxp_ssm_desc &s = m->layers[li].sd;
        void **evs = opts ? opts->scan_events : nullptr;
        const hipEvent_t ev0 = event(evs, li, 0), ev1 = event(evs, li, 1);
        const unsigned pair_grid = (unsigned)((int64_t)B * (p.P / 32)), quad_grid = (unsigned)((int64_t)B * p.P / 16);
        if (r.pairl) {
            ScanPairLArgs q{};
            q.b16 = I16(w.bq); q.xs = I16(w.xs); q.a_re = p.a_re; q.a_im = p.a_im; q.B = B; q.TB = w.TB; q.P = p.P;
            q.ea_re = s.A_re_exp; q.ea_im = s.A_im_exp; q.x0_re = x0(li, 0); q.x0_im = x0(li, 1); q.live_slots = p.live_slots;
            q.cc = carry_check(li);
            // one helper wave (a second one lands on the computing wave's side of the LDS path and costs more than it
            // helps: profiles/r02_ubench_pair.log).  Blocks per LDS buffer = steps per s_barrier / 4: S5FXP_PAIRL_BLOCKS
            const int blocks = cfg.pairl_blocks;
            launch(blocks == 16 ? k_scan_pairl_asm<16> : k_scan_pairl_asm<32>, pair_grid, 128, 3 * (size_t)blocks * 1024, ev0, ev1, q);
        } else if (r.pair) {
            ScanPairArgs q{};
            q.k = I32(w.bq); q.xs = I16(w.xs); q.a_re = p.a_re; q.a_im = p.a_im; q.B = B; q.TB = w.TB; q.P = p.P;
            q.ea_re = s.A_re_exp; q.ea_im = s.A_im_exp; q.x0_re = x0(li, 0); q.x0_im = x0(li, 1);
            q.cc = carry_check(li);
            launch(k_scan_pair_asm, pair_grid, 64, 0, ev0, ev1, q);
        } else {
            // not quad: states of any width, the exact 32-bit chain in the same quad layout
            auto kernel = !r.quad ? k_scan_quad32_asm : r.s16 ? k_scan_quad_asm16 : k_scan_quad_asm;
            launch(kernel, quad_grid, 64, 0, ev0, ev1, quad_args(li, nullptr));
        }
    }

    // ---- fused C projection + D*u + ReLU + out2 + sigmoid + gate (+ range check, + residual maxima); the exact re-run, the
    // carry out and the state trace
    int gate(int li, const BnArgs &bn) const
    {
        const LayerPlan &p = layer[li];
        const Rung &r = p.rung;
        const LayerDev &l = m->layers[li];
        const FastLayer &fl = F.layers[li];
        const s5fxp_ssm_desc &s = l.sd;
        const DenseDev &o = l.out2;
        const s5fxp_layer_trace *tr = trace(li);
        LayerDyn *d = dyn + li;
        CGateArgs a{};
        a.u = I16(w.u); a.skip = h; a.xs = I32(w.xs); a.w_re = *p.w_cre; a.w_im = *p.w_cim; a.w_o2 = fl.out2.w;
        a.D = fl.Dpad; a.bias_eff = fl.out2.bias_eff; a.z = zp; a.sigtab = fl.sigtab; a.sigdir = fl.sigdir; a.sigdir_bits = fl.sigdir_bits; a.mx_slot = 8;
        a.tr_ys = tr ? tr->ys : nullptr; a.tr_out2 = tr ? tr->out2 : nullptr; a.tr_sig = tr ? tr->out2_sigmoid : nullptr;
        a.tr_z = tr ? tr->post_GLU : nullptr;
        a.N = N; a.L = L; a.TB = w.TB; a.H = H;
        a.rs_re = s.x_re_exp + s.C_re_exp - s.y_exp; a.rs_im = s.x_im_exp + s.C_im_exp - s.y_exp;
        a.rs_d = s.D_exp + s.u_exp - s.y_exp; a.y_bits = s.y_bits; a.y_exp = s.y_exp; a.xmax = p.xmax;
        a.conv = (s.y_bits > o.inp_bits || s.y_exp > o.inp_exp) ? 1 : 0; a.inp_bits = o.inp_bits; a.inp_exp = o.inp_exp;
        a.rs_o2 = (a.conv ? o.inp_exp : s.y_exp) + o.w_exp - o.out_exp;
        if (!shift_ok(a.rs_o2)) return S5FXP_ENEGSHIFT;
        a.out_bits = o.out_bits; a.out_exp = o.out_exp; a.sig_x = l.sig_x; a.sig_y = l.sig_y;
        std::memcpy(a.lut, l.lut, sizeof(a.lut));
        a.l_bits = l.l_bits; a.l_exp = l.l_exp; a.r_bits = l.r_bits; a.r_exp = l.r_exp; a.res_bits = l.res_bits;
        a.res_exp = l.res_exp; a.rs_gate = l.l_exp + l.r_exp - l.res_exp; a.skip_e = he; a.dynw = d; a.status = status;
        a.live_slots = p.live_slots;
        a.bad_bits = ST_WIDE_STATE | (defer ? ST_REDO : 0);
        a.bn = bn;
        a.t_lo = 0; a.t_len = L;
        const unsigned threads = sh.gate_threads;
        const size_t HP = sh.hp; // the kernels' LDS extents
        // the untraced, inexact gate launch carries the gate events
        void **evs = opts ? opts->gate_events : nullptr;
        const hipEvent_t gev0 = event(evs, li, 0), gev1 = event(evs, li, 1);
        const size_t sig_lds = p.direct ? (size_t)sigdir_lds_bytes(fl.sigdir_bits) : 4 * (size_t)SIGTAB_WORDS;
        if (exact) {
            // S5FXP_FWD_EXACT: the exact kernels below are the only ones; raise their gate
            for (int g = 0; g < G; ++g)
                if (int rc = hip_rc(hipMemsetAsync(reinterpret_cast<char *>(&d->redo) + (size_t)g * go.ws, 0xff, 4, st))) return rc;
        } else if (p.gate == GATE_FT32) {
            const size_t smem32 = 5 * HP * 4 + 32 + sig_lds + 2 * 32 * (size_t)(2 * p.P + 16) + 2 * 32 * (HP + 16) + 192 +
                                  2 * 32 * (2 * HP + 8);
            if (p.resid_fold) {
                // the fold overload parks the BatchNorm operands of its 12 channel groups behind the tiles (mfma_fused_body.inc):
                // 31 328 + 384 = 31 712 bytes with an 11-bit sigmoid table.  Five workgroups per CU -- what grid_gate32 is sized
                // for -- stay resident up to GATE_FOLD_LDS_5WG bytes each (measured: tools/probe_lds_budget.hip,
                // profiles/r14_gate_ext_lds_budget.txt); beyond it the launch still gives the same results, in two rounds.
                // 288 bytes are left: whoever adds LDS to this kernel re-runs the probe and the per-kernel trace.
                const size_t smem_fold = smem32 + (size_t)(H / 8) * 32;
                // (A layer with a larger sigmoid table or more state slots is beyond it with or without these 384 bytes.)
                static_assert(GATE_FOLD_LDS_5WG * 5 <= 160 * 1024, "five workgroups per CU");
                CGateFoldArgs fa{};
                static_cast<CGateArgs &>(fa) = a;
                fa.skip_dyn = h_lazy;
                fa.ext_next = p.gate_ext ? ext(li + 1) : nullptr;
                launch(gate_fold_kernel(p), grid_gate32, 192, smem_fold, gev0, gev1, fa);
            } else launch(gate_kernel(p, sh), grid_gate32, 192, smem32, gev0, gev1, a);
        } else {
            // phase-split fused kernel (mfma_fused.hpp): six waves per workgroup, 64-frame tiles, no weights in LDS
            const size_t smem = 5 * HP * 4 + 32 + sig_lds + 2 * 64 * (size_t)(2 * p.P + 16) + 2 * 64 * (HP + 16) + 192 +
                                (p.gate_bn ? 16 * HP : 0) +
                                (p.pk16 && !p.gate_bn ? 2 * 64 * (2 * HP + 8) : 0); // + the u / skip / z tiles (mfma_fused.hpp COAL)
            if (tr) launch(gate_traced_kernel(sh), grid_gate, threads, smem, nullptr, nullptr, a);
            else launch(gate_kernel(p, sh), grid_gate, threads, smem, gev0, gev1, a);
        }
        // ---- exact re-run, only if a state left the fast kernels' range (LayerDyn::redo); with
        // S5FXP_FWD_DEFER_REDO the caller repeats the forward instead (S5FXP_ST_REDO)
        if (!defer) {
            if (r.quad) launch(k_scan_quad32_asm, (unsigned)((int64_t)B * p.P / 16), 64, 0, nullptr, nullptr, quad_args(li, &d->redo));
            // the exact gate kernel: four byte planes of the int32 states, no range assumption; its maxima go to
            // slots 11..13, which the residual pass picks when `redo` is set
            CGateArgs e = a;
            e.run_if = &d->redo; e.mx_slot = 11; e.bad_bits = 0;
            const size_t smem_w = 5 * HP * 4 + 32 + 4 * (size_t)SIGTAB_WORDS + 4 * 64 * (size_t)(2 * p.P + 16) + 2 * 64 * (HP + 16) + 192;
            launch(gate_exact_kernel(p, sh, tr != nullptr), grid_gate_exact, threads, smem_w, nullptr, nullptr, e);
        }
        const size_t plane = (size_t)B * p.P;
        if (state_out) // carry out: the state after frame L-1, from whichever kernel wrote the stream last
            launch(k_state_out, (unsigned)((plane + 255) / 256), 256, 0, nullptr, nullptr, (const void *)I32(w.xs),
                   r.pair ? 2 : (r.s16 ? 1 : 0), defer ? (const int32_t *)nullptr : (const int32_t *)&d->redo, B, L, p.P, w.TB,
                   state_out + (size_t)li * 2 * plane, state_out + (size_t)li * 2 * plane + plane);
        if (tr && (tr->xs_re || tr->xs_im))
            hipLaunchKernelGGL(k_unpack_native, dim3(ew_grid(N * p.P)), dim3(256), 0, st, (const int32_t *)I32(w.xs),
                               tr->xs_re, tr->xs_im, B, L, p.P, w.TB);
        return S5FXP_OK;
    }
    // ---- the residual add's exponent, after the cross-rank maxima
    int res_exponent(int li) const
    {
        LayerDyn *d = dyn + li;
        if (pinned) return S5FXP_OK; // LayerDyn::res is the head launch's; the maxima the gate kernel left are not read
        if (allreduce) {
            // ranks may differ in `redo`: move the valid maxima to slots 8..10 before they are exchanged
            hipLaunchKernelGGL(k_select_maxima, dim3(1), dim3(64), 0, st, d);
            if (allreduce(opts->allreduce_ctx, reinterpret_cast<float *>(d->mx + 8), 3, (void *)st)) return S5FXP_EHIP;
        }
        if (!fold)
            hipLaunchKernelGGL(k_res_finalize, dim3(1), dim3(64), 0, st, d, m->layers[li].res_exp, he, m->layers[li].res_bits, status,
                               status_exps(li), redo_slot());
        return S5FXP_OK;
    }
    int redo_slot() const { return (allreduce || defer) ? 8 : 11; } // mode A moved them; deferred: no re-run happened
    ResidHead resid_head(int li) const
    {
        ResidHead hd{};
        hd.d = dyn + li; hd.res_exp = m->layers[li].res_exp; hd.skip_e = he; hd.redo_slot = redo_slot(); hd.status_exps = status_exps(li);
        hd.enable = fold ? 1 : 0;
        return hd;
    }

    // ---- residual pass (+ the extremes of its output, the next layer's BatchNorm operand); the output becomes the layer input
    void residual(int li)
    {
        const LayerDev &l = m->layers[li];
        const s5fxp_layer_trace *tr = trace(li);
        if (bn_ext) {
            const bool more = li + 1 < m->n_layers && !pinned; // (pinned: a storing pass that gathers nothing)
            const int ext_reps = (more && fold) ? EXT_REPS : 1; // the next layer's B projection derives its exponents from the extremes
            if (layer[li].resid_lazy) {
                // the pass reads U for its extremes and stores nothing; the U plane becomes the layer input, and the plane of
                // the old one the next gate kernel's output
                ResidLazyArgs a{};
                a.u = zp; a.N = N; a.span = rm_span; a.H = H; a.res_bits = l.res_bits; a.hd = resid_head(li);
                a.ext = ext(li + 1); a.ext_reps = ext_reps; a.status = status;
                // gate_ext: the extremes are in `ext` already, in U units; one workgroup per group resolves them and reads no plane
                a.head_only = layer[li].gate_ext ? 1 : 0;
                if (a.head_only) a.u = nullptr;
                launch(static_cast<ResidLazyKernel>(k_resid_minmax16<true, true>), a.head_only ? 1u : rm_grid, RESID_THREADS, 0, nullptr, nullptr, a);
                std::swap(h, zp);
                h_lazy = dyn + li;
                hb = l.res_bits;
                he = DynExp{0, &dyn[li].res.eo};
                return;
            }
            // (resid_fold: the z plane holds U and the pass reads nothing else)
            launch(layer[li].resid_fold ? static_cast<ResidKernel>(k_resid_minmax16<true, true>) : static_cast<ResidKernel>(k_resid_minmax16<true, false>),
                   rm_grid, RESID_THREADS, 0,
                   nullptr, nullptr, (const int16_t *)zp, (const int16_t *)h, hn,
                   tr ? tr->residadd : nullptr, N, H, rm_span, l.res_bits, hb, resid_head(li), more ? ext(li + 1) : nullptr, ext_reps,
                   status);
        } else {
            hipLaunchKernelGGL(k_resid16, dim3(ew_grid(NH / 4)), dim3(256), 0, st, (const int16_t *)zp,
                               (const int16_t *)h, hn, tr ? tr->residadd : nullptr, NH, l.res_bits, hb, (const LayerDyn *)(dyn + li));
        }
        std::swap(h, hn);
        h_lazy = nullptr;
        hb = l.res_bits;
        he = DynExp{0, &dyn[li].res.eo};
    }

    // ---- decoder (with dec_resid: after the last layer's residual pass, which it does itself)
    void decoder(void *y) const
    {
        const DenseDev &e = m->dec;
        DecResid dz{};
        DecArgs a{};
        // IO_F32: k_dec_pf stores float bits; IO_I16: k_dec_ps stores int16
        a.x = h; a.y = reinterpret_cast<int32_t *>(y); a.w = F.dec.w; a.bias_eff = F.dec.bias_eff; a.N = N; a.H = H; a.M = e.M;
        a.xb = hb; a.xe = he; a.inp_bits = e.inp_bits; a.inp_exp = e.inp_exp; a.w_exp = e.w_exp;
        a.out_bits = e.out_bits; a.out_exp = e.out_exp; a.status = status;
        if (dec_resid >= 0) {
            const LayerDev &l = m->layers[dec_resid];
            dz.z = zp; dz.res_bits = l.res_bits; dz.skip_bits = hb; dz.hd = resid_head(dec_resid);
            a.xb = l.res_bits;
            if (layer[dec_resid].resid_fold) { // the z plane holds U: the one plane the decoder reads
                dz.usum = 1;
                a.x = zp;
            }
        }
        // the byte planes and the staged output tile (proj_p.hpp dec_lds_bytes): 80 KB at H = 96 with a 4-byte output, two
        // workgroups per CU, which is what cap_dec asks for; where only one fits (H >= 144 with a 4-byte output) the grid is
        // halved, so that all its workgroups are resident at once
        const size_t smem = dec_lds_bytes(sh.nt, io, e.M);
        const unsigned grid = dec_two_per_cu(smem) ? grid_dec : grid_for(tiles64, std::max<int64_t>(per_group(cfg.cap_dec, 64) / 2, 1));
        auto kernel = nt_kernel(sh.nt, [&](auto n) {
            constexpr int NT = decltype(n)::value;
            return io == IO_F32   ? (dec_resid >= 0 ? k_dec_pf<NT, true> : k_dec_pf<NT, false>)
                   : io == IO_I16 ? (dec_resid >= 0 ? k_dec_ps<NT, true> : k_dec_ps<NT, false>)
                                  : (dec_resid >= 0 ? k_dec_p<NT, true> : k_dec_p<NT, false>);
        });
        launch(kernel, grid, 384, smem, nullptr, nullptr, a, dz);
    }
};

// x / y: int32 tensors, float32 ones with io = IO_F32 (s5fxp_model_forward_f32; the same 4 bytes per element) or int16 ones with
// io = IO_I16 (s5fxp_model_forward_i16; 2 bytes per element, 2-byte aligned)
int forward_fast(const s5fxp_model *m, const void *x, int x_bits, int x_exp, int B, int L, void *y, void *workspace,
                 int32_t *status, const s5fxp_layer_trace *traces, const s5fxp_forward_opts *opts, hipStream_t st, int G = 1,
                 size_t ws_stride = 0, int io = IO_I32, const int32_t *exps = nullptr)
{
    FusedForward f{m, opts, traces, status, st, G, B, L, reinterpret_cast<char *>(workspace), ws_stride, io, exps};
    int rc;
    f.clear_status();
    if ((rc = f.encoder(x, x_bits, x_exp))) return rc;
    if (!f.stage_ok("encoder", -1)) return S5FXP_EHIP;
    for (int li = 0; li < m->n_layers; ++li) {
        const BnArgs bn = make_bn(m->layers[li], f.hb, f.he, f.dyn + li);
        if ((rc = f.bn_exponents(li, bn))) return rc;
        // a lazy layer input is shifted on load by the untraced H = 96 B projection and the fold gate kernel alone (proj_p.hpp LAZY,
        // mfma_fused.hpp CGateFoldArgs::skip_dyn); the plan gives it to no other kernel, and this says so where they are chosen
        if (f.h_lazy && (f.sh.nt != 3 || traces || !f.layer[li].resid_fold)) return S5FXP_EUNSUPPORTED;
        f.bproj(li, bn);
        if (!f.stage_ok("B projection", li)) return S5FXP_EHIP;
        f.recurrence(li);
        if (!f.stage_ok("recurrence", li)) return S5FXP_EHIP;
        if ((rc = f.gate(li, bn))) return rc;
        if (!f.stage_ok("gate kernel", li)) return S5FXP_EHIP;
        if ((rc = f.res_exponent(li))) return rc;
        if (li == f.dec_resid) break;
        f.residual(li);
        if (!f.stage_ok("residual pass", li)) return S5FXP_EHIP;
    }
    f.decoder(y);
    if (!f.stage_ok("decoder", -1)) return S5FXP_EHIP;
    return launch_rc();
}

} // namespace
