// mfma_bn.hpp -- BatchNorm exponents from per-channel extremes, and the lean B projection.
//
// (1) The four BatchNorm ops pick their exponents from float32 maxima over the whole (B,L,H) tensor
//     (fxpmodel.py:892-933, fxparray.py:421-432,602-608).  Per channel h every stage is a MONOTONE map of
//     the layer input x (shift, saturate, add a constant, multiply by a constant, floor shift -- no int32
//     wrap while all operands are <= 16 bit with exponents in [0,15], which the host checks), int32->float32
//     and float32 add/mul by a constant are monotone as well, and |.| of a monotone function peaks at an end
//     point.  So max over the tensor = max over channels of the two end points min_h(x), max_h(x): ONE pass
//     over the tensor (k_resid_minmax16, fused with the previous layer's residual add) and one single-workgroup kernel (k_bn_finalize_mm) replace four reduction
//     passes.  The results are identical by construction; tests compare against the oracle's full reductions.
//
// (2) the lean 16-bit BatchNorm chain (Bn16) and the argument block of the B projection (kernel: proj_p.hpp
//     k_bproj_p): BatchNorm parameters come from LDS, the chain runs four elements at a time, and the SSM input u
//     is written once (int16) so the C projection does not recompute the chain.
#pragma once
#include "mfma_proj.hpp"

namespace s5 {

// one launch instead of two memsets at the head of a forward: the status words and the per-layer device state.  What the
// host knows before the forward goes into the status words here: [2] the path, [8 + 8l + 5] layer l's recurrence kernel,
// [8 + 8l + 6] the state slots its kernels run on (P, or P / 2 for a layer compacted to its live states).
struct StatusInit {
    int32_t path;
    int32_t rk[15];    // 8 + 8 * n_layers <= S5FXP_STATUS_WORDS
    int32_t slots[15];
    int32_t stream[15]; // [8 + 8l + 7]: state slots the recurrence streams hold (<= slots)
};
__global__ __launch_bounds__(256) void k_clear2(int32_t *a, int na, int32_t *b, int nb, StatusInit si, int n_layers, GroupOff go)
{
    gshift(a, (int64_t)blockIdx.y * go.status);
    gshift(b, (int64_t)blockIdx.y * go.ws);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < na + nb; i += gridDim.x * 256) {
        if (i < na) {
            int32_t v = 0;
            if (i == 2) v = si.path;
            else if (i >= 8 && (i & 7) == 5 && (i - 8) / 8 < n_layers) v = si.rk[(i - 8) / 8];
            else if (i >= 8 && (i & 7) == 6 && (i - 8) / 8 < n_layers) v = si.slots[(i - 8) / 8];
            else if (i >= 8 && (i & 7) == 7 && (i - 8) / 8 < n_layers) v = si.stream[(i - 8) / 8];
            a[i] = v;
        } else b[i - na] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// per-channel extremes of an int16 (N,H) tensor as POSITIVE floats: ext[h] = 65536 - min_h, ext[H+h] =
// 65536 + max_h (exact for 16-bit data).  Zero-initialised by a memset; atomicMax on the bit pattern;
// the multi-rank hook (element-wise float MAX) can exchange them as they are.
// ---------------------------------------------------------------------------------------------
constexpr float EXT_BIAS = 65536.f;
// Single-rank forwards spread the workgroups' atomics over EXT_REPS replicas of the 2H extremes (replica = blockIdx % EXT_REPS):
// 512 workgroups hitting the same 192 words serialise at the L2 atomic units for several microseconds, and that time sits
// on the critical path between two layers.  The finalize body folds the replicas with EXT_REPS independent loads.
constexpr int EXT_REPS = 8;

__device__ __forceinline__ void unpack8_i16(const v4i &w, int32_t (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = (int32_t)(int16_t)(w[i] & 0xffff);
        v[2 * i + 1] = w[i] >> 16;
    }
}

// eight uint16 values of a row vector (the residual add's aligned sum U, see SumU16 below)
__device__ __forceinline__ void unpack8_u16(const v4i &w, int32_t (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = (int32_t)((uint32_t)w[i] & 0xffffu);
        v[2 * i + 1] = (int32_t)((uint32_t)w[i] >> 16);
    }
}
// U -> h = relu(add_cb_apply(z, skip)) for the result shift post = lsh - rsh (one of them zero) and the result's clip bounds:
// what add_cb_apply and the ReLU do with a sum that is already formed (the ReLU acts only where a left shift beyond 15 wraps)
__device__ __forceinline__ int32_t resolve_u16(int32_t u, int lsh, int rsh, const SatB &so)
{
    const int32_t v = sat(asr(wshl(u, lsh), rsh), so);
    return v < 0 ? 0 : v;
}

// block reduce of NV float maxima over blockDim.x threads (every thread gets the result)
template <int NV>
__device__ __forceinline__ void block_allmax(float (&v)[NV], float (*red)[8])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float t = v[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t = fmaxf(t, __shfl_xor(t, o, 64));
        if (lane == 0) red[i][wave] = t;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float t = red[i][0];
        for (int w = 1; w < nw; ++w) t = fmaxf(t, red[i][w]);
        v[i] = t;
    }
    __syncthreads();
}

// One workgroup (256 threads >= H): thread h owns channel h and walks its two end points through the
// BatchNorm stages; between stages the workgroup reduces the maxima and thread 0 derives the exponent.
// Callable by any 256-thread workgroup: as its own kernel (k_bn_finalize_mm) or as the tail of the kernel that
// produced the extremes, run by the workgroup that finished last (k_resid_minmax16).  There the extremes were
// written by other workgroups' atomics, possibly on other XCDs: agent-scope loads, not cached ones.
// Returns the derived exponents to EVERY thread; `publish` chooses the workgroup that also writes them to *d and the
// status words (the B projection runs this in every workgroup's prologue: k_bproj_p).
__device__ __forceinline__ LayerDyn bn_finalize_mm_body(const BnArgs &a, const float *ext, int H, LayerDyn *d, int32_t *status,
                                                        int32_t *status_exps, int xe, int reps = 1, bool publish = true)
{
    // This runs on the critical path between two layers (nothing else is executing), so it is written for latency:
    // every operand a channel needs is requested up front, each stage costs ONE barrier (its own reduction slots),
    // and every thread derives the exponents itself from the reduced maxima instead of waiting for thread 0.
    __shared__ float red[4][3][8];
    const int h = threadIdx.x, lane = h & 63, wave = h >> 6, nw = (blockDim.x + 63) >> 6;
    const bool act = h < H;
    float e0 = 0.f, e1 = 0.f;
    int32_t pm = 0, pi = 0, ps = 0, pb = 0;
    if (act) {
        for (int rp = 0; rp < reps; ++rp) {
            e0 = fmaxf(e0, __hip_atomic_load(ext + rp * 2 * H + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            e1 = fmaxf(e1, __hip_atomic_load(ext + rp * 2 * H + H + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
        pm = a.mm[h];
        pi = a.isv[h];
        if (a.scale) ps = a.scale[h];
        if (a.bias) pb = a.bias[h];
    }
    const int32_t xlo = act ? (int32_t)(EXT_BIAS - e0) : 0, xhi = act ? (int32_t)(e1 - EXT_BIAS) : 0;
    LayerDyn sd{};
    auto allmax = [&](int stage, float (&v)[3], int nv) {
        for (int i = 0; i < nv; ++i) {
            float t = v[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t = fmaxf(t, __shfl_xor(t, o, 64));
            if (lane == 0) red[stage][i][wave] = t;
        }
        __syncthreads();
        for (int i = 0; i < nv; ++i) {
            float t = red[stage][i][0];
            for (int w = 1; w < nw; ++w) t = fmaxf(t, red[stage][i][w]);
            v[i] = t;
        }
    };
    // the BatchNorm chain of s5fxp_kernels.hpp bn_chain<>, operands in registers
    auto c1 = [&](int32_t x) { return add_cb_apply(x, a.xb, pm, a.mb, sd.bn1, a.b1); };
    auto c2 = [&](int32_t x) { return sat(asr(wmul(c1(x), pi), sd.rs2), a.b2); };
    auto c3 = [&](int32_t x) {
        const int32_t t = c2(x);
        return a.scale ? sat(asr(wmul(t, ps), sd.rs3), a.b3) : t;
    };
    // ---- stage 1: x + (-mean)        fxpmodel.py:892-897
    {
        float v[3] = {0.f, 0.f, 0.f};
        if (act) {
            const float fm = tofloat(pm, a.me), f0 = tofloat(xlo, xe), f1 = tofloat(xhi, xe);
            v[0] = fmaxf(fabsf(__fadd_rn(f0, fm)), fabsf(__fadd_rn(f1, fm)));
        }
        allmax(0, v, 1); // only max |x + y| chooses the exponent (fxparray.py:421-425); the operands' own maxima size an
                         // intermediate width the device code does not need
        uint32_t m3[3] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
        sd.mx[0] = m3[0]; sd.mx[1] = m3[1]; sd.mx[2] = m3[2];
        sd.bn1 = finalize_add_cb(m3, xe, a.me, a.b1, status);
        sd.bn_e = sd.bn1.eo;
    }
    // ---- stage 2: * invsq_var        fxpmodel.py:902-907
    {
        float v[3] = {0.f, 0.f, 0.f};
        if (act) {
            const float fi = tofloat(pi, a.ie);
            const float f0 = tofloat(c1(xlo), sd.bn1.eo), f1 = tofloat(c1(xhi), sd.bn1.eo);
            v[0] = fmaxf(fabsf(__fmul_rn(f0, fi)), fabsf(__fmul_rn(f1, fi)));
        }
        allmax(1, v, 1);
        sd.mx[3] = __float_as_uint(v[0]);
        finalize_mul_cb(sd.mx[3], sd.bn1.eo, a.ie, a.b2, sd.rs2, sd.e2, status);
        sd.bn_e = sd.e2;
    }
    // ---- stage 3: * scale            fxpmodel.py:915-920
    if (a.scale) {
        float v[3] = {0.f, 0.f, 0.f};
        if (act) {
            const float fs = tofloat(ps, a.se);
            const float f0 = tofloat(c2(xlo), sd.e2), f1 = tofloat(c2(xhi), sd.e2);
            v[0] = fmaxf(fabsf(__fmul_rn(f0, fs)), fabsf(__fmul_rn(f1, fs)));
        }
        allmax(2, v, 1);
        sd.mx[4] = __float_as_uint(v[0]);
        finalize_mul_cb(sd.mx[4], sd.e2, a.se, a.b3, sd.rs3, sd.e3, status);
        sd.bn_e = sd.e3;
    }
    // ---- stage 4: + bias             fxpmodel.py:928-933
    if (a.bias) {
        const int e3 = a.scale ? sd.e3 : sd.e2;
        float v[3] = {0.f, 0.f, 0.f};
        if (act) {
            const float fb = tofloat(pb, a.be);
            const float f0 = tofloat(c3(xlo), e3), f1 = tofloat(c3(xhi), e3);
            v[0] = fmaxf(fabsf(__fadd_rn(f0, fb)), fabsf(__fadd_rn(f1, fb)));
        }
        allmax(3, v, 1);
        uint32_t m3[3] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
        sd.mx[5] = m3[0]; sd.mx[6] = m3[1]; sd.mx[7] = m3[2];
        sd.bn4 = finalize_add_cb(m3, e3, a.be, a.b4, status);
        sd.bn_e = sd.bn4.eo;
    }
    if (h == 0 && publish) { // (redo and the residual maxima slots of *d are written later in the layer)
        d->bn1 = sd.bn1; d->rs2 = sd.rs2; d->e2 = sd.e2; d->rs3 = sd.rs3; d->e3 = sd.e3; d->bn4 = sd.bn4; d->bn_e = sd.bn_e;
        for (int i = 0; i < 8; ++i) d->mx[i] = sd.mx[i];
        status_exps[0] = sd.bn1.eo;
        status_exps[1] = sd.e2;
        if (a.scale) status_exps[2] = sd.e3;
        if (a.bias) status_exps[3] = sd.bn4.eo;
    }
    return sd;
}

// stand-alone form (multi-rank mode: the extremes are exchanged between the two kernels)
__global__ __launch_bounds__(256) void k_bn_finalize_mm(BnArgs a, const float *ext, int H, LayerDyn *d, int32_t *status,
                                                        int32_t *status_exps)
{
    (void)bn_finalize_mm_body(a, ext, H, d, status, status_exps, a.xe.get());
}

// Residual add + ReLU of one layer and, in the same pass, the per-channel extremes of its result (the next
// layer's BatchNorm operand).  RESID=false: extremes of z only (the encoder output ahead of layer 0).
// block = 384 threads = G8 channel-groups (8 channels = 16 bytes each) x R frame lanes (64 / 32 / 21 / 16 at H = 48 / 96 / 144 / 192);
// a workgroup owns `span` consecutive frames (a multiple of 4R) and keeps four frames per thread in flight.
// ext == nullptr: no extremes wanted (last layer).
// Two single-workgroup kernels are folded in (single-rank mode; with a multi-rank hook they stay separate
// because the ranks exchange maxima in between):
//   head  the residual add's compute_best exponent (k_res_finalize): every workgroup derives it from the three
//         maxima, workgroup 0 publishes it;
//   tail  the NEXT layer's BatchNorm exponents (k_bn_finalize_mm): the workgroup that takes the last ticket
//         runs it once all extremes are in.  No workgroup ever waits for another.
struct ResidHead {
    LayerDyn *d;
    int32_t res_exp;
    DynExp skip_e;
    int32_t redo_slot;
    int32_t *status_exps;
    int32_t enable; // 0: d->res was written by k_res_finalize
};

// USUM (with RESID): z_ holds the gate kernel's aligned sum U (uint16, SumU16 below) instead of z: the pass reads that one
// plane, not z and skip, and h = resolve_u16(U) (s5fxp_fast.hpp LayerPlan::resid_fold)
constexpr int RESID_THREADS = 384;
template <bool RESID, bool USUM = false>
__global__ __launch_bounds__(RESID_THREADS, 5) void k_resid_minmax16(const int16_t *z_, const int16_t *skip_, int16_t *out_, int32_t *tr_resid,
                                                                  int64_t N, int H, int64_t span, int res_bits, int skip_bits, ResidHead hd,
                                                                  float *ext, int ext_reps, int32_t *status, GroupOff go)
{
    // this group's tensors (scan_quad.hpp GroupOff); the three streams keep their no-alias promise
    const int64_t gws = (int64_t)blockIdx.y * go.ws, gst = (int64_t)blockIdx.y * go.status;
    const int16_t *__restrict__ z = reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(z_) + gws);
    const int16_t *__restrict__ skip = reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(skip_) + gws);
    int16_t *__restrict__ out = reinterpret_cast<int16_t *>(reinterpret_cast<char *>(out_) + gws);
    gshift(ext, gws); gshift_nn(hd.d, gws); gshift(hd.skip_e.dyn, gws); gshift_nn(hd.status_exps, gst); gshift_nn(status, gst);
    __shared__ int32_t smin[RESID_THREADS * 8], smax[RESID_THREADS * 8];
    __shared__ AddCb sp;
    const int G = H >> 3, R = RESID_THREADS / G;
    const int g = threadIdx.x % G, rl = threadIdx.x / G;
    // a round = four frames per thread.  The first round's loads are issued BEFORE the head below: its exponent arithmetic
    // needs the maxima, the loads do not.  (Double-buffering every round was tried: 171 registers, one workgroup per CU
    // instead of three, 29 us instead of 23.)
    // frames of this workgroup: [lo_n, lo_n + cnt).  Everything inside is addressed as a wave-uniform base (the workgroup's
    // first frame) plus a 32-bit byte offset per thread: no 64-bit address arithmetic in the loop (the kernel sits at the
    // 96 registers that three workgroups per CU allow)
    const int64_t lo_n = (int64_t)blockIdx.x * span;
    // (H = 144: 18 groups x 21 frame lanes = 378 threads; the six spare ones, rl == R, own no frame and fold neutral extremes)
    const int cnt = rl < R ? (int)((lo_n + span < N ? lo_n + span : N) - lo_n) : 0;
    const char *zb = reinterpret_cast<const char *>(z + lo_n * H), *sb = reinterpret_cast<const char *>(skip + lo_n * H);
    char *ob = reinterpret_cast<char *>(out + lo_n * H);
    const unsigned rowb = 2u * (unsigned)H;                       // bytes per frame
    const unsigned toff = (unsigned)rl * rowb + 16u * (unsigned)g; // this thread's first vector
    const unsigned kstep = (unsigned)R * rowb;                    // R frames further
    auto fetch = [&](v4i(&zq)[4], v4i(&sq)[4], int i0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k * R + rl < cnt) {
                const unsigned o = toff + (unsigned)(i0 / R) * kstep + (unsigned)k * kstep;
                zq[k] = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(zb + o));
                if constexpr (RESID && !USUM) sq[k] = *reinterpret_cast<const v4i *>(sb + o);
            }
        }
    };
    v4i za[4], sa[4];
    const int first = rl, step = 4 * R; // frame indices relative to lo_n; i0 - rl is always a multiple of R
    if (first < cnt) fetch(za, sa, 0);
    AddCb p{};
    if constexpr (RESID) {
        if (hd.enable) {
            if (threadIdx.x == 0) {
                sp = finalize_add_cb(hd.d->mx + (hd.d->redo ? hd.redo_slot : 8), hd.res_exp, hd.skip_e.get(), res_bits, status);
                if (blockIdx.x == 0) {
                    hd.d->res = sp;
                    hd.status_exps[4] = sp.eo;
                }
            }
            __syncthreads();
            p = sp;
        } else {
            p = hd.d->res;
        }
    }
    AddCbV pv{};
    if constexpr (RESID) pv = make_add_cb_v(p, res_bits, skip_bits, res_bits);
    int32_t lo[8], hi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        lo[e] = 32767;
        hi[e] = -32768;
    }
    auto process = [&](const v4i(&zq)[4], const v4i(&sq)[4], int i0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k * R + rl < cnt) {
                int32_t v[8], s[8];
                if constexpr (USUM) unpack8_u16(zq[k], v);
                else unpack8_i16(zq[k], v);
                if constexpr (RESID && USUM) {
                    const unsigned o = toff + (unsigned)(i0 / R) * kstep + (unsigned)k * kstep;
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = resolve_u16(v[e], pv.lsh, pv.rsh, pv.so);
                    const v2i a = pack4_i16(v[0], v[1], v[2], v[3]), b = pack4_i16(v[4], v[5], v[6], v[7]);
                    *reinterpret_cast<v4i *>(ob + o) = v4i{a[0], a[1], b[0], b[1]};
                } else if constexpr (RESID) {
                    unpack8_i16(sq[k], s);
                    const unsigned o = toff + (unsigned)(i0 / R) * kstep + (unsigned)k * kstep;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int32_t rr = add_cb_apply(v[e], s[e], pv);
                        if (tr_resid) tr_resid[lo_n * H + (o >> 1) + e] = rr;
                        v[e] = rr < 0 ? 0 : rr;
                    }
                    const v2i a = pack4_i16(v[0], v[1], v[2], v[3]), b = pack4_i16(v[4], v[5], v[6], v[7]);
                    *reinterpret_cast<v4i *>(ob + o) = v4i{a[0], a[1], b[0], b[1]};
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    lo[e] = v[e] < lo[e] ? v[e] : lo[e];
                    hi[e] = v[e] > hi[e] ? v[e] : hi[e];
                }
            }
        }
    };
    for (int i0 = 0; i0 + rl < cnt; i0 += step) {
        process(za, sa, i0);
        if (i0 + step + rl < cnt) fetch(za, sa, i0 + step);
    }
    if (!ext) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        smin[threadIdx.x * 8 + e] = lo[e];
        smax[threadIdx.x * 8 + e] = hi[e];
    }
    __syncthreads();
    {
        // fold the R frame lanes: one thread per (bound, channel) -- two per item at H = 96, each folding half the lanes
        const int items = 2 * H, parts = RESID_THREADS / items > 1 ? 2 : 1, per = R / parts;
        const int item = threadIdx.x % items, part = threadIdx.x / items;
        const bool is_max = item >= H;
        const int c = is_max ? item - H : item;
        int32_t v = is_max ? -32768 : 32767;
        if (part < parts) {
            const int32_t *src = is_max ? smax : smin;
            for (int r = part * per; r < (part + 1) * per; ++r) {
                const int32_t t = src[r * G * 8 + c];
                v = is_max ? max(v, t) : min(v, t);
            }
        }
        __syncthreads();
        if (parts == 2 && part == 1) smin[item] = v; // the arrays are free now
        __syncthreads();
        if (part == 0) {
            if (parts == 2) {
                const int32_t t = smin[item];
                v = is_max ? max(v, t) : min(v, t);
            }
            const int rep = ext_reps > 1 ? (int)(blockIdx.x % ext_reps) : 0;
            atomicMax(reinterpret_cast<uint32_t *>(ext) + rep * 2 * H + item,
                      __float_as_uint(is_max ? EXT_BIAS + (float)v : EXT_BIAS - (float)v));
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Lean BatchNorm chain for the MFMA path.  Preconditions (host-checked, the same as for the extremes
// method): every BN operand <= 16 bit, exponents in [0,15]; the input is stored as int16 within its
// nominal bits.  Under them this is bn_chain<> with the data-independent parts moved out of the element:
//   * sat(v << 0, bits) == v for in-range v, so the "shift only if needed" selects disappear;
//   * "post > 0 ? << : >>" is (v << l) >> r with one of l, r zero;
//   * the per-channel operands (mean, bias) are shifted/saturated once per workgroup into LDS;
//   * 16 x 16-bit products fit v_mul_i32_i24 (full rate), whose low 32 bits are the exact product;
//   * change_cfg(t -> u) is a shift pair and one saturation at min(out_bits, u_bits).
// ---------------------------------------------------------------------------------------------
struct Bn16 {
    const int32_t *m1, *isv, *sc, *b4; // LDS, (H) each
    int32_t shx1, l1, r1, b1, xb;
    int32_t rs2, b2;
    int32_t has_sc, rs3, b3;
    int32_t has_b, shx4, tb4, l4, r4, b4b;
    int32_t cl, cr, cbits;
    fxp::SatB sxb, s1, s2, s3, stb4, s4b, scb; // the clip bounds of the chain, resident in VGPRs (fxp_prims.hpp sat_bounds)
};

// builds the LDS tables (all threads) and returns the scalars; call before a __syncthreads()
__device__ __forceinline__ Bn16 bn16_setup(const BnArgs &a, const LayerDyn &d, int32_t *lds, int H)
{
    Bn16 p;
    int32_t *m1 = lds, *isv = lds + H, *sc = lds + 2 * H, *b4 = lds + 3 * H;
    for (int h = threadIdx.x; h < H; h += blockDim.x) {
        m1[h] = sat(wshl(a.mm[h], d.bn1.shy), a.mb);
        isv[h] = a.isv[h];
        sc[h] = a.scale ? a.scale[h] : 0;
        b4[h] = a.bias ? sat(wshl(a.bias[h], d.bn4.shy), a.bb) : 0;
    }
    p.m1 = m1; p.isv = isv; p.sc = sc; p.b4 = b4;
    p.shx1 = d.bn1.shx; p.l1 = d.bn1.post > 0 ? d.bn1.post : 0; p.r1 = d.bn1.post < 0 ? -d.bn1.post : 0;
    p.b1 = a.b1; p.xb = a.xb;
    p.rs2 = d.rs2; p.b2 = a.b2;
    p.has_sc = a.scale != nullptr; p.rs3 = d.rs3; p.b3 = a.b3;
    p.has_b = a.bias != nullptr; p.shx4 = d.bn4.shx; p.tb4 = a.scale ? a.b3 : a.b2;
    p.l4 = d.bn4.post > 0 ? d.bn4.post : 0; p.r4 = d.bn4.post < 0 ? -d.bn4.post : 0; p.b4b = a.b4;
    const int de = a.ue - d.bn_e;
    p.cl = de > 0 ? de : 0; p.cr = de < 0 ? -de : 0;
    p.cbits = a.out_bits < a.ub ? a.out_bits : a.ub;
    p.sxb = fxp::sat_bounds(p.xb); p.s1 = fxp::sat_bounds(p.b1); p.s2 = fxp::sat_bounds(p.b2);
    p.scb = fxp::sat_bounds(p.cbits);
    // (the scale / bias stages are rare: their bounds are only made when the stages exist)
    if (p.has_sc) p.s3 = fxp::sat_bounds(p.b3);
    if (p.has_b) { p.stb4 = fxp::sat_bounds(p.tb4); p.s4b = fxp::sat_bounds(p.b4b); }
    return p;
}

// four consecutive channels h0..h0+3: BatchNorm output t (pre_s5) and SSM input u
__device__ __forceinline__ void bn16_x4(const Bn16 &p, const int32_t (&x)[4], int h0, int32_t (&t)[4], int32_t (&u)[4])
{
    const v4i m4 = *reinterpret_cast<const v4i *>(p.m1 + h0), i4 = *reinterpret_cast<const v4i *>(p.isv + h0);
    v4i s4 = {0, 0, 0, 0}, b4 = {0, 0, 0, 0};
    if (p.has_sc) s4 = *reinterpret_cast<const v4i *>(p.sc + h0);
    if (p.has_b) b4 = *reinterpret_cast<const v4i *>(p.b4 + h0);
    // stage by stage over the four channels: the two optional stages cost one uniform branch per call, not one per element
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int32_t v = sat(asr(wshl(wadd(sat(wshl(x[e], p.shx1), p.sxb), m4[e]), p.l1), p.r1), p.s1);
        t[e] = sat(asr(__mul24(v, i4[e]), p.rs2), p.s2);
    }
    if (p.has_sc) {
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = sat(asr(__mul24(t[e], s4[e]), p.rs3), p.s3);
    }
    if (p.has_b) {
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = sat(asr(wshl(wadd(sat(wshl(t[e], p.shx4), p.stb4), b4[e]), p.l4), p.r4), p.s4b);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = sat(asr(wshl(t[e], p.cl), p.cr), p.scb);
}

// ---- packed 16-bit helpers of the PK16 epilogues (semantics probed on MI355X: tools/probe_pk16.hip -- the clamped forms
// saturate the EXACT result, v_cvt_pk_i16_i32 saturates each half, the SDWA forms sign-extend the selected half)
__device__ __forceinline__ uint32_t pk_cvt(int32_t lo, int32_t hi) // (sat16(lo), sat16(hi))
{
    uint32_t r;
    asm("v_cvt_pk_i16_i32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ uint32_t pk_sub_sat(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_sub_i16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_add_sat(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_add_i16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_mad_sat(uint32_t a, uint32_t m, uint32_t c) // sat16(a * m + c) per half
{
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(m), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_ashr(uint32_t a, uint32_t s) // s = shift in both halves
{
    uint32_t r;
    asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(r) : "v"(s), "v"(a));
    return r;
}
// the same with a wave-uniform second operand taken from an SGPR (no v_mov per use)
__device__ __forceinline__ uint32_t pk_mul_sat_u(uint32_t a, uint32_t m_uniform) // sat16(a * m) per half
{
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, 0 clamp" : "=v"(r) : "v"(a), "s"(m_uniform));
    return r;
}
__device__ __forceinline__ uint32_t pk_ashr_u(uint32_t a, uint32_t s_uniform)
{
    uint32_t r;
    asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(r) : "s"(s_uniform), "v"(a));
    return r;
}
template <int HALF>
__device__ __forceinline__ int32_t mul24_h(int32_t a, uint32_t pk) // a * sext(half HALF of pk)
{
    int32_t r;
    if (HALF == 0)
        asm("v_mul_i32_i24_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(a), "v"(pk));
    else
        asm("v_mul_i32_i24_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(a), "v"(pk));
    return r;
}
template <int HALF>
__device__ __forceinline__ float cvtf_h(uint32_t pk) // float(sext(half))
{
    float r;
    if (HALF == 0) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(r) : "v"(pk));
    else asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(r) : "v"(pk));
    return r;
}
template <int HALF>
__device__ __forceinline__ int32_t ashr_h(int32_t s, uint32_t pk) // sext(half) >> s, s wave-uniform (an SGPR operand)
{
    int32_t r;
    if (HALF == 0)
        asm("v_ashrrev_i32_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "s"(s), "v"(pk));
    else
        asm("v_ashrrev_i32_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "s"(s), "v"(pk));
    return r;
}

// both operands taken from the same half of two packed registers (sign-extended)
template <int HALF>
__device__ __forceinline__ int32_t mul24_hh(uint32_t apk, uint32_t bpk) // sext(half of apk) * sext(half of bpk)
{
    int32_t r;
    if (HALF == 0)
        asm("v_mul_i32_i24_sdwa %0, sext(%1), sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_0" : "=v"(r) : "v"(apk), "v"(bpk));
    else
        asm("v_mul_i32_i24_sdwa %0, sext(%1), sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(r) : "v"(apk), "v"(bpk));
    return r;
}
template <int HALF>
__device__ __forceinline__ int32_t add_hh(uint32_t apk, uint32_t bpk) // sext(half of apk) + sext(half of bpk): the 17-bit sum
{
    int32_t r;
    if (HALF == 0)
        asm("v_add_u32_sdwa %0, sext(%1), sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_0" : "=v"(r) : "v"(apk), "v"(bpk));
    else
        asm("v_add_u32_sdwa %0, sext(%1), sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(r) : "v"(apk), "v"(bpk));
    return r;
}

// ---------------------------------------------------------------------------------------------
// The residual add's aligned sum as an unsigned 16-bit word (resid_fold).  Of the compute_best add
// h = relu(add_cb_apply(z, skip)) (fxp_prims.hpp) only the result shift `post` depends on the batch-wide maximum; the operand
// shifts shx, shy depend on the two operand exponents alone (s5fxp_kernels.hpp finalize_add_cb), and those the gate kernel
// knows.  With 16-bit operands and skip >= 0 (a ReLU output)
//     U = max(sat16(z << shx) + sat16(skip << shy), 0)   lies in [0, 65534]: a uint16, nothing lost, and
//     h = min(shift(U, post), 32767)                     for every post in [-31, 15]
// (the ReLU commutes with the floor shift and the clip; a negative sum shifted LEFT by more than 15 could wrap to a positive
// int32, which is why the plan asks for res_exp >= 0: then post <= 15, s5fxp_fast.hpp plan_layers).  The gate kernel stores U
// where z went; the residual pass and the decoder's fused residual read that one plane instead of z and skip.
// tests/test_resid_fold.py runs tools/probe_resid_u16.hip: both helpers against add_cb_apply + ReLU on every operand pair.
// ---------------------------------------------------------------------------------------------
struct SumU16 {
    // sat16(v << sh) as two clamped packed multiplies, by 2^min(sh, 14) and by 2^(sh > 14): a 16-bit value shifted left by 15 or
    // more is already on its rail (or zero), so sh = 16 gives what sh = 15 gives; beyond 16 the reference's int32 shift wraps,
    // which the plan excludes for every valid batch: 0 <= res_exp <= 16 is checked on the host, and the layer input's exponent
    // is in [0, 15] unless a compute_best op chose a negative one -- that batch carries ST_NEGEXP, the caller raises on it
    // (include/s5fxp.h) and its output, here as in the two-plane kernels, means nothing.  Both halves of a word
    // hold the same multiplier; the gate kernel keeps the four words in LDS (it has no scalar register to spare)
    uint32_t mz, mz2, ms, ms2;
};
__host__ __device__ __forceinline__ SumU16 sum_u16_setup(int shx, int shy)
{
    SumU16 p;
    p.mz = 0x10001u << (shx < 14 ? shx : 14); p.mz2 = shx > 14 ? 0x20002u : 0x10001u;
    p.ms = 0x10001u << (shy < 14 ? shy : 14); p.ms2 = shy > 14 ? 0x20002u : 0x10001u;
    return p;
}
// the shifts finalize_add_cb will derive for x = z at res_exp and y = skip at skip_e
__host__ __device__ __forceinline__ SumU16 sum_u16_setup_exps(int res_exp, int skip_e)
{
    const int ea = res_exp > skip_e ? res_exp : skip_e;
    return sum_u16_setup(ea - res_exp, ea - skip_e);
}
__device__ __forceinline__ uint32_t pk_mul_sat(uint32_t a, uint32_t m) // sat16(a * m) per half
{
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, 0 clamp" : "=v"(r) : "v"(a), "v"(m));
    return r;
}
// one int16 pair of z and of skip (skip >= 0) -> their U pair
__device__ __forceinline__ uint32_t sum_u16_pair(const SumU16 &p, uint32_t z, uint32_t s)
{
    const uint32_t a = pk_mul_sat(pk_mul_sat(z, p.mz), p.mz2), b = pk_mul_sat(pk_mul_sat(s, p.ms), p.ms2);
    // a + b >= 0 fits 16 unsigned bits, and max(a, -b) + b is max(a + b, 0) without the 17-bit intermediate
    const uint32_t m = pk_max(a, pk_sub_sat(0u, b)); // (-b >= -32767: the clamp never acts)
    uint32_t r;
    asm("v_pk_add_u16 %0, %1, %2" : "=v"(r) : "v"(m), "v"(b));
    return r;
}

// ---------------------------------------------------------------------------------------------
// resid_lazy: between two layers the U plane IS the layer input.  The residual pass stores nothing; the next
// layer's B projection and gate kernel load U and shift it themselves, with the result shift the pass published in the
// producer layer's LayerDyn::res.  U -> h is resolve_u16 above: min(shift(U, post), 32767) for post in [-31, 15], monotone
// non-decreasing in U, so the per-channel extremes of h are resolve_u16 of the per-channel extremes of U.
// On a uint16 pair: a logical right shift by -post (a shift of 16 or more leaves zero: the multiplier m1 is 0 then, the
// packed shift takes its count modulo 16), the clip min(., 32767) as an unsigned minimum -- after it both halves are
// non-negative int16 -- and a left shift as two clamped multiplies, by 2^min(post, 14) and by 2^(post > 14), which saturate
// at 32767 as the clip does.  RES_RIGHT (-15 <= post <= 0): the shift and the minimum are all there is.
// tests/test_resid_lazy.py runs tools/probe_resolve_u16.hip: every U x every post against resolve_u16, both halves.
// ---------------------------------------------------------------------------------------------
enum { RES_GENERIC = 0, RES_RIGHT = 1 };
struct ResolveU16 {
    uint32_t shr, m1, m2; // -post mod 16, 2^min(post, 14) or 0, 2^(post > 14): the same in both halves
    int32_t arm;
};
__host__ __device__ __forceinline__ ResolveU16 resolve_u16_setup(int post)
{
    const int lsh = post > 0 ? post : 0, rsh = post < 0 ? -post : 0;
    ResolveU16 p;
    p.shr = 0x10001u * (uint32_t)(rsh & 15);
    p.m1 = rsh > 15 ? 0u : 0x10001u << (lsh < 14 ? lsh : 14);
    p.m2 = lsh > 14 ? 0x20002u : 0x10001u;
    p.arm = lsh == 0 && rsh <= 15 ? RES_RIGHT : RES_GENERIC;
    return p;
}
__device__ __forceinline__ uint32_t pk_lshr(uint32_t a, uint32_t s) // logical, s = shift in both halves
{
    uint32_t r;
    asm("v_pk_lshrrev_b16 %0, %1, %2" : "=v"(r) : "v"(s), "v"(a));
    return r;
}
__device__ __forceinline__ uint32_t pk_min_u(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_max_u(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// one uint16 pair of U -> its h pair (int16, >= 0)
template <int ARM = RES_GENERIC>
__device__ __forceinline__ uint32_t resolve_u16_pair(const ResolveU16 &p, uint32_t u)
{
    const uint32_t t = pk_min_u(pk_lshr(u, p.shr), 0x7fff7fffu);
    if constexpr (ARM == RES_RIGHT) return t;
    else return pk_mul_sat(pk_mul_sat(t, p.m1), p.m2);
}

// The residual pass of a lazy layer: a read-only reduction over the U plane.  Head as in k_resid_minmax16 above (the residual
// add's exponent; workgroup 0 publishes it, and with it the shift the consumers of the plane use); body: packed unsigned
// running extremes of the thread's eight channels, nothing stored; tail: the folded extremes of U go through resolve_u16 and
// into the replicas as the extremes of h.  Same threads, spans and grid as the storing form.  It is an overload on the
// argument block, not a third template argument (the launch list of a forward names k_resid_minmax16<true, true>).
struct ResidLazyArgs {
    const int16_t *u; // (N,H) uint16: the gate kernel's aligned sum
    int64_t N, span;
    int32_t H, res_bits;
    ResidHead hd;
    float *ext;
    int32_t ext_reps;
    int32_t *status;
    // gate_ext: the gate kernel has left the extremes of U in `ext`, all ext_reps replicas, in U units
    // (mfma_fused.hpp CGateFoldArgs::ext_next).  One workgroup per group: the head as always, then every word of the block goes
    // decode -> resolve_u16 -> encode, in place.  The map is monotone, so resolving each replica and letting the B projection's
    // prologue fold them (a float maximum) equals folding first and resolving the fold, which is what the reading pass does.
    // A word no workgroup wrote stays zero, below every encoded value.  `u` is not dereferenced.
    int32_t head_only;
};
template <bool RESID, bool USUM>
__global__ __launch_bounds__(RESID_THREADS, 5) void k_resid_minmax16(ResidLazyArgs a, GroupOff go)
{
    static_assert(RESID && USUM, "the read-only pass exists for the one-plane residual add");
    const int64_t gws = (int64_t)blockIdx.y * go.ws, gst = (int64_t)blockIdx.y * go.status;
    const int16_t *__restrict__ u = reinterpret_cast<const int16_t *>(reinterpret_cast<const char *>(a.u) + gws);
    ResidHead hd = a.hd;
    float *ext = a.ext;
    int32_t *status = a.status;
    gshift(ext, gws); gshift_nn(hd.d, gws); gshift(hd.skip_e.dyn, gws); gshift_nn(hd.status_exps, gst); gshift_nn(status, gst);
    __shared__ uint32_t smin[RESID_THREADS * 4], smax[RESID_THREADS * 4]; // packed pairs: [thread][pair]
    __shared__ AddCb sp;
    const int H = a.H, G = H >> 3, R = RESID_THREADS / G;
    const int g = threadIdx.x % G, rl = threadIdx.x / G;
    const int64_t lo_n = (int64_t)blockIdx.x * a.span;
    const int cnt = rl < R && !a.head_only ? (int)((lo_n + a.span < a.N ? lo_n + a.span : a.N) - lo_n) : 0;
    const char *ub = reinterpret_cast<const char *>(u + lo_n * H);
    const unsigned rowb = 2u * (unsigned)H, toff = (unsigned)rl * rowb + 16u * (unsigned)g, kstep = (unsigned)R * rowb;
    auto fetch = [&](v4i(&q)[4], int i0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k * R + rl < cnt)
                q[k] = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(ub + toff + (unsigned)(i0 / R) * kstep + (unsigned)k * kstep));
    };
    v4i qa[4];
    const int step = 4 * R;
    if (rl < cnt) fetch(qa, 0);
    AddCb p{};
    if (hd.enable) {
        if (threadIdx.x == 0) {
            sp = finalize_add_cb(hd.d->mx + (hd.d->redo ? hd.redo_slot : 8), hd.res_exp, hd.skip_e.get(), a.res_bits, status);
            if (blockIdx.x == 0) {
                hd.d->res = sp;
                hd.status_exps[4] = sp.eo;
            }
        }
        __syncthreads();
        p = sp;
    } else {
        p = hd.d->res;
    }
    if (a.head_only) {
        if (!ext) return;
        const SatB so = sat_bounds(a.res_bits);
        const int lsh = p.post > 0 ? p.post : 0, rsh = p.post < 0 ? -p.post : 0;
        // (the grid is (1, G) by contract, s5fxp_fast.hpp residual(): one workgroup owns its group's block, every word resolved once)
        for (int i = threadIdx.x; i < a.ext_reps * 2 * H; i += RESID_THREADS) {
            const float e = ext[i];
            if (e == 0.f) continue;
            const bool is_max = i % (2 * H) >= H;
            const int32_t v = resolve_u16(is_max ? (int32_t)(e - EXT_BIAS) : (int32_t)(EXT_BIAS - e), lsh, rsh, so);
            ext[i] = is_max ? EXT_BIAS + (float)v : EXT_BIAS - (float)v;
        }
        return;
    }
    uint32_t lo[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[4] = {0u, 0u, 0u, 0u};
    for (int i0 = 0; i0 + rl < cnt; i0 += step) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k * R + rl < cnt) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lo[e] = pk_min_u(lo[e], (uint32_t)qa[k][e]);
                    hi[e] = pk_max_u(hi[e], (uint32_t)qa[k][e]);
                }
            }
        }
        if (i0 + step + rl < cnt) fetch(qa, i0 + step);
    }
    if (!ext) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        smin[threadIdx.x * 4 + e] = lo[e];
        smax[threadIdx.x * 4 + e] = hi[e];
    }
    __syncthreads();
    {
        // fold the R frame lanes: one thread per (bound, channel) -- two per item at H = 96, each folding half the lanes
        const int items = 2 * H, parts = RESID_THREADS / items > 1 ? 2 : 1, per = R / parts;
        const int item = threadIdx.x % items, part = threadIdx.x / items;
        const bool is_max = item >= H;
        const int c = is_max ? item - H : item;
        int32_t v = is_max ? 0 : 65535;
        if (part < parts) {
            const uint16_t *src = reinterpret_cast<const uint16_t *>(is_max ? smax : smin);
            for (int r = part * per; r < (part + 1) * per; ++r) {
                const int32_t t = src[r * G * 8 + c];
                v = is_max ? max(v, t) : min(v, t);
            }
        }
        __syncthreads();
        if (parts == 2 && part == 1) smin[item] = (uint32_t)v; // the arrays are free now
        __syncthreads();
        if (part == 0) {
            if (parts == 2) {
                const int32_t t = (int32_t)smin[item];
                v = is_max ? max(v, t) : min(v, t);
            }
            // the extremes of h: the shift and the clip are monotone in U
            v = resolve_u16(v, p.post > 0 ? p.post : 0, p.post < 0 ? -p.post : 0, sat_bounds(a.res_bits));
            const int rep = a.ext_reps > 1 ? (int)(blockIdx.x % a.ext_reps) : 0;
            atomicMax(reinterpret_cast<uint32_t *>(ext) + rep * 2 * H + item,
                      __float_as_uint(is_max ? EXT_BIAS + (float)v : EXT_BIAS - (float)v));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same chain in ROW layout, for a kernel whose threads hold 16-byte row vectors (eight consecutive channels of one frame
// as int16) and always the SAME eight channels: the gate kernel's tile staging (mfma_fused.hpp k_cgate_p<.., UREC>), which
// rebuilds the SSM input u from the layer input instead of reading the plane the B projection would have stored.  The
// per-channel operands sit in registers as packed int16 pairs (no LDS table); models with a BatchNorm scale or bias stage do
// not come here (host-known: s5fxp_fast.hpp plan_layer).
//
// One of three arms, chosen ONCE per workgroup from the wave-uniform shifts the B projection published in LayerDyn and the
// static widths.  What the models of the benchmark and of the test recipes produce (NumPy oracle, all three layers, configs[1]
// and [2], input scales 0.25 .. 6): every width 16; shx1 = 0..7, the mean never shifted, l1 = 0 always, r1 = 0..4;
// rs2 = 6..14; cl = 0..4 or cr = 1..6.  With W16 := xb == 16 (or shx1 == 0: the stored input is within its bits), b1 == 16,
// b2 == 16, min(out_bits, ub) == 16, mean and isv within 16 bits, shx1 <= 14, l1 == 0, cl <= 14, cr <= 15:
//   ROW_PACKED  W16 && r1 == 0.  sat(x << shx1, 16) is the clamped packed multiply by 2^shx1 (exact product, then the clip:
//               tools/probe_pk16.hip); the sum's clip at b1 = 16 is the clamped packed add; the product's clip at b2 = 16 is
//               the saturating pack; change_cfg is a clamped packed multiply by 2^cl and a packed arithmetic shift by cr, one
//               of them the identity (the clip at 16 bits after a right shift never acts).  9 instructions per channel pair.
//   ROW_SHIFTED W16 && r1 >= 1.  The 17-bit sum x + m is formed in 32 bits from the two sign-extended halves; shifted right
//               by r1 >= 1 it is within 16 bits, so the clip at b1 = 16 never acts (b1 >= 17 - r1).  12 per pair.
//   ROW_GENERIC everything else: bn16_x4's operations in bn16_x4's order (bounds as scalar operands: the fallback does not pin
//               eight more registers in a kernel that has none to spare).
// tests/test_gate_urec.py runs tools/probe_bn16_row8.hip: every arm against bn16_x4 on all 65 536 inputs, every shift
// pattern the arm admits, the patterns it must reject, constants on both rails and at zero.
// ---------------------------------------------------------------------------------------------
enum { ROW_GENERIC = 0, ROW_PACKED = 1, ROW_SHIFTED = 2 };
struct Bn16Row {
    uint32_t m[4], iv[4];      // this thread's eight channels: pre-shifted -mean and isv as int16 pairs (channel 2k | 2k+1 << 16)
    int32_t arm;
    uint32_t mulx, mulc, crp;  // 2^shx1, 2^cl and cr in both halves (wave-uniform: SGPR operands)
    int32_t shx1, l1, r1, rs2, cl, cr;
    int32_t xb, b1, b2, cbits;
};

// arm of a chain with these widths and shifts (wave-uniform)
__host__ __device__ __forceinline__ int bn16_row_arm(int xb, int mb, int ib, int b1, int b2, int cbits, int shx1, int l1, int r1, int cl, int cr)
{
    const bool w16 = (xb == 16 || (shx1 == 0 && xb < 16)) && mb <= 16 && ib <= 16 && b1 == 16 && b2 == 16 && cbits == 16 &&
                     shx1 <= 14 && l1 == 0 && cl <= 14 && cr <= 15;
    return !w16 ? ROW_GENERIC : r1 == 0 ? ROW_PACKED : ROW_SHIFTED;
}

// the uniform part: widths, shifts and the arm, from explicit values (the probe) ...
__host__ __device__ __forceinline__ void bn16_row_shifts(Bn16Row &p, int xb, int mb, int ib, int b1, int b2, int cbits, int shx1, int post1, int rs2, int de)
{
    p.shx1 = shx1; p.l1 = post1 > 0 ? post1 : 0; p.r1 = post1 < 0 ? -post1 : 0;
    p.rs2 = rs2;
    p.cl = de > 0 ? de : 0; p.cr = de < 0 ? -de : 0;
    p.xb = xb; p.b1 = b1; p.b2 = b2; p.cbits = cbits;
    p.arm = bn16_row_arm(xb, mb, ib, b1, b2, cbits, p.shx1, p.l1, p.r1, p.cl, p.cr);
    p.mulx = 0x10001u * (1u << (p.shx1 & 15)); p.mulc = 0x10001u * (1u << (p.cl & 15)); p.crp = 0x10001u * (uint32_t)(p.cr & 15);
}

// ... or from a layer's BatchNorm arguments and published exponents, with the operands of the thread's eight channels
// h0 .. h0 + 7.  No scale / bias stage (the caller's plan guarantees it).
__device__ __forceinline__ Bn16Row bn16_row_setup(const BnArgs &a, const LayerDyn &d, int h0)
{
    Bn16Row p;
    bn16_row_shifts(p, a.xb, a.mb, a.ib, a.b1, a.b2, a.out_bits < a.ub ? a.out_bits : a.ub, d.bn1.shx, d.bn1.post, d.rs2, a.ue - d.bn_e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t m0 = sat(wshl(a.mm[h0 + 2 * k], d.bn1.shy), a.mb), m1 = sat(wshl(a.mm[h0 + 2 * k + 1], d.bn1.shy), a.mb);
        p.m[k] = ((uint32_t)m0 & 0xffffu) | ((uint32_t)m1 << 16);
        p.iv[k] = ((uint32_t)a.isv[h0 + 2 * k] & 0xffffu) | ((uint32_t)a.isv[h0 + 2 * k + 1] << 16);
    }
    return p;
}

// ... or, for a kernel whose threads do NOT keep one channel group (the B projection, proj_p.hpp k_bproj_p<.., ROW>): the uniform
// part as above (m and iv stay unset), and the operand pairs of all H channels in LDS -- H/2 words of mean pairs, then H/2 words
// of isv pairs, formed as bn16_row_setup forms m[k] and iv[k]; a thread takes the two 16-byte vectors of its channel group
// og at word 4 * og of either half.  All threads; call before a __syncthreads().
__device__ __forceinline__ Bn16Row bn16_row_table(const BnArgs &a, const LayerDyn &d, int32_t *lds, int H)
{
    Bn16Row p{};
    bn16_row_shifts(p, a.xb, a.mb, a.ib, a.b1, a.b2, a.out_bits < a.ub ? a.out_bits : a.ub, d.bn1.shx, d.bn1.post, d.rs2, a.ue - d.bn_e);
    for (int k = threadIdx.x; k < H / 2; k += blockDim.x) {
        const int32_t m0 = sat(wshl(a.mm[2 * k], d.bn1.shy), a.mb), m1 = sat(wshl(a.mm[2 * k + 1], d.bn1.shy), a.mb);
        lds[k] = (int32_t)(((uint32_t)m0 & 0xffffu) | ((uint32_t)m1 << 16));
        lds[H / 2 + k] = (int32_t)(((uint32_t)a.isv[2 * k] & 0xffffu) | ((uint32_t)a.isv[2 * k + 1] << 16));
    }
    return p;
}

// the B projection's phase A operands in either form: bn16_x4's (Bn16, four LDS tables) or bn16_row8's (Bn16Row, the pair table)
template <bool ROW>
__device__ __forceinline__ auto bn_operands(const BnArgs &a, const LayerDyn &d, int32_t *lds, int H)
{
    if constexpr (ROW) return bn16_row_table(a, d, lds, H);
    else return bn16_setup(a, d, lds, H);
}

// eight consecutive channels of one frame (int16, as loaded) -> their SSM input u (int16, as bn16_x4 + pack4_i16 give it)
template <int ARM>
__device__ __forceinline__ v4i bn16_row8(const Bn16Row &p, const v4i &x)
{
    v4i u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (ARM == ROW_GENERIC) {
            int32_t o[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int32_t xe = e ? x[k] >> 16 : (int32_t)(int16_t)(x[k] & 0xffff);
                const int32_t me = e ? (int32_t)p.m[k] >> 16 : (int32_t)(int16_t)(p.m[k] & 0xffffu);
                const int32_t ie = e ? (int32_t)p.iv[k] >> 16 : (int32_t)(int16_t)(p.iv[k] & 0xffffu);
                const int32_t v = sat(asr(wshl(wadd(sat(wshl(xe, p.shx1), p.xb), me), p.l1), p.r1), p.b1);
                const int32_t t = sat(asr(__mul24(v, ie), p.rs2), p.b2);
                o[e] = sat(asr(wshl(t, p.cl), p.cr), p.cbits);
            }
            u[k] = (int32_t)(((uint32_t)o[0] & 0xffffu) | ((uint32_t)o[1] << 16));
        } else {
            const uint32_t xs = pk_mul_sat_u((uint32_t)x[k], p.mulx); // sat16(x << shx1)
            int32_t t0, t1;
            if constexpr (ARM == ROW_PACKED) {
                const uint32_t v = pk_add_sat(xs, p.m[k]);
                t0 = mul24_hh<0>(v, p.iv[k]); t1 = mul24_hh<1>(v, p.iv[k]);
            } else {
                const int32_t v0 = asr(add_hh<0>(xs, p.m[k]), p.r1), v1 = asr(add_hh<1>(xs, p.m[k]), p.r1);
                t0 = mul24_h<0>(v0, p.iv[k]); t1 = mul24_h<1>(v1, p.iv[k]);
            }
            const uint32_t t = pk_cvt(asr(t0, p.rs2), asr(t1, p.rs2));
            u[k] = (int32_t)pk_ashr_u(pk_mul_sat_u(t, p.mulc), p.crp);
        }
    }
    return u;
}

// ---------------------------------------------------------------------------------------------
// B projection arguments (kernel: proj_p.hpp k_bproj_p)
// ---------------------------------------------------------------------------------------------
struct BprojM2Args {
    BnArgs bn;
    const int16_t *x; // (N,H)
    MfmaW w;
    int32_t *bq;      // native stream
    int16_t *u;       // (N,H) SSM input, for the C projection
    int32_t *tr_bu_re, *tr_bu_im, *tr_pre_s5, *tr_u; // traces (TRACE instantiation only)
    int64_t N;
    int32_t L, TB, H, P;
    int32_t rs_re, rs_im, bre_bits, bim_bits, sh_re, sh_im;
    int32_t t_lo, t_len; // k_bproj_p: the step range this launch covers (StepRange)
    int32_t k_re;        // SM = 2 (pair-native K stream): 2^16 - 2^(16 - A_re_exp), the addend of the negated product
    int32_t no_u;        // != 0: u is not stored -- the gate kernel rebuilds it (mfma_fused.hpp k_cgate_p<.., UREC> or <.., GBN>)
    int32_t live_slots;  // SM = 3 / 1, > 0: only state slots below it are stored (scan_quad.hpp ScanPairLArgs::live_slots)
    // != nullptr: the per-channel extremes of the layer input (ext_reps replicas of 2H floats); every workgroup derives the
    // BatchNorm exponents from them in its prologue (bn_finalize_mm_body), workgroup 0 publishes them
    const float *ext;
    int32_t ext_reps;
    int32_t *status, *status_exps;
    // != nullptr (resid_lazy): x is the previous layer's U plane (uint16) and this is that layer's LayerDyn, whose res.post
    // shifts it: the row vectors go through resolve_u16_pair before the BatchNorm chain
    const LayerDyn *lazy;
};

} // namespace s5
