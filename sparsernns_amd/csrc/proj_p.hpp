// proj_p.hpp -- phase-split projection kernels: element work spread over the whole workgroup, one 32-column
// tile of the matmul per wave.
//
// The per-wave kernels in mfma_proj.hpp / mfma_bn.hpp keep a whole frame tile (all k-steps of byte planes,
// all column tiles of accumulators) in one wave: 200-256 registers, two waves per SIMD, and every stall of
// the serial load -> chain -> MFMA -> epilogue sequence is exposed.  Here a workgroup of four waves owns a
// tile of 64 frames:
//   phase A  all threads: 16-byte coalesced loads of the (64,H) int16 tile, the BatchNorm chain on eight
//            channels per vector, u stored with 16-byte coalesced stores, byte planes into LDS [frame][k];
//   phase B  wave w: column tile w of the matmul for both 32-frame halves.  The MFMA runs as D = X * W
//            (A operand = byte planes from LDS, B operand = this wave's weight columns, held in registers for
//            the whole kernel), so a lane owns ONE output channel and 4-frame groups of it -- exactly one
//            16-byte item of the scan-native stream per (group) and per-channel constants are per-lane
//            registers.
// Planes are double buffered: one barrier per tile, phase A of tile i+1 overlaps phase B of tile i in other
// waves.  ~30 KB LDS and < 128 registers: four workgroups (16 waves) per CU.
#pragma once
// -DS5_PHASE_PROF (tools/prof_phases.py, never in the shipped library): every thread 0 accumulates the shader clock between
// phase marks of k_enc_p (and of k_enc_pf, which shares its body: proj_enc_body.inc).  A mark first touches a register the preceding work produced (a v_cmp into vcc: the hardware interlock makes
// it wait for an MFMA or a load that is still in flight -- a bare s_memtime is hoisted over pure arithmetic by the compiler
// and overtakes pending MFMAs in the hardware), then reads the clock.
#ifdef S5_PHASE_PROF
__device__ long long g_phase_prof[2048 * 8];
// all state in SGPRs (the kernels are at their register cap: per-lane accumulators would spill and the reloads would queue
// behind the prefetch loads); 32-bit deltas are enough for one launch
#define PHASE_DECL unsigned prof_last, prof_a0 = 0, prof_a1 = 0, prof_a2 = 0, prof_a3 = 0, prof_a4 = 0, prof_a5 = 0, prof_a6 = 0, prof_a7 = 0; \
    { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)); prof_last = __builtin_amdgcn_readfirstlane((unsigned)t_); }
#define PHASE_MARK(i, reg) do { unsigned long long t_; asm volatile("v_cmp_eq_u32 vcc, %1, %1\n\ts_nop 0\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(reg) : "memory", "vcc"); \
    const unsigned tl_ = __builtin_amdgcn_readfirstlane((unsigned)t_); prof_a##i = __builtin_amdgcn_readfirstlane(prof_a##i + (tl_ - prof_last)); prof_last = tl_; } while (0)
#define PHASE_DUMP do { if (threadIdx.x == 0 && blockIdx.x < 2048) { long long *o_ = g_phase_prof + blockIdx.x * 8; o_[0] = prof_a0; o_[1] = prof_a1; o_[2] = prof_a2; o_[3] = prof_a3; \
    o_[4] = prof_a4; o_[5] = prof_a5; o_[6] = prof_a6; o_[7] = prof_a7; } } while (0)
#else
#define PHASE_DECL
#define PHASE_MARK(i, reg)
#define PHASE_DUMP
#endif
#include "mfma_bn.hpp"

namespace s5 {

// Channels of a model whose tile kernels run on NT 32-channel tiles.  The N-DNS recipe has H = 12 * blocks with blocks = 4, 8,
// 12, 16 (dim_scale 0.25 .. 1.0): 48, 96, 144, 192 -- every H a multiple of 16, so a row of an (N,H) int16 plane is whole
// 16-byte vectors, and the last tile of 48 and 144 is half empty.  Rows stay dense in memory: the row stride, the vectors per
// frame and the per-channel loops come from this count; the LDS byte planes and tables keep the padded extent 32 * NT, where
// the padded weights, D and biases are zero (pack_mfma), so a pad channel computes 0 and only its loads, stores and
// extremes are masked.
__host__ __device__ constexpr int shape_channels(int NT) { return (NT == 2 || NT == 5) ? 32 * NT - 16 : 32 * NT; }

// the k tail [HC, HP) of the byte planes of ragged shapes: initialised once per workgroup (it multiplies zero weights, so any
// constant is right; what LDS happens to hold is not relied on).  rows x KP bytes per plane, NPLANES planes from `base`.
template <int HC, int HP, int KP>
__device__ __forceinline__ void zero_plane_tail(int8_t *base, int rows)
{
    if constexpr (HC != HP) {
        static_assert(HP - HC == 16, "half a tile");
        for (int i = threadIdx.x; i < rows; i += blockDim.x) *reinterpret_cast<v4i *>(base + i * KP + HC) = v4i{0, 0, 0, 0};
    }
}

// eight values in int32 registers -> byte planes (2 packed registers each), k order preserved
__device__ __forceinline__ void planes8_from_i32(const int32_t (&v)[8], v2i &hi, v2i &lo)
{
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned p01 = perm((unsigned)v[4 * j + 1], (unsigned)v[4 * j], 0x05010400u);
        const unsigned p23 = perm((unsigned)v[4 * j + 3], (unsigned)v[4 * j + 2], 0x05010400u);
        lo[j] = (int)(perm(p23, p01, 0x05040100u) ^ 0x80808080u);
        hi[j] = (int)perm(p23, p01, 0x07060302u);
    }
}

// Tiles of the per-layer kernels are 64 steps of ONE sequence inside a step range [t_lo, t_lo + t_len) (the
// whole sequence, or one chunk of the bproj | scan | cgate pipeline): tile -> (sequence, first step, valid steps)
struct StepRange {
    int32_t t_lo, t_len; // t_lo: a multiple of 64; t_len: any length >= 1 (a sequence's last 4-step block may be partial)
};
template <int FT = 64>
__device__ __forceinline__ void tile_of(int64_t tile, const StepRange &sr, int64_t &b, int &t, int &nvalid)
{
    const int tps = (sr.t_len + FT - 1) / FT;
    b = tile / tps;
    const int tt = (int)(tile - b * tps) * FT;
    t = sr.t_lo + tt;
    nvalid = sr.t_len - tt < FT ? sr.t_len - tt : FT;
}

// The same walk without a division per tile: a workgroup's tiles are gridDim.x apart, so (sequence, tile within it) advances
// by a fixed pair with one carry.  All wave-uniform scalar arithmetic (tile_of's 64-bit division by a run-time value is a
// software routine of some forty instructions, and the tile kernels called it two or three times per tile).
template <int FT = 64>
struct TileWalk {
    int tps, db, dti; // tiles per sequence; gridDim.x = db * tps + dti
    int b, ti;        // current tile: sequence b, tile ti of it
    __device__ __forceinline__ TileWalk(int64_t tile0, const StepRange &sr, unsigned step)
    {
        tps = (sr.t_len + FT - 1) / FT;
        db = (int)(step / (unsigned)tps); dti = (int)(step % (unsigned)tps);
        b = (int)((unsigned)tile0 / (unsigned)tps); ti = (int)((unsigned)tile0 % (unsigned)tps);
    }
    __device__ __forceinline__ void advance()
    {
        b += db; ti += dti;
        if (ti >= tps) { ti -= tps; ++b; }
    }
    __device__ __forceinline__ TileWalk next() const { TileWalk n = *this; n.advance(); return n; }
    __device__ __forceinline__ int t(const StepRange &sr) const { return sr.t_lo + ti * FT; }
    __device__ __forceinline__ int nvalid(const StepRange &sr) const { const int left = sr.t_len - ti * FT; return left < FT ? left : FT; }
};

// SM (stream mode) 0: int32 scan-native items; 1: int16 items (the host has checked that every value fits: Bu bits minus
// the shift to the state exponent <= 16; one item is then 8 bytes); 2: the pair kernel's K stream (scan_quad.hpp):
// K = (Bu << 16) + k in pair-native order, one 16-byte item per producer lane; 3: the LDS-fed pair kernel's int16 Bu
// stream (pair16-native), one 8-byte item per producer lane
// NC: 32-column tiles of [B_re | B_im] (= 2P / 32).  NC == NT: one tile per wave, both 32-frame halves of the tile's 64
// frames; NC == NT / 2 (a layer compacted to its live states, s5fxp_fast.hpp): wave w takes column tile w % NC and the ONE
// half w / NC -- the workgroup keeps its size, so phase A (the bulk of the kernel) is unchanged; NC == NT / 4 (a 128-state
// layer on 32 slots): the same, and the waves with w / NC >= 2 sit phase B out.
// ROW: phase A runs the gate kernel's row chain (mfma_bn.hpp bn16_row8) on the 16-byte vectors as loaded, instead of unpacking
// them for bn16_x4: u comes out as the packed int16 pairs its store and the byte-plane selectors want.  For layers whose
// BatchNorm has no scale / bias stage (host-known: s5fxp_fast.hpp bproj_row); the traced kernels need t (pre_s5) and keep
// bn16_x4.  ROW = false is the code as it was, instruction for instruction (the fallback and the A/B partner: S5FXP_GATE_BN=2).
template <int KS, int NT, bool TRACE, int SM = 0, int NC = NT, bool ROW = false>
// (waves per SIMD the registers are budgeted for: 4; 3 at H = 144, whose grid holds two workgroups per CU anyway
// (s5fxp_fast.hpp FastShape::wide) and whose 5 k-steps of weights do not fit 128 registers next to the prefetch; 2 for the
// traced kernels, which hold the trace pointers as well and are no hot path)
__global__ __launch_bounds__(64 * NT, TRACE ? 2 : KS == 5 ? 3 : 4) void k_bproj_p(BprojM2Args a, GroupOff go)
{
    {
        const int64_t g = blockIdx.y;
        gshift(a.bn.dyn, g * go.ws); gshift(a.bn.xe.dyn, g * go.ws); gshift(a.x, g * go.ws); gshift(a.bq, g * go.ws); gshift(a.u, g * go.ws);
        gshift(a.ext, g * go.ws); gshift(a.status, g * go.status); gshift(a.status_exps, g * go.status);
    }
    static_assert(NC == NT || 2 * NC == NT || 4 * NC == NT, "column tiles per workgroup");
    static_assert(!ROW || !TRACE, "the traced kernels store pre_s5: bn16_x4");
    // H: the real channels (row stride, vectors per frame, BatchNorm operands); HP: the k extent of the byte planes
    constexpr int H = shape_channels(KS), HP = 32 * KS, FT = 64, KP = 32 * KS + 16, PC = 16 * NC, SUB0_STEP = NT / NC; // halves a wave takes: 2 / SUB0_STEP
    constexpr int VPF = H / 8;             // 16-byte vectors per frame
    constexpr int NTHR = 64 * NT;          // one wave per column tile: 256 threads at dim 0.5, 512 at dim 1.0
    constexpr int NV = FT * VPF / NTHR;    // vectors per thread and tile
    constexpr int NCT = 1;                 // column tiles per wave
    constexpr int PLANE = FT * KP;
    static_assert(FT * VPF % NTHR == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) int8_t smem[];
    int32_t *tab = reinterpret_cast<int32_t *>(smem);             // 4*H BatchNorm operands (ROW: H words of packed pairs)
    int8_t *Xh = smem + 16 * HP, *Xl = Xh + 2 * PLANE;            // [buf][frame][KP]
    zero_plane_tail<H, HP, KP>(Xh, 4 * FT);                       // (visible behind the barrier below)
    const int l = threadIdx.x & 63, r = l & 31, h = l >> 5, wave = threadIdx.x >> 6;
    const int wct = wave % NC, wsub = wave / NC; // this wave's column tile and first 32-frame half
    const StepRange sr{a.t_lo, a.t_len};
    const int64_t tiles = (a.N / a.L) * ((sr.t_len + FT - 1) / FT);
    int64_t tile = blockIdx.x;

    // The two bn16_x4 kernels of the uncompacted H = 192 layer on the pair streams sit at their 128 registers with the prefetch's
    // three per-thread row offsets kept across the tile loop, two of them in scratch (20 bytes per lane, reloaded per tile).
    // There the thread index is hidden from the compiler inside fetch, so that the offsets are formed again per tile (a
    // multiply, a shift and a subtraction each) and nothing spills; every other instantiation keeps its code.
    constexpr bool REFETCH = KS == 6 && NC == 8 && SM >= 2 && !TRACE && !ROW;
    v4i raw[NV];
    auto fetch = [&](const TileWalk<FT> &tw) {
        const int64_t b = tw.b;
        const int t = tw.t(sr), nv = tw.nvalid(sr);
        const char *xb = reinterpret_cast<const char *>(a.x + (b * a.L + t) * H); // wave-uniform; 32-bit byte offsets from here
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            int v;
            if constexpr (REFETCH) {
                unsigned tid = threadIdx.x;
                asm volatile("" : "+v"(tid));
                v = tid + NTHR * i;
            } else v = threadIdx.x + NTHR * i;
            int f = v / VPF;
            f = f < nv ? f : nv - 1;
            raw[i] = *reinterpret_cast<const v4i *>(xb + 2u * (unsigned)(f * H + 8 * (v % VPF)));
        }
    };
    TileWalk<FT> walk(tile, sr, gridDim.x);
    if (tile < tiles) fetch(walk);
    // this wave's weight columns (B operand) and per-channel constants stay in registers
    v4i wreg[NCT][KS];
    int32_t csv[NCT];
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
        const int col = 32 * (wct + NC * c) + r;
        csv[c] = a.w.cs128[col];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            wreg[c][ks] = *reinterpret_cast<const v4i *>(a.w.wt + (size_t)col * a.w.Kp + 32 * ks + 16 * h);
    }
    // The BatchNorm exponents of this layer: read from *dyn, or -- single-rank forwards -- derived here, by every
    // workgroup for itself, from the per-channel extremes the producer of the layer input left behind (the first tile's
    // loads are in flight meanwhile).  A single workgroup doing this at the tail of the producer kernel cost 4-7 us of
    // serialised round trips (atomics -> ticket -> loads -> arithmetic) on the critical path between two layers.
    const LayerDyn d = a.ext ? bn_finalize_mm_body(a.bn, a.ext, H, const_cast<LayerDyn *>(a.bn.dyn), a.status, a.status_exps, a.bn.xe.get(), a.ext_reps,
                                                   blockIdx.x == 0)
                             : *a.bn.dyn;
    // (ROW: a Bn16Row -- the shifts and the arm; the operand pairs of every channel group are in `tab`)
    const std::conditional_t<ROW, Bn16Row, Bn16> bn = bn_operands<ROW>(a.bn, d, tab, H);
    // resid_lazy (mfma_bn.hpp ResolveU16): the rows are the previous layer's aligned sum U; that layer's residual pass has
    // published the shift that makes them the layer input.  0: plain rows; otherwise 1 + the arm, chosen once per workgroup
    // (the route exists where the gate kernel that stores U does: H = 96; the other shapes keep their code)
    constexpr bool LAZY = KS == 3 && !TRACE;
    ResolveU16 rz{};
    int lazy_arm = 0;
    if constexpr (LAZY) {
        if (a.lazy) {
            gshift_nn(a.lazy, (int64_t)blockIdx.y * go.ws);
            rz = resolve_u16_setup(a.lazy->res.post);
            lazy_arm = 1 + rz.arm;
        }
    }
    __syncthreads();

    prologue_loads_done();
    for (int it = 0; tile < tiles; tile += gridDim.x, ++it, walk.advance()) {
        const int64_t b0 = walk.b;
        const int t0 = walk.t(sr), nvalid = walk.nvalid(sr);
        const int64_t n0 = b0 * a.L + t0;
        char *ub = reinterpret_cast<char *>(a.u + n0 * H); // wave-uniform base of this tile's rows of u
        int8_t *xh = Xh + (it & 1) * PLANE, *xl = Xl + (it & 1) * PLANE;
        // ---- phase A: BatchNorm chain, u, byte planes
        if constexpr (ROW) {
            // ROW: phase A of one tile.  ARM (mfma_bn.hpp ROW_*) is wave-uniform and chosen once per tile, as in the gate kernel
            // (mfma_fused_body.inc tiles_in_urec).  A thread's NV vectors are NV different channel groups (NTHR is no multiple of
            // VPF), so each takes its operand pairs from the table: two 16-byte LDS reads where bn16_x4 makes four.  u = bn16_row8 is
            // pack4_i16 of bn16_x4's u (tools/probe_bn16_row8.hip), so it is stored as it is, and the byte planes take the low and the
            // high bytes of the pairs with the selectors of the gate kernel's X1 planes.
            auto phase_a_row = [&](auto arm_c) {
                constexpr int ARM = decltype(arm_c)::value;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int v = threadIdx.x + NTHR * i, f = v / VPF, og = v % VPF;
                    if constexpr (LAZY) {
                        if (lazy_arm == 1 + RES_RIGHT) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) raw[i][e] = (int)resolve_u16_pair<RES_RIGHT>(rz, (uint32_t)raw[i][e]);
                        } else if (lazy_arm) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) raw[i][e] = (int)resolve_u16_pair<RES_GENERIC>(rz, (uint32_t)raw[i][e]);
                        }
                    }
                    const v4i bm = *reinterpret_cast<const v4i *>(tab + 4 * og), bi = *reinterpret_cast<const v4i *>(tab + H / 2 + 4 * og);
                    auto br = bn;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { br.m[k] = (uint32_t)bm[k]; br.iv[k] = (uint32_t)bi[k]; }
                    const v4i uv = bn16_row8<ARM>(br, raw[i]);
                    if (f < nvalid && !a.no_u) *reinterpret_cast<v4i *>(ub + 2u * (unsigned)(f * H + 8 * og)) = uv;
                    v2i hi, lo;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        lo[j] = (int)(perm((unsigned)uv[2 * j + 1], (unsigned)uv[2 * j], 0x06040200u) ^ 0x80808080u);
                        hi[j] = (int)perm((unsigned)uv[2 * j + 1], (unsigned)uv[2 * j], 0x07050301u);
                    }
                    *reinterpret_cast<v2i *>(xh + f * KP + 8 * og) = hi;
                    *reinterpret_cast<v2i *>(xl + f * KP + 8 * og) = lo;
                }
            };
            if (bn.arm == ROW_PACKED) phase_a_row(std::integral_constant<int, ROW_PACKED>{});
            else if (bn.arm == ROW_SHIFTED) phase_a_row(std::integral_constant<int, ROW_SHIFTED>{});
            else phase_a_row(std::integral_constant<int, ROW_GENERIC>{});
        } else
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = threadIdx.x + NTHR * i, f = v / VPF, og = v % VPF;
            const int64_t n = n0 + f;
            int32_t xin[8], t[8], u[8];
            if constexpr (LAZY) {
                if (lazy_arm == 1 + RES_RIGHT) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) raw[i][e] = (int)resolve_u16_pair<RES_RIGHT>(rz, (uint32_t)raw[i][e]);
                } else if (lazy_arm) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) raw[i][e] = (int)resolve_u16_pair<RES_GENERIC>(rz, (uint32_t)raw[i][e]);
                }
            }
            unpack8_i16(raw[i], xin);
            bn16_x4(bn, reinterpret_cast<const int32_t(&)[4]>(xin[0]), 8 * og, reinterpret_cast<int32_t(&)[4]>(t[0]),
                    reinterpret_cast<int32_t(&)[4]>(u[0]));
            bn16_x4(bn, reinterpret_cast<const int32_t(&)[4]>(xin[4]), 8 * og + 4, reinterpret_cast<int32_t(&)[4]>(t[4]),
                    reinterpret_cast<int32_t(&)[4]>(u[4]));
            if (f < nvalid && (TRACE || !a.no_u)) {
                const v2i p0 = pack4_i16(u[0], u[1], u[2], u[3]), p1 = pack4_i16(u[4], u[5], u[6], u[7]);
                *reinterpret_cast<v4i *>(ub + 2u * (unsigned)(f * H + 8 * og)) = v4i{p0[0], p0[1], p1[0], p1[1]};
                if (TRACE) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (a.tr_pre_s5) a.tr_pre_s5[n * H + 8 * og + e] = t[e];
                        if (a.tr_u) a.tr_u[n * H + 8 * og + e] = u[e];
                    }
                }
            }
            v2i hi, lo;
            planes8_from_i32(u, hi, lo);
            *reinterpret_cast<v2i *>(xh + f * KP + 8 * og) = hi;
            *reinterpret_cast<v2i *>(xl + f * KP + 8 * og) = lo;
        }
        if (tile + gridDim.x < tiles) fetch(walk.next()); // in flight during phase B
        __syncthreads();
        // ---- phase B: this wave's column tile(s), both 32-frame halves
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            const int col = 32 * (wct + NC * c) + r;
            // SM >= 2: the weight columns are packed so that lanes r and r ^ 16 hold re and im of the SAME state
            // (pack_fast: bproj_pair); otherwise columns [0, P) are re, [P, 2P) im
            const int cc = SM >= 2 ? (r >> 4) : (col >= PC ? 1 : 0), p = SM >= 2 ? 16 * (wct + NC * c) + (r & 15) : col - cc * PC;
            const int rs = cc ? a.rs_im : a.rs_re, bits = cc ? a.bim_bits : a.bre_bits, sh = cc ? a.sh_im : a.sh_re;
            const int lsh = sh < 0 ? -sh : 0, rsh = sh > 0 ? sh : 0;
            SatB sbu; // this lane's clip bounds (re or im width), pinned in registers: not recomputed per element
            sbu.hi = (int32_t)((1u << (bits - 1)) - 1u); sbu.lo = ~sbu.hi;
            asm volatile("" : "+v"(sbu.lo), "+v"(sbu.hi));
#pragma unroll
            for (int sub0 = 0; sub0 < 2; sub0 += SUB0_STEP) {
                const int sub = sub0 + wsub;
                if (SUB0_STEP > 2 && sub >= 2) break; // a quarter of the column tiles: half of the waves have no unit in phase B
                const int8_t *rowh = xh + (32 * sub + r) * KP + 16 * h, *rowl = xl + (32 * sub + r) * KP + 16 * h;
                v16i acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const v4i *>(rowh + 32 * ks), wreg[c][ks], acc, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = wadd(wshl(acc[i], 8), csv[c]);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const v4i *>(rowl + 32 * ks), wreg[c][ks], acc, 0, 0, 0);
                // rows (frames) (i&3) + 8*(i>>2) + 4*h of this half: registers 4g..4g+3 are one 4-step block
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int o = 32 * sub + 8 * g + 4 * h;
                    // only the stores are guarded: with the arithmetic inside the branch the four groups of a lane run one
                    // after the other, each a short dependent chain, and three waves per SIMD do not hide that
                    const bool live = o < nvalid;
                    {
                        v4i q;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int32_t bu = sat(asr(acc[4 * g + e], rs), sbu);
                            q[e] = asr(wshl(bu, lsh), rsh);
                            if (TRACE && o + e < nvalid) {
                                if (!cc && a.tr_bu_re) a.tr_bu_re[(n0 + o + e) * PC + p] = bu;
                                if (cc && a.tr_bu_im) a.tr_bu_im[(n0 + o + e) * PC + p] = bu;
                            }
                        }
                        if (SM == 3) {
                            // the same item as SM == 2 (steps 0 and 2 from the other component's lane), as plain int16 Bu: the
                            // recurrence kernel's helper wave forms K.  h = 0 / 1 lanes hold the two blocks of a pair, so one
                            // wave store fills 512 contiguous bytes
                            const int32_t o0 = __builtin_amdgcn_ds_swizzle(q[0], 0x401f), o2 = __builtin_amdgcn_ds_swizzle(q[2], 0x401f);
                            const v2i item = pack4_i16(o0, o2, q[1], q[3]);
                            // pair16_half(b0, (t0 + o) >> 2, p, cc): the tile's first block of state group 0 is the uniform base
                            if (live && (a.live_slots <= 0 || p < a.live_slots)) {
                                char *qb = reinterpret_cast<char *>(reinterpret_cast<int16_t *>(a.bq) + pair16_half(b0, t0 >> 2, 0, 0, a.TB, PC));
                                const unsigned qo = 2u * (unsigned)((((((p >> 5) * (a.TB >> 1) + (o >> 3)) << 6) + 2 * (p & 31) + cc) * 8) + 4 * ((o >> 2) & 1));
                                *reinterpret_cast<v2i *>(qb + qo) = item;
                            }
                        } else if (SM == 2) {
                            // K = (Bu << 16) + k.  Pair-native items: lane A = [Kim0 Kim2 Kre1 Kre3], lane B = [Kre0 Kre2
                            // Kim1 Kim3]: steps 0 and 2 come from the OTHER component's lane (r ^ 16, ds_swizzle), steps 1
                            // and 3 are this lane's own; the re lane writes item A, the im lane item B -- one 16-byte store
                            // each, 512 contiguous bytes per half wave
                            const int32_t kc = cc ? 0 : a.k_re;
                            const int32_t k0 = wadd(wshl(q[0], 16), kc), k2 = wadd(wshl(q[2], 16), kc);
                            v4i item;
                            item[0] = __builtin_amdgcn_ds_swizzle(k0, 0x401f);
                            item[1] = __builtin_amdgcn_ds_swizzle(k2, 0x401f);
                            item[2] = wadd(wshl(q[1], 16), kc);
                            item[3] = wadd(wshl(q[3], 16), kc);
                            if (live) *reinterpret_cast<v4i *>(a.bq + pair_word(b0, (t0 + o) >> 2, p, a.TB, PC) + 4 * cc) = item;
                        } else if (SM == 1) {
                            if (live && (a.live_slots <= 0 || p < a.live_slots))
                                *reinterpret_cast<v2i *>(reinterpret_cast<int16_t *>(a.bq) + native_word(b0, t0 + o, p, cc, a.TB, PC)) =
                                    pack4_i16(q[0], q[1], q[2], q[3]);
                        } else if (live)
                            *reinterpret_cast<v4i *>(a.bq + native_word(b0, t0 + o, p, cc, a.TB, PC)) = q;
                    }
                }
            }
        }
    }
}

// uniform operands of a change_cfg (fxp_prims.hpp chcfg) applied to many elements; `on` false = identity
using v2u16 = __attribute__((ext_vector_type(2))) unsigned short;

struct CfgOp {
    int l, r, b;
    SatB sb; // the clip bounds in VGPRs (fxp_prims.hpp sat_bounds): make_cfg is called once per kernel
    __device__ __forceinline__ int32_t operator()(int32_t d) const { return sat(asr(wshl(d, l), r), sb); }
};
__device__ __forceinline__ CfgOp make_cfg(bool on, int bits, int e, int bits2, int e2)
{
    CfgOp c;
    c.l = on && e2 > e ? e2 - e : 0;
    c.r = on && e > e2 ? e - e2 : 0;
    const int b1 = on && e2 != e ? bits : 32, b2 = on && bits > bits2 ? bits2 : 32;
    c.b = b1 < b2 ? b1 : b2;
    c.sb = sat_bounds(c.b);
    return c;
}

// two-plane MFMA, A operand (weights, rows = channels) in registers, B operand (byte planes) from LDS:
// lane = frame, registers = channels (i&3) + 8*(i>>2) + 4*(lane>>5) of the 32-channel tile
template <int KSTEPS>
__device__ __forceinline__ void mfma_planes(v16i &acc, const v4i (&w)[KSTEPS], const int8_t *rowh, const int8_t *rowl,
                                            const int32_t *cs)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[ks], *reinterpret_cast<const v4i *>(rowh + 32 * ks), acc, 0, 0, 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const v4i c = *reinterpret_cast<const v4i *>(cs + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * g + e] = wadd(wshl(acc[4 * g + e], 8), c[e]);
    }
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[ks], *reinterpret_cast<const v4i *>(rowl + 32 * ks), acc, 0, 0, 0);
}

// the same for NPL byte planes [plane][frame][k] (plane NPL-1 = signed top byte), Horner from the top: the constant
// 128*sum(w) enters at every shift, so after NPL-1 shifts it has the weight 2^(8(NPL-2)) + ... + 2^8 + 1 that the
// +128 offsets of the lower planes need
template <int KSTEPS, int NPL>
__device__ __forceinline__ void mfma_nplanes(v16i &acc, const v4i (&w)[KSTEPS], const int8_t *row0, int plane_stride,
                                             const int32_t *cs)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
    for (int pl = NPL - 1; pl >= 0; --pl) {
        if (pl != NPL - 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i c = *reinterpret_cast<const v4i *>(cs + 8 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g + e] = wadd(wshl(acc[4 * g + e], 8), c[e]);
            }
        }
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[ks], *reinterpret_cast<const v4i *>(row0 + pl * plane_stride + 32 * ks), acc, 0, 0, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Encoder, phase-split: x int32 (N,K) -> relu(dense) int16 (N,H).  fxpmodel.py:331-366, 1263-1266.
// Six waves, 64-frame tiles.  Phase A: a wave reads whole rows (64 lanes x 4 consecutive k, 1 KB contiguous)
// plus the K-256 tail, converts, and writes byte planes [frame][304]; phase B: wave (half, column tile).
// ext != nullptr: the per-channel extremes of the output (layer 0's BatchNorm operand, mfma_bn.hpp) are gathered
// on the way -- a lane keeps (max, 65535 - min) of its 16 channels as packed u16 pairs (the output is >= 0 after
// the ReLU); the atomics are spread over ext_reps replicas (mfma_bn.hpp EXT_REPS).
// LDS: [cs128 Np][bias_eff Np][X hi][X lo][ext hi H][ext lo H]
// ---------------------------------------------------------------------------------------------
// The element type of the model boundary (x of the encoder, y of the decoder): one body per kernel, shared as text, with the
// type as a compile-time constant.
enum { IO_I32 = 0, IO_F32 = 1, IO_I16 = 2 };

template <int NT>
__global__ __launch_bounds__(384, 3) void k_enc_p(EncArgs a, float *ext, int ext_reps, GroupOff go)
{
    constexpr int IO = IO_I32;
#include "proj_enc_body.inc"
}

// k_enc_p for a float32 input (s5fxp_model_forward_f32): a.x holds float rows -- the same 4 bytes per element, so loads,
// LDS and stores are k_enc_p's.  Each element is first quantised to (xb, xe) as fxp_from_fp with FLOOR does it
// (fxprun.py:69-75, fxp_prims.hpp fromfp), then takes k_enc_p's change_cfg and int16 check.  The body is shared as text,
// not as a function: with it in a forceinline function template called from thin kernels all 24 encoder / decoder kernels
// compiled to other code (4 to 238 instructions each, the int ones included), with the include every kernel of the library
// keeps its instruction stream (tools/disasm_compare.py) -- these kernels sit at their register caps and wait by
// hand-counted vmcnt.
template <int NT>
__global__ __launch_bounds__(384, 3) void k_enc_pf(EncArgs a, float *ext, int ext_reps, GroupOff go)
{
    constexpr int IO = IO_F32;
#include "proj_enc_body.inc"
}

// k_enc_p for an int16 input (s5fxp_model_forward_i16): a.x holds int16 rows of 2 K bytes, 2-byte aligned.  A lane's four
// elements are two dwords, loaded as they lie (gload8_hidden): with the input at the encoder's configuration they are the
// operands of the byte-plane perms as loaded, otherwise they are sign-extended for the change_cfg first.  Every value is an
// int16, so the wide-input check has nothing to find.  LDS, phase B, its stores and the vm_wait counts are k_enc_p's.
template <int NT>
__global__ __launch_bounds__(384, 3) void k_enc_ps(EncArgs a, float *ext, int ext_reps, GroupOff go)
{
    constexpr int IO = IO_I16;
#include "proj_enc_body.inc"
}

// ---------------------------------------------------------------------------------------------
// Decoder, phase-split: h int16 (N,H) -> dense int32 (N,M), M <= 288.  fxpmodel.py:331-366, 1272-1274.
// Six waves, 64-frame tiles.  Phase B runs as D = X * W (lane = output column, registers = frames) and writes its values into
// an LDS image of the tile's block of y; behind the closing barrier the whole workgroup moves the block out as 16-byte
// vectors, 1 KB of consecutive addresses per wave instruction (proj_dec_body.inc).
// LDS: [X hi][X lo][Y tile: 64 x M output elements]
// ---------------------------------------------------------------------------------------------
// A 16-byte vector at the alignment of an output element: the copy-out's stores assume no more of a tile's base.
typedef v4i v16y_4 __attribute__((aligned(4)));
typedef v4i v16y_2 __attribute__((aligned(2)));
// dynamic LDS of a decoder workgroup (KS: k-steps of the byte planes, io: the boundary's element type): the two byte planes
// and the output tile
__host__ __device__ constexpr size_t dec_lds_bytes(int KS, int io, int M)
{
    return 2 * 64 * (size_t)(32 * KS + 16) + 64 * (size_t)M * (io == IO_I16 ? 2 : 4);
}
// whether two decoder workgroups share a CU's 160 KB of LDS (the RESID kernels hold 16 static bytes on top of the dynamic ones)
constexpr size_t CU_LDS_BYTES = 160 * 1024, DEC_STATIC_LDS = 16;
__host__ __device__ constexpr bool dec_two_per_cu(size_t dynamic_lds) { return 2 * (dynamic_lds + DEC_STATIC_LDS) <= CU_LDS_BYTES; }
// RESID: the last layer's residual pass (mfma_bn.hpp k_resid_minmax16 without its extremes, which nobody needs after the
// last layer) happens here, on the way in: a.x is the layer's INPUT (skip), rz.z the gate kernel's output, and
// h = relu(z + skip) (fxpmodel.py:1147-1159) is formed in registers -- the h plane is neither written nor read back
// (-75 + 25 MB per batch at configs[1]) and the forward is one launch shorter.  The residual exponents come from the
// maxima the gate kernel left, derived by every workgroup for itself as in the B projection.
// usum (s5fxp_fast.hpp LayerPlan::resid_fold): the gate kernel stored the add's aligned sum U (mfma_bn.hpp SumU16) in z's place;
// a.x is that plane, the only one read (25 MB per batch instead of 50), and h = resolve_u16(U).
struct DecResid {
    const int16_t *z;
    ResidHead hd;
    int32_t res_bits, skip_bits;
    int32_t usum;
};
// (Registers: budgeted for three waves per SIMD, two workgroups per CU -- what the launcher's grid asks for and, with a 4-byte
// output tile at H <= 96, what the LDS holds; for two waves per SIMD where the tile leaves room for one workgroup, and at
// KS = 6 with the residual pass or an int16 output, whose weights and prefetch do not fit 168 registers.)
__host__ __device__ constexpr int dec_waves(int KS, bool RESID, int io)
{
    return (KS == 6 && (RESID || io == IO_I16)) || (io != IO_I16 && KS >= 5) ? 2 : 3;
}
template <int KS, bool RESID = false>
__global__ __launch_bounds__(384, dec_waves(KS, RESID, IO_I32)) void k_dec_p(DecArgs a, DecResid rz, GroupOff go)
{
    constexpr int IO = IO_I32;
#include "proj_dec_body.inc"
}

// k_dec_p with a float32 output (s5fxp_model_forward_f32): every value goes into the tile as to_float of k_dec_p's result
// (fxparray.py:72-73, fxp_prims.hpp tofloat, rounded as k_to_float rounds), the same 4 bytes per value, so the tile, the
// copy-out and its store count are k_dec_p's.  One body, shared as text for the reason given at k_enc_pf.
template <int KS, bool RESID>
__global__ __launch_bounds__(384, dec_waves(KS, RESID, IO_F32)) void k_dec_pf(DecArgs a, DecResid rz, GroupOff go)
{
    constexpr int IO = IO_F32;
#include "proj_dec_body.inc"
}

// k_dec_p with an int16 output (s5fxp_model_forward_i16; the host has checked out_bits <= 16, so the narrowing loses
// nothing): one 2-byte LDS store per value into a tile of half the size (pitch 2 M bytes), and half as many 16-byte vectors
// in the copy-out, at 2-byte alignment.
template <int KS, bool RESID>
__global__ __launch_bounds__(384, dec_waves(KS, RESID, IO_I16)) void k_dec_ps(DecArgs a, DecResid rz, GroupOff go)
{
    constexpr int IO = IO_I16;
#include "proj_dec_body.inc"
}


} // namespace s5
