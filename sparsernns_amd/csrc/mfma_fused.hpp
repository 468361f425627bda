// mfma_fused.hpp -- C projection, D*u, ReLU, out2 dense, LUT sigmoid and mult_gate in ONE kernel.
//
// fxpmodel.py:740-793 (C projection, x2, + D*u), :1125 (ReLU), :1133-1137 (out2, sigmoid, gate), plus the
// float32 maxima of the residual compute_best add (:1147-1152).
//
// Kernel: k_cgate_p (phase-split, see the comment block in front of it); redo / multi-rank helpers.
#pragma once
#include "proj_p.hpp"

namespace s5 {

using v2i16 = __attribute__((ext_vector_type(2))) short;

struct CGateArgs {
    const int16_t *u;    // (N,H) SSM input (written by the B projection)
    BnArgs bn;           // GBN instantiations: this layer's BatchNorm; u is recomputed from `skip` and `u` is not read
    const int16_t *skip; // (N,H) layer input
    const int32_t *xs;   // native raw states
    MfmaW w_re, w_im;    // H channels each, K = P
    MfmaW w_o2;          // H channels, K = H, k-permuted
    const int32_t *D;    // (Np)
    const int32_t *bias_eff; // (Np) out2 bias at out_exp
    int16_t *z;          // (N,H)
    int32_t *tr_ys, *tr_out2, *tr_sig, *tr_z; // traces (TRACE instantiation only)
    int64_t N;
    int32_t L, TB, H;
    int32_t rs_re, rs_im, rs_d, y_bits, y_exp;
    int32_t xmax;
    int32_t conv, inp_bits, inp_exp, rs_o2, out_bits, out_exp;
    int32_t sig_x, sig_y;
    int32_t lut[8];
    int32_t l_bits, l_exp, r_bits, r_exp, res_bits, res_exp, rs_gate;
    DynExp skip_e;
    LayerDyn *dynw;
    int32_t *status;
    int32_t bad_bits; // status bits raised when a state is out of range (k_cgate_p)
    int32_t live_slots; // S16, > 0: state slots at or above it are zero and not in the stream (scan_quad.hpp ScanPairLArgs)
    int32_t t_lo, t_len; // k_cgate_p: the step range this launch covers (StepRange)
    const int32_t *sigtab; // [2][7 << sig_x]: gate operand r for a non-positive / positive sigmoid input (k_cgate_p)
    const int32_t *run_if; // WIDE (exact re-run): do the work only when *run_if != 0 (nullptr: always)
    int32_t mx_slot;       // first of the three LayerDyn::mx slots that receive the maxima (8; 11 for the re-run)
    const int16_t *sigdir; // DIRECT: [1 << sigdir_bits] gate operand r for every value of (gq >> (out_exp - sig_x))
    int32_t sigdir_bits;
};

// multi-rank mode only: the residual maxima of a re-run layer live in slots 11..13; move them to 8..10, the
// slots the ranks exchange
__global__ void k_select_maxima(LayerDyn *d)
{
    if (threadIdx.x < 3 && blockIdx.x == 0 && d->redo) d->mx[8 + threadIdx.x] = d->mx[11 + threadIdx.x];
}

// ---------------------------------------------------------------------------------------------
// Phase-split version (see proj_p.hpp for the idea).  Workgroup = one wave per (32-frame half, 32-channel tile): four, six,
// ten, twelve waves at H = 48, 96, 144, 192; tile = 64 frames:
//   A   all threads: one 32-byte stream item (state p, 4 steps, re+im) per thread -> range check, complex
//       ReLU, 4x4 transpose inside the lane quad (DPP) so that a lane holds 4 consecutive states of ONE
//       frame -> byte planes S[frame][re P | im P] in LDS;
//   B1  wave (half, ct): C projection of its 32 channels x 32 frames, weights in registers, epilogue ->
//       x1 (kept in registers for the gate) and its byte planes X1[frame][H] in LDS;
//   B2  the same wave: out2 for the same channels/frames from the X1 planes (natural k order), LUT sigmoid,
//       gate, int16 store, residual maxima.
// No weights in LDS (35 KB at dim 0.5, 65 KB at dim 1.0), ~128 registers.
// LDS: [cs_re][cs_im][D][cs_out2][bias_eff] (Np ints each) [lut pairs 8] [S hi][S lo][X1 hi][X1 lo] [red 3x16]
// ---------------------------------------------------------------------------------------------
// The barriers between the phases order LDS traffic only (planes written by some waves, read by others).  __syncthreads()
// is a fence + barrier and the fence waits for EVERY outstanding memory operation (s_waitcnt vmcnt(0)): the loads requested
// a tile ahead would be drained at the next barrier.  This one waits for the wave's LDS operations and nothing else.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int CTRL>
__device__ __forceinline__ int32_t quad_xchg(int32_t v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

// 4x4 transpose of w[0..3] across the four lanes of a quad: lane q's w[j] <-> lane j's w[q]
__device__ __forceinline__ void quad_transpose(int32_t (&w)[4], int lane)
{
    const bool b0 = lane & 1, b1 = lane & 2;
    { // bit 0: register pairs (0,1), (2,3); partner = lane ^ 1
        const int32_t r01 = quad_xchg<0xB1>(b0 ? w[0] : w[1]), r23 = quad_xchg<0xB1>(b0 ? w[2] : w[3]);
        w[0] = b0 ? r01 : w[0]; w[1] = b0 ? w[1] : r01;
        w[2] = b0 ? r23 : w[2]; w[3] = b0 ? w[3] : r23;
    }
    { // bit 1: register pairs (0,2), (1,3); partner = lane ^ 2
        const int32_t r02 = quad_xchg<0x4E>(b1 ? w[0] : w[2]), r13 = quad_xchg<0x4E>(b1 ? w[1] : w[3]);
        w[0] = b1 ? r02 : w[0]; w[2] = b1 ? w[2] : r02;
        w[1] = b1 ? r13 : w[1]; w[3] = b1 ? w[3] : r13;
    }
}

// (the packed 16-bit helpers of the PK16 epilogues -- pk_cvt, pk_add_sat, mul24_h, ... -- live in mfma_bn.hpp: the row-layout
// BatchNorm chain bn16_row8 uses them as well)

constexpr int SIGTAB_WORDS = 2 * 7 * 64; // sig_x <= 6 on this path (host-checked)
constexpr int SIGDIR_MAX_BITS = 12, SIGDIR_BYTES = 2 << SIGDIR_MAX_BITS;
__host__ __device__ __forceinline__ int sigdir_lds_bytes(int bits) { return ((2 << bits) + 15) & ~15; }

// The argument block of the k_cgate_p overload that stores the aligned sum (FOLD below).
// skip_dyn != nullptr (resid_lazy): `skip` is the previous layer's U plane, not its shifted copy, and this is
// that layer's LayerDyn: every skip row vector goes through resolve_u16_pair (mfma_bn.hpp) with its res.post before it feeds
// bn16_row8 and the skip tile, so that everything downstream sees the layer input as before.
// ext_next != nullptr (gate_ext): the next layer's block of per-channel extremes (mfma_bn.hpp EXT_REPS replicas of
// 2H biased floats).  The kernel gathers the extremes of the U it stores -- packed uint16 running minima / maxima of the thread's
// eight channels, valid frames only -- folds them through the dead tiles at its end and leaves them there IN U UNITS, one
// atomicMax per (bound, channel) and workgroup; the head-only residual pass (mfma_bn.hpp ResidLazyArgs::head_only) turns them
// into the extremes of the layer input.  nullptr: the last layer (its U goes to the decoder) and every route that reads the plane.
struct CGateFoldArgs : CGateArgs {
    const LayerDyn *skip_dyn;
    float *ext_next;
};
__device__ __forceinline__ const LayerDyn *skip_dyn_of(const CGateArgs &) { return nullptr; }
__device__ __forceinline__ const LayerDyn *skip_dyn_of(const CGateFoldArgs &a) { return a.skip_dyn; }
__device__ __forceinline__ float *ext_next_of(const CGateArgs &) { return nullptr; }
__device__ __forceinline__ float *ext_next_of(const CGateFoldArgs &a) { return a.ext_next; }

// S16: the state stream holds int16, written with saturation by k_scan_quad_asm16 (a.xmax <= 32766 then: a saturated
// state fails the range check like any other state beyond the bound)
// DIRECT: the sigmoid input xx = gq >> (out_exp - sig_x) has only out_bits - (out_exp - sig_x) <= 12 bits, so r is read
// from a table over xx itself (no |xx|, segment index, remainder or sign logic at all)
// FTP: frames per tile, 64 (two 32-frame halves, 2*NT waves) or 32 (NT waves: smaller workgroups, more of them per CU)
// WIDE: the exact variant for states of any width (the re-run behind the range check): int32 states are split into
// FOUR byte planes, a = b3*2^24 + (b2'+128)*2^16 + (b1'+128)*2^8 + (b0'+128) with b3 signed and b' = byte ^ 0x80, so
// sum a*w = Horner over four MFMA passes with the same per-channel constant 128*sum(w) added at each of the three shifts
// -- all modulo 2^32, which is the reference's int32 matmul (fxparray.py:662).  No range check, complex ReLU through
// float32 exactly as the reference does it (fxp_prims.hpp crelu).
// PAIR (with S16): the states come from k_scan_pair_asm in pair-native order (scan_quad.hpp)
// PK16 (with DIRECT): y, out2 output, the gate's l operand and its result are all 16 bit, no out2 input conversion and
// every |bias_eff| fits 16 bits (host-checked, s5fxp_fast.hpp): both epilogues run on packed int16 pairs -- saturating
// packs, clamped packed sub / mad / add, SDWA half-word operands -- about a third fewer VALU instructions, same results
// GBN (with PK16): the SSM input u = BatchNorm(layer input) is recomputed here from `skip` -- the layer input this kernel reads
// anyway for the residual maxima -- with the exponents the B projection left in LayerDyn, instead of being written by the B
// projection and read back: -2 x N x H x 2 bytes of traffic per layer for ~12 more VALU operations per element (mfma_bn.hpp bn16_x4)
// UREC (with COAL, see below: PK16 && !TRACE && !WIDE && !GBN): the same idea where it costs least.  The tile staging
// (tiles_in_out) holds each thread's 16-byte row vectors of `skip` with no accumulator live, and a thread's eight channels are
// the same for every vector and tile (NTHR is a multiple of the vectors per frame), so their BatchNorm operands stay in eight
// registers for the whole kernel and the u tile is filled with bn16_row8(skip row) (mfma_bn.hpp) instead of a loaded row: no u
// loads, no LDS table, epilogues and barriers unchanged.  The B projection then does not store u (BprojM2Args::no_u).
// FOLD (with UREC; the k_cgate_p overload that takes CGateFoldArgs): the residual add's aligned sum goes out where z went.  When
// a thread moves its vectors of z(t) out of the z tile, the same position of the skip tile still holds skip(t) -- that thread
// overwrites it with skip(t + 1) only afterwards -- so one more LDS read and seven packed instructions per channel pair give
// U = max(sat16(z << shx) + sat16(skip << shy), 0) (mfma_bn.hpp SumU16), stored as uint16 in z's place.  The residual pass and
// the decoder's fused residual then read one plane instead of z and skip (s5fxp_fast.hpp LayerPlan::resid_fold).  The float
// maximum of |fz + fs| is taken from the unsaturated operands in the second epilogue as before.
template <int KS, int NT, bool TRACE, bool S16 = false, bool DIRECT = false, int FTP = 64, bool WIDE = false, bool PAIR = false, bool PK16 = false,
          bool GBN = false, bool UREC = false>
// <= 128 registers: two six-wave workgroups per CU (at 136 only one was ever resident: measured)
// (measured and lost, DESIGN.md 4a: states, u and skip all requested a tile ahead and waited for by exact count)
// (measured and lost, DESIGN.md 4a: u, skip and z moved in the accumulator's layout instead of through the LDS tiles, COAL)
// (H = 48: three four-wave workgroups fill a CU's LDS, so the three-waves-per-SIMD register budget costs no occupancy there)
__global__ __launch_bounds__(FTP * 2 * NT, NT == 3 && KS == 1 && !WIDE ? 4 : 3) void k_cgate_p(const CGateArgs a_k, GroupOff go)
{
    constexpr bool FOLD = false;
#include "mfma_fused_body.inc"
}
// The same kernel storing the aligned sum U in z's place (FOLD above).  It is told apart by its argument block, not by a
// template argument: the template arguments stay the eleven every k_cgate_p has.  One body, compiled into both (the kernels
// that do not fold keep their code as it was).
template <int KS, int NT, bool TRACE, bool S16, bool DIRECT, int FTP, bool WIDE, bool PAIR, bool PK16, bool GBN, bool UREC>
__global__ __launch_bounds__(FTP * 2 * NT, NT == 3 && KS == 1 && !WIDE ? 4 : 3) void k_cgate_p(const CGateFoldArgs a_k, GroupOff go)
{
    constexpr bool FOLD = true;
#include "mfma_fused_body.inc"
}

} // namespace s5
