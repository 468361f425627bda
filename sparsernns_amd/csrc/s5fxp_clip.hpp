// s5fxp_clip.hpp -- the clip kernel (include/s5fxp.h s5fxp_model_clips): n independent clips of DIFFERENT lengths in ONE
// launch, grid = n, workgroup e serves clip e = one reference batch of B = 1 sequence x len_e frames, its own compute_best
// exponents, status words and carry.  Bit for bit s5fxp_model_forward(B = 1, L = len_e) on that clip alone.
// Included by s5fxp_api.hip after s5fxp_step.hpp: it is the step kernel's stages (s5fxp_step_body.inc) restructured into
// loops over 32-row tiles -- step_mm, step_put2 / step_put4, step_wg_max, StepParams and the generic kernels' primitives,
// op for op; no new arithmetic.  The BatchNorm exponent reductions are the step kernel's function (step_bn_exps); the other
// stages are a copy of the body's text, pinned to it by tests/test_clips.py::test_one_tile_equals_the_step_kernel.
//
// What outlives a tile lives in a workgroup-private scratch in device memory (the caller's workspace): per clip two int16
// planes of Lmax x H, the layer input h and the gate output z.  The tensor-wide maxima (four BatchNorm exponents, the
// residual add's exponent) are over len x H values: the BatchNorm ones re-read h from the scratch, the residual ones are
// gathered in registers while the tiles run, and each ends in one workgroup reduction.  A maximum does not depend on the
// order its operands are visited in, so tiling changes no bit.  The recurrence keeps its state in registers across the
// tiles (one thread per state); the state planes of the C projection are chosen per tile (two byte planes when every state
// of the tile fits 16 bits, four otherwise): both forms are exact, ST_WIDE_STATE is the OR over the tiles.
//
// Visibility of the scratch: only the clip's own workgroup ever writes or reads its two planes.  All its waves run on one
// CU and share that CU's vector L1, so a __syncthreads() (s_waitcnt vmcnt(0) + workgroup barrier) between a pass's stores
// and a later pass's loads is the whole protocol -- no flags, no agent-scope fences, no cross-workgroup data.  What needs
// more is data that ANOTHER CU stored (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup
// visibility": a CU's vector L1 is never refreshed by another CU's stores); there is none here.
//
// LDS: the step kernel's layout (step_lds) at R32 = min(32, Lmax) rows; a tile of fewer rows uses the same strides.
// Padding rows of a tile (rows R..31 of the MFMA tile) are handled as in k_model_step: their A-operand lanes re-read row
// R - 1, their results are dropped by the row < R tests.  Rows len..Lmax-1 of x are never read, of y never written.
#pragma once

namespace s5 {

constexpr int CLIP_MAX_STATES = 128; // one thread per state carries it in registers: P <= the smallest workgroup
constexpr int CLIP_MAX_LEN = 1 << 20; // keeps every in-clip index (len * max(H, d_in, d_out)) inside int32

struct ClipArgs {
    const StepParams *sp;
    const void *x;            // (n,Lmax,d_in) int32, or float32 with f32
    void *y;                  // (n,Lmax,d_out) int32 / float32
    const int32_t *lens;      // n, device memory
    const int32_t *state_in;  // [n][n_layers][2][P] or nullptr (zeros)
    int32_t *state_out;       // the same layout or nullptr; may alias state_in
    int16_t *scratch;         // [n][h | z][Lmax][H]
    int32_t *status;          // n x S5FXP_STATUS_WORDS
    int32_t Lmax, x_bits, x_exp, f32;
};

// The TRACE form (s5fxp_model_clips_traced) is the same text, s5fxp_clip_body.inc, included twice: with
// CLIP_TRACE every stage also stores the value it already holds to the layer's trace plane, padded like y -- rows t < len of
// (n,Lmax,H) / (n,Lmax,P) int32 planes, rows from len on never written.  Those statements sit between #if CLIP_TRACE and
// #endif, so k_model_clips<> is compiled from the text it had (its instruction streams are pinned by tools/disasm_compare.py);
// the trace pointers travel as kernel arguments (CLIP_TRACE_MAX_LAYERS entries of s5fxp_layer_trace).
constexpr int CLIP_TRACE_MAX_LAYERS = 8; // include/s5fxp.h states it: 704 bytes of kernel arguments

struct ClipTraceArgs {
    ClipArgs c;
    s5fxp_layer_trace tr[CLIP_TRACE_MAX_LAYERS]; // device pointers, any may be null
};

#define CLIP_TRACE 0
#include "s5fxp_clip_body.inc"
#define CLIP_TRACE 1
#include "s5fxp_clip_body.inc"

// The PINNED form (s5fxp_model_clips_at): the same text with the exponents as kernel arguments, behind
// CLIP_PINNED as the trace statements are behind CLIP_TRACE, so the two kernels above are compiled from the text they had.
struct ClipPinArgs {
    ClipArgs c;
    PinExps pin;
};
#define CLIP_TRACE 0
#define CLIP_PINNED 1
#include "s5fxp_clip_body.inc"

} // namespace s5

namespace {

// Bytes of one clip's scratch: two int16 planes of Lmax x H (H is a multiple of 16 on the fused path: 32-byte rows)
inline size_t clip_scratch_bytes(const s5fxp_model *m, int Lmax) { return (size_t)4 * (size_t)Lmax * (size_t)m->H; }

// 1: the clip kernel serves this model at Lmax; 0: it does not
inline bool clips_serves(const s5fxp_model *m, int Lmax)
{
    return m->fast && m->fast->step && m->P <= CLIP_MAX_STATES && Lmax <= CLIP_MAX_LEN;
}

int clips_entry(const s5fxp_model *m, const void *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens, void *y,
                const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes, int32_t *status, void *stream,
                bool f32, bool traced = false, const s5fxp_layer_trace *traces = nullptr, bool pinned = false,
                const int32_t *exps = nullptr)
{
    if (pinned && !exps) return S5FXP_EBADARG;
    // step_checks at one row (its row limit is the step kernel's, not this one's): arguments, the model, the static shifts
    if (!lens || !workspace || Lmax < 1 || (traced && !traces)) return S5FXP_EBADARG;
    if (const int rc = step_checks(m, x, x_bits, x_exp, n, 1, 1, y, status, f32)) return rc;
    if (!clips_serves(m, Lmax)) return Lmax > CLIP_MAX_LEN ? S5FXP_EBADARG : S5FXP_EUNSUPPORTED;
    if (traced && m->n_layers > CLIP_TRACE_MAX_LAYERS) return S5FXP_EUNSUPPORTED; // the kernel-argument table's cap
    const size_t ws_need = fit_size((wide_t)n * clip_scratch_bytes(m, Lmax)); // 0: it does not fit a size_t
    if (!ws_need || workspace_bytes < ws_need || (reinterpret_cast<uintptr_t>(workspace) & 1)) return S5FXP_EBADARG;
    if (pinned)
        if (const int rc = exps_check(m, exps)) return rc;
    const int R32 = Lmax < STEP_MAX_ROWS ? Lmax : STEP_MAX_ROWS;
    const size_t smem = step_lds(R32, m->H, m->P, fast_shape(m->H, m->P).hp, m->d_in).total;
    ClipArgs a{};
    a.sp = m->fast->step; a.x = x; a.y = y; a.lens = lens; a.state_in = state_in; a.state_out = state_out;
    a.scratch = reinterpret_cast<int16_t *>(workspace); a.status = status;
    a.Lmax = Lmax; a.x_bits = x_bits; a.x_exp = x_exp; a.f32 = f32 ? 1 : 0;
    if (traced) {
        ClipTraceArgs ta{};
        ta.c = a;
        for (int li = 0; li < m->n_layers; ++li) ta.tr[li] = traces[li]; // the host array is read here, before the entry returns
        return step_launch(n, smem, ta, k_model_clips_traced<512>, k_model_clips_traced<256>, k_model_clips_traced<128>, stream);
    }
    if (pinned) {
        ClipPinArgs pa{a, pin_exps(m, exps)};
        return step_launch(n, smem, pa, k_model_clips_at<512>, k_model_clips_at<256>, k_model_clips_at<128>, stream);
    }
    return step_launch(n, smem, a, k_model_clips<512>, k_model_clips<256>, k_model_clips<128>, stream);
}

} // namespace

extern "C" size_t s5fxp_clips_workspace_bytes(const s5fxp_model *m, int n, int Lmax)
{
    if (!m || n < 1 || Lmax < 1 || Lmax > CLIP_MAX_LEN) return 0;
    return fit_size((wide_t)n * clip_scratch_bytes(m, Lmax));
}

extern "C" int s5fxp_model_clips_ok(const s5fxp_model *m, int Lmax)
{
    if (!m || Lmax < 1) return -1;
    return clips_serves(m, Lmax) ? 1 : 0;
}

extern "C" int s5fxp_model_clips(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                                 int32_t *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                                 int32_t *status, void *stream)
{
    return clips_entry(m, x, x_bits, x_exp, n, Lmax, lens, y, state_in, state_out, workspace, workspace_bytes, status, stream, false);
}

extern "C" int s5fxp_model_clips_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                                     float *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                                     int32_t *status, void *stream)
{
    return clips_entry(m, x, x_bits, x_exp, n, Lmax, lens, y, state_in, state_out, workspace, workspace_bytes, status, stream, true);
}

extern "C" int s5fxp_model_clips_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                                    int32_t *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                                    int32_t *status, const int32_t *exps, void *stream)
{
    return clips_entry(m, x, x_bits, x_exp, n, Lmax, lens, y, state_in, state_out, workspace, workspace_bytes, status, stream, false,
                       false, nullptr, true, exps);
}

extern "C" int s5fxp_model_clips_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                                        float *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                                        int32_t *status, const int32_t *exps, void *stream)
{
    return clips_entry(m, x, x_bits, x_exp, n, Lmax, lens, y, state_in, state_out, workspace, workspace_bytes, status, stream, true,
                       false, nullptr, true, exps);
}

extern "C" int s5fxp_model_clips_traced(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int Lmax,
                                        const int32_t *lens, int32_t *y, const int32_t *state_in, int32_t *state_out, void *workspace,
                                        size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces, void *stream)
{
    return clips_entry(m, x, x_bits, x_exp, n, Lmax, lens, y, state_in, state_out, workspace, workspace_bytes, status, stream, false,
                       true, traces);
}

extern "C" int s5fxp_model_clips_traced_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int Lmax,
                                            const int32_t *lens, float *y, const int32_t *state_in, int32_t *state_out, void *workspace,
                                            size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces, void *stream)
{
    return clips_entry(m, x, x_bits, x_exp, n, Lmax, lens, y, state_in, state_out, workspace, workspace_bytes, status, stream, true,
                       true, traces);
}
