/*
 * s5fxp.h -- C ABI of libs5fxp.so: MI355X (gfx950) kernels for the fixed-point S5 inference
 * path of stevenabreu7/SparseRNNs.
 *
 * This is the drop-in boundary.  The reference is pure Python/JAX and has no
 * FFI of its own, so every entry point below names the reference function it replaces
 * (file:line into /root/reference/sparseRNNs/).  Conventions:
 *   - plain pointers and sizes only; device pointers are raw HIP device addresses
 *     (e.g. torch.Tensor.data_ptr()), `stream` is a hipStream_t passed as void*;
 *   - the caller owns every device buffer; nothing here allocates device memory
 *     (sizes come from the *_bytes query functions);
 *   - every call is asynchronous on `stream` and re-entrant (no global mutable state; the S5FXP_* environment switches
 *     listed under "Environment" below are read once, by s5fxp_model_create, into the handle it returns);
 *   - return value: S5FXP_OK or a negative error code; no exceptions cross the ABI;
 *   - errors that the reference raises from data-dependent values (a negative shift in
 *     fxp_mul's "compute_best", fxparray.py:619-621) are reported through a device status
 *     word, because they are only known on the device.
 * All tensors are int32, row-major, value = data / 2^exp, exactly as fxparray.py:33-38,157.
 */
#ifndef S5FXP_H
#define S5FXP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S5FXP_VERSION 115

enum {
    S5FXP_OK = 0,
    S5FXP_EBADARG = -1,      /* null pointer, non-positive size, unsupported shape */
    S5FXP_ENEGSHIFT = -2,    /* negative/out-of-range shift: the reference raises ValueError (fxparray.py:619-621)
                                or hands XLA an undefined shift (fxparray.py:664-667) */
    S5FXP_EUNSUPPORTED = -3, /* configuration the reference asserts against (fxpmodel.py:429-434,995-999) */
    S5FXP_EHIP = -4,         /* a HIP runtime call failed */
    S5FXP_EWORKSPACE = -5    /* workspace or blob too small */
};

/* rounding modes, fxparray.py:13-17 */
enum { S5FXP_FLOOR = 0, S5FXP_CEIL = 1, S5FXP_ROUND = 2 };

int s5fxp_version(void);
const char *s5fxp_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Op level: one entry point per FxpArray primitive the model uses.
 * ---------------------------------------------------------------------------------------- */

/* fxp_from_fp, fxparray.py:287-307: y = clip(round_mode(x * 2^exp)), x float32. */
int s5fxp_from_fp(const float *x, int32_t *y, int64_t n, int bits, int exp, int round_mode, void *stream);

/* FxpArray.to_float, fxparray.py:72-73. */
int s5fxp_to_float(const int32_t *x, float *y, int64_t n, int exp, void *stream);

/* fxp_change_cfg / fxp_change_exp / fxp_clip, fxparray.py:232-271,310-326,346-357 (signed, FLOOR).
 * Pass new_bits == bits for a pure change_exp; new_exp == exp && new_bits < bits for a pure clip. */
int s5fxp_change_cfg(const int32_t *x, int32_t *y, int64_t n, int bits, int exp, int new_bits, int new_exp,
                     void *stream);

/* fxp_matmul (+ the bias fxp_add of FxpDense.forward), fxparray.py:640-678, fxpmodel.py:352-364.
 * x: (N,K) int32; w: (K,M) int32; bias: (M) int32 or NULL.  y = sat(asr(x@w, x_exp+w_exp-out_exp))
 * [+ change_exp(bias), sat].  flags bit0: apply ReLU (fxpmodel.py:53-63) to the result. */
int s5fxp_dense(const int32_t *x, const int32_t *w, const int32_t *bias, int32_t *y, int64_t N, int K, int M,
                int x_exp, int w_exp, int b_bits, int b_exp, int out_bits, int out_exp, int flags, void *stream);

/* The same layer with a pruned weight (the reference keeps pruned kernels dense with zeros, jaxpruner masks;
 * fxparray.py:662 sums them anyway): the (K,M) kernel stored by output channel -- CSR of kernel^T: rowptr[M+1],
 * colidx[nnz] = k, val[nnz] -- all device int32.  Bit-identical to s5fxp_dense on the densified weight. */
int s5fxp_dense_csr(const int32_t *x, const int32_t *rowptr, const int32_t *colidx, const int32_t *val,
                    const int32_t *bias, int32_t *y, int64_t N, int K, int M, int x_exp, int w_exp, int b_bits, int b_exp,
                    int out_bits, int out_exp, int flags, void *stream);

/* fxp_add with a numeric result_exp, fxparray.py:449-466.  y_len == n (same shape) or a divisor
 * of n (trailing-axis broadcast, e.g. a bias vector). */
int s5fxp_add(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_bits, int x_exp,
              int y_bits, int y_exp, int out_bits, int out_exp, int negate_y, void *stream);

/* fxp_mul with a numeric result_exp, fxparray.py:573-637. */
int s5fxp_mul(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_exp, int y_exp,
              int out_bits, int out_exp, void *stream);

/* result_exp="compute_best" forms (fxparray.py:420-448 and 601-609): the exponent is chosen on
 * the device from float32 maxima over the whole tensor.  `scratch` is >= 16 bytes of device
 * memory, zeroed by the call; out_exp_dev receives {result_exp, status}.  The host reads it back
 * (one sync, like the reference's own np.any/int() syncs). */
int s5fxp_add_cb(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_bits, int x_exp,
                 int y_bits, int y_exp, int out_bits, int32_t *out_exp_dev, void *scratch, void *stream);
int s5fxp_mul_cb(const int32_t *x, const int32_t *y, int32_t *out, int64_t n, int64_t y_len, int x_exp, int y_exp,
                 int out_bits, int32_t *out_exp_dev, void *scratch, void *stream);

/* fxp_relu, fxpmodel.py:27-63.  im == NULL: real max(x,0).  Otherwise the complex form
 * (lexicographic maximum(z,0) through float32). */
int s5fxp_relu(const int32_t *re, const int32_t *im, int32_t *out_re, int32_t *out_im, int64_t n, void *stream);

/* FxpSigmoid.apply, fxpmodel.py:97-144.  lut: 8 host int32 values (fxpmodel.py:89-95). */
int s5fxp_sigmoid(const int32_t *x, int32_t *y, int64_t n, int x_bits, int x_exp, int sig_x_exp, int sig_y_exp,
                  const int32_t *lut_host, void *stream);

/* The sequential diagonal-SSM recurrence, fxpmodel.py:147-208 (make_ssm_step_fn / recurrent_loop,
 * vmapped over the batch at fxpmodel.py:682-704).  bu_*: (B,L,P); a_*: (P); xs_*: (B,L,P).
 * No clip anywhere; int32 wrap.  flags bit0: apply the complex ReLU to the stored states
 * (fxpmodel.py:740-742) instead of storing the raw states. */
int s5fxp_scan(const int32_t *bu_re, const int32_t *bu_im, const int32_t *a_re, const int32_t *a_im, int32_t *xs_re,
               int32_t *xs_im, int B, int L, int P, int a_re_exp, int a_im_exp, int bu_re_exp, int bu_im_exp,
               int x_re_exp, int x_im_exp, int flags, void *stream);

/* The FLOAT model's diagonal-SSM scan, sparseRNNs/model/ssm.py:54-77 (binary operator) + :127
 * (jax.lax.associative_scan over (Lambda_elements, Bu_elements); :166-168 reverse=True for the bidirectional half;
 * vmapped over the batch by the caller of _apply_ssm).  x_t = lambda * x_{t-1} + bu_t in complex64, evaluated as a
 * time-parallel prefix (segment folds, __shfl_up + LDS sweeps over the segment aggregates).  Floating-point prefix sums
 * depend on the combination tree: results agree with the reference's to rounding (tests/: |err| <= 1e-5 * max|x|), not bit
 * for bit.  lambda: (P) complex64 (re, im interleaved); bu, xs: (B,L,P) complex64; x0: (B,P) state before the first
 * step or NULL (zeros -- the reference's scan has no initial element); x_last: (B,P) state after the last step, or NULL.
 * reverse != 0 scans from t = L-1 down to 0. */
int s5fxp_assoc_scan_c64(const float *lambda, const float *bu, float *xs, const float *x0, float *x_last, int B, int L,
                         int P, int reverse, void *stream);

/* The float recurrence with the integer model's per-step rounding (csrc/scan_fq.hpp; the reference of every
 * test is floatmodel.fq_scan).  With F(v, e) = floor(v * 2^e) * 2^-e of the exact real v,
 *   xr' = (F(ar xr, exp_re) - F(ai xi, exp_re)) + F(br, exp_re),  xi' = (F(ar xi, exp_im) + F(ai xr, exp_im)) + F(bi, exp_im),
 * sequentially over time: the statement of fxpmodel.py:147-172 on values instead of integers, for equal exponent pairs and
 * without the int32 wrap.  Inside the domain (every |x| * 2^exp < 2^24, every v * 2^exp a normal number or zero) the result
 * is exact, bit for bit that of the float64 statement.  lambda: (P) complex64; bu, xs: (B,L,P) complex64; x0, x_last: (B,P)
 * or NULL as in s5fxp_assoc_scan_c64; lens: DEVICE int32 (B) or NULL: sequence b runs clamp(lens[b], 0, L) steps of its
 * L-strided rows, nothing behind them is read or written, and x_last[b] is its state after those steps.
 * S5FXP_EBADARG, before the device is touched: a NULL lambda / bu / xs, B, L or P < 1, an exponent outside -24..40, and a
 * shape whose grid or whose 32-bit row offsets do not fit ((64 / P + 2) * L * P * 8 bytes must stay below 2^32). */
int s5fxp_fq_scan_c64(const float *lambda, const float *bu, float *xs, const float *x0, float *x_last, const int32_t *lens,
                      int B, int L, int P, int exp_re, int exp_im, void *stream);

/* The audio steps either side of the model in the N-DNS validation loop, sparseRNNs/fxprun.py:63-78, with the framing of
 * train_helpers.py:1382-1412 (scipy.signal.stft / istft: nperseg = nfft = 512, hop 128, boxcar window, one-sided,
 * boundary="zeros", padded=True, scaling="spectrum").  No model handle, no workspace.  Tensors are frame-major:
 * (B, n_seg, 257), the rows s5fxp_model_forward_f32 takes and returns; the reference's (B, 257, n_seg) is their transpose.
 * Both return S5FXP_EBADARG for a null required pointer or B < 1 and S5FXP_EUNSUPPORTED for T < 512 (where scipy changes
 * nperseg), before the device is touched.
 *
 * Frames of a T-sample signal: ceil(T / 128) + 1, or -1 for T < 512.  The inverse returns (frames - 1) * 128 samples. */
int64_t s5fxp_stft_frames(int64_t T);
/* stft_splitter + the offset of fxprun.py:64-65: x = |Z| - sub (0.0007 for the model's input, 0 for a plain magnitude).
 * audio: (B,T) float32; x: (B,n_seg,257) float32; spec: NULL or (B,n_seg,257) complex64 (re, im interleaved), the
 * spectrum Z itself. */
int s5fxp_stft_mag(const float *audio, int B, int64_t T, float sub, float *x, float *spec, void *stream);
/* fxprun.py:76-78 + stft_mixer (train_helpers.py:1399-1412): the spectrum is rebuilt from the noisy audio (bit for bit
 * s5fxp_stft_mag's), multiplied by 1 + mask -- polar(|Z| * (1 + mask), angle(Z)), negative factors included -- and
 * transformed back, overlap-added, divided by the window cover and trimmed.  mask: (B,n_seg,257) float32 or NULL (zeros:
 * the round trip); out: (B,(n_seg-1)*128) float32; cleaned_mag: NULL or (B,n_seg,257) float32 = |Z| * (1 + mask).
 * No atomics: two calls give identical bits. */
int s5fxp_mask_istft(const float *audio, const float *mask, int B, int64_t T, float *out, float *cleaned_mag,
                     void *stream);

/* The two steps with the model's int16 boundary (s5fxp_model_forward_i16) on the model's side: 2 bytes per value instead of 4.
 * x: (B,n_seg,257) int16 = fxp_from_fp(|Z| - sub, FLOOR) at (x_bits 1..16, x_exp 0..31) of the very float s5fxp_stft_mag
 * stores; mask: (B,n_seg,257) int16 at mask_exp 0..31 (the model's output exponent) or NULL, used as 1 + to_float(mask).  Both
 * conversions restate 16-bit integers, so out and cleaned_mag are bit for bit what s5fxp_stft_mag -> s5fxp_model_forward_f32 ->
 * s5fxp_mask_istft give.  Widths or exponents outside those ranges: S5FXP_EBADARG, before the device is touched. */
int s5fxp_stft_mag_i16(const float *audio, int B, int64_t T, float sub, int x_bits, int x_exp, int16_t *x, float *spec, void *stream);
int s5fxp_mask_istft_i16(const float *audio, const int16_t *mask, int mask_exp, int B, int64_t T, float *out, float *cleaned_mag,
                         void *stream);

/* The two steps for n clips of DIFFERENT lengths, one launch each: with s5fxp_model_clips_f32 between them the denoising loop for
 * n utterances is three launches.  Clip e is row e of audio (n,Tmax) float32 with T_e = clamp(samples[e], 0, Tmax) samples --
 * samples: n int32 in device memory, trusted as the lens of s5fxp_model_clips are -- and len_e = ceil(T_e / 128) + 1 frames.  All
 * row tensors are padded to Lmax = s5fxp_stft_frames(Tmax) frames per clip, the layout s5fxp_model_clips_f32 takes: x, mask,
 * cleaned_mag (n,Lmax,257) float32, spec (n,Lmax,257) complex64, out (n,(Lmax-1)*128) float32.
 *   s5fxp_stft_mag_clips writes rows 0..len_e-1 of x (and of spec, unless NULL) and, unless lens is NULL, lens[e] = len_e: the
 *   model launch takes its lengths from the device, with no host step between the launches.  Rows len_e..Lmax-1 are never
 *   written, samples T_e..Tmax-1 of an audio row never read.
 *   s5fxp_mask_istft_clips writes the first (len_e-1)*128 samples of out[e] and rows 0..len_e-1 of cleaned_mag (unless NULL) and
 *   nothing behind them; mask (NULL: zeros) rows from len_e on are never read.
 * Clip e gets, bit for bit, what s5fxp_stft_mag / s5fxp_mask_istft compute for it alone at B = 1, T = T_e, whatever else is in
 * the launch: a frame's transform and an output hop's sum do not depend on the workgroup that computes them.  No atomics.
 * A clip below 512 samples has no frames: lens[e] = 0, nothing else of it is written, and s5fxp_model_clips skips it.
 * Checked before the device is touched: S5FXP_EBADARG for a null audio, samples, x or out, n < 1 or Tmax > (2^20 - 1) * 128 (Lmax
 * stays within s5fxp_model_clips' cap); S5FXP_EUNSUPPORTED for Tmax < 512. */
int s5fxp_stft_mag_clips(const float *audio, int n, int64_t Tmax, const int32_t *samples, float sub, float *x, float *spec,
                         int32_t *lens, void *stream);
int s5fxp_mask_istft_clips(const float *audio, const float *mask, int n, int64_t Tmax, const int32_t *samples, float *out,
                           float *cleaned_mag, void *stream);

/* The last stage of the validation step, fxprun.py:79-88, folded into the masked inverse: si_snr = si_snr_jax(cleaned, clean)
 * (train_helpers.py:15-53; the cleaned audio is the `target` argument, as fxprun.py:82 calls it) over the T samples of the
 * clip, mag_mse = mean((cleaned_mag - clean_mag)^2) over (n_seg,257) with clean_mag = s5fxp_stft_mag(clean, sub = 0), and
 * loss = lam * mag_mse + (100 - si_snr), one float32 each per sequence, in two launches.  clean: (B,T) float32, the same T as
 * audio; mask as in s5fxp_mask_istft[_i16].  out and cleaned_mag are what s5fxp_mask_istft[_i16] writes, bit for bit, and may
 * each be NULL: the plane is then never stored.  si_snr, mag_mse, loss: (B) float32; mag_mse and loss may be NULL.  The sums
 * behind the scores are taken in double on the float32 values the planes would hold (clean_mag bit for bit
 * s5fxp_stft_mag's), in a fixed order, without atomics: two calls give identical bits, with or without the planes.
 * workspace: s5fxp_score_workspace_bytes(B, T) bytes of device memory, 8-byte aligned, overwritten by the call whatever it
 * held (0 for B < 1, T < 512 or a grid beyond 2^31 - 1, which the entries refuse).  S5FXP_EBADARG for a null audio, clean, workspace or
 * si_snr, B < 1 or mask_exp outside 0..31;
 * S5FXP_EUNSUPPORTED for T < 512 or such a grid; S5FXP_EWORKSPACE for a workspace that is too small -- all before the device is touched. */
size_t s5fxp_score_workspace_bytes(int B, int64_t T);
int s5fxp_mask_istft_score(const float *audio, const float *clean, const float *mask, int B, int64_t T, float lam,
                           float *out, float *cleaned_mag, void *workspace, size_t workspace_bytes,
                           float *si_snr, float *mag_mse, float *loss, void *stream);
int s5fxp_mask_istft_score_i16(const float *audio, const float *clean, const int16_t *mask, int mask_exp, int B, int64_t T,
                               float lam, float *out, float *cleaned_mag, void *workspace, size_t workspace_bytes,
                               float *si_snr, float *mag_mse, float *loss, void *stream);

/* The scored inverse for n clips of DIFFERENT lengths, in two launches whatever n: the layouts of s5fxp_mask_istft_clips, with
 * clean (n,Tmax) float32 padded like audio and sharing its `samples`.  Clip e is scored over its own T_e samples and len_e
 * frames: padding enters neither N, the means nor the MSE denominator.  mask (n,Lmax,257) or NULL (zeros); out
 * (n,(Lmax-1)*128) and cleaned_mag (n,Lmax,257) are what s5fxp_mask_istft_clips writes, padding untouched, and may each be
 * NULL; si_snr, mag_mse, loss: (n) float32, mag_mse and loss may be NULL.  Every score and every plane of clip e is bit for bit
 * what s5fxp_mask_istft_score gives for it alone at B = 1, T = T_e: a tile's sums depend on the clip's own geometry only, and
 * the clip's own tiles are added in the same order.  A clip below 512 samples has no frames: its three scores are quiet NaNs and
 * nothing else of it is written.
 * workspace: s5fxp_score_clips_workspace_bytes(n, Tmax) = 48 * n * ceil((s5fxp_stft_frames(Tmax) - 1) / 13) bytes of device
 * memory, 8-byte aligned, overwritten where a clip has tiles (0 for n < 1, Tmax < 512 or Tmax > (2^20 - 1) * 128); it may hold
 * anything on entry: the tiles a clip does not have keep their bytes, and no score depends on them.
 * Checked before the device is touched, in this order: S5FXP_EBADARG for a null audio, clean, samples, workspace or si_snr,
 * n < 1 or Tmax > (2^20 - 1) * 128; S5FXP_EUNSUPPORTED for Tmax < 512 or a grid beyond 2^31 - 1; S5FXP_EWORKSPACE for a
 * workspace that is too small. */
size_t s5fxp_score_clips_workspace_bytes(int n, int64_t Tmax);
int s5fxp_mask_istft_score_clips(const float *audio, const float *clean, const float *mask, int n, int64_t Tmax,
                                 const int32_t *samples, float lam, float *out, float *cleaned_mag,
                                 void *workspace, size_t workspace_bytes,
                                 float *si_snr, float *mag_mse, float *loss, void *stream);

/* The same framing for a live signal: whole hops of 128 samples in, cleaned hops out (a caller zero-fills its last hop, as
 * scipy's padded=True does).  S streams advance in lock step.  With h = hops_before hops received and a push of c hops
 * (1 .. S5FXP_STREAM_MAX_HOPS): the push completes frames h-1 .. h+c-2 of the batch framing, F = c - (h == 0 ? 1 : 0) of them,
 * and yields output hops max(0, h-3) .. h+c-4, O = min(c, max(0, h+c-3)) of them, plus hop h+c-3 when `final`: a latency of
 * 3 hops.  A stream of m hops ends with a push of two hops of zeros (audio = NULL) with final set -- scipy's trailing
 * boundary: m + 1 frames and m hops in all.  Streamed this way x, cleaned_mag and out are bit for bit s5fxp_stft_mag's and
 * s5fxp_mask_istft's for the whole signal and the concatenated masks.
 *
 * state: S * s5fxp_stream_audio_state_bytes() bytes of device memory owned by the caller, per-stream contiguous, updated in
 * place; all-zero bytes are a fresh stream.  A push is s5fxp_stream_stft, the model on the F rows (s5fxp_model_step_f32),
 * then s5fxp_stream_mask_istft with the same c and hops_before; the host tracks hops_before, nothing on the device counts.
 * Both return S5FXP_EBADARG for a null state, S < 1, c outside 1..32, a negative hops_before or a null required tensor, and
 * s5fxp_stream_mask_istft returns S5FXP_EUNSUPPORTED for final with hops_before < 4 (a signal below 512 samples), before the
 * device is touched.  No atomics: two runs give identical bits. */
#define S5FXP_STREAM_MAX_HOPS 32
size_t s5fxp_stream_audio_state_bytes(void);                          /* per stream, a multiple of 16 */
int64_t s5fxp_stream_frames(int64_t hops_before, int c);              /* F, or -1 for bad arguments */
int64_t s5fxp_stream_out_hops(int64_t hops_before, int c, int final); /* O, or -1 for bad arguments */
/* audio: (S,c*128) float32 or NULL (zeros); x: (S,F,257) float32 = |Z| - sub, may be NULL when F == 0. */
int s5fxp_stream_stft(const float *audio, int S, int c, int64_t hops_before, float sub, void *state, float *x, void *stream);
/* mask: (S,F,257) float32 or NULL (zeros); out: (S,O*128) float32, may be NULL when O == 0; cleaned_mag: NULL or (S,F,257). */
int s5fxp_stream_mask_istft(const float *mask, int S, int c, int64_t hops_before, int final, void *state, float *out,
                            float *cleaned_mag, void *stream);

/* Streams that start, stop and idle on their own: one push serves any subset of a pool of n_slots streams, each entry with
 * its own hop count, phase and flags, in the same three launches (s5fxp_stream_stft_ragged, s5fxp_model_step_ragged_f32,
 * s5fxp_stream_mask_istft_ragged).  All three read ONE array of n descriptors from DEVICE memory, owned by the caller (one
 * host-to-device copy per push); entry e is workgroup e of each launch.  The kernels trust the array as they trust pointers
 * and sizes: validate it on the host with s5fxp_push_desc_check before it is copied.
 *   FRESH  the slot starts a new signal: its carry (step) and its audio state (both audio kernels) are taken as all-zero
 *          bytes, whatever they hold -- a slot is reused after a finished signal without a clearing launch.  (A push of c hops
 *          rewrites the newest c + 3 hops of the audio state and its three segments; the older hops keep their bytes, and no
 *          later push reads them before it has rewritten them);
 *   ZEROS  the entry's audio is zeros, whatever `audio` holds (the two trailing hops of a finishing stream);
 *   FINAL  the entry is the end of its signal (the `final` of s5fxp_stream_mask_istft). */
enum { S5FXP_PUSH_FRESH = 1, S5FXP_PUSH_ZEROS = 2, S5FXP_PUSH_FINAL = 4 };
typedef struct {
    int32_t slot;   /* which stream: index into the caller's carry / audio-state arrays, 0 .. n_slots-1 */
    int32_t rows;   /* model step: frames of this entry, 0 .. Lmax */
    int32_t flags;  /* S5FXP_PUSH_* */
    int32_t hops;   /* audio kernels: hops of this entry, 1 .. cmax */
    int32_t h4;     /* audio kernels: min(hops_before, 4) of this stream */
    int32_t reserved[3];
} s5fxp_push_desc;  /* 32 bytes */
/* Host only, never touches the device; `host` is the array in host memory.  S5FXP_EBADARG: null array, n < 1, a slot outside
 * 0..n_slots-1 or named twice (two workgroups would update one state in place), rows outside 0..Lmax, unknown flag bits,
 * nonzero reserved words; with audio != 0 also cmax outside 1..S5FXP_STREAM_MAX_HOPS, hops outside 1..cmax, h4 outside 0..4,
 * FRESH with h4 != 0, rows != hops - (h4 == 0).  S5FXP_EUNSUPPORTED: audio != 0 and FINAL with h4 < 4 (a signal below 512
 * samples), as s5fxp_stream_mask_istft. */
int s5fxp_push_desc_check(const s5fxp_push_desc *host, int n, int n_slots, int Lmax, int cmax, int audio);
/* The two audio kernels per entry: entry e uses c = hops, h4, final = FINAL and the state of slot `slot`, and gives bit for
 * bit what the lock-step entries give one stream with the same c, hops_before, final and state.  Rows are padded to cmax:
 * audio (n, cmax*128) or NULL (zeros for all), x / mask / cleaned_mag (n, cmax, 257) -- the step's rows with Lmax = cmax,
 * B = 1 -- out (n, (cmax+1)*128); an entry reads its first c hops and writes its F = c - (h4 == 0) rows and its
 * O = min(c, max(0, h+c-3)) + final hops at the front of its row and nothing behind them.  state: n_slots *
 * s5fxp_stream_audio_state_bytes() bytes; a slot no entry names is not touched.  mask NULL = zeros, cleaned_mag NULL = not
 * wanted.  S5FXP_EBADARG for a null desc / state / x / out, n < 1, n_slots < 1 or cmax outside 1..32, before the device is
 * touched. */
int s5fxp_stream_stft_ragged(const float *audio, int n, int cmax, const s5fxp_push_desc *desc, float sub, void *state, int n_slots,
                             float *x, void *stream);
int s5fxp_stream_mask_istft_ragged(const float *mask, int n, int cmax, const s5fxp_push_desc *desc, void *state, int n_slots,
                                   float *out, float *cleaned_mag, void *stream);

/* ------------------------------------------------------------------------------------------
 * Model level: FxpRegressionModel.forward, fxpmodel.py:1431-1439 (-> 1261-1271 -> 1110-1161).
 * The integer parameters are what FxpRegressionModel.export() emits
 * (fxpmodel.py:368-393,819-847,946-968,1163-1207,1441-1458).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t K, M;
    const int32_t *weight; /* host, (K,M) */
    const int32_t *bias;   /* host, (M) */
    int32_t w_bits, w_exp, b_bits, b_exp, inp_bits, inp_exp, out_bits, out_exp;
} s5fxp_dense_desc;

typedef struct {
    int32_t H, P;
    const int32_t *A_re, *A_im; /* host, (P)   Lambda_bar */
    const int32_t *B_re, *B_im; /* host, (P,H) B_bar */
    const int32_t *C_re, *C_im; /* host, (H,P) C_tilde */
    const int32_t *D;           /* host, (H) */
    int32_t A_re_bits, A_re_exp, A_im_bits, A_im_exp, B_re_bits, B_re_exp, B_im_bits, B_im_exp;
    int32_t C_re_bits, C_re_exp, C_im_bits, C_im_exp, D_bits, D_exp;
    int32_t u_bits, u_exp, Bu_re_bits, Bu_re_exp, Bu_im_bits, Bu_im_exp;
    int32_t x_re_bits, x_re_exp, x_im_bits, x_im_exp, y_bits, y_exp;
} s5fxp_ssm_desc;

typedef struct {
    const int32_t *minus_mean, *invsq_var, *scale, *bias; /* host, (H); scale/bias may be NULL */
    int32_t mean_bits, mean_exp, invsq_var_bits, invsq_var_exp, scale_bits, scale_exp, bias_bits, bias_exp;
} s5fxp_norm_desc;

typedef struct {
    s5fxp_norm_desc norm;
    s5fxp_ssm_desc ssm;
    s5fxp_dense_desc out2;
    int32_t l_bits, l_exp, r_bits, r_exp, res_bits, res_exp; /* mult_gate, fxpmodel.py:1075-1093 */
    int32_t sig_x_exp, sig_y_exp;                            /* fxpmodel.py:1097-1104 */
    int32_t lut[8];                                          /* fxpmodel.py:89-95 */
} s5fxp_layer_desc;

typedef struct {
    int32_t n_layers;
    s5fxp_dense_desc encoder;
    const s5fxp_layer_desc *layers;
    s5fxp_dense_desc decoder;
} s5fxp_model_desc;

typedef struct s5fxp_model s5fxp_model; /* opaque host handle */

/* Optional capture of per-layer intermediates (device pointers, any may be NULL); names follow
 * the reference's sow() keys (fxpmodel.py:653,736,742,793,1120,1126,1135,1145,1153). */
typedef struct {
    int32_t *pre_s5;        /* (N,H)  BatchNorm output                       */
    int32_t *u;             /* (N,H)  SSM input after change_cfg             */
    int32_t *Bu_re, *Bu_im; /* (N,P)                                         */
    int32_t *xs_re, *xs_im; /* (N,P)  raw states                             */
    int32_t *ys;            /* (N,H)  "pre_GLU"                              */
    int32_t *out2;          /* (N,H)                                         */
    int32_t *out2_sigmoid;  /* (N,H)                                         */
    int32_t *post_GLU;      /* (N,H)                                         */
    int32_t *residadd;      /* (N,H)                                         */
} s5fxp_layer_trace;

/* Bytes of device memory the packed parameter blob needs. */
size_t s5fxp_model_blob_bytes(const s5fxp_model_desc *desc);

/* Packs the integer parameters (int8 weight planes for the MFMA path, int32 for the generic one) into
 * `dev_blob` (device, blob_bytes) with a stream-ordered copy and returns a host handle that keeps
 * the scalars.  flags: S5FXP_MODEL_* below.  Returns S5FXP_EUNSUPPORTED for shapes outside the
 * kernels' limits.  Pruned models run the dense kernels on their zero-filled weights (bit-exact; on the MFMA path
 * the weights live in registers and the contraction is ~2 us per kernel): S5FXP_MODEL_FORCE_DENSE is the default
 * behaviour, S5FXP_MODEL_FORCE_CSR is refused (EUNSUPPORTED) -- the CSR kernel exists at op level, s5fxp_dense_csr.
 * S5FXP_MODEL_NO_RESID_FOLD: the fused path's gate kernel stores z and the residual add reads z and the layer input again,
 * instead of the one uint16 plane of their aligned sum (same results; for measurements and tests).
 * S5FXP_MODEL_NO_RESID_LAZY: the residual pass between two layers stores the shifted sum as a plane of its own again, instead of
 * leaving the uint16 plane to the next layer's kernels, which shift it as they load it (same results; for measurements and tests).
 * S5FXP_MODEL_NO_GATE_EXT: that residual pass reads the uint16 plane for its per-channel extremes again, instead of taking them
 * from the gate kernel, which gathers them as it stores the plane (same results; for measurements and tests). */
enum { S5FXP_MODEL_DEFAULT = 0, S5FXP_MODEL_FORCE_DENSE = 1, S5FXP_MODEL_FORCE_CSR = 2, S5FXP_MODEL_FORCE_GENERIC = 4,
       S5FXP_MODEL_NO_RESID_FOLD = 8, S5FXP_MODEL_NO_RESID_LAZY = 16, S5FXP_MODEL_NO_GATE_EXT = 32 };
int s5fxp_model_create(const s5fxp_model_desc *desc, void *dev_blob, size_t blob_bytes, int flags, void *stream,
                       s5fxp_model **out);
void s5fxp_model_destroy(s5fxp_model *m);

/* Device workspace for one forward of B sequences of L frames; it may hold anything on entry: no output depends on what it
 * held, nor on what the status words, y, state_out and the trace planes held (tests/test_caller_memory.py).  The status words
 * are always written completely; y, state_out and the trace planes are written completely by a forward that does not come back
 * with S5FXP_ST_REDO (under S5FXP_FWD_DEFER_REDO they are then invalid, see below).  0: a null model, B < 1 or L < 1, or a size that does not fit
 * a size_t (the sum is formed with checked arithmetic and never wraps; it grows with B and with L, so the answer does not
 * return from 0 to a size as either grows).  The forwards refuse such a (B, L), and a grouped call whose G-fold of this
 * value does not fit a size_t, with S5FXP_EWORKSPACE before the device is touched, whatever workspace_bytes claims. */
size_t s5fxp_workspace_bytes(const s5fxp_model *m, int B, int L);

/* Number of int32 words in the device status buffer, and its layout:
 *   [0] error bits (S5FXP_ST_*), [1] decoder output exponent as s5fxp_model_step and s5fxp_model_clips store it (0 from
 *       s5fxp_model_forward[_f32|_i16] and s5fxp_layer_forward: it is a fact of the model, s5fxp_model_out_exp),
 *   [2] which kernels this forward ran: S5FXP_PATH_GENERIC (one-lane / VALU kernels, any int32 operands),
 *       S5FXP_PATH_FUSED (the int8-MFMA tile kernels + the quad / pair recurrence kernels), S5FXP_PATH_STEP (the
 *       one-launch kernel of s5fxp_model_step) or S5FXP_PATH_CLIP (the one-launch kernel of s5fxp_model_clips),
 *   [8 + 8*l + 0..4] layer l: exponents chosen by the 4 BatchNorm ops and the residual add,
 *   [8 + 8*l + 5]    layer l: the recurrence kernel that was enqueued first, coded as s5fxp_model_recurrence_kernel
 *                    (5 = the exact 32-bit quad chain of a S5FXP_FWD_EXACT forward, 6 = the 32-bit recurrence inside
 *                    s5fxp_model_step's kernel),
 *   [8 + 8*l + 6]    layer l: the state slots its kernels ran on: P, or the live states rounded up to a multiple of 32
 *                    when the layer was compacted (s5fxp_model_live_states).
 *   [8 + 8*l + 7]    layer l: the state slots its two recurrence streams hold: [8 + 8*l + 6], or fewer -- the live states
 *                    rounded up to an even number -- when the LDS-fed pair kernel runs a layer compacted to 32 slots. */
#define S5FXP_STATUS_WORDS 128
enum { S5FXP_PATH_GENERIC = 1, S5FXP_PATH_FUSED = 2, S5FXP_PATH_STEP = 3, S5FXP_PATH_CLIP = 4 };
enum {
    S5FXP_ST_NEGSHIFT = 1,   /* a data-dependent shift came out negative: the reference raises ValueError */
    S5FXP_ST_NEGEXP = 2,     /* a compute_best exponent came out negative (1 << exp fails in the reference) */
    S5FXP_ST_WIDE_STATE = 4, /* informational: an SSM state exceeded 24 bits, the 32-bit C projection ran */
    S5FXP_ST_WIDE_INPUT = 8, /* the input tensor holds values beyond 24 bits: results invalid, re-run with a
                                model created with S5FXP_MODEL_FORCE_GENERIC */
    S5FXP_ST_REDO = 16       /* only with S5FXP_FWD_DEFER_REDO: a state left the fast recurrence's exact range -- a
                                stored state, or a state_in value the recurrence started from -- and the exact
                                re-run was NOT enqueued: results invalid, call again with S5FXP_FWD_EXACT */
};

/* s5fxp_forward_opts.flags.  By default a forward is self-contained: next to the fast recurrence it enqueues
 * the exact 32-bit kernels, gated on a device flag, so the output is right whatever the data.  A caller that
 * reads the status words anyway can drop those (normally idle) launches:
 *   DEFER_REDO  do not enqueue the gated exact kernels; S5FXP_ST_REDO in status[0] tells the caller to repeat
 *               the forward with S5FXP_FWD_EXACT.  The recurrence streams are then kept as int16 where the model's
 *               Bu configuration guarantees they fit (half the bytes; a state beyond 16 bits saturates and raises
 *               S5FXP_ST_REDO like any other state outside the fast kernels' range);
 *   EXACT       skip the fast recurrence, run the exact kernels only;
 *   NO_PAIR     (with DEFER_REDO) use the quad kernel with int16 streams instead of the pair kernel: its bound on
 *               |state| is the full 16 bits, the pair kernel's is tighter by what the folded Bu needs -- the middle rung
 *               of a caller's pair -> quad -> exact ladder. */
enum { S5FXP_FWD_DEFER_REDO = 1, S5FXP_FWD_EXACT = 2, S5FXP_FWD_NO_PAIR = 4 };

/* Cross-rank hook for the data-dependent exponents (mode A): when not NULL it is
 * called once per compute_best op, after the local float32 maxima (n <= 4 floats, device memory)
 * are complete on `stream`, and must leave their element-wise MAX over all ranks in place,
 * stream-ordered.  NULL = per-shard exponents (mode B). */
typedef int (*s5fxp_allreduce_max_fn)(void *ctx, float *dev_vals, int n, void *stream);

/* Optional knobs of one forward (all-zero = defaults). */
typedef struct {
    s5fxp_allreduce_max_fn allreduce; /* NULL: per-shard exponents */
    void *allreduce_ctx;
    /* Measurement only: 2*n_layers hipEvent_t handles (or NULL).  Fused path: events [2l] / [2l+1] are attached to
     * layer l's recurrence launch (hipExtLaunchKernelGGL start / stop events: the time stamps of that dispatch, as
     * rocprofv3's kernel trace reports them); both must be set.  Generic path: recorded on `stream` immediately
     * before / after the layer's recurrence kernel.  NULL entries are skipped. */
    void **scan_events;
    int32_t flags; /* S5FXP_FWD_* */
    /* Streaming (sparseRNNs/fxpmodel.py:147-172: the step function's carry is an explicit argument; the reference's
     * recurrent_loop always starts it at zero, :196-207).  Device arrays [n_layers][2][B][P] int32 (re plane, im plane
     * per layer) or NULL: state_in = the SSM states the recurrences start from (NULL: zeros), state_out = where the
     * states after the last frame are left (NULL: not wanted).  Feeding a sequence chunk by chunk with the carry gives,
     * per chunk, what the reference computes for that chunk started from that carry -- every chunk is its own
     * compute_best batch, so the exponents (and with them the low bits) can differ from one pass over the whole
     * sequence.  state_in may hold int32 values of any width (the exact kernels, s5fxp_model_step and a caller leave
     * such carries): the fast recurrence kernels range-check the values they start from against the bound the states
     * are checked with, and a carry beyond it takes the same route as a state beyond it -- the gated exact kernels of
     * a default forward, S5FXP_ST_REDO under S5FXP_FWD_DEFER_REDO.  state_in is only ever read.  With
     * S5FXP_FWD_DEFER_REDO keep state_in and state_out apart: a forward that comes back with S5FXP_ST_REDO has left
     * an unusable state_out, and its repeat needs the old state_in. */
    const int32_t *state_in;
    int32_t *state_out;
    /* Grouped call (0 or 1: a plain forward).  groups = G > 1: x and y hold G * B sequences -- G independent reference
     * batches of B sequences each, exactly what G calls with B sequences compute (every group is its own compute_best
     * batch: own exponents, own status words, own carry), but enqueued as ONE set of kernel launches (gridDim.y = G on
     * the fused path; a loop over the groups elsewhere).  Everything per-forward is G-fold and contiguous, group after
     * group: workspace >= G * s5fxp_workspace_bytes(m, B, L) (that value is the group stride), status
     * G * S5FXP_STATUS_WORDS words, state_in / state_out [G][n_layers][2][B][P], traces G * n_layers entries.  This is the
     * reference's run_validation loop over batches (sparseRNNs/fxprun.py:53-88) taken several batches at a time: at the
     * N-DNS batch of 32 sequences a launch costs about as much as a quarter of its work. */
    int32_t groups;
    /* Measurement only, like scan_events: 2*n_layers hipEvent_t handles (or NULL) attached to layer l's GATE-kernel launch
     * (C projection + out2 + gate) on the fused path; ignored elsewhere. */
    void **gate_events;
} s5fxp_forward_opts;

/* x: (B,L,d_in) int32 device; y: (B,L,d_out) int32 device; status: S5FXP_STATUS_WORDS int32 device.
 * traces: NULL or n_layers entries (host array of device pointers); opts: NULL or see above. */
int s5fxp_model_forward(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int B, int L, int32_t *y,
                        void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                        const s5fxp_forward_opts *opts, void *stream);

/* The same forward, float32 in and float32 out: the reference's N-DNS validation step (sparseRNNs/fxprun.py:63-88) builds
 * fxp_x = fxp_from_fp(x, x_bits, x_exp, FLOOR), runs y = model(fxp_x) and uses y.to_float().  Bit for bit what
 *   s5fxp_from_fp(x -> xi, B*L*d_in, x_bits, x_exp, S5FXP_FLOOR);
 *   s5fxp_model_forward(m, xi, x_bits, x_exp, B, L, yi, ...);
 *   s5fxp_to_float(yi -> y, B*L*d_out, s5fxp_model_out_exp(m));
 * gives -- y, status words, traces and state_out -- for every opts setting the int entry takes.  x: (B,L,d_in) float32 device;
 * y: (B,L,d_out) float32 device; x_bits 1..32 and x_exp 0..31 are the quantisation target of x (usually the encoder's input
 * configuration).  On the fused path the conversions happen inside the encoder and decoder kernels (no extra launch or pass);
 * elsewhere the int32 input and output are staged in the workspace.  workspace_bytes >= G * s5fxp_workspace_bytes_f32(m, B, L)
 * (the group stride of a grouped call).  A model whose output exponent is outside 0..31 returns S5FXP_EUNSUPPORTED. */
int s5fxp_model_forward_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int B, int L, float *y,
                            void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                            const s5fxp_forward_opts *opts, void *stream);
/* Device workspace for one s5fxp_model_forward_f32 of B sequences of L frames: s5fxp_workspace_bytes for a model on the fused
 * path, plus the staged int32 input and output for a generic one.  0: bad argument, or a size that does not fit a size_t
 * (as s5fxp_workspace_bytes; the entry then returns S5FXP_EWORKSPACE). */
size_t s5fxp_workspace_bytes_f32(const s5fxp_model *m, int B, int L);

/* The same forward with an int16 model boundary: x (B,L,d_in) int16 device at (x_bits 1..16, x_exp), y (B,L,d_out) int16 device.
 * Bit for bit what s5fxp_model_forward gives for the sign-extended x -- y narrowed to int16, status words, traces and state_out
 * -- for every opts setting the int entry takes.  The narrowing loses nothing: a model whose decoder has out_bits > 16 returns
 * S5FXP_EUNSUPPORTED, and whatever the int entry rejects returns S5FXP_EBADARG, both before the device is touched.
 * x and y need 2-byte alignment only: rows are 2 * d_in / 2 * d_out bytes (514 at 257 columns) and the groups of a grouped
 * call follow each other densely, so a group's base may be an odd number of int16.  On the fused path the encoder reads and the
 * decoder writes int16 directly (no extra launch or pass; the int forward's grids and workspace); elsewhere int32 copies are
 * staged in the workspace.  workspace_bytes >= G * s5fxp_workspace_bytes_i16(m, B, L). */
int s5fxp_model_forward_i16(const s5fxp_model *m, const int16_t *x, int x_bits, int x_exp, int B, int L, int16_t *y,
                            void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                            const s5fxp_forward_opts *opts, void *stream);
/* Device workspace for one s5fxp_model_forward_i16: s5fxp_workspace_bytes for a model on the fused path, plus the staged int32
 * input and output for a generic one.  0: bad argument, or a size that does not fit a size_t (as s5fxp_workspace_bytes; the
 * entry then returns S5FXP_EWORKSPACE). */
size_t s5fxp_workspace_bytes_i16(const s5fxp_model *m, int B, int L);

/* Environment (experiments and tests only; read ONCE by s5fxp_model_create and stored in the handle, never by a forward):
 *   S5FXP_NO_PAIR, S5FXP_PAIR_GLOBAL, S5FXP_PAIRL_BLOCKS=16   recurrence kernel choice (see s5fxp_model_recurrence_kernel)
 *   S5FXP_NO_PK16, S5FXP_NO_BN_EXT, S5FXP_NO_COMPACT           unpacked gate epilogues / four-reduction BatchNorm exponents / no
 *                                                              live-state compaction
 *   S5FXP_NO_DEC_RESID                                         the last layer's residual pass as a launch of its own
 *   S5FXP_NO_LIVE_LANES                                        a compacted layer's recurrence streams keep their padding slots
 *   S5FXP_GATE_BN=0|1|2                                        where the gate kernel takes the SSM input u from.  Unset: the 32-frame kernel
 *                                                              rebuilds it from the layer input it loads anyway and the B projection does
 *                                                              not store it; 0: u travels through memory (the kernels before that, for A/B
 *                                                              runs); 1: the first experiment, 64-frame tiles with the BatchNorm chain in
 *                                                              the first epilogue (slower than both; kept as the record); 2: the gate
 *                                                              kernel as when unset, and the B projection, which runs the same packed row
 *                                                              chain at H = 96, keeps its element-wise one (the kernels before that, for A/B
 *                                                              runs)
 *   S5FXP_CGATE_FT64, S5FXP_WGS_CGATE32=n                      the gate kernel on 64-frame tiles (six-wave workgroups) / workgroups per launch
 *                                                              of the default 32-frame form
 *   S5FXP_WGS_ENC|DEC|CGATE|BPROJ|RESID=n                      workgroups per launch of the tile kernels
 *   S5FXP_PLANE_SKEW=bytes                                     extra distance between the workspace's planes (multiple of 256)
 *   S5FXP_DEBUG_SYNC                                           synchronise and check after every stage of a forward
 * Results do not depend on any of them. */

/* ------------------------------------------------------------------------------------------
 * Streaming step: one short chunk of G independent streams in ONE kernel launch (grid = G, one workgroup per group).
 * A group is one reference batch of B sequences x L frames with B * L <= S5FXP_STEP_MAX_ROWS rows; group g gets, bit
 * for bit, what s5fxp_model_forward computes for that (B, L) input with that carry -- its own compute_best exponents,
 * status words and carry, the `groups` semantics of s5fxp_forward_opts.  Every tensor-wide maximum of such a batch is a
 * workgroup reduction, so the whole forward (encoder, per layer BatchNorm exponents -> B projection -> the plain
 * 32-bit recurrence of fxpmodel.py:147-172 from the carry -> C projection, exact for int32 states of any width -> out2
 * -> sigmoid -> gate -> residual, decoder) runs between __syncthreads() instead of kernel boundaries.  No workspace, no
 * traces, no cross-rank hook, no flags, no redo: callers who need those use s5fxp_model_forward.
 *   x (G,B,L,d_in), y (G,B,L,d_out): int32, or float32 for _f32 (fxp_from_fp FLOOR in, to_float out, as
 *   s5fxp_model_forward_f32; x_exp 0..31); carry [G][n_layers][2][B][P]: state_in NULL = zeros, state_out NULL = not
 *   wanted, state_out == state_in is allowed (a workgroup reads its carry before it writes it).
 *   status: G * S5FXP_STATUS_WORDS words, written completely by the kernel: [0] error bits (NEGSHIFT, NEGEXP and
 *   WIDE_INPUT as the fused batch path raises them: an input value beyond 16 bits after the encoder's input conversion
 *   makes the results invalid; WIDE_STATE is informational: the four-plane C projection ran), [1] the decoder's output
 *   exponent, [2] S5FXP_PATH_STEP, [8+8l+0..4] the five exponents, [8+8l+5] = 6, [8+8l+6] = [8+8l+7] = P.
 * Returns S5FXP_EBADARG for null x / y / status / model, G < 1, B < 1, L < 1 or B * L > S5FXP_STEP_MAX_ROWS, and
 * S5FXP_EUNSUPPORTED for a model that s5fxp_model_is_fast() does not report -- all before the device is touched. */
#define S5FXP_STEP_MAX_ROWS 32
/* 1: s5fxp_model_step serves this model at (B, L); 0: it does not (generic model, B * L > S5FXP_STEP_MAX_ROWS);
 * -1: bad argument */
int s5fxp_model_step_ok(const s5fxp_model *m, int B, int L);
int s5fxp_model_step(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int G, int B, int L, int32_t *y,
                     const int32_t *state_in, int32_t *state_out, int32_t *status, void *stream);
int s5fxp_model_step_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int G, int B, int L, float *y,
                         const int32_t *state_in, int32_t *state_out, int32_t *status, void *stream);
/* The step with per-entry row counts and carry slots (s5fxp_push_desc above; the array is device memory): grid = n, entry e
 * runs L = desc[e].rows frames of each of its B sequences on the carry of slot s = desc[e].slot and gives, bit for bit,
 *   s5fxp_model_step(m, x_e, x_bits, x_exp, 1, B, L, y_e, FRESH ? NULL : state[s], state[s], status_e, ...)
 * -- the y rows, the carry left in state[s] and all S5FXP_STATUS_WORDS status words.
 *   x (n,B,Lmax,d_in), y (n,B,Lmax,d_out): padded to Lmax frames per sequence; frames L..Lmax-1 of x are never read and of
 *   y never written.  state [n_slots][n_layers][2][B][P], updated in place; a slot no entry names is never touched.
 *   rows == 0: y untouched, the carry untouched (zeroed if FRESH), the status words hold the kernel's initial fill ([1],
 *   [2], the per-layer constants, zeros elsewhere).
 *   S5FXP_ST_WIDE_INPUT, the one difference from s5fxp_model_step: the entry stores its status words and stops, leaving
 *   its y rows and state[s] untouched, so the caller can serve it from the intact carry on the generic engine.
 * B * Lmax <= S5FXP_STEP_MAX_ROWS.  Host checks as s5fxp_model_step at (B, Lmax), and S5FXP_EBADARG for a null desc or
 * state or n_slots < 1. */
int s5fxp_model_step_ragged(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int B, int Lmax, int32_t *y,
                            const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, void *stream);
int s5fxp_model_step_ragged_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int B, int Lmax, float *y,
                                const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Clips: n independent sequences of DIFFERENT lengths in ONE kernel launch (grid = n, one workgroup per clip, looping over
 * 32-row tiles).  Clip e is one reference batch of B = 1 sequence of len_e = clamp(lens[e], 0, Lmax) frames and gets, bit for
 * bit, what s5fxp_model_forward(m, x_e, x_bits, x_exp, 1, len_e, ...) computes for it alone with that carry -- its own
 * compute_best exponents, status words and carry.  A clip's result does not depend on what else is in the launch.
 *   x (n,Lmax,d_in), y (n,Lmax,d_out): int32, or float32 for _f32 (fxp_from_fp FLOOR in, to_float out; x_exp 0..31), padded
 *   to Lmax frames per clip; frames len_e..Lmax-1 of x are never read and of y never written.  lens: n int32, device memory.
 *   carry [n][n_layers][2][P]: state_in NULL = zeros, state_out NULL = not wanted, state_out == state_in is allowed.
 *   workspace: s5fxp_clips_workspace_bytes(m, n, Lmax) bytes of device memory, 2-byte aligned: per clip two int16 planes of
 *   Lmax x H (the layer input and the gate output), written and read by that clip's workgroup only.  It may hold anything
 *   on entry: no output depends on what it held.
 *   status: n * S5FXP_STATUS_WORDS words, written completely by the kernel, laid out as s5fxp_model_step's with
 *   [2] = S5FXP_PATH_CLIP.  S5FXP_ST_WIDE_STATE is the OR over the clip's tiles.
 *   len_e == 0: y untouched, state_out[e] = state_in[e] (zeros for NULL), the status words hold the kernel's initial fill.
 *   S5FXP_ST_WIDE_INPUT (a value beyond 16 bits after the encoder's input conversion, in any frame of the clip): the clip
 *   stores its status words and stops, leaving its y rows and state_out[e] untouched, as s5fxp_model_step_ragged does; the
 *   caller serves it on a generic model.  The other clips of the launch are not affected.
 * One CU serves one clip, tile after tile: the entry is for MANY short clips.  A single long clip, or a few, belong on
 * s5fxp_model_forward, which spreads one sequence over the chip (DESIGN.md §4o has the measured break-even).
 * Checked before the device is touched: S5FXP_EBADARG for a null model / x / y / lens / status / workspace, n < 1, Lmax < 1
 * or Lmax > 2^20, x_bits outside 1..32 (and x_exp outside 0..31 for _f32) or workspace_bytes too small;
 * S5FXP_EUNSUPPORTED for a model that s5fxp_model_is_fast() does not report; S5FXP_ENEGSHIFT for the static shifts
 * s5fxp_model_step checks.  No traces, no cross-rank hook, no flags, no redo, no B > 1. */
/* 0: bad argument, or a size that does not fit a size_t (the entries then return S5FXP_EBADARG, as for any workspace that
 * is too small) */
size_t s5fxp_clips_workspace_bytes(const s5fxp_model *m, int n, int Lmax);
/* 1: s5fxp_model_clips serves this model at Lmax; 0: it does not (generic model, Lmax > 2^20); -1: bad argument */
int s5fxp_model_clips_ok(const s5fxp_model *m, int Lmax);
int s5fxp_model_clips(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                      int32_t *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                      int32_t *status, void *stream);
int s5fxp_model_clips_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                          float *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                          int32_t *status, void *stream);
/* The clip launch WITH TRACE PLANES: the arguments of s5fxp_model_clips[_f32] plus `traces`, n_layers entries
 * in HOST memory (device pointers, any plane may be NULL), read before the entry returns.  Planes are padded like x / y:
 * (n,Lmax,H), or (n,Lmax,P) for Bu_* / xs_*, int32.  Rows t < len_e of every plane of clip e are bit for bit what
 * s5fxp_model_forward(B = 1, L = len_e, traces) stores for that clip alone with that carry -- xs_* the raw states before the
 * complex ReLU, residadd the sum before the ReLU; rows from len_e on are never written.  y, state_out and all status words are
 * bit-identical to the untraced entry.  A clip that stops with S5FXP_ST_WIDE_INPUT leaves its trace rows untouched, like its y
 * rows; len_e == 0 writes nothing.  One launch of the TRACE form of the clip kernel, a diagnostic path: the stages store the
 * values they hold, and the trace pointers travel as kernel arguments, so a model of more than 8 layers gets
 * S5FXP_EUNSUPPORTED before the device is touched.  traces == NULL is S5FXP_EBADARG (the untraced entries are the way to run
 * without traces); every other check and error is that of s5fxp_model_clips. */
int s5fxp_model_clips_traced(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                             int32_t *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                             int32_t *status, const s5fxp_layer_trace *traces, void *stream);
int s5fxp_model_clips_traced_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                                 float *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                                 int32_t *status, const s5fxp_layer_trace *traces, void *stream);

/* ------------------------------------------------------------------------------------------
 * Stated exponents: the step, ragged step and clip launches with the five compute_best exponents of every layer given by
 * the caller instead of chosen from the data of the launch.  A stream then gives the same bits however it
 * is cut into steps, and those of s5fxp_model_clips_at on the whole signal at the same exponents; with the exponents an
 * unpinned forward of the whole signal reports, it gives that forward's bits.
 *   exps: 5 * n_layers int32 in HOST memory, read before the entry returns, in the order of the status words
 *   [8 + 8*l + 0..4]: the result exponents of BN add(-mean), BN mul(invsq_var), BN mul(scale), BN add(bias) and the residual
 *   add of layer l.  A slot whose op the layer lacks (no scale, no bias) is ignored.  Model-wide: every group, entry or clip
 *   of the launch runs at it.
 * Each _at entry is its namesake with `exps` in front of `stream` and computes what the namesake computes, each of the five
 * ops using the stated exponent where the namesake finalizes one from a reduction (fxparray.py:420-448, 601-637 with
 * result_exp given): the same carry, WIDE_INPUT rule, WIDE_STATE, padding rules, rows == 0 / len == 0 rules.  A value beyond
 * the range an exponent leaves saturates at the op's result bits, as fxp_clip does.  Status words: [0] never carries NEGSHIFT
 * or NEGEXP (both are refused here, on the host); [8+8l+0..4] hold the stated exponents, 0 for an op the layer lacks; all
 * other words as the namesake writes them.  The kernels hold no maxima loop and no reduction.
 * Checked before the device is touched: the namesake's checks, S5FXP_EBADARG for a null exps, then s5fxp_model_exps_check.
 * Not served at stated exponents: traced forwards and the traced clip entries, exponents in device memory or per clip or
 * per sequence, the multi-GPU forward.  (The batch forward is served: s5fxp_model_forward_at* below.) */
/* The largest exponent op k (0..4, the order above) of `layer` can take: its result bits - 1, the exponent of a result
 * whose maximum is below 1 (intbits is never negative).  -1 for an op the layer lacks or a bad argument.  Any model. */
int s5fxp_model_exp_max(const s5fxp_model *m, int layer, int k);
/* Host only, never touches the device.  S5FXP_EBADARG: a null model or array; S5FXP_EUNSUPPORTED: a model
 * s5fxp_model_is_fast() does not report, or one of more than 8 layers (the exponents travel as kernel arguments);
 * S5FXP_EBADARG: an exponent outside 0 .. s5fxp_model_exp_max; S5FXP_ENEGSHIFT: a shift these exponents make negative or
 * larger than 31 -- with stated exponents every one is static: what finalize_add_cb / finalize_mul_cb flag on the device
 * (an add's operand and result shifts, a mul's right shift), the change_cfg to the SSM input, the decoder's input
 * conversion and its right shift. */
int s5fxp_model_exps_check(const s5fxp_model *m, const int32_t *exps_host);
int s5fxp_model_step_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int G, int B, int L, int32_t *y,
                        const int32_t *state_in, int32_t *state_out, int32_t *status, const int32_t *exps, void *stream);
int s5fxp_model_step_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int G, int B, int L, float *y,
                            const int32_t *state_in, int32_t *state_out, int32_t *status, const int32_t *exps, void *stream);
int s5fxp_model_step_ragged_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int B, int Lmax, int32_t *y,
                               const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, const int32_t *exps,
                               void *stream);
int s5fxp_model_step_ragged_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int B, int Lmax, float *y,
                                   const s5fxp_push_desc *desc, int32_t *state, int n_slots, int32_t *status, const int32_t *exps,
                                   void *stream);
int s5fxp_model_clips_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                         int32_t *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                         int32_t *status, const int32_t *exps, void *stream);
int s5fxp_model_clips_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int n, int Lmax, const int32_t *lens,
                             float *y, const int32_t *state_in, int32_t *state_out, void *workspace, size_t workspace_bytes,
                             int32_t *status, const int32_t *exps, void *stream);

/* The batch forward at stated exponents: s5fxp_model_forward / _f32 / _i16 with `exps` in front of `stream`,
 * on the whole chip like its namesake.  Every sequence of the batch, and every group of a grouped launch (opts->groups), gets
 * bit for bit the rows s5fxp_model_clips_at[_f32] gives that sequence alone at the same exponents; with opts->state_in /
 * state_out the carry matches too, chunk for chunk, so a signal cut into several calls gives the rows of one call.  A value
 * beyond the range an exponent leaves saturates at the op's result bits.  Everything else is the namesake's: the S5FXP_FWD_*
 * flags and the recurrence rungs they choose, S5FXP_ST_REDO / WIDE_STATE / WIDE_INPUT, live-state compaction, padding, and the
 * workspace (s5fxp_workspace_bytes*).  Status words: [0] never carries NEGSHIFT or NEGEXP; [2] is S5FXP_PATH_FUSED;
 * [8+8l+0..4] hold the stated exponents, 0 for an op the layer lacks; [8+8l+5..7] as the namesake writes them.
 * opts->allreduce is NEVER called: with every exponent stated there is no maximum to exchange, and ranks that pass the same
 * exps agree without talking.  A grouped call runs its groups one after the other.
 * Checked before the device is touched, in this order: the namesake's checks; S5FXP_EBADARG for a null exps;
 * S5FXP_EUNSUPPORTED for a non-null `traces`; s5fxp_model_exps_check (which refuses a generic model).
 * A fused model whose unpinned forward takes four full reductions per layer (a BatchNorm operand exponent outside 0..15, or a
 * model created under S5FXP_NO_BN_EXT) is served, not refused: the same kernels read the stated exponents, and the residual
 * add runs as the two-plane pass of that route. */
int s5fxp_model_forward_at(const s5fxp_model *m, const int32_t *x, int x_bits, int x_exp, int B, int L, int32_t *y, void *workspace,
                           size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces, const s5fxp_forward_opts *opts,
                           const int32_t *exps, void *stream);
int s5fxp_model_forward_at_f32(const s5fxp_model *m, const float *x, int x_bits, int x_exp, int B, int L, float *y, void *workspace,
                               size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                               const s5fxp_forward_opts *opts, const int32_t *exps, void *stream);
int s5fxp_model_forward_at_i16(const s5fxp_model *m, const int16_t *x, int x_bits, int x_exp, int B, int L, int16_t *y,
                               void *workspace, size_t workspace_bytes, int32_t *status, const s5fxp_layer_trace *traces,
                               const s5fxp_forward_opts *opts, const int32_t *exps, void *stream);

/* FxpSequenceLayer.forward, fxpmodel.py:1110-1161, for layer `layer` of a created model -- the unit the reference's
 * verification walks (fxprun.py:583-727).  x: (B,L,H) int32 device with configuration (x_bits, x_exp); y: (B,L,H) int32
 * device, s5fxp_model_layer_out_bits() bits at the exponent the residual compute_best add chose: written to
 * status[8 + 8*layer + 4] and, when y_exp_dev is not NULL, to that device int.  Runs the generic int32 kernels (exact for
 * any int32 operands) whatever path whole forwards of the model take.  workspace / status / trace (ONE entry) / opts as
 * s5fxp_model_forward; opts->state_in / state_out here are [2][B][P], the carry of this layer alone; opts->groups must be
 * 0 or 1. */
int s5fxp_layer_forward(const s5fxp_model *m, int layer, const int32_t *x, int x_bits, int x_exp, int B, int L, int32_t *y,
                        int32_t *y_exp_dev, void *workspace, size_t workspace_bytes, int32_t *status,
                        const s5fxp_layer_trace *trace, const s5fxp_forward_opts *opts, void *stream);
int s5fxp_model_layer_out_bits(const s5fxp_model *m, int layer);
/* States of `layer` whose rows of B_bar are not all zero.  The others receive Bu = 0 at every step and stay (0, 0) from a
 * zero carry (fxpmodel.py:147-172), so their columns of C multiply zeros: when at most P / 2 states are live, forwards on
 * the fused path that neither trace the states nor carry them in or out run the layer's kernels on the fewest groups of 32
 * state slots that hold the live ones (32 or 64 of 128, 32 of 64; layers of 32 or 96 states -- the N-DNS recipe at
 * dim_scale 0.25 and 0.75 -- always run on all of them: the rule needs P to be a multiple of 64)
 * (bit-identical; S5FXP_NO_COMPACT at model creation switches it off).  -1: bad argument. */
int s5fxp_model_live_states(const s5fxp_model *m, int layer);

/* Static facts about a created model (for INTEGRATION / debugging). */
int s5fxp_model_out_exp(const s5fxp_model *m);
int s5fxp_model_out_bits(const s5fxp_model *m);
/* 1 if the int8-MFMA kernels were packed for this model (the N-DNS recipe's shapes at dim_scale 0.25, 0.5, 0.75 and 1.0:
 * (H, P) = (48, 32), (96, 64), (144, 96), (192, 128); <= 8-bit weights, <= 16-bit activations, 257 <= d_in <= 288,
 * d_out <= 288); every forward of such a model runs them, whatever B and L (a sequence's last 4-step block may be
 * partial: L = 3751, the N-DNS clips' native length, or single frames of a stream).  status[2] reports it per forward. */
int s5fxp_model_is_fast(const s5fxp_model *m);
/* Which recurrence kernel an optimistic forward (S5FXP_FWD_DEFER_REDO) runs for `layer`:
 * 0 one lane per state (generic), 1 quad kernel with int32 streams, 2 quad kernel with int16 streams,
 * 3 pair kernel (int32 K stream in, int16 states out; sparseRNNs/fxpmodel.py:147-172 in four instructions per step),
 * 4 the same pair kernel fed through LDS by a helper wave from an int16 Bu stream (the default where it applies).
 * (Status word [8 + 8*l + 5] uses two more codes that this query never returns: 5 = the exact 32-bit quad chain of a
 * S5FXP_FWD_EXACT forward, 6 = the plain 32-bit recurrence that runs inside s5fxp_model_step's one kernel.)
 * -1: bad argument.  The exact re-run (S5FXP_FWD_EXACT) always uses the 32-bit quad kernel on the MFMA path. */
int s5fxp_model_recurrence_kernel(const s5fxp_model *m, int layer);
/* The bound on |state| up to which that kernel is exact, as the forward checks it: on every stored state by the consumer
 * of the states, on the carry in (state_in) by the recurrence kernel itself; beyond it S5FXP_ST_REDO is raised / the exact
 * kernels run.  Pair kernels (3, 4): the value checked, 32766 at most, less when the layer's coefficients and Bu width leave
 * less room.  Quad kernel with int16 streams (2): min(the quad kernel's bound, 32766), the value checked.  Quad kernel with
 * int32 streams (1): the quad kernel's bound (2^31 - 1 - 2^16) / max|A * 2^(16 - exp)|; a generic model checks exactly that,
 * a default (not DEFER_REDO) forward on the fused path checks min(that, 32767), the reach of its 16-bit state planes.
 * 0: no bound (generic 32-bit recurrence), -1: bad argument. */
int s5fxp_model_recurrence_xmax(const s5fxp_model *m, int layer);

/* ------------------------------------------------------------------------------------------
 * The FLOAT model, whole: the forward every integer path approximates and is calibrated from (the reference's float
 * S5 model with prenorm BatchNorm on running statistics, relufication, GLU "half1": sparseRNNs/model/layers.py:181-243,
 * model/ssm.py:84-185).  float32 throughout; the scan is s5fxp_assoc_scan_c64, the four kernels around it contract on the
 * exact f32 MFMA (csrc/float_model.hpp).  2 + 3 * n_layers launches.  Results agree with a float64 evaluation to float32
 * rounding (tests/test_float_model.py states the bounds), not bit for bit with any other float32 implementation.
 *
 * Parameters are HOST pointers, as in s5fxp_model_desc; s5fxp_float_model_create packs them into the caller's device blob:
 * every tensor on a 256-byte boundary, the encoder kernel as (260,H) with rows 257..259 zero (K padded to the MFMA's k = 4),
 * the decoder kernel as (H,272) with columns 257..271 zero, inv_std = 1 / sqrtf(var + 1e-5f), B_bar as (H,2P) and C as (2P,H)
 * with re / im interleaved along P (the im rows of C negated), scale = 1 and bias = 0 where the model has none.
 * Served: d_in = d_out = 257 and (H, P) = (48, 32), (96, 64), (144, 96), (192, 128); anything else S5FXP_EUNSUPPORTED. */
typedef struct {
    const float *mean, *var;     /* (H) BatchNorm running statistics */
    const float *scale, *bias;   /* (H) or NULL */
    const float *lambda_bar;     /* (P) complex64, re / im interleaved: the discretised diagonal */
    const float *B_bar;          /* (P,H) complex64 */
    const float *C;              /* (H,P) complex64 */
    const float *D;              /* (H) */
    const float *w2, *b2;        /* out2: (H,H) kernel, (H) bias */
} s5fxp_float_layer_desc;

typedef struct {
    int32_t n_layers, d_in, H, P, d_out;
    const float *enc_w, *enc_b;  /* (d_in,H), (H) */
    const s5fxp_float_layer_desc *layers;
    const float *dec_w, *dec_b;  /* (H,d_out), (d_out) */
} s5fxp_float_model_desc;

typedef struct s5fxp_float_model s5fxp_float_model; /* opaque host handle */

/* Bytes of the packed blob; 0 for a description s5fxp_float_model_create refuses. */
size_t s5fxp_float_model_blob_bytes(const s5fxp_float_model_desc *desc);
/* The blob exactly as s5fxp_float_model_create uploads it, written to HOST memory (never touches the device). */
int s5fxp_float_model_pack(const s5fxp_float_model_desc *desc, void *host_blob, size_t blob_bytes);
/* S5FXP_EBADARG for a null or non-positive field, S5FXP_EUNSUPPORTED for a shape outside the list above, S5FXP_EWORKSPACE
 * for a blob that is too small -- all before the device is touched. */
int s5fxp_float_model_create(const s5fxp_float_model_desc *desc, void *dev_blob, size_t blob_bytes, void *stream,
                             s5fxp_float_model **out);
void s5fxp_float_model_destroy(s5fxp_float_model *m);

/* Device workspace of one forward: two (N,H) planes for the layer input and output and the (N,P) complex64 planes Bu and xs,
 * N = B * L -- one pair shared by all layers, or with trace != 0 one pair per layer, kept: floats
 * [2 N H][layer 0: Bu, xs][layer 1: ...].  0: bad argument, or a size that does not fit a size_t (checked arithmetic, never
 * a wrapped value); the forwards refuse such a (B, L) with S5FXP_EWORKSPACE before the device is touched.  The workspace, y and
 * the trace planes may hold anything on entry, NaN included: nothing of it reaches y, an observer or a histogram. */
size_t s5fxp_float_workspace_bytes(const s5fxp_float_model *m, int B, int L, int trace);
/* Bytes of the trace buffer: per layer five (N,H) float32 planes u, y, g_in, g, h' (the layer's output), layer after layer. */
size_t s5fxp_float_trace_bytes(const s5fxp_float_model *m, int B, int L);

/* x: (B,L,257) float32 device; y: (B,L,257) float32 device.
 * stats: NULL, or 4 + 10 * n_layers float32 in device memory, the absmax observers in the key order of the reference's
 * calibration run: encoder.inp, encoder.out, per layer u, Bu_re, Bu_im, x_re, x_im (raw states), y, out2.inp, out2.out,
 * gate.l, gate.r, then decoder.inp, decoder.out.  The entry only ever RAISES the array (one atomic max per observer and
 * workgroup, on the value's bits): zero it before the first batch and stream a calibration set through.  A NaN in a plane
 * reaches its observer as NaN.
 * trace: NULL, or s5fxp_float_trace_bytes of device memory that receives every intermediate plane; Bu and xs of every layer
 * are then left in the workspace.  y and stats are bit-identical with and without it.
 * S5FXP_EBADARG for a null model / x / y / workspace or B, L < 1; S5FXP_EWORKSPACE for a workspace that is too small. */
int s5fxp_float_model_forward(const s5fxp_float_model *m, const float *x, int B, int L, float *y, float *stats, float *trace,
                              void *workspace, size_t workspace_bytes, void *stream);

/* The same forward, which also gathers one HISTOGRAM OVER THE FLOAT32 EXPONENT FIELD per observer.  For a
 * float32 v with E = (bits(v) >> 23) & 0xff the bin is clamp(E - 87, 0, 63): bin b in 1..62 holds
 * 2^(b + S5FXP_FLOAT_HIST_EMIN) <= |v| < 2^(b + S5FXP_FLOAT_HIST_EMIN + 1), bin 0 everything below 2^-39 (zero and subnormals
 * included), bin 63 |v| >= 2^23, infinities and NaN.  So the sum of the bins from k + 40 on is exactly the number of values
 * with |v| >= 2^k, for -39 <= k <= 23 -- every threshold of a fixed-point configuration is such a power of two.
 * hist: NULL, or (4 + 10 * n_layers) * S5FXP_FLOAT_HIST_BINS 64-bit counters in device memory, 8-byte aligned, one row per
 * observer in the order of stats (gate.l has a row of its own, equal to out2.inp's).  A value enters its row exactly where
 * it enters its observer: rows beyond N and padded columns never do.  The entry only ever ADDS to the array (per workgroup
 * one 64-bit atomic add for every counter it found non-zero): zero it before the first batch.
 * With hist == NULL the kernels launched are those of the entry above; y, stats and the trace planes are bit-identical with
 * and without hist, and the workspace and trace sizes are the same.
 * Wrap rule: a workgroup counts in 32-bit words of LDS and adds them to hist once, at its end.  It sees at most
 * ceil(tiles / grid) * 32 rows * 272 values of one observer (tiles = ceil(B L / 32), grid = min(tiles, 512)); a B * L at
 * which that product reaches 2^32 (B * L above about 8.08e9) is refused with S5FXP_EBADARG when hist is given.
 * S5FXP_EBADARG also for a hist that is not 8-byte aligned; otherwise the errors of the entry above. */
#define S5FXP_FLOAT_HIST_BINS 64
#define S5FXP_FLOAT_HIST_EMIN (-40)
int s5fxp_float_model_forward_hist(const s5fxp_float_model *m, const float *x, int B, int L, float *y, float *stats,
                                   unsigned long long *hist, float *trace, void *workspace, size_t workspace_bytes,
                                   void *stream);

/* The float forward over n CLIPS OF DIFFERENT LENGTHS in the same 2 + 3 * n_layers launches.
 * x: (n,Lmax,257) float32 device, padded; y: (n,Lmax,257) float32 device, padded.
 * lens: n int32 in DEVICE memory, exactly what s5fxp_stft_mag_clips writes; clip e has len_e = clamp(lens[e], 0, Lmax) frames.
 * Rows t < len_e of y, and what stats and hist receive, are bit for bit those of s5fxp_float_model_forward[_hist] on clip e
 * alone (B = 1, L = len_e).  Rows from len_e on of x are never read and of y never written, and no padding row enters an
 * observer or a histogram: a clip with len_e == 0 leaves y untouched and contributes nothing, and a launch whose clips are
 * all empty returns 0 and changes nothing.
 * stats, hist: as in s5fxp_float_model_forward_hist -- NULL switches each off, stats is only raised, hist only added to; with
 * hist == NULL the kernels without the histogram run, and y and stats are bit-identical with and without hist.
 * workspace: s5fxp_float_workspace_bytes(m, n, Lmax, 0).  There are no trace planes.
 * Errors, all before the device is touched: S5FXP_EBADARG for a null model / x / y / lens / workspace, for n < 1 or Lmax < 1,
 * for a hist that is not 8-byte aligned, and, when hist is given, for an n * ceil(Lmax / 32) at which the wrap rule above is
 * reached (tiles = n * ceil(Lmax / 32)); S5FXP_EWORKSPACE for a workspace that is too small. */
int s5fxp_float_model_clips(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens, float *y,
                            float *stats, unsigned long long *hist, void *workspace, size_t workspace_bytes, void *stream);

/* The float forward with chosen tensors FAKE-QUANTISED: every observed tensor has a site, and a site that is
 * on replaces the value, in the statement right after it entered its observer, by
 *     q(v) = clamp(R(v * 2^exp), -2^(bits-1), 2^(bits-1) - 1) * 2^-exp,   R = floor or round-half-to-even by `mode`,
 * the clamp left out when saturate == 0.  NaN stays NaN; either zero may come out.  Within the accepted fields both products
 * and the rounded integer are exact in float32, so q is one exactly defined float32 function (floatmodel.fake_quant).
 * Observers keep their place and meaning: under fake quantisation one reports the range its tensor has when everything
 * upstream is quantised.  u is quantised in both kernels that build it, Bu before it is stored (the scan runs on quantised
 * Bu), the raw state where the gate kernel reads it, before the complex ReLU, which decides on the quantised pair; the
 * rounding inside the integer recurrence is not modelled, and the scan itself is unchanged.  gate.l and out2.inp quantise
 * the same value, each for its own consumer.  The trace planes u, y, g_in, g, the workspace's Bu and y hold what
 * downstream consumed (post-quantiser); xs stays raw.
 * fq: NULL, or 4 + 10 * n_layers sites in HOST memory in the order of stats, read before the entry returns.  bits == 0
 * switches a site off.  With fq == NULL or every site off the kernels launched are exactly those of
 * s5fxp_float_model_forward / s5fxp_float_model_clips.  There is no histogram together with fake quantisation.
 * S5FXP_EBADARG, before the device is touched, for bits outside {0, 2..24}, exp outside -24..40, an unknown mode, a saturate
 * other than 0 / 1, and saturate == 1 on a state site (x_re, x_im: the integer model wraps its state, it does not clip it);
 * every other argument, error, and the workspace and trace sizes as in the entries without fq.
 * mode S5FXP_FQ_STEP is accepted on the state sites x_re / x_im only, on both of a layer together and with
 * saturate == 0: that layer's recurrence is then s5fxp_fq_scan_c64 at the two sites' exponents in place of the associative
 * scan (for clips with lens), so the rounding of the integer recurrence is inside the loop and fed back through the pole.
 * The gate kernel gets the two sites as off (the states are on their grids already); the observers keep their place; bits
 * is checked and unused.  S5FXP_EBADARG for the mode on any other site, on one state site of a layer only, and for a shape
 * s5fxp_fq_scan_c64 refuses.  A spec without step sites launches exactly what it launched without this mode. */
typedef struct {
    int8_t bits, exp;
    uint8_t mode, saturate;
} s5fxp_float_fq_site;
enum { S5FXP_FQ_FLOOR = 0, S5FXP_FQ_NEAREST = 1, S5FXP_FQ_STEP = 2 };
int s5fxp_float_model_forward_fq(const s5fxp_float_model *m, const float *x, int B, int L, float *y, float *stats,
                                 const s5fxp_float_fq_site *fq, float *trace, void *workspace, size_t workspace_bytes,
                                 void *stream);
int s5fxp_float_model_clips_fq(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens, float *y,
                               float *stats, const s5fxp_float_fq_site *fq, void *workspace, size_t workspace_bytes,
                               void *stream);
/* The clip forward WITH TRACE PLANES, with or without fake quantisation (fq may be NULL; no histogram is
 * offered).  trace: s5fxp_float_trace_bytes(m, n, Lmax) bytes, never NULL (S5FXP_EBADARG); workspace:
 * s5fxp_float_workspace_bytes(m, n, Lmax, 1), so every layer's Bu and xs stay there, as in the rectangular traced forward.
 * Every plane is padded like y.  Rows t < len_e of h_enc (the workspace's first plane), of u / y / g_in / g / h' and of Bu / xs
 * of every layer are bit for bit those of s5fxp_float_model_forward[_fq] with a trace on clip e alone; rows from len_e on are
 * never written.  y and stats are bit-identical to s5fxp_float_model_clips[_fq].  S5FXP_FQ_STEP layers run s5fxp_fq_scan_c64
 * with lens.  Every other argument and error as s5fxp_float_model_clips_fq. */
int s5fxp_float_model_clips_traced(const s5fxp_float_model *m, const float *x, int n, int Lmax, const int32_t *lens, float *y,
                                   float *stats, const s5fxp_float_fq_site *fq, float *trace, void *workspace,
                                   size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Stage errors: two sides of a forward compared where they lie (csrc/stage_err.hpp).  One call compares up to
 * 4096 PAIRS of planes in two launches, an accumulate kernel and a finalize kernel, whatever the number of pairs, and leaves
 * per pair the sums behind the verification report's figures (sparseRNNs/fxpreporter.py:12-24, compute_error).
 *
 * A pair is a 3-D box (nb, rows, cols) read from two sides with element strides, so a whole (B,L,H) plane, the real or the
 * imaginary half of an interleaved complex64 plane (column stride 2), one sequence of a batch and one time bucket of all
 * sequences are all boxes of the planes the engines leave behind, without a copy.  Strides may be any int64, zero and
 * negative included; the kernels trust them as they trust pointers.
 *
 * Arithmetic, for every element (the NumPy statement is verify.stage_errors_host):
 *   va = (double)a * 2^-a_exp, exact for any int32 (S5FXP_STAGE_I32), or (double)a of a float32 a (S5FXP_STAGE_F32);
 *   vb = (double)b; an element whose a or b is an infinity or a NaN is counted in n_nonfinite and enters nothing else;
 *   with S5FXP_STAGE_RELU_A a negative va is replaced by 0; e = |va - vb|, one rounding; where vb != 0, rel = e / |vb|,
 *   one rounding.  -0 equals +0.  sum_sq adds the rounded squares e * e, sum_ref_sq the exact squares vb * vb.
 * hist_abs / hist_rel bin (float)e / (float)rel by the float32 exponent field with the rule of S5FXP_FLOAT_HIST_BINS above
 * (hist_rel over the elements with vb != 0): each brackets its median to a factor of two and counts the errors at or above
 * any power of two 2^-39 .. 2^23.
 * Counts, histograms and the two maxima are exact.  The four sums are taken in double, per thread, then lanes, waves and
 * workgroups in a fixed order, with no floating-point atomics: two calls give identical bits, and any order of summing n
 * non-negative doubles is within (n - 1) * 2^-53 relative of the exact sum.
 *
 * pairs_host: HOST memory, read before the entry returns.  out_dev: n_pairs records in device memory, 8-byte aligned.
 * workspace: s5fxp_stage_err_workspace_bytes(n_pairs) bytes of device memory, 256-byte aligned, overwritten by the call
 * (0 for n_pairs outside 1..4096); it and out_dev may hold anything on entry, every record is written completely.  A pair with
 * a zero extent is legal (its pointers may be NULL) and gets an all-zero record.
 * S5FXP_EBADARG, before the device is touched: a null pairs_host / out_dev / workspace, or a null a / b of a pair that has
 * elements; n_pairs outside 1..4096; an unknown kind or unknown flag bits; a_exp outside 0..40 on an I32 pair; a negative
 * extent; and the wrap rule: a workgroup counts in 32-bit words, so a pair of more than (2^32 - 256) * W elements is refused,
 * W = min(512, max(1, 16384 / n_pairs)) the most workgroups the call gives a pair.  S5FXP_EWORKSPACE for a workspace that is
 * too small. */
enum { S5FXP_STAGE_I32 = 0, S5FXP_STAGE_F32 = 1 }; /* s5fxp_stage_pair.a_kind */
enum { S5FXP_STAGE_RELU_A = 1 };                   /* s5fxp_stage_pair.flags */
typedef struct {
    const void *a;       /* device; int32 or float32 by a_kind */
    int32_t a_kind;
    int32_t a_exp;       /* S5FXP_STAGE_I32: value = a * 2^-a_exp; S5FXP_STAGE_F32: ignored */
    const float *b;      /* device; the reference side ("xhat"), float32 */
    int64_t a_stride[3]; /* elements; batch, row, column */
    int64_t b_stride[3];
    int32_t nb, rows, cols;
    int32_t flags;       /* S5FXP_STAGE_RELU_A: max(a, 0) before comparing */
} s5fxp_stage_pair;      /* 88 bytes */
typedef struct {
    uint64_t n;             /* elements of the box */
    uint64_t n_nonfinite;   /* of them not compared */
    uint64_t n_equal;       /* compared with e == 0 */
    uint64_t n_ref_nonzero; /* compared with vb != 0 */
    double sum_abs, sum_sq, max_abs; /* of e */
    double sum_ref_sq;               /* of vb, over the compared elements */
    double sum_rel, max_rel;         /* of rel */
    uint64_t hist_abs[S5FXP_FLOAT_HIST_BINS], hist_rel[S5FXP_FLOAT_HIST_BINS];
} s5fxp_stage_err_rec;      /* 1104 bytes */
size_t s5fxp_stage_err_workspace_bytes(int n_pairs);
int s5fxp_stage_err(const s5fxp_stage_pair *pairs_host, int n_pairs, s5fxp_stage_err_rec *out_dev, void *workspace,
                    size_t workspace_bytes, void *stream);

/* The same comparison over CLIPS OF DIFFERENT LENGTHS (k_stage_err_clips).  A pair is a box (nb = clips, rows,
 * cols) of two PADDED planes, as both traced clip forwards leave them, plus
 *   lens          nb int32 in device memory: clip b of the box reads lens[b];
 *   row0          the frame index of the box's row 0 inside its clip (a time bucket t0..t1 is row0 = t0, rows = t1 - t0);
 *   a_exp_dev, a_exp_stride   device memory or NULL.  When set, the integer side of clip b has the exponent
 *                 a_exp_dev[b * a_exp_stride], read on the device -- word 8 + 8 l + k of the clips' status words with stride
 *                 S5FXP_STATUS_WORDS gives every clip its own compute_best exponent -- and box.a_exp is ignored; with NULL
 *                 box.a_exp is used, as in s5fxp_stage_err.  Ignored for a float32 a.
 * Element (b, r, c) is compared iff row0 + r < lens[b].  Elements outside belong to no count and are NEVER READ: the padding
 * of the planes may hold anything, NaN and poison included.  rec.n is the number of elements inside.  A clip whose device
 * exponent is outside 0..40 contributes its elements to n and n_nonfinite and to nothing else.  The per-element arithmetic,
 * the record, the two launches (the finalize kernel is s5fxp_stage_err's), no floating-point atomics and identical bits from
 * run to run, and the 4096-pair cap are those of s5fxp_stage_err; the wrap rule is applied to the PADDED box.  One pair per
 * stage over all clips is by="stage"; the same box with nb = 1 and lens + e is one clip.
 * workspace: s5fxp_stage_err_clips_workspace_bytes(n_pairs), 256-byte aligned (the descriptors are larger than
 * s5fxp_stage_err's; the partial records are the same).
 * S5FXP_EBADARG, before the device is touched: what s5fxp_stage_err refuses (a_exp only without a_exp_dev), a null lens on a
 * pair with elements, a negative row0, a non-zero reserved.  S5FXP_EWORKSPACE for a workspace that is too small. */
struct s5fxp_stage_pair_clips {
    s5fxp_stage_pair box;     /* nb = clips; a_stride[0] / b_stride[0]: from one clip to the next */
    const int32_t *lens;      /* device */
    const int32_t *a_exp_dev; /* device or NULL */
    int64_t a_exp_stride;     /* int32 words */
    int32_t row0;
    int32_t reserved;         /* 0 */
};                            /* 120 bytes */
typedef struct s5fxp_stage_pair_clips s5fxp_stage_pair_clips;
size_t s5fxp_stage_err_clips_workspace_bytes(int n_pairs);
int s5fxp_stage_err_clips(const s5fxp_stage_pair_clips *pairs_host, int n_pairs, s5fxp_stage_err_rec *out_dev, void *workspace,
                          size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* S5FXP_H */
