// float_model_kernels.inc -- the float model's four tile kernels (encoder, B projection, gate, decoder), written once.
// float_model.hpp includes this file once per form, six times (no include guard), and states before each inclusion only what
// tells the form from the others: three 0/1 flags and the kernel-name suffix,
//   FM_HIST    count every value into its observer's exponent histogram where it enters the observer (DESIGN.md 4s);
//   FM_CLIPS   run n clips of different lengths: a tile maps to one clip's rows through an FClipMap (DESIGN.md 4t);
//   FM_FAKEQ   fake-quantise the observed tensors whose site is on (DESIGN.md 4u); built without the histogram;
//   FM_KERNEL(name)  name##_suffix: none, _hist, _clips, _clips_hist, _fq, _clips_fq.
// The prologue below derives from the flags every macro the kernel text uses, the epilogue at the foot undefines them and
// the flags and FM_KERNEL with them, so no macro state goes from one inclusion to the next:
//   FM_CLIPS_PARAM, FM_HIST_PARAM, FM_FQ_PARAM(n)  the parameters a form takes after the kernel's argument struct:
//       `FClipMap cm`, `unsigned long long *hist`, `FFq<n> fq`, each only in its form;
//   FM_TILES(N), FM_TILE(tile, N, r0, rows)  the launch's tile count, and the declaration of a tile's first row r0 and its
//       valid row prefix `rows`: rows 32 * tile .. of N, or the rows the tile's clip has there (a tile without rows is
//       skipped);
//   FM_GATE_ATTR  the gate kernel's occupancy attribute in the clip forms;
//   FM_HIST_BEGIN(planes), FM_HIST_ADD(plane, v), FM_HIST_END(planes[, dup_src, dup_row])  the workgroup's LDS histograms:
//       set up, one value in, flush; all three empty without FM_HIST;
//   FM_FQ(site, v)  fm_fq(v, fq.s[site]), the value the site hands downstream, placed right behind the statement where v
//       enters its observer; FM_FQ2(odd, site_odd, site_even, v) chooses between two sites by a lane predicate;
//       FM_FQ_V4(site, v) / FM_FQ_V2(site_x, site_y, v) are statements that quantise a float4 by one site / a float2 by one
//       site per component in place.  Without FM_FAKEQ the first two are (v) and the statements are empty.
// Not a translation unit of its own; everything it uses is declared in float_model.hpp, inside namespace s5.
#if !defined(FM_HIST) || !defined(FM_CLIPS) || !defined(FM_FAKEQ) || !defined(FM_KERNEL) || (FM_HIST && FM_FAKEQ)
#error "float_model_kernels.inc: define FM_HIST, FM_CLIPS, FM_FAKEQ (0/1, not FM_HIST with FM_FAKEQ) and FM_KERNEL(name)"
#endif

#if FM_CLIPS
#define FM_CLIPS_PARAM , FClipMap cm
#define FM_TILES(N) cm.tiles
// the clip's tile: rows = clamp(len - t0, 0, 32) stays a contiguous prefix; a tile without rows is left before its first
// load (workgroup-uniform, so the barriers stay matched)
#define FM_TILE(tile, N, r0, rows)                                                                   \
    const int clip_ = (int)(tile / cm.tpc), t0_ = FM_FT * (int)(tile - (long long)clip_ * cm.tpc); \
    const int raw_ = cm.lens[clip_], len_ = raw_ < cm.Lmax ? raw_ : cm.Lmax;                         \
    const int rows = len_ - t0_ < FM_FT ? len_ - t0_ : FM_FT;                                        \
    if (rows <= 0) continue;                                                                         \
    const long long r0 = (long long)clip_ * cm.Lmax + t0_
// the clip mapping's row addresses cost k_fgate_clips<2> ten VGPRs (246 for the rectangular kernel's 236), one granule past
// two waves per SIMD, and at one wave it ran 196 us for the rectangular kernel's 122; asked for two, the allocator fits 240
// without scratch
#define FM_GATE_ATTR __attribute__((amdgpu_waves_per_eu(DS == 2 ? 2 : 1)))
#else
#define FM_CLIPS_PARAM
#define FM_TILES(N) (((N) + FM_FT - 1) / FM_FT)
#define FM_TILE(tile, N, r0, rows)     \
    const long long r0 = tile * FM_FT; \
    const int rows = (int)(N - r0 < FM_FT ? N - r0 : FM_FT)
#define FM_GATE_ATTR
#endif

#if FM_HIST
#define FM_HIST_PARAM , unsigned long long *hist
#define FM_HIST_BEGIN(planes)                       \
    unsigned *const shist = fm_hist_lds<planes>(); \
    fm_hist_zero<planes>(shist)
#define FM_HIST_ADD(plane, v) fm_hist_add(shist, plane, v)
#define FM_HIST_END(...) fm_hist_flush<__VA_ARGS__>(shist, hist)
#else
#define FM_HIST_PARAM
#define FM_HIST_BEGIN(planes)
#define FM_HIST_ADD(plane, v)
#define FM_HIST_END(...)
#endif

#if FM_FAKEQ
#define FM_FQ_PARAM(n) , FFq<n> fq
#define FM_FQ(site, v) fm_fq(v, fq.s[site])
#define FM_FQ2(odd, site_odd, site_even, v) ((odd) ? fm_fq(v, fq.s[site_odd]) : fm_fq(v, fq.s[site_even]))
#define FM_FQ_V4(site, v) v = make_float4(fm_fq(v.x, fq.s[site]), fm_fq(v.y, fq.s[site]), fm_fq(v.z, fq.s[site]), fm_fq(v.w, fq.s[site]))
#define FM_FQ_V2(site_x, site_y, v) v = make_float2(fm_fq(v.x, fq.s[site_x]), fm_fq(v.y, fq.s[site_y]))
#else
#define FM_FQ_PARAM(n)
#define FM_FQ(site, v) (v)
#define FM_FQ2(odd, site_odd, site_even, v) (v)
#define FM_FQ_V4(site, v)
#define FM_FQ_V2(site_x, site_y, v)
#endif

// ------------------------------------------------------------------------------------------------------------------
// encoder: h = relu(x W + b); observers [0] encoder.inp, [1] encoder.out (before the ReLU)
// ------------------------------------------------------------------------------------------------------------------

template <int DS>
__global__ __launch_bounds__(256) void FM_KERNEL(k_fenc)(FEncArgs a FM_CLIPS_PARAM FM_HIST_PARAM FM_FQ_PARAM(2)) // hist: rows encoder.inp, encoder.out
{
    constexpr int H = 48 * DS, HT = 3 * DS, NT = (HT + 3) / 4, KS = FM_KENC / 4, LDA = fm_lda(FM_KENC);
    __shared__ float sx[FM_FT * LDA];
    __shared__ unsigned sobs[FM_WAVES * 2];
    FM_HIST_BEGIN(2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float breg[NT][KS];
    fm_load_w<KS, NT>(breg, a.w, H, HT);
    float bias[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = wave + FM_WAVES * nt;
        bias[nt] = t < HT ? a.b[t * 16 + (lane & 15)] : 0.f;
    }
    unsigned om[2] = {0u, 0u};
    const long long tiles = FM_TILES(a.N);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        FM_TILE(tile, a.N, r0, rows); // const long long r0, const int rows: the tile's first row and its valid prefix
        // rows are 257 floats: dword loads, all of a thread's issued before the first is used.  Addresses are clamped into the
        // tile's valid rows and columns, so no load is conditional; what lies outside is replaced by zero afterwards.
        const float *src = a.x + (size_t)r0 * FM_DIN;
        constexpr int PER = (FM_FT * FM_KENC + 255) / 256;
        float v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + 256 * j, r = i / FM_KENC, c = i - r * FM_KENC;
            const int rc = r < rows ? r : rows - 1, cc = c < FM_DIN ? c : FM_DIN - 1;
            v[j] = src[(size_t)rc * FM_DIN + cc];
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + 256 * j, r = i / FM_KENC, c = i - r * FM_KENC;
            if (i >= FM_FT * FM_KENC) continue; // the last round is partial: 8320 = 32.5 x 256
            const bool ok = r < rows && c < FM_DIN;
            const float w = ok ? v[j] : 0.f;
            if (ok) {
                om[0] = fm_umax(om[0], fm_absbits(w));
                FM_HIST_ADD(0, w);
            }
            sx[r * LDA + c] = FM_FQ(0, w);
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS, NT>(acc, sx, LDA, breg, HT);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= HT) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows) continue;
                    const float v = __fadd_rn(acc[rt][nt][r], bias[nt]);
                    om[1] = fm_umax(om[1], fm_absbits(v));
                    FM_HIST_ADD(1, v);
                    a.h[(size_t)(r0 + row) * H + t * 16 + (lane & 15)] = fm_relu(FM_FQ(1, v));
                }
            }
        __syncthreads();
    }
    fm_obs_flush<2>(om, sobs, a.stats);
    FM_HIST_END(2);
}

// ------------------------------------------------------------------------------------------------------------------
// B projection: u = BatchNorm(h); Bu = u B_bar^T as ONE real product against bcat (H, 2P) whose columns interleave re and
// im, so the result is the (N,P) complex64 plane the scan takes.  Observers [0] u, [1] Bu_re, [2] Bu_im.
// ------------------------------------------------------------------------------------------------------------------

template <int DS, bool TRACE>
__global__ __launch_bounds__(256) void FM_KERNEL(k_fbproj)(FBprojArgs a FM_CLIPS_PARAM FM_HIST_PARAM FM_FQ_PARAM(3)) // hist: rows u, Bu_re, Bu_im
{
    constexpr int H = 48 * DS, P2 = 64 * DS, PT = 4 * DS, NT = DS, KS = H / 4, LDA = fm_lda(H);
    __shared__ float su[FM_FT * LDA];
    __shared__ float snm[4 * H];
    __shared__ unsigned sobs[FM_WAVES * 3];
    FM_HIST_BEGIN(3);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float breg[NT][KS];
    fm_load_w<KS, NT>(breg, a.bcat, P2, PT);
    for (int i = threadIdx.x; i < H; i += 256) {
        snm[i] = a.nm.mean[i]; snm[H + i] = a.nm.istd[i]; snm[2 * H + i] = a.nm.scale[i]; snm[3 * H + i] = a.nm.bias[i];
    }
    __syncthreads();
    unsigned om_u = 0u, om_bu = 0u; // a lane's Bu columns all have the lane's parity: even = re, odd = im
    const long long tiles = FM_TILES(a.N);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        FM_TILE(tile, a.N, r0, rows); // const long long r0, const int rows: the tile's first row and its valid prefix
        for (int i = threadIdx.x; i < FM_FT * (H / 4); i += 256) {
            const int r = i / (H / 4), c = (i - r * (H / 4)) * 4;
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) {
                const float4 h = *reinterpret_cast<const float4 *>(a.h + (size_t)(r0 + r) * H + c);
                u.x = fm_bn(h.x, snm[c], snm[H + c], snm[2 * H + c], snm[3 * H + c]);
                u.y = fm_bn(h.y, snm[c + 1], snm[H + c + 1], snm[2 * H + c + 1], snm[3 * H + c + 1]);
                u.z = fm_bn(h.z, snm[c + 2], snm[H + c + 2], snm[2 * H + c + 2], snm[3 * H + c + 2]);
                u.w = fm_bn(h.w, snm[c + 3], snm[H + c + 3], snm[2 * H + c + 3], snm[3 * H + c + 3]);
                om_u = fm_umax(fm_umax(fm_umax(om_u, fm_absbits(u.x)), fm_umax(fm_absbits(u.y), fm_absbits(u.z))), fm_absbits(u.w));
                FM_HIST_ADD(0, u.x);
                FM_HIST_ADD(0, u.y);
                FM_HIST_ADD(0, u.z);
                FM_HIST_ADD(0, u.w);
                FM_FQ_V4(0, u);
                if (TRACE) *reinterpret_cast<float4 *>(a.u_trace + (size_t)(r0 + r) * H + c) = u;
            }
            *reinterpret_cast<float4 *>(su + r * LDA + c) = u;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS, NT>(acc, su, LDA, breg, PT);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt; // < PT always: PT = 4 * NT
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows) continue;
                    const float v = acc[rt][nt][r];
                    om_bu = fm_umax(om_bu, fm_absbits(v));
                    FM_HIST_ADD(1 + (lane & 1), v);
                    a.bu[(size_t)(r0 + row) * P2 + t * 16 + (lane & 15)] = FM_FQ2(lane & 1, 2, 1, v);
                }
            }
        __syncthreads();
    }
    const unsigned om[3] = {om_u, (lane & 1) ? 0u : om_bu, (lane & 1) ? om_bu : 0u};
    fm_obs_flush<3>(om, sobs, a.stats);
    FM_HIST_END(3);
}

// ------------------------------------------------------------------------------------------------------------------
// gate: complex ReLU on the raw states, y = 2 (x_re C_re^T - x_im C_im^T) + D u as ONE real product of the interleaved
// rectified states against ccat (2P,H) = rows (C_re^T, -C_im^T) interleaved, with u rebuilt from the layer input;
// x1 = relu(y), g_in = x1 W2 + b2, g = sigmoid(g_in), h' = relu(x1 g + h).
// Observers [0] x_re, [1] x_im (raw states), [2] y, [3] out2.inp, [4] out2.out, [5] gate.l (= out2.inp), [6] gate.r.
// Sites: [0] u (the layer's u, rebuilt here exactly as k_fbproj quantised it), then [1 + i] for observer [i].
// ------------------------------------------------------------------------------------------------------------------

template <int DS, bool TRACE>
__global__ __launch_bounds__(256) FM_GATE_ATTR void FM_KERNEL(k_fgate)(FGateArgs a FM_CLIPS_PARAM FM_HIST_PARAM FM_FQ_PARAM(8)) // hist: the layer's rows x_re .. gate.r
{
    constexpr int H = 48 * DS, P = 32 * DS, P2 = 64 * DS, HT = 3 * DS, NT = (HT + 3) / 4, KS1 = P2 / 4, KS2 = H / 4;
    constexpr int LD1 = fm_lda(P2), LDH = fm_lda(H);
    __shared__ float sxs[FM_FT * LD1];
    __shared__ float sh[FM_FT * LDH];
    __shared__ float sx1[FM_FT * LDH];
    __shared__ float spar[6 * H]; // mean, istd, scale, bias, D, b2
    __shared__ unsigned sobs[FM_WAVES * 7];
    FM_HIST_BEGIN(6); // LDS planes: x_re, x_im, y, out2.inp (= gate.l), out2.out, gate.r
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float bc[NT][KS1], bw[NT][KS2];
    fm_load_w<KS1, NT>(bc, a.ccat, H, HT);
    fm_load_w<KS2, NT>(bw, a.w2, H, HT);
    for (int i = threadIdx.x; i < H; i += 256) {
        spar[i] = a.nm.mean[i]; spar[H + i] = a.nm.istd[i]; spar[2 * H + i] = a.nm.scale[i]; spar[3 * H + i] = a.nm.bias[i];
        spar[4 * H + i] = a.D[i]; spar[5 * H + i] = a.b2[i];
    }
    __syncthreads();
    unsigned o_xre = 0u, o_xim = 0u, o_y = 0u, o_x1 = 0u, o_gin = 0u, o_g = 0u;
    const long long tiles = FM_TILES(a.N);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        FM_TILE(tile, a.N, r0, rows); // const long long r0, const int rows: the tile's first row and its valid prefix
        for (int i = threadIdx.x; i < FM_FT * P; i += 256) {
            const int r = i / P, p = i - r * P;
            float2 v = make_float2(0.f, 0.f);
            if (r < rows) {
                v = *reinterpret_cast<const float2 *>(a.xs + (size_t)(r0 + r) * P2 + 2 * p);
                o_xre = fm_umax(o_xre, fm_absbits(v.x));
                o_xim = fm_umax(o_xim, fm_absbits(v.y));
                FM_HIST_ADD(0, v.x);
                FM_HIST_ADD(1, v.y);
                FM_FQ_V2(1, 2, v);
                const bool keep = v.x > 0.f || (v.x == 0.f && v.y > 0.f);
                if (!keep) v = make_float2(0.f, 0.f);
            }
            *reinterpret_cast<float2 *>(sxs + r * LD1 + 2 * p) = v;
        }
        for (int i = threadIdx.x; i < FM_FT * (H / 4); i += 256) {
            const int r = i / (H / 4), c = (i - r * (H / 4)) * 4;
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) h = *reinterpret_cast<const float4 *>(a.h + (size_t)(r0 + r) * H + c);
            *reinterpret_cast<float4 *>(sh + r * LDH + c) = h;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS1, NT>(acc, sxs, LD1, bc, HT);
        float x1v[2][NT][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= HT) continue;
                const int col = t * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    const float u = FM_FQ(0, fm_bn(sh[row * LDH + col], spar[col], spar[H + col], spar[2 * H + col], spar[3 * H + col]));
                    const float y = __fadd_rn(__fmul_rn(2.f, acc[rt][nt][r]), __fmul_rn(spar[4 * H + col], u));
                    const float yq = FM_FQ(3, y);
                    const float x1 = fm_relu(yq);
                    x1v[rt][nt][r] = FM_FQ(6, x1);      // gate.l: the factor of x1 g
                    sx1[row * LDH + col] = FM_FQ(4, x1); // out2.inp: the operand of the out2 contraction
                    if (row < rows) {
                        o_y = fm_umax(o_y, fm_absbits(y));
                        o_x1 = fm_umax(o_x1, fm_absbits(x1));
                        FM_HIST_ADD(2, y);
                        FM_HIST_ADD(3, x1);
                        if (TRACE) a.y_trace[(size_t)(r0 + row) * H + col] = yq;
                    }
                }
            }
        __syncthreads();
        fm_mma<KS2, NT>(acc, sx1, LDH, bw, HT);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= HT) continue;
                const int col = t * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows) continue;
                    const float gin = __fadd_rn(acc[rt][nt][r], spar[5 * H + col]);
                    const float ginq = FM_FQ(5, gin);
                    const float g = 1.f / (1.f + expf(-ginq));
                    const float gq = FM_FQ(7, g);
                    o_gin = fm_umax(o_gin, fm_absbits(gin));
                    o_g = fm_umax(o_g, fm_absbits(g));
                    FM_HIST_ADD(4, gin);
                    FM_HIST_ADD(5, g);
                    const size_t o = (size_t)(r0 + row) * H + col;
                    a.hout[o] = fm_relu(__fadd_rn(__fmul_rn(x1v[rt][nt][r], gq), sh[row * LDH + col]));
                    if (TRACE) {
                        a.gin_trace[o] = ginq;
                        a.g_trace[o] = gq;
                    }
                }
            }
        __syncthreads();
    }
    const unsigned om[7] = {o_xre, o_xim, o_y, o_x1, o_gin, o_x1, o_g};
    fm_obs_flush<7>(om, sobs, a.stats);
    FM_HIST_END(6, 3, 5); // plane 3 goes to out2.inp and to gate.l
}

// ------------------------------------------------------------------------------------------------------------------
// decoder: out = h Wd + bd; observers [0] decoder.inp, [1] decoder.out.  The 257 columns leave a masked last tile.
// ------------------------------------------------------------------------------------------------------------------

template <int DS>
__global__ __launch_bounds__(256) void FM_KERNEL(k_fdec)(FDecArgs a FM_CLIPS_PARAM FM_HIST_PARAM FM_FQ_PARAM(2)) // hist: rows decoder.inp, decoder.out
{
    constexpr int H = 48 * DS, NT = (FM_DEC_TILES + 3) / 4, KS = H / 4, LDA = fm_lda(H);
    __shared__ float sh[FM_FT * LDA];
    __shared__ unsigned sobs[FM_WAVES * 2];
    FM_HIST_BEGIN(2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float breg[NT][KS];
    fm_load_w<KS, NT>(breg, a.w, FM_MDEC, FM_DEC_TILES);
    float bias[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = wave + FM_WAVES * nt;
        bias[nt] = t < FM_DEC_TILES ? a.b[t * 16 + (lane & 15)] : 0.f;
    }
    unsigned om[2] = {0u, 0u};
    const long long tiles = FM_TILES(a.N);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        FM_TILE(tile, a.N, r0, rows); // const long long r0, const int rows: the tile's first row and its valid prefix
        for (int i = threadIdx.x; i < FM_FT * (H / 4); i += 256) {
            const int r = i / (H / 4), c = (i - r * (H / 4)) * 4;
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) {
                h = *reinterpret_cast<const float4 *>(a.h + (size_t)(r0 + r) * H + c);
                om[0] = fm_umax(fm_umax(fm_umax(om[0], fm_absbits(h.x)), fm_umax(fm_absbits(h.y), fm_absbits(h.z))), fm_absbits(h.w));
                FM_HIST_ADD(0, h.x);
                FM_HIST_ADD(0, h.y);
                FM_HIST_ADD(0, h.z);
                FM_HIST_ADD(0, h.w);
                FM_FQ_V4(0, h);
            }
            *reinterpret_cast<float4 *>(sh + r * LDA + c) = h;
        }
        __syncthreads();
        fm_f32x4 acc[2][NT];
        fm_mma<KS, NT>(acc, sh, LDA, breg, FM_DEC_TILES);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int t = wave + FM_WAVES * nt;
                if (t >= FM_DEC_TILES) continue;
                const int col = t * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rt * 16 + (lane >> 4) * 4 + r;
                    if (row >= rows || col >= FM_DIN) continue;
                    const float v = __fadd_rn(acc[rt][nt][r], bias[nt]);
                    om[1] = fm_umax(om[1], fm_absbits(v));
                    FM_HIST_ADD(1, v);
                    a.out[(size_t)(r0 + row) * FM_DIN + col] = FM_FQ(1, v);
                }
            }
        __syncthreads();
    }
    fm_obs_flush<2>(om, sobs, a.stats);
    FM_HIST_END(2);
}

#undef FM_HIST
#undef FM_CLIPS
#undef FM_FAKEQ
#undef FM_KERNEL
#undef FM_CLIPS_PARAM
#undef FM_TILES
#undef FM_TILE
#undef FM_GATE_ATTR
#undef FM_HIST_PARAM
#undef FM_HIST_BEGIN
#undef FM_HIST_ADD
#undef FM_HIST_END
#undef FM_FQ_PARAM
#undef FM_FQ
#undef FM_FQ2
#undef FM_FQ_V4
#undef FM_FQ_V2
