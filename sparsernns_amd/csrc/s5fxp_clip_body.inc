// s5fxp_clip_body.inc -- the clip kernel's text, written once.  s5fxp_clip.hpp includes it twice (no include guard), inside
// namespace s5, and states before each inclusion the one flag that tells the forms apart:
//   CLIP_TRACE 0  k_model_clips<STEP_THREADS>(ClipArgs)
//   CLIP_TRACE 1  k_model_clips_traced<STEP_THREADS>(ClipTraceArgs): the stages also store the values they hold to the
//                 layer's trace planes (the statements between #if CLIP_TRACE and #endif)
// and, with CLIP_TRACE 0, optionally a second one:
//   CLIP_PINNED 1 k_model_clips_at<STEP_THREADS>(ClipPinArgs): the form of s5fxp_model_clips_at -- the five compute_best
//                 exponents of a layer are kernel arguments, so the maxima loops and their workgroup reductions are not
//                 compiled (the statements behind #if CLIP_PINNED / #if !CLIP_PINNED)
// Both flags are undefined at the foot.  What the text does and how it is kept in step with s5fxp_step_body.inc: s5fxp_clip.hpp.
#ifndef CLIP_TRACE
#error "s5fxp_clip_body.inc: define CLIP_TRACE (0/1)"
#endif
#ifndef CLIP_PINNED
#define CLIP_PINNED 0
#endif
#if CLIP_PINNED && CLIP_TRACE
#error "s5fxp_clip_body.inc: the pinned form has no trace planes"
#endif

template <int STEP_THREADS>
#if CLIP_PINNED
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_clips_at(ClipPinArgs pa)
{
    const ClipArgs &a = pa.c;
    const PinExps &pin = pa.pin;
#elif CLIP_TRACE
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_clips_traced(ClipTraceArgs ta)
{
    const ClipArgs &a = ta.c;
#else
__global__ __launch_bounds__(STEP_THREADS, 2) void k_model_clips(ClipArgs a)
{
#endif
    constexpr int STEP_WAVES = STEP_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) int8_t step_smem[];
    __shared__ int32_t s_status[128]; // S5FXP_STATUS_WORDS: built here, stored once at the end
#if !CLIP_PINNED
    __shared__ float s_red[3][STEP_MAX_WAVES];
#endif
    __shared__ LayerDyn s_d;
    __shared__ int32_t s_lut[8];
    __shared__ int32_t s_wide;

    const StepParams &sp = *a.sp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t g = blockIdx.x;
    const int Lmax = a.Lmax, H = sp.H, P = sp.P, HP = sp.hp, nl = sp.n_layers;
    int len = as_global(a.lens)[g];
    len = len < 0 ? 0 : (len > Lmax ? Lmax : len);
    const int R32 = Lmax < STEP_MAX_ROWS ? Lmax : STEP_MAX_ROWS;
    const StepLds lds = step_lds(R32, H, P, HP, sp.d_in);
    int8_t *pla = step_smem + lds.pla, *plb = step_smem + lds.plb;
    int16_t *hb = reinterpret_cast<int16_t *>(step_smem + lds.hb), *x1b = reinterpret_cast<int16_t *>(step_smem + lds.x1);
    int32_t *bq = reinterpret_cast<int32_t *>(step_smem + lds.bq); // [re | im][row][state]
    const int KPB = lds.kpb, psb = R32 * KPB;
    int16_t *hg = as_global(a.scratch) + g * 2 * Lmax * H, *zg = hg + (int64_t)Lmax * H; // this workgroup's planes
    int32_t *stg = as_global(a.status) + g * 128;
    const int LH = len * H;

    for (int i = tid; i < 128; i += STEP_THREADS) {
        int32_t v = 0;
        if (i == 1) v = sp.dec.out_exp;
        else if (i == 2) v = 4; // S5FXP_PATH_CLIP
        else if (i >= 8 && (i - 8) / 8 < nl) v = (i & 7) == 5 ? 6 : ((i & 7) >= 6 ? P : 0);
        s_status[i] = v;
    }
    __syncthreads();
    // no frame: the carry after zero frames is the carry in; the status words keep their fill
    if (len == 0) {
        if (a.state_out && a.state_out != a.state_in) {
            int32_t *co = as_global(a.state_out) + g * nl * 2 * P;
            for (int i = tid; i < nl * 2 * P; i += STEP_THREADS) co[i] = a.state_in ? as_global(a.state_in)[g * nl * 2 * P + i] : 0;
        }
        for (int i = tid; i < 128; i += STEP_THREADS) stg[i] = s_status[i];
        return;
    }

    // ---- input rows -> byte planes (float rows: fxp_from_fp FLOOR first), the encoder's input conversion, the 16-bit check,
    // encoder + bias + ReLU (fxpmodel.py:331-366, 1263-1266) -> h rows in the scratch, tile after tile
    {
        const StepDense &e = sp.enc;
        const int K = e.K, KPA = lds.kpa_enc, psa = R32 * KPA;
        const bool conv = a.x_bits > e.inp_bits || a.x_exp > e.inp_exp;
        const float sc = ldexpf(1.f, a.x_exp);
        const int32_t *xg = as_global(reinterpret_cast<const int32_t *>(a.x)) + g * Lmax * K;
        const int rs = (conv ? e.inp_exp : a.x_exp) + e.w_exp - e.out_exp; // checked by the host
        const int nks = (K + 31) / 32;
        for (int t0 = 0; t0 < len; t0 += STEP_MAX_ROWS) {
            const int R = len - t0 < STEP_MAX_ROWS ? len - t0 : STEP_MAX_ROWS, arow = r < R ? r : R - 1;
            bool wide = false;
            for (int i = tid; i < R * K; i += STEP_THREADS) {
                const int row = i / K, k = i - row * K;
                int32_t v = xg[t0 * K + i];
                if (a.f32) v = fromfp(__int_as_float(v), sc, a.x_bits);
                if (conv) v = chcfg(v, a.x_bits, a.x_exp, e.inp_bits, e.inp_exp);
                wide |= v != (int32_t)(int16_t)v;
                step_put2(pla, psa, row * KPA + k, v);
            }
            if (__any(wide) && lane == 0) atomicOr(&s_status[0], ST_WIDE_INPUT);
            __syncthreads();
            // a clip whose input the 16-bit planes cannot hold leaves y and its carry alone, so the caller can serve it on the
            // generic engine (workgroup-uniform: read behind the barrier; no layer has run yet)
            if (s_status[0] & ST_WIDE_INPUT) {
                for (int i = tid; i < 128; i += STEP_THREADS) stg[i] = s_status[i];
                return;
            }
            for (int tile = wave; tile < HP / 32; tile += STEP_WAVES) {
                const int col = 32 * tile + r;
                const v16i acc = step_mm<2>(pla, psa, KPA, arow, h, e.w, col, nks);
                const int32_t be = as_global(e.bias_eff)[col];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (row < R && col < H) {
                        int32_t v = sat(asr(acc[i], rs), e.out_bits);
                        v = sat(wadd(v, be), e.out_bits);
                        hg[(t0 + row) * H + col] = (int16_t)(v < 0 ? 0 : v);
                    }
                }
            }
            __syncthreads(); // the planes are free for the next tile; after the last tile: h is complete
        }
    }

    int hbits = sp.enc.out_bits, he = sp.enc.out_exp; // the layer input's configuration (he: chosen on the device from layer 1 on)
    for (int li = 0; li < nl; ++li) {
        const StepLayer &sl = sp.layers[li];
        BnArgs bn = sl.bn;
        bn.xe.stat = he; bn.xe.dyn = nullptr; bn.dyn = nullptr;
        int32_t *st_exps = s_status + 8 + 8 * li;
        if (tid < 8) s_lut[tid] = sl.lut[tid];
#if CLIP_TRACE
        const s5fxp_layer_trace tr = ta.tr[li]; // this layer's planes, and the clip's first row in them
        const int64_t trow = g * Lmax;
#endif

#if CLIP_PINNED
        // ---- the four BatchNorm exponents as stated (s5fxp_step.hpp step_bn_pinned): no pass over h
        step_bn_pinned(pin.e + 5 * li, bn, he, s_d, st_exps);
#else
        // ---- the four BatchNorm compute_best exponents over the len x H values of h, re-read from the scratch: the step
        // kernel's function (s5fxp_step.hpp step_bn_exps)
        step_bn_exps<STEP_THREADS>(hg, LH, H, bn, he, s_d, s_status, st_exps, s_red);
#endif
        const LayerDyn d = s_d;

        // ---- the tiles: u -> B projection -> recurrence -> C projection -> out2 -> gate -> z rows in the scratch.
        // Thread p < P owns state p: it reads its carry before tile 0 and keeps it in registers until it writes it behind
        // the last tile, so state_out may be state_in.
        const int64_t cbase = (g * nl + li) * 2 * P;
        int32_t xr = 0, xi = 0;
        if (tid < P && a.state_in) {
            xr = as_global(a.state_in)[cbase + tid];
            xi = as_global(a.state_in)[cbase + P + tid];
        }
#if !CLIP_PINNED
        float rv3[3] = {0.f, 0.f, 0.f}; // the residual add's maxima, over all tiles
#endif
        for (int t0 = 0; t0 < len; t0 += STEP_MAX_ROWS) {
            const int R = len - t0 < STEP_MAX_ROWS ? len - t0 : STEP_MAX_ROWS, arow = r < R ? r : R - 1;
            if (tid == 0) s_wide = 0;
            // ---- the tile's h rows -> LDS, u = change_cfg(BatchNorm(h)) -> byte planes (fxpmodel.py:620-624)
            for (int i = tid; i < R * H; i += STEP_THREADS) {
                const int row = i / H, c = i - row * H;
                const int16_t hv = hg[t0 * H + i];
                hb[i] = hv;
                step_put2(plb, psb, row * KPB + c, bn_chain<5>(bn, d, hv, c));
#if CLIP_TRACE
                {
                    const int64_t o = (trow + t0) * H + i;
                    if (tr.pre_s5) as_global(tr.pre_s5)[o] = bn_chain<4>(bn, d, hv, c);
                    if (tr.u) as_global(tr.u)[o] = bn_chain<5>(bn, d, hv, c);
                }
#endif
            }
            __syncthreads();

            // ---- B projection, Bu saturate and the shift to the state exponent (fxpmodel.py:626-644, 158-167)
            for (int tile = wave; tile < 2 * P / 32; tile += STEP_WAVES) {
                const int col = 32 * tile + r, c = col >= P ? 1 : 0, p = col - c * P;
                const v16i acc = step_mm<2>(plb, psb, KPB, arow, h, sl.bproj, col, HP / 32);
                const int rs = c ? sl.rs_bim : sl.rs_bre, bits = c ? sl.bim_bits : sl.bre_bits, sh = c ? sl.sh_im : sl.sh_re;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (row < R) {
                        const int32_t bu = sat(asr(acc[i], rs), bits);
                        bq[(c * R32 + row) * P + p] = sh > 0 ? asr(bu, sh) : wshl(bu, -sh);
#if CLIP_TRACE
                        {
                            int32_t *const pl = c ? tr.Bu_im : tr.Bu_re;
                            if (pl) as_global(pl)[(trow + t0 + row) * P + p] = bu;
                        }
#endif
                    }
                }
            }
            __syncthreads();

            // ---- the recurrence, 32-bit wrap arithmetic (fxpmodel.py:147-172); complex ReLU (fxpmodel.py:740-742).  The
            // states replace Bu in place.
            {
                bool wide = false;
                if (tid < P) {
                    const int32_t Ar = as_global(sl.a_re)[tid], Ai = as_global(sl.a_im)[tid];
                    for (int t = 0; t < R; ++t) {
                        const int o = t * P + tid;
                        scan_step(Ar, Ai, sl.ea_re, sl.ea_im, bq[o], bq[R32 * P + o], xr, xi);
#if CLIP_TRACE // the raw states, before the complex ReLU
                        if (tr.xs_re) as_global(tr.xs_re)[(trow + t0 + t) * P + tid] = xr;
                        if (tr.xs_im) as_global(tr.xs_im)[(trow + t0 + t) * P + tid] = xi;
#endif
                        int32_t sr = xr, si = xi;
                        crelu(sr, si);
                        wide |= sr != (int32_t)(int16_t)sr || si != (int32_t)(int16_t)si;
                        bq[o] = sr;
                        bq[R32 * P + o] = si;
                    }
                }
                if (__any(wide) && lane == 0) atomicOr(&s_wide, 1);
            }
            __syncthreads();
            const bool wide_states = s_wide != 0; // workgroup-uniform, this tile's
            const int KPS = lds.kpa_st, pss = R32 * KPS, npl = wide_states ? 4 : 2;
            for (int i = tid; i < 2 * R * P; i += STEP_THREADS) {
                const int c = i / (R * P), rem = i - c * R * P, row = rem / P, p = rem - row * P;
                int8_t *base = pla + c * npl * pss;
                const int32_t sv = bq[(c * R32 + row) * P + p];
                if (wide_states) step_put4(base, pss, row * KPS + p, sv);
                else step_put2(base, pss, row * KPS + p, sv);
            }
            if (wide_states && tid == 0) atomicOr(&s_status[0], ST_WIDE_STATE);
            __syncthreads();

            // ---- C projection + D u + ReLU (fxpmodel.py:746-793, 1125) -> x1 and out2's input planes
            for (int tile = wave; tile < HP / 32; tile += STEP_WAVES) {
                const int col = 32 * tile + r;
                v16i are, aim;
                if (wide_states) {
                    are = step_mm<4>(pla, pss, KPS, arow, h, sl.cre, col, P / 32);
                    aim = step_mm<4>(pla + 4 * pss, pss, KPS, arow, h, sl.cim, col, P / 32);
                } else {
                    are = step_mm<2>(pla, pss, KPS, arow, h, sl.cre, col, P / 32);
                    aim = step_mm<2>(pla + 2 * pss, pss, KPS, arow, h, sl.cim, col, P / 32);
                }
                const int32_t Dv = as_global(sl.Dpad)[col];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (row < R && col < H) {
                        const int32_t cr = sat(asr(are[i], sl.rs_cre), sl.y_bits);
                        const int32_t ci = sat(asr(aim[i], sl.rs_cim), sl.y_bits);
                        const int32_t cx = sat(wadd(cr, wmul(ci, -1)), sl.y_bits);
                        const int32_t cx2 = wmul(cx, 2); // not clipped, fxpmodel.py:765-767
                        const int32_t u = bn_chain<5>(bn, d, hb[row * H + col], col);
                        const int32_t du = sat(asr(wmul(Dv, u), sl.rs_d), sl.y_bits);
                        const int32_t yv = sat(wadd(cx2, du), sl.y_bits);
                        const int32_t x1 = yv < 0 ? 0 : yv;
#if CLIP_TRACE
                        if (tr.ys) as_global(tr.ys)[(trow + t0 + row) * H + col] = yv;
#endif
                        x1b[row * H + col] = (int16_t)x1;
                        step_put2(plb, psb, row * KPB + col,
                                  sl.o2_conv ? chcfg(x1, sl.y_bits, sl.y_exp, sl.o2_inp_bits, sl.o2_inp_exp) : x1);
                    }
                }
            }
            __syncthreads();

            // ---- out2 + LUT sigmoid + gate (fxpmodel.py:1133-1137, 97-144, 1075-1093) -> z rows; the residual add's maxima
            for (int tile = wave; tile < HP / 32; tile += STEP_WAVES) {
                const int col = 32 * tile + r;
                const v16i acc = step_mm<2>(plb, psb, KPB, arow, h, sl.out2, col, HP / 32);
                const int32_t be = as_global(sl.o2_bias_eff)[col];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (row < R && col < H) {
                        int32_t gq = sat(asr(acc[i], sl.rs_o2), sl.o2_out_bits);
                        gq = sat(wadd(gq, be), sl.o2_out_bits);
                        const int32_t s = sigmoid_lut(gq, sl.o2_out_bits, sl.o2_out_exp, sl.sig_x, sl.sig_y, s_lut);
                        const int32_t lv = chcfg(x1b[row * H + col], sl.y_bits, sl.y_exp, sl.l_bits, sl.l_exp);
                        const int32_t rv = chcfg(s, sl.o2_out_bits, sl.sig_y, sl.r_bits, sl.r_exp);
                        const int32_t z = sat(asr(wmul(lv, rv), sl.rs_gate), sl.res_bits);
                        zg[(t0 + row) * H + col] = (int16_t)z;
#if CLIP_TRACE
                        {
                            const int64_t o = (trow + t0 + row) * H + col;
                            if (tr.out2) as_global(tr.out2)[o] = gq;
                            if (tr.out2_sigmoid) as_global(tr.out2_sigmoid)[o] = s;
                            if (tr.post_GLU) as_global(tr.post_GLU)[o] = z;
                        }
#endif
#if !CLIP_PINNED
                        const float fz = tofloat(z, sl.res_exp), fs = tofloat(hb[row * H + col], he);
                        rv3[0] = fmaxf(rv3[0], fabsf(__fadd_rn(fz, fs)));
                        rv3[1] = fmaxf(rv3[1], fabsf(fz));
                        rv3[2] = fmaxf(rv3[2], fabsf(fs));
#endif
                    }
                }
            }
            __syncthreads(); // the tile's LDS is free for the next tile; after the last tile: z is complete
        }
        if (tid < P && a.state_out) {
            as_global(a.state_out)[cbase + tid] = xr;
            as_global(a.state_out)[cbase + P + tid] = xi;
        }
#if CLIP_PINNED
        if (tid == 0) {
            s_d.res = pinned_add_cb(pin.e[5 * li + 4], sl.res_exp, he);
            st_exps[4] = s_d.res.eo;
        }
#else
        step_wg_max<3, STEP_WAVES>(rv3, s_red);
        if (tid == 0) {
            const uint32_t m3[3] = {__float_as_uint(rv3[0]), __float_as_uint(rv3[1]), __float_as_uint(rv3[2])};
            s_d.res = finalize_add_cb(m3, sl.res_exp, he, sl.res_bits, s_status);
            st_exps[4] = s_d.res.eo;
        }
#endif
        __syncthreads();
        // ---- residual compute_best add + ReLU (fxpmodel.py:1147-1159) over all rows: the next layer's input, in place
        {
            const AddCb rp = s_d.res;
            for (int i = tid; i < LH; i += STEP_THREADS) {
                const int32_t rr = add_cb_apply(zg[i], sl.res_bits, hg[i], hbits, rp, sl.res_bits);
#if CLIP_TRACE
                if (tr.residadd) as_global(tr.residadd)[trow * H + i] = rr; // before the ReLU
#endif
                hg[i] = (int16_t)(rr < 0 ? 0 : rr);
            }
            hbits = sl.res_bits;
            he = rp.eo;
        }
        __syncthreads();
    }

    // ---- decoder (fxpmodel.py:1437, 331-366), tile after tile: its input exponent is the last residual's
    {
        const StepDense &e = sp.dec;
        const bool conv = hbits > e.inp_bits || he > e.inp_exp;
        int rs = (conv ? e.inp_exp : he) + e.w_exp - e.out_exp;
        if (rs < 0 || rs > 31) {
            if (tid == 0) atomicOr(&s_status[0], ST_NEGSHIFT);
            rs = rs < 0 ? 0 : 31;
        }
        const int M = e.M;
        int32_t *yg = as_global(reinterpret_cast<int32_t *>(a.y)) + g * Lmax * M;
        for (int t0 = 0; t0 < len; t0 += STEP_MAX_ROWS) {
            const int R = len - t0 < STEP_MAX_ROWS ? len - t0 : STEP_MAX_ROWS, arow = r < R ? r : R - 1;
            for (int i = tid; i < R * H; i += STEP_THREADS) {
                const int row = i / H, c = i - row * H;
                const int32_t v = hg[t0 * H + i];
                step_put2(plb, psb, row * KPB + c, conv ? chcfg(v, hbits, he, e.inp_bits, e.inp_exp) : v);
            }
            __syncthreads();
            for (int tile = wave; tile < (M + 31) / 32; tile += STEP_WAVES) {
                const int col = 32 * tile + r;
                const v16i acc = step_mm<2>(plb, psb, KPB, arow, h, e.w, col, HP / 32);
                const int32_t be = as_global(e.bias_eff)[col];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (row < R && col < M) {
                        int32_t v = sat(asr(acc[i], rs), e.out_bits);
                        v = sat(wadd(v, be), e.out_bits);
                        yg[(t0 + row) * M + col] = a.f32 ? __float_as_int(tofloat(v, e.out_exp)) : v;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < 128; i += STEP_THREADS) stg[i] = s_status[i];
}
#undef CLIP_TRACE
#undef CLIP_PINNED
