// s5fxp_step_body.inc -- the body of the one-launch step kernel, included by s5fxp_step.hpp once per kernel:
//   STEP_RAGGED 0  k_model_step(StepArgs a): every group has B x L rows, group g owns carry g and rows g * R ..
//   STEP_RAGGED 1  k_model_step_ragged(StepRaggedArgs a): entry e = blockIdx.x reads its row count L and its carry's slot from
//                  a.desc[e]; x and y are padded to Lmax frames per sequence, so row b * L + t of the group is frame t of
//                  sequence b there.  Only the input staging and the decoder's stores see that; the LDS regions are laid out
//                  for the entry's own R = B * L.
// STEP_PINNED 1 (with either STEP_RAGGED) is the form of the _at entries, k_model_step_at(StepPinArgs) and
// k_model_step_ragged_at(StepRaggedPinArgs): the five compute_best exponents of a layer are kernel arguments, so the maxima
// loops and their workgroup reductions are not compiled -- step_bn_pinned for step_bn_exps, and the residual block takes its
// shifts from the stated exponent.  Every other statement is shared.
// The two share every line that computes, so they cannot drift.  The clip kernel (s5fxp_clip.hpp) holds a copy of these
// stages over tiles, except step_bn_exps (s5fxp_step.hpp), which both call: a change to any other stage is made in both.
    constexpr int STEP_WAVES = STEP_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) int8_t step_smem[];
    __shared__ int32_t s_status[128]; // S5FXP_STATUS_WORDS: built here, stored once at the end
#if !STEP_PINNED
    __shared__ float s_red[3][STEP_MAX_WAVES];
#endif
    // the layer's per-channel and per-state operands, fetched together at the head of the layer
    __shared__ LayerDyn s_d;
    __shared__ int32_t s_lut[8];
    __shared__ int32_t s_wide;

    const StepParams &sp = *a.sp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t g = blockIdx.x;
#if STEP_RAGGED
    const s5fxp_push_desc *pd = as_global(a.desc) + g;
    const int64_t slot = pd->slot;
    const int L = pd->rows, Lmax = a.Lmax;
    const bool fresh = (pd->flags & S5FXP_PUSH_FRESH) != 0;
    const int B = a.B, R = B * L, H = sp.H, P = sp.P, HP = sp.hp, nl = sp.n_layers;
#else
    const int B = a.B, L = a.L, R = B * L, H = sp.H, P = sp.P, HP = sp.hp, nl = sp.n_layers;
#endif
    const int arow = r < R ? r : R - 1; // padding rows of the MFMA tile re-read the last real row
    const StepLds lds = step_lds(R, H, P, HP, sp.d_in);
    int8_t *pla = step_smem + lds.pla, *plb = step_smem + lds.plb;
    int16_t *hb = reinterpret_cast<int16_t *>(step_smem + lds.hb), *x1b = reinterpret_cast<int16_t *>(step_smem + lds.x1),
            *zb = reinterpret_cast<int16_t *>(step_smem + lds.z);
    int32_t *bq = reinterpret_cast<int32_t *>(step_smem + lds.bq); // [re | im][row][state]
    const int KPB = lds.kpb, psb = R * KPB;

    for (int i = tid; i < 128; i += STEP_THREADS) {
        int32_t v = 0;
        if (i == 1) v = sp.dec.out_exp;
        else if (i == 2) v = 3; // S5FXP_PATH_STEP
        else if (i >= 8 && (i - 8) / 8 < nl) v = (i & 7) == 5 ? 6 : ((i & 7) >= 6 ? P : 0);
        s_status[i] = v;
    }
    __syncthreads();
#if STEP_RAGGED
    // no frame: the carry after zero frames is the carry in (zeros for a fresh stream); the status words keep their fill
    if (R == 0) {
        if (fresh) {
            int32_t *cz = as_global(a.state) + slot * nl * 2 * B * P;
            for (int i = tid; i < nl * 2 * B * P; i += STEP_THREADS) cz[i] = 0;
        }
        int32_t *st0 = as_global(a.status) + g * 128;
        for (int i = tid; i < 128; i += STEP_THREADS) st0[i] = s_status[i];
        return;
    }
#endif

    // ---- input rows -> byte planes (float rows: fxp_from_fp FLOOR first), with the encoder's input conversion
    // (fxpmodel.py:335-347) and the 16-bit check of the fused encoder (proj_p.hpp k_enc_p)
    {
        const StepDense &e = sp.enc;
        const int K = e.K, KPA = lds.kpa_enc, psa = R * KPA;
        const bool conv = a.x_bits > e.inp_bits || a.x_exp > e.inp_exp;
        const float sc = ldexpf(1.f, a.x_exp);
#if STEP_RAGGED
        const int32_t *xg = as_global(reinterpret_cast<const int32_t *>(a.x)) + g * B * Lmax * K;
#else
        const int32_t *xg = as_global(reinterpret_cast<const int32_t *>(a.x)) + g * R * K;
#endif
        bool wide = false;
        for (int i = tid; i < R * K; i += STEP_THREADS) {
            const int row = i / K, k = i - row * K;
#if STEP_RAGGED
            const int sb = row / L;
            int32_t v = xg[(sb * Lmax + (row - sb * L)) * K + k];
#else
            int32_t v = xg[i];
#endif
            if (a.f32) v = fromfp(__int_as_float(v), sc, a.x_bits);
            if (conv) v = chcfg(v, a.x_bits, a.x_exp, e.inp_bits, e.inp_exp);
            wide |= v != (int32_t)(int16_t)v;
            step_put2(pla, psa, row * KPA + k, v);
        }
        if (__any(wide) && lane == 0) atomicOr(&s_status[0], ST_WIDE_INPUT);
        __syncthreads();
#if STEP_RAGGED
        // the carry is updated in place: an entry whose input the 16-bit planes cannot hold leaves y and its slot alone, so
        // the caller can serve it from the intact carry on the generic engine (workgroup-uniform: read behind the barrier)
        if (s_status[0] & ST_WIDE_INPUT) {
            int32_t *st0 = as_global(a.status) + g * 128;
            for (int i = tid; i < 128; i += STEP_THREADS) st0[i] = s_status[i];
            return;
        }
#endif
        // ---- encoder + bias + ReLU (fxpmodel.py:331-366, 1263-1266)
        const int rs = (conv ? e.inp_exp : a.x_exp) + e.w_exp - e.out_exp; // checked by the host
        const int nks = (K + 31) / 32;
        for (int tile = wave; tile < HP / 32; tile += STEP_WAVES) {
            const int col = 32 * tile + r;
            const v16i acc = step_mm<2>(pla, psa, KPA, arow, h, e.w, col, nks);
            const int32_t be = as_global(e.bias_eff)[col];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
                if (row < R && col < H) { // (a wave whose lanes all hold padding rows skips the element)
                    int32_t v = sat(asr(acc[i], rs), e.out_bits);
                    v = sat(wadd(v, be), e.out_bits);
                    hb[row * H + col] = (int16_t)(v < 0 ? 0 : v);
                }
            }
        }
        __syncthreads();
    }

    int hbits = sp.enc.out_bits, he = sp.enc.out_exp; // the layer input's configuration (he: chosen on the device from layer 1 on)
    for (int li = 0; li < nl; ++li) {
        const StepLayer &sl = sp.layers[li];
        BnArgs bn = sl.bn;
        bn.xe.stat = he; bn.xe.dyn = nullptr; bn.dyn = nullptr;
        int32_t *st_exps = s_status + 8 + 8 * li;
        if (tid < 8) s_lut[tid] = sl.lut[tid];
        if (tid == 0) s_wide = 0;

#if STEP_PINNED
        // ---- the four BatchNorm exponents as stated: the shifts finalize_*_cb would derive, no reduction
        step_bn_pinned(pin.e + 5 * li, bn, he, s_d, st_exps);
#else
        // ---- the four BatchNorm compute_best exponents over the R x H values of h: the stage the clip kernel shares
        step_bn_exps<STEP_THREADS>(hb, R * H, H, bn, he, s_d, s_status, st_exps, s_red);
#endif
        const LayerDyn d = s_d;

        // ---- u = change_cfg(BatchNorm(x)) -> byte planes (fxpmodel.py:620-624)
        for (int i = tid; i < R * H; i += STEP_THREADS) {
            const int row = i / H, c = i - row * H;
            step_put2(plb, psb, row * KPB + c, bn_chain<5>(bn, d, hb[i], c));
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
                    bq[(c * R + row) * P + p] = sh > 0 ? asr(bu, sh) : wshl(bu, -sh);
                }
            }
        }
        __syncthreads();

        // ---- the recurrence from the carry, 32-bit wrap arithmetic (fxpmodel.py:147-172); carry out; complex ReLU
        // (fxpmodel.py:740-742).  A thread owns one (sequence, state): it reads its carry before it writes it, so
        // state_out may be state_in.  The states replace Bu in place.
        {
            const size_t plane = (size_t)B * P;
#if STEP_RAGGED
            const size_t cbase = ((size_t)slot * nl + li) * 2 * plane;
#else
            const size_t cbase = ((size_t)g * nl + li) * 2 * plane;
#endif
            bool wide = false;
            for (int i = tid; i < B * P; i += STEP_THREADS) {
                const int b = i / P, p = i - b * P;
                const int32_t Ar = as_global(sl.a_re)[p], Ai = as_global(sl.a_im)[p];
#if STEP_RAGGED
                int32_t xr = fresh ? 0 : as_global(a.state)[cbase + i];
                int32_t xi = fresh ? 0 : as_global(a.state)[cbase + plane + i];
#else
                int32_t xr = a.state_in ? as_global(a.state_in)[cbase + i] : 0;
                int32_t xi = a.state_in ? as_global(a.state_in)[cbase + plane + i] : 0;
#endif
                for (int t = 0; t < L; ++t) {
                    const int o = (b * L + t) * P + p;
                    scan_step(Ar, Ai, sl.ea_re, sl.ea_im, bq[o], bq[R * P + o], xr, xi);
                    int32_t sr = xr, si = xi;
                    crelu(sr, si);
                    wide |= sr != (int32_t)(int16_t)sr || si != (int32_t)(int16_t)si;
                    bq[o] = sr;
                    bq[R * P + o] = si;
                }
#if STEP_RAGGED
                as_global(a.state)[cbase + i] = xr;
                as_global(a.state)[cbase + plane + i] = xi;
#else
                if (a.state_out) {
                    as_global(a.state_out)[cbase + i] = xr;
                    as_global(a.state_out)[cbase + plane + i] = xi;
                }
#endif
            }
            if (__any(wide) && lane == 0) atomicOr(&s_wide, 1);
        }
        __syncthreads();
        const bool wide_states = s_wide != 0; // workgroup-uniform
        const int KPS = lds.kpa_st, pss = R * KPS, npl = wide_states ? 4 : 2;
        for (int i = tid; i < 2 * R * P; i += STEP_THREADS) {
            const int c = i / (R * P), rem = i - c * R * P, row = rem / P, p = rem - row * P;
            int8_t *base = pla + c * npl * pss;
            if (wide_states) step_put4(base, pss, row * KPS + p, bq[i]);
            else step_put2(base, pss, row * KPS + p, bq[i]);
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
                    x1b[row * H + col] = (int16_t)x1;
                    step_put2(plb, psb, row * KPB + col,
                              sl.o2_conv ? chcfg(x1, sl.y_bits, sl.y_exp, sl.o2_inp_bits, sl.o2_inp_exp) : x1);
                }
            }
        }
        __syncthreads();

        // ---- out2 + LUT sigmoid + gate (fxpmodel.py:1133-1137, 97-144, 1075-1093) + the residual add's maxima
        {
#if !STEP_PINNED
            float v[3] = {0.f, 0.f, 0.f};
#endif
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
                        zb[row * H + col] = (int16_t)z;
#if !STEP_PINNED
                        const float fz = tofloat(z, sl.res_exp), fs = tofloat(hb[row * H + col], he);
                        v[0] = fmaxf(v[0], fabsf(__fadd_rn(fz, fs)));
                        v[1] = fmaxf(v[1], fabsf(fz));
                        v[2] = fmaxf(v[2], fabsf(fs));
#endif
                    }
                }
            }
#if STEP_PINNED
            if (tid == 0) {
                s_d.res = pinned_add_cb(pin.e[5 * li + 4], sl.res_exp, he);
                st_exps[4] = s_d.res.eo;
            }
#else
            step_wg_max<3, STEP_WAVES>(v, s_red);
            if (tid == 0) {
                const uint32_t m3[3] = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
                s_d.res = finalize_add_cb(m3, sl.res_exp, he, sl.res_bits, s_status);
                st_exps[4] = s_d.res.eo;
            }
#endif
            __syncthreads();
        }
        // ---- residual compute_best add + ReLU (fxpmodel.py:1147-1159): the next layer's input, in place
        {
            const AddCb rp = s_d.res;
            for (int i = tid; i < R * H; i += STEP_THREADS) {
                const int32_t rr = add_cb_apply(zb[i], sl.res_bits, hb[i], hbits, rp, sl.res_bits);
                hb[i] = (int16_t)(rr < 0 ? 0 : rr);
            }
            hbits = sl.res_bits;
            he = rp.eo;
        }
        __syncthreads();
    }

    // ---- decoder (fxpmodel.py:1437, 331-366): its input exponent is the last residual's
    {
        const StepDense &e = sp.dec;
        const bool conv = hbits > e.inp_bits || he > e.inp_exp;
        int rs = (conv ? e.inp_exp : he) + e.w_exp - e.out_exp;
        if (rs < 0 || rs > 31) {
            if (tid == 0) atomicOr(&s_status[0], ST_NEGSHIFT);
            rs = rs < 0 ? 0 : 31;
        }
        for (int i = tid; i < R * H; i += STEP_THREADS) {
            const int row = i / H, c = i - row * H;
            const int32_t v = hb[i];
            step_put2(plb, psb, row * KPB + c, conv ? chcfg(v, hbits, he, e.inp_bits, e.inp_exp) : v);
        }
        __syncthreads();
        const int M = e.M;
#if STEP_RAGGED
        int32_t *yg = as_global(reinterpret_cast<int32_t *>(a.y)) + g * B * Lmax * M;
#else
        int32_t *yg = as_global(reinterpret_cast<int32_t *>(a.y)) + g * R * M;
#endif
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
#if STEP_RAGGED
                    const int sb = row / L;
                    yg[(sb * Lmax + (row - sb * L)) * M + col] = a.f32 ? __float_as_int(tofloat(v, e.out_exp)) : v;
#else
                    yg[row * M + col] = a.f32 ? __float_as_int(tofloat(v, e.out_exp)) : v;
#endif
                }
            }
        }
    }
    __syncthreads();
    int32_t *stg = as_global(a.status) + g * 128;
    for (int i = tid; i < 128; i += STEP_THREADS) stg[i] = s_status[i];
