// mfma_fused_body.inc -- the body of k_cgate_p (mfma_fused.hpp), included by its two overloads with FOLD = false / true.
    CGateArgs a = a_k; // (the LUT is indexed by thread below: that read stays on the kernel argument, so that this copy lives in registers)
    {
        const int64_t g = blockIdx.y;
        gshift(a.u, g * go.ws); gshift(a.skip, g * go.ws); gshift(a.xs, g * go.ws); gshift(a.z, g * go.ws);
        gshift(a.skip_e.dyn, g * go.ws); gshift(a.dynw, g * go.ws); gshift(a.run_if, g * go.ws); gshift(a.status, g * go.status);
        if constexpr (GBN || UREC) { gshift(a.bn.dyn, g * go.ws); gshift(a.bn.xe.dyn, g * go.ws); }
    }
    static_assert(!GBN || (PK16 && !TRACE && !WIDE), "the BatchNorm rides on the packed-epilogue kernel only");
    static_assert(!UREC || (PK16 && !TRACE && !WIDE && !GBN), "u is rebuilt in the row tiles' staging: COAL only");
    // H: the real channels (row stride in memory, vectors per frame); HP: the padded extent of the LDS tables, the X1 planes
    // and the row tiles (proj_p.hpp shape_channels).  RAGGED: channel groups of the last tile at or beyond H are pad lanes:
    // their weights, D and bias are zero, so they compute x1 = 0 and z = 0; their u and skip are zero instead of loaded (a zero
    // adds nothing to the residual maximum) and they store nothing.
    constexpr int P = 32 * KS, H = shape_channels(NT), HP = 32 * NT, FT = FTP, NW = (FT / 32) * NT, NTHR = 64 * NW; // one wave per (half, column tile)
    constexpr bool RAGGED = H != HP;
    constexpr int KPS = 2 * P + 16, KPX = HP + 16;
    constexpr int NU = 1, SUBSTEP = 0;   // units per wave
    constexpr int ITEMS = (FT / 4) * P, ROUNDS = (ITEMS + NTHR - 1) / NTHR;
    extern __shared__ __attribute__((aligned(16))) int8_t smem[];
    int32_t *csr = reinterpret_cast<int32_t *>(smem), *csi = csr + HP, *Dl = csi + HP, *cs2 = Dl + HP, *be = cs2 + HP, *lutp = be + HP;
    int32_t *sigt = lutp + 8; // SIGTAB_WORDS, or the direct table (int16, SIGDIR_BYTES)
    const int16_t *sigd = reinterpret_cast<const int16_t *>(sigt);
    constexpr int NPL = WIDE ? 4 : 2; // byte planes of the state operand; plane NPL-1 is the signed top byte
    // the direct table takes what it needs (2 bytes x 2^sigdir_bits, to a multiple of 16), not the 8 KB of its widest form
    int8_t *Sbase = reinterpret_cast<int8_t *>(sigt) + (DIRECT ? sigdir_lds_bytes(a.sigdir_bits) : 4 * SIGTAB_WORDS);
    int8_t *Sl = Sbase, *Sh = Sbase + (NPL - 1) * FT * KPS, *Xh = Sbase + NPL * FT * KPS, *Xl = Xh + FT * KPX;
    float *red = reinterpret_cast<float *>(Xl + FT * KPX);
    int32_t *bntab = reinterpret_cast<int32_t *>(red + 48); // GBN: 4 * H BatchNorm operands (bn16_setup)
    // COAL: u and skip come in, and z goes out, as whole rows -- 16 bytes per lane, a wave instruction covers 1 KB of
    // consecutive addresses -- through two LDS tiles [frame][TROW]; the epilogues, whose lanes are FRAMES (the accumulator
    // layout of the channel-major MFMA), pick their 8-byte (frame, four channels) pieces out of LDS.  In the accumulator's own
    // layout every global load / store instruction touched 64 different rows with 8 bytes each: the bytes per batch are the
    // same, the memory pipeline sees an eighth of the requests.  TROW: 8-byte reads by 32 lanes 200 bytes apart hit 32 bank pairs.
    constexpr bool COAL = PK16 && !TRACE && !WIDE && !GBN;
    // bytes per tile row; 16-byte vectors per frame / per thread (ragged shapes: the last round is predicated, NVC_FULL false)
    constexpr int TROW = 2 * HP + 8, VPF = H / 8, NVC = (FT * VPF + NTHR - 1) / NTHR;
    constexpr bool NVC_FULL = FT * VPF % NTHR == 0;
    static_assert(!COAL || NVC_FULL || RAGGED, "tile vectors per thread");
    static_assert(!UREC || NTHR % VPF == 0, "a thread's channel group must be the same for every vector");
    static_assert(!FOLD || (UREC && !RAGGED), "the aligned sum is formed in the UREC staging");
    int8_t *Ut = reinterpret_cast<int8_t *>(red + 48), *St = Ut + FT * TROW; // u (then z) and skip of the current tile
    const int l = threadIdx.x & 63, r = l & 31, h = l >> 5, wave = threadIdx.x >> 6;
    const int ct = wave % NT, sub0 = wave / NT;
    const StepRange sr{a.t_lo, a.t_len};
    const int64_t tiles = (a.N / a.L) * ((sr.t_len + FT - 1) / FT);
    if (WIDE && a.run_if && *a.run_if == 0) return;

    // weights of this wave's 32 channels (A operand rows), all k-steps, in registers
    v4i wre[KS], wim[KS], wo2[NT];
    {
        const size_t row = (size_t)(32 * ct + r);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            wre[ks] = *reinterpret_cast<const v4i *>(a.w_re.wt + row * a.w_re.Kp + 32 * ks + 16 * h);
            wim[ks] = *reinterpret_cast<const v4i *>(a.w_im.wt + row * a.w_im.Kp + 32 * ks + 16 * h);
        }
#pragma unroll
        for (int ks = 0; ks < NT; ++ks) wo2[ks] = *reinterpret_cast<const v4i *>(a.w_o2.wt + row * a.w_o2.Kp + 32 * ks + 16 * h);
    }
    for (int i = threadIdx.x; i < HP; i += NTHR) {
        csr[i] = a.w_re.cs128[i]; csi[i] = a.w_im.cs128[i]; Dl[i] = a.D[i]; cs2[i] = a.w_o2.cs128[i];
        if (!PK16) be[i] = a.bias_eff[i];
    }
    if (PK16) // packed pairs (every value fits 16 bits: host-checked)
        for (int i = threadIdx.x; i < HP / 2; i += NTHR)
            be[i] = (int32_t)(((uint32_t)a.bias_eff[2 * i] & 0xffffu) | ((uint32_t)a.bias_eff[2 * i + 1] << 16));
    if (threadIdx.x < 8) lutp[threadIdx.x] = a_k.lut[threadIdx.x] | (a_k.lut[threadIdx.x < 7 ? threadIdx.x + 1 : 7] << 16);
    if (DIRECT) {
        for (int i = threadIdx.x; i < (1 << a.sigdir_bits) / 2; i += NTHR)
            sigt[i] = reinterpret_cast<const int32_t *>(a.sigdir)[i];
    } else {
        for (int i = threadIdx.x; i < (14 << a.sig_x); i += NTHR) sigt[i] = a.sigtab[i];
    }
    Bn16 bn{};
    if constexpr (GBN) bn = bn16_setup(a.bn, *a.bn.dyn, bntab, H); // the B projection of this layer has published the exponents
    std::conditional_t<UREC, Bn16Row, int> brow{};
    if constexpr (UREC) brow = bn16_row_setup(a.bn, *a.bn.dyn, 8 * (int)(threadIdx.x % VPF)); // ... and so here
    // FOLD: the eight operand words of a channel group go behind the tiles, [group][m0..3, iv0..3], and every staging call reads
    // its group's back into short-lived registers: the eight registers they held for the whole kernel are the ones the running
    // extremes below (gate_ext) live in.  VPF x 32 bytes of LDS more; the five workgroups per CU stay (s5fxp_fast.hpp gate()).
    [[maybe_unused]] v4i *brow_lds = reinterpret_cast<v4i *>(St + FT * TROW);
    if constexpr (FOLD) {
        if (threadIdx.x < VPF) {
            brow_lds[2 * threadIdx.x] = v4i{(int)brow.m[0], (int)brow.m[1], (int)brow.m[2], (int)brow.m[3]};
            brow_lds[2 * threadIdx.x + 1] = v4i{(int)brow.iv[0], (int)brow.iv[1], (int)brow.iv[2], (int)brow.iv[3]};
        }
    }
    const int dsh = a.out_exp - a.sig_x, dbias = 1 << (a.sigdir_bits - 1);
    const int skip_e = a.skip_e.get();
    const float kz = ldexpf(1.f, skip_e - a.res_exp); // fz + fs = 2^-skip_e * (z * kz + s), exactly
    // FOLD: the multipliers that align the residual add's operands (mfma_bn.hpp SumU16), in four spare words of `red`: every
    // use reads them back into short-lived registers (the kernel has neither a scalar nor a vector register to pin them in)
    const v4i *usum_lds = reinterpret_cast<const v4i *>(red + 8);
    if constexpr (FOLD) {
        if (threadIdx.x == 0) {
            const SumU16 us = sum_u16_setup_exps(a.res_exp, skip_e);
            *reinterpret_cast<v4i *>(red + 8) = v4i{(int)us.mz, (int)us.mz2, (int)us.ms, (int)us.ms2};
            // resid_lazy: `skip` is the previous layer's U plane; the words that shift it into the layer input (mfma_bn.hpp
            // ResolveU16) sit beside the four above, [3] != 0 says that there is something to shift
            const LayerDyn *sd = skip_dyn_of(a_k);
            gshift(sd, (int64_t)blockIdx.y * go.ws);
            const ResolveU16 rz = resolve_u16_setup(sd ? sd->res.post : 0);
            *reinterpret_cast<v4i *>(red + 12) = v4i{(int)rz.shr, (int)rz.m1, (int)rz.m2, sd ? 1 : 0};
        }
    }
    // FOLD: a row vector of `skip` as the layer input h (a plain row unless the layer input is lazy)
    auto resolve_skip = [&](v4i &sv) {
        const v4i rw = *reinterpret_cast<const v4i *>(red + 12);
        if (__builtin_amdgcn_readfirstlane(rw[3])) {
            const ResolveU16 rz{(uint32_t)rw[0], (uint32_t)rw[1], (uint32_t)rw[2], RES_GENERIC};
#pragma unroll
            for (int q = 0; q < 4; ++q) sv[q] = (int)resolve_u16_pair<RES_GENERIC>(rz, (uint32_t)sv[q]);
        }
    };
    const int sx = a.sig_x, S = 1 << sx;
    // out2 input conversion (fxpmodel.py:335-347) as uniform shift/clip operands; identity when not needed
    const int cv_l = a.conv && a.inp_exp > a.y_exp ? a.inp_exp - a.y_exp : 0, cv_r = a.conv && a.y_exp > a.inp_exp ? a.y_exp - a.inp_exp : 0;
    const int cv_b1 = a.conv && a.inp_exp != a.y_exp ? a.y_bits : 32, cv_b2 = a.conv && a.y_bits > a.inp_bits ? a.inp_bits : 32;
    const int cv_b = cv_b1 < cv_b2 ? cv_b1 : cv_b2;
    // PK16: change_cfg(x1 -> l operand) with equal widths is a left shift that saturates or a right shift (fxp_prims.hpp chcfg)
    const int lq_l = a.l_exp > a.y_exp ? a.l_exp - a.y_exp : 0, lq_r = a.y_exp > a.l_exp ? a.y_exp - a.l_exp : 0;
    uint32_t xrange = 0;
    v2i16 pmax = {0, 0}, pmin = {0, 0}; // S16: running extremes of (re, im) as packed int16
    float mx[3] = {0.f, 0.f, 0.f}; // [0]: |z*kz + s| as converted integers, scaled once at the end; [1], [2] stay 0
    const int ch0 = 32 * ct + 4 * h;
    // u and skip of this wave's unit (32 frames x 32 channels), 8 bytes per lane and 8-channel group.  They are requested a
    // whole tile ahead and IN TURN: the next tile's u goes into the registers the first epilogue has just emptied, the next
    // tile's skip into those the second epilogue has emptied -- no extra registers, and the kernel has loads in flight during
    // its arithmetic phases instead of one burst at the top of every tile (32 KB per tile and workgroup outstanding for a third
    // of the tile's time is all that two workgroups per CU had in flight: ~3 TB/s by Little's law, which is what it ran at)
    v2i uq[NU][4], sq[NU][4];
    v4i urow[COAL && !UREC ? NVC : 1], srow[COAL ? NVC : 1]; // COAL: this thread's vectors of the NEXT tile's u and skip rows (UREC: skip only)
    auto load_tile = [&](v4i(&dst)[COAL ? NVC : 1], const int16_t *src, const TileWalk<FT> &tw) {
        const int64_t b = tw.b;
        const int t = tw.t(sr), nv = tw.nvalid(sr);
        const char *base = reinterpret_cast<const char *>(src + (b * a.L + t) * H); // wave-uniform
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int v = threadIdx.x + NTHR * i;
            if (!NVC_FULL && v >= FT * VPF) break; // (the last round of a ragged shape)
            int f = v / VPF;
            f = f < nv ? f : nv - 1;
            dst[i] = *reinterpret_cast<const v4i *>(base + 2u * (unsigned)(f * H + 8 * (v % VPF)));
        }
    };
    auto load_rows = [&](v2i(&dst)[NU][4], const int16_t *src, const TileWalk<FT> &tw) {
        const int64_t b = tw.b;
        const int t = tw.t(sr), nv = tw.nvalid(sr);
        const char *base = reinterpret_cast<const char *>(src + (b * a.L + t) * H); // wave-uniform
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            int fo = 32 * (sub0 + u * SUBSTEP) + r;
            fo = fo < nv ? fo : nv - 1;
            const unsigned fb = 2u * (unsigned)(fo * H + ch0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (RAGGED && ch0 + 8 * g >= H) dst[u][g] = v2i{0, 0}; // a pad lane
                else dst[u][g] = *reinterpret_cast<const v2i *>(base + fb + 16 * g);
            }
        }
    };
    // (the recurrence's states are requested at the top of the tile that uses them: requesting them a tile ahead as well
    // made the kernel slower, DESIGN.md 4a)
    if constexpr (COAL && RAGGED) { // the pad lanes' u and skip: zero once, no row vector ever lands there
        for (int i = threadIdx.x; i < 2 * FT; i += NTHR) {
            int8_t *t = Ut + i * TROW + 2 * H; // (rows of Ut, then of St; 8-byte aligned like every access to the tiles)
#pragma unroll
            for (int j = 0; j < (HP - H) / 4; ++j) *reinterpret_cast<v2i *>(t + 8 * j) = v2i{0, 0};
        }
    }
    // EARLY (the 32-frame UREC forms at KS = 1): phase A's items are mapped over the live state slots, and a tile's states are
    // requested at the top of the tile, in front of the staging, as loads the compiler cannot see (see the tile loop).
    //   The stream holds live_slots slots (0: all P); PL = live_slots up to a multiple of 4 (the quad transposes need whole
    // quads), ITEMS = (FT / 4) PL: one round of the workgroup for PL <= 24, otherwise a second round on wave 0.  A thread's
    // (group, slot) of round i never changes: half-word i of `items` holds group | slot << 3, or 0xffff for no item.  The
    // columns p >= PL of the Sl / Sh planes (re and im halves) are written here, once, with the bytes of a zero state: nothing
    // else touches the planes (the row tiles, which also park the extremes at the end, lie behind X1).
    // KS = 2 (three rounds, 142 registers) keeps the general form below.
    constexpr bool EARLY = UREC && S16 && KS == 1 && FT == 32;
    [[maybe_unused]] uint32_t items = 0;
    static_assert(!EARLY || (ROUNDS <= 2 && FT / 4 <= 8), "a half-word per round: three bits of group, the slot above them");
    [[maybe_unused]] auto item_of = [&](int i) { return (int)((items >> (16 * i)) & 0xffffu); };
    if constexpr (EARLY) {
        const int PL = a.live_slots > 0 ? (a.live_slots + 3) & ~3 : P;
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
            const int q = threadIdx.x + NTHR * i, grp = q / PL;
            items |= (uint32_t)(q < (FT / 4) * PL ? grp | ((q - grp * PL) << 3) : 0xffff) << (16 * i);
        }
        for (int i = threadIdx.x; i < FT * ((P - PL) >> 2); i += NTHR) {
            const int f = i / ((P - PL) >> 2), c = PL + 4 * (i % ((P - PL) >> 2));
            *reinterpret_cast<int32_t *>(Sl + f * KPS + c) = (int32_t)0x80808080u;
            *reinterpret_cast<int32_t *>(Sh + f * KPS + c) = 0;
            *reinterpret_cast<int32_t *>(Sl + f * KPS + P + c) = (int32_t)0x80808080u;
            *reinterpret_cast<int32_t *>(Sh + f * KPS + P + c) = 0;
        }
    }
    TileWalk<FT> walk((int64_t)blockIdx.x, sr, gridDim.x);
    if ((int64_t)blockIdx.x < tiles) {
        if constexpr (COAL) {
            if constexpr (!UREC) load_tile(urow, a.u, walk);
            load_tile(srow, a.skip, walk);
        } else {
            if constexpr (!GBN) load_rows(uq, a.u, walk);
            load_rows(sq, a.skip, walk);
        }
    }
    __syncthreads();
    char *zb_prev = nullptr; // COAL: where the z tile still sitting in LDS belongs (the previous tile of this workgroup)
    int nvalid_prev = 0;
    // FOLD: the two z vectors a thread is about to move out become U; the skip tile still holds the skip of the tile z belongs to
    auto fold_z = [&](v2i &z0, v2i &z1, const int8_t *cs_) {
        const v2i s0 = *reinterpret_cast<const v2i *>(cs_), s1 = *reinterpret_cast<const v2i *>(cs_ + 8);
        const v4i uw = *usum_lds;
        const SumU16 usum{(uint32_t)uw[0], (uint32_t)uw[1], (uint32_t)uw[2], (uint32_t)uw[3]};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            z0[q] = (int)sum_u16_pair(usum, (uint32_t)z0[q], (uint32_t)s0[q]);
            z1[q] = (int)sum_u16_pair(usum, (uint32_t)z1[q], (uint32_t)s1[q]);
        }
    };
    // FOLD (gate_ext, mfma_fused.hpp CGateFoldArgs::ext_next): running extremes of the U this thread stores, as packed uint16
    // pairs of its eight channels.  Only what is stored counts: a frame beyond nvalid_prev holds values of padded steps.
    // (Every fold kernel keeps them, also the one whose ext_next is null -- the last layer, the engines that read the plane: a
    // uniform branch around the eight packed instructions per vector would pin the pointer or a flag in the scalar registers the
    // kernel is short of, DESIGN.md 4i; the per-launch time of the three layers' launches is the same with and without.)
    uint32_t elo[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, ehi[4] = {0u, 0u, 0u, 0u};
    auto ext_u = [&](const v2i &z0, const v2i &z1) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            elo[q] = pk_min_u(elo[q], (uint32_t)z0[q]); ehi[q] = pk_max_u(ehi[q], (uint32_t)z0[q]);
            elo[2 + q] = pk_min_u(elo[2 + q], (uint32_t)z1[q]); ehi[2 + q] = pk_max_u(ehi[2 + q], (uint32_t)z1[q]);
        }
    };
    // COAL: a thread moves the SAME vectors of the z tile out and of the u tile in, so the tile changes owner without a barrier
    auto tiles_in_out = [&](bool incoming) {
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int v = threadIdx.x + NTHR * i, f = v / VPF, og = v % VPF;
            if (!NVC_FULL && v >= FT * VPF) break;
            int8_t *cu = Ut + f * TROW + 16 * og, *cs_ = St + f * TROW + 16 * og;
            if (zb_prev) {
                v2i z0 = *reinterpret_cast<const v2i *>(cu), z1 = *reinterpret_cast<const v2i *>(cu + 8);
                if constexpr (FOLD) fold_z(z0, z1, cs_);
                if (f < nvalid_prev) {
                    *reinterpret_cast<v4i *>(zb_prev + 2u * (unsigned)(f * H + 8 * og)) = v4i{z0[0], z0[1], z1[0], z1[1]};
                    if constexpr (FOLD) ext_u(z0, z1);
                }
            }
            if (incoming) {
                const v4i &uv = urow[UREC ? 0 : i]; // (UREC calls this for the last tile's z only)
                *reinterpret_cast<v2i *>(cu) = v2i{uv[0], uv[1]};
                *reinterpret_cast<v2i *>(cu + 8) = v2i{uv[2], uv[3]};
                *reinterpret_cast<v2i *>(cs_) = v2i{srow[i][0], srow[i][1]};
                *reinterpret_cast<v2i *>(cs_ + 8) = v2i{srow[i][2], srow[i][3]};
            }
        }
    };
    // UREC: the same, with the u vectors made here: bn16_row8(skip vector).  ARM (mfma_bn.hpp ROW_*) is wave-uniform and chosen
    // once per call.  Frames clamped past nvalid recompute a valid row, as the loads re-read one.
    auto tiles_in_urec = [&](auto arm_c) {
        constexpr int ARM = decltype(arm_c)::value;
        auto br = brow;
        if constexpr (FOLD) {
            const v4i bm = brow_lds[2 * (threadIdx.x % VPF)], bi = brow_lds[2 * (threadIdx.x % VPF) + 1];
#pragma unroll
            for (int k = 0; k < 4; ++k) { br.m[k] = (uint32_t)bm[k]; br.iv[k] = (uint32_t)bi[k]; }
        }
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
            const int v = threadIdx.x + NTHR * i, f = v / VPF, og = v % VPF;
            if (!NVC_FULL && v >= FT * VPF) break;
            int8_t *cu = Ut + f * TROW + 16 * og, *cs_ = St + f * TROW + 16 * og;
            if (zb_prev) {
                v2i z0 = *reinterpret_cast<const v2i *>(cu), z1 = *reinterpret_cast<const v2i *>(cu + 8);
                if constexpr (FOLD) fold_z(z0, z1, cs_);
                if (f < nvalid_prev) {
                    *reinterpret_cast<v4i *>(zb_prev + 2u * (unsigned)(f * H + 8 * og)) = v4i{z0[0], z0[1], z1[0], z1[1]};
                    if constexpr (FOLD) ext_u(z0, z1);
                }
            }
            if constexpr (FOLD) resolve_skip(srow[i]);
            const v4i uv = bn16_row8<ARM>(br, srow[i]);
            *reinterpret_cast<v2i *>(cu) = v2i{uv[0], uv[1]};
            *reinterpret_cast<v2i *>(cu + 8) = v2i{uv[2], uv[3]};
            *reinterpret_cast<v2i *>(cs_) = v2i{srow[i][0], srow[i][1]};
            *reinterpret_cast<v2i *>(cs_ + 8) = v2i{srow[i][2], srow[i][3]};
        }
    };

    prologue_loads_done();
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, walk.advance()) {
        const int64_t b0 = walk.b;
        const int t0 = walk.t(sr), nvalid = walk.nvalid(sr);
        const TileWalk<FT> walk_next = walk.next();
        const int64_t n0 = b0 * a.L + t0;
        // wave-uniform base of this tile; everything below is a 32-bit byte offset from it (no 64-bit address arithmetic per
        // thread: the kernel sits at its register cap)
        char *zb = reinterpret_cast<char *>(a.z + n0 * H);
        const int64_t tile_next = tile + gridDim.x;
        // EARLY: this tile's states, all rounds, requested here: they are the only loads of the loop whose result the issuing
        // tile needs, and behind the staging every wave waited a full round trip for them (and, vmcnt retiring in order, for the
        // acknowledgement of the U stores the staging had just issued).  The staging holds no accumulator, so their registers
        // are free there.  The loads are hidden from the compiler (scan_quad.hpp gload8_hidden): its own wait at their first
        // use would be vmcnt(0) behind the stores.  First the rows requested a tile ago must have landed (they have, long
        // since): a wait the compiler places for them inside the staging would count the state loads it cannot see as well.
        //   `xs` is only ever read by this kernel (the recurrence wrote it in an earlier launch), so moving its loads across
        // the U stores changes nothing.
        // A lane without an item, or on a slot the stream does not hold, re-reads slot 0 (always stored); its words are zeroed.
        constexpr int XW = PAIR ? 2 : 1; // hidden loads per round
        [[maybe_unused]] std::conditional_t<PAIR, v2i, v4i> xq[EARLY ? XW * ROUNDS : 1] = {}; // (a round the wave does not run stays zero)
        [[maybe_unused]] const bool full_prev = zb_prev && nvalid_prev == FT; // wave-uniform
        auto item_offset = [&](int i, int &o) { // the 4-step block and the byte offset of the thread's item of round i
            const int it = item_of(i), grp = it & 7;
            int p = it >> 3;
            p = it != 0xffff && (a.live_slots <= 0 || p < a.live_slots) ? p : 0;
            o = 4 * grp;
            if (o >= nvalid) o = (nvalid - 1) & ~3; // partial tile: re-read the last block (results unused)
            return PAIR ? 2u * (unsigned)(((((o >> 3) << 5) + p) << 4) + (o & 4)) : 16u * (unsigned)((o >> 2) * P + p);
        };
        if constexpr (EARLY) {
            prologue_loads_done();
            const char *xb = reinterpret_cast<const char *>(reinterpret_cast<const int16_t *>(a.xs) +
                                                            (PAIR ? pair_word(b0, t0 >> 3, 0, a.TB >> 1, P) << 1 : native_word(b0, t0, 0, 0, a.TB, P)));
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i) {
                if (i > 0 && __builtin_amdgcn_readfirstlane(item_of(i)) == 0xffff) break; // wave-uniform: no item of this round in the wave
                int o;
                const unsigned xo = item_offset(i, o);
                if constexpr (PAIR) { xq[2 * i] = gload8_hidden(xb, xo); xq[2 * i + 1] = gload8_hidden(xb, xo + 16); }
                else xq[i] = gload16_hidden(xb, xo);
            }
        }
        if constexpr (UREC) { // z of the previous tile out, skip of this one in, and u made from it
            if (brow.arm == ROW_PACKED) tiles_in_urec(std::integral_constant<int, ROW_PACKED>{});
            else if (brow.arm == ROW_SHIFTED) tiles_in_urec(std::integral_constant<int, ROW_SHIFTED>{});
            else tiles_in_urec(std::integral_constant<int, ROW_GENERIC>{});
            if constexpr (EARLY) {
                // Behind a full previous tile (zb_prev set, every frame valid: wave-uniform) each of the staging's NVC guarded
                // store instructions has been issued exactly once since the requests, whatever the compiler made of the
                // guards -- a branch around the store that a non-empty exec mask does not take, or the mask alone -- so the
                // states have landed when at most NVC operations are outstanding.  (Two copies of the staging, the second
                // with the guards compiled out, do not fit the registers: 20 to 44 bytes of scratch.)  Every other tile (the
                // first, one behind a partial tile) drains, as the encoder and decoder do for their partial tile.
                // tools/check_vmwait.py counts the stores between the requests and this wait in the compiled code.
                vm_wait_or_drain<NVC>(full_prev, xq);
            }
        } else if constexpr (COAL) tiles_in_out(true); // z of the previous tile out, u and skip of this one in
        // ---- phase A: stream items -> byte planes
        if constexpr (EARLY) {
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i) {
                if (i > 0 && __builtin_amdgcn_readfirstlane(item_of(i)) == 0xffff) break;
                if (item_of(i) != 0xffff) {
                    const int grp = item_of(i) & 7, p = item_of(i) >> 3;
                    int o;
                    item_offset(i, o);
                    const int nlive = nvalid - o; // >= 1; >= 4 everywhere but in a sequence's last block (see below)
                    const bool held = a.live_slots <= 0 || p < a.live_slots;
                    int32_t w[4];
                    if constexpr (PAIR) { // lane A: [im0 im2 | re1 re3], lane B: [re0 re2 | im1 im3] (per half)
                        const v2i qa = held ? xq[2 * i] : v2i{0, 0}, qb = held ? xq[2 * i + 1] : v2i{0, 0};
                        w[0] = (int32_t)perm((unsigned)qa[0], (unsigned)qb[0], 0x05040100u);
                        w[1] = (int32_t)perm((unsigned)qb[1], (unsigned)qa[1], 0x05040100u);
                        w[2] = (int32_t)perm((unsigned)qa[0], (unsigned)qb[0], 0x07060302u);
                        w[3] = (int32_t)perm((unsigned)qb[1], (unsigned)qa[1], 0x07060302u);
                    } else { // re of steps 0..3, then im of steps 0..3, as int16
                        const v4i q4 = held ? xq[i] : v4i{0, 0, 0, 0};
                        w[0] = (int32_t)perm((unsigned)q4[2], (unsigned)q4[0], 0x05040100u);
                        w[1] = (int32_t)perm((unsigned)q4[2], (unsigned)q4[0], 0x07060302u);
                        w[2] = (int32_t)perm((unsigned)q4[3], (unsigned)q4[1], 0x05040100u);
                        w[3] = (int32_t)perm((unsigned)q4[3], (unsigned)q4[1], 0x07060302u);
                    }
                    if (nlive < 4) {
#pragma unroll
                        for (int j = 1; j < 4; ++j) w[j] = j < nlive ? w[j] : 0;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) { // range check and complex ReLU, as in the general form below
                        pmax = __builtin_elementwise_max(pmax, __builtin_bit_cast(v2i16, w[j]));
                        pmin = __builtin_elementwise_min(pmin, __builtin_bit_cast(v2i16, w[j]));
                        const bool keep = ((int32_t)((uint32_t)w[j] << 16) + (w[j] >> 16)) > 0;
                        w[j] = keep ? w[j] : 0;
                    }
                    quad_transpose(w, l);
                    const unsigned t01 = perm((unsigned)w[1], (unsigned)w[0], 0x05010400u), u01 = perm((unsigned)w[1], (unsigned)w[0], 0x07030602u);
                    const unsigned t23 = perm((unsigned)w[3], (unsigned)w[2], 0x05010400u), u23 = perm((unsigned)w[3], (unsigned)w[2], 0x07030602u);
                    const int row = (4 * grp + (l & 3)) * KPS + (p & ~3);
                    *reinterpret_cast<int32_t *>(Sl + row) = (int32_t)(perm(t23, t01, 0x05040100u) ^ 0x80808080u);
                    *reinterpret_cast<int32_t *>(Sh + row) = (int32_t)perm(t23, t01, 0x07060302u);
                    *reinterpret_cast<int32_t *>(Sl + row + P) = (int32_t)(perm(u23, u01, 0x05040100u) ^ 0x80808080u);
                    *reinterpret_cast<int32_t *>(Sh + row + P) = (int32_t)perm(u23, u01, 0x07060302u);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < (EARLY ? 0 : ROUNDS); ++i) {
            const int q = threadIdx.x + NTHR * i;
            if (ROUNDS * NTHR == ITEMS || q < ITEMS) {
                const int grp = q / P, p = q % P;
                int o = 4 * grp;
                if (o >= nvalid) o = (nvalid - 1) & ~3; // partial tile: re-read the last block (results unused)
                // steps of the sequence's last block beyond its length (L % 4 != 0): the recurrence ran on through them
                // from whatever the stream holds there; they must not reach the range check
                const int nlive = nvalid - o; // >= 1; >= 4 everywhere but in that block
                int32_t w[4];
                if (WIDE) {
                    const int32_t *src = a.xs + native_word(b0, t0 + o, p, 0, a.TB, P);
                    const v4i cre = *reinterpret_cast<const v4i *>(src), cim = *reinterpret_cast<const v4i *>(src + 4);
                    int32_t xr[4] = {cre[0], cre[1], cre[2], cre[3]}, xi[4] = {cim[0], cim[1], cim[2], cim[3]};
#pragma unroll
                    for (int j = 0; j < 4; ++j) crelu(xr[j], xi[j]);
                    quad_transpose(xr, l);
                    quad_transpose(xi, l);
                    // this lane = frame 4*grp + (l&3); xr[m], xi[m] = state (p & ~3) + m: four byte planes each
                    const int row = (4 * grp + (l & 3)) * KPS + (p & ~3);
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int32_t(&v)[4] = c ? xi : xr;
                        const unsigned t01 = perm((unsigned)v[1], (unsigned)v[0], 0x05010400u), u01 = perm((unsigned)v[1], (unsigned)v[0], 0x07030602u);
                        const unsigned t23 = perm((unsigned)v[3], (unsigned)v[2], 0x05010400u), u23 = perm((unsigned)v[3], (unsigned)v[2], 0x07030602u);
                        int8_t *dst = Sbase + row + c * P;
                        *reinterpret_cast<int32_t *>(dst) = (int32_t)(perm(t23, t01, 0x05040100u) ^ 0x80808080u);
                        *reinterpret_cast<int32_t *>(dst + FT * KPS) = (int32_t)(perm(t23, t01, 0x07060302u) ^ 0x80808080u);
                        *reinterpret_cast<int32_t *>(dst + 2 * FT * KPS) = (int32_t)(perm(u23, u01, 0x05040100u) ^ 0x80808080u);
                        *reinterpret_cast<int32_t *>(dst + 3 * FT * KPS) = (int32_t)perm(u23, u01, 0x07060302u);
                    }
                    continue;
                }
                if (S16) {
                    if (PAIR) {
                        // one 8-step item per lane of the pair: this thread takes the half with its 4 steps from both.
                        // lane A: [im0 im2 | re1 re3], lane B: [re0 re2 | im1 im3] (per half)
                        // the tile's items of state group p >> 5 start at pair_word(b0, t0 >> 3, 32 (p >> 5), ...): uniform base + 32-bit offset
                        const char *xb = reinterpret_cast<const char *>(reinterpret_cast<const int16_t *>(a.xs) + (pair_word(b0, t0 >> 3, 0, a.TB >> 1, P) << 1));
                        const unsigned xo = 2u * (unsigned)((((((p >> 5) * (a.TB >> 1) + (o >> 3)) << 5) + (p & 31)) << 4) + (o & 4));
                        v2i qa = {0, 0}, qb = {0, 0};
                        if (a.live_slots <= 0 || p < a.live_slots) {
                            qa = *reinterpret_cast<const v2i *>(xb + xo); qb = *reinterpret_cast<const v2i *>(xb + xo + 16);
                        }
                        w[0] = (int32_t)perm((unsigned)qa[0], (unsigned)qb[0], 0x05040100u);
                        w[1] = (int32_t)perm((unsigned)qb[1], (unsigned)qa[1], 0x05040100u);
                        w[2] = (int32_t)perm((unsigned)qa[0], (unsigned)qb[0], 0x07060302u);
                        w[3] = (int32_t)perm((unsigned)qb[1], (unsigned)qa[1], 0x07060302u);
                    } else {
                    // 16 bytes: re of steps 0..3, then im of steps 0..3, as int16; w[j] = re_j | im_j << 16 by two perms
                    v4i q4 = {0, 0, 0, 0};
                    if (a.live_slots <= 0 || p < a.live_slots)
                        q4 = *reinterpret_cast<const v4i *>(reinterpret_cast<const int16_t *>(a.xs) + native_word(b0, t0 + o, p, 0, a.TB, P));
                    w[0] = (int32_t)perm((unsigned)q4[2], (unsigned)q4[0], 0x05040100u);
                    w[1] = (int32_t)perm((unsigned)q4[2], (unsigned)q4[0], 0x07060302u);
                    w[2] = (int32_t)perm((unsigned)q4[3], (unsigned)q4[1], 0x05040100u);
                    w[3] = (int32_t)perm((unsigned)q4[3], (unsigned)q4[1], 0x07060302u);
                    }
                    if (nlive < 4) { // tile-uniform except in a sequence's last tile
#pragma unroll
                        for (int j = 1; j < 4; ++j) w[j] = j < nlive ? w[j] : 0;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        pmax = __builtin_elementwise_max(pmax, __builtin_bit_cast(v2i16, w[j]));
                        pmin = __builtin_elementwise_min(pmin, __builtin_bit_cast(v2i16, w[j]));
                        // lexicographic (re, im) > (0, 0)  <=>  re * 2^16 + im > 0 (|im| < 2^15 cannot outweigh re != 0; the
                        // sum wraps only for re = -32768, a value beyond xmax: such a tile raises `redo` and is discarded)
                        const bool keep = ((int32_t)((uint32_t)w[j] << 16) + (w[j] >> 16)) > 0;
                        w[j] = keep ? w[j] : 0;
                    }
                } else {
                const int32_t *src = a.xs + native_word(b0, t0 + o, p, 0, a.TB, P);
                const v4i cre = *reinterpret_cast<const v4i *>(src), cim = *reinterpret_cast<const v4i *>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int32_t xr = j < nlive ? cre[j] : 0, xi = j < nlive ? cim[j] : 0;
                    const uint32_t ur = (uint32_t)(xr + a.xmax), ui = (uint32_t)(xi + a.xmax);
                    xrange = xrange > ur ? xrange : ur;
                    xrange = xrange > ui ? xrange : ui;
                    // complex ReLU = lexicographic max(z, 0); exact in integers while |x| <= xmax < 2^24
                    const bool keep = (xr > 0) | ((xr == 0) & (xi > 0));
                    w[j] = keep ? (int32_t)perm((unsigned)xi, (unsigned)xr, 0x05040100u) : 0;
                }
                }
                quad_transpose(w, l);
                // now: this lane = frame 4*grp + (l&3), w[m] = (re | im << 16) of state (p & ~3) + m
                const unsigned t01 = perm((unsigned)w[1], (unsigned)w[0], 0x05010400u), u01 = perm((unsigned)w[1], (unsigned)w[0], 0x07030602u);
                const unsigned t23 = perm((unsigned)w[3], (unsigned)w[2], 0x05010400u), u23 = perm((unsigned)w[3], (unsigned)w[2], 0x07030602u);
                const int row = (4 * grp + (l & 3)) * KPS + (p & ~3);
                *reinterpret_cast<int32_t *>(Sl + row) = (int32_t)(perm(t23, t01, 0x05040100u) ^ 0x80808080u);
                *reinterpret_cast<int32_t *>(Sh + row) = (int32_t)perm(t23, t01, 0x07060302u);
                *reinterpret_cast<int32_t *>(Sl + row + P) = (int32_t)(perm(u23, u01, 0x05040100u) ^ 0x80808080u);
                *reinterpret_cast<int32_t *>(Sh + row + P) = (int32_t)perm(u23, u01, 0x07060302u);
            }
        }
        if constexpr (COAL) {
            if (tile_next < tiles) { // the registers are free again: the next tile's rows, a whole tile ahead
                if constexpr (!UREC) load_tile(urow, a.u, walk_next);
                load_tile(srow, a.skip, walk_next);
            }
        }
        lds_barrier();
        // ---- phase B1: C projection + first epilogue
        int32_t x1v[NU][16];
        uint32_t x1p[NU][8]; // PK16: the same values as int16 pairs (channels 2q, 2q+1 of group g at [2g + q])
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int sub = sub0 + u * SUBSTEP;
            const int64_t n = n0 + 32 * sub + r;
            const int8_t *row0 = Sbase + (32 * sub + r) * KPS + 16 * h;
            v16i are, aim;
            mfma_nplanes<KS, NPL>(are, wre, row0, FT * KPS, csr + ch0);
            mfma_nplanes<KS, NPL>(aim, wim, row0 + P, FT * KPS, csi + ch0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const v4i Dv = *reinterpret_cast<const v4i *>(Dl + ch0 + 8 * g);
                const int off = (32 * sub + r) * KPX + ch0 + 8 * g;
                if constexpr (PK16) {
                    // fxpmodel.py:746-793 + :1125 on int16 pairs: cx = sat(sat(cr) - sat(ci)); y = sat(2 cx + sat(D u)); x1 = max(y, 0)
                    int32_t ubn[4];
                    if constexpr (GBN) { // u = BatchNorm(layer input) of these four channels, as the B projection computes it
                        int32_t hin[4], tbn[4];
                        unpack4_i16(sq[u][g], hin);
                        bn16_x4(bn, hin, ch0 + 8 * g, tbn, ubn);
                    }
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const uint32_t crp = pk_cvt(asr(are[4 * g + 2 * q], a.rs_re), asr(are[4 * g + 2 * q + 1], a.rs_re));
                        const uint32_t cip = pk_cvt(asr(aim[4 * g + 2 * q], a.rs_im), asr(aim[4 * g + 2 * q + 1], a.rs_im));
                        uint32_t dup;
                        if constexpr (GBN) {
                            dup = pk_cvt(asr(__mul24(Dv[2 * q], ubn[2 * q]), a.rs_d), asr(__mul24(Dv[2 * q + 1], ubn[2 * q + 1]), a.rs_d));
                        } else {
                            uint32_t upk;
                            if constexpr (COAL) upk = (uint32_t)(*reinterpret_cast<const v2i *>(Ut + (32 * sub + r) * TROW + 2 * (ch0 + 8 * g)))[q];
                            else upk = (uint32_t)uq[u][g][q];
                            dup = pk_cvt(asr(mul24_h<0>(Dv[2 * q], upk), a.rs_d), asr(mul24_h<1>(Dv[2 * q + 1], upk), a.rs_d));
                        }
                        const uint32_t yp = pk_mad_sat(pk_sub_sat(crp, cip), 0x00020002u, dup); // 2*cx is not clipped, :765-767
                        x1p[u][2 * g + q] = pk_max(yp, 0u);
                    }
                    const uint32_t p01 = x1p[u][2 * g], p23 = x1p[u][2 * g + 1];
                    *reinterpret_cast<int32_t *>(Xl + off) = (int32_t)(perm(p23, p01, 0x06040200u) ^ 0x80808080u);
                    *reinterpret_cast<int32_t *>(Xh + off) = (int32_t)perm(p23, p01, 0x07050301u);
                } else {
                int32_t uv[4], xv[4];
                unpack4_i16(uq[u][g], uv);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int32_t cr = sat(asr(are[4 * g + e], a.rs_re), a.y_bits);
                    const int32_t ci = sat(asr(aim[4 * g + e], a.rs_im), a.y_bits);
                    const int32_t cx = sat(cr - ci, a.y_bits);
                    const int32_t du = sat(asr(__mul24(Dv[e], uv[e]), a.rs_d), a.y_bits);
                    const int32_t y = sat(2 * cx + du, a.y_bits); // 2*cx is not clipped, fxpmodel.py:765-767
                    if (TRACE) {
                        if (a.tr_ys && 32 * sub + r < nvalid && (!RAGGED || ch0 + 8 * g < H)) a.tr_ys[n * H + ch0 + 8 * g + e] = y;
                    }
                    const int32_t x1 = y < 0 ? 0 : y;
                    x1v[u][4 * g + e] = x1;
                    xv[e] = x1;
                }
                if (a.conv) { // uniform: the out2 input conversion is usually the identity
#pragma unroll
                    for (int e = 0; e < 4; ++e) xv[e] = sat(asr(wshl(xv[e], cv_l), cv_r), cv_b);
                }
                const unsigned p01 = perm((unsigned)xv[1], (unsigned)xv[0], 0x05010400u), p23 = perm((unsigned)xv[3], (unsigned)xv[2], 0x05010400u);
                *reinterpret_cast<int32_t *>(Xl + off) = (int32_t)(perm(p23, p01, 0x05040100u) ^ 0x80808080u);
                *reinterpret_cast<int32_t *>(Xh + off) = (int32_t)perm(p23, p01, 0x07060302u);
                }
            }
        }
        if constexpr (!GBN) {
            if (!COAL && tile_next < tiles) load_rows(uq, a.u, walk_next); // the first epilogue is done with u
        }
        lds_barrier();
        // ---- phase B2: out2 + second epilogue
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int sub = sub0 + u * SUBSTEP;
            const int64_t n = n0 + 32 * sub + r;
            v16i acc;
            mfma_planes<NT>(acc, wo2, Xh + (32 * sub + r) * KPX + 16 * h, Xl + (32 * sub + r) * KPX + 16 * h, cs2 + ch0);
            auto b2_pk16 = [&]() {
                // out2 bias, table sigmoid, gate (fxpmodel.py:1133-1137, :97-144, :1075-1093) on int16 pairs
                const uint32_t lm = 0x10001u * (uint32_t)(1 << lq_l), lr = 0x10001u * (uint32_t)lq_r;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = ch0 + 8 * g;
                    const v2i bp = *reinterpret_cast<const v2i *>(be + (ch >> 1));
                    v2i zo;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        uint32_t gp = pk_cvt(asr(acc[4 * g + 2 * q], a.rs_o2), asr(acc[4 * g + 2 * q + 1], a.rs_o2));
                        gp = pk_add_sat(gp, (uint32_t)bp[q]);
                        const int32_t r0 = sigd[ashr_h<0>(dsh, gp) + dbias], r1 = sigd[ashr_h<1>(dsh, gp) + dbias];
                        uint32_t lp = x1p[u][2 * g + q];
                        // change_cfg of the gate's l operand: a saturating left shift (x lm) or a right shift, never both -- applied
                        // as both (x 1 and >> 0 are the identity) rather than behind two uniform branches per pair
                        lp = pk_ashr_u(pk_mul_sat_u(lp, lm), lr);
                        const uint32_t zp = pk_cvt(asr(mul24_h<0>(r0, lp), a.rs_gate), asr(mul24_h<1>(r1, lp), a.rs_gate));
                        zo[q] = (int)zp;
                        uint32_t sp;
                        if constexpr (COAL) sp = (uint32_t)(*reinterpret_cast<const v2i *>(St + (32 * sub + r) * TROW + 2 * ch))[q];
                        else sp = (uint32_t)sq[u][g][q];
                        mx[0] = fmaxf(mx[0], fabsf(__fmaf_rn(cvtf_h<0>(zp), kz, cvtf_h<0>(sp))));
                        mx[0] = fmaxf(mx[0], fabsf(__fmaf_rn(cvtf_h<1>(zp), kz, cvtf_h<1>(sp))));
                    }
                    if constexpr (COAL) *reinterpret_cast<v2i *>(Ut + (32 * sub + r) * TROW + 2 * ch) = zo; // u is done with: B1 is behind a barrier
                    else if (!RAGGED || ch < H) *reinterpret_cast<v2i *>(zb + 2u * (unsigned)((32 * sub + r) * H + ch)) = zo;
                }
            };
            if constexpr (PK16) {
                if (32 * sub + r < nvalid) b2_pk16();
            }
            if (!PK16 && 32 * sub + r < nvalid) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = ch0 + 8 * g;
                    const v4i bv = *reinterpret_cast<const v4i *>(be + ch);
                    int32_t sv[4], o[4];
                    unpack4_i16(sq[u][g], sv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        int32_t gq = sat(asr(acc[4 * g + e], a.rs_o2), a.out_bits);
                        gq = sat(gq + bv[e], a.out_bits);
                        // LUT sigmoid (fxp_prims.hpp sigmoid_lut) + change_cfg to the gate's r operand.  Both are
                        // functions of the sign of xx and of (min(|xx| >> sx, 6), |xx| mod 2^sx) only: 2 x 7 x 2^sx
                        // values, tabulated by the host with the same formula (s5fxp_fast.hpp).  The TRACE
                        // instantiation computes s the long way (it has to write it out).
                        int32_t s = 0, rq;
                        if (DIRECT) {
                            rq = sigd[(gq >> dsh) + dbias];
                        } else {
                        const int32_t xx = chexp(gq, a.out_bits, a.out_exp, sx);
                        const int32_t ax = xx < 0 ? -xx : xx;
                        int32_t ind = ax >> sx;
                        ind = ind > 6 ? 6 : ind;
                        const int32_t mu = ax & (S - 1);
                        if (TRACE) {
                            const uint32_t pr = (uint32_t)lutp[ind];
                            const int32_t half = (__mul24(S - mu, (int32_t)(pr & 0xffffu)) >> sx) + (__mul24(mu, (int32_t)(pr >> 16)) >> sx);
                            s = (1 << (a.sig_y - 1)) + (xx > 0 ? half : -half);
                            rq = chcfg(s, a.out_bits, a.sig_y, a.r_bits, a.r_exp);
                        } else {
                            rq = sigt[((ind << sx) | mu) + (xx > 0 ? 7 * S : 0)];
                        }
                        }
                        const int32_t lq = chcfg(x1v[u][4 * g + e], a.y_bits, a.y_exp, a.l_bits, a.l_exp);
                        const int32_t z = sat(asr(__mul24(lq, rq), a.rs_gate), a.res_bits);
                        if (TRACE && (!RAGGED || ch < H)) {
                            if (a.tr_out2) a.tr_out2[n * H + ch + e] = gq;
                            if (a.tr_sig) a.tr_sig[n * H + ch + e] = s;
                            if (a.tr_z) a.tr_z[n * H + ch + e] = z;
                        }
                        o[e] = z;
                        const float cz = (float)z, cs = (float)sv[e];
                        // only max |z + skip| chooses the exponent (fxparray.py:421-425); the operands' own maxima
                        // (slots 9, 10) merely size the reference's intermediate bit width and are not needed
                        mx[0] = fmaxf(mx[0], fabsf(__fmaf_rn(cz, kz, cs)));
                    }
                    if (!RAGGED || ch < H) *reinterpret_cast<v2i *>(zb + 2u * (unsigned)((32 * sub + r) * H + ch)) = pack4_i16(o[0], o[1], o[2], o[3]);
                }
            }
        }
        if constexpr (COAL) {
            zb_prev = zb; nvalid_prev = nvalid;
            lds_barrier(); // every wave's z pieces are in the tile, every wave is done with the skip tile
        } else {
            if (tile_next < tiles) load_rows(sq, a.skip, walk_next); // the second epilogue is done with skip
        }
    }
    if constexpr (COAL) tiles_in_out(false); // the last tile's z
    // FOLD, gate_ext: the tiles are dead.  Behind a barrier (other threads' vectors lie where this one writes) every thread parks
    // its eight packed words in the tile space: [bound][thread][pair]
    [[maybe_unused]] float *ext_next = nullptr;
    [[maybe_unused]] uint32_t *ext_lds = reinterpret_cast<uint32_t *>(Ut);
    if constexpr (FOLD) {
        static_assert(2 * NTHR * 16 <= 2 * FT * TROW, "the parked extremes fit the two tiles");
        ext_next = ext_next_of(a_k);
        if (ext_next) { // (a kernel argument: uniform)
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) { // (8-byte accesses, like every access to the tiles)
                *reinterpret_cast<v2i *>(ext_lds + 4 * threadIdx.x + 2 * q) = v2i{(int)elo[2 * q], (int)elo[2 * q + 1]};
                *reinterpret_cast<v2i *>(ext_lds + 4 * (NTHR + threadIdx.x) + 2 * q) = v2i{(int)ehi[2 * q], (int)ehi[2 * q + 1]};
            }
        }
    }
    // ---- range flag and the three maxima (scaled back: power-of-two factors, exact)
    if (S16) {
        const int hi = pmax[0] > pmax[1] ? pmax[0] : pmax[1], lo = pmin[0] < pmin[1] ? pmin[0] : pmin[1];
        if (hi > a.xmax || lo < -a.xmax) xrange = 0xffffffffu;
    }
    if (__any(xrange > 2u * (uint32_t)a.xmax) && l == 0) {
        atomicExch(&a.dynw->redo, 1);
        atomicOr(a.status, a.bad_bits);
    }
    mx[0] = ldexpf(mx[0], -skip_e);
    mx[1] = ldexpf(mx[1], -a.res_exp);
    mx[2] = ldexpf(mx[2], -skip_e);
    // EARLY: the thread index behind an empty statement, so that what the tail derives from it (the wave index, the word of the
    // maxima) is computed here: kept across the tile loop for these uses alone, two such values were spilled
    unsigned tx = threadIdx.x;
    if constexpr (EARLY) asm volatile("" : "+v"(tx));
    const int wave_r = EARLY ? (int)(tx >> 6) : wave;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = mx[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
        if (l == 0) red[i * 16 + wave_r] = x;
    }
    __syncthreads();
    if (tx < 3) {
        float x = red[tx * 16];
        for (int w = 1; w < NW; ++w) x = fmaxf(x, red[tx * 16 + w]);
        atomicMax(a.dynw->mx + a.mx_slot + tx, __float_as_uint(x));
    }
    // FOLD, gate_ext: one thread per (bound, channel) folds the NTHR / VPF threads that own the channel's group (the barrier above
    // stands between their stores and these loads) and issues one biased-float atomicMax into this workgroup's replica of the
    // next layer's extremes: EXT_BIAS -+ U as the read-only pass encodes h, but in U units (U <= 65534 is exact in float32)
    // A workgroup that had no tile (the launcher's grid_for() never makes one: the grid is at most the tile count) holds the
    // identities alone and publishes nothing: its replica's words keep their zeros or what the other workgroups left there.
    if constexpr (FOLD) {
        if (ext_next && (int64_t)blockIdx.x < tiles) {
            gshift_nn(ext_next, (int64_t)blockIdx.y * go.ws);
            for (int item = threadIdx.x; item < 2 * H; item += NTHR) {
                const bool is_max = item >= H;
                const int c = is_max ? item - H : item;
                const uint16_t *src = reinterpret_cast<const uint16_t *>(ext_lds + (is_max ? 4 * NTHR : 0)) + 8 * (c >> 3) + (c & 7);
                int32_t v = is_max ? 0 : 65535;
#pragma unroll 4
                for (int k = 0; k < NTHR / VPF; ++k) {
                    const int32_t t = src[8 * VPF * k];
                    v = is_max ? max(v, t) : min(v, t);
                }
                atomicMax(reinterpret_cast<uint32_t *>(ext_next) + (int)(blockIdx.x % EXT_REPS) * 2 * H + item,
                          __float_as_uint(is_max ? EXT_BIAS + (float)v : EXT_BIAS - (float)v));
            }
        }
    }
