// proj_enc_body.inc -- the body of k_enc_p, k_enc_pf and k_enc_ps (proj_p.hpp), included by each with IO = IO_I32 / IO_F32 /
// IO_I16.
    constexpr bool F32 = IO == IO_F32, I16 = IO == IO_I16;
    {
        const int64_t g = blockIdx.y;
        gshift(a.x, g * go.x); gshift(a.y, g * go.ws); gshift(a.status, g * go.status); gshift(ext, g * go.ws);
    }
    constexpr int KS = 9, FT = 64, KP = 32 * KS + 16, NW = 6, H = 32 * NT;
    // phase B units (32-frame half, column tile) per wave: NT <= 3: wave -> (half wave / NT, tile wave % NT), one unit;
    // NT > 3: wave -> tile `wave`, both halves.  UW waves have units: all six at NT = 3 and 6; at NT = 2 and 5 the last
    // two / the last one sit phase B out (its weights stay per wave: a second tile's would not fit the registers)
    constexpr int NU = NT <= 3 ? 1 : 2, SUBSTEP = NT <= 3 ? 0 : 1, UW = NT <= 3 ? 2 * NT : NT;
    static_assert(UW <= NW, "one wave per unit or per column tile");
    constexpr bool RAGGED = shape_channels(NT) != 32 * NT; // the last column tile is half empty: its stores are conditional
    constexpr int RPW = (FT + NW - 1) / NW; // rows per wave
    extern __shared__ __attribute__((aligned(16))) int8_t smem[];
    int32_t *cs = reinterpret_cast<int32_t *>(smem), *be = cs + H;
    int8_t *Xh = reinterpret_cast<int8_t *>(be + H), *Xl = Xh + FT * KP;
    uint32_t *ehi = reinterpret_cast<uint32_t *>(Xl + FT * KP), *elo = ehi + H;
    const int l = threadIdx.x & 63, r = l & 31, h = l >> 5, wave = threadIdx.x >> 6;
    const int ct = wave % NT, sub0 = wave / NT, ch0 = 32 * ct + 4 * h;
    const int64_t tiles = (a.N + FT - 1) / FT;
    const int K = a.K, rem = K - 256;
    uint32_t pk[16]; // low half: max, high half: 65535 - min
#pragma unroll
    for (int i = 0; i < 16; ++i) pk[i] = 0;
    v4i wreg[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        wreg[ks] = *reinterpret_cast<const v4i *>(a.w.wt + (size_t)(32 * ct + r) * a.w.Kp + 32 * ks + 16 * h);
    for (int i = threadIdx.x; i < H; i += 384) {
        cs[i] = a.w.cs128[i];
        be[i] = a.bias_eff[i];
        ehi[i] = 0;
        elo[i] = 0;
    }
    const CfgOp cv = make_cfg(a.conv != 0, a.xb, a.xe, a.inp_bits, a.inp_exp);
    const SatB so = sat_bounds(a.out_bits);
    [[maybe_unused]] const float sc = F32 ? ldexpf(1.f, a.xe) : 0.f; // the float input's quantisation scale
    // rows wave, wave+6, ... of the tile.  Two workgroups of six waves per CU are three waves per SIMD whatever the kernel
    // does, so it may hold 168 registers: all of a tile's rows are requested a tile ahead (dim 0.5; the two-unit phase B
    // of dim 1.0 has no room for that: there the first RA rows are prefetched and the rest requested at the top of phase A).
    // The prefetch is issued behind the compiler's back (scan_quad.hpp vm_wait): its own wait at the first use -- a tile
    // later, behind phase B's stores -- would be vmcnt(0), every tile opening with a wait for the previous tile's stores.
    constexpr int RA = NT <= 3 ? RPW : 3, RB = RPW - RA;
    using RowVec = std::conditional_t<I16, v2i, v4i>; // a lane's four elements of a row
    constexpr unsigned RVB = I16 ? 8u : 16u;
    RowVec rawa[RA], rawb[RB > 0 ? RB : 1];
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto row_base = [&](int64_t tl, int i) { // wave-uniform
        int64_t n = tl * FT + wave_u + NW * i;
        n = n < a.N ? n : a.N - 1;
        if constexpr (I16) return reinterpret_cast<const char *>(reinterpret_cast<const int16_t *>(a.x) + n * K);
        else return reinterpret_cast<const char *>(a.x + n * K);
    };
    auto row_ptr = [&](int64_t tl, int i) {
        return reinterpret_cast<const RowVec *>(row_base(tl, i) + (int)RVB * l); // 4-byte aligned 16-byte load (int16: 2-byte aligned, 8 bytes)
    };
    auto load_hidden = [&](const char *base) { return gload_hidden<RowVec>(base, RVB * (unsigned)l); };
    auto convert_row = [&](const auto &q, int f, bool &wide) { // (generic: the arm of the other row type is not instantiated)
        constexpr bool Q16 = sizeof(q) == 8;
        static_assert(Q16 == I16, "row vector");
        if constexpr (Q16) {
            if (!a.conv) { // uniform: the loaded pairs are the perms' operands
                *reinterpret_cast<int32_t *>(Xl + f * KP + 4 * l) = (int32_t)(perm((unsigned)q[1], (unsigned)q[0], 0x06040200u) ^ 0x80808080u);
                *reinterpret_cast<int32_t *>(Xh + f * KP + 4 * l) = (int32_t)perm((unsigned)q[1], (unsigned)q[0], 0x07050301u);
                return;
            }
        }
        int32_t v[4];
        if constexpr (Q16) unpack4_i16(q, v);
        else { v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3]; }
        if constexpr (F32) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fromfp(__int_as_float(q[e]), sc, a.xb);
        }
        if (a.conv) { // uniform: usually the input already has the encoder's configuration
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = cv(v[e]);
        }
        if constexpr (!Q16) { // (an int16 input cannot be wide)
#pragma unroll
            for (int e = 0; e < 4; ++e) wide |= (v[e] != (int32_t)(int16_t)v[e]);
        }
        const unsigned p01 = perm((unsigned)v[1], (unsigned)v[0], 0x05010400u), p23 = perm((unsigned)v[3], (unsigned)v[2], 0x05010400u);
        *reinterpret_cast<int32_t *>(Xl + f * KP + 4 * l) = (int32_t)(perm(p23, p01, 0x05040100u) ^ 0x80808080u);
        *reinterpret_cast<int32_t *>(Xh + f * KP + 4 * l) = (int32_t)perm(p23, p01, 0x07060302u);
    };
    int64_t tile = blockIdx.x;
    if (tile < tiles) {
#pragma unroll
        for (int i = 0; i < RA; ++i) rawa[i] = load_hidden(row_base(tile, i));
    }
    bool wide = false;
    __syncthreads();
    PHASE_DECL
    prologue_loads_done();
    const bool even = a.M == H; // no ragged column tile: full tiles store unconditionally
    for (; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * FT;
        PHASE_MARK(0, l); // loop top (includes the previous tile's closing barrier)
        // ---- phase A
        // the prefetched rows are older than the previous tile's stores: NU x 4 per wave on the unconditional path (the
        // conditional one ends with a full wait)
        vm_wait<RAGGED ? 0 : 4 * NU>(rawa);
        if constexpr (RB > 0) {
#pragma unroll
            for (int i = 0; i < RB; ++i) rawb[i] = *row_ptr(tile, RA + i);
        }
#pragma unroll
        for (int i = 0; i < RA; ++i)
            if (wave_u + NW * i < FT) convert_row(rawa[i], wave_u + NW * i, wide);
        PHASE_MARK(1, rawa[RA - 1][0]); // prefetched rows converted
        if constexpr (RB > 0) {
#pragma unroll
            for (int i = 0; i < RB; ++i)
                if (wave_u + NW * (RA + i) < FT) convert_row(rawb[i], wave_u + NW * (RA + i), wide);
        }
        PHASE_MARK(2, rawb[0][0]); // rows requested at the top (their HBM latency included)
        for (int e = threadIdx.x; e < FT * rem; e += 384) { // the K-256 tail of every row
            const int f = e / rem, k = 256 + e % rem;
            int64_t n = n0 + f;
            n = n < a.N ? n : a.N - 1;
            int32_t xv;
            if constexpr (I16) xv = reinterpret_cast<const int16_t *>(a.x)[n * K + k];
            else xv = a.x[n * K + k];
            if constexpr (F32) xv = fromfp(__int_as_float(xv), sc, a.xb);
            const int32_t v = cv(xv);
            if constexpr (!I16) wide |= (v != (int32_t)(int16_t)v);
            Xl[f * KP + k] = (int8_t)((v & 0xff) ^ 0x80);
            Xh[f * KP + k] = (int8_t)(v >> 8);
        }
        if (tile + gridDim.x < tiles) {
#pragma unroll
            for (int i = 0; i < RA; ++i) rawa[i] = load_hidden(row_base(tile + gridDim.x, i)); // in flight during phase B
        }
        PHASE_MARK(3, l); // tail column + prefetch issue
        __syncthreads();
        PHASE_MARK(4, l); // mid barrier
        // ---- phase B
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (UW < NW && wave_u >= UW) break;
            const int sub = sub0 + u * SUBSTEP;
            const int64_t n = n0 + 32 * sub + r;
            v16i acc;
            mfma_planes<KS>(acc, wreg, Xh + (32 * sub + r) * KP + 16 * h, Xl + (32 * sub + r) * KP + 16 * h, cs + ch0);
            PHASE_MARK(5, acc[15]); // operand reads + MFMA chain, complete
            auto group = [&](int g) {
                const int ch = ch0 + 8 * g;
                const v4i bv = *reinterpret_cast<const v4i *>(be + ch);
                int32_t o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int32_t v = sat(asr(acc[4 * g + e], a.rs), so);
                    v = sat(wadd(v, bv[e]), so);
                    o[e] = v < 0 ? 0 : v;
                    // (v, 65535 - v) as a u16 pair; one packed max keeps both running extremes
                    const uint32_t t = (uint32_t)__umul24((unsigned)o[e], 0x10001u) ^ 0xffff0000u;
                    pk[4 * g + e] = __builtin_bit_cast(
                        uint32_t, __builtin_elementwise_max(__builtin_bit_cast(v2u16, pk[4 * g + e]), __builtin_bit_cast(v2u16, t)));
                }
                *reinterpret_cast<v2i *>(a.y + n * a.M + ch) = pack4_i16(o[0], o[1], o[2], o[3]);
            };
            if (even && n0 + FT <= a.N) { // no control flow around the stores (see vm_wait above)
#pragma unroll
                for (int g = 0; g < 4; ++g) group(g);
            } else {
                if (n < a.N) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (ch0 + 8 * g < a.M) group(g);
                }
                prologue_loads_done(); // nothing in flight behind a conditional store
            }
        }
        PHASE_MARK(6, pk[15]); // epilogue arithmetic done, stores issued
        __syncthreads(); // planes are single-buffered
    }
    PHASE_DUMP;
    if (__any(wide) && l == 0) atomicOr(a.status, ST_WIDE_INPUT);
    if (!ext) return;
    // ---- extremes: fold the 32 frame lanes of each half wave, then the waves of the workgroup (LDS), then one
    // atomic per channel and bound
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        uint32_t v = pk[i];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
            const uint32_t lo16 = (v & 0xffffu) > (w & 0xffffu) ? (v & 0xffffu) : (w & 0xffffu);
            const uint32_t hi16 = (v >> 16) > (w >> 16) ? (v >> 16) : (w >> 16);
            v = lo16 | (hi16 << 16);
        }
        const int ch = ch0 + 8 * (i >> 2) + (i & 3);
        if (r == 0 && ch < a.M) {
            atomicMax(&ehi[ch], v & 0xffffu);
            atomicMax(&elo[ch], v >> 16);
        }
    }
    __syncthreads();
    if (threadIdx.x < a.M) { // max = ehi, min = 65535 - elo; as the positive floats of mfma_bn.hpp
        const int c = threadIdx.x;
        uint32_t *dst = reinterpret_cast<uint32_t *>(ext) + (ext_reps > 1 ? (int)(blockIdx.x % ext_reps) : 0) * 2 * a.M;
        atomicMax(dst + c, __float_as_uint(EXT_BIAS - (float)(65535 - (int)elo[c])));
        atomicMax(dst + a.M + c, __float_as_uint(EXT_BIAS + (float)ehi[c]));
    }
