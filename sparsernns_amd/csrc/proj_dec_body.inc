// proj_dec_body.inc -- the body of k_dec_p, k_dec_pf and k_dec_ps (proj_p.hpp), included by each with IO = IO_I32 / IO_F32 /
// IO_I16.
    constexpr bool F32 = IO == IO_F32, I16 = IO == IO_I16;
    constexpr unsigned YB = I16 ? 2u : 4u; // bytes of an output value
    {
        const int64_t g = blockIdx.y;
        gshift(a.x, g * go.ws); gshift(a.y, g * go.y); gshift(a.xe.dyn, g * go.ws); gshift(a.status, g * go.status);
        if constexpr (RESID) {
            gshift(rz.z, g * go.ws); gshift_nn(rz.hd.d, g * go.ws); gshift(rz.hd.skip_e.dyn, g * go.ws);
            gshift_nn(rz.hd.status_exps, g * go.status);
        }
    }
    // H: the real channels (row stride, vectors per frame); HP: the k extent of the byte planes (shape_channels)
    constexpr int H = shape_channels(KS), HP = 32 * KS, FT = 64, KP = HP + 16, NW = 6, CT = 9, CPW = 3;
    constexpr int VPF = H / 8, NV = FT * VPF / 384;
    constexpr bool USUM = RESID && KS == 3; // the one-plane route exists where the 32-frame gate kernel does: H = 96 (DecResid::usum)
    static_assert(FT * VPF % 384 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) int8_t smem[];
    int8_t *Xh = smem, *Xl = Xh + FT * KP;
    // Phase B writes its values into an LDS tile behind the planes -- the flat image of the tile's FT x M block of y, pitch
    // exactly M, no padding -- and after the closing barrier all threads move that block out as 16-byte vectors: one wave
    // instruction covers 1 KB of consecutive addresses, where a store from the accumulator layout covers two 128-byte pieces
    // of two rows.  Vector v = threadIdx.x + 384 i; a wave issues round i while one of its lanes has a vector.
    int8_t *Yt = Xl + FT * KP;
    constexpr int MAXR = (FT * 288 * (int)YB / 16 + 383) / 384;                  // rounds at the widest output (M <= 288)
    static_assert(MAXR <= 12, "vm_wait_upto12");
    const unsigned nvec_full = (unsigned)(FT * YB / 16) * (unsigned)a.M;        // 16-byte vectors of a full tile: FT M YB is a multiple of 16
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the copy-out's store instructions of this wave on a full tile (a partly active last round is issued)
    const int cnt_full = nvec_full > 64u * wv ? (int)((nvec_full - 64u * wv + 383u) / 384u) : 0;
    zero_plane_tail<H, HP, KP>(Xh, 2 * FT); // (visible behind the first tile's barrier)
    const int l = threadIdx.x & 63, r = l & 31, h = l >> 5, wave = threadIdx.x >> 6;
    const int sub = wave / 3, c0 = wave % 3;
    const int64_t tiles = (a.N + FT - 1) / FT;
    AddCb rp{};
    if constexpr (RESID) {
        __shared__ AddCb sp;
        if (rz.hd.enable) {
            if (threadIdx.x == 0) {
                sp = finalize_add_cb(rz.hd.d->mx + (rz.hd.d->redo ? rz.hd.redo_slot : 8), rz.hd.res_exp, rz.hd.skip_e.get(), rz.res_bits, a.status);
                if (blockIdx.x == 0) {
                    rz.hd.d->res = sp;
                    rz.hd.status_exps[4] = sp.eo;
                }
            }
            __syncthreads();
            rp = sp;
        } else {
            rp = rz.hd.d->res;
        }
    }
    const int xe0 = RESID ? rp.eo : a.xe.get();
    const bool conv = a.xb > a.inp_bits || xe0 > a.inp_exp;
    int rs = (conv ? a.inp_exp : xe0) + a.w_exp - a.out_exp;
    if (rs < 0 || rs > 31) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(a.status, ST_NEGSHIFT);
        rs = rs < 0 ? 0 : 31;
    }
    const CfgOp cv = make_cfg(conv, a.xb, xe0, a.inp_bits, a.inp_exp);
    const SatB so = sat_bounds(a.out_bits);
    AddCbV rpv{};
    if constexpr (RESID) rpv = make_add_cb_v(rp, rz.res_bits, rz.skip_bits, rz.res_bits);
    v4i wreg[CPW][KS];
    int32_t csv[CPW], bev[CPW];
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
        const int col = 32 * (c0 + 3 * c) + r;
        csv[c] = a.w.cs128[col];
        bev[c] = a.bias_eff[col];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            wreg[c][ks] = *reinterpret_cast<const v4i *>(a.w.wt + (size_t)col * a.w.Kp + 32 * ks + 16 * h);
    }
    v4i raw[NV], rawz[RESID ? NV : 1];
    auto fetch = [&](int64_t tl) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = threadIdx.x + 384 * i;
            const int64_t left = a.N - tl * FT; // frames from the tile's first to the end of the tensor (wave-uniform)
            int f = v / VPF;
            f = f < left ? f : (int)left - 1;
            if (RESID && !(USUM && rz.usum))
                rawz[i] = gload16_hidden(reinterpret_cast<const char *>(rz.z + tl * FT * H), 2u * (unsigned)(f * H + 8 * (v % VPF)));
            // issued behind the compiler's back (see vm_wait): its wait-count pass would otherwise guard the first use of
            // these registers, a tile later, with vmcnt(0) -- behind the stores of this tile's copy-out
            raw[i] = gload16_hidden(reinterpret_cast<const char *>(a.x + tl * FT * H), 2u * (unsigned)(f * H + 8 * (v % VPF)));
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < tiles) fetch(tile);
    prologue_loads_done();
    for (; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * FT;
        // the prefetched rows are older than the previous tile's copy-out and nothing else: cnt_full stores of this wave (every
        // tile but the tensor's last is full; that last one has no successor, and the first tile's rows have arrived)
        vm_wait_upto12(cnt_full, raw);
        if (RESID && !(USUM && rz.usum)) vm_wait_upto12(cnt_full, rawz);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = threadIdx.x + 384 * i, f = v / VPF, og = v % VPF;
            int32_t x[8];
            if (USUM && rz.usum) {
                unpack8_u16(raw[i], x);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = resolve_u16(x[e], rpv.lsh, rpv.rsh, rpv.so);
            } else if constexpr (!RESID) {
                unpack8_i16(raw[i], x);
            } else {
                unpack8_i16(raw[i], x);
                int32_t z[8];
                unpack8_i16(rawz[i], z);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int32_t rr = add_cb_apply(z[e], x[e], rpv);
                    x[e] = rr < 0 ? 0 : rr;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = cv(x[e]);
            v2i hi, lo;
            planes8_from_i32(x, hi, lo);
            *reinterpret_cast<v2i *>(Xh + f * KP + 8 * og) = hi;
            *reinterpret_cast<v2i *>(Xl + f * KP + 8 * og) = lo;
        }
        if (tile + gridDim.x < tiles) fetch(tile + gridDim.x);
        __syncthreads();
        const int8_t *rowh = Xh + (32 * sub + r) * KP + 16 * h, *rowl = Xl + (32 * sub + r) * KP + 16 * h;
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
            const int col = 32 * (c0 + 3 * c) + r;
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
            // one LDS store per value; lanes of the ragged last column tile (col >= M) write nothing.  Frames past the end of the
            // tensor hold copies of its last row (fetch clamps) and are written too: the copy-out leaves them behind
            if (col < a.M) {
                // a running pointer formed per tile: sixteen hoisted offsets per column tile would cost the kernel its registers
                unsigned tq = YB * (unsigned)((32 * sub + 4 * h) * a.M + col);
                asm volatile("" : "+v"(tq));
                int8_t *tp = Yt + tq;
                const unsigned tstep = YB * (unsigned)a.M;
#pragma unroll
                for (int i = 0; i < 16; ++i) { // frames (i & 3) + 8 * (i >> 2)
                    const int32_t v = sat(asr(acc[i], rs), so);
                    if constexpr (F32) *reinterpret_cast<float *>(tp) = tofloat(sat(wadd(v, bev[c]), so), a.out_exp);
                    else if constexpr (I16) *reinterpret_cast<int16_t *>(tp) = (int16_t)sat(wadd(v, bev[c]), so);
                    else *reinterpret_cast<int32_t *>(tp) = sat(wadd(v, bev[c]), so);
                    tp += (i & 3) == 3 ? 5 * tstep : tstep;
                }
            }
            __builtin_amdgcn_sched_barrier(0); // one column tile at a time: interleaved, the three of a wave do not fit its registers
        }
        __syncthreads(); // planes are single-buffered; the output tile is complete
        {
            // ---- copy-out: the tile's valid bytes, front to back.  The tile's base is aligned to an output element and no
            // further (a group's y lies B L M elements behind the previous one's), and that is all these stores assume.
            const int64_t left = a.N - n0;
            const unsigned nbytes = left >= FT ? 16u * nvec_full : YB * (unsigned)left * (unsigned)a.M, nvec = nbytes >> 4;
            char *yt; // wave-uniform; 32-bit byte offsets from here
            if constexpr (I16) yt = reinterpret_cast<char *>(reinterpret_cast<int16_t *>(a.y) + n0 * a.M);
            else yt = reinterpret_cast<char *>(a.y + n0 * a.M);
            constexpr int CH = 6; // rounds whose LDS reads are in flight together
            // the thread index is hidden from the compiler here, so that a round's offsets are formed per tile from one
            // register: hoisted out of the tile loop, the twelve rounds' LDS and global offsets are forty registers and spill
            unsigned tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const unsigned o0 = 16u * tid, vbytes = 16u * nvec;
#pragma unroll
            for (int i0 = 0; i0 < MAXR; i0 += CH) {
                v4i t[CH];
#pragma unroll
                for (int i = i0; i < i0 + CH && i < MAXR; ++i) { // (read unconditionally, clamped into the tile: a round nobody stores, the twelfth at M = 257, costs one LDS read)
                    const unsigned o = o0 + 6144u * i;
                    t[i - i0] = *reinterpret_cast<const v4i *>(Yt + (o < 16u * nvec_full ? o : 16u * nvec_full - 16u));
                }
#pragma unroll
                for (int i = i0; i < i0 + CH && i < MAXR; ++i) {
                    const unsigned o = o0 + 6144u * i;
                    if (6144u * i + 1024u * wv < vbytes) { // wave-uniform: a round this wave has a vector in is one store instruction
                        if (o < vbytes) {
                            if constexpr (I16) *reinterpret_cast<v16y_2 *>(yt + o) = t[i - i0];
                            else *reinterpret_cast<v16y_4 *>(yt + o) = t[i - i0];
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (left < FT) {
                // the tensor's last tile: the remainder behind its whole vectors, one element per thread
                if (threadIdx.x < (nbytes & 15u) / YB) {
                    const unsigned o = 16u * nvec + YB * threadIdx.x;
                    if constexpr (I16) *reinterpret_cast<int16_t *>(yt + o) = *reinterpret_cast<const int16_t *>(Yt + o);
                    else *reinterpret_cast<int32_t *>(yt + o) = *reinterpret_cast<const int32_t *>(Yt + o);
                }
                prologue_loads_done(); // nothing is left in flight on this path
            }
        }
    }
