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
            // these registers, a tile later, with vmcnt(0) -- behind the 48 stores of this tile's phase B
            raw[i] = gload16_hidden(reinterpret_cast<const char *>(a.x + tl * FT * H), 2u * (unsigned)(f * H + 8 * (v % VPF)));
        }
    };
    int64_t tile = blockIdx.x;
    if (tile < tiles) fetch(tile);
    prologue_loads_done();
    for (; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * FT;
        // the prefetched rows are older than the previous tile's 3 x 16 stores per wave (every tile but the tensor's last is
        // full and stores unconditionally; that last one has no successor)
        vm_wait<3 * 16>(raw);
        if (RESID && !(USUM && rz.usum)) vm_wait<3 * 16>(rawz);
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
        const int64_t nb = n0 + 32 * sub + 4 * h; // frame of accumulator register 0
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
            // Stores without control flow around them on full tiles (all but the tensor's last): lanes of the ragged last
            // column tile (col >= M) write to a sink word instead of being masked off.  Every conditional store would make
            // the number of memory operations in flight unknowable to the compiler's wait-count pass, and the wait it
            // then puts at the top of the next tile -- for the rows prefetched BEFORE these stores -- degenerates to
            // vmcnt(0): every tile would begin by waiting for the previous tile's stores to be acknowledged.
            const bool okc = col < a.M;
            char *ybase; // this tile's first output row
            if constexpr (I16) ybase = reinterpret_cast<char *>(reinterpret_cast<int16_t *>(a.y) + n0 * a.M);
            else ybase = reinterpret_cast<char *>(a.y + n0 * a.M);
            char *yl = okc ? ybase + YB * (unsigned)((32 * sub + 4 * h) * a.M + col)
                           : reinterpret_cast<char *>(as_global(&g_store_sink[l]));
            const unsigned ystep = okc ? YB * (unsigned)a.M : 0u;
            if (n0 + FT <= a.N) {
                char *yp = yl; // a running pointer: sixteen hoisted offsets per column tile would cost the kernel its occupancy
#pragma unroll
                for (int i = 0; i < 16; ++i) { // frames (i & 3) + 8 * (i >> 2)
                    const int32_t v = sat(asr(acc[i], rs), so);
                    if constexpr (F32) *reinterpret_cast<float *>(yp) = tofloat(sat(wadd(v, bev[c]), so), a.out_exp);
                    else if constexpr (I16) *reinterpret_cast<int16_t *>(yp) = (int16_t)sat(wadd(v, bev[c]), so);
                    else *reinterpret_cast<int32_t *>(yp) = sat(wadd(v, bev[c]), so);
                    yp += (i & 3) == 3 ? 5 * ystep : ystep;
                }
            } else {
                char *yp = yl;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int fo = (i & 3) + 8 * (i >> 2);
                    if (nb + fo < a.N) {
                        const int32_t v = sat(asr(acc[i], rs), so);
                        if constexpr (F32) *reinterpret_cast<float *>(yp) = tofloat(sat(wadd(v, bev[c]), so), a.out_exp);
                        else if constexpr (I16) *reinterpret_cast<int16_t *>(yp) = (int16_t)sat(wadd(v, bev[c]), so);
                        else *reinterpret_cast<int32_t *>(yp) = sat(wadd(v, bev[c]), so);
                    }
                    yp += (i & 3) == 3 ? 5 * ystep : ystep;
                }
                prologue_loads_done(); // the tensor's last tile: nothing is left in flight on this path
            }
            __builtin_amdgcn_sched_barrier(0); // one column tile at a time: interleaved, the three of a wave do not fit its registers
        }
        __syncthreads(); // planes are single-buffered
    }
