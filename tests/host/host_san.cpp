// host_san.cpp -- a stand-alone driver of the library's HOST paths, for a build of sparsernns_amd/csrc/s5fxp_api.hip whose host
// half is compiled with -fsanitize=address,undefined (tests/test_host_sanitizers.py builds and runs it).
//
// It calls what needs no device: descriptor validation, the size passes and the packers behind s5fxp_model_create /
// s5fxp_float_model_pack, the size queries, s5fxp_push_desc_check, the validation loop of s5fxp_stage_err and the argument
// checks of every launching entry.  Nothing here gets past an entry's argument checks to a launch.  "Device" pointers are a
// made-up address that is not device memory, so the program must never meet a device: its first act is hipGetDeviceCount, and
// with a device present it leaves with status 77 before it calls anything else (--expect-device inverts that test, to show
// that the guard leaves before the first case).
//
//   host_san [--expect-device] [--out DIR]
//
// Every case prints "case <name>" to stderr before it runs (stderr is unbuffered: a sanitizer that ends the process loses
// nothing), every return code that is not the expected one prints "FAIL ...", and the exit status is 0 only without any.
// With --out, DIR/float_desc.bin receives the arrays of one small float model (int32 n_layers, d_in, H, P, d_out, has_scale,
// has_bias, then float32 enc_w, enc_b, per layer mean, var, [scale], [bias], lambda_bar, B_bar, C, D, w2, b2, then dec_w,
// dec_b) and DIR/float_blob.bin the blob s5fxp_float_model_pack made of them.
#include "../../include/s5fxp.h"

#include <hip/hip_runtime_api.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

int g_fail = 0;

void begin(const char *name) { std::fprintf(stderr, "case %s\n", name); }

#define EXPECT(expr, want)                                                                                              \
    do {                                                                                                                \
        const long long got_ = (long long)(expr), want_ = (long long)(want);                                            \
        if (got_ != want_) {                                                                                            \
            std::fprintf(stderr, "FAIL %s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #expr, got_, want_);     \
            ++g_fail;                                                                                                   \
        }                                                                                                               \
    } while (0)

// an address that is neither host nor device memory: whatever dereferences it on the host is a report
template <class T> T *fake() { return reinterpret_cast<T *>(uintptr_t(1) << 20); }

struct Lcg {
    uint32_t s;
    uint32_t next()
    {
        s = s * 1664525u + 1013904223u;
        return s >> 8;
    }
    int32_t range(int32_t lo, int32_t hi) { return lo + (int32_t)(next() % (uint32_t)(hi - lo + 1)); }
    float unit() { return (float)(next() & 0xffff) / 65536.0f - 0.5f; }
};

// ------------------------------------------------------------------------------------------------------------------------
// integer models
// ------------------------------------------------------------------------------------------------------------------------
struct Spec {
    int d_in = 257, H = 96, P = 64, d_out = 257, n_layers = 3, wbits = 8;
    bool scale = false, bias = false, rails = false;
    int live = -1; // states whose rows of B_bar are not all zero (-1: all P)
};

struct IntModel {
    std::vector<std::unique_ptr<int32_t[]>> store; // every array is its own allocation of exactly its size
    std::vector<s5fxp_layer_desc> layers;
    s5fxp_model_desc desc{};
    Lcg g{12345u};

    int32_t *arr(size_t n, int32_t lo, int32_t hi)
    {
        store.emplace_back(new int32_t[n]);
        int32_t *p = store.back().get();
        for (size_t i = 0; i < n; ++i) p[i] = g.range(lo, hi);
        return p;
    }
    s5fxp_dense_desc dense(int K, int M, int wmax, int inp_exp, bool rails)
    {
        s5fxp_dense_desc d{};
        d.K = K; d.M = M;
        d.weight = arr((size_t)K * M, -wmax - 1, wmax);
        int32_t *b = arr((size_t)M, -2000, 2000);
        if (rails) b[0] = 32767, b[M - 1] = -32768;
        d.bias = b;
        d.w_bits = wmax == 127 ? 8 : 4; d.w_exp = 6; d.b_bits = 16; d.b_exp = 10; d.inp_bits = 16; d.inp_exp = inp_exp;
        d.out_bits = 16; d.out_exp = 10;
        return d;
    }
    explicit IntModel(const Spec &sp)
    {
        const int H = sp.H, P = sp.P, wmax = sp.wbits == 8 ? 127 : 7;
        layers.resize((size_t)sp.n_layers);
        for (s5fxp_layer_desc &l : layers) {
            l = s5fxp_layer_desc{};
            l.norm.minus_mean = arr(H, -3000, 3000);
            l.norm.invsq_var = arr(H, 1, 30000);
            l.norm.scale = sp.scale ? arr(H, -20000, 20000) : nullptr;
            l.norm.bias = sp.bias ? arr(H, -20000, 20000) : nullptr;
            l.norm.mean_bits = 16; l.norm.mean_exp = 10; l.norm.invsq_var_bits = 16; l.norm.invsq_var_exp = 8;
            l.norm.scale_bits = 16; l.norm.scale_exp = 12; l.norm.bias_bits = 16; l.norm.bias_exp = 12;
            s5fxp_ssm_desc &s = l.ssm;
            s.H = H; s.P = P;
            int32_t *are = arr(P, -16384, 16383), *aim = arr(P, -16384, 16383);
            int32_t *bre = arr((size_t)P * H, -wmax - 1, wmax), *bim = arr((size_t)P * H, -wmax - 1, wmax);
            s.C_re = arr((size_t)H * P, -wmax - 1, wmax); s.C_im = arr((size_t)H * P, -wmax - 1, wmax);
            int32_t *D = arr(H, -30000, 30000);
            for (int q = 0; q < P; ++q) {
                const bool live = sp.live < 0 || q < sp.live;
                if (live) bre[(size_t)q * H] = 1; // a live state has a non-zero row whatever the generator gave
                else
                    for (int h = 0; h < H; ++h) bre[(size_t)q * H + h] = bim[(size_t)q * H + h] = 0;
            }
            if (sp.rails) {
                are[0] = 32767; aim[0] = -32768; are[P - 1] = -32768; aim[P - 1] = 32767;
                D[0] = 32767; D[H - 1] = -32768;
            }
            s.A_re = are; s.A_im = aim; s.B_re = bre; s.B_im = bim; s.D = D;
            s.A_re_bits = 16; s.A_re_exp = 14; s.A_im_bits = 16; s.A_im_exp = 14;
            s.B_re_bits = sp.wbits; s.B_re_exp = 6; s.B_im_bits = sp.wbits; s.B_im_exp = 6;
            s.C_re_bits = sp.wbits; s.C_re_exp = 6; s.C_im_bits = sp.wbits; s.C_im_exp = 6;
            s.D_bits = 16; s.D_exp = 6; s.u_bits = 16; s.u_exp = 10;
            s.Bu_re_bits = 16; s.Bu_re_exp = 12; s.Bu_im_bits = 16; s.Bu_im_exp = 12;
            s.x_re_bits = 24; s.x_re_exp = 12; s.x_im_bits = 24; s.x_im_exp = 12; s.y_bits = 16; s.y_exp = 10;
            l.out2 = dense(H, H, wmax, 10, sp.rails);
            l.l_bits = 16; l.l_exp = 10; l.r_bits = 16; l.r_exp = 14; l.res_bits = 16; l.res_exp = 10;
            l.sig_x_exp = 6; l.sig_y_exp = 14;
            for (int i = 0; i < 8; ++i) l.lut[i] = sp.rails && i == 7 ? 65535 : 1000 * i;
        }
        desc.n_layers = sp.n_layers;
        desc.encoder = dense(sp.d_in, H, wmax, 15, sp.rails);
        desc.layers = sp.n_layers ? layers.data() : nullptr;
        desc.decoder = dense(H, sp.d_out, wmax, 10, sp.rails);
    }
};

// size pass, then creation against an address that is no device memory: without a device the copy fails, and the handle, the
// staging buffer and the fused path's host structures must all be gone when the entry returns
void create_cases(const char *name, const Spec &sp)
{
    begin(name);
    IntModel m(sp);
    const size_t need = s5fxp_model_blob_bytes(&m.desc);
    EXPECT(need > 0, 1);
    EXPECT(need % 256, 0);
    for (int flags : {(int)S5FXP_MODEL_DEFAULT, (int)S5FXP_MODEL_FORCE_GENERIC}) {
        s5fxp_model *h = fake<s5fxp_model>();
        EXPECT(s5fxp_model_create(&m.desc, fake<void>(), need, flags, nullptr, &h), S5FXP_EHIP);
        EXPECT(h == nullptr, 1);
    }
    s5fxp_model *h = fake<s5fxp_model>();
    EXPECT(s5fxp_model_create(&m.desc, fake<void>(), need - 1, 0, nullptr, &h), S5FXP_EWORKSPACE);
    EXPECT(h == nullptr, 1);
}

void int_model_creation()
{
    const int recipe[4][2] = {{48, 32}, {96, 64}, {144, 96}, {192, 128}};
    for (const auto &hp : recipe) {
        Spec sp;
        sp.H = hp[0]; sp.P = hp[1];
        create_cases(("create_recipe_H" + std::to_string(sp.H)).c_str(), sp);
    }
    { Spec sp; sp.d_out = 272; create_cases("create_257x272", sp); }
    { Spec sp; sp.d_in = 20; sp.H = 40; sp.P = 24; sp.d_out = 9; sp.n_layers = 2; create_cases("create_generic_small", sp); }
    { Spec sp; sp.n_layers = 0; create_cases("create_no_layers", sp); }
    { Spec sp; sp.scale = true; create_cases("create_bn_scale", sp); }
    { Spec sp; sp.bias = true; create_cases("create_bn_bias", sp); }
    { Spec sp; sp.scale = sp.bias = true; create_cases("create_bn_scale_bias", sp); }
    for (int live : {0, 1, 32, 33, 64}) {
        Spec sp;
        sp.live = live;
        create_cases(("create_live_" + std::to_string(live) + "_of_64").c_str(), sp);
    }
    for (int live : {0, 1, 32, 33, 64, 65, 128}) {
        Spec sp;
        sp.H = 192; sp.P = 128; sp.live = live;
        create_cases(("create_live_" + std::to_string(live) + "_of_128").c_str(), sp);
    }
    { Spec sp; sp.wbits = 4; create_cases("create_w4", sp); }
    { Spec sp; sp.rails = true; create_cases("create_rails", sp); }
    { Spec sp; sp.rails = true; sp.H = 192; sp.P = 128; sp.live = 33; create_cases("create_rails_compact", sp); }

    begin("create_arguments");
    Spec sp;
    sp.H = 48; sp.P = 32; sp.n_layers = 1;
    IntModel m(sp);
    const size_t need = s5fxp_model_blob_bytes(&m.desc);
    s5fxp_model *h = fake<s5fxp_model>();
    EXPECT(s5fxp_model_create(&m.desc, fake<void>(), need, 0, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_create(&m.desc, nullptr, need, 0, nullptr, &h), S5FXP_EBADARG);
    EXPECT(s5fxp_model_create(&m.desc, fake<void>(), need, S5FXP_MODEL_FORCE_CSR, nullptr, &h), S5FXP_EUNSUPPORTED);
    EXPECT(h == nullptr, 1);
    s5fxp_model_destroy(nullptr);
}

// one bad descriptor per early return of validate(): the size query answers 0, creation the documented code and a null handle
struct Refusals {
    IntModel base;
    Refusals() : base([] { Spec sp; sp.H = 48; sp.P = 32; sp.n_layers = 2; return sp; }()) {}

    template <class Mutate> void one(const char *name, int code, Mutate mutate)
    {
        begin(name);
        std::vector<s5fxp_layer_desc> layers = base.layers;
        s5fxp_model_desc d = base.desc;
        d.layers = layers.data();
        mutate(d, layers[1]);
        EXPECT(s5fxp_model_blob_bytes(&d), 0);
        s5fxp_model *h = fake<s5fxp_model>();
        EXPECT(s5fxp_model_create(&d, fake<void>(), size_t(1) << 30, 0, nullptr, &h), code);
        EXPECT(h == nullptr, 1);
    }
};

void validate_refusals()
{
    Refusals r;
    using MD = s5fxp_model_desc;
    using LD = s5fxp_layer_desc;
    begin("validate_null_desc");
    EXPECT(s5fxp_model_blob_bytes(nullptr), 0);
    {
        s5fxp_model *h = fake<s5fxp_model>();
        EXPECT(s5fxp_model_create(nullptr, fake<void>(), 1 << 20, 0, nullptr, &h), S5FXP_EBADARG);
        EXPECT(h == nullptr, 1);
    }
    r.one("validate_negative_layers", S5FXP_EBADARG, [](MD &d, LD &) { d.n_layers = -1; });
    r.one("validate_null_layers", S5FXP_EBADARG, [](MD &d, LD &) { d.layers = nullptr; });
    r.one("validate_encoder_weight", S5FXP_EBADARG, [](MD &d, LD &) { d.encoder.weight = nullptr; });
    r.one("validate_encoder_bias", S5FXP_EBADARG, [](MD &d, LD &) { d.encoder.bias = nullptr; });
    r.one("validate_encoder_K", S5FXP_EBADARG, [](MD &d, LD &) { d.encoder.K = 0; });
    r.one("validate_encoder_M", S5FXP_EBADARG, [](MD &d, LD &) { d.encoder.M = 0; });
    r.one("validate_decoder_weight", S5FXP_EBADARG, [](MD &d, LD &) { d.decoder.weight = nullptr; });
    r.one("validate_decoder_bias", S5FXP_EBADARG, [](MD &d, LD &) { d.decoder.bias = nullptr; });
    r.one("validate_decoder_K_zero", S5FXP_EBADARG, [](MD &d, LD &) { d.decoder.K = 0; });
    r.one("validate_decoder_M", S5FXP_EBADARG, [](MD &d, LD &) { d.decoder.M = -3; });
    r.one("validate_decoder_K_not_H", S5FXP_EBADARG, [](MD &d, LD &) { d.decoder.K = 47; });
    r.one("validate_mw_H", S5FXP_EUNSUPPORTED, [](MD &d, LD &) { d.encoder.M = d.decoder.K = 193; });
    r.one("validate_mw_d_out", S5FXP_EUNSUPPORTED, [](MD &d, LD &) { d.decoder.M = 273; });
    r.one("validate_status_words", S5FXP_EUNSUPPORTED, [](MD &d, LD &) { d.n_layers = 16; });
    r.one("validate_ssm_H", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.H = 47; });
    r.one("validate_ssm_P", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.P = 0; });
    r.one("validate_A_re", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.A_re = nullptr; });
    r.one("validate_A_im", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.A_im = nullptr; });
    r.one("validate_B_re", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.B_re = nullptr; });
    r.one("validate_B_im", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.B_im = nullptr; });
    r.one("validate_C_re", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.C_re = nullptr; });
    r.one("validate_C_im", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.C_im = nullptr; });
    r.one("validate_D", S5FXP_EBADARG, [](MD &, LD &l) { l.ssm.D = nullptr; });
    r.one("validate_minus_mean", S5FXP_EBADARG, [](MD &, LD &l) { l.norm.minus_mean = nullptr; });
    r.one("validate_invsq_var", S5FXP_EBADARG, [](MD &, LD &l) { l.norm.invsq_var = nullptr; });
    r.one("validate_out2_weight", S5FXP_EBADARG, [](MD &, LD &l) { l.out2.weight = nullptr; });
    r.one("validate_out2_bias", S5FXP_EBADARG, [](MD &, LD &l) { l.out2.bias = nullptr; });
    r.one("validate_out2_K", S5FXP_EBADARG, [](MD &, LD &l) { l.out2.K = 47; });
    r.one("validate_out2_M", S5FXP_EBADARG, [](MD &, LD &l) { l.out2.M = 49; });
    r.one("validate_mw_2P", S5FXP_EUNSUPPORTED, [](MD &, LD &l) { l.ssm.P = 137; });
    // the eight static shifts, each negative on its own, and the two ends of the range
    r.one("validate_shift_Bu_re", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.Bu_re_exp = l.ssm.u_exp + l.ssm.B_re_exp + 1; });
    r.one("validate_shift_Bu_im", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.Bu_im_exp = l.ssm.u_exp + l.ssm.B_im_exp + 1; });
    r.one("validate_shift_C_re", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.C_re_exp = l.ssm.y_exp - l.ssm.x_re_exp - 1; });
    r.one("validate_shift_C_im", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.C_im_exp = l.ssm.y_exp - l.ssm.x_im_exp - 1; });
    r.one("validate_shift_D", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.D_exp = l.ssm.y_exp - l.ssm.u_exp - 1; });
    r.one("validate_shift_gate", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.res_exp = l.l_exp + l.r_exp + 1; });
    r.one("validate_shift_A_re", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.A_re_exp = -1; });
    r.one("validate_shift_A_im", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.A_im_exp = -1; });
    r.one("validate_shift_A_re_32", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.A_re_exp = 32; });
    r.one("validate_shift_gate_32", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.res_exp = l.l_exp + l.r_exp - 32; });
    // |Bu_exp - x_exp| beyond 31, with the C shift kept legal
    r.one("validate_shift_x_re", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.x_re_exp = l.ssm.Bu_re_exp - 32; l.ssm.C_re_exp += 32; });
    r.one("validate_shift_x_im", S5FXP_ENEGSHIFT, [](MD &, LD &l) { l.ssm.x_im_exp = l.ssm.Bu_im_exp + 32; l.ssm.C_im_exp -= 32; });
    r.one("validate_sig_x_low", S5FXP_EUNSUPPORTED, [](MD &, LD &l) { l.sig_x_exp = -1; });
    r.one("validate_sig_x_high", S5FXP_EUNSUPPORTED, [](MD &, LD &l) { l.sig_x_exp = 16; });
    r.one("validate_sig_y_low", S5FXP_EUNSUPPORTED, [](MD &, LD &l) { l.sig_y_exp = 0; });
    r.one("validate_sig_y_high", S5FXP_EUNSUPPORTED, [](MD &, LD &l) { l.sig_y_exp = 31; });
}

// ------------------------------------------------------------------------------------------------------------------------
// the float model's packer
// ------------------------------------------------------------------------------------------------------------------------
struct FloatModel {
    std::vector<std::unique_ptr<float[]>> store;
    std::vector<size_t> sizes; // of store, in order
    std::vector<s5fxp_float_layer_desc> layers;
    s5fxp_float_model_desc desc{};
    bool scale, bias;
    Lcg g{777u};

    float *arr(size_t n, bool positive = false)
    {
        store.emplace_back(new float[n]);
        sizes.push_back(n);
        float *p = store.back().get();
        for (size_t i = 0; i < n; ++i) p[i] = positive ? g.unit() + 0.75f : g.unit();
        return p;
    }
    FloatModel(int DS, int n_layers, bool scale_, bool bias_) : scale(scale_), bias(bias_)
    {
        const size_t H = 48 * (size_t)DS, P = 32 * (size_t)DS;
        desc.n_layers = n_layers; desc.d_in = 257; desc.H = (int)H; desc.P = (int)P; desc.d_out = 257;
        desc.enc_w = arr(257 * H); desc.enc_b = arr(H);
        layers.resize((size_t)n_layers);
        for (s5fxp_float_layer_desc &l : layers) {
            l.mean = arr(H); l.var = arr(H, true);
            l.scale = scale ? arr(H) : nullptr; l.bias = bias ? arr(H) : nullptr;
            l.lambda_bar = arr(2 * P); l.B_bar = arr(P * H * 2); l.C = arr(H * P * 2); l.D = arr(H);
            l.w2 = arr(H * H); l.b2 = arr(H);
        }
        desc.layers = layers.data();
        desc.dec_w = arr(H * 257); desc.dec_b = arr(257);
    }
};

bool write_file(const std::string &path, const std::vector<std::pair<const void *, size_t>> &parts)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = true;
    for (const auto &p : parts) ok = ok && std::fwrite(p.first, 1, p.second, f) == p.second;
    return std::fclose(f) == 0 && ok;
}

void float_pack_valid(const char *name, const FloatModel &m, const std::string &out_dir)
{
    begin(name);
    const size_t need = s5fxp_float_model_blob_bytes(&m.desc);
    EXPECT(need > 0, 1);
    EXPECT(need % 256, 0);
    // exactly blob_bytes: a write one float too far lands in the red zone
    std::unique_ptr<char, void (*)(void *)> blob(static_cast<char *>(std::malloc(need)), std::free);
    std::memset(blob.get(), 0xa5, need);
    EXPECT(s5fxp_float_model_pack(&m.desc, blob.get(), need), S5FXP_OK);
    EXPECT(s5fxp_float_model_pack(&m.desc, blob.get(), need - 1), S5FXP_EWORKSPACE);
    EXPECT(s5fxp_float_model_pack(&m.desc, nullptr, need), S5FXP_EBADARG);
    s5fxp_float_model *h = fake<s5fxp_float_model>();
    EXPECT(s5fxp_float_model_create(&m.desc, fake<void>(), need, nullptr, &h), S5FXP_EHIP);
    EXPECT(h == nullptr, 1);
    h = fake<s5fxp_float_model>();
    EXPECT(s5fxp_float_model_create(&m.desc, fake<void>(), need - 1, nullptr, &h), S5FXP_EWORKSPACE);
    EXPECT(h == nullptr, 1);
    EXPECT(s5fxp_float_model_create(&m.desc, fake<void>(), need, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_float_model_create(&m.desc, nullptr, need, nullptr, &h), S5FXP_EBADARG);
    if (out_dir.empty()) return;
    const int32_t head[7] = {m.desc.n_layers, m.desc.d_in, m.desc.H, m.desc.P, m.desc.d_out, m.scale, m.bias};
    std::vector<std::pair<const void *, size_t>> parts{{head, sizeof(head)}};
    for (size_t i = 0; i < m.store.size(); ++i) parts.push_back({m.store[i].get(), m.sizes[i] * sizeof(float)});
    EXPECT(write_file(out_dir + "/float_desc.bin", parts), 1);
    EXPECT(write_file(out_dir + "/float_blob.bin", {{blob.get(), need}}), 1);
}

void float_refusals()
{
    FloatModel m(1, 2, true, true);
    using FD = s5fxp_float_model_desc;
    using FL = s5fxp_float_layer_desc;
    std::vector<char> blob(1 << 20);
    auto one = [&](const char *name, int code, auto mutate) {
        begin(name);
        std::vector<FL> layers = m.layers;
        FD d = m.desc;
        d.layers = layers.data();
        mutate(d, layers[1]);
        EXPECT(s5fxp_float_model_blob_bytes(&d), 0);
        EXPECT(s5fxp_float_model_pack(&d, blob.data(), blob.size()), code);
        s5fxp_float_model *h = fake<s5fxp_float_model>();
        EXPECT(s5fxp_float_model_create(&d, fake<void>(), blob.size(), nullptr, &h), code);
        EXPECT(h == nullptr, 1);
    };
    begin("float_validate_null_desc");
    EXPECT(s5fxp_float_model_blob_bytes(nullptr), 0);
    EXPECT(s5fxp_float_model_pack(nullptr, blob.data(), blob.size()), S5FXP_EBADARG);
    one("float_validate_no_layers", S5FXP_EBADARG, [](FD &d, FL &) { d.n_layers = 0; });
    one("float_validate_65_layers", S5FXP_EBADARG, [](FD &d, FL &) { d.n_layers = 65; });
    one("float_validate_null_layers", S5FXP_EBADARG, [](FD &d, FL &) { d.layers = nullptr; });
    one("float_validate_enc_w", S5FXP_EBADARG, [](FD &d, FL &) { d.enc_w = nullptr; });
    one("float_validate_enc_b", S5FXP_EBADARG, [](FD &d, FL &) { d.enc_b = nullptr; });
    one("float_validate_dec_w", S5FXP_EBADARG, [](FD &d, FL &) { d.dec_w = nullptr; });
    one("float_validate_dec_b", S5FXP_EBADARG, [](FD &d, FL &) { d.dec_b = nullptr; });
    one("float_validate_d_in_zero", S5FXP_EBADARG, [](FD &d, FL &) { d.d_in = 0; });
    one("float_validate_d_out_zero", S5FXP_EBADARG, [](FD &d, FL &) { d.d_out = 0; });
    one("float_validate_H_zero", S5FXP_EBADARG, [](FD &d, FL &) { d.H = 0; });
    one("float_validate_P_zero", S5FXP_EBADARG, [](FD &d, FL &) { d.P = -1; });
    one("float_validate_mean", S5FXP_EBADARG, [](FD &, FL &l) { l.mean = nullptr; });
    one("float_validate_var", S5FXP_EBADARG, [](FD &, FL &l) { l.var = nullptr; });
    one("float_validate_lambda_bar", S5FXP_EBADARG, [](FD &, FL &l) { l.lambda_bar = nullptr; });
    one("float_validate_B_bar", S5FXP_EBADARG, [](FD &, FL &l) { l.B_bar = nullptr; });
    one("float_validate_C", S5FXP_EBADARG, [](FD &, FL &l) { l.C = nullptr; });
    one("float_validate_D", S5FXP_EBADARG, [](FD &, FL &l) { l.D = nullptr; });
    one("float_validate_w2", S5FXP_EBADARG, [](FD &, FL &l) { l.w2 = nullptr; });
    one("float_validate_b2", S5FXP_EBADARG, [](FD &, FL &l) { l.b2 = nullptr; });
    one("float_validate_d_in_256", S5FXP_EUNSUPPORTED, [](FD &d, FL &) { d.d_in = 256; });
    one("float_validate_d_out_258", S5FXP_EUNSUPPORTED, [](FD &d, FL &) { d.d_out = 258; });
    one("float_validate_H_47", S5FXP_EUNSUPPORTED, [](FD &d, FL &) { d.H = 47; });
    one("float_validate_H_50", S5FXP_EUNSUPPORTED, [](FD &d, FL &) { d.H = 50; });
    one("float_validate_H_240", S5FXP_EUNSUPPORTED, [](FD &d, FL &) { d.H = 240; d.P = 160; });
    one("float_validate_P_64_at_H_48", S5FXP_EUNSUPPORTED, [](FD &d, FL &) { d.P = 64; });
}

void float_packing(const std::string &out_dir)
{
    float_pack_valid("float_pack_ds1_out", FloatModel(1, 1, true, false), out_dir);
    for (int ds = 1; ds <= 4; ++ds)
        float_pack_valid(("float_pack_ds" + std::to_string(ds)).c_str(), FloatModel(ds, 3, ds % 2 == 0, ds > 2), "");
    float_refusals();
}

// ------------------------------------------------------------------------------------------------------------------------
// entries that need no handle
// ------------------------------------------------------------------------------------------------------------------------
void handle_free_entries()
{
    const int64_t CLIP_T = ((int64_t(1) << 20) - 1) * 128; // the longest clip row the ragged audio entries take
    begin("stft_frames");
    EXPECT(s5fxp_stft_frames(511), -1);
    EXPECT(s5fxp_stft_frames(512), 5);
    EXPECT(s5fxp_stft_frames(513), 6);
    EXPECT(s5fxp_stft_frames(0), -1);
    EXPECT(s5fxp_stft_frames(-1), -1);
    EXPECT(s5fxp_stft_frames(INT64_MIN), -1);
    EXPECT(s5fxp_stft_frames(INT64_MAX), INT64_MAX / 128 + 2);
    EXPECT(s5fxp_stft_frames(INT64_MAX - 127), INT64_MAX / 128 + 1);

    begin("score_workspace_bytes");
    EXPECT(s5fxp_score_workspace_bytes(0, 512), 0);
    EXPECT(s5fxp_score_workspace_bytes(1, 511), 0);
    EXPECT(s5fxp_score_workspace_bytes(1, 512), 48);
    EXPECT(s5fxp_score_workspace_bytes(3, 512 + 13 * 128), 3 * 2 * 48);
    EXPECT(s5fxp_score_workspace_bytes(-1, 4096), 0);
    EXPECT(s5fxp_score_workspace_bytes(INT_MAX, 512), 48ll * INT_MAX);
    EXPECT(s5fxp_score_workspace_bytes(INT_MAX, 512 + 13 * 128), 0);   // a grid the entry refuses
    EXPECT(s5fxp_score_workspace_bytes(1, INT64_MAX), 0);
    EXPECT(s5fxp_score_workspace_bytes(INT_MAX, INT64_MAX), 0);
    EXPECT(s5fxp_score_workspace_bytes(INT_MIN, INT64_MIN), 0);

    begin("score_clips_workspace_bytes");
    EXPECT(s5fxp_score_clips_workspace_bytes(0, 512), 0);
    EXPECT(s5fxp_score_clips_workspace_bytes(1, 511), 0);
    EXPECT(s5fxp_score_clips_workspace_bytes(1, 512), 48);
    EXPECT(s5fxp_score_clips_workspace_bytes(5, 512 + 13 * 128), 5 * 2 * 48);
    EXPECT(s5fxp_score_clips_workspace_bytes(1, CLIP_T), 48ll * (((int64_t(1) << 20) - 1 + 12) / 13));
    EXPECT(s5fxp_score_clips_workspace_bytes(1, CLIP_T + 1), 0);
    EXPECT(s5fxp_score_clips_workspace_bytes(INT_MAX, CLIP_T), 48ll * INT_MAX * (((int64_t(1) << 20) - 1 + 12) / 13));
    EXPECT(s5fxp_score_clips_workspace_bytes(INT_MAX, INT64_MAX), 0);
    EXPECT(s5fxp_score_clips_workspace_bytes(INT_MIN, INT64_MIN), 0);

    begin("stage_err_workspace_bytes");
    EXPECT(s5fxp_stage_err_workspace_bytes(0), 0);
    EXPECT(s5fxp_stage_err_workspace_bytes(1), 256 + 512 * sizeof(s5fxp_stage_err_rec));
    EXPECT(s5fxp_stage_err_workspace_bytes(4096) >= 4096 * 4 * sizeof(s5fxp_stage_err_rec), 1);
    EXPECT(s5fxp_stage_err_workspace_bytes(4096) < (32u << 20), 1);
    EXPECT(s5fxp_stage_err_workspace_bytes(4097), 0);
    EXPECT(s5fxp_stage_err_workspace_bytes(-1), 0);
    EXPECT(s5fxp_stage_err_workspace_bytes(INT_MAX), 0);
    EXPECT(s5fxp_stage_err_workspace_bytes(INT_MIN), 0);

    begin("stream_frames_out_hops");
    EXPECT(s5fxp_stream_audio_state_bytes() > 0, 1);
    EXPECT(s5fxp_stream_audio_state_bytes() % 16, 0);
    EXPECT(s5fxp_stream_frames(0, 1), 0);
    EXPECT(s5fxp_stream_frames(0, 32), 31);
    EXPECT(s5fxp_stream_frames(1, 32), 32);
    EXPECT(s5fxp_stream_frames(-1, 1), -1);
    EXPECT(s5fxp_stream_frames(0, 0), -1);
    EXPECT(s5fxp_stream_frames(0, 33), -1);
    EXPECT(s5fxp_stream_frames(INT64_MAX, 32), 32);
    EXPECT(s5fxp_stream_frames(INT64_MIN, INT_MIN), -1);
    EXPECT(s5fxp_stream_frames(INT64_MAX, INT_MAX), -1);
    EXPECT(s5fxp_stream_out_hops(0, 1, 0), 0);
    EXPECT(s5fxp_stream_out_hops(0, 3, 0), 0);
    EXPECT(s5fxp_stream_out_hops(0, 4, 0), 1);
    EXPECT(s5fxp_stream_out_hops(2, 2, 0), 1);
    EXPECT(s5fxp_stream_out_hops(3, 2, 0), 2);
    EXPECT(s5fxp_stream_out_hops(4, 2, 1), 3);
    EXPECT(s5fxp_stream_out_hops(0, 32, 1), 30);
    EXPECT(s5fxp_stream_out_hops(-1, 1, 0), -1);
    EXPECT(s5fxp_stream_out_hops(0, 0, 0), -1);
    EXPECT(s5fxp_stream_out_hops(0, 33, 0), -1);
    EXPECT(s5fxp_stream_out_hops(INT64_MAX, 32, 1), 33);
    EXPECT(s5fxp_stream_out_hops(INT64_MAX, 1, 0), 1);
    EXPECT(s5fxp_stream_out_hops(INT64_MIN, INT_MAX, INT_MAX), -1);

    begin("strerror");
    const char *known[] = {"ok", "bad argument", "negative", "unsupported", "HIP", "workspace"};
    for (int code = 0; code >= -5; --code) {
        const char *s = s5fxp_strerror(code);
        EXPECT(s && std::strstr(s, known[-code]) != nullptr, 1);
    }
    for (int code : {1, 2, -6, -7, 100, INT_MAX, INT_MIN}) {
        const char *s = s5fxp_strerror(code);
        EXPECT(s && std::strcmp(s, "unknown error") == 0, 1);
    }
    EXPECT(s5fxp_version(), S5FXP_VERSION);
}

// ------------------------------------------------------------------------------------------------------------------------
// s5fxp_push_desc_check
// ------------------------------------------------------------------------------------------------------------------------
s5fxp_push_desc push(int slot, int rows, int flags, int hops, int h4)
{
    s5fxp_push_desc d{};
    d.slot = slot; d.rows = rows; d.flags = flags; d.hops = hops; d.h4 = h4;
    return d;
}

void push_desc_cases()
{
    begin("push_desc_valid");
    // exactly n entries on the heap: reading entry n is a report
    auto check = [](std::vector<s5fxp_push_desc> v, int n_slots, int Lmax, int cmax, int audio) {
        std::unique_ptr<s5fxp_push_desc[]> p(new s5fxp_push_desc[v.size()]);
        std::memcpy(p.get(), v.data(), v.size() * sizeof(s5fxp_push_desc));
        return s5fxp_push_desc_check(p.get(), (int)v.size(), n_slots, Lmax, cmax, audio);
    };
    EXPECT(check({push(2, 0, 0, 0, 0), push(0, 8, S5FXP_PUSH_FRESH, 0, 0), push(1, 1, 7, 99, 99)}, 3, 8, 0, 0), S5FXP_OK);
    EXPECT(check({push(0, 0, 0, 0, 0)}, 1, 0, -5, 0), S5FXP_OK);
    EXPECT(check({push(4095, 1, 0, 0, 0)}, 4096, INT_MAX, INT_MAX, 0), S5FXP_OK);
    EXPECT(check({push(0, 1, S5FXP_PUSH_FRESH, 2, 0), push(3, 4, S5FXP_PUSH_FINAL | S5FXP_PUSH_ZEROS, 4, 4), push(1, 2, 0, 2, 3),
                  push(2, 0, S5FXP_PUSH_FRESH, 1, 0)}, 4, 4, 4, 1), S5FXP_OK);
    EXPECT(check({push(0, 32, 0, 32, 1)}, 1, 32, 32, 1), S5FXP_OK);

    begin("push_desc_refusals");
    const s5fxp_push_desc ok = push(0, 1, 0, 0, 0);
    EXPECT(s5fxp_push_desc_check(nullptr, 1, 1, 1, 0, 0), S5FXP_EBADARG);
    EXPECT(s5fxp_push_desc_check(&ok, 0, 1, 1, 0, 0), S5FXP_EBADARG);
    EXPECT(s5fxp_push_desc_check(&ok, -1, 1, 1, 0, 0), S5FXP_EBADARG);
    EXPECT(s5fxp_push_desc_check(&ok, 1, 0, 1, 0, 0), S5FXP_EBADARG);
    EXPECT(s5fxp_push_desc_check(&ok, 1, 1, -1, 0, 0), S5FXP_EBADARG);
    EXPECT(s5fxp_push_desc_check(&ok, INT_MIN, INT_MIN, INT_MIN, INT_MIN, 1), S5FXP_EBADARG);
    EXPECT(check({push(1, 1, 0, 0, 0), push(1, 1, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);  // a repeated slot
    EXPECT(check({push(-1, 1, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    EXPECT(check({push(2, 1, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    EXPECT(check({push(INT_MAX, 1, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    EXPECT(check({push(INT_MIN, 1, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    EXPECT(check({push(0, -1, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    EXPECT(check({push(0, 5, 0, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);                         // rows > Lmax
    EXPECT(check({push(0, 1, 8, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);                         // unknown flags
    EXPECT(check({push(0, 1, -1, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    EXPECT(check({push(0, 1, INT_MIN, 0, 0)}, 2, 4, 0, 0), S5FXP_EBADARG);
    for (int k = 0; k < 3; ++k) {
        s5fxp_push_desc d = ok;
        d.reserved[k] = 1;
        EXPECT(check({d}, 2, 4, 0, 0), S5FXP_EBADARG);
    }
    // the audio rules: refused with audio = 1, not looked at with audio = 0
    struct { s5fxp_push_desc d; int cmax, code; } audio[] = {
        {push(0, 1, 0, 1, 1), 0, S5FXP_EBADARG},                  // cmax outside 1..32
        {push(0, 1, 0, 1, 1), 33, S5FXP_EBADARG},
        {push(0, 0, 0, 0, 1), 4, S5FXP_EBADARG},                  // hops outside 1..cmax
        {push(0, 4, 0, 5, 1), 4, S5FXP_EBADARG},
        {push(0, 1, 0, 1, -1), 4, S5FXP_EBADARG},                 // h4 outside 0..4
        {push(0, 1, 0, 1, 5), 4, S5FXP_EBADARG},
        {push(0, 2, S5FXP_PUSH_FRESH, 2, 1), 4, S5FXP_EBADARG},   // FRESH in the middle of a signal
        {push(0, 2, 0, 2, 0), 4, S5FXP_EBADARG},                  // rows != hops - (h4 == 0)
        {push(0, 1, 0, 2, 2), 4, S5FXP_EBADARG},
        {push(0, 2, S5FXP_PUSH_FINAL, 2, 3), 4, S5FXP_EUNSUPPORTED}, // the end of a signal below 512 samples
        {push(0, 1, S5FXP_PUSH_FINAL | S5FXP_PUSH_FRESH, 2, 0), 4, S5FXP_EUNSUPPORTED},
    };
    for (const auto &c : audio) {
        EXPECT(check({c.d}, 1, 4, c.cmax, 1), c.code);
        EXPECT(check({c.d}, 1, 4, c.cmax, 0), S5FXP_OK);
    }
    // a later bad entry decides over an earlier short final
    EXPECT(check({push(0, 2, S5FXP_PUSH_FINAL, 2, 3), push(1, 0, 0, 0, 0)}, 2, 4, 4, 1), S5FXP_EBADARG);
}

// ------------------------------------------------------------------------------------------------------------------------
// s5fxp_stage_err: everything it refuses before the copy
// ------------------------------------------------------------------------------------------------------------------------
s5fxp_stage_pair pair()
{
    s5fxp_stage_pair p{};
    p.a = fake<void>(); p.b = fake<float>(); p.a_kind = S5FXP_STAGE_I32; p.a_exp = 15; p.nb = 2; p.rows = 3; p.cols = 4;
    const int64_t st[3] = {12, 4, 1};
    for (int k = 0; k < 3; ++k) p.a_stride[k] = p.b_stride[k] = st[k];
    return p;
}

void stage_err_cases()
{
    begin("stage_err_refusals");
    const size_t need = s5fxp_stage_err_workspace_bytes(1);
    s5fxp_stage_err_rec *out = fake<s5fxp_stage_err_rec>();
    void *ws = fake<void>();
    auto call = [&](const s5fxp_stage_pair &p, size_t nbytes) {
        std::unique_ptr<s5fxp_stage_pair[]> one(new s5fxp_stage_pair[1]);
        one[0] = p;
        return s5fxp_stage_err(one.get(), 1, out, ws, nbytes, nullptr);
    };
    const s5fxp_stage_pair good = pair();
    EXPECT(s5fxp_stage_err(nullptr, 1, out, ws, need, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stage_err(&good, 1, nullptr, ws, need, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stage_err(&good, 1, out, nullptr, need, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stage_err(&good, 0, out, ws, need, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stage_err(&good, 4097, out, ws, need, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stage_err(&good, INT_MAX, out, ws, need, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stage_err(&good, INT_MIN, out, ws, need, nullptr), S5FXP_EBADARG);
    auto with = [&](auto mutate) { s5fxp_stage_pair p = good; mutate(p); return p; };
    using SP = s5fxp_stage_pair;
    EXPECT(call(with([](SP &p) { p.a_kind = 2; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.a_kind = -1; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.flags = 2; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.flags = -1; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.a_exp = -1; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.a_exp = 41; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.nb = -1; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.rows = -1; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.cols = INT_MIN; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.a = nullptr; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.b = nullptr; }), need), S5FXP_EBADARG);
    // the wrap rule, far beyond 64 bits, and just beyond it: 2^41 > 512 * (2^32 - 256)
    EXPECT(call(with([](SP &p) { p.nb = p.rows = p.cols = INT_MAX; }), need), S5FXP_EBADARG);
    EXPECT(call(with([](SP &p) { p.nb = 512; p.rows = INT_MAX; p.cols = 2; }), need), S5FXP_EBADARG);
    // everything legal, but no room: refused on the host as well
    EXPECT(call(good, need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.a_kind = S5FXP_STAGE_F32; p.a_exp = 99; }), need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.flags = S5FXP_STAGE_RELU_A; }), need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.a_exp = 0; }), need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.a_exp = 40; }), need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.rows = 0; p.a = nullptr; p.b = nullptr; }), need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.nb = 511; p.rows = INT_MAX; p.cols = 2; }), need - 1), S5FXP_EWORKSPACE);
    EXPECT(call(with([](SP &p) { p.a_stride[0] = INT64_MIN; p.b_stride[2] = INT64_MAX; }), 0), S5FXP_EWORKSPACE);

    begin("stage_err_4096_pairs");
    const int n = 4096;
    std::unique_ptr<s5fxp_stage_pair[]> many(new s5fxp_stage_pair[n]);
    for (int i = 0; i < n; ++i) {
        many[i] = good;
        many[i].nb = i % 7; many[i].a_exp = i % 41; many[i].a_kind = i % 2; many[i].flags = (i / 2) % 2;
    }
    const size_t need_n = s5fxp_stage_err_workspace_bytes(n);
    EXPECT(s5fxp_stage_err(many.get(), n, out, ws, need_n - 1, nullptr), S5FXP_EWORKSPACE);
    // with 4096 pairs a pair gets 4 workgroups at the most: 4 * (2^32 - 256) elements pass, one row more does not
    many[n - 1].nb = 4; many[n - 1].rows = 0xffffff00u / 256; many[n - 1].cols = 256;
    EXPECT(s5fxp_stage_err(many.get(), n, out, ws, need_n - 1, nullptr), S5FXP_EWORKSPACE);
    many[n - 1].rows += 1;
    EXPECT(s5fxp_stage_err(many.get(), n, out, ws, need_n, nullptr), S5FXP_EBADARG);
    many[n - 1] = good;
    many[n - 1].a_exp = 41;
    EXPECT(s5fxp_stage_err(many.get(), n, out, ws, need_n, nullptr), S5FXP_EBADARG);
}

// ------------------------------------------------------------------------------------------------------------------------
// one refused call, at least, of every launching entry
// ------------------------------------------------------------------------------------------------------------------------
void launching_entries()
{
    int32_t *I = fake<int32_t>();
    float *F = fake<float>();
    int16_t *H16 = fake<int16_t>();
    void *V = fake<void>();
    const int32_t lut[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    const int64_t CLIP_T = ((int64_t(1) << 20) - 1) * 128;

    begin("entries_ops");
    EXPECT(s5fxp_from_fp(nullptr, nullptr, 4, 16, 8, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_from_fp(F, I, 4, 33, 8, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_from_fp(F, I, 4, 16, 32, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_from_fp(F, I, 4, 16, 8, 3, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_from_fp(F, I, 0, 16, 8, 0, nullptr), S5FXP_OK);
    EXPECT(s5fxp_to_float(I, nullptr, 4, 8, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_to_float(I, F, -1, 8, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_to_float(I, F, 4, 32, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_change_cfg(I, I, 4, 16, 40, 16, 2, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_change_cfg(I, I, 4, 0, 4, 16, 2, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_change_cfg(nullptr, I, 4, 16, 4, 16, 2, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_dense(I, nullptr, I, I, 1, 8, 4, 3, 3, 16, 0, 16, 2, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_dense(I, I, nullptr, I, 1, 8, 4000, 3, 3, 0, 0, 16, 2, 0, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_dense(I, I, nullptr, I, 1, 8, 4, 3, 3, 0, 0, 16, 7, 0, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_dense(I, I, I, I, 1, 8, 4, 3, 3, 16, 40, 16, 2, 0, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_dense(I, I, I, I, 0, 8, 4, 3, 3, 16, 2, 16, 2, 0, nullptr), S5FXP_OK);
    EXPECT(s5fxp_dense_csr(I, I, nullptr, I, I, I, 1, 8, 4, 3, 3, 16, 0, 16, 2, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_dense_csr(I, I, I, I, I, I, 1, 577, 4, 3, 3, 16, 0, 16, 2, 0, nullptr), S5FXP_EUNSUPPORTED); // 575 still fits the LDS
    EXPECT(s5fxp_dense_csr(I, I, I, I, I, I, 1, 8, 4, 3, 3, 16, 0, 16, 7, 0, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_add(I, I, I, 6, 4, 16, 3, 16, 3, 16, 3, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_add(I, I, I, 8, 4, 16, 3, 16, 40, 16, 3, 0, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_add(I, I, nullptr, 8, 4, 16, 3, 16, 3, 16, 3, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mul(I, I, I, 1, 1, 3, 3, 16, 9, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_mul(I, I, I, 1, 0, 3, 3, 16, 2, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_add_cb(I, I, I, 8, 4, 16, 3, 16, 3, 16, nullptr, V, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_add_cb(I, I, I, 0, 4, 16, 3, 16, 3, 16, I, V, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mul_cb(I, I, I, 8, 4, 3, 3, 16, I, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mul_cb(I, I, I, 6, 4, 3, 3, 16, I, V, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_relu(nullptr, nullptr, I, nullptr, 4, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_relu(I, I, I, nullptr, 4, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_sigmoid(I, I, 4, 16, 8, 6, 14, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_sigmoid(I, I, 4, 16, 8, 16, 14, lut, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_sigmoid(I, I, 4, 16, 8, 6, 31, lut, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_sigmoid(I, I, 4, 16, 40, 6, 14, lut, nullptr), S5FXP_ENEGSHIFT);

    begin("entries_scans");
    EXPECT(s5fxp_scan(I, I, I, I, I, I, 2, 8, 0, 15, 15, 15, 15, 14, 14, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_scan(I, I, I, I, I, nullptr, 2, 8, 4, 15, 15, 15, 15, 14, 14, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_scan(I, I, I, I, I, I, 2, 8, 4, 32, 15, 15, 15, 14, 14, 0, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_scan(I, I, I, I, I, I, 2, 8, 4, 15, 15, 50, 15, 14, 14, 0, nullptr), S5FXP_ENEGSHIFT);
    EXPECT(s5fxp_scan(I, I, I, I, I, I, 0, 8, 4, 15, 15, 15, 15, 14, 14, 0, nullptr), S5FXP_OK);
    EXPECT(s5fxp_assoc_scan_c64(nullptr, F, F, nullptr, nullptr, 1, 8, 4, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_assoc_scan_c64(F, F, F, nullptr, nullptr, 1, 8, 0, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_assoc_scan_c64(F, F, F, nullptr, nullptr, -1, 8, 4, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_assoc_scan_c64(F, F, F, nullptr, nullptr, INT_MAX, 8, INT_MAX, 0, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, nullptr, nullptr, nullptr, nullptr, 1, 8, 4, 10, 10, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, F, nullptr, nullptr, nullptr, 0, 8, 4, 10, 10, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, F, nullptr, nullptr, nullptr, 1, 8, 4, -25, 10, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, F, nullptr, nullptr, nullptr, 1, 8, 4, 10, 41, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, F, nullptr, nullptr, nullptr, INT_MAX, 8, INT_MAX, 10, 10, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, F, nullptr, nullptr, nullptr, 1, INT_MAX, 64, 10, 10, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_fq_scan_c64(F, F, F, nullptr, nullptr, nullptr, 1, INT_MAX, INT_MAX, 10, 10, nullptr), S5FXP_EBADARG);

    begin("entries_audio");
    EXPECT(s5fxp_stft_mag(nullptr, 1, 4096, 0.f, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag(F, 0, 4096, 0.f, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag(F, 1, 511, 0.f, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_stft_mag(F, INT_MAX, INT64_MAX, 0.f, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_stft_mag(F, 1, INT64_MAX, 0.f, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft(F, nullptr, 1, 4096, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft(F, nullptr, 1, 100, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft(F, nullptr, INT_MAX, INT64_MAX, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_stft_mag_i16(F, 1, 4096, 0.f, 17, 8, H16, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_i16(F, 1, 4096, 0.f, 16, 32, H16, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_i16(F, 1, 4096, 0.f, 16, 8, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_i16(F, 1, 511, 0.f, 16, 8, H16, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_i16(F, H16, 32, 1, 4096, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_i16(F, H16, -1, 1, 4096, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_i16(F, H16, 8, 1, 511, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_stft_mag_clips(F, 1, 4096, nullptr, 0.f, F, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_clips(F, 0, 4096, I, 0.f, F, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_clips(F, 1, CLIP_T + 1, I, 0.f, F, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_clips(F, 1, INT64_MAX, I, 0.f, F, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stft_mag_clips(F, 1, 511, I, 0.f, F, nullptr, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_stft_mag_clips(F, INT_MAX, CLIP_T, I, 0.f, F, nullptr, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_clips(F, nullptr, 1, 4096, I, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_clips(F, nullptr, 1, 100, I, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_clips(F, nullptr, INT_MAX, CLIP_T, I, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    const size_t sw = s5fxp_score_workspace_bytes(2, 4096);
    EXPECT(s5fxp_mask_istft_score(F, nullptr, nullptr, 2, 4096, 1.f, F, F, V, sw, F, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score(F, F, nullptr, 2, 4096, 1.f, F, F, nullptr, sw, F, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score(F, F, nullptr, 2, 4096, 1.f, F, F, V, sw, nullptr, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score(F, F, nullptr, 2, 100, 1.f, F, F, V, sw, F, F, F, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_score(F, F, nullptr, 2, 4096, 1.f, F, F, V, sw - 1, F, F, F, nullptr), S5FXP_EWORKSPACE);
    EXPECT(s5fxp_mask_istft_score(F, F, nullptr, INT_MAX, INT64_MAX, 1.f, F, F, V, SIZE_MAX, F, F, F, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_score_i16(F, F, H16, 32, 2, 4096, 1.f, F, F, V, sw, F, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score_i16(F, F, H16, 8, 2, 4096, 1.f, F, F, V, sw - 1, F, F, F, nullptr), S5FXP_EWORKSPACE);
    const size_t cw = s5fxp_score_clips_workspace_bytes(3, 4096);
    EXPECT(s5fxp_mask_istft_score_clips(F, nullptr, nullptr, 3, 4096, I, 1.f, F, F, V, cw, F, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score_clips(F, F, nullptr, 3, 4096, nullptr, 1.f, F, F, V, cw, F, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score_clips(F, F, nullptr, 3, CLIP_T + 1, I, 1.f, F, F, V, cw, F, F, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_mask_istft_score_clips(F, F, nullptr, 3, 100, I, 1.f, F, F, V, cw, F, F, F, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_score_clips(F, F, nullptr, INT_MAX, CLIP_T, I, 1.f, F, F, V, SIZE_MAX, F, F, F, nullptr), S5FXP_EUNSUPPORTED);
    EXPECT(s5fxp_mask_istft_score_clips(F, F, nullptr, 3, 4096, I, 1.f, F, F, V, cw - 1, F, F, F, nullptr), S5FXP_EWORKSPACE);

    begin("entries_stream");
    EXPECT(s5fxp_stream_stft(F, 1, 4, 0, 0.f, nullptr, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft(F, 0, 4, 0, 0.f, V, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft(F, 1, 33, 0, 0.f, V, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft(F, 1, 4, -1, 0.f, V, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft(F, 1, 4, 0, 0.f, V, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft(F, 1, 4, 0, 0, nullptr, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft(F, 1, 0, 0, 0, V, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft(F, 1, 4, 0, 0, V, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft(F, 1, 4, INT64_MAX, 1, V, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft(F, 1, 2, 3, 1, V, F, nullptr, nullptr), S5FXP_EUNSUPPORTED);
    const s5fxp_push_desc *PD = fake<s5fxp_push_desc>();
    EXPECT(s5fxp_stream_stft_ragged(F, 1, 4, nullptr, 0.f, V, 1, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft_ragged(F, 1, 4, PD, 0.f, nullptr, 1, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft_ragged(F, 1, 4, PD, 0.f, V, 1, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft_ragged(F, 0, 4, PD, 0.f, V, 1, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft_ragged(F, 1, 4, PD, 0.f, V, 0, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_stft_ragged(F, 1, 33, PD, 0.f, V, 1, F, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft_ragged(F, 1, 4, nullptr, V, 1, F, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft_ragged(F, 1, 4, PD, V, 1, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_stream_mask_istft_ragged(F, 1, 0, PD, V, 1, F, nullptr, nullptr), S5FXP_EBADARG);

    begin("entries_step_clips");
    EXPECT(s5fxp_model_step_ok(nullptr, 1, 1), -1);
    EXPECT(s5fxp_model_step(nullptr, I, 16, 15, 1, 1, 1, I, nullptr, nullptr, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_step_f32(nullptr, F, 16, 15, 1, 1, 1, F, nullptr, nullptr, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_step_ragged(nullptr, I, 16, 15, 1, 1, 1, I, PD, I, 1, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_step_ragged(nullptr, I, 16, 15, 1, 1, 1, I, nullptr, I, 1, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_step_ragged_f32(nullptr, F, 16, 15, 1, 1, 1, F, PD, I, 0, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_clips_workspace_bytes(nullptr, 1, 1), 0);
    EXPECT(s5fxp_model_clips_ok(nullptr, 1), -1);
    EXPECT(s5fxp_model_clips(nullptr, I, 16, 15, 1, 8, I, I, nullptr, nullptr, V, 1 << 20, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_clips(nullptr, I, 16, 15, 1, 8, nullptr, I, nullptr, nullptr, V, 1 << 20, I, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_clips_f32(nullptr, F, 16, 15, 1, 0, I, F, nullptr, nullptr, V, 1 << 20, I, nullptr), S5FXP_EBADARG);

    begin("entries_forwards");
    EXPECT(s5fxp_workspace_bytes(nullptr, 1, 1), 0);
    EXPECT(s5fxp_workspace_bytes_f32(nullptr, 1, 1), 0);
    EXPECT(s5fxp_workspace_bytes_i16(nullptr, 1, 1), 0);
    EXPECT(s5fxp_model_forward(nullptr, I, 16, 15, 1, 8, I, V, 1 << 20, I, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_forward_f32(nullptr, F, 16, 15, 1, 8, F, V, 1 << 20, I, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_forward_i16(nullptr, H16, 16, 15, 1, 8, H16, V, 1 << 20, I, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_layer_forward(nullptr, 0, I, 16, 10, 1, 8, I, nullptr, V, 1 << 20, I, nullptr, nullptr, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_model_out_exp(nullptr), 0);
    EXPECT(s5fxp_model_out_bits(nullptr), 0);
    EXPECT(s5fxp_model_is_fast(nullptr), 0);
    EXPECT(s5fxp_model_recurrence_kernel(nullptr, 0), -1);
    EXPECT(s5fxp_model_recurrence_xmax(nullptr, 0), -1);
    EXPECT(s5fxp_model_live_states(nullptr, 0), -1);
    EXPECT(s5fxp_model_layer_out_bits(nullptr, 0), -1);
    EXPECT(s5fxp_float_workspace_bytes(nullptr, 1, 1, 0), 0);
    EXPECT(s5fxp_float_trace_bytes(nullptr, 1, 1), 0);
    unsigned long long *U = fake<unsigned long long>();
    const s5fxp_float_fq_site *Q = fake<s5fxp_float_fq_site>();
    EXPECT(s5fxp_float_model_forward(nullptr, F, 1, 8, F, nullptr, nullptr, V, 1 << 20, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_float_model_forward_hist(nullptr, F, 1, 8, F, nullptr, U, nullptr, V, 1 << 20, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_float_model_forward_fq(nullptr, F, 1, 8, F, nullptr, Q, nullptr, V, 1 << 20, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_float_model_clips(nullptr, F, 1, 8, I, F, nullptr, U, V, 1 << 20, nullptr), S5FXP_EBADARG);
    EXPECT(s5fxp_float_model_clips_fq(nullptr, F, 1, 8, I, F, nullptr, Q, V, 1 << 20, nullptr), S5FXP_EBADARG);
    s5fxp_float_model_destroy(nullptr);
}

} // namespace

int main(int argc, char **argv)
{
    bool expect_device = false;
    std::string out_dir;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--expect-device")) expect_device = true;
        else if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out_dir = argv[++i];
        else {
            std::fprintf(stderr, "usage: host_san [--expect-device] [--out DIR]\n");
            return 2;
        }
    }
    int n_dev = 0;
    const bool device = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
    if (device || expect_device) { // --expect-device: the guard believes in a device whatever the runtime said
        std::fprintf(stderr, "host_san: %s; leaving before the first call\n",
                     device ? "a device is visible" : "--expect-device was given");
        return 77;
    }
    int_model_creation();
    validate_refusals();
    float_packing(out_dir);
    handle_free_entries();
    push_desc_cases();
    stage_err_cases();
    launching_entries();
    std::fprintf(stderr, "host_san: %d unexpected return code%s\n", g_fail, g_fail == 1 ? "" : "s");
    return g_fail ? 1 : 0;
}
