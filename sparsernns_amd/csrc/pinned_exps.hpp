// pinned_exps.hpp -- stated exponents (the _at entries): what turns the five compute_best exponents
// of a layer into its LayerDyn.  Included by s5fxp_fast.hpp (the batch forward's head, k_clear2_at below) and by
// s5fxp_step.hpp (the step and clip kernels, which call the two functions per layer): one derivation for all of them.
#pragma once

namespace s5 {

// ---- stated exponents (the _at entries).  finalize_add_cb / finalize_mul_cb turn ONE float per op, the maximum
// of the result, into the result exponent eo; every shift follows from eo and the operands' exponents, and the widening of
// the operands never clips (add_cb_apply).  So an op run at a stated eo is the same statements with eo taken from the caller:
// the functions below are finalize_*_cb without the float, and without the flags -- s5fxp_model_exps_check has refused on
// the host every eo that is negative or makes a shift leave 0..31 (-31..31 for an add's post shift).
constexpr int PIN_MAX_LAYERS = 8; // the exponents travel as kernel arguments (160 bytes), as the trace pointers of the clips do

struct PinExps {
    int32_t e[5 * PIN_MAX_LAYERS]; // [layer][BN add(-mean), BN mul(invsq_var), BN mul(scale), BN add(bias), residual add]
};

__device__ __forceinline__ AddCb pinned_add_cb(int eo, int xe, int ye)
{
    AddCb p;
    p.eo = eo;
    const int ea = xe > ye ? xe : ye;
    p.shx = ea - xe;
    p.shy = ea - ye;
    p.post = eo - ea;
    return p;
}

// step_bn_exps at stated exponents: thread 0 fills s_d and the status words, one barrier publishes them (and the layer's
// s_lut / s_wide stores in front of the call).  A slot whose op the layer lacks is not read; its status word keeps its 0.
__device__ __forceinline__ void step_bn_pinned(const int32_t *pe, const BnArgs &bn, int he, LayerDyn &s_d, int32_t *st_exps)
{
    if (threadIdx.x == 0) {
        s_d.bn1 = pinned_add_cb(pe[0], he, bn.me);
        st_exps[0] = pe[0];
        s_d.e2 = pe[1];
        s_d.rs2 = pe[0] + bn.ie - pe[1];
        st_exps[1] = pe[1];
        int e = pe[1];
        if (bn.scale) {
            s_d.e3 = pe[2];
            s_d.rs3 = e + bn.se - pe[2];
            st_exps[2] = pe[2];
            e = pe[2];
        }
        if (bn.bias) {
            s_d.bn4 = pinned_add_cb(pe[3], e, bn.be);
            st_exps[3] = pe[3];
            e = pe[3];
        }
        s_d.bn_e = e;
    }
    __syncthreads();
}

// The head of a batch forward at stated exponents (s5fxp_model_forward_at, s5fxp_fast.hpp FusedForward::clear_status): k_clear2's
// work -- the status words with what the host knows, the per-layer device state zeroed -- and, in the same launch, EVERY layer's
// LayerDyn and exponent status words, by the two functions above.  One workgroup per group builds both blocks in LDS and
// stores each word once; the block of per-channel extremes behind the LayerDyn array is neither cleared nor read by a pinned
// forward.  After this launch no kernel of the forward derives, gathers or publishes an exponent.
struct PinHeadArgs {
    StatusInit si;
    PinExps pin;
    BnArgs bn[PIN_MAX_LAYERS];      // make_bn of every layer: the operands' static exponents and which stages exist
    int32_t res_exp[PIN_MAX_LAYERS]; // the gate output's exponent, the residual add's first operand
    int32_t enc_exp;                 // layer 0's input exponent
    int32_t n_layers;
};
constexpr int PIN_STATUS_WORDS = 128; // S5FXP_STATUS_WORDS (include/s5fxp.h); the launcher asserts it
__global__ __launch_bounds__(256) void k_clear2_at(int32_t *status, LayerDyn *dyn, PinHeadArgs a, GroupOff go)
{
    gshift(status, (int64_t)blockIdx.y * go.status);
    gshift(dyn, (int64_t)blockIdx.y * go.ws);
    __shared__ int32_t s_st[PIN_STATUS_WORDS];
    __shared__ LayerDyn s_d[PIN_MAX_LAYERS];
    constexpr int DW = (int)(sizeof(LayerDyn) / 4);
    for (int i = threadIdx.x; i < PIN_STATUS_WORDS; i += 256) {
        int32_t v = 0; // as k_clear2
        if (i == 2) v = a.si.path;
        else if (i >= 8 && (i & 7) == 5 && (i - 8) / 8 < a.n_layers) v = a.si.rk[(i - 8) / 8];
        else if (i >= 8 && (i & 7) == 6 && (i - 8) / 8 < a.n_layers) v = a.si.slots[(i - 8) / 8];
        else if (i >= 8 && (i & 7) == 7 && (i - 8) / 8 < a.n_layers) v = a.si.stream[(i - 8) / 8];
        s_st[i] = v;
    }
    for (int i = threadIdx.x; i < PIN_MAX_LAYERS * DW; i += 256) reinterpret_cast<int32_t *>(s_d)[i] = 0;
    __syncthreads();
    int he = a.enc_exp;
    for (int li = 0; li < a.n_layers; ++li) {
        const int32_t *pe = a.pin.e + 5 * li;
        step_bn_pinned(pe, a.bn[li], he, s_d[li], s_st + 8 + 8 * li);
        if (threadIdx.x == 0) {
            s_d[li].res = pinned_add_cb(pe[4], a.res_exp[li], he);
            s_st[8 + 8 * li + 4] = pe[4];
        }
        he = pe[4];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PIN_STATUS_WORDS; i += 256) status[i] = s_st[i];
    for (int i = threadIdx.x; i < a.n_layers * DW; i += 256) reinterpret_cast<int32_t *>(dyn)[i] = reinterpret_cast<const int32_t *>(s_d)[i];
}

} // namespace s5
