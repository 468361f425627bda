/* abi_layout.c -- include/s5fxp.h read by a C compiler (C11, -pedantic -Wall -Wextra -Werror), and nothing of the library.
 *
 * Prints, one item per line, what a C caller's compiler makes of the header:
 *   struct <name> <sizeof>
 *   field <struct> <field> <offsetof> <sizeof the field>      in declaration order
 *   enum <name> <value>                                        every enumerator
 *   macro <name> <value>                                       every numeric #define
 * tests/test_host_sanitizers.py compares the lines with the ctypes twins in sparsernns_amd/_lib.py.
 */
#include "../../include/s5fxp.h"

#include <stddef.h>
#include <stdio.h>

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("field %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))
#define E(name) printf("enum %s %lld\n", #name, (long long)(name))
#define M(name) printf("macro %s %lld\n", #name, (long long)(name))

int main(void)
{
    S(s5fxp_dense_desc);
    F(s5fxp_dense_desc, K); F(s5fxp_dense_desc, M); F(s5fxp_dense_desc, weight); F(s5fxp_dense_desc, bias);
    F(s5fxp_dense_desc, w_bits); F(s5fxp_dense_desc, w_exp); F(s5fxp_dense_desc, b_bits); F(s5fxp_dense_desc, b_exp);
    F(s5fxp_dense_desc, inp_bits); F(s5fxp_dense_desc, inp_exp); F(s5fxp_dense_desc, out_bits); F(s5fxp_dense_desc, out_exp);

    S(s5fxp_ssm_desc);
    F(s5fxp_ssm_desc, H); F(s5fxp_ssm_desc, P);
    F(s5fxp_ssm_desc, A_re); F(s5fxp_ssm_desc, A_im); F(s5fxp_ssm_desc, B_re); F(s5fxp_ssm_desc, B_im);
    F(s5fxp_ssm_desc, C_re); F(s5fxp_ssm_desc, C_im); F(s5fxp_ssm_desc, D);
    F(s5fxp_ssm_desc, A_re_bits); F(s5fxp_ssm_desc, A_re_exp); F(s5fxp_ssm_desc, A_im_bits); F(s5fxp_ssm_desc, A_im_exp);
    F(s5fxp_ssm_desc, B_re_bits); F(s5fxp_ssm_desc, B_re_exp); F(s5fxp_ssm_desc, B_im_bits); F(s5fxp_ssm_desc, B_im_exp);
    F(s5fxp_ssm_desc, C_re_bits); F(s5fxp_ssm_desc, C_re_exp); F(s5fxp_ssm_desc, C_im_bits); F(s5fxp_ssm_desc, C_im_exp);
    F(s5fxp_ssm_desc, D_bits); F(s5fxp_ssm_desc, D_exp);
    F(s5fxp_ssm_desc, u_bits); F(s5fxp_ssm_desc, u_exp);
    F(s5fxp_ssm_desc, Bu_re_bits); F(s5fxp_ssm_desc, Bu_re_exp); F(s5fxp_ssm_desc, Bu_im_bits); F(s5fxp_ssm_desc, Bu_im_exp);
    F(s5fxp_ssm_desc, x_re_bits); F(s5fxp_ssm_desc, x_re_exp); F(s5fxp_ssm_desc, x_im_bits); F(s5fxp_ssm_desc, x_im_exp);
    F(s5fxp_ssm_desc, y_bits); F(s5fxp_ssm_desc, y_exp);

    S(s5fxp_norm_desc);
    F(s5fxp_norm_desc, minus_mean); F(s5fxp_norm_desc, invsq_var); F(s5fxp_norm_desc, scale); F(s5fxp_norm_desc, bias);
    F(s5fxp_norm_desc, mean_bits); F(s5fxp_norm_desc, mean_exp); F(s5fxp_norm_desc, invsq_var_bits); F(s5fxp_norm_desc, invsq_var_exp);
    F(s5fxp_norm_desc, scale_bits); F(s5fxp_norm_desc, scale_exp); F(s5fxp_norm_desc, bias_bits); F(s5fxp_norm_desc, bias_exp);

    S(s5fxp_layer_desc);
    F(s5fxp_layer_desc, norm); F(s5fxp_layer_desc, ssm); F(s5fxp_layer_desc, out2);
    F(s5fxp_layer_desc, l_bits); F(s5fxp_layer_desc, l_exp); F(s5fxp_layer_desc, r_bits); F(s5fxp_layer_desc, r_exp);
    F(s5fxp_layer_desc, res_bits); F(s5fxp_layer_desc, res_exp); F(s5fxp_layer_desc, sig_x_exp); F(s5fxp_layer_desc, sig_y_exp);
    F(s5fxp_layer_desc, lut);

    S(s5fxp_model_desc);
    F(s5fxp_model_desc, n_layers); F(s5fxp_model_desc, encoder); F(s5fxp_model_desc, layers); F(s5fxp_model_desc, decoder);

    S(s5fxp_layer_trace);
    F(s5fxp_layer_trace, pre_s5); F(s5fxp_layer_trace, u); F(s5fxp_layer_trace, Bu_re); F(s5fxp_layer_trace, Bu_im);
    F(s5fxp_layer_trace, xs_re); F(s5fxp_layer_trace, xs_im); F(s5fxp_layer_trace, ys); F(s5fxp_layer_trace, out2);
    F(s5fxp_layer_trace, out2_sigmoid); F(s5fxp_layer_trace, post_GLU); F(s5fxp_layer_trace, residadd);

    S(s5fxp_forward_opts);
    F(s5fxp_forward_opts, allreduce); F(s5fxp_forward_opts, allreduce_ctx); F(s5fxp_forward_opts, scan_events);
    F(s5fxp_forward_opts, flags); F(s5fxp_forward_opts, state_in); F(s5fxp_forward_opts, state_out);
    F(s5fxp_forward_opts, groups); F(s5fxp_forward_opts, gate_events);

    S(s5fxp_push_desc);
    F(s5fxp_push_desc, slot); F(s5fxp_push_desc, rows); F(s5fxp_push_desc, flags); F(s5fxp_push_desc, hops);
    F(s5fxp_push_desc, h4); F(s5fxp_push_desc, reserved);

    S(s5fxp_float_layer_desc);
    F(s5fxp_float_layer_desc, mean); F(s5fxp_float_layer_desc, var); F(s5fxp_float_layer_desc, scale);
    F(s5fxp_float_layer_desc, bias); F(s5fxp_float_layer_desc, lambda_bar); F(s5fxp_float_layer_desc, B_bar);
    F(s5fxp_float_layer_desc, C); F(s5fxp_float_layer_desc, D); F(s5fxp_float_layer_desc, w2); F(s5fxp_float_layer_desc, b2);

    S(s5fxp_float_model_desc);
    F(s5fxp_float_model_desc, n_layers); F(s5fxp_float_model_desc, d_in); F(s5fxp_float_model_desc, H);
    F(s5fxp_float_model_desc, P); F(s5fxp_float_model_desc, d_out); F(s5fxp_float_model_desc, enc_w);
    F(s5fxp_float_model_desc, enc_b); F(s5fxp_float_model_desc, layers); F(s5fxp_float_model_desc, dec_w);
    F(s5fxp_float_model_desc, dec_b);

    S(s5fxp_float_fq_site);
    F(s5fxp_float_fq_site, bits); F(s5fxp_float_fq_site, exp); F(s5fxp_float_fq_site, mode); F(s5fxp_float_fq_site, saturate);

    S(s5fxp_stage_pair);
    F(s5fxp_stage_pair, a); F(s5fxp_stage_pair, a_kind); F(s5fxp_stage_pair, a_exp); F(s5fxp_stage_pair, b);
    F(s5fxp_stage_pair, a_stride); F(s5fxp_stage_pair, b_stride); F(s5fxp_stage_pair, nb); F(s5fxp_stage_pair, rows);
    F(s5fxp_stage_pair, cols); F(s5fxp_stage_pair, flags);

    S(s5fxp_stage_err_rec);
    F(s5fxp_stage_err_rec, n); F(s5fxp_stage_err_rec, n_nonfinite); F(s5fxp_stage_err_rec, n_equal);
    F(s5fxp_stage_err_rec, n_ref_nonzero); F(s5fxp_stage_err_rec, sum_abs); F(s5fxp_stage_err_rec, sum_sq);
    F(s5fxp_stage_err_rec, max_abs); F(s5fxp_stage_err_rec, sum_ref_sq); F(s5fxp_stage_err_rec, sum_rel);
    F(s5fxp_stage_err_rec, max_rel); F(s5fxp_stage_err_rec, hist_abs); F(s5fxp_stage_err_rec, hist_rel);

    E(S5FXP_OK); E(S5FXP_EBADARG); E(S5FXP_ENEGSHIFT); E(S5FXP_EUNSUPPORTED); E(S5FXP_EHIP); E(S5FXP_EWORKSPACE);
    E(S5FXP_FLOOR); E(S5FXP_CEIL); E(S5FXP_ROUND);
    E(S5FXP_PUSH_FRESH); E(S5FXP_PUSH_ZEROS); E(S5FXP_PUSH_FINAL);
    E(S5FXP_MODEL_DEFAULT); E(S5FXP_MODEL_FORCE_DENSE); E(S5FXP_MODEL_FORCE_CSR); E(S5FXP_MODEL_FORCE_GENERIC);
    E(S5FXP_MODEL_NO_RESID_FOLD); E(S5FXP_MODEL_NO_RESID_LAZY); E(S5FXP_MODEL_NO_GATE_EXT);
    E(S5FXP_PATH_GENERIC); E(S5FXP_PATH_FUSED); E(S5FXP_PATH_STEP); E(S5FXP_PATH_CLIP);
    E(S5FXP_ST_NEGSHIFT); E(S5FXP_ST_NEGEXP); E(S5FXP_ST_WIDE_STATE); E(S5FXP_ST_WIDE_INPUT); E(S5FXP_ST_REDO);
    E(S5FXP_FWD_DEFER_REDO); E(S5FXP_FWD_EXACT); E(S5FXP_FWD_NO_PAIR);
    E(S5FXP_FQ_FLOOR); E(S5FXP_FQ_NEAREST); E(S5FXP_FQ_STEP);
    E(S5FXP_STAGE_I32); E(S5FXP_STAGE_F32); E(S5FXP_STAGE_RELU_A);

    M(S5FXP_VERSION); M(S5FXP_STREAM_MAX_HOPS); M(S5FXP_STATUS_WORDS); M(S5FXP_STEP_MAX_ROWS);
    M(S5FXP_FLOAT_HIST_BINS); M(S5FXP_FLOAT_HIST_EMIN);
    return 0;
}
