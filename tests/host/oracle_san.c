/* oracle_san.c -- oracle/s5fxp_ref.c as a stand-alone program, for a build with -fsanitize=address,undefined
 * (oracle/Makefile, target asan-exe).  Test infrastructure only.
 *
 *   oracle_san <model+input file> <output file>
 *
 * Both files are flat arrays of little-endian int32, written and read by tests/test_host_sanitizers.py.  The input holds the
 * integer model field by field in the order of the structs oracle/cref.py marshals (the ones declared below, which mirror
 * oracle/s5fxp_ref.c), every array in front of the scalars that follow it in its struct:
 *   magic, n_layers, x_bits, x_exp, B, L
 *   dense  := K, M, w[K*M], has_bias, bias[M] if has_bias, w_exp, b_bits, b_exp, inp_bits, inp_exp, out_bits, out_exp
 *   enc    := dense
 *   layer  := has_scale, has_bias, minus_mean[H], invsq_var[H], scale[H] if has_scale, bias[H] if has_bias, 8 scalars of the
 *             BatchNorm; H, P, a_re[P], a_im[P], b_re[P*H], b_im[P*H], c_re[H*P], c_im[H*P], d[H], 17 scalars of the SSM;
 *             out2 := dense; l_bits .. sig_y_exp (8 scalars); lut[8]
 *   dec    := dense
 *   x[B*L*d_in]
 * The output: rc, y_bits, y_exp, y[B*L*d_out], then per layer the eleven trace planes in the order of ref_layer_trace
 * ((B*L,H) each, the four state planes (B*L,P)), pre_s5_exp, residadd_exp.
 * Every array is a malloc of exactly its size, so a read or write one element too far is a report.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t K, M;
    const int32_t *w;
    const int32_t *bias;
    int32_t w_exp, b_bits, b_exp, inp_bits, inp_exp, out_bits, out_exp;
} ref_dense;

typedef struct {
    int32_t H, P;
    const int32_t *a_re, *a_im;
    const int32_t *b_re, *b_im;
    const int32_t *c_re, *c_im;
    const int32_t *d;
    int32_t a_re_exp, a_im_exp, b_re_exp, b_im_exp, c_re_exp, c_im_exp, d_exp;
    int32_t u_bits, u_exp, bu_re_bits, bu_re_exp, bu_im_bits, bu_im_exp;
    int32_t x_re_exp, x_im_exp, y_bits, y_exp;
} ref_ssm;

typedef struct {
    const int32_t *minus_mean, *invsq_var, *scale, *bias;
    int32_t mean_bits, mean_exp, isv_bits, isv_exp, scale_bits, scale_exp, bias_bits, bias_exp;
} ref_bn;

typedef struct {
    ref_bn bn;
    ref_ssm ssm;
    ref_dense out2;
    int32_t l_bits, l_exp, r_bits, r_exp, res_bits, res_exp;
    int32_t sig_x_exp, sig_y_exp;
    int32_t lut[8];
} ref_layer;

typedef struct {
    int32_t n_layers;
    ref_dense enc;
    const ref_layer *layers;
    ref_dense dec;
} ref_model;

typedef struct {
    int32_t *pre_s5, *u, *bu_re, *bu_im, *xs_re, *xs_im, *ys, *out2, *sigmoid, *post_glu, *residadd;
    int32_t pre_s5_exp, residadd_exp;
} ref_layer_trace;

int ref_forward(const ref_model *m, const int32_t *x, int x_bits, int x_exp, int B, int L, int32_t *y, int *y_bits,
                int *y_exp, ref_layer_trace *traces, int nthreads);

#define MAGIC 0x53354f52 /* "S5OR" */
#define MAX_ALLOCS 4096

static FILE *in;
static void *allocs[MAX_ALLOCS];
static int n_allocs;

static void die(const char *what)
{
    fprintf(stderr, "oracle_san: %s\n", what);
    exit(2);
}

static void *keep(void *p)
{
    if (!p || n_allocs == MAX_ALLOCS) die("out of memory");
    allocs[n_allocs++] = p;
    return p;
}

static int32_t scalar(void)
{
    int32_t v;
    if (fread(&v, sizeof v, 1, in) != 1) die("input file too short");
    return v;
}

static void scalars(int32_t *first, int n)
{
    for (int i = 0; i < n; ++i) first[i] = scalar();
}

static int32_t *array(size_t n)
{
    int32_t *p = keep(malloc(n ? n * sizeof(int32_t) : 1));
    if (n && fread(p, sizeof(int32_t), n, in) != n) die("input file too short");
    return p;
}

static void dense(ref_dense *d)
{
    d->K = scalar();
    d->M = scalar();
    if (d->K < 1 || d->M < 1) die("bad dense shape");
    d->w = array((size_t)d->K * (size_t)d->M);
    d->bias = scalar() ? array((size_t)d->M) : NULL;
    scalars(&d->w_exp, 7);
}

static void put(FILE *out, const void *p, size_t n)
{
    if (n && fwrite(p, sizeof(int32_t), n, out) != n) die("cannot write the output file");
}

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: oracle_san <input> <output>");
    in = fopen(argv[1], "rb");
    if (!in) die("cannot open the input file");
    if (scalar() != MAGIC) die("not an oracle_san input file");
    ref_model m;
    memset(&m, 0, sizeof m);
    m.n_layers = scalar();
    const int x_bits = scalar(), x_exp = scalar(), B = scalar(), L = scalar();
    if (m.n_layers < 0 || m.n_layers > 64 || B < 1 || L < 1) die("bad header");
    dense(&m.enc);
    const size_t H = (size_t)m.enc.M;
    ref_layer *layers = keep(calloc(m.n_layers ? (size_t)m.n_layers : 1, sizeof(ref_layer)));
    m.layers = layers;
    for (int i = 0; i < m.n_layers; ++i) {
        ref_layer *l = &layers[i];
        const int has_scale = scalar(), has_bias = scalar();
        l->bn.minus_mean = array(H);
        l->bn.invsq_var = array(H);
        l->bn.scale = has_scale ? array(H) : NULL;
        l->bn.bias = has_bias ? array(H) : NULL;
        scalars(&l->bn.mean_bits, 8);
        l->ssm.H = scalar();
        l->ssm.P = scalar();
        if ((size_t)l->ssm.H != H || l->ssm.P < 1) die("bad SSM shape");
        const size_t P = (size_t)l->ssm.P;
        l->ssm.a_re = array(P);
        l->ssm.a_im = array(P);
        l->ssm.b_re = array(P * H);
        l->ssm.b_im = array(P * H);
        l->ssm.c_re = array(H * P);
        l->ssm.c_im = array(H * P);
        l->ssm.d = array(H);
        scalars(&l->ssm.a_re_exp, 17);
        dense(&l->out2);
        scalars(&l->l_bits, 8);
        scalars(l->lut, 8);
    }
    dense(&m.dec);
    const size_t N = (size_t)B * (size_t)L;
    const int32_t *x = array(N * (size_t)m.enc.K);
    if (fgetc(in) != EOF) die("input file too long");
    fclose(in);

    int32_t *y = keep(malloc(N * (size_t)m.dec.M * sizeof(int32_t)));
    ref_layer_trace *tr = keep(calloc(m.n_layers ? (size_t)m.n_layers : 1, sizeof(ref_layer_trace)));
    for (int i = 0; i < m.n_layers; ++i) {
        const size_t nh = N * H * sizeof(int32_t), np = N * (size_t)layers[i].ssm.P * sizeof(int32_t);
        tr[i].pre_s5 = keep(malloc(nh)); tr[i].u = keep(malloc(nh));
        tr[i].bu_re = keep(malloc(np)); tr[i].bu_im = keep(malloc(np));
        tr[i].xs_re = keep(malloc(np)); tr[i].xs_im = keep(malloc(np));
        tr[i].ys = keep(malloc(nh)); tr[i].out2 = keep(malloc(nh)); tr[i].sigmoid = keep(malloc(nh));
        tr[i].post_glu = keep(malloc(nh)); tr[i].residadd = keep(malloc(nh));
    }
    int y_bits = 0, y_exp = 0;
    fprintf(stderr, "case forward n_layers=%d H=%zu B=%d L=%d\n", m.n_layers, H, B, L);
    const int32_t rc = ref_forward(&m, x, x_bits, x_exp, B, L, y, &y_bits, &y_exp, tr, 0);
    fprintf(stderr, "forward rc=%d y_bits=%d y_exp=%d\n", rc, y_bits, y_exp);

    FILE *out = fopen(argv[2], "wb");
    if (!out) die("cannot open the output file");
    const int32_t head[3] = {rc, y_bits, y_exp};
    put(out, head, 3);
    if (rc == 0) {
        put(out, y, N * (size_t)m.dec.M);
        for (int i = 0; i < m.n_layers; ++i) {
            const size_t nh = N * H, np = N * (size_t)layers[i].ssm.P;
            put(out, tr[i].pre_s5, nh); put(out, tr[i].u, nh);
            put(out, tr[i].bu_re, np); put(out, tr[i].bu_im, np); put(out, tr[i].xs_re, np); put(out, tr[i].xs_im, np);
            put(out, tr[i].ys, nh); put(out, tr[i].out2, nh); put(out, tr[i].sigmoid, nh);
            put(out, tr[i].post_glu, nh); put(out, tr[i].residadd, nh);
            put(out, &tr[i].pre_s5_exp, 1); put(out, &tr[i].residadd_exp, 1);
        }
    }
    if (fclose(out)) die("cannot write the output file");
    while (n_allocs) free(allocs[--n_allocs]);
    return rc == 0 ? 0 : 1;
}
