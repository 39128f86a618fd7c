/* C restatement of the reference mixing path -- TEST INFRASTRUCTURE ONLY.
 *
 * Restates utils/consensus_simple/mixer.py:43-49 (Mixer._mix_params_once) and
 * mixer.py:57-66 (_get_deviation_dict: np.mean over agents, then ||x_a - mean||) in plain C.
 * Built with -ffp-contract=off so every product and sum rounds separately, as numpy does;
 * tests/test_oracle_golden.py checks it bit-exact against the reference-generated fixtures.
 * Also the arithmetic contracts of the training-step entry points (ref_sgd_step, ref_bgemm),
 * with explicit fmaf where the device fuses; tests/test_bgemm_ref_cpu.py checks ref_bgemm.
 * Used by the tests as a fast checker at mid sizes and by bench.py as the timed CPU baseline
 * ("port", single thread).  Never linked into the product library.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* out[a, :] = sum_{e in row a} w[e] * x[col[e], :]  (left fold starting at +0.0).
 * Optional fused local step: x <- x - lr * g applied to every source row first
 * (g == NULL: plain mix).  Column-blocked so each source row block stays in cache. */
void ref_mix_round(const float *x, int64_t ldx, const float *g, int64_t ldg, float lr,
                   float *out, int64_t ldo, int32_t n_rows, int64_t n_params,
                   const int64_t *rowptr, const int64_t *col, const double *w,
                   float *scratch /* n_rows*block floats when g != NULL */, int64_t block) {
    for (int64_t p0 = 0; p0 < n_params; p0 += block) {
        int64_t pb = n_params - p0 < block ? n_params - p0 : block;
        const float *src = x + p0;
        int64_t lds = ldx;
        if (g) {
            for (int32_t r = 0; r < n_rows; ++r)
                for (int64_t p = 0; p < pb; ++p) {
                    float t = lr * g[r * ldg + p0 + p];
                    scratch[r * block + p] = x[r * ldx + p0 + p] - t;
                }
            src = scratch;
            lds = block;
        }
        for (int32_t a = 0; a < n_rows; ++a) {
            float *o = out + a * ldo + p0;
            for (int64_t p = 0; p < pb; ++p) o[p] = 0.0f;
            for (int64_t e = rowptr[a]; e < rowptr[a + 1]; ++e) {
                const float we = (float)w[e];
                const float *s = src + col[e] * lds;
                for (int64_t p = 0; p < pb; ++p) {
                    float prod = s[p] * we;
                    o[p] = o[p] + prod;
                }
            }
        }
    }
}

/* mean[p] = (sum_r x[r,p]) / n_rows, rows added in order from +0.0 (numpy add.reduce over axis 0:
 * a column of -0.0 sums to +0.0). */
void ref_column_mean(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params, float *mean) {
    for (int64_t p = 0; p < n_params; ++p) mean[p] = 0.0f + x[p];
    for (int32_t r = 1; r < n_rows; ++r)
        for (int64_t p = 0; p < n_params; ++p) mean[p] = mean[p] + x[r * ldx + p];
    const float n = (float)n_rows;
    for (int64_t p = 0; p < n_params; ++p) mean[p] = mean[p] / n;
}

/* dev_sq[a] = sum_p (x[a,p] - mean[p])^2, accumulated in double (the reference's fp32 BLAS
 * dot order is not reproducible; parity for this value is a tolerance, not bit-exact). */
void ref_deviation_sq(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params,
                      const float *mean, double *dev_sq) {
    for (int32_t a = 0; a < n_rows; ++a) {
        double s = 0.0;
        for (int64_t p = 0; p < n_params; ++p) {
            float d = x[a * ldx + p] - mean[p];
            s += (double)d * (double)d;
        }
        dev_sq[a] = s;
    }
}

/* torch.optim.SGD.step (torch/optim/sgd.py, single-tensor form) on an [n_rows, n_params] block,
 * restated with explicit fmaf for each of torch's add-with-alpha (ATen's add kernels compute
 * a + alpha*b as one fused multiply-add) -- the local step of config c5 (Man_Colab.ipynb cell 19).
 *   d = g + wd*x;  buf = first ? d : mu*buf + (1-damp)*d;  d = nesterov ? d + mu*buf : buf;
 *   out = x - lr*d      (buf may be NULL when mu == 0; out may alias x) */
void ref_sgd_step(const float *x, int64_t ldx, const float *g, int64_t ldg, float *buf,
                  int64_t ldb, float *out, int64_t ldo, int32_t n_rows, int64_t n_params,
                  float lr, float mu, float damp, float wd, int32_t nesterov, int32_t first) {
    for (int32_t r = 0; r < n_rows; ++r)
        for (int64_t p = 0; p < n_params; ++p) {
            const float xv = x[r * ldx + p];
            float d = g[r * ldg + p];
            if (wd != 0.0f) d = fmaf(wd, xv, d);
            if (mu != 0.0f) {
                float *b = buf + r * ldb + p;
                if (first) {
                    *b = d;
                } else {
                    const float m = mu * *b;
                    *b = fmaf(1.0f - damp, d, m);
                }
                d = nesterov ? fmaf(mu, *b, d) : *b;
            }
            out[r * ldo + p] = fmaf(-lr, d, xv);
        }
}

/* dl_bgemm (include/dlamd.h, "batched per-agent GEMMs") restated as the arithmetic the header
 * promises: per output element a k-ordered fp32 fma chain from +0.0,
 *   acc = 0;  for k in 0..K-1: acc = fmaf(opA[m][k], opB[k][n], acc)
 * with dl_bgemm_args' meaning of ta / tb / ld* / batch strides, then the epilogue (epi as enum
 * dl_epilogue), every operation rounded once:
 *   0 NONE acc;  1 BIAS acc + bias[n];  2 BIAS_RELU max(acc + bias[n], 0);
 *   5 DRELU acc * (h > 0 ? 1 : 0);  7 DELU acc * (h > 0 ? 1 : fl(h + 1));
 *   6 DTANH two candidates: C = acc * fl(1 - fl(h h)),  C2 = acc * fmaf(-h, h, 1) (a device
 *     compiler may contract 1 - h*h or not; C2 has C's layout and is required for epi 6);
 *   3 BIAS_TANH, 4 BIAS_ELU, 8 BIAS_XENT: C = the pre-activation z = acc + bias[n] only -- the
 *     transcendental part is the caller's, in float64 from this z.
 * bias == NULL adds nothing.  rowsum (nullable): s = 0; for k: s += opA[m][k], k in order.
 * Only the M x N (and M) logical elements are written. */
void ref_bgemm(int32_t batch, int32_t M, int32_t N, int32_t K, const float *A, int64_t lda,
               int64_t sA, int32_t ta, const float *B, int64_t ldb, int64_t sB, int32_t tb,
               float *C, int64_t ldc, int64_t sC, int32_t epi, const float *bias, int64_t s_bias,
               const float *H, int64_t ldh, int64_t sH, float *C2, float *rowsum,
               int64_t s_rowsum) {
    for (int32_t b = 0; b < batch; ++b) {
        const float *Ab = A + b * sA, *Bb = B + b * sB;
        const float *biasb = bias ? bias + b * s_bias : NULL;
        const float *Hb = H ? H + b * sH : NULL;
        for (int32_t m = 0; m < M; ++m) {
            const float *am = ta ? Ab + m : Ab + m * lda;
            const int64_t ak = ta ? lda : 1;
            if (rowsum) {
                float s = 0.0f;
                for (int32_t k = 0; k < K; ++k) s = s + am[k * ak];
                rowsum[b * s_rowsum + m] = s;
            }
            for (int32_t n = 0; n < N; ++n) {
                const float *bn = tb ? Bb + n * ldb : Bb + n;
                const int64_t bk = tb ? 1 : ldb;
                float acc = 0.0f;
                for (int32_t k = 0; k < K; ++k) acc = fmaf(am[k * ak], bn[k * bk], acc);
                float *c = C + b * sC + m * ldc + n;
                const int has_bias = biasb && (epi == 1 || epi == 2 || epi == 3 || epi == 4 ||
                                               epi == 8);
                float v = has_bias ? acc + biasb[n] : acc;
                if (epi == 2) v = v > 0.0f ? v : 0.0f;
                if (epi >= 5 && epi <= 7) {
                    const float h = Hb[m * ldh + n];
                    if (epi == 5) {
                        v = acc * (h > 0.0f ? 1.0f : 0.0f);
                    } else if (epi == 7) {
                        const float d = h > 0.0f ? 1.0f : h + 1.0f;
                        v = acc * d;
                    } else {
                        const float hh = h * h;
                        const float d = 1.0f - hh;
                        v = acc * d;
                        C2[b * sC + m * ldc + n] = acc * fmaf(-h, h, 1.0f);
                    }
                }
                *c = v;
            }
        }
    }
}
