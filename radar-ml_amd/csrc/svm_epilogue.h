// The float64 epilogue arithmetic of every SVM decision kernel (128 x 128 tile, 256 x 256 ring, small-batch pair): the kernel
// value of one (support vector, sample) pair from their inner product, and the in-lane sums  S[p] += W[p][m] K  over support
// vectors.  Decision values do not depend on which kernel ran because all of them evaluate these functions, in the same order.
#pragma once
#include "rml_internal.h"
#include <math.h>

namespace {

// exp(x) for x <= 0 in float64, table-driven (Tang 1989): x = n L + r with L = ln2/64, n = 64 k + j, |r| <= L/2 = 0.0054,
//     exp(x) = 2^k * T[j] * (1 + p(r)),   p(r) = r + r^2 (1/2 + r (1/6 + r (1/24 + r (1/120 + r/720)))),   T[j] = 2^(j/64).
// Error: n L_hi is exact (L_hi carries 32 bits, |n| < 2^17), the reduction error is ~|n| ulp(L_lo) ~ 1e-22; the polynomial is
// truncated at r^7/5040 < 3e-20; T[j] is correctly rounded (0.5 ulp) and T + T p is one fma (0.5 ulp) on a p computed to
// ~1e-19 absolute: < 1.1 ulp in all, against ~1 ulp for the library routine it replaces (a degree-11 polynomial on |r| <= ln2/2
// plus range selects: ~35 instructions and a 20-deep dependent chain per kernel value, here 17 and 12).  Arguments below
// -1000 are clamped; v_ldexp_f64 then underflows to 0 like libm.  tab = the 64-entry table in LDS (exp_tab_init).
__constant__ double kExp2Tab[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0};
constexpr int kExpTabBytes = 64 * 8;

__device__ __forceinline__ void exp_tab_init(double* tab, int tid) {
    if (tid < 64) tab[tid] = kExp2Tab[tid];
}

__device__ __forceinline__ double rml_exp_neg(double x, const double* tab) {
    x = fmax(x, -1000.0);
    const double nf = rint(x * 0x1.71547652b82fep+6);              // x * 64/ln2
    double r = fma(nf, -0x1.62e42fee00000p-7, x);
    r = fma(nf, -0x1.a39ef35793c76p-39, r);
    const int n = (int)nf;
    const double T = tab[n & 63];
    double p = fma(r, 0x1.6c16c16c16c17p-10, 0x1.1111111111111p-7);   // 1/720, 1/120
    p = fma(r, p, 0x1.5555555555555p-5);                               // 1/24
    p = fma(r, p, 0x1.5555555555555p-3);                               // 1/6
    p = fma(r, p, 0.5);
    p = fma(r * r, p, r);
    return ldexp(fma(T, p, T), n >> 6);
}

// K(x, s) from the inner product term g, the sample term xt and the SV term e0 (what the three mean depends on the operand path:
// rml_svm_load).  RBF: d^2 = xt + e0 - 2 g, K = exp(-gs d^2).  Linear: on the exact path (EXACT) the biased-code identity
// K = (g + xt + e0) gs, otherwise the inner product itself.
template <bool EXACT>
__device__ __forceinline__ double kernel_value(bool rbf, double g, double xt, double e0, double gs, const double* etab) {
    if (rbf) {
        double d2 = xt + e0 - 2.0 * g;
        d2 = d2 > 0.0 ? d2 : 0.0;
        return rml_exp_neg(-gs * d2, etab);
    }
    return EXACT ? (g + xt + e0) * gs : g;
}

// the sample term of the exact path, from the row statistics of the codes:
// d^2 = (isq_x - 256 isum_x) + (isq_s - 256 isum_s + 32768 D) - 2 G'
__device__ __forceinline__ double exact_sample_term(bool rbf, const int32_t* isum, const int64_t* isq, int64_t n) {
    return rbf ? (double)(isq[n] - 256 * (int64_t)isum[n]) : 128.0 * (double)isum[n];
}

// per-SV epilogue table in LDS: [ROWS][1 + PT] float64 (SV term, then the pair weights W[p][m0 + row]), then the 2^(j/64) table
// of rml_exp_neg; returns that table.  GUARD: rows at or past Mpad are zeros (the ring kernel's last SV tile may be half a tile).
template <int PT, int ROWS, int THREADS, bool GUARD>
__device__ __forceinline__ const double* load_sv_table(double* svw, const double* sv_term, const double* W, int64_t Mpad, int64_t m0, int tid) {
    exp_tab_init(svw + ROWS * (1 + PT), tid);
    for (int idx = tid; idx < ROWS * (1 + PT); idx += THREADS) {
        int m = idx / (1 + PT), c = idx - m * (1 + PT);
        const bool in = !GUARD || m0 + m < Mpad;
        svw[idx] = !in ? 0.0 : ((c == 0) ? sv_term[m0 + m] : W[(int64_t)(c - 1) * Mpad + m0 + m]);
    }
    return svw + ROWS * (1 + PT);
}

// one link of the in-lane chain: S[p] = fma(W[p], kv, S[p]); w points at W[0], consecutive pairs are ws doubles apart
template <int PT>
__device__ __forceinline__ void chain_link(double (&S)[PT], const double* w, int ws, double kv) {
#pragma unroll
    for (int p = 0; p < PT; ++p) S[p] = fma(w[p * ws], kv, S[p]);
}

// The chain over the run of SV rows [ml0, ml0 + ROWS) of the table svw, in ascending order, from S = 0:  g_of(ml) is the inner
// product term of row ml and this thread's sample, seen(ml, kv) gets every kernel value (the kernel-matrix instantiations).
template <int PT, int ROWS, bool EXACT, class G, class Seen>
__device__ __forceinline__ void chain_run(double (&S)[PT], const double* svw, int ml0, bool rbf, double xt, double gs, const double* etab,
                                          G g_of, Seen seen) {
#pragma unroll
    for (int p = 0; p < PT; ++p) S[p] = 0.0;
#pragma unroll 2
    for (int mm = 0; mm < ROWS; ++mm) {
        const int ml = ml0 + mm;
        const double* e = svw + ml * (1 + PT);
        const double kv = kernel_value<EXACT>(rbf, g_of(ml), xt, e[0], gs, etab);
        seen(ml, kv);
        chain_link<PT>(S, e + 1, 1, kv);
    }
}

}  // namespace
