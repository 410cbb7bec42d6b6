// What follows the GEMM: fixed-order sum of the partials with the libsvm / scikit-learn tail, Platt probabilities, and the
// linear classifier.
#pragma once
#include "rml_internal.h"
#include <math.h>

namespace {

// ---- finishing kernel: fixed-order sum of the SV-tile partials + libsvm/sklearn tail ------
struct FinishArgs {
    const double* partial; int64_t Npart; int ST, PT;
    int64_t N; int C, P;
    const double* intercept; const double* calib; int has_calib;
    const int32_t* row_flags; const int32_t* tile_exact;   // forced-i8 validity (rows with flag 0 -> NaN)
    int forced_i8;
    double* dec_ovo; double* dec_ovr; double* proba; int32_t* label_vote; int32_t* label_calib;
};

__device__ __forceinline__ double expit_d(double x) {
    if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
    double e = exp(x);
    return e / (1.0 + e);
}

// up to 6 classes (15 one-vs-one pairs): person / dog / cat plus the aliases of train.py:656-663 fit with room to spare
constexpr int kMaxC = 6, kMaxP = 15;

__global__ __launch_bounds__(256) void k_svm_finish(FinishArgs a) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    const int C = a.C, P = a.P;
    double dec[kMaxP];
    for (int p = 0; p < P; ++p) {
        double s = 0.0;
        for (int st = 0; st < a.ST; ++st) s += a.partial[((int64_t)st * a.Npart + n) * a.PT + p];
        dec[p] = s + a.intercept[p];           // sum -= rho[p]  (rho = -intercept_)
    }
    bool valid = true;
    if (a.forced_i8 && a.row_flags) valid = a.row_flags[n] != 0;
    if (!valid) for (int p = 0; p < P; ++p) dec[p] = NAN;
    if (a.dec_ovo) for (int p = 0; p < P; ++p) a.dec_ovo[n * P + p] = dec[p];

    // libsvm vote: dec > 0 -> ++vote[i] else ++vote[j]; first maximum wins (svm.cpp:2884-2894)
    int vote[kMaxC];
    for (int c = 0; c < C; ++c) vote[c] = 0;
    {
        int p = 0;
        for (int i = 0; i < C; ++i)
            for (int j = i + 1; j < C; ++j, ++p) { if (dec[p] > 0) ++vote[i]; else ++vote[j]; }
    }
    int best = 0;
    for (int c = 1; c < C; ++c) if (vote[c] > vote[best]) best = c;
    if (a.label_vote) a.label_vote[n] = valid ? best : -1;

    double T[kMaxC];
    if (C == 2) {
        // sklearn flips the sign for binary problems (sk:svm/_base.py:546-547): T = -dec
        T[0] = -dec[0];
        if (a.dec_ovr) a.dec_ovr[n] = T[0];
    } else {
        // _ovr_decision_function(dec < 0, -dec, C)
        double soc[kMaxC]; double vt[kMaxC];
        for (int c = 0; c < C; ++c) { soc[c] = 0.0; vt[c] = 0.0; }
        int p = 0;
        for (int i = 0; i < C; ++i)
            for (int j = i + 1; j < C; ++j, ++p) {
                double conf = -dec[p];
                soc[i] -= conf; soc[j] += conf;
                if (dec[p] < 0) vt[j] += 1.0; else vt[i] += 1.0;
            }
        for (int c = 0; c < C; ++c) T[c] = vt[c] + soc[c] / (3.0 * (fabs(soc[c]) + 1.0));
        if (!valid) for (int c = 0; c < C; ++c) T[c] = NAN;
        if (a.dec_ovr) for (int c = 0; c < C; ++c) a.dec_ovr[n * C + c] = T[c];
    }
    if (a.has_calib && (a.proba || a.label_calib)) {
        double pr[kMaxC];
        if (C == 2) {
            pr[1] = expit_d(-(a.calib[0] * T[0] + a.calib[C + 0]));
            pr[0] = 1.0 - pr[1];
        } else {
            double den = 0.0;
            for (int c = 0; c < C; ++c) { pr[c] = expit_d(-(a.calib[c] * T[c] + a.calib[C + c])); den += pr[c]; }
            for (int c = 0; c < C; ++c) pr[c] = (den != 0.0) ? pr[c] / den : 1.0 / C;
        }
        for (int c = 0; c < C; ++c) if (pr[c] > 1.0 && pr[c] <= 1.0 + 1e-5) pr[c] = 1.0;
        if (a.proba) for (int c = 0; c < C; ++c) a.proba[n * C + c] = valid ? pr[c] : NAN;
        int bc = 0;
        for (int c = 1; c < C; ++c) if (pr[c] > pr[bc]) bc = c;
        if (a.label_calib) a.label_calib[n] = valid ? bc : -1;
    }
}

// ---- libsvm probability estimates (SVC(probability=True).predict_proba) ---------------------------------
// sigmoid_predict + multiclass_probability (method 2 of Wu, Lin & Weng) of sk:svm/src/libsvm/svm.cpp:2032-2104,
// 2918-2952, one thread per sample, float64, same iteration order as the C loops.
__global__ __launch_bounds__(256) void k_pairwise_proba(const double* dec, int64_t N, int k, const double* probA, const double* probB,
                                                        double* proba) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int P = k * (k - 1) / 2;
    double r[kMaxC][kMaxC], Q[kMaxC][kMaxC], p[kMaxC], Qp[kMaxC];
    int q = 0;
    for (int i = 0; i < k; ++i)
        for (int j = i + 1; j < k; ++j, ++q) {
            const double f = dec[n * P + q] * probA[q] + probB[q];
            double s = f >= 0 ? exp(-f) / (1.0 + exp(-f)) : 1.0 / (1.0 + exp(f));
            s = fmin(fmax(s, 1e-7), 1.0 - 1e-7);
            r[i][j] = s; r[j][i] = 1.0 - s;
        }
    for (int t = 0; t < k; ++t) {
        p[t] = 1.0 / k;
        Q[t][t] = 0.0;
        for (int j = 0; j < t; ++j) { Q[t][t] += r[j][t] * r[j][t]; Q[t][j] = Q[j][t]; }
        for (int j = t + 1; j < k; ++j) { Q[t][t] += r[j][t] * r[j][t]; Q[t][j] = -r[j][t] * r[t][j]; }
    }
    const double eps = 0.005 / k;
    const int max_iter = k > 100 ? k : 100;
    for (int iter = 0; iter < max_iter; ++iter) {
        double pQp = 0.0;
        for (int t = 0; t < k; ++t) {
            Qp[t] = 0.0;
            for (int j = 0; j < k; ++j) Qp[t] += Q[t][j] * p[j];
            pQp += p[t] * Qp[t];
        }
        double max_error = 0.0;
        for (int t = 0; t < k; ++t) max_error = fmax(max_error, fabs(Qp[t] - pQp));
        if (max_error < eps) break;
        for (int t = 0; t < k; ++t) {
            const double diff = (-Qp[t] + pQp) / Q[t][t];
            p[t] += diff;
            pQp = (pQp + diff * (diff * Q[t][t] + 2 * Qp[t])) / (1 + diff) / (1 + diff);
            for (int j = 0; j < k; ++j) { Qp[j] = (Qp[j] + diff * Q[t][j]) / (1 + diff); p[j] /= (1 + diff); }
        }
    }
    for (int t = 0; t < k; ++t) proba[n * k + t] = p[t];
}

// ---- linear classifier: one wave per row, float64 accumulation ----------------------------
__global__ __launch_bounds__(256) void k_linear(const float* feat, int64_t ld, int64_t N, int64_t D, int C,
                                                const double* coef, const double* intercept, const double* calib, int has_calib,
                                                double* dec, double* proba, int32_t* label, int32_t* label_calib) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    double s[kMaxC];
    for (int c = 0; c < C; ++c) s[c] = 0.0;
    for (int64_t d = lane; d < D; d += 64) {
        double x = (double)feat[n * ld + d];
        for (int c = 0; c < C; ++c) s[c] = fma(x, coef[c * D + d], s[c]);
    }
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s[c] += __shfl_xor(s[c], off);
        s[c] += intercept[c];
    }
    if (lane != 0) return;
    if (C == 2) {
        // binary SGD: coef_ has one row (class 1 score)
        if (dec) dec[n] = s[0];
        if (label) label[n] = s[0] > 0 ? 1 : 0;
        if (has_calib) {
            double p1 = expit_d(-(calib[0] * s[0] + calib[C]));
            if (proba) { proba[n * 2] = 1.0 - p1; proba[n * 2 + 1] = p1; }
            if (label_calib) label_calib[n] = p1 > 1.0 - p1 ? 1 : 0;
        }
        return;
    }
    if (dec) for (int c = 0; c < C; ++c) dec[n * C + c] = s[c];
    int b = 0;
    for (int c = 1; c < C; ++c) if (s[c] > s[b]) b = c;
    if (label) label[n] = b;
    if (has_calib && (proba || label_calib)) {
        double pr[kMaxC]; double den = 0.0;
        for (int c = 0; c < C; ++c) { pr[c] = expit_d(-(calib[c] * s[c] + calib[C + c])); den += pr[c]; }
        for (int c = 0; c < C; ++c) pr[c] = (den != 0.0) ? pr[c] / den : 1.0 / C;
        for (int c = 0; c < C; ++c) if (pr[c] > 1.0 && pr[c] <= 1.0 + 1e-5) pr[c] = 1.0;
        if (proba) for (int c = 0; c < C; ++c) proba[n * C + c] = pr[c];
        int bc = 0;
        for (int c = 1; c < C; ++c) if (pr[c] > pr[bc]) bc = c;
        if (label_calib) label_calib[n] = bc;
    }
}

}  // namespace
