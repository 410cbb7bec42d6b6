// Binary logistic-regression fits of SGDClassifier solved on the device, one workgroup per fit (rml_sgd_solve), the held-out
// rows scored from the solutions (rml_sgd_score), and a chain of partial_fit calls of one estimator with the weights resident for
// all its steps (rml_sgd_online).
//
// Reference arithmetic replaced (sk: = scikit-learn 1.7.2, the reference's dependency):
//   sk:linear_model/_sgd_fast.pyx.tp:275-603    _plain_sgd64 (the epoch loop, the 'optimal' schedule, the stopping rule)
//   sk:linear_model/_sgd_fast.pyx.tp:631-659    l1penalty64 (cumulative-penalty truncation, u and q)
//   sk:utils/_weight_vector.pyx.tp:77-201       WeightVector64: add, add_average, dot, scale, reset_wscale
//   sk:utils/_seq_dataset.pyx.tp:137-145        SequentialDataset64.shuffle (Fisher-Yates on a persisting index array)
//   sk:utils/_random.pxd:20-34                  our_rand_r (xorshift 13 / 17 / 5, taken mod 2^31)
//   sk:_loss/_loss.pyx.tp:256-266, 686-725      log1pexp, closs_half_binomial, cgradient_half_binomial (labels 0 / 1)
// called once per candidate, fold and class by the GridSearchCV(SGDClassifier(loss='log')) of train.py:350-381, and once per
// class by every partial_fit of train.py:432.
//
// Everything outside the dot product w . x is element-wise or scalar and keeps scikit-learn's expressions and their order,
// WITHOUT contraction (the pragma below).  The D-term dot product is summed in an order of this file's own:
//
//   ownership   thread t (0 .. 1023) owns the elements t, t + 1024, t + 2048, .. below D
//   thread sum  s = 0; for its elements in ascending order: s += w[e] * (double)x[e]      (product rounded, then added)
//   wave sum    the 64 lanes of a wave (threads 64 v .. 64 v + 63) butterfly: for m = 32, 16, 8, 4, 2, 1: s += s of lane ^ m
//               (every lane ends with the same bits: each level adds the same two values in either order)
//   block sum   the 16 wave sums added in wave order: ((S0 + S1) + S2) + .. + S15
//
// then p = sum * wscale + intercept as in WeightVector.dot.  The order does not depend on the variant, on the problem's place in
// the batch or on the batch: a result is a function of its problem alone, and bit-reproducible.  tests/sgd_common.py restates it
// in NumPy (dot order 'kernel').
//
// k_sgd<EPT, ..> with EPT = 1, 2, 4, 10 keeps the state (w, and q / the averaged weights where the problem has them) in
// registers, EPT elements per thread, and the current and next row beside it: D up to 10 240.  k_sgd<0, ..> is the same code
// with the state in a slice of the context's workspace and the row re-read from memory, for any D (RML_OPT_SGD_RESIDENT_D).
// k_sgd_online<EPT, ..> runs the same epoch (sgd_epoch) once per partial_fit step of train.py:409-438.
#include "rml_internal.h"
#include <math.h>
#include <string.h>
#include <algorithm>

// scikit-learn's binary has no fused multiply-add; a*b+c must stay two roundings in every expression of this file
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = RML_SGD_MAX_ROWS;          // the permutation of a problem's rows lives in LDS
constexpr int kMaxClasses = 8;
constexpr double kMaxDloss = 1e12;                  // sk:_sgd_fast.pyx.tp:427

// sk:utils/_random.pxd:20-34
__host__ __device__ inline uint32_t our_rand_r(uint32_t* seed) {
    if (*seed == 0) *seed = 1;
    *seed ^= (uint32_t)(*seed << 13);
    *seed ^= (uint32_t)(*seed >> 17);
    *seed ^= (uint32_t)(*seed << 5);
    return *seed % ((uint32_t)2147483647 + 1);
}

// sk:utils/_seq_dataset.pyx.tp:137-145
__host__ __device__ inline void fisher_yates(uint32_t seed, int n, int32_t* ind) {
    for (unsigned i = 0; i + 1 < (unsigned)n; ++i) {
        const unsigned j = i + our_rand_r(&seed) % ((unsigned)n - i);
        const int32_t a = ind[i]; ind[i] = ind[j]; ind[j] = a;
    }
}

// sk:_loss/_loss.pyx.tp:256-266
__device__ inline double log1pexp(double x) {
    if (x <= -37) return exp(x);
    if (x <= -2) return log1p(exp(x));
    if (x <= 18) return log(1. + exp(x));
    if (x <= 33.3) return x + exp(-x);
    return x;
}
// sk:_loss/_loss.pyx.tp:686-725
__device__ inline double half_binomial_loss(double y, double p) { return log1pexp(p) - y * p; }
__device__ inline double half_binomial_grad(double y, double p) {
    if (p > -37) {
        const double e = exp(-p);
        return ((1 - y) - y * e) / (1 + e);
    }
    return exp(p) - y;
}

struct SgdDev {                                     // one problem, device form
    const int32_t* rows;                            // n row indices into X
    const int32_t* y;                               // n labels, 0 / 1
    double* coef;                                   // D
    double* avg_coef;                               // D
    double* ws;                                     // state of the workspace variant: w, q, aw (D each)
    double alpha, l1_ratio, tol, weight_pos, weight_neg, t0, optimal_init;
    int64_t out;                                    // slot of the scalar outputs
    int32_t n, penalty, average, max_iter, n_iter_no_change, shuffle, warm;
    uint32_t seed;
};

// the elements a thread owns: registers (EPT > 0) or a strided slice of the workspace (EPT == 0)
template <int EPT>
struct Own {
    double v[EPT];
    __device__ inline void bind(double*, int) {}
    __device__ inline double get(int k) const { return v[k]; }
    __device__ inline void set(int k, double x) { v[k] = x; }
};
template <>
struct Own<0> {
    double* p;
    __device__ inline void bind(double* base, int tid) { p = base + tid; }
    __device__ inline double get(int k) const { return p[(size_t)k * kThreads]; }
    __device__ inline void set(int k, double x) { p[(size_t)k * kThreads] = x; }
};
template <int EPT>
struct Row {                                        // the row of the step: registers, or read where it is used
    float v[EPT];
};
template <>
struct Row<0> {};

// the block sum of the header: butterfly, 16 wave sums through slot `buf` of the double-buffered LDS scratch, one barrier
__device__ inline double block_sum(double s, double (*red)[kWaves], int& buf, int lane, int wave) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) red[buf][wave] = s;
    __syncthreads();
    double tot = red[buf][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) tot += red[buf][w];
    buf ^= 1;
    return tot;
}

// what _plain_sgd64 carries from sample to sample; k_sgd and k_sgd_online run the same epoch on it
template <int EPT>
struct SgdState {
    Own<EPT> w, q, aw;
    double intercept, avg_intercept, wscale, average_a, average_b, u, t;
};

// WeightVector.reset_wscale (sk:_weight_vector.pyx.tp:191-201)
template <int EPT, bool AVG>
__device__ __forceinline__ void sgd_reset_wscale(SgdState<EPT>& S, int nk, int tid, int64_t D) {
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        if (tid + (int64_t)k * kThreads < D) {
            if (AVG) {
                double a = S.aw.get(k);
                a += S.average_a * S.w.get(k);
                a *= 1.0 / S.average_b;
                S.aw.set(k, a);
            }
            S.w.set(k, S.w.get(k) * S.wscale);
        }
    }
    if (AVG) { S.average_a = 0.0; S.average_b = 1.0; }
    S.wscale = 1.0;
}

template <int EPT>
__device__ __forceinline__ void sgd_load_row(Row<EPT>& r, const float* __restrict__ X, int64_t row, int64_t ld, int64_t D, int tid) {
    if constexpr (EPT > 0) {
        const float* __restrict__ xr = X + row * ld;
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int64_t e = tid + (int64_t)k * kThreads;
            r.v[k] = e < D ? xr[e] : 0.0f;
        }
    }
}

// One epoch of _plain_sgd64 (sk:_sgd_fast.pyx.tp:470-552) over the n rows rows[perm[0]], rows[perm[1]], ..; returns the epoch's summed
// loss.  The label of a row is lab[.] itself (pos < 0: 0 / 1), or lab[.] == pos (class indices, the problem of class pos).
template <int EPT, bool L1, bool AVG>
__device__ __forceinline__ double sgd_epoch(SgdState<EPT>& S, const SgdDev& P, const int32_t* __restrict__ rows,
                                            const int32_t* __restrict__ lab, int pos_class, int n, const int32_t* perm,
                                            const float* __restrict__ X, int64_t D, int64_t ld, int nk, double l1_ratio,
                                            double (*red)[kWaves], int& buf, int tid, int lane, int wave) {
    const double alpha = P.alpha, optimal_init = P.optimal_init, average = (double)P.average;
    double sumloss = 0;
    Row<EPT> xn;
    sgd_load_row(xn, X, rows[perm[0]], ld, D, tid);
    for (int i = 0; i < n; ++i) {
        const int pos = perm[i];
        const double y = pos_class < 0 ? (double)lab[pos] : (lab[pos] == pos_class ? 1.0 : 0.0);
        const float* __restrict__ xrow = X + (int64_t)rows[pos] * ld;
        Row<EPT> x = xn;
        if (i + 1 < n) sgd_load_row(xn, X, rows[perm[i + 1]], ld, D, tid);     // the next row travels while this one is reduced
        auto xval = [&](int k, int64_t e) -> double {
            if constexpr (EPT > 0) return (double)x.v[k]; else return (double)xrow[e];
        };

        // p = w.dot(x) + intercept, in the order of the header
        double s = 0;
#pragma unroll
        for (int k = 0; k < nk; ++k) {
            const int64_t e = tid + (int64_t)k * kThreads;
            if (e < D) s += S.w.get(k) * xval(k, e);
        }
        double p = block_sum(s, red, buf, lane, wave);
        p *= S.wscale;
        p = p + S.intercept;
        const double eta = 1.0 / (alpha * (optimal_init + S.t - 1));
        sumloss += half_binomial_loss(y, p);
        const double class_weight = y > 0.0 ? P.weight_pos : P.weight_neg;
        double dloss = half_binomial_grad(y, p);
        if (dloss < -kMaxDloss) dloss = -kMaxDloss;
        else if (dloss > kMaxDloss) dloss = kMaxDloss;
        double update = -eta * dloss;
        update *= class_weight * 1.0;
        if (P.penalty >= RML_SGD_L2) {                          // not for the pure L1 penalty (sk:513-516)
            const double c = 1.0 - ((1.0 - l1_ratio) * eta * alpha);
            S.wscale *= c > 0 ? c : 0;
            if (S.wscale < 1e-9) sgd_reset_wscale<EPT, AVG>(S, nk, tid, D);
        }
        if (update != 0.0) S.intercept += update * 1.0;
        const bool averaging = AVG && 0 < average && average <= S.t;
        const double num_iter = S.t - average + 1;
        if (L1) S.u += (l1_ratio * eta * alpha);
        const double c_add = update / S.wscale, c_avg = -update / S.wscale;
        // w.add, w.add_average and l1penalty, element by element in that order
#pragma unroll
        for (int k = 0; k < nk; ++k) {
            const int64_t e = tid + (int64_t)k * kThreads;
            if (e < D) {
                const double val = xval(k, e);
                double wk = S.w.get(k);
                if (update != 0.0) wk += val * c_add;
                if (AVG && averaging) S.aw.set(k, S.aw.get(k) + S.average_a * val * c_avg);
                if (L1) {
                    const double z = wk;
                    const double qk = S.q.get(k);
                    if (S.wscale * z > 0.0) { const double v = wk - ((S.u + qk) / S.wscale); wk = v > 0.0 ? v : 0.0; }
                    else if (S.wscale * z < 0.0) { const double v = wk + ((S.u - qk) / S.wscale); wk = v < 0.0 ? v : 0.0; }
                    S.q.set(k, qk + S.wscale * (wk - z));
                }
                S.w.set(k, wk);
            }
        }
        if (AVG && averaging) {
            const double mu = 1.0 / num_iter;
            if (num_iter > 1) S.average_b /= (1.0 - mu);
            S.average_a += mu * S.average_b * S.wscale;
            S.avg_intercept += ((S.intercept - S.avg_intercept) / num_iter);
        }
        S.t += 1;
    }
    return sumloss;
}

// floating-point under-/overflow check on the stored (unscaled) weights, sk:554-557: this thread's share
template <int EPT>
__device__ __forceinline__ int sgd_nonfinite(const SgdState<EPT>& S, int nk, int tid, int64_t D) {
    int nonfinite = !isfinite(S.intercept);
#pragma unroll
    for (int k = 0; k < nk; ++k)
        if (tid + (int64_t)k * kThreads < D) nonfinite |= !isfinite(S.w.get(k));
    return nonfinite;
}

template <int EPT, bool L1, bool AVG>
__global__ __launch_bounds__(kThreads) void k_sgd(const SgdDev* __restrict__ probs, const int32_t* __restrict__ order,
                                                  const float* __restrict__ X, int64_t N, int64_t D, int64_t ld,
                                                  double* __restrict__ intercept_out, double* __restrict__ avg_intercept_out,
                                                  int32_t* __restrict__ iter_out, double* __restrict__ t_out,
                                                  int32_t* __restrict__ status_out) {
    __shared__ int32_t perm[kMaxRows];
    __shared__ double red[2][kWaves];
    __shared__ int flag[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SgdDev P = probs[order[blockIdx.x]];
    const int n = P.n;
    const int nk = EPT ? EPT : (int)((D + kThreads - 1) / kThreads);

    // ---- row indices checked before anything is read or written; the index array of the dataset (0 .. n-1) ----
    if (tid < 2) flag[tid] = 0;
    __syncthreads();
    int bad = 0;
    for (int i = tid; i < n; i += kThreads) {
        const int64_t r = P.rows[i];
        if (r < 0 || r >= N) bad = 1;
        perm[i] = i;
    }
    if (bad) flag[0] = 1;
    __syncthreads();
    if (flag[0]) {
        if (tid == 0) status_out[P.out] = -1;
        return;
    }

    SgdState<EPT> S;
    S.w.bind(P.ws, tid); S.q.bind(P.ws + D, tid); S.aw.bind(P.ws + 2 * D, tid);
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int64_t e = tid + (int64_t)k * kThreads;
        const bool in = e < D;
        if (EPT || in) {
            S.w.set(k, P.warm && in ? P.coef[e] : 0.0);
            if (L1) S.q.set(k, 0.0);
            if (AVG) S.aw.set(k, P.warm && in ? P.avg_coef[e] : 0.0);
        }
    }
    S.intercept = P.warm ? intercept_out[P.out] : 0.0;
    S.avg_intercept = P.warm && AVG ? avg_intercept_out[P.out] : 0.0;
    S.wscale = 1.0; S.average_a = 0.0; S.average_b = 1.0; S.u = 0.0; S.t = P.t0;
    const double l1_ratio = P.penalty == RML_SGD_L2 ? 0.0 : (P.penalty == RML_SGD_L1 ? 1.0 : P.l1_ratio);
    double best_loss = INFINITY;
    int no_improvement = 0, buf = 0, status = 1, epochs = 0;

    for (int epoch = 0; epoch < P.max_iter; ++epoch) {
        if (P.shuffle) {
            if (tid == 0) fisher_yates(P.seed, n, perm);           // every read of the last epoch lies before its last barrier
            __syncthreads();
        }
        const double sumloss = sgd_epoch<EPT, L1, AVG>(S, P, P.rows, P.y, -1, n, perm, X, D, ld, nk, l1_ratio, red, buf, tid, lane, wave);
        epochs = epoch + 1;

        if (sgd_nonfinite(S, nk, tid, D)) flag[1] = 1;
        __syncthreads();
        if (flag[1]) { status = 2; break; }
        if (P.tol > -INFINITY && sumloss > best_loss - P.tol * (double)(unsigned)n) ++no_improvement;
        else no_improvement = 0;
        if (sumloss < best_loss) best_loss = sumloss;
        if (no_improvement >= P.n_iter_no_change) { status = 0; break; }
    }

    if (status != 2) sgd_reset_wscale<EPT, AVG>(S, nk, tid, D);     // (sklearn raises instead; the outputs are then whatever the epoch left)
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int64_t e = tid + (int64_t)k * kThreads;
        if (e < D) {
            P.coef[e] = S.w.get(k);
            if (AVG) P.avg_coef[e] = S.aw.get(k);
        }
    }
    if (tid == 0) {
        intercept_out[P.out] = S.intercept;
        if (AVG) avg_intercept_out[P.out] = S.avg_intercept;
        iter_out[P.out] = epochs;
        t_out[P.out] = P.t0 + (double)((int64_t)epochs * n);
        status_out[P.out] = status;
    }
}

// ---- scoring: SGDClassifier.predict on the held-out rows of every fit ----------------------------------------------------------
struct FitDev {
    const int32_t* test_rows;
    const int32_t* test_y;
    double* dec;                                    // n_test x n_dec
    int32_t* labels;                                // n_test
    int32_t prob0, n_test;
};

// one workgroup per held-out row: the row's decision value per class in the dot order of the header, the label, the count
__global__ __launch_bounds__(kThreads) void k_sgd_score(const FitDev* __restrict__ fits, const SgdDev* __restrict__ probs,
                                                        const float* __restrict__ X, int64_t N, int64_t D, int64_t ld, int C,
                                                        const double* __restrict__ intercept, const double* __restrict__ avg_intercept,
                                                        const double* __restrict__ t, int32_t* __restrict__ correct) {
    __shared__ double red[2][kWaves];
    const FitDev F = fits[blockIdx.x];
    const int r = blockIdx.y;
    if (r >= F.n_test) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_dec = C == 2 ? 1 : C;
    const int64_t row = F.test_rows[r];
    const bool bad = row < 0 || row >= N;           // a row outside the matrix is not read: NaN, label -1
    const float* __restrict__ xr = X + (bad ? 0 : row) * ld;
    double tfit = probs[F.prob0].t0;                // est.t_: the largest of the fit's problems
    for (int c = 0; c < n_dec; ++c) { const double tc = t[probs[F.prob0 + c].out]; tfit = tc > tfit ? tc : tfit; }
    int buf = 0, best = 0;
    double bestv = 0;
    for (int c = 0; c < n_dec; ++c) {
        const SgdDev Q = probs[F.prob0 + c];
        const bool avg = Q.average > 0 && (double)Q.average <= tfit - 1.0;
        const double* __restrict__ cf = avg ? Q.avg_coef : Q.coef;
        double s = 0;
        for (int64_t e = tid; e < D; e += kThreads) s += cf[e] * (double)xr[e];
        double d = block_sum(s, red, buf, lane, wave);
        d = d + (avg ? avg_intercept[Q.out] : intercept[Q.out]);
        if (bad) d = NAN;
        if (tid == 0) F.dec[(int64_t)r * n_dec + c] = d;
        if (c == 0 || d > bestv) { bestv = d; best = c; }
    }
    if (tid == 0) {
        int label = C == 2 ? (bestv > 0 ? 1 : 0) : best;
        if (bad) label = -1;
        F.labels[r] = label;
        if (label == F.test_y[r]) atomicAdd(&correct[blockIdx.x], 1);
    }
}

// ---- a chain of partial_fit calls of one estimator: rml_sgd_online --------------------------------------------------------------
struct StepDev {                                    // one partial_fit call
    int64_t off;                                    // its rows and class indices in the two lists
    int32_t n;
    int32_t slot;                                   // which block of the decision workspace a scored step fills, else -1
    int32_t next_scored;                            // the next scored step after this one, or the step count
    uint32_t seed[kMaxClasses];                     // the shuffle seed of every class problem
};
constexpr int32_t kNoFail = 0x7f7f7f7f;             // the failure word as hipMemsetAsync leaves it: no step has failed

// One workgroup per class problem, alive for all the steps: the weights stay where k_sgd keeps them, every step is one epoch of
// sgd_epoch from what the last step left, followed by the intercept statements of _fit_binary / _fit_multiclass (SI, AI, A: see
// include/radarml.h) and, for a scored step, this class's decision value of every held-out row.  The workgroups exchange nothing
// but the failure word: a problem whose weights go non-finite at step s lowers it to s with an integer atomic, and the others read
// it (one lane, an agent-scope atomic load) before every step and stop before a step later than it.
template <int EPT, bool L1, bool AVG>
__global__ __launch_bounds__(kThreads) void k_sgd_online(const SgdDev* __restrict__ probs, const StepDev* __restrict__ steps, int n_steps,
                                                         const int32_t* __restrict__ rows, const int32_t* __restrict__ cls, int n_classes,
                                                         const float* __restrict__ X, int64_t N, int64_t D, int64_t ld,
                                                         const int32_t* __restrict__ test_rows, int n_test,
                                                         double* __restrict__ intercept_out, double* __restrict__ avg_intercept_out,
                                                         double* __restrict__ t_out, int32_t* __restrict__ status_out,
                                                         const int32_t* __restrict__ avg_flag, int32_t* fail,
                                                         int32_t* __restrict__ avg_flag_out, double* __restrict__ decws) {
    __shared__ int32_t perm[kMaxRows];
    __shared__ double red[2][kWaves];
    __shared__ int flag[2];
    __shared__ int32_t seen;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kp = blockIdx.x;
    const SgdDev P = probs[kp];
    const int pos_class = n_classes == 2 ? 1 : kp;
    const int n_dec = n_classes == 2 ? 1 : n_classes;
    const int nk = EPT ? EPT : (int)((D + kThreads - 1) / kThreads);

    // ---- every row index of every step and of the held-out rows checked before anything is written ----
    if (tid < 2) flag[tid] = 0;
    __syncthreads();
    int bad = 0;
    for (int s = 0; s < n_steps; ++s) {
        const int64_t off = steps[s].off;
        const int n = steps[s].n;
        for (int i = tid; i < n; i += kThreads) {
            const int64_t r = rows[off + i];
            if (r < 0 || r >= N) bad = 1;
        }
    }
    for (int i = tid; i < n_test; i += kThreads) {
        const int64_t r = test_rows[i];
        if (r < 0 || r >= N) bad = 1;
    }
    if (bad) flag[0] = 1;
    __syncthreads();
    if (flag[0]) {
        if (tid == 0) status_out[P.out] = -1;
        return;
    }

    SgdState<EPT> S;
    S.w.bind(P.ws, tid); S.q.bind(P.ws + D, tid); S.aw.bind(P.ws + 2 * D, tid);
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int64_t e = tid + (int64_t)k * kThreads;
        const bool in = e < D;
        if (EPT || in) {
            S.w.set(k, P.warm && in ? P.coef[e] : 0.0);
            if (AVG) S.aw.set(k, P.warm && in ? P.avg_coef[e] : 0.0);
        }
    }
    double SI = P.warm ? intercept_out[P.out] : 0.0;
    double AI = P.warm && AVG ? avg_intercept_out[P.out] : 0.0;
    bool A = P.warm && AVG && *avg_flag != 0;
    S.t = P.t0;
    const double l1_ratio = P.penalty == RML_SGD_L2 ? 0.0 : (P.penalty == RML_SGD_L1 ? 1.0 : P.l1_ratio);
    int buf = 0, status = 1;

    for (int s = 0; s < n_steps; ++s) {
        const int64_t off = steps[s].off;
        const int n = steps[s].n, slot = steps[s].slot;
        if (tid == 0) seen = __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int i = tid; i < n; i += kThreads) perm[i] = i;       // a fresh _plain_sgd call: the index array 0 .. n-1
        __syncthreads();                                            // (every read of the last step lies before its last barrier)
        if (seen < s) break;                                        // another problem of the estimator failed at an earlier step
        if (P.shuffle) {
            if (tid == 0) fisher_yates(steps[s].seed[kp], n, perm);
            __syncthreads();
        }
        if (L1) {
#pragma unroll
            for (int k = 0; k < nk; ++k)
                if (EPT || tid + (int64_t)k * kThreads < D) S.q.set(k, 0.0);
        }
        S.intercept = SI; S.avg_intercept = AI;
        S.wscale = 1.0; S.average_a = 0.0; S.average_b = 1.0; S.u = 0.0;
        sgd_epoch<EPT, L1, AVG>(S, P, rows + off, cls + off, pos_class, n, perm, X, D, ld, nk, l1_ratio, red, buf, tid, lane, wave);

        if (sgd_nonfinite(S, nk, tid, D)) flag[1] = 1;
        __syncthreads();
        if (flag[1]) {
            status = 2;
            if (tid == 0) atomicMin(fail, s);
            break;
        }
        sgd_reset_wscale<EPT, AVG>(S, nk, tid, D);

        // _fit_binary / _fit_multiclass after the solver, on SI, AI and A
        if (AVG) AI = S.avg_intercept;
        const bool now = AVG && (double)P.average <= S.t - 1.0;
        if (n_classes > 2) {
            if (A) AI = S.intercept; else SI = S.intercept;
            A = now;
        } else if (now) {
            A = true;
        } else {
            SI = S.intercept;
            A = false;
        }

        if (slot >= 0 && n_test > 0) {                              // coef_[class] . x + intercept_[class] of every held-out row
            const double icpt = A ? AI : SI;
            double* __restrict__ out = decws + (int64_t)slot * n_test * n_dec + kp;
            Row<EPT> xn;
            sgd_load_row(xn, X, test_rows[0], ld, D, tid);
            for (int r = 0; r < n_test; ++r) {
                const float* __restrict__ xrow = X + (int64_t)test_rows[r] * ld;
                Row<EPT> x = xn;
                if (r + 1 < n_test) sgd_load_row(xn, X, test_rows[r + 1], ld, D, tid);
                double sum = 0;
#pragma unroll
                for (int k = 0; k < nk; ++k) {
                    const int64_t e = tid + (int64_t)k * kThreads;
                    if (e < D) {
                        double xv;
                        if constexpr (EPT > 0) xv = (double)x.v[k]; else xv = (double)xrow[e];
                        double c = S.w.get(k);
                        if constexpr (AVG) c = A ? S.aw.get(k) : c;
                        sum += c * xv;
                    }
                }
                double d = block_sum(sum, red, buf, lane, wave);
                d = d + icpt;
                if (tid == 0) out[(int64_t)r * n_dec] = d;
            }
        }
    }

    // the weights go to memory once (after a failure: whatever the failed epoch left, as rml_sgd_solve)
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int64_t e = tid + (int64_t)k * kThreads;
        if (e < D) {
            P.coef[e] = S.w.get(k);
            if (AVG) P.avg_coef[e] = S.aw.get(k);
        }
    }
    if (tid == 0) {
        intercept_out[P.out] = SI;
        if (AVG) avg_intercept_out[P.out] = AI;
        t_out[P.out] = S.t;
        status_out[P.out] = status;
        if (kp == 0) *avg_flag_out = A ? 1 : 0;     // k_sgd_online_finish hands it on: a late workgroup may still read avg_flag
    }
}

// After k_sgd_online, one workgroup per step: the labels of a scored step from the decision values the class workgroups left, and
// the count of correct ones (an integer sum through LDS); -1 for a step that was not scored or not reached.  The last scored step
// also leaves its labels and decision values in the call's outputs.
constexpr int kFinishThreads = 256;
__global__ __launch_bounds__(kFinishThreads) void k_sgd_online_finish(const StepDev* __restrict__ steps, int n_steps, int n_classes,
                                                                      const int32_t* __restrict__ test_y, int n_test,
                                                                      const double* __restrict__ decws, const int32_t* __restrict__ status0,
                                                                      const int32_t* __restrict__ fail, const int32_t* __restrict__ avg_flag_new,
                                                                      int32_t* __restrict__ avg_flag, int32_t* __restrict__ fail_step,
                                                                      int32_t* __restrict__ correct, int32_t* __restrict__ labels,
                                                                      double* __restrict__ dec) {
    __shared__ int32_t count;
    if (*status0 == -1) return;                                     // a row outside the matrix: every output stays as it was
    const int s = blockIdx.x, tid = threadIdx.x;
    const int32_t failed = *fail;
    const int reached = failed < n_steps ? failed : n_steps;        // the steps 0 .. reached-1 were run by every problem
    if (s == 0 && tid == 0) {
        *fail_step = failed < n_steps ? failed : -1;
        *avg_flag = *avg_flag_new;
    }
    const StepDev st = steps[s];
    if (st.slot < 0 || s >= reached) {
        if (tid == 0) correct[s] = -1;
        return;
    }
    if (tid == 0) count = 0;
    __syncthreads();
    const int n_dec = n_classes == 2 ? 1 : n_classes;
    const bool last = st.next_scored >= reached;
    const double* __restrict__ dv = decws + (int64_t)st.slot * n_test * n_dec;
    int mine = 0;
    for (int r = tid; r < n_test; r += kFinishThreads) {
        int best = 0;
        double bestv = dv[(int64_t)r * n_dec];
        for (int c = 1; c < n_dec; ++c) {
            const double d = dv[(int64_t)r * n_dec + c];
            if (d > bestv) { bestv = d; best = c; }
        }
        const int label = n_classes == 2 ? (bestv > 0 ? 1 : 0) : best;
        mine += label == test_y[r];
        if (last) {
            labels[r] = label;
            for (int c = 0; c < n_dec; ++c) dec[(int64_t)r * n_dec + c] = dv[(int64_t)r * n_dec + c];
        }
    }
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    if (tid == 0) correct[s] = count;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int check_problems(const char* who, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int64_t n_probs, int64_t n_rows_total,
                   int64_t n_y_total, int64_t n_out) {
    RML_REQUIRE(N >= 1 && D >= 1 && ld >= D, RML_ERR_INVALID, "%s: bad matrix layout N=%lld D=%lld ld=%lld", who, (long long)N, (long long)D,
                (long long)ld);
    RML_REQUIRE(n_probs >= 0 && n_probs < ((int64_t)1 << 24) && n_rows_total >= 0 && n_y_total >= 0 && n_out >= 0, RML_ERR_INVALID,
                "%s: bad counts", who);
    for (int64_t i = 0; i < n_probs; ++i) {
        const rml_sgd_problem& p = probs[i];
        RML_REQUIRE(p.n >= 1 && p.n <= kMaxRows, RML_ERR_INVALID, "%s: problem %lld: n=%d outside [1, %d]", who, (long long)i, p.n, kMaxRows);
        RML_REQUIRE(p.rows_off >= 0 && p.rows_off + p.n <= n_rows_total, RML_ERR_INVALID, "%s: problem %lld: rows [%lld, +%d) outside the %lld "
                    "row indices", who, (long long)i, (long long)p.rows_off, p.n, (long long)n_rows_total);
        RML_REQUIRE(p.y_off >= 0 && p.y_off + p.n <= n_y_total, RML_ERR_INVALID, "%s: problem %lld: labels [%lld, +%d) outside the %lld given",
                    who, (long long)i, (long long)p.y_off, p.n, (long long)n_y_total);
        RML_REQUIRE(p.out >= 0 && p.out < n_out, RML_ERR_INVALID, "%s: problem %lld: output slot %lld outside [0, %lld)", who, (long long)i,
                    (long long)p.out, (long long)n_out);
        RML_REQUIRE(p.penalty == RML_SGD_L1 || p.penalty == RML_SGD_L2 || p.penalty == RML_SGD_ELASTICNET, RML_ERR_INVALID,
                    "%s: problem %lld: penalty %d", who, (long long)i, p.penalty);
        RML_REQUIRE(p.alpha > 0 && isfinite(p.alpha) && p.l1_ratio >= 0 && p.l1_ratio <= 1, RML_ERR_INVALID, "%s: problem %lld: alpha=%g "
                    "(finite, > 0: the 'optimal' schedule divides by it) l1_ratio=%g (0..1)", who, (long long)i, p.alpha, p.l1_ratio);
        RML_REQUIRE(p.average >= 0 && p.max_iter >= 1 && p.n_iter_no_change >= 1, RML_ERR_INVALID, "%s: problem %lld: average=%d max_iter=%d "
                    "n_iter_no_change=%d", who, (long long)i, p.average, p.max_iter, p.n_iter_no_change);
        RML_REQUIRE(!isnan(p.tol) && isfinite(p.weight_pos) && isfinite(p.weight_neg) && p.t0 >= 1 && isfinite(p.t0), RML_ERR_INVALID,
                    "%s: problem %lld: tol=%g weight_pos=%g weight_neg=%g t0=%g", who, (long long)i, p.tol, p.weight_pos, p.weight_neg, p.t0);
    }
    return RML_OK;
}

// the 'optimal' schedule's offset (sk:_sgd_fast.pyx.tp:446-451), on the host with libm as scikit-learn computes it
double optimal_init_of(double alpha) {
    const double typw = sqrt(1.0 / sqrt(alpha));
    const double e = exp(typw);                     // cy_gradient(1.0, -typw): -typw > -37 for every alpha > 5.4e-7; else exp(-typw) - 1
    const double g = -typw > -37 ? ((1 - 1.0) - 1.0 * e) / (1 + e) : exp(-typw) - 1.0;
    const double initial_eta0 = typw / (g > 1.0 ? g : 1.0);
    return 1.0 / (initial_eta0 * alpha);
}

SgdDev to_dev(const rml_sgd_problem& p, int64_t D, const int32_t* rows, const int32_t* y, double* coef, double* avg_coef) {
    SgdDev d{};
    d.rows = rows ? rows + p.rows_off : nullptr;
    d.y = y ? y + p.y_off : nullptr;
    d.coef = coef + p.out * D;
    d.avg_coef = avg_coef + p.out * D;
    d.alpha = p.alpha; d.l1_ratio = p.l1_ratio; d.tol = p.tol; d.weight_pos = p.weight_pos; d.weight_neg = p.weight_neg; d.t0 = p.t0;
    d.optimal_init = optimal_init_of(p.alpha);
    d.out = p.out;
    d.n = p.n; d.penalty = p.penalty; d.average = p.average; d.max_iter = p.max_iter; d.n_iter_no_change = p.n_iter_no_change;
    d.shuffle = p.shuffle != 0; d.warm = p.warm != 0; d.seed = p.seed;
    return d;
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

int ept_of(int64_t D, int cap) {                    // elements per thread of the resident variant, 0: the workspace variant
    if (D > cap) return 0;
    for (int e : {1, 2, 4, 10})
        if (D <= (int64_t)e * kThreads) return e;
    return 0;
}

typedef void (*sgd_kernel)(const SgdDev*, const int32_t*, const float*, int64_t, int64_t, int64_t, double*, double*, int32_t*, double*,
                           int32_t*);
template <int EPT>
sgd_kernel pick_flags(bool l1, bool avg) {
    return l1 ? (avg ? k_sgd<EPT, true, true> : k_sgd<EPT, true, false>) : (avg ? k_sgd<EPT, false, true> : k_sgd<EPT, false, false>);
}
sgd_kernel pick(int ept, bool l1, bool avg) {
    switch (ept) {
        case 1: return pick_flags<1>(l1, avg);
        case 2: return pick_flags<2>(l1, avg);
        case 4: return pick_flags<4>(l1, avg);
        case 10: return pick_flags<10>(l1, avg);
        default: return pick_flags<0>(l1, avg);
    }
}

typedef void (*sgd_online_kernel)(const SgdDev*, const StepDev*, int, const int32_t*, const int32_t*, int, const float*, int64_t, int64_t,
                                  int64_t, const int32_t*, int, double*, double*, double*, int32_t*, const int32_t*, int32_t*, int32_t*, double*);
template <int EPT>
sgd_online_kernel pick_online_flags(bool l1, bool avg) {
    return l1 ? (avg ? k_sgd_online<EPT, true, true> : k_sgd_online<EPT, true, false>)
              : (avg ? k_sgd_online<EPT, false, true> : k_sgd_online<EPT, false, false>);
}
sgd_online_kernel pick_online(int ept, bool l1, bool avg) {
    switch (ept) {
        case 1: return pick_online_flags<1>(l1, avg);
        case 2: return pick_online_flags<2>(l1, avg);
        case 4: return pick_online_flags<4>(l1, avg);
        case 10: return pick_online_flags<10>(l1, avg);
        default: return pick_online_flags<0>(l1, avg);
    }
}

}  // namespace

extern "C" int rml_sgd_shuffle(uint32_t seed, int64_t n, int32_t* perm_inout) {
    RML_REQUIRE(n >= 0 && n <= INT32_MAX && (perm_inout || n == 0), RML_ERR_INVALID, "rml_sgd_shuffle: bad argument");
    fisher_yates(seed, (int)n, perm_inout);
    return RML_OK;
}

extern "C" int rml_sgd_solve(rml_ctx* ctx, const float* X, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int64_t n_probs,
                             const int32_t* rows, int64_t n_rows_total, const int32_t* y, int64_t n_y_total, int64_t n_out, double* coef,
                             double* avg_coef, double* intercept, double* avg_intercept, int32_t* n_iter, double* t, int32_t* status,
                             void* stream) {
    RML_REQUIRE(ctx && (probs || n_probs == 0), RML_ERR_INVALID, "rml_sgd_solve: NULL argument");
    if (n_probs == 0) return RML_OK;
    RML_REQUIRE(X && rows && y && coef && avg_coef && intercept && avg_intercept && n_iter && t && status, RML_ERR_INVALID,
                "rml_sgd_solve: NULL argument");
    int rc = check_problems("rml_sgd_solve", N, D, ld, probs, n_probs, n_rows_total, n_y_total, n_out);
    if (rc) return rc;
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);
    const int ept = ept_of(D, ctx->opt.sgd_resident_d);
    // one launch per (L1, averaging) pair present in the batch, the longest problems first within it
    std::vector<int32_t> order((size_t)n_probs);
    auto group = [&](int32_t a) { return (probs[a].penalty != RML_SGD_L2 ? 2 : 0) + (probs[a].average > 0 ? 1 : 0); };
    for (int64_t i = 0; i < n_probs; ++i) order[(size_t)i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        if (group(a) != group(b)) return group(a) < group(b);
        return (int64_t)probs[a].n * probs[a].max_iter > (int64_t)probs[b].n * probs[b].max_iter;
    });
    const size_t dev_bytes = align16((size_t)n_probs * sizeof(SgdDev)), ord_bytes = align16((size_t)n_probs * 4);
    const size_t state = ept ? 0 : align16((size_t)D * 3 * sizeof(double));
    void* ws = nullptr;
    rc = rml_ws_reserve(ctx, dev_bytes + ord_bytes + state * (size_t)n_probs, &ws, st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    void* stage = nullptr;
    rc = rml_stage_reserve(ctx, dev_bytes + ord_bytes, &stage);
    if (rc) return rc;
    SgdDev* dev = static_cast<SgdDev*>(stage);
    for (int64_t i = 0; i < n_probs; ++i) {
        dev[i] = to_dev(probs[i], D, rows, y, coef, avg_coef);
        if (!ept) dev[i].ws = reinterpret_cast<double*>(wsb + dev_bytes + ord_bytes + state * (size_t)i);
    }
    memcpy(static_cast<unsigned char*>(stage) + dev_bytes, order.data(), (size_t)n_probs * 4);
    rc = rml_stage_upload(ctx, wsb, dev_bytes + ord_bytes, st);
    if (rc) return rc;
    const SgdDev* dprobs = reinterpret_cast<const SgdDev*>(wsb);
    const int32_t* dorder = reinterpret_cast<const int32_t*>(wsb + dev_bytes);
    for (int64_t b = 0; b < n_probs;) {
        int64_t e = b;
        while (e < n_probs && group(order[(size_t)e]) == group(order[(size_t)b])) ++e;
        const int g = group(order[(size_t)b]);
        hipLaunchKernelGGL(pick(ept, (g & 2) != 0, (g & 1) != 0), dim3((unsigned)(e - b)), dim3(kThreads), 0, st, dprobs, dorder + b, X, N, D,
                           ld, intercept, avg_intercept, n_iter, t, status);
        RML_HIP(hipGetLastError());
        b = e;
    }
    return RML_OK;
}

extern "C" int rml_sgd_score(rml_ctx* ctx, const float* X, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int64_t n_probs,
                             int64_t n_out, const double* coef, const double* avg_coef, const double* intercept,
                             const double* avg_intercept, const double* t, int n_classes, const rml_sgd_fit* fits, int64_t n_fits,
                             const int32_t* test_rows, const int32_t* test_y, int64_t n_test_total, double* dec, int32_t* labels,
                             int32_t* correct, void* stream) {
    RML_REQUIRE(ctx && (fits || n_fits == 0), RML_ERR_INVALID, "rml_sgd_score: NULL argument");
    if (n_fits == 0) return RML_OK;
    RML_REQUIRE(X && probs && coef && avg_coef && intercept && avg_intercept && t && test_rows && test_y && dec && labels && correct,
                RML_ERR_INVALID, "rml_sgd_score: NULL argument");
    RML_REQUIRE(n_classes >= 2 && n_classes <= kMaxClasses, RML_ERR_INVALID, "rml_sgd_score: n_classes=%d outside [2, %d]", n_classes,
                kMaxClasses);
    RML_REQUIRE(N >= 1 && D >= 1 && ld >= D && n_probs >= 0 && n_probs < ((int64_t)1 << 24) && n_out >= 0, RML_ERR_INVALID,
                "rml_sgd_score: bad matrix layout or counts");
    for (int64_t i = 0; i < n_probs; ++i)
        RML_REQUIRE(probs[i].out >= 0 && probs[i].out < n_out, RML_ERR_INVALID, "rml_sgd_score: problem %lld: output slot %lld outside "
                    "[0, %lld)", (long long)i, (long long)probs[i].out, (long long)n_out);
    const int n_dec = n_classes == 2 ? 1 : n_classes;
    RML_REQUIRE(n_fits < 65536 && n_test_total >= 0, RML_ERR_INVALID, "rml_sgd_score: bad counts");
    int64_t max_test = 0;
    for (int64_t f = 0; f < n_fits; ++f) {
        const rml_sgd_fit& F = fits[f];
        RML_REQUIRE(F.prob0 >= 0 && (int64_t)F.prob0 + n_dec <= n_probs, RML_ERR_INVALID, "rml_sgd_score: fit %lld: problems [%d, +%d) outside "
                    "the %lld problems", (long long)f, F.prob0, n_dec, (long long)n_probs);
        RML_REQUIRE(F.n_test >= 0 && F.test_off >= 0 && F.test_off + F.n_test <= n_test_total, RML_ERR_INVALID, "rml_sgd_score: fit %lld: "
                    "held-out rows [%lld, +%d) outside the %lld given", (long long)f, (long long)F.test_off, F.n_test, (long long)n_test_total);
        max_test = std::max(max_test, (int64_t)F.n_test);
    }
    RML_REQUIRE(max_test < 65536, RML_ERR_INVALID, "rml_sgd_score: more than 65 535 held-out rows in one fit");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);
    const size_t dev_bytes = align16((size_t)n_probs * sizeof(SgdDev)), fit_bytes = align16((size_t)n_fits * sizeof(FitDev));
    void* ws = nullptr;
    int rc = rml_ws_reserve(ctx, dev_bytes + fit_bytes, &ws, st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    void* stage = nullptr;
    rc = rml_stage_reserve(ctx, dev_bytes + fit_bytes, &stage);
    if (rc) return rc;
    SgdDev* dev = static_cast<SgdDev*>(stage);
    for (int64_t i = 0; i < n_probs; ++i)
        dev[i] = to_dev(probs[i], D, nullptr, nullptr, const_cast<double*>(coef), const_cast<double*>(avg_coef));
    FitDev* fd = reinterpret_cast<FitDev*>(static_cast<unsigned char*>(stage) + dev_bytes);
    for (int64_t f = 0; f < n_fits; ++f) {
        const rml_sgd_fit& F = fits[f];
        FitDev& d = fd[f];
        d.test_rows = test_rows + F.test_off; d.test_y = test_y + F.test_off;
        d.dec = dec + F.test_off * n_dec; d.labels = labels + F.test_off;
        d.prob0 = F.prob0; d.n_test = F.n_test;
    }
    rc = rml_stage_upload(ctx, wsb, dev_bytes + fit_bytes, st);
    if (rc) return rc;
    RML_HIP(hipMemsetAsync(correct, 0, (size_t)n_fits * sizeof(int32_t), st));
    if (max_test > 0) {
        hipLaunchKernelGGL(k_sgd_score, dim3((unsigned)n_fits, (unsigned)max_test), dim3(kThreads), 0, st,
                           reinterpret_cast<const FitDev*>(wsb + dev_bytes), reinterpret_cast<const SgdDev*>(wsb), X, N, D, ld, n_classes,
                           intercept, avg_intercept, t, correct);
        RML_HIP(hipGetLastError());
    }
    return RML_OK;
}

extern "C" int rml_sgd_online(rml_ctx* ctx, const float* X, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int n_classes,
                              const rml_sgd_step* steps, int64_t n_steps, const int32_t* rows, const int32_t* cls, int64_t n_rows_total,
                              const int32_t* test_rows, const int32_t* test_y, int64_t n_test, int64_t n_out, double* coef, double* avg_coef,
                              double* intercept, double* avg_intercept, double* t, int32_t* avg_flag, int32_t* status, int32_t* fail_step,
                              int32_t* correct, int32_t* labels, double* dec, void* stream) {
    RML_REQUIRE(ctx && (steps || n_steps == 0), RML_ERR_INVALID, "rml_sgd_online: NULL argument");
    if (n_steps == 0) return RML_OK;
    RML_REQUIRE(X && probs && rows && cls && coef && avg_coef && intercept && avg_intercept && t && avg_flag && status && fail_step && correct,
                RML_ERR_INVALID, "rml_sgd_online: NULL argument");
    RML_REQUIRE(n_classes >= 2 && n_classes <= kMaxClasses, RML_ERR_INVALID, "rml_sgd_online: n_classes=%d outside [2, %d]", n_classes,
                kMaxClasses);
    RML_REQUIRE(n_steps > 0 && n_steps < ((int64_t)1 << 24) && n_test >= 0 && n_test < ((int64_t)1 << 24), RML_ERR_INVALID,
                "rml_sgd_online: bad counts");
    RML_REQUIRE(n_test == 0 || (test_rows && test_y && labels && dec), RML_ERR_INVALID, "rml_sgd_online: NULL argument");
    const int K = n_classes == 2 ? 1 : n_classes;
    // the descriptors checked as rml_sgd_solve checks them, with the fields a partial_fit call does not have set to what it is
    rml_sgd_problem pr[kMaxClasses];
    for (int k = 0; k < K; ++k) {
        pr[k] = probs[k];
        pr[k].n = 1; pr[k].rows_off = 0; pr[k].y_off = 0; pr[k].max_iter = 1; pr[k].n_iter_no_change = 1; pr[k].tol = -INFINITY;
    }
    int rc = check_problems("rml_sgd_online", N, D, ld, pr, K, 1, 1, n_out);
    if (rc) return rc;
    for (int k = 1; k < K; ++k) {
        RML_REQUIRE(pr[k].penalty == pr[0].penalty && pr[k].average == pr[0].average && pr[k].t0 == pr[0].t0 && pr[k].warm == pr[0].warm,
                    RML_ERR_INVALID, "rml_sgd_online: problem %d: the class problems of one estimator share penalty, average, t0 and warm", k);
        for (int j = 0; j < k; ++j)
            RML_REQUIRE(pr[k].out != pr[j].out, RML_ERR_INVALID, "rml_sgd_online: problems %d and %d share output slot %lld", j, k,
                        (long long)pr[k].out);
    }
    int64_t n_scored = 0;
    for (int64_t s = 0; s < n_steps; ++s) {
        const rml_sgd_step& st = steps[s];
        RML_REQUIRE(st.n >= 1 && st.n <= kMaxRows, RML_ERR_INVALID, "rml_sgd_online: step %lld: n=%d outside [1, %d]", (long long)s, st.n,
                    kMaxRows);
        RML_REQUIRE(st.off >= 0 && st.off + st.n <= n_rows_total, RML_ERR_INVALID, "rml_sgd_online: step %lld: rows [%lld, +%d) outside the "
                    "%lld given", (long long)s, (long long)st.off, st.n, (long long)n_rows_total);
        if (st.score && n_test > 0) ++n_scored;
    }
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);
    const int ept = ept_of(D, ctx->opt.sgd_resident_d);
    const int n_dec = n_classes == 2 ? 1 : n_classes;
    // workspace: the failure word and the new flag (one 16-byte block, set before every call) | descriptors | steps |
    // the state of the workspace variant | the decision values of every scored step
    const size_t word_bytes = 16, dev_bytes = align16((size_t)K * sizeof(SgdDev)), step_bytes = align16((size_t)n_steps * sizeof(StepDev));
    const size_t state = ept ? 0 : align16((size_t)D * 3 * sizeof(double));
    const size_t dec_bytes = align16((size_t)n_scored * (size_t)n_test * n_dec * sizeof(double));
    void* ws = nullptr;
    rc = rml_ws_reserve(ctx, word_bytes + dev_bytes + step_bytes + state * (size_t)K + dec_bytes, &ws, st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    void* stage = nullptr;
    rc = rml_stage_reserve(ctx, dev_bytes + step_bytes, &stage);
    if (rc) return rc;
    SgdDev* dev = static_cast<SgdDev*>(stage);
    for (int k = 0; k < K; ++k) {
        dev[k] = to_dev(pr[k], D, nullptr, nullptr, coef, avg_coef);
        if (!ept) dev[k].ws = reinterpret_cast<double*>(wsb + word_bytes + dev_bytes + step_bytes + state * (size_t)k);
    }
    StepDev* sd = reinterpret_cast<StepDev*>(static_cast<unsigned char*>(stage) + dev_bytes);
    int32_t slot = 0;
    for (int64_t s = 0; s < n_steps; ++s) {
        sd[s].off = steps[s].off;
        sd[s].n = steps[s].n;
        sd[s].slot = steps[s].score && n_test > 0 ? slot++ : -1;
        for (int k = 0; k < kMaxClasses; ++k) sd[s].seed[k] = steps[s].seed[k];
    }
    int32_t next = (int32_t)n_steps;
    for (int64_t s = n_steps - 1; s >= 0; --s) {
        sd[s].next_scored = next;
        if (sd[s].slot >= 0) next = (int32_t)s;
    }
    RML_HIP(hipMemsetAsync(wsb, 0x7f, word_bytes, st));
    rc = rml_stage_upload(ctx, wsb + word_bytes, dev_bytes + step_bytes, st);
    if (rc) return rc;
    int32_t* fail = reinterpret_cast<int32_t*>(wsb);
    int32_t* flag_new = fail + 1;
    const SgdDev* dprobs = reinterpret_cast<const SgdDev*>(wsb + word_bytes);
    const StepDev* dsteps = reinterpret_cast<const StepDev*>(wsb + word_bytes + dev_bytes);
    double* decws = reinterpret_cast<double*>(wsb + word_bytes + dev_bytes + step_bytes + state * (size_t)K);
    hipLaunchKernelGGL(pick_online(ept, pr[0].penalty != RML_SGD_L2, pr[0].average > 0), dim3((unsigned)K), dim3(kThreads), 0, st, dprobs, dsteps,
                       (int)n_steps, rows, cls, n_classes, X, N, D, ld, test_rows, (int)n_test, intercept, avg_intercept, t, status, avg_flag,
                       fail, flag_new, decws);
    RML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sgd_online_finish, dim3((unsigned)n_steps), dim3(kFinishThreads), 0, st, dsteps, (int)n_steps, n_classes, test_y,
                       (int)n_test, decws, status + pr[0].out, fail, flag_new, avg_flag, fail_step, correct, labels, dec);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
