// Binary logistic-regression fits of SGDClassifier solved on the device, one workgroup per fit (rml_sgd_solve), and the held-out
// rows scored from the solutions (rml_sgd_score).
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

    Own<EPT> w, q, aw;
    w.bind(P.ws, tid); q.bind(P.ws + D, tid); aw.bind(P.ws + 2 * D, tid);
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int64_t e = tid + (int64_t)k * kThreads;
        const bool in = e < D;
        if (EPT || in) {
            w.set(k, P.warm && in ? P.coef[e] : 0.0);
            if (L1) q.set(k, 0.0);
            if (AVG) aw.set(k, P.warm && in ? P.avg_coef[e] : 0.0);
        }
    }
    double intercept = P.warm ? intercept_out[P.out] : 0.0;
    double avg_intercept = P.warm && AVG ? avg_intercept_out[P.out] : 0.0;
    double wscale = 1.0, average_a = 0.0, average_b = 1.0, u = 0.0, t = P.t0;
    const double alpha = P.alpha;
    const double l1_ratio = P.penalty == RML_SGD_L2 ? 0.0 : (P.penalty == RML_SGD_L1 ? 1.0 : P.l1_ratio);
    const double optimal_init = P.optimal_init;
    const double average = (double)P.average;
    double best_loss = INFINITY;
    int no_improvement = 0, buf = 0, status = 1, epochs = 0;

    // WeightVector.reset_wscale (sk:_weight_vector.pyx.tp:191-201)
    auto reset_wscale = [&]() {
#pragma unroll
        for (int k = 0; k < nk; ++k) {
            if (tid + (int64_t)k * kThreads < D) {
                if (AVG) {
                    double a = aw.get(k);
                    a += average_a * w.get(k);
                    a *= 1.0 / average_b;
                    aw.set(k, a);
                }
                w.set(k, w.get(k) * wscale);
            }
        }
        if (AVG) { average_a = 0.0; average_b = 1.0; }
        wscale = 1.0;
    };
    auto load_row = [&](Row<EPT>& r, int64_t row) {
        if constexpr (EPT > 0) {
            const float* __restrict__ xr = X + row * ld;
#pragma unroll
            for (int k = 0; k < EPT; ++k) {
                const int64_t e = tid + (int64_t)k * kThreads;
                r.v[k] = e < D ? xr[e] : 0.0f;
            }
        }
    };

    for (int epoch = 0; epoch < P.max_iter; ++epoch) {
        double sumloss = 0;
        if (P.shuffle) {
            if (tid == 0) fisher_yates(P.seed, n, perm);           // every read of the last epoch lies before its last barrier
            __syncthreads();
        }
        Row<EPT> xn;
        load_row(xn, P.rows[perm[0]]);
        for (int i = 0; i < n; ++i) {
            const int pos = perm[i];
            const double y = (double)P.y[pos];
            const float* __restrict__ xrow = X + (int64_t)P.rows[pos] * ld;
            Row<EPT> x = xn;
            if (i + 1 < n) load_row(xn, P.rows[perm[i + 1]]);       // the next row travels while this one is reduced
            auto xval = [&](int k, int64_t e) -> double {
                if constexpr (EPT > 0) return (double)x.v[k]; else return (double)xrow[e];
            };

            // p = w.dot(x) + intercept, in the order of the header
            double s = 0;
#pragma unroll
            for (int k = 0; k < nk; ++k) {
                const int64_t e = tid + (int64_t)k * kThreads;
                if (e < D) s += w.get(k) * xval(k, e);
            }
            double p = block_sum(s, red, buf, lane, wave);
            p *= wscale;
            p = p + intercept;
            const double eta = 1.0 / (alpha * (optimal_init + t - 1));
            sumloss += half_binomial_loss(y, p);
            const double class_weight = y > 0.0 ? P.weight_pos : P.weight_neg;
            double dloss = half_binomial_grad(y, p);
            if (dloss < -kMaxDloss) dloss = -kMaxDloss;
            else if (dloss > kMaxDloss) dloss = kMaxDloss;
            double update = -eta * dloss;
            update *= class_weight * 1.0;
            if (P.penalty >= RML_SGD_L2) {                          // not for the pure L1 penalty (sk:513-516)
                const double c = 1.0 - ((1.0 - l1_ratio) * eta * alpha);
                wscale *= c > 0 ? c : 0;
                if (wscale < 1e-9) reset_wscale();
            }
            if (update != 0.0) intercept += update * 1.0;
            const bool averaging = AVG && 0 < average && average <= t;
            const double num_iter = t - average + 1;
            if (L1) u += (l1_ratio * eta * alpha);
            const double c_add = update / wscale, c_avg = -update / wscale;
            // w.add, w.add_average and l1penalty, element by element in that order
#pragma unroll
            for (int k = 0; k < nk; ++k) {
                const int64_t e = tid + (int64_t)k * kThreads;
                if (e < D) {
                    const double val = xval(k, e);
                    double wk = w.get(k);
                    if (update != 0.0) wk += val * c_add;
                    if (AVG && averaging) aw.set(k, aw.get(k) + average_a * val * c_avg);
                    if (L1) {
                        const double z = wk;
                        const double qk = q.get(k);
                        if (wscale * z > 0.0) { const double v = wk - ((u + qk) / wscale); wk = v > 0.0 ? v : 0.0; }
                        else if (wscale * z < 0.0) { const double v = wk + ((u - qk) / wscale); wk = v < 0.0 ? v : 0.0; }
                        q.set(k, qk + wscale * (wk - z));
                    }
                    w.set(k, wk);
                }
            }
            if (AVG && averaging) {
                const double mu = 1.0 / num_iter;
                if (num_iter > 1) average_b /= (1.0 - mu);
                average_a += mu * average_b * wscale;
                avg_intercept += ((intercept - avg_intercept) / num_iter);
            }
            t += 1;
        }
        epochs = epoch + 1;

        // floating-point under-/overflow check on the stored (unscaled) weights, sk:554-557
        int nonfinite = !isfinite(intercept);
#pragma unroll
        for (int k = 0; k < nk; ++k)
            if (tid + (int64_t)k * kThreads < D) nonfinite |= !isfinite(w.get(k));
        if (nonfinite) flag[1] = 1;
        __syncthreads();
        if (flag[1]) { status = 2; break; }
        if (P.tol > -INFINITY && sumloss > best_loss - P.tol * (double)(unsigned)n) ++no_improvement;
        else no_improvement = 0;
        if (sumloss < best_loss) best_loss = sumloss;
        if (no_improvement >= P.n_iter_no_change) { status = 0; break; }
    }

    if (status != 2) reset_wscale();                // (sklearn raises instead; the outputs are then whatever the epoch left)
#pragma unroll
    for (int k = 0; k < nk; ++k) {
        const int64_t e = tid + (int64_t)k * kThreads;
        if (e < D) {
            P.coef[e] = w.get(k);
            if (AVG) P.avg_coef[e] = aw.get(k);
        }
    }
    if (tid == 0) {
        intercept_out[P.out] = intercept;
        if (AVG) avg_intercept_out[P.out] = avg_intercept;
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
