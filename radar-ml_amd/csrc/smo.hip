// Binary C-SVC duals of an SVC search solved on the device, one workgroup per dual (rml_smo_solve), and the held-out rows
// scored from the solutions (rml_smo_score).
//
// Reference arithmetic replaced (sk: = scikit-learn, the reference's SVM dependency):
//   sk:svm/src/libsvm/svm.cpp:560-1160     Solver::Solve, select_working_set, do_shrinking, reconstruct_gradient, calculate_rho
//   sk:svm/src/libsvm/svm.cpp:1423-1470    SVC_Q::get_Q / get_QD / swap_index (the Qfloat rounding of a kernel row)
//   sk:svm/src/libsvm/svm.cpp:2842-2900    svm_predict_values: pairwise decision values and the vote
// called once per grid point, fold and class pair by the GridSearchCV(SVC) of train.py:462-491.
//
// The solver follows libsvm's iterate path exactly: the state lives in libsvm's POSITION order (swap_index permutes y, G, G_bar,
// alpha, alpha_status, active_set, C and QD together; the permutation decides ties and the order of the reconstruction sums),
// the arg-max / arg-min reductions keep libsvm's "last position among equal values wins", every element-wise expression is the
// same double expression WITHOUT contraction (libsvm's binary has no fused multiply-add; see the pragma below), and the few true
// sums (reconstruct_gradient per output, calculate_rho) run sequentially in position order.  n_iter, alpha and rho are then the
// bits SVC(kernel='precomputed').fit produces on the same matrix.  libsvm's kernel cache only saves recomputation and is left out:
// a kernel row is a gather from the Gram matrix (which must be bit-exactly symmetric, as rml_gram writes it).
//
// k_smo<true> keeps the state (59 bytes per row) in LDS; k_smo<false> is the same code on a slice of the context's workspace,
// for problems above the RML_OPT_SMO_LDS_ROWS cap.
#include "rml_internal.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <numeric>

// libsvm is compiled without FMA contraction; a*b+c must stay two roundings in every expression of this file
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr double kTau = 1e-12;
constexpr int kScratch = 320;                       // bytes of reduction scratch in front of the LDS state
constexpr int kRowBytes = 59;                       // state bytes per row (carve below)
constexpr int kMaxLds = 160 * 1024;
constexpr int kMaxClasses = 8;
enum : signed char { ST_LOWER = 0, ST_UPPER = 1, ST_FREE = 2 };

inline size_t state_bytes(int64_t l) { return ((size_t)l * kRowBytes + 15) & ~(size_t)15; }

struct SmoDev {                                     // one dual, device form
    const double* K;                                // its Gram matrix
    const int32_t* rows;                            // l Gram rows in libsvm's order (class i, then class j)
    double* alpha_out;                              // l
    unsigned char* ws;                              // state of the global variant (unused by the LDS variant)
    double Cp, Cn, eps;
    int32_t l, n_pos, shrinking, max_iter;
};

struct SmoState {
    double *G, *Gb, *alpha, *C, *QD;
    int32_t *aset, *grow, *pairs;
    float* Qi;
    signed char *y, *st, *flag;
};

__device__ inline SmoState carve(unsigned char* b, int l) {
    SmoState s;
    s.G = reinterpret_cast<double*>(b);
    s.Gb = s.G + l; s.alpha = s.Gb + l; s.C = s.alpha + l; s.QD = s.C + l;
    s.aset = reinterpret_cast<int32_t*>(s.QD + l);
    s.grow = s.aset + l; s.pairs = s.grow + l;
    s.Qi = reinterpret_cast<float*>(s.pairs + l);
    s.y = reinterpret_cast<signed char*>(s.Qi + l);
    s.st = s.y + l; s.flag = s.st + l;
    return s;
}

// libsvm scans positions upwards with >= (arg-max) / <= (arg-min): among equal values the highest position wins
__device__ inline bool better(double av, int ai, double bv, int bi) { return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai > bi)); }

__device__ inline void wave_best(double& v, int& idx) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(idx, m);
        if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
}

__device__ inline double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        v = ov > v ? ov : v;
    }
    return v;
}

template <typename T>
__device__ inline void swap_at(T* a, int i, int j) { const T t = a[i]; a[i] = a[j]; a[j] = t; }

template <bool LDS>
__global__ __launch_bounds__(kThreads) void k_smo(const SmoDev* __restrict__ probs, const int32_t* __restrict__ order, int64_t N,
                                                  int64_t ld, double* __restrict__ rho_out, int32_t* __restrict__ iter_out,
                                                  int32_t* __restrict__ stop_out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pi = order[blockIdx.x];
    const SmoDev P = probs[pi];
    double* red_v = reinterpret_cast<double*>(smem);            // [6 slots][kWaves]
    int* red_i = reinterpret_cast<int*>(smem + 192);            // [6 slots][kWaves]
    int* sh = reinterpret_cast<int*>(smem + 288);               // act, npairs of the compaction; bad-row flag
    unsigned char* base;
    if constexpr (LDS) base = smem + kScratch; else base = P.ws;
    const int l = P.l;
    const SmoState s = carve(base, l);
    const double* __restrict__ K = P.K;
    const double eps = P.eps;

    // ---- Solver::Solve initialisation: alpha = 0, G = p = -1, G_bar = 0, every variable at its lower bound ----
    int bad = 0;
    if (tid == 0) sh[2] = 0;
    __syncthreads();
    for (int t = tid; t < l; t += kThreads) {
        int64_t r = P.rows[t];
        if (r < 0 || r >= N) { bad = 1; r = 0; }
        s.aset[t] = t; s.grow[t] = (int32_t)r;
        s.y[t] = t < P.n_pos ? 1 : -1;
        s.C[t] = t < P.n_pos ? P.Cp : P.Cn;
        s.alpha[t] = 0.0; s.st[t] = ST_LOWER;
        s.G[t] = -1.0; s.Gb[t] = 0.0;
        s.QD[t] = K[r * ld + r];
    }
    if (bad) sh[2] = 1;
    __syncthreads();                                // (no __syncthreads_or: its static LDS would shift the dynamic base)
    if (sh[2]) {                                    // a row index outside the matrix: no solve, status -1
        for (int t = tid; t < l; t += kThreads) P.alpha_out[t] = 0.0;
        if (tid == 0) { rho_out[pi] = 0.0; iter_out[pi] = 0; stop_out[pi] = -1; }
        return;
    }

    int act = l;
    bool unshrink = false;

    // block arg-best of (v, idx) through scratch slot `slot`; every thread returns the same pair
    auto block_best = [&](double& v, int& idx, int slot) {
        wave_best(v, idx);
        if (lane == 0) { red_v[slot * kWaves + wave] = v; red_i[slot * kWaves + wave] = idx; }
    };
    auto read_best = [&](double& v, int& idx, int slot) {
        v = red_v[slot * kWaves]; idx = red_i[slot * kWaves];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            const double ov = red_v[slot * kWaves + w];
            const int oi = red_i[slot * kWaves + w];
            if (better(ov, oi, v, idx)) { v = ov; idx = oi; }
        }
    };
    auto read_max = [&](int slot) {
        double v = red_v[slot * kWaves];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) { const double ov = red_v[slot * kWaves + w]; v = ov > v ? ov : v; }
        return v;
    };
    // one element of kernel row Q_i (SVC_Q::get_Q): the product in double, rounded to Qfloat
    auto qval = [&](const double* krow, int yi, int k) -> float { return (float)((double)(yi * s.y[k]) * krow[s.grow[k]]); };

    // ---- reconstruct_gradient: G of the inactive positions from G_bar and the free active variables, ascending position ----
    auto reconstruct = [&]() {
        if (act == l) return;
        for (int j = act + tid; j < l; j += kThreads) {
            double g = s.Gb[j] + (-1.0);
            const int yj = s.y[j];
            const int64_t cj = s.grow[j];
            for (int i = 0; i < act; ++i)
                if (s.st[i] == ST_FREE) {
                    const float q = (float)((double)(s.y[i] * yj) * K[(int64_t)s.grow[i] * ld + cj]);
                    g += s.alpha[i] * q;
                }
            s.G[j] = g;
        }
        __syncthreads();
    };

    // ---- select_working_set; leaves Q_i[0, act) in s.Qi ----
    auto select = [&](int& out_i, int& out_j) -> int {
        double gmax = -INFINITY;
        int gi = -1;
        for (int t = tid; t < act; t += kThreads) {
            const double g = s.G[t];
            const signed char st = s.st[t];
            if (s.y[t] > 0) { if (st != ST_UPPER && -g >= gmax) { gmax = -g; gi = t; } }
            else            { if (st != ST_LOWER && g >= gmax) { gmax = g; gi = t; } }
        }
        block_best(gmax, gi, 0);
        __syncthreads();
        read_best(gmax, gi, 0);
        const int i = gi;
        if (i < 0) { __syncthreads(); return 1; }
        const int yi = s.y[i];
        const double* krow = K + (int64_t)s.grow[i] * ld;
        const double QDi = s.QD[i];
        const double two_yi = 2.0 * yi;
        double gmax2 = -INFINITY, best = -INFINITY;             // best = -obj_diff_min
        int gj = -1;
        for (int t = tid; t < act; t += kThreads) {
            const float q = qval(krow, yi, t);
            s.Qi[t] = q;
            const double g = s.G[t];
            const signed char st = s.st[t];
            if (s.y[t] > 0) {
                if (st != ST_LOWER) {
                    const double grad_diff = gmax + g;
                    if (g >= gmax2) gmax2 = g;
                    if (grad_diff > 0) {
                        const double quad = QDi + s.QD[t] - two_yi * q;
                        const double obj = quad > 0 ? -(grad_diff * grad_diff) / quad : -(grad_diff * grad_diff) / kTau;
                        if (gj < 0 || -obj >= best) { best = -obj; gj = t; }
                    }
                }
            } else {
                if (st != ST_UPPER) {
                    const double grad_diff = gmax - g;
                    if (-g >= gmax2) gmax2 = -g;
                    if (grad_diff > 0) {
                        const double quad = QDi + s.QD[t] + two_yi * q;
                        const double obj = quad > 0 ? -(grad_diff * grad_diff) / quad : -(grad_diff * grad_diff) / kTau;
                        if (gj < 0 || -obj >= best) { best = -obj; gj = t; }
                    }
                }
            }
        }
        block_best(best, gj, 1);
        gmax2 = wave_max(gmax2);
        if (lane == 0) red_v[2 * kWaves + wave] = gmax2;
        __syncthreads();
        read_best(best, gj, 1);
        gmax2 = read_max(2);
        if (gmax + gmax2 < eps || gj < 0) return 1;
        out_i = i; out_j = gj;
        return 0;
    };

    // ---- do_shrinking ----
    auto shrink = [&]() {
        double g1 = -INFINITY, g2 = -INFINITY;
        for (int t = tid; t < act; t += kThreads) {
            const double g = s.G[t];
            const signed char st = s.st[t];
            if (s.y[t] > 0) {
                if (st != ST_UPPER && -g >= g1) g1 = -g;
                if (st != ST_LOWER && g >= g2) g2 = g;
            } else {
                if (st != ST_UPPER && -g >= g2) g2 = -g;
                if (st != ST_LOWER && g >= g1) g1 = g;
            }
        }
        g1 = wave_max(g1); g2 = wave_max(g2);
        if (lane == 0) { red_v[3 * kWaves + wave] = g1; red_v[4 * kWaves + wave] = g2; }
        __syncthreads();
        g1 = read_max(3); g2 = read_max(4);
        if (!unshrink && g1 + g2 <= eps * 10) {
            unshrink = true;
            reconstruct();
            act = l;
        }
        for (int t = tid; t < act; t += kThreads) {             // be_shrunk
            const double g = s.G[t];
            const signed char st = s.st[t];
            bool f = false;
            if (st == ST_UPPER) f = s.y[t] > 0 ? -g > g1 : -g > g2;
            else if (st == ST_LOWER) f = s.y[t] > 0 ? g > g2 : g > g1;
            s.flag[t] = f;
        }
        __syncthreads();
        if (tid == 0) {                                         // libsvm's two-pointer compaction, in its order; the swaps are disjoint
            int a = act, np = 0;
            for (int i = 0; i < a; ++i)
                if (s.flag[i]) {
                    --a;
                    while (a > i) {
                        if (!s.flag[a]) { s.pairs[2 * np] = i; s.pairs[2 * np + 1] = a; ++np; break; }
                        --a;
                    }
                }
            sh[0] = a; sh[1] = np;
        }
        __syncthreads();
        act = sh[0];
        const int np = sh[1];
        for (int n = tid; n < np; n += kThreads) {              // swap_index
            const int a = s.pairs[2 * n], b = s.pairs[2 * n + 1];
            swap_at(s.y, a, b); swap_at(s.G, a, b); swap_at(s.st, a, b); swap_at(s.alpha, a, b); swap_at(s.aset, a, b);
            swap_at(s.grow, a, b); swap_at(s.Gb, a, b); swap_at(s.C, a, b); swap_at(s.QD, a, b);
        }
        __syncthreads();
    };

    auto status_of = [](double a, double C) -> signed char { return a >= C ? ST_UPPER : (a <= 0 ? ST_LOWER : ST_FREE); };

    // ---- the main loop of Solver::Solve ----
    const int period = l < 1000 ? l : 1000;
    int iter = 0, counter = period + 1, stopped = 0;
    while (true) {
        if (P.max_iter != -1 && iter >= P.max_iter) { stopped = 1; break; }
        if (--counter == 0) {
            counter = period;
            if (P.shrinking) shrink();
        }
        int i = -1, j = -1;
        if (select(i, j) != 0) {
            reconstruct();
            act = l;
            if (select(i, j) != 0) break;
            counter = 1;
        }
        ++iter;

        const int yi = s.y[i], yj = s.y[j];
        const double* krow_i = K + (int64_t)s.grow[i] * ld;
        const double* krow_j = K + (int64_t)s.grow[j] * ld;
        const double C_i = s.C[i], C_j = s.C[j];
        const double old_ai = s.alpha[i], old_aj = s.alpha[j];
        const double G_i = s.G[i], G_j = s.G[j];
        const double Qij = s.Qi[j];
        double ai = old_ai, aj = old_aj;
        if (yi != yj) {
            double quad = s.QD[i] + s.QD[j] + 2 * Qij;
            if (quad <= 0) quad = kTau;
            const double delta = (-G_i - G_j) / quad;
            const double diff = ai - aj;
            ai += delta; aj += delta;
            if (diff > 0) { if (aj < 0) { aj = 0; ai = diff; } }
            else          { if (ai < 0) { ai = 0; aj = -diff; } }
            if (diff > C_i - C_j) { if (ai > C_i) { ai = C_i; aj = C_i - diff; } }
            else                  { if (aj > C_j) { aj = C_j; ai = C_j + diff; } }
        } else {
            double quad = s.QD[i] + s.QD[j] - 2 * Qij;
            if (quad <= 0) quad = kTau;
            const double delta = (G_i - G_j) / quad;
            const double sum = ai + aj;
            ai -= delta; aj += delta;
            if (sum > C_i) { if (ai > C_i) { ai = C_i; aj = sum - C_i; } }
            else           { if (aj < 0) { aj = 0; ai = sum; } }
            if (sum > C_j) { if (aj > C_j) { aj = C_j; ai = sum - C_j; } }
            else           { if (ai < 0) { ai = 0; aj = sum; } }
        }
        const double d_ai = ai - old_ai, d_aj = aj - old_aj;
        const bool ui = s.st[i] == ST_UPPER, uj = s.st[j] == ST_UPPER;
        const signed char nsi = status_of(ai, C_i), nsj = status_of(aj, C_j);
        __syncthreads();                                        // every thread has read G[i], G[j], alpha, status
        for (int k = tid; k < act; k += kThreads) {
            const float qj = qval(krow_j, yj, k);
            s.G[k] += s.Qi[k] * d_ai + qj * d_aj;
        }
        if (tid == 0) { s.alpha[i] = ai; s.alpha[j] = aj; s.st[i] = nsi; s.st[j] = nsj; }
        const bool ci = ui != (nsi == ST_UPPER), cj = uj != (nsj == ST_UPPER);
        if (ci || cj)
            for (int k = tid; k < l; k += kThreads) {
                double gb = s.Gb[k];
                if (ci) { const float q = qval(krow_i, yi, k); if (ui) gb -= C_i * q; else gb += C_i * q; }
                if (cj) { const float q = qval(krow_j, yj, k); if (uj) gb -= C_j * q; else gb += C_j * q; }
                s.Gb[k] = gb;
            }
        __syncthreads();
    }

    // ---- calculate_rho (one lane, position order) and the solution scattered back through active_set ----
    if (tid == 0) {
        int nr_free = 0;
        double ub = INFINITY, lb = -INFINITY, sum_free = 0;
        for (int k = 0; k < act; ++k) {
            const double yG = s.y[k] * s.G[k];
            const signed char st = s.st[k];
            if (st == ST_UPPER) { if (s.y[k] < 0) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
            else if (st == ST_LOWER) { if (s.y[k] > 0) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
            else { ++nr_free; sum_free += yG; }
        }
        rho_out[pi] = nr_free > 0 ? sum_free / nr_free : (ub + lb) / 2;
        iter_out[pi] = iter;
        stop_out[pi] = stopped;
    }
    for (int t = tid; t < l; t += kThreads) P.alpha_out[s.aset[t]] = s.alpha[t];
}

// ---- scoring: svm_predict_values on K[test, train] for every (candidate, split) ---------------------------------------------
struct FitDev {
    const double* K;
    const int32_t* test_rows;
    const int32_t* test_y;
    double* dec;                                    // n_test x P
    int32_t* labels;                                // n_test
    int32_t prob0, n_test;
};

// one thread per (held-out row, class pair): sum over the pair's rows with alpha > 0 in libsvm's SV order (class i in row order,
// then class j), coefficient +alpha / -alpha, then -= rho
__global__ __launch_bounds__(kThreads) void k_smo_decision(const FitDev* __restrict__ fits, const SmoDev* __restrict__ probs,
                                                           const double* __restrict__ rho, int64_t N, int64_t ld, int P) {
    const FitDev F = fits[blockIdx.x];
    const int64_t item = (int64_t)blockIdx.y * kThreads + threadIdx.x;
    if (item >= (int64_t)F.n_test * P) return;
    const int p = (int)(item / F.n_test), r = (int)(item % F.n_test);       // a wave shares the pair: its alpha loads are uniform
    const SmoDev Q = probs[F.prob0 + p];
    // a row index outside the matrix (held-out or training) is not read: the value is NaN and k_smo_vote labels the row -1
    const int64_t tr = F.test_rows[r];
    bool bad = tr < 0 || tr >= N;
    const double* krow = F.K + (bad ? 0 : tr) * ld;
    double sum = 0;
    for (int k = 0; k < Q.l; ++k) {
        const double a = Q.alpha_out[k];
        if (a > 0) {
            const double coef = k < Q.n_pos ? a : -a;
            const int64_t c = Q.rows[k];
            if (c < 0 || c >= N) { bad = true; break; }
            sum += coef * krow[c];
        }
    }
    sum -= rho[F.prob0 + p];
    F.dec[(int64_t)r * P + p] = bad ? NAN : sum;
}

// libsvm's vote: dec > 0 votes for i, else for j; the first maximum wins.  Writes the labels (class indices; -1 for a row with a
// NaN decision value) and the count of labels equal to test_y.
__global__ __launch_bounds__(kThreads) void k_smo_vote(const FitDev* __restrict__ fits, int C, int P, int32_t* __restrict__ correct) {
    __shared__ int cnt;
    const FitDev F = fits[blockIdx.x];
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int r = threadIdx.x; r < F.n_test; r += kThreads) {
        int vote[kMaxClasses];
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) vote[c] = 0;
        int p = 0;
        bool bad = false;
        for (int i = 0; i < C; ++i)
            for (int j = i + 1; j < C; ++j, ++p) {
                const double d = F.dec[(int64_t)r * P + p];
                bad |= d != d;
                const int w = d > 0 ? i : j;
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) vote[c] += c == w;
            }
        int bestc = 0, bestv = vote[0];
#pragma unroll
        for (int c = 1; c < kMaxClasses; ++c)
            if (c < C && vote[c] > bestv) { bestv = vote[c]; bestc = c; }
        if (bad) bestc = -1;
        F.labels[r] = bestc;
        mine += bestc == F.test_y[r];
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) correct[blockIdx.x] = cnt;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
int check_problems(const char* who, int64_t N, int64_t ld, int64_t stride_k, int n_mats, const rml_smo_problem* probs, int64_t n_probs,
                   int64_t n_rows_total, int64_t n_alpha_total) {
    RML_REQUIRE(N >= 1 && ld >= N && stride_k >= N * ld && n_mats >= 1, RML_ERR_INVALID, "%s: bad matrix layout N=%lld ld=%lld stride_k=%lld "
                "n_mats=%d", who, (long long)N, (long long)ld, (long long)stride_k, n_mats);
    RML_REQUIRE(n_probs >= 0 && n_probs < ((int64_t)1 << 24) && n_rows_total >= 0 && n_alpha_total >= 0, RML_ERR_INVALID, "%s: bad counts", who);
    for (int64_t i = 0; i < n_probs; ++i) {
        const rml_smo_problem& p = probs[i];
        RML_REQUIRE(p.matrix >= 0 && p.matrix < n_mats, RML_ERR_INVALID, "%s: problem %lld: matrix %d outside [0, %d)", who, (long long)i,
                    p.matrix, n_mats);
        RML_REQUIRE(p.l >= 1 && p.n_pos >= 0 && p.n_pos <= p.l, RML_ERR_INVALID, "%s: problem %lld: l=%d n_pos=%d", who, (long long)i, p.l,
                    p.n_pos);
        RML_REQUIRE(p.rows_off >= 0 && p.rows_off + p.l <= n_rows_total, RML_ERR_INVALID, "%s: problem %lld: rows [%lld, +%d) outside the %lld "
                    "row indices", who, (long long)i, (long long)p.rows_off, p.l, (long long)n_rows_total);
        RML_REQUIRE(p.alpha_off >= 0 && p.alpha_off + p.l <= n_alpha_total, RML_ERR_INVALID, "%s: problem %lld: alpha [%lld, +%d) outside the "
                    "%lld outputs", who, (long long)i, (long long)p.alpha_off, p.l, (long long)n_alpha_total);
        RML_REQUIRE(p.Cp > 0 && p.Cn > 0 && p.eps > 0 && isfinite(p.Cp) && isfinite(p.Cn) && isfinite(p.eps), RML_ERR_INVALID,
                    "%s: problem %lld: Cp=%g Cn=%g eps=%g must be finite and > 0", who, (long long)i, p.Cp, p.Cn, p.eps);
        RML_REQUIRE(p.max_iter >= -1, RML_ERR_INVALID, "%s: problem %lld: max_iter=%d (-1: no limit)", who, (long long)i, p.max_iter);
    }
    return RML_OK;
}

SmoDev to_dev(const rml_smo_problem& p, const double* gram, int64_t stride_k, const int32_t* rows, double* alpha) {
    SmoDev d{};
    d.K = gram + (int64_t)p.matrix * stride_k;
    d.rows = rows + p.rows_off;
    d.alpha_out = alpha + p.alpha_off;
    d.Cp = p.Cp; d.Cn = p.Cn; d.eps = p.eps;
    d.l = p.l; d.n_pos = p.n_pos; d.shrinking = p.shrinking != 0; d.max_iter = p.max_iter;
    return d;
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" int rml_smo_solve(rml_ctx* ctx, const double* gram, int64_t N, int64_t ld, int64_t stride_k, int n_mats,
                             const rml_smo_problem* probs, int64_t n_probs, const int32_t* rows, int64_t n_rows_total,
                             double* alpha, int64_t n_alpha_total, double* rho, int32_t* n_iter, int32_t* stopped, void* stream) {
    RML_REQUIRE(ctx && (probs || n_probs == 0), RML_ERR_INVALID, "rml_smo_solve: NULL argument");
    if (n_probs == 0) return RML_OK;
    RML_REQUIRE(gram && rows && alpha && rho && n_iter && stopped, RML_ERR_INVALID, "rml_smo_solve: NULL argument");
    int rc = check_problems("rml_smo_solve", N, ld, stride_k, n_mats, probs, n_probs, n_rows_total, n_alpha_total);
    if (rc) return rc;
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);
    // largest problems first (they end last); the LDS variant takes what fits under the cap, the workspace variant the rest
    const int cap = ctx->opt.smo_lds_rows;
    std::vector<int32_t> order((size_t)n_probs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return probs[a].l > probs[b].l; });
    const int64_t n_glob = std::partition_point(order.begin(), order.end(), [&](int32_t a) { return probs[a].l > cap; }) - order.begin();
    const size_t dev_bytes = align16((size_t)n_probs * sizeof(SmoDev)), ord_bytes = align16((size_t)n_probs * 4);
    size_t ws_bytes = dev_bytes + ord_bytes;
    std::vector<size_t> ws_off((size_t)n_glob);
    for (int64_t i = 0; i < n_glob; ++i) { ws_off[(size_t)i] = ws_bytes; ws_bytes += state_bytes(probs[order[(size_t)i]].l); }
    void* ws = nullptr;
    rc = rml_ws_reserve(ctx, ws_bytes, &ws, st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    // descriptors and launch order through the context's pinned staging buffer: one asynchronous copy
    void* stage = nullptr;
    rc = rml_stage_reserve(ctx, dev_bytes + ord_bytes, &stage);
    if (rc) return rc;
    SmoDev* dev = static_cast<SmoDev*>(stage);
    for (int64_t i = 0; i < n_probs; ++i) dev[i] = to_dev(probs[i], gram, stride_k, rows, alpha);
    for (int64_t i = 0; i < n_glob; ++i) dev[order[(size_t)i]].ws = wsb + ws_off[(size_t)i];
    memcpy(static_cast<unsigned char*>(stage) + dev_bytes, order.data(), (size_t)n_probs * 4);
    rc = rml_stage_upload(ctx, wsb, dev_bytes + ord_bytes, st);
    if (rc) return rc;
    const SmoDev* dprobs = reinterpret_cast<const SmoDev*>(wsb);
    const int32_t* dorder = reinterpret_cast<const int32_t*>(wsb + dev_bytes);
    if (n_glob > 0) {
        hipLaunchKernelGGL(k_smo<false>, dim3((unsigned)n_glob), dim3(kThreads), kScratch, st, dprobs, dorder, N, ld, rho, n_iter, stopped);
        RML_HIP(hipGetLastError());
    }
    if (n_probs > n_glob) {
        const int lds = kScratch + (int)state_bytes(probs[order[(size_t)n_glob]].l);
        RML_MAX_DYN_LDS(kMaxLds, k_smo<true>);
        hipLaunchKernelGGL(k_smo<true>, dim3((unsigned)(n_probs - n_glob)), dim3(kThreads), lds, st, dprobs, dorder + n_glob, N, ld, rho,
                           n_iter, stopped);
        RML_HIP(hipGetLastError());
    }
    return RML_OK;
}

extern "C" int rml_smo_score(rml_ctx* ctx, const double* gram, int64_t N, int64_t ld, int64_t stride_k, int n_mats,
                             const rml_smo_problem* probs, int64_t n_probs, const int32_t* rows, int64_t n_rows_total,
                             const double* alpha, int64_t n_alpha_total, const double* rho, int n_classes,
                             const rml_smo_fit* fits, int64_t n_fits, const int32_t* test_rows, const int32_t* test_y,
                             int64_t n_test_total, double* dec, int32_t* labels, int32_t* correct, void* stream) {
    RML_REQUIRE(ctx && (fits || n_fits == 0), RML_ERR_INVALID, "rml_smo_score: NULL argument");
    if (n_fits == 0) return RML_OK;
    RML_REQUIRE(gram && probs && rows && alpha && rho && test_rows && test_y && dec && labels && correct, RML_ERR_INVALID,
                "rml_smo_score: NULL argument");
    RML_REQUIRE(n_classes >= 2 && n_classes <= kMaxClasses, RML_ERR_INVALID, "rml_smo_score: n_classes=%d outside [2, %d]", n_classes,
                kMaxClasses);
    int rc = check_problems("rml_smo_score", N, ld, stride_k, n_mats, probs, n_probs, n_rows_total, n_alpha_total);
    if (rc) return rc;
    const int P = n_classes * (n_classes - 1) / 2;
    RML_REQUIRE(n_fits < ((int64_t)1 << 24) && n_test_total >= 0, RML_ERR_INVALID, "rml_smo_score: bad counts");
    int64_t max_items = 0;
    for (int64_t f = 0; f < n_fits; ++f) {
        const rml_smo_fit& F = fits[f];
        RML_REQUIRE(F.prob0 >= 0 && (int64_t)F.prob0 + P <= n_probs, RML_ERR_INVALID, "rml_smo_score: fit %lld: problems [%d, +%d) outside "
                    "the %lld problems", (long long)f, F.prob0, P, (long long)n_probs);
        RML_REQUIRE(F.n_test >= 0 && F.test_off >= 0 && F.test_off + F.n_test <= n_test_total, RML_ERR_INVALID, "rml_smo_score: fit %lld: "
                    "held-out rows [%lld, +%d) outside the %lld given", (long long)f, (long long)F.test_off, F.n_test, (long long)n_test_total);
        for (int p = 1; p < P; ++p)
            RML_REQUIRE(probs[F.prob0 + p].matrix == probs[F.prob0].matrix, RML_ERR_INVALID, "rml_smo_score: fit %lld: its class pairs name "
                        "different matrices", (long long)f);
        max_items = std::max(max_items, (int64_t)F.n_test * P);
    }
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);
    const size_t dev_bytes = align16((size_t)n_probs * sizeof(SmoDev)), fit_bytes = align16((size_t)n_fits * sizeof(FitDev));
    void* ws = nullptr;
    rc = rml_ws_reserve(ctx, dev_bytes + fit_bytes, &ws, st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(ws);
    void* stage = nullptr;
    rc = rml_stage_reserve(ctx, dev_bytes + fit_bytes, &stage);
    if (rc) return rc;
    SmoDev* dev = static_cast<SmoDev*>(stage);
    for (int64_t i = 0; i < n_probs; ++i) dev[i] = to_dev(probs[i], gram, stride_k, rows, const_cast<double*>(alpha));
    FitDev* fd = reinterpret_cast<FitDev*>(static_cast<unsigned char*>(stage) + dev_bytes);
    for (int64_t f = 0; f < n_fits; ++f) {
        const rml_smo_fit& F = fits[f];
        FitDev& d = fd[f];
        d.K = gram + (int64_t)probs[F.prob0].matrix * stride_k;
        d.test_rows = test_rows + F.test_off; d.test_y = test_y + F.test_off;
        d.dec = dec + F.test_off * P; d.labels = labels + F.test_off;
        d.prob0 = F.prob0; d.n_test = F.n_test;
    }
    rc = rml_stage_upload(ctx, wsb, dev_bytes + fit_bytes, st);
    if (rc) return rc;
    const SmoDev* dprobs = reinterpret_cast<const SmoDev*>(wsb);
    const FitDev* dfits = reinterpret_cast<const FitDev*>(wsb + dev_bytes);
    if (max_items > 0) {
        hipLaunchKernelGGL(k_smo_decision, dim3((unsigned)n_fits, (unsigned)((max_items + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           dfits, dprobs, rho, N, ld, P);
        RML_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_smo_vote, dim3((unsigned)n_fits), dim3(kThreads), 0, st, dfits, n_classes, P, correct);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
