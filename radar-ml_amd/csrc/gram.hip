// Kernel matrices of one set of rows against itself for SVC training with kernel='precomputed' (rml_gram).
//
// Reference arithmetic replaced (sk: = scikit-learn, the reference's SVM dependency):
//   sk:svm/src/libsvm/svm.cpp:457            K[i][j] = x_i . x_j                                       (linear)
//   sk:svm/src/libsvm/svm.cpp:461-475        K[i][j] = exp(-gamma (x_i.x_i + x_j.x_j - 2 x_i.x_j))     (RBF)
// called, pair by pair and per grid point, by the GridSearchCV(SVC) of train.py:462-491.
//
// The inner products do not depend on the kernel: they are formed ONCE, on v_mfma_f64_16x16x4_f64 (float32 rows widened to
// float64 in registers: every product is exact, the accumulation is float64 -- libsvm's arithmetic class on float32 rows), and
// every requested kernel matrix is written from them in one epilogue (d^2 once per stored element, one exp per gamma).  An
// off-diagonal tile stores each inner product twice (K[i][j] and K[j][i]) and forms d^2 and the exps for each store from the same
// G, in the same order: the two values are the same bits.  Staging the values instead would need a second 64 KiB LDS image per
// kernel; the recomputation is ~10 % of the K loop at D = 10 010.
//
// Tiles: 128 x 128 per workgroup, 4 waves as 2 x 2, each wave 4 x 4 MFMA tiles of 16 x 16; K-step = 32 floats = 128 bytes per
// row, staged by LDS-DMA into swizzled [128 rows][128 B] images, double-buffered (mfma_tile.h: the K loop of k_svm_gemm<PATH_F64>).
// Only the upper triangle of tile pairs (bi <= bj) is launched.  An off-diagonal tile writes K[i][j] and its mirror K[j][i] from
// the same inner product; a diagonal tile writes its upper half and mirrors it -- every matrix is symmetric by construction.
// Both stores go through one LDS image of the accumulator half so that each wave stores 512 contiguous bytes of one row.
// The rows are first copied into a zero-padded workspace (k_gram_prep: N_pad x D_pad float32 + float64 row norms), so the
// K loop needs no clamping and no tail.  Every reduction has a fixed order: results are deterministic run to run.
#include "rml_internal.h"
#include "mfma_tile.h"
#include <math.h>

namespace {

constexpr int kStepFloats = kStepBytes / 4;
constexpr int kHalfRows = 64;                       // epilogue: one row half of the tile at a time
constexpr int kLdG = kTile + 1;                     // doubles per LDS row of the G image (odd: the column reads are conflict free)
constexpr int kGBytes = kHalfRows * kLdG * 8;       // 66 048 B
constexpr int kMaxKinds = 8;
constexpr int kLdsBytes = (kGBytes > 4 * kTileBytes ? kGBytes : 4 * kTileBytes) + 2 * kTile * 8 + kMaxKinds * 8;   // + row norms, gammas

struct GramArgs {
    const float* a; int64_t lda;                    // padded rows (N_pad x lda floats, lda % 32 == 0)
    const double* nsq;                              // N_pad row norms
    int KT;                                          // K-steps
    int64_t N;                                      // valid rows
    int NT;                                         // row tiles
    int nk;
    int kind[kMaxKinds];
    double gamma[kMaxKinds];
    double* out; int64_t ld_out, stride_k;
};

// rows -> zero-padded float32 copy and float64 norms (a fixed-order tree: deterministic).  One workgroup per padded row.
__global__ __launch_bounds__(256) void k_gram_prep(const float* __restrict__ feat, int64_t ld_feat, int64_t N, int64_t D,
                                                   float* __restrict__ a, int64_t lda, double* __restrict__ nsq) {
    __shared__ double red[256];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const bool valid = r < N;
    double s = 0.0;
    for (int64_t d = tid; d < lda; d += 256) {
        const float v = (valid && d < D) ? feat[r * ld_feat + d] : 0.0f;
        a[r * lda + d] = v;
        s = fma((double)v, (double)v, s);
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) nsq[r] = red[0];
}

__global__ __launch_bounds__(256, 2) void k_gram(GramArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // block -> tile pair (bi <= bj): consecutive blocks share the column tile bj
    const int64_t b = blockIdx.x;
    int64_t bj = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (bj * (bj + 1) / 2 > b) --bj;
    while ((bj + 1) * (bj + 2) / 2 <= b) ++bj;
    const int64_t bi = b - bj * (bj + 1) / 2;
    const int64_t r0 = bi * kTile, c0 = bj * kTile;
    const bool diag = bi == bj;

    // row norms of the two tiles and the kernels' gammas (-1: linear), behind the epilogue's G image (untouched by the K loop)
    double* tn = reinterpret_cast<double*>(smem + (kLdsBytes - 2 * kTile * 8 - kMaxKinds * 8));
    double* kg = tn + 2 * kTile;
    tn[tid] = a.nsq[(tid < kTile ? r0 : c0 - kTile) + tid];
    if (tid < a.nk) kg[tid] = a.kind[tid] == RML_GRAM_LINEAR ? -1.0 : a.gamma[tid];

    TileStager sg;
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(a.a);
    sg.init<false>(rows, a.lda * 4, r0, rows, a.lda * 4, c0, 0, wave, lane);
    Frag64 fa, fb;
    fa.init(wr * 64, lane); fb.init(wc * 64, lane);
    const int kgrp = lane >> 4;
    v4d acc[4][4];
    zero_acc(acc);
    tile_k_loop(sg, smem, 0, a.KT, [&](const unsigned char* sA, const unsigned char* sB) { kstep_f64(acc, sA, sB, fa, fb, kgrp); });

    // ---- epilogue: one row half (64 rows x 128 columns of G) at a time through LDS ----
    double* gd = reinterpret_cast<double*>(smem);      // [64][kLdG]
    const int nk = a.nk;
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();                               // tile images / the previous half consumed
        if (wr == pass) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ml = cd64_row(i * 16, r, lane);
                        const int nl = cd64_col(wc * 64 + j * 16, lane);
                        gd[ml * kLdG + nl] = acc[i][j][r];
                    }
        }
        __syncthreads();
        // direct store K[r0 + rl][c0 + cl]: lanes on consecutive columns
        {
            const int cl = tid & 127;
            const int64_t col = c0 + cl;
            const double ncol = tn[kTile + cl];
            for (int s = 0; s < kHalfRows / 2; ++s) {
                const int hl = (tid >> 7) + 2 * s;
                const int rl = pass * kHalfRows + hl;
                const int64_t row = r0 + rl;
                if (row >= a.N || col >= a.N || (diag && rl > cl)) continue;
                const double g = gd[hl * kLdG + cl];
                const double d2 = (tn[rl] + ncol) - 2.0 * g;
                double* o = a.out + row * a.ld_out + col;
                for (int k = 0; k < nk; ++k) {
                    const double gk = kg[k];
                    o[k * a.stride_k] = gk < 0.0 ? g : exp(-gk * d2);
                }
            }
        }
        // mirrored store K[c0 + cl][r0 + rl]: lanes on consecutive rows of the half (= consecutive columns of the mirror)
        {
            const int hl = tid & 63;
            const int rl = pass * kHalfRows + hl;
            const int64_t row = r0 + rl;
            const double nrow = tn[rl];
            for (int s = 0; s < kTile / 4; ++s) {
                const int cl = (tid >> 6) + 4 * s;
                const int64_t col = c0 + cl;
                if (row >= a.N || col >= a.N || (diag && rl >= cl)) continue;
                const double g = gd[hl * kLdG + cl];
                const double d2 = (nrow + tn[kTile + cl]) - 2.0 * g;
                double* o = a.out + col * a.ld_out + row;
                for (int k = 0; k < nk; ++k) {
                    const double gk = kg[k];
                    o[k * a.stride_k] = gk < 0.0 ? g : exp(-gk * d2);
                }
            }
        }
    }
}

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

}  // namespace

extern "C" int rml_gram(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int64_t D,
                        int nk, const int* kinds, const double* gammas,
                        double* out, int64_t ld_out, int64_t stride_k, void* stream) {
    RML_REQUIRE(ctx && kinds && gammas, RML_ERR_INVALID, "rml_gram: NULL argument");
    RML_REQUIRE(N >= 0 && D >= 1, RML_ERR_INVALID, "rml_gram: bad shape N=%lld D=%lld", (long long)N, (long long)D);
    RML_REQUIRE(nk >= 1 && nk <= kMaxKinds, RML_ERR_INVALID, "rml_gram: nk=%d outside [1, %d]", nk, kMaxKinds);
    for (int k = 0; k < nk; ++k) {
        RML_REQUIRE(kinds[k] == RML_GRAM_LINEAR || kinds[k] == RML_GRAM_RBF, RML_ERR_INVALID, "rml_gram: unknown kind %d (entry %d)",
                    kinds[k], k);
        RML_REQUIRE(kinds[k] == RML_GRAM_LINEAR || (isfinite(gammas[k]) && gammas[k] >= 0.0), RML_ERR_INVALID,
                    "rml_gram: gamma[%d] = %g is not a finite non-negative number", k, gammas[k]);
    }
    RML_REQUIRE(ld_feat >= D, RML_ERR_INVALID, "rml_gram: ld_feat=%lld < D=%lld", (long long)ld_feat, (long long)D);
    RML_REQUIRE(ld_out >= N, RML_ERR_INVALID, "rml_gram: ld_out=%lld < N=%lld", (long long)ld_out, (long long)N);
    RML_REQUIRE(stride_k >= N * ld_out, RML_ERR_INVALID, "rml_gram: stride_k=%lld < N*ld_out=%lld", (long long)stride_k,
                (long long)(N * ld_out));
    if (N == 0) return RML_OK;
    RML_REQUIRE(feat && out, RML_ERR_INVALID, "rml_gram: NULL argument");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);                      // shared workspace
    const int64_t Np = round_up(N, kTile), lda = round_up(D, kStepFloats);
    const int64_t NT = Np / kTile;
    RML_REQUIRE(NT * (NT + 1) / 2 < (int64_t)1 << 31, RML_ERR_INVALID, "rml_gram: N=%lld is too large", (long long)N);
    const size_t abytes = (size_t)(Np * lda * 4);
    void* ws = nullptr;
    int rc = rml_ws_reserve(ctx, abytes + (size_t)Np * 8, &ws, st);
    if (rc) return rc;
    float* a = static_cast<float*>(ws);
    double* nsq = reinterpret_cast<double*>(static_cast<unsigned char*>(ws) + abytes);
    hipLaunchKernelGGL(k_gram_prep, dim3((unsigned)Np), dim3(256), 0, st, feat, ld_feat, N, D, a, lda, nsq);
    RML_HIP(hipGetLastError());
    GramArgs g{};
    g.a = a; g.lda = lda; g.nsq = nsq;
    g.KT = (int)(lda / kStepFloats);
    g.N = N; g.NT = (int)NT; g.nk = nk;
    for (int k = 0; k < nk; ++k) { g.kind[k] = kinds[k]; g.gamma[k] = kinds[k] == RML_GRAM_LINEAR ? 0.0 : gammas[k]; }
    g.out = out; g.ld_out = ld_out; g.stride_k = stride_k;
    RML_MAX_DYN_LDS(kLdsBytes, k_gram);
    hipLaunchKernelGGL(k_gram, dim3((unsigned)(NT * (NT + 1) / 2)), dim3(256), kLdsBytes, st, g);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
