// Kernel matrices of one set of rows against itself for SVC training with kernel='precomputed' (rml_gram), the inner products
// kept apart per column segment (rml_gram_segments) and the kernel matrices of any union of segments composed from them
// (rml_gram_compose): the Gram service of an SVC search over kernels and projection masks.
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
// gram_tile, the body of k_gram and k_gseg.  Tiles: 128 x 128 per workgroup, 4 waves as 2 x 2, each wave 4 x 4 MFMA tiles of
// 16 x 16; K-step = 32 floats = 128 bytes per row, staged by LDS-DMA into swizzled [128 rows][128 B] images, double-buffered
// (mfma_tile.h: the K loop of k_svm_gemm<PATH_F64>).  Only the upper triangle of tile pairs (bi <= bj) is launched.  An
// off-diagonal tile writes K[i][j] and its mirror K[j][i] from the same inner product; a diagonal tile writes its upper half and
// mirrors it -- every matrix is symmetric by construction.  Both stores go through one LDS image of the accumulator half so that
// each wave stores 512 contiguous bytes of one row.  The rows are first copied into a zero-padded workspace (k_gram_prep:
// N_pad x D_pad float32 + float64 row norms), so the K loop needs no clamping and no tail.  Every reduction has a fixed order:
// results are deterministic run to run.
//
// Segments.  A feature row of the reference is concat(xz, yz, xy) (common.py: the ProjMask picks which projections are
// concatenated), so for a mask the inner products and squared norms are sums of the per-projection ones:
//   G_mask = sum_{s in mask} G_s        |x|^2_mask = sum_{s in mask} |x|^2_s
// One pass over the rows gives every mask x kernel matrix of the search.  k_gseg runs gram_tile over the K-steps of ONE segment
// and stores the inner products: grid = tile pairs x segments, the longest segment dispatched first.  k_gram_prep pads every
// segment of the copy to a whole number of K-steps with zeros, so no K-step straddles a segment.  Segments are not cut into K
// pieces: every element is one accumulator chain in ascending k, no partial sums, no atomics.
//
// k_gram_compose is elementwise and memory-bound: per element and mask g = sum G_s and n_i, n_j = sum nsq_s (set bits in ascending
// s) are formed once, then d2 = (n_i + n_j) - 2 g and one store per output of that mask.  G_s is bit-symmetric and n_i + n_j
// commutes, so element (i, j) and (j, i) run the same operations on the same bits: every output is bit-exactly symmetric.
#include "rml_internal.h"
#include "mfma_tile.h"
#include <math.h>
#include <vector>

namespace {

constexpr int kStepFloats = kStepBytes / 4;
constexpr int kHalfRows = 64;                       // epilogue: one row half of the tile at a time
constexpr int kLdG = kTile + 1;                     // doubles per LDS row of the G image (odd: the column reads are conflict free)
constexpr int kGBytes = kHalfRows * kLdG * 8;       // 66 048 B
constexpr int kTileLds = kGBytes > 4 * kTileBytes ? kGBytes : 4 * kTileBytes;      // what gram_tile uses
constexpr int kMaxKinds = 8;
constexpr int kGramLds = kTileLds + 2 * kTile * 8 + kMaxKinds * 8;                 // k_gram: + row norms, gammas
constexpr int kMaxSeg = 8;
constexpr int kMaxOut = 8;                          // outputs of one mask per k_gram_compose launch

struct SegLayout {
    int nseg;
    int64_t len[kMaxSeg];                           // columns of the segment
    int64_t src[kMaxSeg];                           // its first column in the caller's rows
    int64_t dst[kMaxSeg];                           // ... in the padded copy (a multiple of 32)
    int64_t plen[kMaxSeg];                          // its padded length
};

struct GramArgs {
    const float* a; int64_t lda;                    // padded rows (N_pad x lda floats, lda % 32 == 0)
    const double* nsq;                              // N_pad row norms
    int KT;                                          // K-steps
    int64_t N;                                      // valid rows
    int nk;
    int kind[kMaxKinds];
    double gamma[kMaxKinds];
    double* out; int64_t ld_out, stride_k;
};

struct SegArgs {
    const float* a; int64_t lda;                    // padded rows (N_pad x lda floats)
    int64_t N;
    int seg[kMaxSeg];                               // blockIdx.y -> segment, longest first
    int kt0[kMaxSeg], kt1[kMaxSeg];                 // K-steps of the segment (by segment)
    double* G; int64_t ld_g, stride_s;
};

struct ComposeArgs {
    const double* G; int64_t ld_g, stride_s;
    const double* nsq;
    int64_t N;
    int nseg;
    unsigned bits;
    int nk;
    int kidx[kMaxOut];                              // output slots of this mask
    double gamma[kMaxOut];                          // -1: linear
    double* out; int64_t ld_out, stride_k;
};

// rows -> copy with every segment zero-padded to whole K-steps, and the float64 squared norm of every segment of the row (a
// fixed-order tree: deterministic).  One workgroup per padded row; columns past the segments (ld_feat padding) are never read.
// Norms are written for the first `nrows` rows, segment s at nsq + s * nrows: rml_gram (one segment) takes them for every padded
// row, rml_gram_segments for the caller's N.
__global__ __launch_bounds__(256) void k_gram_prep(const float* __restrict__ feat, int64_t ld_feat, int64_t N, SegLayout L,
                                                   float* __restrict__ a, int64_t lda, double* __restrict__ nsq, int64_t nrows) {
    __shared__ double red[256];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const bool valid = r < N;
    for (int s = 0; s < L.nseg; ++s) {
        double acc = 0.0;
        for (int64_t d = tid; d < L.plen[s]; d += 256) {
            const float v = (valid && d < L.len[s]) ? feat[r * ld_feat + L.src[s] + d] : 0.0f;
            a[r * lda + L.dst[s] + d] = v;
            acc = fma((double)v, (double)v, acc);
        }
        red[tid] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0 && r < nrows) nsq[(int64_t)s * nrows + r] = red[0];
        __syncthreads();
    }
}

// The symmetric tile of block b: the inner products of the padded rows of its tile pair over K-steps [kt0, kt1), each handed to
// put(out_row, out_col, rl, cl, g) -- g of tile-local (row rl, column cl) for the output element (out_row, out_col) -- once as
// itself and once mirrored.  begin(r0, c0) runs before the K loop with the first row of the two tiles; LDS past kTileLds is the
// caller's.
template <class Begin, class Put>
__device__ __forceinline__ void gram_tile(unsigned char* smem, const float* a, int64_t lda, int64_t N, int kt0, int kt1, Begin begin,
                                          Put put) {
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
    begin(r0, c0);

    TileStager sg;
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(a);
    sg.init<false>(rows, lda * 4, r0, rows, lda * 4, c0, 0, wave, lane);
    Frag64 fa, fb;
    fa.init(wr * 64, lane); fb.init(wc * 64, lane);
    const int kgrp = lane >> 4;
    v4d acc[4][4];
    zero_acc(acc);
    tile_k_loop(sg, smem, kt0, kt1, [&](const unsigned char* sA, const unsigned char* sB) { kstep_f64(acc, sA, sB, fa, fb, kgrp); });

    // ---- epilogue: one row half (64 rows x 128 columns of G) at a time through LDS ----
    double* gd = reinterpret_cast<double*>(smem);      // [64][kLdG]
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
        // direct store [r0 + rl][c0 + cl]: lanes on consecutive columns
        {
            const int cl = tid & 127;
            const int64_t col = c0 + cl;
            for (int s = 0; s < kHalfRows / 2; ++s) {
                const int hl = (tid >> 7) + 2 * s;
                const int rl = pass * kHalfRows + hl;
                const int64_t row = r0 + rl;
                if (row >= N || col >= N || (diag && rl > cl)) continue;
                put(row, col, rl, cl, gd[hl * kLdG + cl]);
            }
        }
        // mirrored store [c0 + cl][r0 + rl]: lanes on consecutive rows of the half (= consecutive columns of the mirror)
        {
            const int hl = tid & 63;
            const int rl = pass * kHalfRows + hl;
            const int64_t row = r0 + rl;
            for (int s = 0; s < kTile / 4; ++s) {
                const int cl = (tid >> 6) + 4 * s;
                const int64_t col = c0 + cl;
                if (row >= N || col >= N || (diag && rl >= cl)) continue;
                put(col, row, rl, cl, gd[hl * kLdG + cl]);
            }
        }
    }
}

// the kernel value of one element from its inner product g and squared distance d2; gk = gamma, or -1 for the linear kernel
__device__ __forceinline__ double gram_value(double g, double d2, double gk) { return gk < 0.0 ? g : exp(-gk * d2); }

__global__ __launch_bounds__(256, 2) void k_gram(GramArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    // row norms of the two tiles and the kernels' gammas (-1: linear), behind gram_tile's LDS
    double* tn = reinterpret_cast<double*>(smem + kTileLds);
    double* kg = tn + 2 * kTile;
    const int tid = threadIdx.x;
    gram_tile(smem, a.a, a.lda, a.N, 0, a.KT,
              [&](int64_t r0, int64_t c0) {
                  tn[tid] = a.nsq[(tid < kTile ? r0 : c0 - kTile) + tid];
                  if (tid < a.nk) kg[tid] = a.kind[tid] == RML_GRAM_LINEAR ? -1.0 : a.gamma[tid];
              },
              [&](int64_t row, int64_t col, int rl, int cl, double g) {
                  const double d2 = (tn[rl] + tn[kTile + cl]) - 2.0 * g;
                  double* o = a.out + row * a.ld_out + col;
                  for (int k = 0; k < a.nk; ++k) o[k * a.stride_k] = gram_value(g, d2, kg[k]);
              });
}

__global__ __launch_bounds__(256, 2) void k_gseg(SegArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int seg = a.seg[blockIdx.y];
    double* out = a.G + (int64_t)seg * a.stride_s;
    gram_tile(smem, a.a, a.lda, a.N, a.kt0[seg], a.kt1[seg], [](int64_t, int64_t) {},
              [&](int64_t row, int64_t col, int, int, double g) { out[row * a.ld_g + col] = g; });
}

// outputs of ONE mask: thread = column j, blockIdx.y strides the rows
__global__ __launch_bounds__(256) void k_gram_compose(ComposeArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.N) return;
    double nj = 0.0;
    bool first = true;
    for (int s = 0; s < a.nseg; ++s)
        if (a.bits >> s & 1u) {
            const double v = a.nsq[(int64_t)s * a.N + j];
            nj = first ? v : nj + v;
            first = false;
        }
    for (int64_t i = blockIdx.y; i < a.N; i += gridDim.y) {
        double g = 0.0, ni = 0.0;
        first = true;
        for (int s = 0; s < a.nseg; ++s)
            if (a.bits >> s & 1u) {
                const double gs = a.G[(int64_t)s * a.stride_s + i * a.ld_g + j];
                const double ns = a.nsq[(int64_t)s * a.N + i];
                g = first ? gs : g + gs;
                ni = first ? ns : ni + ns;
                first = false;
            }
        const double d2 = (ni + nj) - 2.0 * g;
        for (int k = 0; k < a.nk; ++k)
            a.out[(int64_t)a.kidx[k] * a.stride_k + i * a.ld_out + j] = gram_value(g, d2, a.gamma[k]);
    }
}

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// entry k of a kinds / gammas list of the entry point `fn`
int check_kind(const char* fn, int k, int kind, double gamma) {
    RML_REQUIRE(kind == RML_GRAM_LINEAR || kind == RML_GRAM_RBF, RML_ERR_INVALID, "%s: unknown kind %d (entry %d)", fn, kind, k);
    RML_REQUIRE(kind == RML_GRAM_LINEAR || (isfinite(gamma) && gamma >= 0.0), RML_ERR_INVALID,
                "%s: gamma[%d] = %g is not a finite non-negative number", fn, k, gamma);
    return RML_OK;
}

}  // namespace

extern "C" int rml_gram(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int64_t D,
                        int nk, const int* kinds, const double* gammas,
                        double* out, int64_t ld_out, int64_t stride_k, void* stream) {
    RML_REQUIRE(ctx && kinds && gammas, RML_ERR_INVALID, "rml_gram: NULL argument");
    RML_REQUIRE(N >= 0 && D >= 1, RML_ERR_INVALID, "rml_gram: bad shape N=%lld D=%lld", (long long)N, (long long)D);
    RML_REQUIRE(nk >= 1 && nk <= kMaxKinds, RML_ERR_INVALID, "rml_gram: nk=%d outside [1, %d]", nk, kMaxKinds);
    for (int k = 0; k < nk; ++k)
        if (int rc = check_kind("rml_gram", k, kinds[k], gammas[k])) return rc;
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
    SegLayout L{};                                     // the rows as one segment; norms of all padded rows
    L.nseg = 1; L.len[0] = D; L.plen[0] = lda;
    hipLaunchKernelGGL(k_gram_prep, dim3((unsigned)Np), dim3(256), 0, st, feat, ld_feat, N, L, a, lda, nsq, Np);
    RML_HIP(hipGetLastError());
    GramArgs g{};
    g.a = a; g.lda = lda; g.nsq = nsq;
    g.KT = (int)(lda / kStepFloats);
    g.N = N; g.nk = nk;
    for (int k = 0; k < nk; ++k) { g.kind[k] = kinds[k]; g.gamma[k] = kinds[k] == RML_GRAM_LINEAR ? 0.0 : gammas[k]; }
    g.out = out; g.ld_out = ld_out; g.stride_k = stride_k;
    RML_MAX_DYN_LDS(kGramLds, k_gram);
    hipLaunchKernelGGL(k_gram, dim3((unsigned)(NT * (NT + 1) / 2)), dim3(256), kGramLds, st, g);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

extern "C" int rml_gram_segments(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int nseg, const int64_t* seg_len,
                                 double* G, int64_t ld_g, int64_t stride_s, double* nsq, void* stream) {
    RML_REQUIRE(ctx && seg_len, RML_ERR_INVALID, "rml_gram_segments: NULL argument");
    RML_REQUIRE(N >= 0, RML_ERR_INVALID, "rml_gram_segments: bad shape N=%lld", (long long)N);
    RML_REQUIRE(nseg >= 1 && nseg <= kMaxSeg, RML_ERR_INVALID, "rml_gram_segments: nseg=%d outside [1, %d]", nseg, kMaxSeg);
    int64_t D = 0;
    for (int s = 0; s < nseg; ++s) {
        RML_REQUIRE(seg_len[s] >= 1 && seg_len[s] < ((int64_t)1 << 31) - kStepFloats, RML_ERR_INVALID,
                    "rml_gram_segments: seg_len[%d] = %lld is not a positive length", s, (long long)seg_len[s]);
        D += seg_len[s];
    }
    RML_REQUIRE(ld_feat >= D, RML_ERR_INVALID, "rml_gram_segments: ld_feat=%lld < sum of seg_len=%lld", (long long)ld_feat, (long long)D);
    RML_REQUIRE(ld_g >= N, RML_ERR_INVALID, "rml_gram_segments: ld_g=%lld < N=%lld", (long long)ld_g, (long long)N);
    RML_REQUIRE(stride_s >= N * ld_g, RML_ERR_INVALID, "rml_gram_segments: stride_s=%lld < N*ld_g=%lld", (long long)stride_s,
                (long long)(N * ld_g));
    if (N == 0) return RML_OK;
    RML_REQUIRE(feat && G && nsq, RML_ERR_INVALID, "rml_gram_segments: NULL argument");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);                      // shared workspace
    SegLayout L{};
    SegArgs g{};
    L.nseg = nseg;
    int64_t lda = 0;
    for (int s = 0; s < nseg; ++s) {
        L.len[s] = seg_len[s];
        L.src[s] = s ? L.src[s - 1] + seg_len[s - 1] : 0;
        L.dst[s] = lda;
        L.plen[s] = round_up(seg_len[s], kStepFloats);
        g.kt0[s] = (int)(lda / kStepFloats);
        lda += L.plen[s];
        g.kt1[s] = (int)(lda / kStepFloats);
        // longest first (stable): the long K loops start before the short ones fill the remaining slots
        int p = s;
        for (; p > 0 && seg_len[g.seg[p - 1]] < seg_len[s]; --p) g.seg[p] = g.seg[p - 1];
        g.seg[p] = s;
    }
    const int64_t Np = round_up(N, kTile);
    const int64_t NT = Np / kTile;
    RML_REQUIRE(NT * (NT + 1) / 2 < (int64_t)1 << 31, RML_ERR_INVALID, "rml_gram_segments: N=%lld is too large", (long long)N);
    void* ws = nullptr;
    int rc = rml_ws_reserve(ctx, (size_t)(Np * lda * 4), &ws, st);
    if (rc) return rc;
    float* a = static_cast<float*>(ws);
    hipLaunchKernelGGL(k_gram_prep, dim3((unsigned)Np), dim3(256), 0, st, feat, ld_feat, N, L, a, lda, nsq, N);
    RML_HIP(hipGetLastError());
    g.a = a; g.lda = lda; g.N = N;
    g.G = G; g.ld_g = ld_g; g.stride_s = stride_s;
    RML_MAX_DYN_LDS(kTileLds, k_gseg);
    hipLaunchKernelGGL(k_gseg, dim3((unsigned)(NT * (NT + 1) / 2), (unsigned)nseg), dim3(256), kTileLds, st, g);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

extern "C" int rml_gram_compose(rml_ctx* ctx, const double* G, int64_t ld_g, int64_t stride_s, const double* nsq, int64_t N, int nseg,
                                int n_out, const int* seg_bits, const int* kinds, const double* gammas,
                                double* out, int64_t ld_out, int64_t stride_k, void* stream) {
    RML_REQUIRE(ctx && seg_bits && kinds && gammas, RML_ERR_INVALID, "rml_gram_compose: NULL argument");
    RML_REQUIRE(N >= 0, RML_ERR_INVALID, "rml_gram_compose: bad shape N=%lld", (long long)N);
    RML_REQUIRE(nseg >= 1 && nseg <= kMaxSeg, RML_ERR_INVALID, "rml_gram_compose: nseg=%d outside [1, %d]", nseg, kMaxSeg);
    RML_REQUIRE(n_out >= 1, RML_ERR_INVALID, "rml_gram_compose: n_out=%d < 1", n_out);
    for (int k = 0; k < n_out; ++k) {
        RML_REQUIRE(seg_bits[k] > 0 && seg_bits[k] < (1 << nseg), RML_ERR_INVALID,
                    "rml_gram_compose: seg_bits[%d] = %d is not a non-empty subset of %d segments", k, seg_bits[k], nseg);
        if (int rc = check_kind("rml_gram_compose", k, kinds[k], gammas[k])) return rc;
    }
    RML_REQUIRE(ld_g >= N, RML_ERR_INVALID, "rml_gram_compose: ld_g=%lld < N=%lld", (long long)ld_g, (long long)N);
    RML_REQUIRE(stride_s >= N * ld_g, RML_ERR_INVALID, "rml_gram_compose: stride_s=%lld < N*ld_g=%lld", (long long)stride_s,
                (long long)(N * ld_g));
    RML_REQUIRE(ld_out >= N, RML_ERR_INVALID, "rml_gram_compose: ld_out=%lld < N=%lld", (long long)ld_out, (long long)N);
    RML_REQUIRE(stride_k >= N * ld_out, RML_ERR_INVALID, "rml_gram_compose: stride_k=%lld < N*ld_out=%lld", (long long)stride_k,
                (long long)(N * ld_out));
    if (N == 0) return RML_OK;
    RML_REQUIRE(G && nsq && out, RML_ERR_INVALID, "rml_gram_compose: NULL argument");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    ComposeArgs c{};
    c.G = G; c.ld_g = ld_g; c.stride_s = stride_s; c.nsq = nsq; c.N = N; c.nseg = nseg;
    c.out = out; c.ld_out = ld_out; c.stride_k = stride_k;
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)(N < 65535 ? N : 65535));
    // one launch per mask and up to kMaxOut of its outputs: g and d2 are formed once per element and mask
    std::vector<char> done((size_t)n_out, 0);
    for (int k0 = 0; k0 < n_out; ++k0) {
        if (done[k0]) continue;
        c.bits = (unsigned)seg_bits[k0];
        c.nk = 0;
        for (int k = k0; k < n_out; ++k) {
            if (done[k] || seg_bits[k] != seg_bits[k0]) continue;
            c.kidx[c.nk] = k;
            c.gamma[c.nk] = kinds[k] == RML_GRAM_LINEAR ? -1.0 : gammas[k];
            done[k] = 1;
            if (++c.nk == kMaxOut) {
                hipLaunchKernelGGL(k_gram_compose, grid, dim3(256), 0, st, c);
                RML_HIP(hipGetLastError());
                c.nk = 0;
            }
        }
        if (c.nk) {
            hipLaunchKernelGGL(k_gram_compose, grid, dim3(256), 0, st, c);
            RML_HIP(hipGetLastError());
        }
    }
    return RML_OK;
}
