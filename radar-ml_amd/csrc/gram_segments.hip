// Inner products of one set of rows against itself, kept apart per column segment (rml_gram_segments), and the kernel matrices
// of any union of segments composed from them (rml_gram_compose): the Gram service of an SVC search over projection masks.
//
// A feature row of the reference is concat(xz, yz, xy) (common.py: the ProjMask picks which projections are concatenated), so for
// a mask the inner products and squared norms are sums of the per-projection ones:
//   G_mask = sum_{s in mask} G_s        |x|^2_mask = sum_{s in mask} |x|^2_s
// and sk:svm/src/libsvm/svm.cpp:457 (linear) / 461-475 (RBF) follow from them as in gram.hip.  One pass over the rows gives every
// mask x kernel matrix of the search.
//
// k_gseg is k_gram's K loop (mfma_tile.h: float32 rows widened in registers, exact products, float64 accumulation on
// v_mfma_f64_16x16x4_f64, 128 x 128 tiles, upper-triangle tile pairs, mirrored stores) run over the K-steps of ONE segment:
// grid = tile pairs x segments, the longest segment dispatched first.  k_gseg_prep pads every segment of the copy to a whole
// number of K-steps with zeros, so no K-step straddles a segment.  Segments are not cut into K pieces: every element is one
// accumulator chain in ascending k, no partial sums, no atomics.
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
constexpr int kLdsBytes = kGBytes > 4 * kTileBytes ? kGBytes : 4 * kTileBytes;
constexpr int kMaxSeg = 8;
constexpr int kMaxOut = 8;                          // outputs of one mask per k_gram_compose launch

struct SegLayout {
    int nseg;
    int len[kMaxSeg];                               // columns of the segment
    int64_t src[kMaxSeg];                           // its first column in the caller's rows
    int64_t dst[kMaxSeg];                           // ... in the padded copy (a multiple of 32)
    int64_t plen[kMaxSeg];                          // its padded length
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
__global__ __launch_bounds__(256) void k_gseg_prep(const float* __restrict__ feat, int64_t ld_feat, int64_t N, SegLayout L,
                                                   float* __restrict__ a, int64_t lda, double* __restrict__ nsq) {
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
        if (tid == 0 && valid) nsq[(int64_t)s * N + r] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256, 2) void k_gseg(SegArgs a) {
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
    const int seg = a.seg[blockIdx.y];

    TileStager sg;
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(a.a);
    sg.init<false>(rows, a.lda * 4, r0, rows, a.lda * 4, c0, 0, wave, lane);
    Frag64 fa, fb;
    fa.init(wr * 64, lane); fb.init(wc * 64, lane);
    const int kgrp = lane >> 4;
    v4d acc[4][4];
    zero_acc(acc);
    tile_k_loop(sg, smem, a.kt0[seg], a.kt1[seg],
                [&](const unsigned char* sA, const unsigned char* sB) { kstep_f64(acc, sA, sB, fa, fb, kgrp); });

    // ---- epilogue: one row half (64 rows x 128 columns of G) at a time through LDS, as k_gram ----
    double* gd = reinterpret_cast<double*>(smem);      // [64][kLdG]
    double* out = a.G + (int64_t)seg * a.stride_s;
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
        // direct store G[r0 + rl][c0 + cl]: lanes on consecutive columns
        {
            const int cl = tid & 127;
            const int64_t col = c0 + cl;
            for (int s = 0; s < kHalfRows / 2; ++s) {
                const int hl = (tid >> 7) + 2 * s;
                const int rl = pass * kHalfRows + hl;
                const int64_t row = r0 + rl;
                if (row >= a.N || col >= a.N || (diag && rl > cl)) continue;
                out[row * a.ld_g + col] = gd[hl * kLdG + cl];
            }
        }
        // mirrored store G[c0 + cl][r0 + rl]: lanes on consecutive rows of the half (= consecutive columns of the mirror)
        {
            const int hl = tid & 63;
            const int rl = pass * kHalfRows + hl;
            const int64_t row = r0 + rl;
            for (int s = 0; s < kTile / 4; ++s) {
                const int cl = (tid >> 6) + 4 * s;
                const int64_t col = c0 + cl;
                if (row >= a.N || col >= a.N || (diag && rl >= cl)) continue;
                out[col * a.ld_g + row] = gd[hl * kLdG + cl];
            }
        }
    }
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
        for (int k = 0; k < a.nk; ++k) {
            const double gk = a.gamma[k];
            a.out[(int64_t)a.kidx[k] * a.stride_k + i * a.ld_out + j] = gk < 0.0 ? g : exp(-gk * d2);
        }
    }
}

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

}  // namespace

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
        L.len[s] = (int)seg_len[s];
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
    hipLaunchKernelGGL(k_gseg_prep, dim3((unsigned)Np), dim3(256), 0, st, feat, ld_feat, N, L, a, lda, nsq);
    RML_HIP(hipGetLastError());
    g.a = a; g.lda = lda; g.N = N;
    g.G = G; g.ld_g = ld_g; g.stride_s = stride_s;
    RML_MAX_DYN_LDS(kLdsBytes, k_gseg);
    hipLaunchKernelGGL(k_gseg, dim3((unsigned)(NT * (NT + 1) / 2), (unsigned)nseg), dim3(256), kLdsBytes, st, g);
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
        RML_REQUIRE(kinds[k] == RML_GRAM_LINEAR || kinds[k] == RML_GRAM_RBF, RML_ERR_INVALID,
                    "rml_gram_compose: unknown kind %d (entry %d)", kinds[k], k);
        RML_REQUIRE(kinds[k] == RML_GRAM_LINEAR || (isfinite(gammas[k]) && gammas[k] >= 0.0), RML_ERR_INVALID,
                    "rml_gram_compose: gamma[%d] = %g is not a finite non-negative number", k, gammas[k]);
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
