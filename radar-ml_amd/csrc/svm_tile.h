// RBF / linear C-SVC decision function on gfx950 matrix cores.
//
// Reference arithmetic replaced (sk: = scikit-learn, the reference's SVM dependency):
//   sk:svm/src/libsvm/svm.cpp:461-475,514   K[n,m] = exp(-gamma * ||x_n - sv_m||^2)      (RBF)
//   sk:svm/src/libsvm/svm.cpp:457            K[n,m] = x_n . sv_m                          (linear)
//   sk:svm/src/libsvm/svm.cpp:2847-2890      dec[n,p] = sum_m coef*K - rho[p]; OvO vote
//   sk:utils/multiclass.py:542-584           ovr = votes + s/(3(|s|+1))
//   sk:calibration.py:727-784,928-942        expit(-(a*T+b)), normalise, clip, argmax
// called from train.py:217,723-724 and predict.py:60.
//
// libsvm walks samples x SVs x D serially in float64.  Here the sample x SV inner products are
// one GEMM on the matrix cores and everything after it is a fused float64 epilogue; the N x M
// kernel matrix never exists in memory.
//
//   ||x - s||^2 = ||x||^2 + ||s||^2 - 2 x.s
//
// Three operand paths share one kernel skeleton (tiles staged by LDS-DMA, 128-byte rows: mfma_tile.h):
//   I8   radar features are integer codes c in [0,255] (optionally scaled by 1/255), so
//        x.s is EXACT in int32 on v_mfma_i32_32x32x32_i8.  Codes are stored biased
//        (byte = c ^ 0x80 = int8 c-128):  sum (a-128)(b-128) = sum ab - 128 (sum a + sum b) + 128^2 D.
//        d^2 is then an exact integer, evaluated in float64.
//   F64  general rows (anything not on the code grid: augmented / zoomed data) on
//        v_mfma_f64_16x16x4_f64: the float32 operands are widened to float64 in registers, the
//        products and the accumulation are float64 -- the arithmetic class of libsvm itself, at
//        the f64 matrix rate (78.6 TF).  This is what RML_PATH_AUTO uses for non-grid rows.
//        It runs the staging, K loop and f64 K-step that k_gram runs (mfma_tile.h) at an accepted cost of up to two
//        VGPRs on five of its ten instantiations, inside the 256 that two workgroups per CU leave a lane.
//   F32  opt-in approximate path on v_mfma_f32_32x32x2_f32 (f32 accumulate, 2x the F64 rate;
//        measured error of the decision values ~1e-4..1e-3, i.e. outside the 1e-5 bar).
// Epilogue (float64): K = exp(-gamma d^2); per-pair weights W[p][m] (the libsvm pair loop
// unrolled into a P x M matrix at load) -> S[n][p] += W[p][m] K.  The MFMA is issued with the
// SV tile as the A (row) operand and the sample tile as the B (column) operand, so that a lane
// owns ONE sample column and 16 SV rows per accumulator: the sum over SVs is in-lane, only a
// 2-lane + 2-wave reduction per workgroup remains.  Per-SV-tile partial sums are written to
// HBM (ST x N x P float64, fixed order) and summed by the finishing kernel in tile order, so
// results are deterministic run to run.
//
// Workgroup tile 128 SVs x 128 samples, 4 waves as 2x2, each wave 2x2 MFMA tiles of 32x32.
// K-step = 128 bytes per row (128 codes or 32 floats).  LDS image of a tile: row-major
// [128 rows][128 B] with the 16-byte chunk index XOR-swizzled by (row>>1)&7, which makes the
// ds_read_b128 fragment reads (lane = row, 16 B each) bank-conflict free.  LDS-DMA writes
// lane-linear, so the swizzle is applied to the per-lane GLOBAL source address and again on
// the read (both-sides rule).  Double-buffered: the DMA of K-step t+1 is in flight while the
// MFMAs of K-step t run.  Block index -> (sample tile, SV tile) is XCD-aware: the 16 SV tiles
// that share a sample tile run on one XCD so the sample K-slices are L2 hits.
//
// This file: the 128 x 128 tile kernel and its split-K companion.  The other kernels of the SVM path: svm_ring.h (256 x 256 ring),
// svm_small.h (single observations and the split-K epilogue), svm_rows.h (row preparation, tile flags), svm_finish.h (vote, Platt,
// linear); the arithmetic every epilogue shares: svm_epilogue.h; the host side: svm.hip.
#pragma once
#include "mfma_tile.h"
#include "svm_epilogue.h"
#include <type_traits>

namespace {

struct GemmArgs {
    const uint8_t* sv; int64_t ld_sv;     // SV operand, bytes per row
    const uint8_t* x;  int64_t ld_x;      // sample operand, bytes per row
    int KT;                                // K-steps
    int64_t N;                             // valid sample rows
    int ST, FT;                            // SV tiles, sample tiles
    const int32_t* tile_exact; int want;   // process sample tile ft iff tile_exact[ft] == want (NULL: all)
    const int32_t* x_isum; const int64_t* x_isq;   // exact path row statistics
    const double* x_nsq;                            // f32 path row norms
    const double* sv_term;                 // Mpad per-SV term (path/kernel specific)
    const double* W; int64_t Mpad;         // PT x Mpad pair weights
    double gs;                             // gamma/scale^2 (rbf) ; 1/scale^2 (linear, exact path)
    int kernel;
    double* partial; int64_t Npart;        // ST x Npart x PT
    double* kmat; int64_t ld_k; int64_t M; // KM instantiations: kernel values K[n][m] for m < M (rml_svm_kernel_matrix)
    int64_t sv_rows;                       // SV rows that exist in memory (Mpad); the 256-row kernel clamps to it
    // SPARSE instantiation (mfma_tile.h SparseStager): occupancy words of the SV rows and of the sample rows, `ow` dwords per row, and
    // the context's line of background codes
    const uint32_t* sv_occ; const uint32_t* x_occ; int ow; const uint8_t* bg_line;
};

template <int PATH, int PT, bool KM = false, bool SPARSE = false>
__global__ __launch_bounds__(256, 2) void k_svm_gemm(GemmArgs a) {
    static_assert(!SPARSE || (PATH == PATH_I8 && !KM), "occupancy words exist for code rows only");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3;
    // an XCD owns the sample tiles {xcd, xcd+8, ...} and walks them FASTEST, so the workgroups resident on an
    // XCD form an (all its sample tiles) x (few SV tiles) block sharing K-slices through that XCD's L2
    // (measured with TCC_HIT/MISS: L2 misses -30 % vs walking the SV tiles fastest)
    const int XPX = (a.FT + 7) >> 3;
    const int ftile = (slot % XPX) * 8 + xcd;
    const int stile = slot / XPX;
    if (ftile >= a.FT) return;
    if (a.tile_exact && a.tile_exact[ftile] != a.want) return;
    const int64_t f0 = (int64_t)ftile * kTile;
    const int64_t m0 = (int64_t)stile * kTile;

    // per-SV epilogue table in LDS behind the four tile images
    double* svw = reinterpret_cast<double*>(smem + 4 * kTileBytes);
    const double* etab = load_sv_table<PT, kTile, 256, false>(svw, a.sv_term, a.W, a.Mpad, m0, tid);

    auto store_k = [&](int64_t n, int ml, double kv) {      // KM: the kernel value of (sample n, SV row ml of this tile)
        if constexpr (KM) {
            const int64_t mg = (int64_t)stile * kTile + ml;
            if (n < a.N && mg < a.M) a.kmat[n * a.ld_k + mg] = kv;
        }
    };

    if constexpr (PATH == PATH_F64) {
        TileStager sg;
        sg.init<true>(a.sv, a.ld_sv, m0, a.x, a.ld_x, f0, a.N, wave, lane);
        // accumulators: 4x4 tiles of 16x16 (4 doubles each)
        Frag64 fa, fb;
        fa.init(wr * 64, lane); fb.init(wc * 64, lane);
        const int kgrp = lane >> 4;
        v4d accd[4][4];
        zero_acc(accd);
        tile_k_loop(sg, smem, 0, a.KT, [&](const unsigned char* sA, const unsigned char* sB) { kstep_f64(accd, sA, sB, fa, fb, kgrp); });

        const bool rbf = (a.kernel == RML_KERNEL_RBF);
        // float64 accumulators: 128 x 128 x 8 B = 128 KiB, so the LDS round trip is done in two column
        // halves of 64 KiB (the waves with wc == pass own that half).  Thread t then owns sample column
        // n' = t & 63 of the half and the SV quarter t >> 6 (32 in-lane SV rows).
        double* gd = reinterpret_cast<double*>(smem);
        const int nq = tid & 63, qd = tid >> 6;
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();
            if (wc == pass) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ml = cd64_row(wr * 64 + i * 16, r, lane);
                            const int nl = cd64_col(j * 16, lane);
                            gd[ml * 64 + nl] = accd[i][j][r];
                        }
            }
            __syncthreads();
            const int64_t n = f0 + pass * 64 + nq;
            const int64_t nc = n < a.N ? n : a.N - 1;
            const double xt = rbf ? a.x_nsq[nc] : 0.0;
            double S[PT];
            chain_run<PT, 32, false>(S, svw, qd * 32, rbf, xt, a.gs, etab, [&](int ml) { return gd[ml * 64 + nq]; },
                                     [&](int ml, double kv) { store_k(n, ml, kv); });
            __syncthreads();                   // G half consumed: reuse its LDS for the exchange
            double* x4 = gd;                   // [4 quarters][64][PT]
#pragma unroll
            for (int p = 0; p < PT; ++p) x4[(qd * 64 + nq) * PT + p] = S[p];
            __syncthreads();
            if (qd == 0 && n < a.N) {
#pragma unroll
                for (int p = 0; p < PT; ++p) {
                    double t = x4[(0 * 64 + nq) * PT + p] + x4[(1 * 64 + nq) * PT + p];
                    t += x4[(2 * 64 + nq) * PT + p] + x4[(3 * 64 + nq) * PT + p];
                    a.partial[((int64_t)stile * a.Npart + n) * PT + p] = t;
                }
            }
        }
    } else {
        // accumulators: 2x2 tiles of 32x32 (16 regs each)
        using acc_t = typename std::conditional<PATH == PATH_I8, v16i, v16f>::type;
        Frag32<2> fa, fb;
        fa.init(wr * 64, lane); fb.init(wc * 64, lane);
        const int chalf = lane >> 5;
        acc_t acc[2][2];
        zero_acc(acc);
        auto ks32 = [&](const unsigned char* sA, const unsigned char* sB) { kstep_32<PATH>(acc, sA, sB, fa, fb, chalf); };
        if constexpr (SPARSE) {
            // the tile's occupancy words behind the epilogue tables (launch_gemm asks for the bytes)
            uint32_t* occ_l = reinterpret_cast<uint32_t*>(smem + 4 * kTileBytes + kTile * (1 + PT) * sizeof(double) + kExpTabBytes);
            SparseStager::fill(occ_l, a.sv_occ, m0, a.x_occ, f0, a.N, a.ow, tid);
            __syncthreads();
            SparseStager sg;
            sg.init(a.sv, a.ld_sv, m0, a.x, a.ld_x, f0, a.N, occ_l, a.ow, a.bg_line, wave, lane);
            tile_k_loop(sg, smem, 0, a.KT, ks32);
        } else {
            TileStager sg;
            sg.init<true>(a.sv, a.ld_sv, m0, a.x, a.ld_x, f0, a.N, wave, lane);
            tile_k_loop(sg, smem, 0, a.KT, ks32);
        }

        const bool rbf = (a.kernel == RML_KERNEL_RBF);
        // ---- fused float64 epilogue ----------------------------------------------------------
        // The accumulators go through LDS once (the four 16 KiB tile images are free now and are
        // exactly 128 x 128 x 4 B) so that the epilogue can use its own thread mapping: thread t
        // owns sample column n = t & 127 and the SV half h = t >> 7, i.e. 64 in-lane SV rows, reads
        // G[m][n] with consecutive lanes on consecutive banks and the per-SV table as broadcasts.
        __syncthreads();                           // everyone is done reading the tile images
        {
            int* gl = reinterpret_cast<int*>(smem);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ml = cd32_row(wr * 64 + i * 32, r, lane);
                        const int nl = cd32_col(wc * 64 + j * 32, lane);
                        int bits;
                        if constexpr (PATH == PATH_I8) bits = acc[i][j][r]; else bits = __float_as_int(acc[i][j][r]);
                        gl[ml * kTile + nl] = bits;
                    }
        }
        __syncthreads();
        const int nl = tid & 127, h = tid >> 7;
        int64_t n = f0 + nl;
        const int64_t nc = n < a.N ? n : a.N - 1;
        double xt;
        if constexpr (PATH == PATH_I8) xt = exact_sample_term(rbf, a.x_isum, a.x_isq, nc);
        else xt = rbf ? a.x_nsq[nc] : 0.0;
        double S[PT];
        const int* gcol = reinterpret_cast<const int*>(smem) + nl;
        chain_run<PT, 64, PATH == PATH_I8>(S, svw, h * 64, rbf, xt, a.gs, etab,
                                          [&](int ml) {
                                              const int bits = gcol[ml * kTile];
                                              return (PATH == PATH_I8) ? (double)bits : (double)__int_as_float(bits);
                                          },
                                          [&](int ml, double kv) { store_k(n, ml, kv); });
        // [128][PT] cross-thread exchange, over the tile images once they are consumed: the request stays at 4 tiles + the SV table
        // (69 632 B for three pairs; with the exchange behind the table it was 72 704 B.  Same-box A/B of the fused pipeline at
        // 64x64x128: +2 % with the smaller request, the byte-native rows unchanged)
        double* xch = reinterpret_cast<double*>(smem);
        __syncthreads();                           // G consumed: its LDS carries the exchange between the two SV halves
        if (h == 1) {
#pragma unroll
            for (int p = 0; p < PT; ++p) xch[nl * PT + p] = S[p];
        }
        __syncthreads();
        if (h == 0 && n < a.N) {
#pragma unroll
            for (int p = 0; p < PT; ++p) a.partial[((int64_t)stile * a.Npart + n) * PT + p] = S[p] + xch[nl * PT + p];
        }
    }
}

// ------------------------------------------------------------------------------------------
// Batches that do not fill the machine with 128 x 128 tiles (9 .. ~1 500 rows: what train.py's `clf.predict(X_test)` and a
// few dozen observations look like): FT x ST tiles are 21 .. 250 workgroups on 256 CUs, each walking all 160 K-steps -- 104 us
// for 64 rows, whatever their number.  The int32 dot products are EXACT, so K may be cut anywhere and the pieces added in any
// order: k_svm_gemm_splitk gives every (tile, K range) a workgroup -- the tile kernel's staging and MFMA loop over its range -- and
// adds its accumulators into G[m][n] with int32 atomics (lanes run along n: whole 128-byte requests); k_svm_epi_small then forms the
// kernel values and the partial sums in the tile kernels' order.  Bit-identical decision values, asserted with the small path.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_zero16(v4i* p, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = v4i{0, 0, 0, 0};
}

struct SplitArgs {
    const uint8_t* sv; int64_t ld_sv;
    const uint8_t* x; int64_t ld_x;
    int KT, per;                               // K-steps in all, per K range
    int64_t N; int FT;
    const int32_t* tile_exact;
    int32_t* G; int64_t ldg;                   // [Mpad][ldg] (zeroed by the caller), ldg = FT * 128
};

__global__ __launch_bounds__(256, 2) void k_svm_gemm_splitk(SplitArgs a) {
    __shared__ __align__(16) unsigned char smem[4 * kTileBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int ftile = blockIdx.x % a.FT, stile = blockIdx.x / a.FT;
    if (a.tile_exact && a.tile_exact[ftile] != 1) return;
    const int kt0 = blockIdx.y * a.per;
    const int kt1 = a.KT < kt0 + a.per ? a.KT : kt0 + a.per;
    if (kt0 >= kt1) return;
    const int64_t f0 = (int64_t)ftile * kTile, m0 = (int64_t)stile * kTile;
    TileStager sg;
    sg.init<true>(a.sv, a.ld_sv, m0, a.x, a.ld_x, f0, a.N, wave, lane);
    Frag32<2> fa, fb;
    fa.init(wr * 64, lane); fb.init(wc * 64, lane);
    const int chalf = lane >> 5;
    v16i acc[2][2];
    zero_acc(acc);
    auto ks = [&](const unsigned char* sA, const unsigned char* sB) { kstep_i8_plain(acc, sA, sB, fa, fb, chalf); };
    tile_k_loop(sg, smem, kt0, kt1, ks);
    // the lanes of an atomic run along n (the C/D map's column)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = cd32_row(wr * 64 + i * 32, r, lane);
                const int nl = cd32_col(wc * 64 + j * 32, lane);
                __hip_atomic_fetch_add(a.G + (m0 + ml) * a.ldg + f0 + nl, acc[i][j][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
}

template <int PATH, bool KM = false, bool SPARSE = false>
int launch_gemm(const rml_svm* m, const GemmArgs& ga, hipStream_t st) {
    const size_t lds = 4 * kTileBytes + (size_t)kTile * (1 + m->PT) * sizeof(double) + kExpTabBytes + (SPARSE ? (size_t)2 * kTile * ga.ow * 4 : 0);
    const int FT8 = (ga.FT + 7) / 8 * 8;
    dim3 grid((unsigned)(FT8 * ga.ST)), block(256);
#define RML_GEMM_CASE(PTV)                                                                                         \
    case PTV: {                                                                                                    \
        RML_MAX_DYN_LDS(144 * 1024, &k_svm_gemm<PATH, PTV, KM, SPARSE>);                                           \
        hipLaunchKernelGGL((k_svm_gemm<PATH, PTV, KM, SPARSE>), grid, block, lds, st, ga);                         \
    } break;
    switch (m->PT) {
        RML_GEMM_CASE(1)
        RML_GEMM_CASE(3)
        RML_GEMM_CASE(6)
        RML_GEMM_CASE(10)
        RML_GEMM_CASE(15)
        default: RML_REQUIRE(false, RML_ERR_UNSUPPORTED, "svm: unsupported pair count");
    }
#undef RML_GEMM_CASE
    RML_HIP(hipGetLastError());
    return RML_OK;
}

}  // namespace
