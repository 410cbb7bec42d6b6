// Single observations and small batches on the exact path: int8 dot products into G[m][n] (k_svm_dot_small, or k_svm_gemm_splitk
// of svm_tile.h), then k_svm_epi_small forms kernel values and partial sums with the tile kernels' epilogue functions.
#pragma once
#include "mfma_tile.h"
#include "svm_epilogue.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------
// Single observations (round 6): the exact path for a handful of rows.
//
// The reference classifies ONE observation per call (predict.py:98-119).  A 128 x 128 tile kernel then launches one workgroup per
// 128 support vectors -- 21 workgroups, each streaming 2.6 MB of SV codes through one CU: 100-103 us per call
// (profiles/r06_stats_latency.txt), a twelfth of the machine.  For n <= RML_SMALL_FRAMES rows the work is a matrix-VECTOR product,
// bound by reading the SV codes once (52 MB at M = 2 562, D = 20 480): k_svm_dot_small gives every 8 SV rows a workgroup
// (Mpad / 8 = 336 of them), a thread 16 bytes of K per step, v_dot4_i32_i8 on the biased codes (the very int32 the MFMA path
// accumulates: exact, so the order does not matter), one wave reduction per (SV row, sample); k_svm_epi_small then evaluates the
// kernel values of a 128-SV tile in parallel and adds them up EXACTLY as the tile kernels do -- two chains of 64 support vectors in
// ascending order, fma(W, K, S), partial = chain 0 + chain 1 -- so decision values do not depend on which path ran (asserted:
// tests/test_svm_gpu.py::test_single_observations_take_the_small_path_with_the_same_bits).
// ------------------------------------------------------------------------------------------
struct SmallArgs {
    const uint8_t* sv; int64_t ld_sv;          // biased SV codes
    const uint8_t* x; int64_t ld_x;            // biased sample codes
    int64_t Kb;                                // bytes of K per row (a multiple of 128; pad bytes are 0 on both sides)
    int N; int64_t Mpad;
    const int32_t* tile_exact;                 // run iff NULL or tile_exact[0] == 1 (n <= 128: one sample tile)
    int32_t* G;                                // biased dot products of (SV m, sample n) at G[m * g_sm + n * g_sn]
    int64_t g_sm, g_sn;
    const int32_t* x_isum; const int64_t* x_isq;
    const double* sv_term; const double* W;
    double gs; int kernel;
    double* partial; int64_t Npart;
};

__device__ __forceinline__ int wave_sum_i32(int r) {
    auto mv = [](int v, auto ctrl, auto rowmask, auto bound) {
        return __builtin_amdgcn_update_dpp(0, v, decltype(ctrl)::value, decltype(rowmask)::value, 0xF, decltype(bound)::value);
    };
    r += mv(r, std::integral_constant<int, 0xB1>{}, std::integral_constant<int, 0xF>{}, std::true_type{});     // quad_perm [1,0,3,2]
    r += mv(r, std::integral_constant<int, 0x4E>{}, std::integral_constant<int, 0xF>{}, std::true_type{});     // quad_perm [2,3,0,1]
    r += mv(r, std::integral_constant<int, 0x141>{}, std::integral_constant<int, 0xF>{}, std::true_type{});    // row_half_mirror
    r += mv(r, std::integral_constant<int, 0x140>{}, std::integral_constant<int, 0xF>{}, std::true_type{});    // row_mirror
    r += mv(r, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{}, std::false_type{});   // row_bcast15 into rows 1, 3
    r += mv(r, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{}, std::false_type{});   // row_bcast31 into rows 2, 3
    return __builtin_amdgcn_readlane(r, 63);
}

constexpr int kSmallSv = 8;                    // SV rows per workgroup of k_svm_dot_small

template <int NS>
__global__ __launch_bounds__(256) void k_svm_dot_small(SmallArgs a) {
    if (a.tile_exact && a.tile_exact[0] != 1) return;
    __shared__ int red[4][kSmallSv * NS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * kSmallSv;
    int acc[kSmallSv][NS];
#pragma unroll
    for (int r = 0; r < kSmallSv; ++r)
#pragma unroll
        for (int n = 0; n < NS; ++n) acc[r][n] = 0;
    const uint8_t* __restrict__ xr[NS];
#pragma unroll
    for (int n = 0; n < NS; ++n) xr[n] = a.x + (int64_t)(n < a.N ? n : a.N - 1) * a.ld_x;
    const uint8_t* __restrict__ svr = a.sv + m0 * a.ld_sv;
#pragma unroll 2
    for (int64_t off = (int64_t)tid * 16; off < a.Kb; off += 256 * 16) {
        v4i xs[NS], ss[kSmallSv];
#pragma unroll
        for (int r = 0; r < kSmallSv; ++r) ss[r] = *reinterpret_cast<const v4i*>(svr + r * a.ld_sv + off);
#pragma unroll
        for (int n = 0; n < NS; ++n) xs[n] = *reinterpret_cast<const v4i*>(xr[n] + off);
#pragma unroll
        for (int r = 0; r < kSmallSv; ++r)
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                int t = acc[r][n];
                t = __builtin_amdgcn_sdot4(ss[r].x, xs[n].x, t, false);
                t = __builtin_amdgcn_sdot4(ss[r].y, xs[n].y, t, false);
                t = __builtin_amdgcn_sdot4(ss[r].z, xs[n].z, t, false);
                t = __builtin_amdgcn_sdot4(ss[r].w, xs[n].w, t, false);
                acc[r][n] = t;
            }
    }
#pragma unroll
    for (int r = 0; r < kSmallSv; ++r)
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            const int v = wave_sum_i32(acc[r][n]);
            if (lane == 0) red[wave][r * NS + n] = v;
        }
    __syncthreads();
    if (tid < kSmallSv * NS) {
        const int r = tid / NS, n = tid - r * NS;
        if (n < a.N) a.G[(m0 + r) * a.g_sm + (int64_t)n * a.g_sn] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

template <int PT>
__global__ __launch_bounds__(128) void k_svm_epi_small(SmallArgs a) {
    if (a.tile_exact && a.tile_exact[blockIdx.y / kTile] != 1) return;
    __shared__ double etab[64];
    __shared__ double kvs[kTile];
    __shared__ double wl[PT][kTile];
    __shared__ double xch[PT];
    const int tid = threadIdx.x, stile = blockIdx.x, n = blockIdx.y;
    exp_tab_init(etab, tid);
    const int64_t m = (int64_t)stile * kTile + tid;
#pragma unroll
    for (int p = 0; p < PT; ++p) wl[p][tid] = a.W[(int64_t)p * a.Mpad + m];
    __syncthreads();
    const bool rbf = (a.kernel == RML_KERNEL_RBF);
    // the tile kernels' epilogue functions (svm_epilogue.h), one kernel value per thread
    const double xt = exact_sample_term(rbf, a.x_isum, a.x_isq, n);
    const double g = (double)a.G[m * a.g_sm + (int64_t)n * a.g_sn];
    kvs[tid] = kernel_value<true>(rbf, g, xt, a.sv_term[m], a.gs, etab);
    __syncthreads();
    if (tid < 2) {                                  // the two 64-row chains of the tile, in the tile kernels' order
        double S[PT];
#pragma unroll
        for (int p = 0; p < PT; ++p) S[p] = 0.0;
        for (int mm = 0; mm < 64; ++mm) {
            const int ml = tid * 64 + mm;
            chain_link<PT>(S, &wl[0][ml], kTile, kvs[ml]);
        }
        if (tid == 1) {
#pragma unroll
            for (int p = 0; p < PT; ++p) xch[p] = S[p];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // both chains live in one wave
        if (tid == 0) {
#pragma unroll
            for (int p = 0; p < PT; ++p) a.partial[((int64_t)stile * a.Npart + n) * PT + p] = S[p] + xch[p];
        }
    }
}

}  // namespace
