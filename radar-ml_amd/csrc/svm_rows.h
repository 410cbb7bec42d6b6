// Row preparation of the SVM path (codes, statistics, digit planes) and the per-tile path decision.
#pragma once
#include "mfma_tile.h"

namespace {

// digit planes of float32 rows: one workgroup per row, a thread takes 4 consecutive features per step.
// ok[row] = every feature is finite and inside the model's fixed-point range.
__global__ __launch_bounds__(256) void k_digit_rows(const float* f32, int64_t ld, int64_t D, int64_t Dq, int64_t plane, int8_t* dig,
                                                    double* nsq, int32_t* ok, double c0, double k31, const int32_t* skip_if_set) {
    if (skip_if_set && *skip_if_set) return;
    __shared__ double redn[4];
    __shared__ int redo[4];
    const int64_t b = blockIdx.x;
    double nn = 0.0; int good = 1;
    for (int64_t i4 = (int64_t)threadIdx.x * 4; i4 < Dq; i4 += 1024) {
        uint32_t pk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t idx = i4 + e;
            uint32_t packed = 0;
            if (idx < D) {
                const double t = rint(((double)f32[b * ld + idx] - c0) * k31);
                const bool in = t >= -2147483648.0 && t <= 2139062143.0;       // NaN fails both
                good &= in ? 1 : 0;
                const int I = in ? (int)t : 0;
                const double u = (double)I * 0x1p-31;
                nn = fma(u, u, nn);
                packed = ((uint32_t)I + 0x00808080u) ^ 0x00808080u;           // bytes = balanced digits a0 (top) .. a3
            }
            pk[e] = packed;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int sh = 8 * (3 - d);
            const uint32_t w = ((pk[0] >> sh) & 255u) | (((pk[1] >> sh) & 255u) << 8) | (((pk[2] >> sh) & 255u) << 16) | (((pk[3] >> sh) & 255u) << 24);
            *reinterpret_cast<uint32_t*>(dig + (int64_t)d * plane + b * Dq + i4) = w;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { nn += __shfl_xor(nn, off); good &= __shfl_xor(good, off); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { redn[wave] = nn; redo[wave] = good; }
    __syncthreads();
    if (threadIdx.x == 0) {
        nsq[b] = (redn[0] + redn[1]) + (redn[2] + redn[3]);
        ok[b] = redo[0] & redo[1] & redo[2] & redo[3];
    }
}

// ---- row preparation for callers that bring float32 feature rows -------------------------
// One workgroup per row: zero-padded float copy (ld = Df), float64 norm, codes + statistics.
__global__ __launch_bounds__(256) void k_prepare_rows(const float* feat, int64_t ld, int64_t D, float code_scale,
                                                      float* f32, int64_t Df, double* nsq,
                                                      uint8_t* q, int64_t Dq, int32_t* isum, int64_t* isq, int32_t* flags) {
    __shared__ int64_t red[16];
    const int64_t b = blockIdx.x;
    const bool scaled = code_scale > 1.0f;
    int32_t s = 0; int64_t sq = 0; int ok = 1; double nn = 0.0;
    // eight of the thread's values in flight at a time (the loop used to wait out a memory latency per value: its stores may alias
    // its loads as far as the compiler knows -- 44 us for ONE row of 20 480 values, most of a predict.py:60 call); the values are
    // consumed in the same ascending order, so every sum is the one it was
    const int64_t lim = Dq > Df ? Dq : Df;
    const float* __restrict__ src = feat + b * ld;
    for (int64_t base = threadIdx.x; base < lim; base += 256 * 8) {
        float vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t idx = base + (int64_t)u * 256;
            vv[u] = idx < D ? src[idx] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t idx = base + (int64_t)u * 256;
            if (idx >= lim) break;
            const float v = vv[u];
            if (idx < Df) f32[b * Df + idx] = v;
            nn += (double)v * (double)v;
            if (q && idx < Dq) {
                uint8_t code = 0;
                if (idx < D) {
                    float c = rintf(scaled ? v * code_scale : v);
                    float back = scaled ? __fdiv_rn(c, code_scale) : c;
                    bool good = (back == v) && c >= 0.0f && c <= 255.0f;
                    int ci = good ? (int)c : 0;
                    ok &= good ? 1 : 0;
                    s += ci; sq += (int64_t)(ci * ci);
                    code = (uint8_t)(ci ^ 0x80);
                }
                q[b * Dq + idx] = code;
            }
        }
    }
    int64_t s64 = s;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s64 += __shfl_xor(s64, off); sq += __shfl_xor(sq, off); ok &= __shfl_xor(ok, off); nn += __shfl_xor(nn, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* redd = reinterpret_cast<double*>(red + 12);
    if (lane == 0) { red[wave * 3] = s64; red[wave * 3 + 1] = sq; red[wave * 3 + 2] = ok; redd[wave] = nn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t S = 0, Q = 0, G = 1; double NN = 0;
        for (int w = 0; w < 4; ++w) { S += red[w * 3]; Q += red[w * 3 + 1]; G &= red[w * 3 + 2]; NN += redd[w]; }
        if (isum) isum[b] = (int32_t)S;
        if (isq) isq[b] = Q;
        if (flags) flags[b] = q ? (int32_t)G : 0;
        nsq[b] = NN;
    }
}

// tile_exact[ft] = policy(flags of the 128 rows of tile ft); *all_exact = AND over tiles.
// One 128-thread block per tile, one row flag per thread; with all_exact, ONE MORE block that scans every row flag and writes the AND
// (round 3 pre-set the word with a one-thread kernel and cleared it with atomics: a launch and its gap per chunk on the stream whose
// chain is the period of the Walabot pipeline).
// group = sample tiles decided together (2 when the 256-sample GEMM kernel takes the exact tiles): blockDim = group * 128.
__global__ __launch_bounds__(256) void k_tile_flags(const int32_t* flags, int64_t N, int FT, int policy /*0 auto,1 force general,2 force i8*/,
                                                    int model_exact, int32_t* tile_exact, int32_t* all_exact, int group) {
    const int tile_blocks = (FT + group - 1) / group;
    if ((int)blockIdx.x >= tile_blocks) {
        int mine = 1;
        if (policy == 1) mine = 0;
        else if (policy != 2) {
            if (!(model_exact && flags != nullptr)) mine = 0;
            else if ((reinterpret_cast<uintptr_t>(flags) & 15) == 0) {
                // eight independent 16-byte loads per thread and trip (a plain `mine &= flags[r]` loop waits out a memory latency per
                // flag: 65-75 us for 8 192 rows in the kernel timeline of session r4aq -- on the stream whose chain is the period)
                const int4* f4 = reinterpret_cast<const int4*>(flags);
                const int64_t n4 = N >> 2;
                for (int64_t i = threadIdx.x; i < n4; i += (int64_t)blockDim.x * 8) {
                    int4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int64_t idx = i + (int64_t)u * blockDim.x;
                        v[u] = idx < n4 ? f4[idx] : make_int4(1, 1, 1, 1);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) mine &= (v[u].x != 0) & (v[u].y != 0) & (v[u].z != 0) & (v[u].w != 0);
                }
                for (int64_t r = (n4 << 2) + threadIdx.x; r < N; r += blockDim.x) mine &= flags[r] != 0;
            } else {
                for (int64_t r = threadIdx.x; r < N; r += blockDim.x) mine &= flags[r] != 0;
            }
        }
        const int e = __syncthreads_and(mine);
        if (threadIdx.x == 0) *all_exact = e;
        return;
    }
    const int ft0 = blockIdx.x * group;
    int e;
    if (policy == 1) e = 0;
    else if (policy == 2) e = 1;
    else {
        const int64_t r = (int64_t)ft0 * kTile + threadIdx.x;
        int mine = (model_exact && flags != nullptr) ? ((r < N) ? (flags[r] != 0) : 1) : 0;
        e = __syncthreads_and(mine);
    }
    if (threadIdx.x == 0)
        for (int g = 0; g < group; ++g) if (ft0 + g < FT) tile_exact[ft0 + g] = e;
}

// second decision, once the digit planes of a chunk exist: a tile group that is not on the code grid (tile_exact == 0) goes
// to the multi-digit int8 GEMM (tile_exact = 2) when every one of its rows fits the model's fixed-point range
__global__ __launch_bounds__(256) void k_tile_dig(const int32_t* dflags, int64_t N, int FT, int32_t* tile_exact, const int32_t* skip_if_set) {
    if (skip_if_set && *skip_if_set) return;
    const int ft0 = blockIdx.x * 2;
    const int64_t r = (int64_t)ft0 * kTile + threadIdx.x;
    const int mine = (r < N) ? (dflags[r] != 0) : 1;
    const int e = __syncthreads_and(mine);
    if (threadIdx.x == 0 && e && tile_exact[ft0] == 0) {
        tile_exact[ft0] = 2;
        if (ft0 + 1 < FT) tile_exact[ft0 + 1] = 2;
    }
}

}  // namespace
