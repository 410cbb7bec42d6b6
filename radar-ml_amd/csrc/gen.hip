// Output layer of the SGAN generator (sgan.py:112-114): Conv2D(1, 7x7, 'same', tanh) on a dense NHWC half tensor with C = 128
// channels -- the generator's largest activation (N x 128 x 128 x 128) in, one float32 plane out.  With ONE output channel the
// layer is three GEMMs with one tiny side (49 taps, padded to 64), which an implicit-GEMM library kernel tiles badly; here:
//
//   forward   P[pixel][tap] = X[pixel][0:128] . W[tap][0:128] on the matrix cores (v_mfma_f32_32x32x16, M = 32 pixels, N = 2 x 32 taps,
//             K = 128), input row by input row into LDS, followed by the stencil sum over kx and the accumulation over ky into a band
//             of 16 output rows held in LDS; y = tanh(sum + bias).  x is read once (plus the six halo rows of a band).
//   backward  k_c7_dz:  dz = dy (1 - y^2) into a zero-padded plane [N][H+6][W+6] (no bounds tests afterwards) + partial sums of dbias
//             k_c7_dx:  dx[pixel][0:128] = im2col(dz)[pixel][0:64] . W[0:64][0:128] on the matrix cores (M = 32 pixels, N = 4 x 32
//                       channels, K = 64); the channel of column r of tile u is 4 r + u, so a lane stores 8 bytes and a wave whole rows
//             k_c7_dw:  dweight[tap][c] = sum over pixels of dz[pixel - off(tap)] x[pixel][c]: a wave per image row, two channels per
//                       lane, 49 packed float32 accumulators, dz through wave-uniform loads; per-workgroup partials in the workspace
//             k_c7_sum: fixed-order combine of the partials (the pattern of k_sum_partials, bnact.hip).
// No atomics; every sum runs in an order fixed by the shape alone, and the order inside one sample does not
// depend on the batch: y and dx of a sample are the same bits alone and inside a batch.
// Weights arrive as float32 [49][C] (tap = ky * 7 + kx) and are rounded to the operand type on load, as autocast would.
#include "rml_internal.h"

namespace {

constexpr int kT = 256;
constexpr int kC = 128;             // channels
constexpr int kTaps = 49;
constexpr int kBand = 16;           // output rows per forward workgroup
constexpr int kMaxHW = 256;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <bool BF> __device__ __forceinline__ float h2f(uint16_t h);
template <> __device__ __forceinline__ float h2f<true>(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
template <> __device__ __forceinline__ float h2f<false>(uint16_t h) {
    _Float16 v;
    __builtin_memcpy(&v, &h, 2);
    return (float)v;
}
template <bool BF> __device__ __forceinline__ uint16_t f2h(float f);
template <> __device__ __forceinline__ uint16_t f2h<true>(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);      // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
template <> __device__ __forceinline__ uint16_t f2h<false>(float f) {
    _Float16 v = (_Float16)f;
    uint16_t h;
    __builtin_memcpy(&h, &v, 2);
    return h;
}

template <bool BF> __device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2h<BF>(v[2 * i]) | ((uint32_t)f2h<BF>(v[2 * i + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <bool BF> __device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b, const f32x16& c) {
    if constexpr (BF) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&a), *reinterpret_cast<const f16x8*>(&b), c, 0, 0, 0);
    }
}

// row of the 32 x 32 accumulator that register i of a lane holds (mfma_tile.h: cd32_row)
__device__ __forceinline__ int acc_row(int i, int lane) { return (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); }

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (sample, band of kBand output rows).  K order of the MFMA: slot (step s, half h, element j) is channel
// 64 h + 8 s + j, so lane (pixel r, half h) reads 128 contiguous bytes of its pixel and a wave 8 KB in a row.
// LDS: P[W][49] products of the current input row, Y[kBand][W] the band's sums.
template <bool BF>
__global__ __launch_bounds__(kT) void k_c7_fwd(const uint16_t* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
                                               float* __restrict__ y, int H, int W, int bands) {
    extern __shared__ float smem[];
    float* P = smem;
    float* Y = smem + (size_t)W * kTaps;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int n = blockIdx.x / bands, band = blockIdx.x - n * bands;
    const int oy0 = band * kBand, oy1 = min(H, oy0 + kBand);

    uint4 bfrag[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int tap = 32 * u + r;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tap < kTaps ? wgt[tap * kC + 64 * h + 8 * s + j] : 0.0f;
            bfrag[u][s] = pack8<BF>(v);
        }
    }
    for (int i = tid; i < kBand * W; i += kT) Y[i] = 0.0f;
    __syncthreads();

    const int iy0 = max(0, oy0 - 3), iy1 = min(H, oy1 + 3);
    const int ntile = (W + 31) >> 5;
    for (int iy = iy0; iy < iy1; ++iy) {
        const uint16_t* xrow = x + ((int64_t)n * H + iy) * (int64_t)W * kC;
        for (int t = wave; t < ntile; t += 4) {
            const int ix = min(t * 32 + r, W - 1);
            const uint4* src = reinterpret_cast<const uint4*>(xrow + (int64_t)ix * kC + 64 * h);
            uint4 a[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) a[s] = src[s];
            f32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                acc0 = mfma16<BF>(a[s], bfrag[0][s], acc0);
                acc1 = mfma16<BF>(a[s], bfrag[1][s], acc1);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int px = t * 32 + acc_row(i, lane);
                if (px < W) {
                    P[px * kTaps + r] = acc0[i];
                    if (r < kTaps - 32) P[px * kTaps + 32 + r] = acc1[i];
                }
            }
        }
        __syncthreads();
        // input row iy feeds output row iy + 3 - ky through kernel row ky: one thread per (ky, ox), seven taps in kx order
        for (int item = tid; item < 7 * W; item += kT) {
            const int ky = item / W, ox = item - ky * W, oy = iy + 3 - ky;
            if (oy >= oy0 && oy < oy1) {
                float s = 0.0f;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const int jx = ox + kx - 3;
                    if (jx >= 0 && jx < W) s += P[jx * kTaps + ky * 7 + kx];
                }
                Y[(oy - oy0) * W + ox] += s;
            }
        }
        __syncthreads();
    }
    const float b = bias[0];
    float* yo = y + ((int64_t)n * H + oy0) * (int64_t)W;
    for (int i = tid; i < (oy1 - oy0) * W; i += kT) yo[i] = tanhf(Y[i] + b);
}

// ---- backward 1: dz into the zero-padded plane, partial sums of dbias ----------------------------------------------------------------
// dzp[n][a][b] = dz[n][a - 3][b - 3] inside the image, 0 in the frame of 3; part[blockIdx] = this workgroup's sum (fixed tree)
__global__ __launch_bounds__(kT) void k_c7_dz(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dzp, int64_t total,
                                              int H, int W, float* __restrict__ part) {
    __shared__ float red[kT];
    const int Hp = H + 6, Wp = W + 6;
    float s = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const int64_t row = i / Wp;
        const int b = (int)(i - row * Wp), a = (int)(row % Hp);
        const int64_t n = row / Hp;
        float v = 0.0f;
        if (a >= 3 && a < H + 3 && b >= 3 && b < W + 3) {
            const int64_t q = (n * H + (a - 3)) * W + (b - 3);
            const float yy = y[q];
            v = dy[q] * (1.0f - yy * yy);
        }
        dzp[i] = v;
        s += v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = kT / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// ---- backward 2: dx ---------------------------------------------------------------------------------------------------------------
// One wave per tile of 32 pixels of one image row.  A = im2col(dz): lane (pixel r, half h) holds taps 16 s + 8 h + j of its pixel,
// dz[iy + 3 - ky][ix + 3 - kx] = dzp[iy + 6 - ky][ix + 6 - kx].  B = the weights, column r of tile u = channel 4 r + u.
template <bool BF>
__global__ __launch_bounds__(kT) void k_c7_dx(const float* __restrict__ dzp, const float* __restrict__ wgt, uint16_t* __restrict__ dx,
                                              int64_t rows /* N * H */, int H, int W) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int Hp = H + 6, Wp = W + 6;
    uint4 bfrag[4][4];                  // [k-step][channel tile]
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int tap = 16 * s + 8 * h + j;
                v[j] = tap < kTaps ? wgt[tap * kC + 4 * r + u] : 0.0f;
            }
            bfrag[s][u] = pack8<BF>(v);
        }
    const int ntile = (W + 31) >> 5;
    const int64_t ntask = rows * ntile;
    for (int64_t task = (int64_t)blockIdx.x * 4 + wave; task < ntask; task += (int64_t)gridDim.x * 4) {
        const int64_t row = task / ntile;
        const int t = (int)(task - row * ntile);
        const int64_t n = row / H;
        const int iy = (int)(row - n * H);
        const int ix = min(t * 32 + r, W - 1);
        const float* base = dzp + ((n * Hp + iy + 6) * (int64_t)Wp + ix + 6);
        uint4 a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int tap = 16 * s + 8 * h + j;
                const int ky = tap / 7, kx = tap - ky * 7;
                v[j] = tap < kTaps ? base[-(int64_t)ky * Wp - kx] : 0.0f;
            }
            a[s] = pack8<BF>(v);
        }
        f32x16 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[u][i] = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = mfma16<BF>(a[s], bfrag[s][u], acc[u]);
        uint16_t* orow = dx + row * (int64_t)W * kC;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int px = t * 32 + acc_row(i, lane);
            if (px < W) {
                uint2 o;
                o.x = (uint32_t)f2h<BF>(acc[0][i]) | ((uint32_t)f2h<BF>(acc[1][i]) << 16);
                o.y = (uint32_t)f2h<BF>(acc[2][i]) | ((uint32_t)f2h<BF>(acc[3][i]) << 16);
                *reinterpret_cast<uint2*>(orow + (int64_t)px * kC + 4 * r) = o;
            }
        }
    }
}

// ---- backward 3: dweight -------------------------------------------------------------------------------------------------------------
// A wave takes image rows wave_id, wave_id + waves, ...; lane l holds channels 2 l and 2 l + 1 and all 49 taps.  dz comes through
// wave-uniform addresses (the row index is made uniform with readfirstlane, so the loads can go down the scalar path).  The four
// waves of a workgroup are summed through LDS in wave order into part[blockIdx][49][128].
template <bool BF>
__global__ __launch_bounds__(kT) void k_c7_dw(const uint16_t* __restrict__ x, const float* __restrict__ dzp, int64_t rows, int H, int W,
                                              float* __restrict__ part) {
    __shared__ float red[kTaps * kC];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Hp = H + 6, Wp = W + 6;
    f32x2 acc[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) acc[t] = f32x2{0.0f, 0.0f};
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int64_t n = row / H;
        const int iy = (int)(row - n * H);
        const uint32_t* xr = reinterpret_cast<const uint32_t*>(x + row * (int64_t)W * kC) + lane;
        const float* dzr = dzp + (n * Hp + iy + 6) * (int64_t)Wp + 6;
        for (int ix = 0; ix < W; ++ix) {
            const uint32_t pk = xr[(int64_t)ix * (kC / 2)];
            const f32x2 xv = f32x2{h2f<BF>((uint16_t)(pk & 0xFFFFu)), h2f<BF>((uint16_t)(pk >> 16))};
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                const float* d = dzr - (int64_t)ky * Wp + ix;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float dv = d[-kx];
                    acc[ky * 7 + kx] += xv * f32x2{dv, dv};
                }
            }
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                f32x2* slot = reinterpret_cast<f32x2*>(red + t * kC + 2 * lane);
                *slot = w == 0 ? acc[t] : *slot + acc[t];
            }
        }
        __syncthreads();
    }
    float* out = part + (size_t)blockIdx.x * (kTaps * kC);
    for (int i = tid; i < kTaps * kC; i += kT) out[i] = red[i];
}

// out[j] = sum over g of part[g][j] (float64, strided partial sums + fixed tree): one workgroup per j
__global__ __launch_bounds__(kT) void k_c7_sum(const float* __restrict__ part, int G, int L, float* __restrict__ out) {
    __shared__ double sa[kT];
    const int j = blockIdx.x, t = threadIdx.x;
    double a = 0.0;
    for (int g = t; g < G; g += kT) a += (double)part[(size_t)g * L + j];
    sa[t] = a;
    __syncthreads();
    for (int off = kT / 2; off >= 1; off >>= 1) {
        if (t < off) sa[t] += sa[t + off];
        __syncthreads();
    }
    if (t == 0) out[j] = (float)sa[0];
}

// workgroups of the dz pass / of the dweight pass: functions of the shape (and the device's CU count) alone
int dz_grid(const rml_ctx* ctx, int64_t N, int H, int W) {
    const int64_t total = N * (H + 6) * (int64_t)(W + 6);
    const int64_t g = (total + kT - 1) / kT, cap = (int64_t)ctx->num_cu * 4;
    return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}
int dw_grid(const rml_ctx* ctx, int64_t N, int H) {
    const int64_t g = (N * H + 3) / 4, cap = (int64_t)ctx->num_cu * 2;
    return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}

int check_conv7(const char* who, const rml_ctx* ctx, int64_t N, int H, int W, int C, int dtype) {
    RML_REQUIRE(ctx && N >= 0 && H > 0 && W > 0 && C > 0, RML_ERR_INVALID, "%s: bad arguments", who);
    RML_REQUIRE(rml_conv7_tanh_supported(H, W, C), RML_ERR_UNSUPPORTED, "%s: C = %d, H = %d, W = %d (C = 128, H and W <= 256)", who, C, H, W);
    RML_REQUIRE(dtype == 0 || dtype == 1, RML_ERR_INVALID, "%s: dtype 0 = float16, 1 = bfloat16", who);
    RML_REQUIRE(N * (int64_t)(H + 6) < ((int64_t)1 << 24), RML_ERR_UNSUPPORTED, "%s: too many rows for one launch", who);
    return RML_OK;
}

}  // namespace

extern "C" int rml_conv7_tanh_supported(int H, int W, int C) { return C == kC && H >= 1 && W >= 1 && H <= kMaxHW && W <= kMaxHW; }

extern "C" int64_t rml_conv7_workspace_floats(rml_ctx* ctx, int64_t N, int H, int W, int C) {
    if (!ctx || N < 0 || !rml_conv7_tanh_supported(H, W, C)) return 0;
    // the padded dz planes, the dbias partials, the dweight partials
    return N * (H + 6) * (int64_t)(W + 6) + dz_grid(ctx, N, H, W) + (int64_t)dw_grid(ctx, N, H) * kTaps * kC;
}

extern "C" int rml_conv7_tanh_forward(rml_ctx* ctx, const void* x, int dtype, int64_t N, int H, int W, int C, const float* weight,
                                      const float* bias, float* y, void* stream) {
    int rc = check_conv7("rml_conv7_tanh_forward", ctx, N, H, W, C, dtype);
    if (rc) return rc;
    if (N == 0) return RML_OK;
    RML_REQUIRE(x && weight && bias && y, RML_ERR_INVALID, "rml_conv7_tanh_forward: NULL argument");
    RML_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, RML_ERR_INVALID, "rml_conv7_tanh_forward: x must be 16-byte aligned");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int bands = (H + kBand - 1) / kBand;
    const size_t lds = ((size_t)W * kTaps + (size_t)kBand * W) * sizeof(float);
    const uint16_t* xs = static_cast<const uint16_t*>(x);
    const unsigned grid = (unsigned)(N * bands);
    if (dtype) {
        RML_MAX_DYN_LDS((int)(kMaxHW * (kTaps + kBand) * sizeof(float)), k_c7_fwd<true>);
        hipLaunchKernelGGL(k_c7_fwd<true>, dim3(grid), dim3(kT), lds, st, xs, weight, bias, y, H, W, bands);
    } else {
        RML_MAX_DYN_LDS((int)(kMaxHW * (kTaps + kBand) * sizeof(float)), k_c7_fwd<false>);
        hipLaunchKernelGGL(k_c7_fwd<false>, dim3(grid), dim3(kT), lds, st, xs, weight, bias, y, H, W, bands);
    }
    RML_HIP(hipGetLastError());
    return RML_OK;
}

extern "C" int rml_conv7_tanh_backward(rml_ctx* ctx, const void* x, const float* y, const float* dy, int dtype, int64_t N, int H, int W, int C,
                                       const float* weight, float* workspace, void* dx, float* dweight, float* dbias, void* stream) {
    int rc = check_conv7("rml_conv7_tanh_backward", ctx, N, H, W, C, dtype);
    if (rc) return rc;
    if (N == 0) return RML_OK;
    RML_REQUIRE(x && y && dy && weight && workspace && dx && dweight && dbias, RML_ERR_INVALID, "rml_conv7_tanh_backward: NULL argument");
    RML_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0, RML_ERR_INVALID,
                "rml_conv7_tanh_backward: x and dx must be 16-byte aligned");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t total = N * (H + 6) * (int64_t)(W + 6), rows = N * H;
    const int Gz = dz_grid(ctx, N, H, W), Gw = dw_grid(ctx, N, H);
    float* dzp = workspace;
    float* zpart = dzp + total;
    float* wpart = zpart + Gz;
    const uint16_t* xs = static_cast<const uint16_t*>(x);
    uint16_t* os = static_cast<uint16_t*>(dx);
    hipLaunchKernelGGL(k_c7_dz, dim3(Gz), dim3(kT), 0, st, y, dy, dzp, total, H, W, zpart);
    hipLaunchKernelGGL(k_c7_sum, dim3(1), dim3(kT), 0, st, zpart, Gz, 1, dbias);
    const int64_t ntask = rows * ((W + 31) / 32);
    const int64_t gx64 = (ntask + 3) / 4, capx = (int64_t)ctx->num_cu * 8;
    const unsigned Gx = (unsigned)(gx64 < capx ? gx64 : capx);
    if (dtype) {
        hipLaunchKernelGGL(k_c7_dx<true>, dim3(Gx), dim3(kT), 0, st, dzp, weight, os, rows, H, W);
        hipLaunchKernelGGL(k_c7_dw<true>, dim3(Gw), dim3(kT), 0, st, xs, dzp, rows, H, W, wpart);
    } else {
        hipLaunchKernelGGL(k_c7_dx<false>, dim3(Gx), dim3(kT), 0, st, dzp, weight, os, rows, H, W);
        hipLaunchKernelGGL(k_c7_dw<false>, dim3(Gw), dim3(kT), 0, st, xs, dzp, rows, H, W, wpart);
    }
    hipLaunchKernelGGL(k_c7_sum, dim3(kTaps * kC), dim3(kT), 0, st, wpart, Gw, kTaps * kC, dweight);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
