// The SGAN generator at inference (sgan.py:57-122 through g_model.predict, sgan.py:450): per branch Dense + ReLU, n_up x
// [Conv2DTranspose(C -> C, 4x4, stride 2, 'same') + BatchNormalization + ReLU] with the moving statistics folded into weights and
// bias by the caller, then the 7x7 tanh layer of gen.hip.
//
//   k_gen_dense  y[n][j] = relu(sum_l z[n][l] W[l][j] + b[j]) in float32 FMAs, l ascending; half out in Keras' unit order, which IS
//                the NHWC image [base][base][C] of the reshape.
//   k_gen_up     out[2m+p][2n+q][co] = relu(bias[co] + sum over a, b in {0,1} and ci of x[m-1+p+a][n-1+q+b][ci] wt[p*2+q][co][(a*2+b)*C + ci]):
//                a transposed convolution with stride 2 is four ordinary 2x2 convolutions, one per output phase (p, q) -- four implicit
//                GEMMs with M = N H W, K = 4 C = 512 and 128 output channels -- on v_mfma_f32_32x32x16_{f16,bf16}.
//                One workgroup per 8 x 8 patch of input positions: the patch with its one-pixel halo (10 x 10 pixels, zeros outside the
//                plane, so the inner loop has no bounds test) is staged in LDS once and feeds all four phases; wave w IS phase w
//                (p = w >> 1, q = w & 1): M = 64 positions (two 32-row tiles) x 128 channels (four 32-column tiles), 8 accumulators.
//                A fragments come from LDS (pixel stride 272 B: the 256-byte pixel rows would all start on one bank), B fragments
//                straight from the packed weights (512 KB for all phases: L2-resident), 16 bytes per lane and step.  K order of a
//                step: slot (tap t, step s, half h, element j) is channel 64 h + 8 s + j of tap t, so a lane walks 128 contiguous
//                bytes of its pixel / of its weight row per tap.  Column r of channel tile u is channel 4 r + u: a lane stores 8 bytes
//                and a half-wave one whole 256-byte output pixel.
// No atomics, no split K: an output element is ONE chain of 32 MFMAs in an order that depends on nothing, so a sample has the same
// bits alone, anywhere in any batch, and on a second call.
#include "rml_internal.h"

namespace {

constexpr int kT = 256;
constexpr int kC = 128;             // channels
constexpr int kP = 8;               // patch edge (input positions)
constexpr int kPH = kP + 2;         // with the halo
constexpr int kPixB = 2 * kC + 16;  // LDS bytes per staged pixel
constexpr int kDenseNB = 8;         // samples per k_gen_dense workgroup
constexpr int64_t kWsBudget = (int64_t)128 << 20;   // the two activation buffers of a chunk stay within this (one sample always fits)
constexpr int64_t kMaxChunk = 4096;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

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

template <bool BF> __device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b, const f32x16& c) {
    if constexpr (BF) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&a), *reinterpret_cast<const f16x8*>(&b), c, 0, 0, 0);
    }
}

// row of the 32 x 32 accumulator that register i of a lane holds (mfma_tile.h: cd32_row)
__device__ __forceinline__ int acc_row(int i, int lane) { return (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ float relu(float v) { return v < 0.0f ? 0.0f : v; }      // NaN stays NaN

// ---- Dense + ReLU ------------------------------------------------------------------------------------------------------------------
// grid (ceil(U / kT), ceil(N / kDenseNB)): a thread owns unit j of kDenseNB samples, so a weight is read once per kDenseNB samples;
// z through wave-uniform addresses.
template <bool BF>
__global__ __launch_bounds__(kT) void k_gen_dense(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ b,
                                                  uint16_t* __restrict__ y, int64_t N, int L, int64_t U) {
    const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;
    const int64_t n0 = (int64_t)blockIdx.y * kDenseNB;
    if (j >= U) return;
    float acc[kDenseNB];
#pragma unroll
    for (int s = 0; s < kDenseNB; ++s) acc[s] = 0.0f;
    for (int l = 0; l < L; ++l) {
        const float wv = w[(int64_t)l * U + j];
#pragma unroll
        for (int s = 0; s < kDenseNB; ++s) {
            const int64_t n = n0 + s < N ? n0 + s : N - 1;
            acc[s] = fmaf(z[n * L + l], wv, acc[s]);
        }
    }
    const float bj = b[j];
#pragma unroll
    for (int s = 0; s < kDenseNB; ++s)
        if (n0 + s < N) y[(n0 + s) * U + j] = f2h<BF>(relu(acc[s] + bj));
}

// ---- Conv2DTranspose 4x4 stride 2 'same' + bias + ReLU ---------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(kT) void k_gen_up(const uint16_t* __restrict__ x, const uint16_t* __restrict__ wt, const float* __restrict__ bias,
                                               uint16_t* __restrict__ y, int H, int W, int tiles_x, int tiles) {
    __shared__ __attribute__((aligned(16))) unsigned char patch[kPH * kPH * kPixB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t n = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - n * tiles);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int m0 = ty * kP, n0 = tx * kP;

    // the patch and its halo: 100 pixels of 16 chunks of 16 bytes; zeros outside the plane
    const uint16_t* xs = x + n * (int64_t)H * W * kC;
    for (int i = tid; i < kPH * kPH * 16; i += kT) {
        const int pix = i >> 4, c16 = i & 15;
        const int pr = pix / kPH, pc = pix - pr * kPH;
        const int iy = m0 - 1 + pr, ix = n0 - 1 + pc;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const uint4*>(xs + ((int64_t)iy * W + ix) * kC + c16 * 8);
        *reinterpret_cast<uint4*>(patch + pix * kPixB + c16 * 16) = v;
    }
    __syncthreads();

    const int p = wave >> 1, q = wave & 1;
    // A: position 32 mt + r of the patch = (my, nx); its window starts at patch pixel (my + p, nx + q)
    const unsigned char* abase[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int pos = 32 * mt + r, my = pos >> 3, nx = pos & 7;
        abase[mt] = patch + ((my + p) * kPH + nx + q) * kPixB + 128 * h;
    }
    // B: column r of channel tile u is output channel 4 r + u
    const uint16_t* brow = wt + ((int64_t)wave * kC + 4 * r) * (4 * kC) + 64 * h;

    f32x16 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][u][i] = 0.0f;

#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
        const int aoff = ((tap >> 1) * kPH + (tap & 1)) * kPixB;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            uint4 av[2], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) bv[u] = *reinterpret_cast<const uint4*>(brow + u * (4 * kC) + tap * kC + 8 * s);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) av[mt] = *reinterpret_cast<const uint4*>(abase[mt] + aoff + 16 * s);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[mt][u] = mfma16<BF>(av[mt], bv[u], acc[mt][u]);
        }
    }

    const float4 bj = *reinterpret_cast<const float4*>(bias + 4 * r);
    uint16_t* ys = y + n * (int64_t)(2 * H) * (2 * W) * kC;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int pos = 32 * mt + acc_row(i, lane), my = pos >> 3, nx = pos & 7;
            const int oy = 2 * (m0 + my) + p, ox = 2 * (n0 + nx) + q;
            uint2 o;
            o.x = (uint32_t)f2h<BF>(relu(acc[mt][0][i] + bj.x)) | ((uint32_t)f2h<BF>(relu(acc[mt][1][i] + bj.y)) << 16);
            o.y = (uint32_t)f2h<BF>(relu(acc[mt][2][i] + bj.z)) | ((uint32_t)f2h<BF>(relu(acc[mt][3][i] + bj.w)) << 16);
            *reinterpret_cast<uint2*>(ys + ((int64_t)oy * (2 * W) + ox) * kC + 4 * r) = o;
        }
}

int launch_up(const void* x, int dtype, int64_t N, int H, int W, const void* wt, const float* bias, void* y, hipStream_t st) {
    const int tiles_x = W / kP, tiles = (H / kP) * tiles_x;
    const unsigned grid = (unsigned)(N * tiles);
    const uint16_t* xs = static_cast<const uint16_t*>(x);
    const uint16_t* ws = static_cast<const uint16_t*>(wt);
    uint16_t* ys = static_cast<uint16_t*>(y);
    if (dtype) hipLaunchKernelGGL(k_gen_up<true>, dim3(grid), dim3(kT), 0, st, xs, ws, bias, ys, H, W, tiles_x, tiles);
    else hipLaunchKernelGGL(k_gen_up<false>, dim3(grid), dim3(kT), 0, st, xs, ws, bias, ys, H, W, tiles_x, tiles);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

inline int64_t round256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// chunk of samples and the two ping-pong activation buffers (bytes per sample, rounded to 256): layer l (0 = the dense output,
// l = 1..n_up the transposed convolutions) writes buffer l & 1
struct gen_plan {
    int64_t chunk, buf[2];
    int S;
};

bool gen_plan_make(int64_t N, int base, int n_up, int C, gen_plan* gp) {
    if (N < 0 || C != kC || base < 1 || n_up < 0 || n_up > 8 || ((int64_t)base << n_up) > 256) return false;
    for (int l = 0; l < n_up; ++l)
        if (!rml_gen_up_supported(base << l, base << l, C)) return false;
    gp->S = base << n_up;
    if (!rml_conv7_tanh_supported(gp->S, gp->S, C)) return false;
    gp->buf[0] = gp->buf[1] = 0;
    for (int l = 0; l <= n_up; ++l) {
        const int64_t e = (int64_t)(base << l) * (base << l) * C * 2;
        if (e > gp->buf[l & 1]) gp->buf[l & 1] = e;
    }
    gp->buf[0] = round256(gp->buf[0]);
    gp->buf[1] = round256(gp->buf[1]);
    int64_t ch = kWsBudget / (gp->buf[0] + gp->buf[1]);
    ch = ch < 1 ? 1 : (ch > kMaxChunk ? kMaxChunk : ch);
    gp->chunk = N < ch ? (N > 0 ? N : 1) : ch;
    return true;
}

}  // namespace

extern "C" int rml_gen_up_supported(int H, int W, int C) {
    return C == kC && H >= kP && W >= kP && H <= 128 && W <= 128 && H % kP == 0 && W % kP == 0;
}

extern "C" int rml_gen_up_forward(rml_ctx* ctx, const void* x, int dtype, int64_t N, int H, int W, int C, const void* wt, const float* bias,
                                  void* y, void* stream) {
    RML_REQUIRE(ctx && N >= 0 && H > 0 && W > 0 && C > 0, RML_ERR_INVALID, "rml_gen_up_forward: bad arguments");
    RML_REQUIRE(rml_gen_up_supported(H, W, C), RML_ERR_UNSUPPORTED,
                "rml_gen_up_forward: C = %d, H = %d, W = %d (C = 128, H and W multiples of 8 in [8, 128])", C, H, W);
    RML_REQUIRE(dtype == 0 || dtype == 1, RML_ERR_INVALID, "rml_gen_up_forward: dtype 0 = float16, 1 = bfloat16");
    RML_REQUIRE(N * (int64_t)((H / kP) * (W / kP)) < ((int64_t)1 << 31), RML_ERR_UNSUPPORTED, "rml_gen_up_forward: too many samples for one launch");
    if (N == 0) return RML_OK;
    RML_REQUIRE(x && wt && bias && y, RML_ERR_INVALID, "rml_gen_up_forward: NULL argument");
    RML_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wt) | reinterpret_cast<uintptr_t>(y) |
                  reinterpret_cast<uintptr_t>(bias)) & 15) == 0, RML_ERR_INVALID, "rml_gen_up_forward: x, wt, bias and y must be 16-byte aligned");
    RML_HIP(hipSetDevice(ctx->device));
    return launch_up(x, dtype, N, H, W, wt, bias, y, static_cast<hipStream_t>(stream));
}

extern "C" int64_t rml_sgan_generate_workspace_bytes(int64_t N, int base, int n_up, int C) {
    gen_plan gp;
    if (!gen_plan_make(N, base, n_up, C, &gp)) return 0;
    return gp.chunk * (gp.buf[0] + gp.buf[1]);
}

extern "C" int rml_sgan_generate(rml_ctx* ctx, const float* z, int64_t N, int latent_dim, int base, int n_up, int C, int dtype,
                                 const float* dense_w, const float* dense_b, const void* up_wt, const float* up_bias, const float* out_w,
                                 const float* out_b, float* y_xz, float* y_yz, float* y_xy, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
    RML_REQUIRE(ctx && N >= 0 && latent_dim >= 1, RML_ERR_INVALID, "rml_sgan_generate: bad arguments");
    RML_REQUIRE(dtype == 0 || dtype == 1, RML_ERR_INVALID, "rml_sgan_generate: dtype 0 = float16, 1 = bfloat16");
    gen_plan gp;
    RML_REQUIRE(gen_plan_make(N, base, n_up, C, &gp), RML_ERR_UNSUPPORTED,
                "rml_sgan_generate: base = %d, n_up = %d, C = %d (C = 128; every transposed convolution on a plane whose edge is a multiple "
                "of 8 in [8, 128]; images of at most 256 x 256)", base, n_up, C);
    if (N == 0) return RML_OK;
    RML_REQUIRE(z && dense_w && dense_b && out_w && out_b && y_xz && y_yz && y_xy && workspace && (n_up == 0 || (up_wt && up_bias)),
                RML_ERR_INVALID, "rml_sgan_generate: NULL argument");
    RML_REQUIRE(workspace_bytes >= gp.chunk * (gp.buf[0] + gp.buf[1]), RML_ERR_INVALID,
                "rml_sgan_generate: workspace of %lld bytes, %lld needed (rml_sgan_generate_workspace_bytes)", (long long)workspace_bytes,
                (long long)(gp.chunk * (gp.buf[0] + gp.buf[1])));
    RML_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(up_wt) | reinterpret_cast<uintptr_t>(up_bias)) & 15) == 0,
                RML_ERR_INVALID, "rml_sgan_generate: workspace, up_wt and up_bias must be 16-byte aligned");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* bufs[2] = {static_cast<unsigned char*>(workspace), static_cast<unsigned char*>(workspace) + gp.chunk * gp.buf[0]};
    float* ys[3] = {y_xz, y_yz, y_xy};
    const int64_t U = (int64_t)base * base * C;
    const int64_t wt_layer = (int64_t)4 * C * 4 * C;       // halves per packed layer
    for (int64_t s0 = 0; s0 < N; s0 += gp.chunk) {
        const int64_t nb = N - s0 < gp.chunk ? N - s0 : gp.chunk;
        for (int br = 0; br < 3; ++br) {
            const dim3 gd((unsigned)((U + kT - 1) / kT), (unsigned)((nb + kDenseNB - 1) / kDenseNB));
            const float* zs = z + s0 * latent_dim;
            const float* dw = dense_w + (int64_t)br * latent_dim * U;
            const float* db = dense_b + (int64_t)br * U;
            uint16_t* a0 = reinterpret_cast<uint16_t*>(bufs[0]);
            if (dtype) hipLaunchKernelGGL(k_gen_dense<true>, gd, dim3(kT), 0, st, zs, dw, db, a0, nb, latent_dim, U);
            else hipLaunchKernelGGL(k_gen_dense<false>, gd, dim3(kT), 0, st, zs, dw, db, a0, nb, latent_dim, U);
            RML_HIP(hipGetLastError());
            for (int l = 0; l < n_up; ++l) {
                const uint16_t* w = static_cast<const uint16_t*>(up_wt) + ((int64_t)br * n_up + l) * wt_layer;
                const float* b = up_bias + ((int64_t)br * n_up + l) * C;
                int rc = launch_up(bufs[l & 1], dtype, nb, base << l, base << l, w, b, bufs[(l + 1) & 1], st);
                if (rc) return rc;
            }
            int rc = rml_conv7_tanh_forward(ctx, bufs[n_up & 1], dtype, nb, gp.S, gp.S, C, out_w + (int64_t)br * 49 * C, out_b + br,
                                            ys[br] + s0 * (int64_t)gp.S * gp.S, stream);
            if (rc) return rc;
        }
    }
    return RML_OK;
}
