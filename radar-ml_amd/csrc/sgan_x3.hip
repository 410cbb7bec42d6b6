// The trunk of the SGAN classifier (sgan.py:132-199; the layers of sgan_infer.hip) at float32-class accuracy on the bf16 matrix cores:
// the second opinion of the margin guard (radar-ml_amd/sgan.py Discriminator.rescore_exact), for the handful of rows whose two largest
// probabilities the bf16 chain cannot tell apart.  Throughput is not a goal here; one owner and one order per sum is.
//
// The arithmetic is dnn_x3.hip's: every float32 operand x is carried as NS bf16 numbers (part 0 = bf16(x), part 1 = bf16 of what that
// rounding left, part 2 = bf16 of what THAT left), every product as the v_mfma_f32_32x32x16_bf16 products of the part pairs (i, j) with
// i + j < NS, the smallest terms first, accumulated in float32.  NS = 2 ("x3"): 16 significant bits, three products, what is dropped
// is <= 2^-16 |a b|; NS = 3 ("x6"): 24 bits, six products, float32-class in the strict sense.
//
// Three launches per call, the structure of sgan_infer.hip without its LDS pipeline:
//  * k_sx_pack<NS>: the float32 weights of layers 2 and 3, split into parts, in MFMA operand order in the workspace (every fragment a
//    wave reads is then one lane-contiguous 1 KB run, shared by the waves of a workgroup through the vector cache);
//  * k_sx_conv12<NS>: layers 1 and 2.  As in k_sgan_conv12 the layer-1 activation never exists: conv1 is evaluated AT the 32 conv1 pixels
//    a tap of a wave's 32-pixel conv2 tile reads (M = 32 channels, K = 9 taps + 3 bias slots + zeros), bias + LeakyReLU in float32, and
//    the float32 accumulators, split in registers, ARE the B operands of that tap's conv2 products.  Windows come straight from the
//    float32 planes; no LDS, no barrier: a wave is on its own.
//  * k_sx_conv3<NS>: layer 3 as an implicit GEMM on the float32 layer-2 activation in the workspace.
// conv1's bias rides in three K slots of the part-0 fragment (three bf16 pieces = the float32 bias, the pixel side holds 1.0); the
// biases of layers 2 and 3 start the accumulators: all exact.  A tile's sums run tap by tap, k-step by k-step, part pair by part
// pair in one fixed order that depends on (H, W) alone, every output element has one owner, there are no atomics: a sample's features
// are the same bits alone, at any position of any batch, and on a second call.
// In: float32 planes, float32 folded weights.  Out: float32 features feat[b][(h*(W/8)+w)*96 + branch*32 + n] -- the float32 LeakyReLU
// tail (dense.hip, rml_dense_tail_lrelu_f32) runs on them.
#include "rml_internal.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int C1 = 128, C2 = 64, C3 = 32, KTAPS = 9;
constexpr int K2 = KTAPS * C1;                  // 1152
constexpr int K3 = KTAPS * C2;                  // 576
constexpr int FRAG2 = KTAPS * 8 * 2;            // conv2 A fragments per branch and part: (tap, k-step, channel tile), 64 lanes x 16 B each
constexpr int FRAG3 = KTAPS * 4;                // conv3: (tap, k-step)
constexpr int MAX_PARTS = 3;
constexpr int64_t WP2_BYTES = (int64_t)3 * FRAG2 * MAX_PARTS * 1024;       // 1 327 104
constexpr int64_t WP3_BYTES = (int64_t)3 * FRAG3 * MAX_PARTS * 1024;       //   331 776
constexpr int WAVES = 4;                        // waves (tiles in flight) per workgroup
constexpr int MAX_HW = 1 << 12;

struct SxArgs {
    const float* in[3];     // (B, H, W) float32 per branch
    int64_t B;
    int H, W;
    const float* w1;        // [3][128][9]
    const float* b1;        // [3][128]
    const float* w2;        // [3][64][1152], k = (ky*3+kx)*128 + cin
    const float* b2;        // [3][64]
    const float* w3;        // [3][32][576], k = (ky*3+kx)*64 + cin
    const float* b3;        // [3][32]
    uint4* wp2;             // [3][9][8 k-steps][2 channel tiles][NS][64 lanes] 16 B: conv2 A operands
    uint4* wp3;             // [3][9][4 k-steps][NS][64 lanes] 16 B: conv3 A operands
    float slope;
    float* act2;            // [3][B][(H/4)(W/4)][64] float32
    float* feat;            // [B][(H/8)(W/8)*96] float32
};

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {     // v_cvt_pk_bf16_f32 (round to nearest even)
    bf16x2 b = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
    return *reinterpret_cast<uint32_t*>(&b);
}
// x > 0 ? x : slope * x for 0 <= slope <= 1 (the entry point checks)
__device__ __forceinline__ float lrelu(float x, float slope) { return fmaxf(x, slope * x); }

// (x0, x1) -> NS packed bf16 pairs, as dnn_x3.hip's split2 / split8
template <int NS>
__device__ __forceinline__ void split2(float x0, float x1, uint32_t (&part)[NS]) {
#pragma unroll
    for (int p = 0; p < NS; ++p) {
        part[p] = pk_bf16(x0, x1);
        if (p + 1 < NS) {
            x0 -= __uint_as_float(part[p] << 16);
            x1 -= __uint_as_float(part[p] & 0xFFFF0000u);
        }
    }
}
template <int NS>
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, bf16x8 (&part)[NS]) {
    uint32_t q[4][NS];
    split2<NS>(a[0], a[1], q[0]); split2<NS>(a[2], a[3], q[1]);
    split2<NS>(b[0], b[1], q[2]); split2<NS>(b[2], b[3], q[3]);
#pragma unroll
    for (int p = 0; p < NS; ++p) {
        uint4 u = make_uint4(q[0][p], q[1][p], q[2][p], q[3][p]);
        part[p] = *reinterpret_cast<bf16x8*>(&u);
    }
}
// acc += sum over part pairs (i, j), i + j < NS, of A_i x B_j, the smallest terms first
template <int NS>
__device__ __forceinline__ f32x16 mfma_parts(const bf16x8 (&A)[NS], const bf16x8 (&B)[NS], f32x16 acc) {
#pragma unroll
    for (int sum = NS - 1; sum >= 0; --sum)
#pragma unroll
        for (int i = sum; i >= 0; --i)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[i], B[sum - i], acc, 0, 0, 0);
    return acc;
}

// w2 [3][64][1152], w3 [3][32][576] float32 -> parts in operand order.  Layer 2, fragment (tap t, k-step s, channel tile mt), lane l = (m,
// h): output channel 32 mt + m, input channels 16 s + 8 (i / 4) + 4 h + i % 4, i = 0..7 -- the order the conv1 accumulators of a lane
// come in.  Layer 3, fragment (t, s), lane (m, h): output channel m, input channels 16 s + 8 h + i.
template <int NS>
__global__ __launch_bounds__(256) void k_sx_pack(SxArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    constexpr int n2 = 3 * FRAG2 * 64, n3 = 3 * FRAG3 * 64;
    if (i < n2) {
        const int l = i & 63, f = i >> 6;                   // f = (br * 9 + t) * 16 + s * 2 + mt
        const int mt = f & 1, s = (f >> 1) & 7, bt = f >> 4, br = bt / KTAPS, t = bt - br * KTAPS;
        const float* g = a.w2 + (size_t)(br * C2 + mt * 32 + (l & 31)) * K2 + t * C1 + 16 * s + 4 * (l >> 5);
        bf16x8 wp[NS];
        split8<NS>(*reinterpret_cast<const f32x4*>(g), *reinterpret_cast<const f32x4*>(g + 8), wp);
#pragma unroll
        for (int p = 0; p < NS; ++p) a.wp2[((size_t)f * NS + p) * 64 + l] = *reinterpret_cast<uint4*>(&wp[p]);
    } else if (i < n2 + n3) {
        const int j = i - n2, l = j & 63, f = j >> 6;       // f = (br * 9 + t) * 4 + s
        const int s = f & 3, bt = f >> 2, br = bt / KTAPS, t = bt - br * KTAPS;
        const float* g = a.w3 + (size_t)(br * C3 + (l & 31)) * K3 + t * C2 + 16 * s + 8 * (l >> 5);
        bf16x8 wp[NS];
        split8<NS>(*reinterpret_cast<const f32x4*>(g), *reinterpret_cast<const f32x4*>(g + 4), wp);
#pragma unroll
        for (int p = 0; p < NS; ++p) a.wp3[((size_t)f * NS + p) * 64 + l] = *reinterpret_cast<uint4*>(&wp[p]);
    }
}

template <int NS>
__global__ __launch_bounds__(64 * WAVES) void k_sx_conv12(SxArgs a) {
    const int H = a.H, W = a.W, OH1 = H / 2, OW1 = W / 2, OW2 = W / 4, P2 = (H / 4) * OW2;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5, wave = tid >> 6;
    const int br = blockIdx.y;
    const int NT = (P2 + 31) >> 5;              // conv2 tiles of 32 pixels per sample
    const int64_t U = a.B * NT;                 // work units (sample, tile)
    const float slope = a.slope;

    // conv1 weights as A operands: lane (channel 32 ct + n, k-group h).  K slots of a window: k-group 0 [r0c0 r0c1 r0c2 r0c3 r1c0 r1c1
    // r1c2 r1c3] with weights [w00 w01 w02 0 w10 w11 w12 0]; k-group 1 [r2c0 r2c1 r2c2 r2c3 1 1 1 0] with [w20 w21 w22 0 bias bias'
    // bias'' 0]: three bf16 pieces in part 0 = the float32 bias to 24 bits; the other parts hold zeros there
    bf16x8 w1p[4][NS];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const float* wr = a.w1 + (size_t)(br * C1 + ct * 32 + n) * KTAPS;
        const float bias = a.b1[br * C1 + ct * 32 + n];
        uint32_t q[4][NS];
        if (h == 0) {
            split2<NS>(wr[0], wr[1], q[0]); split2<NS>(wr[2], 0.f, q[1]);
            split2<NS>(wr[3], wr[4], q[2]); split2<NS>(wr[5], 0.f, q[3]);
        } else {
            split2<NS>(wr[6], wr[7], q[0]); split2<NS>(wr[8], 0.f, q[1]);
            const float bh = __uint_as_float(pk_bf16(bias, 0.f) << 16);
            const float r1 = bias - bh;
            const float bm = __uint_as_float(pk_bf16(r1, 0.f) << 16);
#pragma unroll
            for (int p = 0; p < NS; ++p) { q[2][p] = 0; q[3][p] = 0; }
            q[2][0] = pk_bf16(bias, r1); q[3][0] = pk_bf16(r1 - bm, 0.f);
        }
#pragma unroll
        for (int p = 0; p < NS; ++p) {
            uint4 u = make_uint4(q[0][p], q[1][p], q[2][p], q[3][p]);
            w1p[ct][p] = *reinterpret_cast<bf16x8*>(&u);
        }
    }
    const uint4* __restrict__ wsrc = a.wp2 + (size_t)br * FRAG2 * NS * 64 + lane;
    const float* __restrict__ bias2 = a.b2 + br * C2 + 4 * h;

    // persistent: wave w of the grid takes units w, w + #waves, ...; a wave meets no barrier, so the trip counts may differ
    for (int64_t u = (int64_t)blockIdx.x * WAVES + wave; u < U; u += (int64_t)gridDim.x * WAVES) {
        const int64_t b = u / NT;
        const int tile = (int)(u - b * NT);
        const int q = tile * 32 + n;
        const bool live = q < P2;
        const int qc = live ? q : P2 - 1;
        const int pr = qc / OW2, pc = qc - pr * OW2;
        const float* __restrict__ plane = a.in[br] + b * (int64_t)H * W;

        // two neighbouring plane values (col even: 8-byte aligned); 0 where the window leaves the plane ('same': bottom / right)
        auto ld2 = [&](int row, int col, bool ok) -> f32x2 {
            const f32x2 v = *reinterpret_cast<const f32x2*>(plane + (ok ? row * W + col : 0));
            return ok ? v : f32x2{0.f, 0.f};
        };
        // accumulator registers 4 j .. 4 j + 3 of tile mt are channels 32 mt + 8 j + 4 h ..: the bias starts them
        f32x16 acc[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 bb = *reinterpret_cast<const f32x4*>(bias2 + mt * 32 + 8 * j);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mt][4 * j + r] = bb[r];
            }
#pragma unroll 1
        for (int t = 0; t < KTAPS; ++t) {
            // the B operand of conv1 at the conv1 pixel tap t of this lane's conv2 pixel reads.  A conv1 pixel in row OH1 / column OW1 is
            // conv2's 'same' padding: window and bias slots all zero, so it comes out as LeakyReLU(0) = 0
            const int ky = t / 3, kx = t - ky * 3;
            const int y1 = 2 * pr + ky, x1 = 2 * pc + kx;
            const bool v1 = y1 < OH1 && x1 < OW1;
            const int iy = 2 * y1 + 2 * h, ix = 2 * x1;             // k-group 0: window rows 0 and 1; k-group 1: row 2
            const bool okA = v1 && iy < H, okC = ix + 2 < W, okB = v1 && h == 0;
            const f32x2 a0 = ld2(iy, ix, okA), a1 = ld2(iy, ix + 2, okA && okC);
            const f32x2 c0 = ld2(iy + 1, ix, okB), c1 = ld2(iy + 1, ix + 2, okB && okC);
            // (the second pair's high half is window column 3, a zero-weight slot: dropped, so that a non-finite plane value there cannot
            // reach a pixel whose window does not hold it)
            const f32x4 va = f32x4{a0[0], a0[1], a1[0], 0.f};
            const float one = v1 ? 1.f : 0.f;
            const f32x4 vb = h ? f32x4{one, one, one, 0.f} : f32x4{c0[0], c0[1], c1[0], 0.f};
            bf16x8 win[NS];
            split8<NS>(va, vb, win);
            const uint4* __restrict__ wt = wsrc + (size_t)t * 16 * NS * 64;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                f32x16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                const f32x16 c = mfma_parts<NS>(w1p[ct], win, z);
                // LeakyReLU in float32, then the split: registers 8 j .. 8 j + 7 of channel tile ct are the B fragment of conv2's k-step 2 ct + j
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    f32x4 lo, hi;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { lo[r] = lrelu(c[8 * j + r], slope); hi[r] = lrelu(c[8 * j + 4 + r], slope); }
                    bf16x8 pb[NS];
                    split8<NS>(lo, hi, pb);
                    const int s = 2 * ct + j;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        bf16x8 wa[NS];
#pragma unroll
                        for (int p = 0; p < NS; ++p) {
                            const uint4 wv = wt[(size_t)((s * 2 + mt) * NS + p) * 64];
                            wa[p] = *reinterpret_cast<const bf16x8*>(&wv);
                        }
                        acc[mt] = mfma_parts<NS>(wa, pb, acc[mt]);
                    }
                }
            }
        }
        // LeakyReLU in float32; a lane holds channels 32 mt + 8 j + 4 h + (0..3) of its pixel: 16-byte stores
        float* dst = a.act2 + (((int64_t)br * a.B + b) * P2 + qc) * C2 + 4 * h;
        if (live) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = lrelu(acc[mt][4 * j + r], slope);
                    *reinterpret_cast<f32x4*>(dst + mt * 32 + 8 * j) = o;
                }
        }
    }
}

template <int NS>
__global__ __launch_bounds__(64 * WAVES) void k_sx_conv3(SxArgs a) {
    const int OH2 = a.H / 4, OW2 = a.W / 4, P2 = OH2 * OW2, OW3 = a.W / 8, P3 = (a.H / 8) * OW3;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5, wave = tid >> 6;
    const int br = blockIdx.y;
    const int NT = (P3 + 31) >> 5;
    const int64_t U = a.B * NT;
    const float slope = a.slope;
    const uint4* __restrict__ wsrc = a.wp3 + (size_t)br * FRAG3 * NS * 64 + lane;
    const float* __restrict__ bias3 = a.b3 + br * C3 + 4 * h;
    for (int64_t u = (int64_t)blockIdx.x * WAVES + wave; u < U; u += (int64_t)gridDim.x * WAVES) {
        const int64_t b = u / NT;
        const int tile = (int)(u - b * NT);
        const int q = tile * 32 + n;
        const bool live = q < P3;
        const int qc = live ? q : P3 - 1;
        const int pr = qc / OW3, pc = qc - pr * OW3;
        const float* __restrict__ src = a.act2 + ((int64_t)br * a.B + b) * P2 * C2;
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bias3 + 8 * j);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[4 * j + r] = bb[r];
        }
#pragma unroll 1
        for (int t = 0; t < KTAPS; ++t) {
            const int ky = t / 3, kx = t - ky * 3;
            const int y2 = 2 * pr + ky, x2 = 2 * pc + kx;
            const bool ok = y2 < OH2 && x2 < OW2;           // row OH2 / column OW2: 'same' zeros
            // k-step s of the lane: input channels 16 s + 8 h ..+ 7 of the pixel = 32 contiguous bytes
            const f32x4* px = reinterpret_cast<const f32x4*>(src + (size_t)(ok ? y2 * OW2 + x2 : 0) * C2 + 8 * h);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                f32x4 v0 = px[4 * s], v1 = px[4 * s + 1];
                if (!ok) { v0 = f32x4{0.f, 0.f, 0.f, 0.f}; v1 = v0; }
                bf16x8 xb[NS], wa[NS];
                split8<NS>(v0, v1, xb);
#pragma unroll
                for (int p = 0; p < NS; ++p) {
                    const uint4 wv = wsrc[(size_t)((t * 4 + s) * NS + p) * 64];
                    wa[p] = *reinterpret_cast<const bf16x8*>(&wv);
                }
                acc = mfma_parts<NS>(wa, xb, acc);
            }
        }
        // feat[b][(pixel)*96 + branch*32 + channel]: registers 4 j .. 4 j + 3 are channels 8 j + 4 h ..
        float* dst = a.feat + (b * P3 + qc) * 96 + br * C3 + 4 * h;
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = lrelu(acc[4 * j + r], slope);
                *reinterpret_cast<f32x4*>(dst + 8 * j) = o;
            }
        }
    }
}

template <int NS>
void launch_sx(rml_ctx* ctx, const SxArgs& a, hipStream_t st) {
    constexpr int npack = 3 * (FRAG2 + FRAG3) * 64;
    hipLaunchKernelGGL(k_sx_pack<NS>, dim3((npack + 255) / 256), dim3(256), 0, st, a);
    const int64_t u2 = a.B * (((a.H / 4) * (a.W / 4) + 31) / 32);
    const int64_t need2 = (u2 + WAVES - 1) / WAVES;
    hipLaunchKernelGGL(k_sx_conv12<NS>, dim3((unsigned)(need2 < ctx->num_cu ? need2 : ctx->num_cu), 3), dim3(64 * WAVES), 0, st, a);
    const int64_t u3 = a.B * (((a.H / 8) * (a.W / 8) + 31) / 32);
    const int64_t need3 = (u3 + WAVES - 1) / WAVES;
    hipLaunchKernelGGL(k_sx_conv3<NS>, dim3((unsigned)(need3 < ctx->num_cu ? need3 : ctx->num_cu), 3), dim3(64 * WAVES), 0, st, a);
}

}  // namespace

extern "C" int rml_sgan_trunk_x3_supported(int H, int W) {
    return H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && H <= MAX_HW && W <= MAX_HW;
}

extern "C" int64_t rml_sgan_trunk_x3_workspace_bytes(int64_t B, int H, int W) {
    if (B < 0 || !rml_sgan_trunk_x3_supported(H, W)) return 0;
    return WP2_BYTES + WP3_BYTES + (int64_t)3 * B * (H / 4) * (W / 4) * C2 * 4;
}

extern "C" int rml_sgan_trunk_x3(rml_ctx* ctx, const float* xz, const float* yz, const float* xy, int64_t B, int H, int W, const float* w1,
                                 const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float slope, int parts,
                                 float* feat, void* workspace, int64_t workspace_bytes, void* stream) {
    RML_REQUIRE(ctx && B >= 0 && (parts == 2 || parts == 3), RML_ERR_INVALID, "rml_sgan_trunk_x3: bad arguments (parts: 2 or 3)");
    RML_REQUIRE(rml_sgan_trunk_x3_supported(H, W), RML_ERR_UNSUPPORTED,
                "rml_sgan_trunk_x3: planes of %dx%d: H and W must be multiples of 8, at most %d", H, W, MAX_HW);
    RML_REQUIRE(slope >= 0.0f && slope <= 1.0f, RML_ERR_UNSUPPORTED, "rml_sgan_trunk_x3: LeakyReLU slope %g outside [0, 1]", (double)slope);
    if (B == 0) return RML_OK;
    RML_REQUIRE(xz && yz && xy && w1 && b1 && w2 && b2 && w3 && b3 && feat && workspace, RML_ERR_INVALID, "rml_sgan_trunk_x3: NULL argument");
    RML_REQUIRE(B * (int64_t)(H / 4) * (W / 4) < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "rml_sgan_trunk_x3: B too large");
    const uintptr_t al = reinterpret_cast<uintptr_t>(xz) | reinterpret_cast<uintptr_t>(yz) | reinterpret_cast<uintptr_t>(xy) |
                         reinterpret_cast<uintptr_t>(w2) | reinterpret_cast<uintptr_t>(w3) | reinterpret_cast<uintptr_t>(b2) |
                         reinterpret_cast<uintptr_t>(b3) | reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(workspace);
    RML_REQUIRE((al & 15) == 0, RML_ERR_INVALID, "rml_sgan_trunk_x3: planes, w2, b2, w3, b3, feat and the workspace must be 16-byte aligned");
    RML_REQUIRE(workspace_bytes >= rml_sgan_trunk_x3_workspace_bytes(B, H, W), RML_ERR_INVALID, "rml_sgan_trunk_x3: workspace too small");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    SxArgs a{};
    a.in[0] = xz; a.in[1] = yz; a.in[2] = xy; a.B = B; a.H = H; a.W = W;
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.slope = slope; a.feat = feat;
    a.wp2 = reinterpret_cast<uint4*>(ws);
    a.wp3 = reinterpret_cast<uint4*>(ws + WP2_BYTES);
    a.act2 = reinterpret_cast<float*>(ws + WP2_BYTES + WP3_BYTES);
    if (parts == 2) launch_sx<2>(ctx, a, st);
    else launch_sx<3>(ctx, a, st);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
