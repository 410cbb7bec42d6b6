// Inference trunk of the SGAN classifier (the reference's c_model, sgan.py:132-199) for gfx950: per projection branch
//   Conv2D(1->128, 3x3, stride 2, 'same') -> Conv2D(128->64, s2) -> Conv2D(64->32, s2), each followed by BatchNorm and LeakyReLU,
// the three branches concatenated on the channel axis and flattened in NHWC order -- the (H/8)(W/8)*96-long bf16 feature rows the dense
// tail (dense.hip, rml_dense_tail_lrelu) reads.  In inference mode a BatchNorm is an affine map: the caller folds it into the weights
// and biases in front of it (sgan.py, folded_packs), so a layer here is convolution + bias + LeakyReLU.
//
// Three launches per call:
//  * k_sgan_pack: the two implicit-GEMM kernels' weights from the C ABI's [cout][k] rows into MFMA operand order, in the workspace
//    (553 KB; every slab the other kernels stage is then one contiguous, lane-contiguous read);
//  * k_sgan_conv12: layers 1 and 2.  The layer-1 activation (64x64x128 bf16 = 1 MB per sample and branch at 128x128) never exists:
//    as in k_dnn_trunk_rf (dnn.hip) conv1 is evaluated on the matrix cores AT the 32 conv1 pixels a tap of a 32-pixel conv2 tile
//    reads -- v_mfma_f32_32x32x16_bf16, M = 32 channels (A = the weights), N = the pixels, K = 9 taps + 3 bias slots + zeros --,
//    bias + LeakyReLU are applied to the float32 accumulators, and the accumulators, rounded to bf16, ARE the B operands of that
//    tap's conv2 MFMAs (K = 16 conv1 channels per instruction, in the accumulator's own permuted channel order; the packed weights
//    use the same one).  conv1 is recomputed 2.25 times: 4 MFMAs beside the 16 of conv2 per tap, +25 %.
//    Layer 2's weights (147 KB per branch) are streamed per tap: one tap = a 128 x 64 bf16 slab = 16 KB, two LDS stages, the eight
//    waves of a workgroup in step over the taps with one LDS-only barrier each, every wave on its own tile of 32 conv2 pixels
//    (two accumulator tiles: 64 output channels).  A tile's input windows come straight from the planes (L1 / L2: a 128x128 plane
//    is 32-64 KB and a workgroup's eight tiles are neighbours), one tap ahead in registers.
//  * k_sgan_conv3: layer 3 as an implicit GEMM on the layer-2 activation in the workspace (128 KB per sample and branch): M = 32
//    output channels, N = 32 output pixels per wave, K = 9 x 64; a lane's B fragment is 16 contiguous bytes of one input pixel.
// The conv1 bias rides in THREE bf16 K slots (= the float32 bias, see k_dnn_trunk_rf); the biases of layers 2 and 3 are added in
// float32 to the accumulators.  bf16 operands, float32 accumulation, bf16 activations.
// Every output element has one owner and one summation order that depends on (H, W) alone -- no atomics, no split sums: a sample's
// features are the same bits alone, at any position of any batch, and on a second call.
#include "rml_internal.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int C1 = 128, C2 = 64, C3 = 32, KTAPS = 9;
constexpr int K2 = KTAPS * C1;                  // 1152
constexpr int K3 = KTAPS * C2;                  // 576
constexpr int SLAB2 = C1 * C2 / 8;              // 16-byte chunks of one tap of layer 2: 1024 (16 KB)
constexpr int SLAB3 = C2 * C3 / 8;              // ... of layer 3: 256 (4 KB)
constexpr int WAVES = 8;                        // waves (conv2 tiles in flight) per workgroup of k_sgan_conv12
constexpr int64_t WP2_BYTES = (int64_t)3 * KTAPS * SLAB2 * 16;     // 442 368
constexpr int64_t WP3_BYTES = (int64_t)3 * KTAPS * SLAB3 * 16;     // 110 592
constexpr int MAX_H = 1 << 15;

struct SganArgs {
    const void* in[3];      // (B, H, W) per branch: float32, or bf16 (template INBF)
    int64_t B;
    int H, W;
    const float* w1;        // [3][128][9]
    const float* b1;        // [3][128]
    const float* b2;        // [3][64]
    const float* b3;        // [3][32]
    const uint4* wp2;       // [3][9][8 k-steps][2 channel tiles][64 lanes] 16 B: conv2 A operands
    const uint4* wp3;       // [3][9][4 k-steps][64 lanes] 16 B: conv3 A operands
    float slope;
    uint16_t* act2;         // [3][B][(H/4)(W/4)][64] bf16
    uint16_t* feat;         // [B][(H/8)(W/8)*96] bf16
    int rounds;             // k_sgan_conv12: tile rounds per workgroup (the same for every workgroup: barriers inside)
};

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {     // v_cvt_pk_bf16_f32 (round to nearest even)
    bf16x2 b = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
    return *reinterpret_cast<uint32_t*>(&b);
}
// x > 0 ? x : slope * x for 0 <= slope <= 1 (the entry point checks): two instructions, no compare
__device__ __forceinline__ float lrelu(float x, float slope) { return fmaxf(x, slope * x); }

// LDS-only barrier: __syncthreads() would also drain vmcnt, i.e. wait for the prefetched windows and weight slab
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// w2t [3][64][1152], w3t [3][32][576] (k = tap * Cin + cin) -> operand order.  Layer 2, chunk (tap t, k-step s, channel tile mt, lane
// l = (m, h)): output channel 32 mt + m, input channels 16 s + 8 (i / 4) + 4 h + i % 4, i = 0..7 -- the order the conv1 accumulators of
// a lane come in.  Layer 3, chunk (t, s, l): output channel m, input channels 16 s + 8 h + i.
__global__ __launch_bounds__(256) void k_sgan_pack(const uint16_t* __restrict__ w2t, const uint16_t* __restrict__ w3t, uint4* __restrict__ wp2,
                                                   uint4* __restrict__ wp3) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    constexpr int n2 = 3 * KTAPS * SLAB2, n3 = 3 * KTAPS * SLAB3;
    if (i < n2) {
        const int br = i / (KTAPS * SLAB2), r = i - br * (KTAPS * SLAB2);
        const int t = r / SLAB2, c = r - t * SLAB2, s = c >> 7, mt = (c >> 6) & 1, l = c & 63;
        const uint16_t* g = w2t + (size_t)(br * C2 + mt * 32 + (l & 31)) * K2 + t * C1 + 16 * s + 4 * (l >> 5);
        const uint2 lo = *reinterpret_cast<const uint2*>(g), hi = *reinterpret_cast<const uint2*>(g + 8);
        wp2[i] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    } else if (i < n2 + n3) {
        const int j = i - n2;
        const int br = j / (KTAPS * SLAB3), r = j - br * (KTAPS * SLAB3);
        const int t = r / SLAB3, c = r - t * SLAB3, s = c >> 6, l = c & 63;
        wp3[j] = *reinterpret_cast<const uint4*>(w3t + (size_t)(br * C3 + (l & 31)) * K3 + t * C2 + 16 * s + 8 * (l >> 5));
    }
}

template <bool INBF>
__global__ __launch_bounds__(64 * WAVES) void k_sgan_conv12(SganArgs a) {
    __shared__ uint4 wlds[2][SLAB2];            // two stages of one tap's conv2 weights
    const int H = a.H, W = a.W, OH1 = H / 2, OW1 = W / 2, OW2 = W / 4, P2 = (H / 4) * OW2;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int br = blockIdx.y;
    const int NT = (P2 + 31) >> 5;              // conv2 tiles of 32 pixels per sample
    const int64_t U = a.B * NT;                 // work units (sample, tile)
    const float slope = a.slope;

    // conv1 weights as A operands: lane (channel 32 ct + n, k-group h).  K slots of a window: k-group 0 [r0c0 r0c1 r0c2 r0c3 r1c0 r1c1
    // r1c2 r1c3] with weights [w00 w01 w02 0 w10 w11 w12 0]; k-group 1 [r2c0 r2c1 r2c2 r2c3 1 1 1 0] with [w20 w21 w22 0 bias-hi bias-mid
    // bias-lo 0]: bf16(bias) + bf16 of what that left + bf16 of what that left = the float32 bias to 24 bits
    bf16x8 w1f[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const float* wr = a.w1 + (size_t)(br * C1 + ct * 32 + n) * KTAPS;
        const float bias = a.b1[br * C1 + ct * 32 + n];
        uint4 u;
        if (h == 0) u = make_uint4(pk_bf16(wr[0], wr[1]), pk_bf16(wr[2], 0.f), pk_bf16(wr[3], wr[4]), pk_bf16(wr[5], 0.f));
        else {
            const float bh = __uint_as_float(pk_bf16(bias, 0.f) << 16);
            const float r1 = bias - bh;
            const float bm = __uint_as_float(pk_bf16(r1, 0.f) << 16);
            u = make_uint4(pk_bf16(wr[6], wr[7]), pk_bf16(wr[8], 0.f), pk_bf16(bias, r1), pk_bf16(r1 - bm, 0.f));
        }
        w1f[ct] = *reinterpret_cast<bf16x8*>(&u);
    }

    const uint4* __restrict__ wsrc = a.wp2 + (size_t)br * KTAPS * SLAB2;
    wlds[0][tid] = wsrc[tid];
    wlds[0][tid + 64 * WAVES] = wsrc[tid + 64 * WAVES];

    for (int round = 0; round < a.rounds; ++round) {
        // the wave's tile; units past the end recompute the last one and store nothing (every wave keeps to the barriers)
        const int64_t u = ((int64_t)round * gridDim.x + blockIdx.x) * WAVES + wave;
        const bool uvalid = u < U;
        const int64_t uc = uvalid ? u : U - 1;
        const int64_t b = uc / NT;
        const int tile = (int)(uc - b * NT);
        const int q = tile * 32 + n;
        const bool live = uvalid && q < P2;
        const int qc = q < P2 ? q : P2 - 1;
        const int pr = qc / OW2, pc = qc - pr * OW2;
        const unsigned char* __restrict__ plane = static_cast<const unsigned char*>(a.in[br]) + b * (int64_t)H * W * (INBF ? 2 : 4);

        // two neighbouring plane values (col even) as a bf16 pair; 0 where the window leaves the plane ('same': bottom / right)
        auto ld2 = [&](int row, int col, bool ok) -> uint32_t {
            const int off = ok ? row * W + col : 0;
            uint32_t v;
            if (INBF) v = *reinterpret_cast<const uint32_t*>(plane + (size_t)off * 2);
            else {
                const float2 f = *reinterpret_cast<const float2*>(plane + (size_t)off * 4);
                v = pk_bf16(f.x, f.y);
            }
            return ok ? v : 0u;
        };
        // the B operand of conv1 at the conv1 pixel tap t of this lane's conv2 pixel reads.  A conv1 pixel in row OH1 / column OW1 is
        // conv2's 'same' padding: window and bias slots all zero, so it comes out as LeakyReLU(0) = 0
        auto gather = [&](int t) -> bf16x8 {
            const int ky = t / 3, kx = t - ky * 3;
            const int y1 = 2 * pr + ky, x1 = 2 * pc + kx;
            const bool v1 = y1 < OH1 && x1 < OW1;
            const int iy = 2 * y1 + 2 * h, ix = 2 * x1;         // k-group 0: window rows 0 and 1; k-group 1: row 2
            const bool okA = v1 && iy < H, okC = ix + 2 < W, okB = v1 && h == 0;
            uint4 w;
            w.x = ld2(iy, ix, okA);
            // (the second pair's high half is window column 3, a zero-weight slot: masked, so that a non-finite plane value there
            // cannot reach a pixel whose window does not hold it)
            w.y = ld2(iy, ix + 2, okA && okC) & 0xFFFFu;
            const uint32_t bz = ld2(iy + 1, ix, okB), bw = ld2(iy + 1, ix + 2, okB && okC) & 0xFFFFu;
            w.z = h ? (v1 ? 0x3F803F80u : 0u) : bz;
            w.w = h ? (v1 ? 0x00003F80u : 0u) : bw;
            return *reinterpret_cast<bf16x8*>(&w);
        };

        f32x16 acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
        bf16x8 win = gather(0);
#pragma unroll
        for (int t = 0; t < KTAPS; ++t) {
            // the next tap's slab (tap 0 of the next round behind tap 8) and window: in flight under this tap's MFMAs
            const int tn = t + 1 < KTAPS ? t + 1 : 0;
            const uint4 g0 = wsrc[tn * SLAB2 + tid], g1 = wsrc[tn * SLAB2 + tid + 64 * WAVES];
            bf16x8 winn = win;
            if (t + 1 < KTAPS) winn = gather(t + 1);
            // conv1 at the tap's 32 pixels, bias included; LeakyReLU in float32; bf16: registers 8 j .. 8 j + 7 of channel tile ct are the
            // B fragment of conv2's k-step 2 ct + j
            bf16x8 p[8];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                f32x16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                const f32x16 c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1f[ct], win, z, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    uint4 v;
                    v.x = pk_bf16(lrelu(c[8 * j], slope), lrelu(c[8 * j + 1], slope));
                    v.y = pk_bf16(lrelu(c[8 * j + 2], slope), lrelu(c[8 * j + 3], slope));
                    v.z = pk_bf16(lrelu(c[8 * j + 4], slope), lrelu(c[8 * j + 5], slope));
                    v.w = pk_bf16(lrelu(c[8 * j + 6], slope), lrelu(c[8 * j + 7], slope));
                    p[2 * ct + j] = *reinterpret_cast<bf16x8*>(&v);
                }
            }
            // this tap's stage (written during the previous tap) is complete and visible; the other stage (read during the previous
            // tap) is free for the next slab
            lds_barrier();
            const int stage = (round + t) & 1;          // 9 taps per round: the parity of round * 9 + t
            const uint4* st = wlds[stage] + lane;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const uint4 wv = st[(s * 2 + mt) * 64];
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&wv), p[s], acc[mt], 0, 0, 0);
                }
            }
            wlds[stage ^ 1][tid] = g0;
            wlds[stage ^ 1][tid + 64 * WAVES] = g1;
            win = winn;
        }
        // bias + LeakyReLU in float32, bf16; accumulator registers 4 j .. 4 j + 3 of tile mt are channels 32 mt + 8 j + 4 h ..: 8-byte stores
        uint16_t* dst = a.act2 + (((int64_t)br * a.B + b) * P2 + qc) * C2 + 4 * h;
        const float* bias = a.b2 + br * C2 + 4 * h;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* bb = bias + mt * 32 + 8 * j;
                const uint2 o = make_uint2(pk_bf16(lrelu(acc[mt][4 * j] + bb[0], slope), lrelu(acc[mt][4 * j + 1] + bb[1], slope)),
                                           pk_bf16(lrelu(acc[mt][4 * j + 2] + bb[2], slope), lrelu(acc[mt][4 * j + 3] + bb[3], slope)));
                if (live) *reinterpret_cast<uint2*>(dst + mt * 32 + 8 * j) = o;
            }
    }
}

__global__ __launch_bounds__(256) void k_sgan_conv3(SganArgs a) {
    __shared__ uint4 w3s[KTAPS * SLAB3];        // 36 KB: the branch's weights in operand order
    const int OH2 = a.H / 4, OW2 = a.W / 4, P2 = OH2 * OW2, OW3 = a.W / 8, P3 = (a.H / 8) * OW3;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5, wave = tid >> 6;
    const int br = blockIdx.y;
    for (int i = tid; i < KTAPS * SLAB3; i += 256) w3s[i] = a.wp3[(size_t)br * KTAPS * SLAB3 + i];
    __syncthreads();
    const int NT = (P3 + 31) >> 5;
    const int64_t U = a.B * NT;
    const float slope = a.slope;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u < U; u += (int64_t)gridDim.x * 4) {
        const int64_t b = u / NT;
        const int tile = (int)(u - b * NT);
        const int q = tile * 32 + n;
        const bool live = q < P3;
        const int qc = live ? q : P3 - 1;
        const int pr = qc / OW3, pc = qc - pr * OW3;
        const uint16_t* __restrict__ src = a.act2 + ((int64_t)br * a.B + b) * P2 * C2;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int t = 0; t < KTAPS; ++t) {
            const int ky = t / 3, kx = t - ky * 3;
            const int y2 = 2 * pr + ky, x2 = 2 * pc + kx;
            const bool ok = y2 < OH2 && x2 < OW2;           // row OH2 / column OW2: 'same' zeros
            // k-step s of the lane: input channels 16 s + 8 h ..+ 7 of the pixel = 16 contiguous bytes
            const uint4* px = reinterpret_cast<const uint4*>(src + (size_t)(ok ? y2 * OW2 + x2 : 0) * C2) + h;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                uint4 v = px[2 * s];
                if (!ok) v = make_uint4(0, 0, 0, 0);
                const uint4 wv = w3s[(t * 4 + s) * 64 + lane];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&wv), *reinterpret_cast<const bf16x8*>(&v), acc, 0, 0, 0);
            }
        }
        // feat[b][(pixel)*96 + branch*32 + channel]: registers 4 j .. 4 j + 3 are channels 8 j + 4 h ..
        uint16_t* dst = a.feat + (b * P3 + qc) * 96 + br * C3 + 4 * h;
        const float* bias = a.b3 + br * C3 + 4 * h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* bb = bias + 8 * j;
            const uint2 o = make_uint2(pk_bf16(lrelu(acc[4 * j] + bb[0], slope), lrelu(acc[4 * j + 1] + bb[1], slope)),
                                       pk_bf16(lrelu(acc[4 * j + 2] + bb[2], slope), lrelu(acc[4 * j + 3] + bb[3], slope)));
            if (live) *reinterpret_cast<uint2*>(dst + 8 * j) = o;
        }
    }
}

}  // namespace

extern "C" int rml_sgan_trunk_supported(int H, int W) {
    return H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && W <= 128 && H <= MAX_H;
}

extern "C" int64_t rml_sgan_trunk_workspace_bytes(int64_t B, int H, int W) {
    if (B < 0 || !rml_sgan_trunk_supported(H, W)) return 0;
    return WP2_BYTES + WP3_BYTES + (int64_t)3 * B * (H / 4) * (W / 4) * C2 * 2;
}

extern "C" int rml_sgan_trunk(rml_ctx* ctx, const void* xz, const void* yz, const void* xy, int in_bf16, int64_t B, int H, int W,
                              const float* w1, const float* b1, const uint16_t* w2t, const float* b2, const uint16_t* w3t,
                              const float* b3, float slope, uint16_t* feat, void* workspace, int64_t workspace_bytes, void* stream) {
    RML_REQUIRE(ctx && B >= 0, RML_ERR_INVALID, "rml_sgan_trunk: bad arguments");
    RML_REQUIRE(rml_sgan_trunk_supported(H, W), RML_ERR_UNSUPPORTED,
                "rml_sgan_trunk: planes of %dx%d: H and W must be multiples of 8, W <= 128, H <= %d", H, W, MAX_H);
    RML_REQUIRE(slope >= 0.0f && slope <= 1.0f, RML_ERR_UNSUPPORTED, "rml_sgan_trunk: LeakyReLU slope %g outside [0, 1]", (double)slope);
    if (B == 0) return RML_OK;
    RML_REQUIRE(xz && yz && xy && w1 && b1 && w2t && b2 && w3t && b3 && feat && workspace, RML_ERR_INVALID, "rml_sgan_trunk: NULL argument");
    RML_REQUIRE(B * (int64_t)(H / 4) * (W / 4) < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "rml_sgan_trunk: B too large");
    const uintptr_t al = reinterpret_cast<uintptr_t>(xz) | reinterpret_cast<uintptr_t>(yz) | reinterpret_cast<uintptr_t>(xy) |
                         reinterpret_cast<uintptr_t>(w2t) | reinterpret_cast<uintptr_t>(w3t) | reinterpret_cast<uintptr_t>(feat) |
                         reinterpret_cast<uintptr_t>(workspace);
    RML_REQUIRE((al & 15) == 0, RML_ERR_INVALID, "rml_sgan_trunk: planes, w2t, w3t, feat and the workspace must be 16-byte aligned");
    RML_REQUIRE(workspace_bytes >= rml_sgan_trunk_workspace_bytes(B, H, W), RML_ERR_INVALID, "rml_sgan_trunk: workspace too small");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    SganArgs a{};
    a.in[0] = xz; a.in[1] = yz; a.in[2] = xy; a.B = B; a.H = H; a.W = W;
    a.w1 = w1; a.b1 = b1; a.b2 = b2; a.b3 = b3; a.slope = slope; a.feat = feat;
    a.wp2 = reinterpret_cast<const uint4*>(ws);
    a.wp3 = reinterpret_cast<const uint4*>(ws + WP2_BYTES);
    a.act2 = reinterpret_cast<uint16_t*>(ws + WP2_BYTES + WP3_BYTES);
    constexpr int npack = 3 * KTAPS * (SLAB2 + SLAB3);
    hipLaunchKernelGGL(k_sgan_pack, dim3((npack + 255) / 256), dim3(256), 0, st, w2t, w3t, reinterpret_cast<uint4*>(ws),
                       reinterpret_cast<uint4*>(ws + WP2_BYTES));
    const int64_t u2 = B * (((H / 4) * (W / 4) + 31) / 32);
    const int64_t need2 = (u2 + WAVES - 1) / WAVES;
    const int64_t g2 = need2 < ctx->num_cu ? need2 : ctx->num_cu;
    a.rounds = (int)((need2 + g2 - 1) / g2);
    if (in_bf16) hipLaunchKernelGGL(k_sgan_conv12<true>, dim3((unsigned)g2, 3), dim3(64 * WAVES), 0, st, a);
    else hipLaunchKernelGGL(k_sgan_conv12<false>, dim3((unsigned)g2, 3), dim3(64 * WAVES), 0, st, a);
    const int64_t u3 = B * (((H / 8) * (W / 8) + 31) / 32);
    const int64_t need3 = (u3 + 3) / 4, cap3 = (int64_t)4 * ctx->num_cu;
    hipLaunchKernelGGL(k_sgan_conv3, dim3((unsigned)(need3 < cap3 ? need3 : cap3), 3), dim3(256), 0, st, a);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
