// Training-mode 3x3 stride-2 convolutions of the SGAN discriminator (layers 2 and 3 of a projection branch, sgan.py:137-158) for
// gfx950: the forward pass and the two gradients autograd needs, on the matrix cores, without a convolution library.
//
// The operation is a VALID convolution of an already padded NHWC half tensor (what bn_lrelu_pad / conv1_bn_lrelu_pad write):
//   X (N, Hp, Wp, Cin), Hp = 2 Ho + 1, Wp = 2 Wo + 1;  W [Cout][ky][kx][Cin] (the channels_last storage of a (Cout, Cin, 3, 3) tensor,
//   k = tap * Cin + cin as in sgan_infer.hip);  Z (N, Ho, Wo, Cout).  float16 or bfloat16 operands (template BF), float32 accumulation on
//   v_mfma_f32_32x32x16_{f16,bf16}, every result rounded to the half type once.  No bias (the batch norm behind it cancels it).
//
//  * forward  Z[n,oy,ox,co] = sum X[n,2oy+ky,2ox+kx,ci] W[co,ky,kx,ci]: an implicit GEMM shaped like k_sgan_conv3 -- M = output
//    channels (A = the weights, packed into operand order in the workspace once per call), N = 32 pixels per wave, K = 9 Cin; a lane's
//    pixel fragment is 16 contiguous bytes of one input pixel.  One tap's weights (Cin x Cout halves) are a slab in LDS, two stages,
//    the four waves of a workgroup in step over the taps with one LDS-only barrier each (the layer-2 half of k_sgan_conv12).  Pixel
//    tiles run over the flattened (n, oy, ox) index: a tile may cross a row and a sample.
//  * data gradient  dX[n,y,x,ci] = sum over ky = y, kx = x (mod 2) and co of dZ[n,(y-ky)/2,(x-kx)/2,co] W[co,ky,kx,ci]: the four parity
//    classes of (y, x) are four implicit GEMMs of the same kernel (blockIdx.y) with 4, 2, 2 and 1 taps, K = taps * Cout, M = Cin; a
//    tap that falls outside dZ (rows / columns 0 and 2 Ho / 2 Wo) contributes a zero fragment.  The classes tile the whole padded dX,
//    its bottom / right pad row and column included: every element is written by exactly one lane.
//  * weight gradient  dW[co,ky,kx,ci] = sum over pixels of dZ[n,oy,ox,co] X[n,2oy+ky,2ox+kx,ci]: the sum runs over pixels and both
//    operands are stored channel-contiguous, so 64-pixel tiles of both are staged in LDS as they lie in memory and read transposed
//    with ds_read_b64_tr_b16 -- every lane of every wave takes part in every such read (EXEC all ones), lane addresses are multiples
//    of 8, the tile past the end of a piece is zero-filled rather than masked, and the LDS image is 16-byte aligned.  Rows are padded
//    by 64 bytes: the four pixel rows of a 16-lane group then fall on disjoint banks.  The pixel range is split into pieces whose
//    count and length follow from the pixel count alone (wgrad_plan: never from the CU count; the fixed K pieces of k_fc1_splitk);
//    a workgroup owns (piece, tap), writes float32 partials to the workspace, and k_conv_wreduce adds the pieces in index order and
//    rounds once.
//
// Properties:
//  - no atomics, no zeroed workspace: every workspace element that is read was written earlier in the same call;
//  - every output has ONE summation order, and it depends on the shapes alone: the same call gives the same bits;
//  - a sample's forward output is the same bits alone and at any position of any batch (an output's order is taps 0..8, channels in
//    16-wide steps, whatever tile it falls in);
//  - all three passes launch on the caller's stream, allocate nothing and never synchronise: they can be captured into a HIP graph.
#include "rml_internal.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int KTAPS = 9;
constexpr int IG_WAVES = 4;                 // waves (32-pixel tiles) per workgroup of k_conv_ig
constexpr int CHP = 64;                     // pixels per staged tile of k_conv_wgrad: four MFMA k-steps
constexpr int PIECE_MIN = 256;              // wgrad_plan: no more pieces than pixels / PIECE_MIN ...
constexpr int MAX_PIECES = 128;             // ... and at most this many
constexpr int MAX_EDGE = 8193;              // Hp, Wp

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
template <bool BF> __device__ __forceinline__ uint32_t pk2(float lo, float hi) { return (uint32_t)f2h<BF>(lo) | ((uint32_t)f2h<BF>(hi) << 16); }

template <bool BF> __device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b, const f32x16& c) {
    if constexpr (BF) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
    } else {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(&a), *reinterpret_cast<const f16x8*>(&b), c, 0, 0, 0);
    }
}

// LDS-only barrier: __syncthreads() would also drain vmcnt, i.e. wait for the prefetched fragments and weight slab
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- weights into operand order ------------------------------------------------------------------------------------------------------
// W [cout][9][cin] -> chunks of 16 bytes [tap][k-step s][M tile mt][lane l = (m, h)].  Forward: M = output channels: chunk = W[32 mt + m]
// [tap][16 s + 8 h ..+ 7], contiguous.  Data gradient: M = input channels, k = output channels: element i of the chunk =
// W[16 s + 8 h + i][tap][32 mt + m].
template <bool DGRAD>
__global__ __launch_bounds__(256) void k_conv_pack(const uint16_t* __restrict__ w, uint4* __restrict__ wp, int cin, int cout) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int MT = (DGRAD ? cin : cout) / 32, KS = (DGRAD ? cout : cin) / 16;
    if (i >= KTAPS * KS * MT * 64) return;
    const int l = i & 63, m = l & 31, h = l >> 5;
    int r = i >> 6;
    const int mt = r % MT;
    r /= MT;
    const int s = r % KS, t = r / KS;
    if (!DGRAD) {
        wp[i] = *reinterpret_cast<const uint4*>(w + ((size_t)(32 * mt + m) * KTAPS + t) * cin + 16 * s + 8 * h);
    } else {
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = w[((size_t)(16 * s + 8 * h + j) * KTAPS + t) * cin + 32 * mt + m];
        wp[i] = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16));
    }
}

// ---- forward and data gradient: one implicit GEMM ------------------------------------------------------------------------------------
struct IgArgs {
    const uint16_t* src;    // forward: X (N, Hp, Wp, 16 KS); data gradient: dZ (N, Ho, Wo, 16 KS)
    const uint4* wp;        // k_conv_pack's chunks
    uint16_t* dst;          // forward: Z (N, Ho, Wo, 32 MT); data gradient: dX (N, Hp, Wp, 32 MT)
    int64_t N;
    int Ho, Wo, Hp, Wp;
};

template <bool BF, int MT, int KS, bool DGRAD>
__global__ __launch_bounds__(64 * IG_WAVES) void k_conv_ig(IgArgs a) {
    constexpr int SLAB = MT * KS * 64;              // 16-byte chunks of one tap
    constexpr int NT = 64 * IG_WAVES;
    constexpr int GL = (SLAB + NT - 1) / NT;
    constexpr int CS = 16 * KS, CD = 32 * MT;       // channels of a source / destination pixel
    __shared__ uint4 wl[2][SLAB];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Ho = a.Ho, Wo = a.Wo;
    // the pixels of this launch row: the output pixels (forward) or the pixels (2 ar + py, 2 ac + px) of one parity class of dX
    const int py = DGRAD ? (int)(blockIdx.y >> 1) : 0, px = DGRAD ? (int)(blockIdx.y & 1) : 0;
    const int RA = DGRAD ? Ho + 1 - py : Ho, CA = DGRAD ? Wo + 1 - px : Wo;
    const int nkx = DGRAD ? (px ? 1 : 2) : 3;
    const int nt = DGRAD ? (py ? 1 : 2) * nkx : KTAPS;
    const int64_t P = a.N * RA * CA;
    const int64_t q0 = (int64_t)blockIdx.x * (32 * IG_WAVES);
    if (q0 >= P) return;                            // the whole workgroup: before any barrier
    const int64_t q = q0 + wave * 32 + n;
    const bool live = q < P;
    const int64_t qc = live ? q : P - 1;
    const int64_t smp = qc / ((int64_t)RA * CA);
    const int rem = (int)(qc - smp * RA * CA);
    const int ar = rem / CA, ac = rem - ar * CA;

    auto tap_of = [&](int ti, int& ky, int& kx) {
        const int iy = ti / nkx, ix = ti - iy * nkx;
        ky = DGRAD ? (py ? 1 : 2 * iy) : iy;
        kx = DGRAD ? (px ? 1 : 2 * ix) : ix;
    };
    // the lane's B fragments of tap ti: k-step s = source channels 16 s + 8 h ..+ 7 of one pixel, 16 contiguous bytes
    auto frags = [&](int ti, uint4 (&v)[KS]) {
        int ky, kx;
        tap_of(ti, ky, kx);
        int64_t pix;
        bool ok = true;
        if (DGRAD) {
            const int oy = ar - (ky >> 1), ox = ac - (kx >> 1);
            ok = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
            pix = ok ? (smp * Ho + oy) * Wo + ox : 0;
        } else {
            pix = (smp * a.Hp + 2 * ar + ky) * a.Wp + 2 * ac + kx;
        }
        const uint4* p = reinterpret_cast<const uint4*>(a.src + pix * CS) + h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            uint4 u = p[2 * s];
            if (DGRAD && !ok) u = make_uint4(0, 0, 0, 0);
            v[s] = u;
        }
    };
    auto slab_of = [&](int ti) -> const uint4* {
        int ky, kx;
        tap_of(ti, ky, kx);
        return a.wp + (size_t)(ky * 3 + kx) * SLAB;
    };

    {
        const uint4* w0 = slab_of(0);
#pragma unroll
        for (int i = 0; i < GL; ++i)
            if (tid + i * NT < SLAB) wl[0][tid + i * NT] = w0[tid + i * NT];
    }
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    uint4 cur[KS], nxt[KS];
    frags(0, cur);
    for (int ti = 0; ti < nt; ++ti) {
        // the next tap's slab and fragments: in flight under this tap's MFMAs
        const bool more = ti + 1 < nt;
        uint4 g[GL];
        if (more) {
            const uint4* wn = slab_of(ti + 1);
#pragma unroll
            for (int i = 0; i < GL; ++i)
                if (tid + i * NT < SLAB) g[i] = wn[tid + i * NT];
            frags(ti + 1, nxt);
        }
        // this tap's stage (written during the previous tap) is complete and visible; the other one (read then) is free
        lds_barrier();
        const int stage = ti & 1;
        const uint4* st = wl[stage] + lane;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16<BF>(st[(s * MT + mt) * 64], cur[s], acc[mt]);
        if (more) {
#pragma unroll
            for (int i = 0; i < GL; ++i)
                if (tid + i * NT < SLAB) wl[stage ^ 1][tid + i * NT] = g[i];
#pragma unroll
            for (int s = 0; s < KS; ++s) cur[s] = nxt[s];
        }
    }
    // accumulator registers 4 j .. 4 j + 3 of tile mt are channels 32 mt + 8 j + 4 h ..: 8-byte stores
    const int64_t dpix = DGRAD ? (smp * a.Hp + 2 * ar + py) * a.Wp + 2 * ac + px : qc;
    uint16_t* dst = a.dst + dpix * CD + 4 * h;
    if (live) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<uint2*>(dst + mt * 32 + 8 * j) =
                    make_uint2(pk2<BF>(acc[mt][4 * j], acc[mt][4 * j + 1]), pk2<BF>(acc[mt][4 * j + 2], acc[mt][4 * j + 3]));
    }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------------------
struct WgPlan {
    int64_t pieces, len;    // pieces of `len` pixels (a multiple of CHP; the last one may be shorter), none empty
};
// a function of the pixel count alone (nn_common.conv3s2_wgrad_plan mirrors it for the error bound of the tests)
WgPlan wgrad_plan(int64_t P) {
    int64_t np = (P + PIECE_MIN - 1) / PIECE_MIN;
    np = np < 1 ? 1 : (np > MAX_PIECES ? MAX_PIECES : np);
    int64_t len = (P + np - 1) / np;
    len = (len + CHP - 1) / CHP * CHP;
    if (len < CHP) len = CHP;
    return WgPlan{P > 0 ? (P + len - 1) / len : 1, len};
}

// one operand of v_mfma_f32_32x32x16 out of a [pixel][channel] LDS image with rows of RB bytes: the lane's row of the M / N index is
// channel c0 + (lane & 31), its eight k are pixels r0 + 8 (lane >> 5) ..+ 7.  Per 16-lane group one transposed read takes 4 pixel rows x
// 16 channels: lane 4 q + p of the group addresses row q, channels 4 p ..+ 3, and receives its own channel of the four rows.
__device__ __forceinline__ uint4 tr_operand(const unsigned char* img, int RB, int r0, int c0, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const unsigned char* p = img + (size_t)(r0 + 8 * (g >> 1) + (i >> 2)) * RB + (c0 + 16 * (g & 1) + 4 * (i & 3)) * 2;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * RB));
    uint4 out;
    __builtin_memcpy(&out.x, &lo, 8);
    __builtin_memcpy(&out.z, &hi, 8);
    return out;
}

// grid (pieces, 9 taps), 4 waves: wave = (input-channel tile ct, k phase kp); a wave holds the COUT / 32 accumulator tiles of its ct and
// takes the k-steps kp, kp + KH, .. of every staged tile.  part [pieces * KH][cout][9][cin] float32.
template <bool BF, int CIN, int COUT>
__global__ __launch_bounds__(256) void k_conv_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dz, float* __restrict__ part,
                                                    int64_t P, int Ho, int Wo, int Hp, int Wp, int64_t len) {
    constexpr int CT = CIN / 32, KH = 4 / CT, MT = COUT / 32;
    constexpr int RBX = CIN * 2 + 64, RBZ = COUT * 2 + 64;
    constexpr int XCH = CIN / 8, ZCH = COUT / 8;    // 16-byte chunks per pixel
    __shared__ __attribute__((aligned(16))) unsigned char lds[CHP * (RBX + RBZ)];
    unsigned char* const xi = lds;
    unsigned char* const zi = lds + CHP * RBX;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = wave % CT, kp = wave / CT;
    const int tap = blockIdx.y, ky = tap / 3, kx = tap - ky * 3;
    const int64_t p0 = (int64_t)blockIdx.x * len;
    const int64_t p1 = p0 + len < P ? p0 + len : P;
    const int HW = Ho * Wo;
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    for (int64_t c0 = p0; c0 < p1; c0 += CHP) {
        __syncthreads();                            // the previous tile has been read
        // pixels past the end of the piece are zero rows of both images (they add exact zeros)
#pragma unroll
        for (int i = tid; i < CHP * XCH; i += 256) {
            const int pl = i / XCH, ch = i - pl * XCH;
            const int64_t p = c0 + pl;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (p < p1) {
                const int64_t smp = p / HW;
                const int rem = (int)(p - smp * HW);
                const int oy = rem / Wo, ox = rem - oy * Wo;
                v = reinterpret_cast<const uint4*>(x + ((smp * Hp + 2 * oy + ky) * Wp + 2 * ox + kx) * CIN)[ch];
            }
            *reinterpret_cast<uint4*>(xi + pl * RBX + ch * 16) = v;
        }
#pragma unroll
        for (int i = tid; i < CHP * ZCH; i += 256) {
            const int pl = i / ZCH, ch = i - pl * ZCH;
            const int64_t p = c0 + pl;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (p < p1) v = reinterpret_cast<const uint4*>(dz + p * COUT)[ch];
            *reinterpret_cast<uint4*>(zi + pl * RBZ + ch * 16) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = kp; ks < CHP / 16; ks += KH) {
            const uint4 b = tr_operand(xi, RBX, 16 * ks, 32 * ct, lane);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16<BF>(tr_operand(zi, RBZ, 16 * ks, 32 * mt, lane), b, acc[mt]);
        }
    }
    // register r of tile mt: output channel 32 mt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), input channel 32 ct + (lane & 31)
    float* dst = part + (((size_t)blockIdx.x * KH + kp) * COUT * KTAPS + tap) * CIN + 32 * ct + (lane & 31);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            dst[(size_t)co * KTAPS * CIN] = acc[mt][r];
        }
}

// dW[i] = the pieces' partials added in index order, rounded once; four elements per thread
template <bool BF>
__global__ __launch_bounds__(256) void k_conv_wreduce(const float* __restrict__ part, uint16_t* __restrict__ dw, int count, int pieces) {
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;
    float4 s = *reinterpret_cast<const float4*>(part + i);
    for (int p = 1; p < pieces; ++p) {
        const float4 v = *reinterpret_cast<const float4*>(part + (size_t)p * count + i);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<uint2*>(dw + i) = make_uint2(pk2<BF>(s.x, s.y), pk2<BF>(s.z, s.w));
}

bool pair_ok(int cin, int cout) { return (cin == 128 && cout == 64) || (cin == 64 && cout == 32); }

int check_common(const char* who, rml_ctx* ctx, int dtype, int64_t n, int hp, int wp, int cin, int cout) {
    RML_REQUIRE(ctx && n >= 0, RML_ERR_INVALID, "%s: bad arguments", who);
    RML_REQUIRE(dtype == 0 || dtype == 1, RML_ERR_INVALID, "%s: dtype %d (0: float16, 1: bfloat16)", who, dtype);
    RML_REQUIRE(rml_conv3s2_supported(cin, cout, hp, wp), RML_ERR_UNSUPPORTED,
                "%s: %d -> %d channels on a %dx%d padded plane: 128 -> 64 or 64 -> 32 channels, odd edges in [3, %d]", who, cin, cout, hp,
                wp, MAX_EDGE);
    RML_REQUIRE(n * (int64_t)hp * wp < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "%s: batch too large", who);
    return RML_OK;
}

template <bool DGRAD>
void launch_ig(bool bf, int cin, int cout, const IgArgs& a, hipStream_t st) {
    const int64_t P = DGRAD ? a.N * (a.Ho + 1) * (a.Wo + 1) : a.N * a.Ho * a.Wo;
    const dim3 grid((unsigned)((P + 32 * IG_WAVES - 1) / (32 * IG_WAVES)), DGRAD ? 4 : 1), block(64 * IG_WAVES);
    constexpr bool D = DGRAD;
    const bool big = cin == 128;
    // forward: M tiles = cout / 32, k-steps = cin / 16; data gradient: M tiles = cin / 32, k-steps = cout / 16
    if (bf) {
        if (big) hipLaunchKernelGGL((k_conv_ig<true, D ? 4 : 2, D ? 4 : 8, D>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_conv_ig<true, D ? 2 : 1, D ? 2 : 4, D>), grid, block, 0, st, a);
    } else {
        if (big) hipLaunchKernelGGL((k_conv_ig<false, D ? 4 : 2, D ? 4 : 8, D>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_conv_ig<false, D ? 2 : 1, D ? 2 : 4, D>), grid, block, 0, st, a);
    }
}

template <bool DGRAD>
int run_ig(const char* who, rml_ctx* ctx, const void* src, const void* w, int dtype, int64_t n, int hp, int wp, int cin, int cout,
           void* dst, void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = check_common(who, ctx, dtype, n, hp, wp, cin, cout);
    if (rc != RML_OK) return rc;
    if (n == 0) return RML_OK;
    RML_REQUIRE(src && w && dst && workspace, RML_ERR_INVALID, "%s: NULL argument", who);
    const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dst) |
                         reinterpret_cast<uintptr_t>(workspace);
    RML_REQUIRE((al & 15) == 0, RML_ERR_INVALID, "%s: tensors and workspace must be 16-byte aligned", who);
    RML_REQUIRE(workspace_bytes >= (int64_t)KTAPS * cin * cout * 2, RML_ERR_INVALID, "%s: workspace too small", who);
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int chunks = KTAPS * cin * cout / 8;
    hipLaunchKernelGGL(k_conv_pack<DGRAD>, dim3((chunks + 255) / 256), dim3(256), 0, st, static_cast<const uint16_t*>(w),
                       static_cast<uint4*>(workspace), cin, cout);
    IgArgs a{};
    a.src = static_cast<const uint16_t*>(src); a.wp = static_cast<const uint4*>(workspace); a.dst = static_cast<uint16_t*>(dst);
    a.N = n; a.Hp = hp; a.Wp = wp; a.Ho = (hp - 1) / 2; a.Wo = (wp - 1) / 2;
    launch_ig<DGRAD>(dtype == 1, cin, cout, a, st);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

}  // namespace

extern "C" int rml_conv3s2_supported(int cin, int cout, int hp, int wp) {
    return pair_ok(cin, cout) && hp >= 3 && wp >= 3 && (hp & 1) && (wp & 1) && hp <= MAX_EDGE && wp <= MAX_EDGE;
}

extern "C" int64_t rml_conv3s2_workspace_bytes(rml_ctx* ctx, int64_t n, int hp, int wp, int cin, int cout, int pass) {
    (void)ctx;
    if (n < 0 || !rml_conv3s2_supported(cin, cout, hp, wp)) return 0;
    if (pass == RML_CONV3S2_FORWARD || pass == RML_CONV3S2_DGRAD) return (int64_t)KTAPS * cin * cout * 2;
    if (pass != RML_CONV3S2_WGRAD) return 0;
    const WgPlan pl = wgrad_plan(n * ((hp - 1) / 2) * ((wp - 1) / 2));
    return pl.pieces * (4 / (cin / 32)) * (int64_t)KTAPS * cin * cout * 4;
}

extern "C" int rml_conv3s2_forward(rml_ctx* ctx, const void* x, const void* w, int dtype, int64_t n, int hp, int wp, int cin, int cout,
                                   void* z, void* workspace, int64_t workspace_bytes, void* stream) {
    return run_ig<false>("rml_conv3s2_forward", ctx, x, w, dtype, n, hp, wp, cin, cout, z, workspace, workspace_bytes, stream);
}

extern "C" int rml_conv3s2_dgrad(rml_ctx* ctx, const void* dz, const void* w, int dtype, int64_t n, int hp, int wp, int cin, int cout,
                                 void* dx, void* workspace, int64_t workspace_bytes, void* stream) {
    return run_ig<true>("rml_conv3s2_dgrad", ctx, dz, w, dtype, n, hp, wp, cin, cout, dx, workspace, workspace_bytes, stream);
}

extern "C" int rml_conv3s2_wgrad(rml_ctx* ctx, const void* x, const void* dz, int dtype, int64_t n, int hp, int wp, int cin, int cout,
                                 void* dw, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "rml_conv3s2_wgrad";
    const int rc = check_common(who, ctx, dtype, n, hp, wp, cin, cout);
    if (rc != RML_OK) return rc;
    RML_REQUIRE(n > 0, RML_ERR_INVALID, "%s: an empty batch has no weight gradient", who);
    RML_REQUIRE(x && dz && dw && workspace, RML_ERR_INVALID, "%s: NULL argument", who);
    const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(dw) |
                         reinterpret_cast<uintptr_t>(workspace);
    RML_REQUIRE((al & 15) == 0, RML_ERR_INVALID, "%s: tensors and workspace must be 16-byte aligned", who);
    RML_REQUIRE(workspace_bytes >= rml_conv3s2_workspace_bytes(ctx, n, hp, wp, cin, cout, RML_CONV3S2_WGRAD), RML_ERR_INVALID,
                "%s: workspace too small", who);
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Ho = (hp - 1) / 2, Wo = (wp - 1) / 2;
    const int64_t P = n * Ho * Wo;
    const WgPlan pl = wgrad_plan(P);
    const dim3 grid((unsigned)pl.pieces, KTAPS), block(256);
    const uint16_t* xs = static_cast<const uint16_t*>(x);
    const uint16_t* zs = static_cast<const uint16_t*>(dz);
    float* part = static_cast<float*>(workspace);
    const bool bf = dtype == 1;
    if (cin == 128) {
        if (bf) hipLaunchKernelGGL((k_conv_wgrad<true, 128, 64>), grid, block, 0, st, xs, zs, part, P, Ho, Wo, hp, wp, pl.len);
        else hipLaunchKernelGGL((k_conv_wgrad<false, 128, 64>), grid, block, 0, st, xs, zs, part, P, Ho, Wo, hp, wp, pl.len);
    } else {
        if (bf) hipLaunchKernelGGL((k_conv_wgrad<true, 64, 32>), grid, block, 0, st, xs, zs, part, P, Ho, Wo, hp, wp, pl.len);
        else hipLaunchKernelGGL((k_conv_wgrad<false, 64, 32>), grid, block, 0, st, xs, zs, part, P, Ho, Wo, hp, wp, pl.len);
    }
    const int count = KTAPS * cin * cout;
    const int pieces = (int)(pl.pieces * (4 / (cin / 32)));
    if (bf) hipLaunchKernelGGL(k_conv_wreduce<true>, dim3((count / 4 + 255) / 256), dim3(256), 0, st, part, static_cast<uint16_t*>(dw), count, pieces);
    else hipLaunchKernelGGL(k_conv_wreduce<false>, dim3((count / 4 + 255) / 256), dim3(256), 0, st, part, static_cast<uint16_t*>(dw), count, pieces);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
