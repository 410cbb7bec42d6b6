// Training-mode Conv2DTranspose(128 -> 128, 4x4, stride 2, 'same') of the SGAN generator (sgan.py:65-87) for gfx950: the forward pass
// and the two gradients autograd needs, on the matrix cores, without a convolution library.  The generator-side counterpart of
// conv_train.hip, with the same contract.
//
//   X (N, H, W, 128);  Z and dZ (N, 2H, 2W, 128);  W [ci][ky][kx][co] -- the channels_last storage of torch's (ci, co, 4, 4)
//   ConvTranspose2d weight --, tap = ky * 4 + kx;  dW like W.  float16 or bfloat16 operands (template BF), float32 accumulation on
//   v_mfma_f32_32x32x16_{f16,bf16}, every result rounded to the half type once.  No bias (the batch norm behind it cancels it).
//   oy = 2 iy + ky - 1, ox = 2 ix + kx - 1; what falls outside a plane is zero.
//
//  * forward  Z[n,oy,ox,co] = sum X[n,iy,ix,ci] W[ci,ky,kx,co]: output pixel (2a + p, 2b + q) meets 2 x 2 taps, ky = 1 + 2i at row
//    a - i (p = 0) or ky = 2 - 2i at row a + i (p = 1), i = 0, 1, and the same along x.  The four (p, q) classes are four implicit
//    GEMMs of one kernel (blockIdx.y; the phase GEMMs of k_gen_up with the unfolded weight), K = 4 * 128.
//  * data gradient  dX[n,iy,ix,ci] = sum dZ[n,2iy+ky-1,2ix+kx-1,co] W[ci,ky,kx,co]: a 4x4 stride-2 pad-1 convolution of dZ, the same
//    kernel with 16 taps, K = 16 * 128.
//    Both are shaped like k_conv_ig: M = 128 destination channels (A = the weights, packed into operand order in the workspace once
//    per call), N = 32 pixels per wave, a lane's pixel fragment is 16 contiguous bytes of one source pixel; one tap's weights
//    (128 x 128 halves, 32 KB) are a slab in LDS, two stages, the eight waves of a workgroup in step over the taps with one LDS-only
//    barrier each.  Pixel tiles run over the flattened (n, a, b) index.  A tap outside the source plane is a zero fragment.
//  * weight gradient  dW[ci,ky,kx,co] = sum over pixels of X[n,iy,ix,ci] dZ[n,2iy+ky-1,2ix+kx-1,co]: 64-pixel tiles of X and, per
//    tap, of the dZ pixels facing them (zero rows where they fall outside) are staged in LDS as they lie in memory and read
//    transposed with ds_read_b64_tr_b16 (k_conv_wgrad's tr_operand: EXEC all ones, 8-byte lane addresses, rows padded by 64 bytes).
//    A workgroup owns (piece of the pixel range, ky): the four taps kx of that row share one X image, so X is fetched four times
//    and not sixteen.  Its 64 accumulator tiles (4 taps x 4 ci tiles x 4 co tiles) are 8 per wave over 8 waves: wave = (kx, half of
//    the ci tiles).  The next tile's global loads are in flight under the MFMAs of the current one.  The pieces follow from the pixel
//    count alone (wgrad_plan: never from the CU count), float32 partials go to the workspace (1 MB per piece), and k_convt_wreduce
//    adds them in index order and rounds once.
//
// Properties: no atomics, no zeroed workspace (every workspace element that is read was written earlier in the same call); every
// output has ONE summation order, and it depends on the shapes alone; a sample's Z and dX are the same bits alone and at any position
// of any batch (taps in index order, channels in 16-wide steps, whatever tile the pixel falls in); all passes launch on the caller's
// stream, allocate nothing and never synchronise.
#include "rml_internal.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int C = 128;                      // channels, in and out
constexpr int KTAPS = 16;
constexpr int MT = C / 32, KS = C / 16;     // M tiles and k-steps of one tap
constexpr int SLAB = MT * KS * 64;          // 16-byte chunks of one tap's packed weights
constexpr int IG_WAVES = 8;                 // waves (32-pixel tiles) per workgroup of k_convt_ig
constexpr int CHP = 64;                     // pixels per staged tile of k_convt_wgrad: four MFMA k-steps
constexpr int PIECE_MIN = 128;              // wgrad_plan: no more pieces than pixels / PIECE_MIN ...
constexpr int MAX_PIECES = 64;              // ... and at most this many: 64 MB of partials
constexpr int MIN_EDGE = 8, MAX_EDGE = 128; // H, W: multiples of 8

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
// W [ci][tap][co] -> chunks of 16 bytes [tap][k-step s][M tile mt][lane l = (m, h)].  Forward: M = output channels, k = input channels:
// element i of the chunk = W[16 s + 8 h + i][tap][32 mt + m].  Data gradient: M = input channels, k = output channels: chunk =
// W[32 mt + m][tap][16 s + 8 h ..+ 7], contiguous.
template <bool DGRAD>
__global__ __launch_bounds__(256) void k_convt_pack(const uint16_t* __restrict__ w, uint4* __restrict__ wp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= KTAPS * SLAB) return;
    const int l = i & 63, m = l & 31, h = l >> 5;
    int r = i >> 6;
    const int mt = r % MT;
    r /= MT;
    const int s = r % KS, t = r / KS;
    if (DGRAD) {
        wp[i] = *reinterpret_cast<const uint4*>(w + ((size_t)(32 * mt + m) * KTAPS + t) * C + 16 * s + 8 * h);
    } else {
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = w[((size_t)(16 * s + 8 * h + j) * KTAPS + t) * C + 32 * mt + m];
        wp[i] = make_uint4(e[0] | ((uint32_t)e[1] << 16), e[2] | ((uint32_t)e[3] << 16), e[4] | ((uint32_t)e[5] << 16), e[6] | ((uint32_t)e[7] << 16));
    }
}

// ---- forward and data gradient: one implicit GEMM ------------------------------------------------------------------------------------
struct IgArgs {
    const uint16_t* src;    // forward: X (N, H, W, C); data gradient: dZ (N, 2H, 2W, C)
    const uint4* wp;        // k_convt_pack's chunks
    uint16_t* dst;          // forward: Z (N, 2H, 2W, C); data gradient: dX (N, H, W, C)
    int64_t N;
    int H, W;               // the small plane (X, dX)
};

template <bool BF, bool DGRAD>
__global__ __launch_bounds__(64 * IG_WAVES) void k_convt_ig(IgArgs a) {
    constexpr int NT = 64 * IG_WAVES;
    static_assert(SLAB == 4 * NT, "the slab is copied in four rounds");
    __shared__ uint4 wl[2][SLAB];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = a.H, W = a.W;
    // a workgroup's pixels: (n, a, b) of the small plane; forward writes (2a + p, 2b + q) of the class (p, q) = blockIdx.y
    const int p = DGRAD ? 0 : (int)(blockIdx.y >> 1), q = DGRAD ? 0 : (int)(blockIdx.y & 1);
    constexpr int nt = DGRAD ? KTAPS : 4;
    const int64_t P = a.N * H * W;
    const int64_t q0 = (int64_t)blockIdx.x * (32 * IG_WAVES);
    if (q0 >= P) return;                            // the whole workgroup: before any barrier
    const int64_t pq = q0 + wave * 32 + n;
    const bool live = pq < P;
    const int64_t qc = live ? pq : P - 1;
    const int64_t smp = qc / ((int64_t)H * W);
    const int rem = (int)(qc - smp * H * W);
    const int ar = rem / W, ac = rem - ar * W;

    // tap ti of this launch row: the kernel tap (ky, kx) and the source pixel it reads for destination (ar, ac)
    auto tap_of = [&](int ti, int& ky, int& kx, int& sy, int& sx) {
        if (DGRAD) {
            ky = ti >> 2; kx = ti & 3;
            sy = 2 * ar + ky - 1; sx = 2 * ac + kx - 1;
        } else {
            const int iy = ti >> 1, ix = ti & 1;
            ky = p ? 2 - 2 * iy : 1 + 2 * iy; kx = q ? 2 - 2 * ix : 1 + 2 * ix;
            sy = p ? ar + iy : ar - iy; sx = q ? ac + ix : ac - ix;
        }
    };
    // the lane's B fragments of tap ti: k-step s = source channels 16 s + 8 h ..+ 7 of one pixel, 16 contiguous bytes
    auto frags = [&](int ti, uint4 (&v)[KS]) {
        int ky, kx, sy, sx;
        tap_of(ti, ky, kx, sy, sx);
        const int SH = DGRAD ? 2 * H : H, SW = DGRAD ? 2 * W : W;
        const bool ok = sy >= 0 && sy < SH && sx >= 0 && sx < SW;
        const int64_t pix = ok ? (smp * SH + sy) * SW + sx : 0;
        const uint4* src = reinterpret_cast<const uint4*>(a.src + pix * C) + h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            uint4 u = src[2 * s];
            if (!ok) u = make_uint4(0, 0, 0, 0);
            v[s] = u;
        }
    };
    auto slab_of = [&](int ti) -> const uint4* {
        int ky, kx, sy, sx;
        tap_of(ti, ky, kx, sy, sx);
        return a.wp + (size_t)(ky * 4 + kx) * SLAB;
    };

    {
        const uint4* w0 = slab_of(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) wl[0][tid + i * NT] = w0[tid + i * NT];
    }
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    uint4 cur[KS], nxt[KS];
    frags(0, cur);
#pragma unroll                                      // nt is a constant: `more` and the stage are known per copy, g[] stays in registers
    for (int ti = 0; ti < nt; ++ti) {
        // the next tap's slab and fragments: in flight under this tap's MFMAs
        const bool more = ti + 1 < nt;
        uint4 g0, g1, g2, g3;                       // named, not an array: the compiler keeps an array across the barrier in scratch
        if (more) {
            const uint4* wn = slab_of(ti + 1) + tid;
            g0 = wn[0]; g1 = wn[NT]; g2 = wn[2 * NT]; g3 = wn[3 * NT];
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
            uint4* wo = wl[stage ^ 1] + tid;
            wo[0] = g0; wo[NT] = g1; wo[2 * NT] = g2; wo[3 * NT] = g3;
#pragma unroll
            for (int s = 0; s < KS; ++s) cur[s] = nxt[s];
        }
    }
    // accumulator registers 4 j .. 4 j + 3 of tile mt are channels 32 mt + 8 j + 4 h ..: 8-byte stores
    const int64_t dpix = DGRAD ? qc : (smp * 2 * H + 2 * ar + p) * (2 * W) + 2 * ac + q;
    uint16_t* dst = a.dst + dpix * C + 4 * h;
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
// a function of the pixel count alone (nn_common.convt4s2_wgrad_plan mirrors it for the error bound of the tests)
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

// grid (pieces, 4 kernel rows ky), 8 waves: wave = (kx, half ch of the input-channel tiles); a wave holds the 2 x 4 accumulator tiles
// (ci tiles 2 ch, 2 ch + 1) x (co tiles 0..3) of tap (ky, kx) and takes every k-step of every staged tile.
// part [pieces][ci][16][co] float32.
constexpr int RB = C * 2 + 64;              // bytes of an LDS row: one pixel's 128 halves + the padding of k_conv_wgrad
constexpr int PCH = C / 8;                  // 16-byte chunks per pixel
constexpr int WG_NT = 512;
constexpr int XL = CHP * PCH / WG_NT;       // chunks per thread of the X image (2) ...
constexpr int ZL = 4 * XL;                  // ... and of the four dZ images (8)

template <bool BF>
__global__ __launch_bounds__(WG_NT) void k_convt_wgrad(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dz, float* __restrict__ part,
                                                      int64_t P, int H, int W, int64_t len) {
    static_assert(CHP * PCH % WG_NT == 0, "the images are copied in whole rounds");
    __shared__ __attribute__((aligned(16))) unsigned char lds[5 * CHP * RB];
    unsigned char* const xi = lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kx = wave >> 1, ch = wave & 1;
    unsigned char* const zi = lds + (size_t)(1 + kx) * CHP * RB;
    const int ky = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * len;
    const int64_t p1 = p0 + len < P ? p0 + len : P;
    const int HW = H * W;
    f32x16 acc[2][MT];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][mt][r] = 0.f;

    // chunk i = tid + j * WG_NT of an image: pixel i / PCH of the tile, 16-byte chunk i % PCH.  Pixels past the end of the piece and dZ
    // pixels outside the plane are zero rows (they add exact zeros).
    uint4 gx[XL], gz[ZL];
    auto fetch = [&](int64_t c0) {
#pragma unroll
        for (int j = 0; j < XL; ++j) {
            const int i = tid + j * WG_NT, pl = i / PCH, cc = i - pl * PCH;
            const int64_t px = c0 + pl;
            const bool in = px < p1;
            const int64_t pc = in ? px : p1 - 1;
            const int64_t smp = pc / HW;
            const int rem = (int)(pc - smp * HW);
            const int iy = rem / W, ix = rem - iy * W;
            uint4 v = reinterpret_cast<const uint4*>(x + pc * C)[cc];
            if (!in) v = make_uint4(0, 0, 0, 0);
            gx[j] = v;
            const int oy = 2 * iy + ky - 1;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ox = 2 * ix + t - 1;
                const bool ok = in && oy >= 0 && oy < 2 * H && ox >= 0 && ox < 2 * W;
                const int64_t zp = ok ? (smp * 2 * H + oy) * (2 * W) + ox : 0;
                uint4 u = reinterpret_cast<const uint4*>(dz + zp * C)[cc];
                if (!ok) u = make_uint4(0, 0, 0, 0);
                gz[j * 4 + t] = u;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < XL; ++j) {
            const int i = tid + j * WG_NT, pl = i / PCH, cc = i - pl * PCH;
            *reinterpret_cast<uint4*>(xi + pl * RB + cc * 16) = gx[j];
#pragma unroll
            for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4*>(lds + (size_t)(1 + t) * CHP * RB + pl * RB + cc * 16) = gz[j * 4 + t];
        }
    };

    fetch(p0);
    for (int64_t c0 = p0; c0 < p1; c0 += CHP) {
        __syncthreads();                            // the previous tile has been read
        stage();
        __syncthreads();
        if (c0 + CHP < p1) fetch(c0 + CHP);         // in flight under this tile's MFMAs
#pragma unroll
        for (int ks = 0; ks < CHP / 16; ++ks) {
            uint4 b[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) b[mt] = tr_operand(zi, RB, 16 * ks, 32 * mt, lane);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const uint4 av = tr_operand(xi, RB, 16 * ks, 32 * (2 * ch + ct), lane);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[ct][mt] = mfma16<BF>(av, b[mt], acc[ct][mt]);
            }
        }
    }
    // register r of tile (ct, mt): input channel 32 (2 ch + ct) + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), output channel 32 mt + (lane & 31)
    float* dst = part + ((size_t)blockIdx.x * C * KTAPS + (ky * 4 + kx)) * C + (lane & 31);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = 32 * (2 * ch + ct) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                dst[(size_t)ci * KTAPS * C + 32 * mt] = acc[ct][mt][r];
            }
}

// dW[i] = the pieces' partials added in index order, rounded once; four elements per thread
template <bool BF>
__global__ __launch_bounds__(256) void k_convt_wreduce(const float* __restrict__ part, uint16_t* __restrict__ dw, int count, int pieces) {
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;
    float4 s = *reinterpret_cast<const float4*>(part + i);
    for (int p = 1; p < pieces; ++p) {
        const float4 v = *reinterpret_cast<const float4*>(part + (size_t)p * count + i);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<uint2*>(dw + i) = make_uint2(pk2<BF>(s.x, s.y), pk2<BF>(s.z, s.w));
}

constexpr int64_t PACK_BYTES = (int64_t)KTAPS * C * C * 2;
constexpr int64_t PIECE_BYTES = (int64_t)KTAPS * C * C * 4;

int check_common(const char* who, rml_ctx* ctx, int dtype, int64_t n, int h, int w, int cin, int cout) {
    RML_REQUIRE(ctx && n >= 0, RML_ERR_INVALID, "%s: bad arguments", who);
    RML_REQUIRE(dtype == 0 || dtype == 1, RML_ERR_INVALID, "%s: dtype %d (0: float16, 1: bfloat16)", who, dtype);
    RML_REQUIRE(rml_convt4s2_supported(cin, cout, h, w), RML_ERR_UNSUPPORTED,
                "%s: %d -> %d channels on a %dx%d input plane: 128 -> 128 channels, edges that are multiples of 8 in [%d, %d]", who, cin, cout,
                h, w, MIN_EDGE, MAX_EDGE);
    RML_REQUIRE(n * (int64_t)h * w * 4 < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "%s: batch too large", who);
    return RML_OK;
}

template <bool DGRAD>
int run_ig(const char* who, rml_ctx* ctx, const void* src, const void* w, int dtype, int64_t n, int h, int w_, int cin, int cout, void* dst,
           void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = check_common(who, ctx, dtype, n, h, w_, cin, cout);
    if (rc != RML_OK) return rc;
    if (n == 0) return RML_OK;
    RML_REQUIRE(src && w && dst && workspace, RML_ERR_INVALID, "%s: NULL argument", who);
    const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dst) |
                         reinterpret_cast<uintptr_t>(workspace);
    RML_REQUIRE((al & 15) == 0, RML_ERR_INVALID, "%s: tensors and workspace must be 16-byte aligned", who);
    RML_REQUIRE(workspace_bytes >= PACK_BYTES, RML_ERR_INVALID, "%s: workspace too small", who);
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_convt_pack<DGRAD>, dim3(KTAPS * SLAB / 256), dim3(256), 0, st, static_cast<const uint16_t*>(w),
                       static_cast<uint4*>(workspace));
    IgArgs a{};
    a.src = static_cast<const uint16_t*>(src); a.wp = static_cast<const uint4*>(workspace); a.dst = static_cast<uint16_t*>(dst);
    a.N = n; a.H = h; a.W = w_;
    const int64_t P = n * h * w_;
    const dim3 grid((unsigned)((P + 32 * IG_WAVES - 1) / (32 * IG_WAVES)), DGRAD ? 1 : 4), block(64 * IG_WAVES);
    if (dtype == 1) hipLaunchKernelGGL((k_convt_ig<true, DGRAD>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_convt_ig<false, DGRAD>), grid, block, 0, st, a);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

}  // namespace

extern "C" int rml_convt4s2_supported(int cin, int cout, int h, int w) {
    return cin == C && cout == C && h >= MIN_EDGE && w >= MIN_EDGE && h <= MAX_EDGE && w <= MAX_EDGE && h % 8 == 0 && w % 8 == 0;
}

extern "C" int64_t rml_convt4s2_workspace_bytes(rml_ctx* ctx, int64_t n, int h, int w, int cin, int cout, int pass) {
    (void)ctx;
    if (n < 0 || !rml_convt4s2_supported(cin, cout, h, w)) return 0;
    if (pass == RML_CONVT4S2_FORWARD || pass == RML_CONVT4S2_DGRAD) return PACK_BYTES;
    if (pass != RML_CONVT4S2_WGRAD) return 0;
    return wgrad_plan(n * h * w).pieces * PIECE_BYTES;
}

extern "C" int rml_convt4s2_forward(rml_ctx* ctx, const void* x, const void* w, int dtype, int64_t n, int h, int w_, int cin, int cout,
                                    void* z, void* workspace, int64_t workspace_bytes, void* stream) {
    return run_ig<false>("rml_convt4s2_forward", ctx, x, w, dtype, n, h, w_, cin, cout, z, workspace, workspace_bytes, stream);
}

extern "C" int rml_convt4s2_dgrad(rml_ctx* ctx, const void* dz, const void* w, int dtype, int64_t n, int h, int w_, int cin, int cout,
                                  void* dx, void* workspace, int64_t workspace_bytes, void* stream) {
    return run_ig<true>("rml_convt4s2_dgrad", ctx, dz, w, dtype, n, h, w_, cin, cout, dx, workspace, workspace_bytes, stream);
}

extern "C" int rml_convt4s2_wgrad(rml_ctx* ctx, const void* x, const void* dz, int dtype, int64_t n, int h, int w_, int cin, int cout,
                                  void* dw, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "rml_convt4s2_wgrad";
    const int rc = check_common(who, ctx, dtype, n, h, w_, cin, cout);
    if (rc != RML_OK) return rc;
    RML_REQUIRE(n > 0, RML_ERR_INVALID, "%s: an empty batch has no weight gradient", who);
    RML_REQUIRE(x && dz && dw && workspace, RML_ERR_INVALID, "%s: NULL argument", who);
    const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(dw) |
                         reinterpret_cast<uintptr_t>(workspace);
    RML_REQUIRE((al & 15) == 0, RML_ERR_INVALID, "%s: tensors and workspace must be 16-byte aligned", who);
    const int64_t P = n * h * w_;
    const WgPlan pl = wgrad_plan(P);
    RML_REQUIRE(workspace_bytes >= pl.pieces * PIECE_BYTES, RML_ERR_INVALID, "%s: workspace too small", who);
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)pl.pieces, 4), block(WG_NT);
    const uint16_t* xs = static_cast<const uint16_t*>(x);
    const uint16_t* zs = static_cast<const uint16_t*>(dz);
    float* part = static_cast<float*>(workspace);
    const bool bf = dtype == 1;
    if (bf) hipLaunchKernelGGL(k_convt_wgrad<true>, grid, block, 0, st, xs, zs, part, P, h, w_, pl.len);
    else hipLaunchKernelGGL(k_convt_wgrad<false>, grid, block, 0, st, xs, zs, part, P, h, w_, pl.len);
    const int count = KTAPS * C * C;
    const dim3 rgrid((count / 4 + 255) / 256), rblock(256);
    if (bf) hipLaunchKernelGGL(k_convt_wreduce<true>, rgrid, rblock, 0, st, part, static_cast<uint16_t*>(dw), count, (int)pl.pieces);
    else hipLaunchKernelGGL(k_convt_wreduce<false>, rgrid, rblock, 0, st, part, static_cast<uint16_t*>(dw), count, (int)pl.pieces);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
