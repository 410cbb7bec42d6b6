// What the two fused CNN preprocessing kernels share: k_pre3 (preprocess.hip: feature / code rows in) and k_pre3s
// (preprocess_slice.hip: the three planes through a target's voxel, gathered straight from the volumes).  The plan of a (grid, output
// size) pair and its device tables (host side, defined in preprocess.hip), the LDS layout, and the horizontal and vertical passes:
// the two kernels differ in how a row's image gets into LDS and in nothing behind that, so their planes agree bit for bit on equal
// images.  The passes themselves are described at the top of preprocess.hip.
#pragma once
#include "rml_internal.h"
#include <vector>

namespace rmlpre {

constexpr int PU = 5;       // 16-element units of a row a thread holds (rows up to 20 480 elements)
constexpr int VT = 4;       // taps of the vertical pass (Pillow's bicubic window when the height does not shrink)

struct PreArgs {
    const float* rows; int64_t ld;          // float32 feature rows (k_pre3<false>)
    const uint8_t* codes; int64_t ldq;      // biased uint8 code rows, byte = code ^ 0x80 (k_pre3<true>)
    const int32_t* flags;                   // per row: != 0 -> the code row is valid (nullptr: every row)
    const int32_t* skip_if_set;             // k_pre3<false>: the whole launch is a no-op when *skip_if_set != 0
    int64_t B;
    int X, Y, Z, OH, OW;
    int SZ, TW;                             // LDS row strides in elements: [xz | yz] image, intermediate
    const int* hz_a0; const float* hz_w;    // Z -> OW: aligned window start per output column, [OW][WZ] weights
    const int* hy_a0; const float* hy_w;    // Y -> OW: window start, [OW][WY] weights (unshifted)
    const float* vw; const int* vfirst;     // [2][OH][VT] weights, [2][OH] first rows: table 0 = X -> OH (xz, xy), 1 = Y -> OH (yz)
    uint16_t* out[3];                       // bf16 (B, OH, OW) per projection
};

// ---- host side (preprocess.hip) ----
struct Plan {
    bool ok = false;
    int wz = 0, wy = 0, TW = 0;
    int SZ[2] = {0, 0};         // image row stride: float32 images, float16 images
    size_t lds[2] = {0, 0};
    std::vector<int> hz_a0, hy_a0, vfirst;
    std::vector<float> hz_w, hy_w, vw;
};
// the plan of a (grid, output size) pair is a pure function of the five numbers: built once per process, not once per call
// (four Pillow coefficient tables and their window tables: ~10^4 double operations at the Walabot grid)
Plan make_plan(int X, int Y, int Z, int OH, int OW);
// device copy of a plan's tables, cached in the context per (X, Y, Z, OH, OW): fills the table pointers of `a`
int pre_tables(rml_ctx* ctx, int X, int Y, int Z, int OH, int OW, const Plan& p, PreArgs& a);

// ---- device side ----
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {     // v_cvt_pk_bf16_f32 (round to nearest even)
    bf16x2 b = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
    return *reinterpret_cast<uint32_t*>(&b);
}
// LDS-only barrier: __syncthreads() would also wait for the prefetch of the next sample (vmcnt)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the reference's (p - 127.5) / 127.5 (dnn.py:202-205), applied to the horizontal pass's result: the weights of a window sum to 1
__device__ __forceinline__ float unit_range(float p) { return fmaf(p, 1.0f / 127.5f, -1.0f); }

// four consecutive image values (8- / 16-byte aligned) as floats
__device__ __forceinline__ float4 quad(const _Float16* s) {
    const f16x4 v = *reinterpret_cast<const f16x4*>(s);
    return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}
__device__ __forceinline__ float4 quad(const float* s) { return *reinterpret_cast<const float4*>(s); }

template <int WIN, typename T>
__device__ __forceinline__ float window_dot(const T* s, const float (&w)[WIN]) {
    float ax = 0.0f, ay = 0.0f, az = 0.0f, aw = 0.0f;
#pragma unroll
    for (int q = 0; q < WIN / 4; ++q) {
        const float4 v = quad(s + 4 * q);
        ax = fmaf(v.x, w[4 * q], ax);
        ay = fmaf(v.y, w[4 * q + 1], ay);
        az = fmaf(v.z, w[4 * q + 2], az);
        aw = fmaf(v.w, w[4 * q + 3], aw);
    }
    return (ax + ay) + (az + aw);
}
// the same on an unaligned window, element by element (the small xy image, kept linear)
template <int WIN, typename T>
__device__ __forceinline__ float window_dot1(const T* s, const float (&w)[WIN]) {
    float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
    for (int t = 0; t + 1 < WIN; t += 2) {
        a0 = fmaf((float)s[t], w[t], a0);
        a1 = fmaf((float)s[t + 1], w[t + 1], a1);
    }
    if (WIN & 1) a0 = fmaf((float)s[WIN - 1], w[WIN - 1], a0);
    return a0 + a1;
}

// The dynamic LDS of a workgroup: the intermediate, the vertical tables, then the images of one sample in element type T
// (_Float16: raw codes 0..255, exact; float: anything else).
template <typename T>
struct PreLds {
    float* tmp;         // [R1 + X + 3][TW]: xz, yz, xy rows after the horizontal pass, 3 pad rows
    float* vw_s;        // [2][OH][VT]
    int* vf_s;          // [2][OH]
    T* inA;             // [R1][SZ] + 16: xz rows, then yz rows
    T* inB;             // [XY] linear + pad
};

// carves the LDS and initialises it.  Every pad (row tails, the elements behind each image, the pad rows of the intermediate) is read
// under a zero weight and must be finite: zeroed once, never written again.  The caller synchronises before the first pass.
template <typename T>
__device__ __forceinline__ PreLds<T> pre_lds_init(unsigned char* smem, const PreArgs& a, int tid) {
    const int X = a.X, Y = a.Y, OH = a.OH, SZ = a.SZ, TW = a.TW;
    const int R1 = X + Y, XY = X * Y;
    const int nimg = R1 * SZ + 16 + ((XY + 15) & ~15) + 32;     // image elements: [R1][SZ] + 16 pad, then xy linear + pad
    PreLds<T> l;
    l.tmp = reinterpret_cast<float*>(smem);
    l.vw_s = l.tmp + (R1 + X + 3) * TW;
    l.vf_s = reinterpret_cast<int*>(l.vw_s + 2 * OH * VT);
    l.inA = reinterpret_cast<T*>(l.vf_s + ((2 * OH + 3) & ~3));
    l.inB = l.inA + R1 * SZ + 16;
    for (int i = tid; i < (R1 + X + 3) * TW; i += 256) l.tmp[i] = 0.0f;
    for (int i = tid; i < nimg; i += 256) l.inA[i] = (T)0.0f;
    for (int i = tid; i < 2 * OH * VT; i += 256) l.vw_s[i] = a.vw[i];
    for (int i = tid; i < 2 * OH; i += 256) l.vf_s[i] = a.vfirst[i];
    return l;
}

// horizontal pass: thread (hg, hx) owns output column hx, its window weights in registers for the whole launch
template <int WZ, int WY>
struct PreWin {
    float wz[WZ], wy[WY];
    int az, ay;         // window starts in a [xz | yz] row (aligned) and in an xy row
    int G, hg, hx;      // G = 256 / OW row groups
    bool hact;
};

template <int WZ, int WY>
__device__ __forceinline__ void pre_win_load(PreWin<WZ, WY>& h, const PreArgs& a, int tid) {
    h.G = 256 / a.OW;
    h.hg = tid / a.OW; h.hx = tid - h.hg * a.OW;
    h.hact = h.hg < h.G;
    h.az = 0; h.ay = 0;
#pragma unroll
    for (int t = 0; t < WZ; ++t) h.wz[t] = 0.0f;
#pragma unroll
    for (int t = 0; t < WY; ++t) h.wy[t] = 0.0f;
    if (h.hact) {
        h.az = a.hz_a0[h.hx]; h.ay = a.hy_a0[h.hx];
#pragma unroll
        for (int t = 0; t < WZ; ++t) h.wz[t] = a.hz_w[h.hx * WZ + t];
#pragma unroll
        for (int t = 0; t < WY; ++t) h.wy[t] = a.hy_w[h.hx * WY + t];
    }
}

// rows of [xz | yz] (length Z) and of xy (length Y) -> column hx of the intermediate, scaled to [-1, 1]
template <typename T, int WZ, int WY>
__device__ __forceinline__ void pre_horizontal(const PreLds<T>& l, const PreWin<WZ, WY>& h, const PreArgs& a) {
    if (!h.hact) return;
    const int X = a.X, Y = a.Y, SZ = a.SZ, TW = a.TW, R1 = X + Y, G = h.G, az = h.az, ay = h.ay;
    float* tc = l.tmp + h.hx;
    int y = h.hg;
    for (; y + G < R1; y += 2 * G) {        // two rows at a time: independent chains
        const float r0 = window_dot<WZ, T>(l.inA + y * SZ + az, h.wz);
        const float r1 = window_dot<WZ, T>(l.inA + (y + G) * SZ + az, h.wz);
        tc[y * TW] = unit_range(r0);
        tc[(y + G) * TW] = unit_range(r1);
    }
    if (y < R1) tc[y * TW] = unit_range(window_dot<WZ, T>(l.inA + y * SZ + az, h.wz));
    tc += R1 * TW;
    for (y = h.hg; y < X; y += G) tc[y * TW] = unit_range(window_dot1<WY, T>(l.inB + y * Y + ay, h.wy));
}

// vertical pass of the three projections of output row b: a thread produces four adjacent outputs of a row from four ds_read_b128
// and stores them as one 8-byte piece -- consecutive threads write consecutive bytes
template <typename T>
__device__ __forceinline__ void pre_vertical(const PreLds<T>& l, const PreArgs& a, int64_t b, int tid) {
    const int X = a.X, OH = a.OH, TW = a.TW, R1 = a.X + a.Y;
    const int OW4 = a.OW >> 2;
    const int per = OH * OW4;                       // 8-byte output pieces per projection
    const int vdq = 256 / OW4, vdr = 256 - vdq * OW4;
    const int64_t opl = (int64_t)OH * a.OW;
#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
        const float* tp = l.tmp + (p == 0 ? 0 : (p == 1 ? X : R1)) * TW;
        const float* wv = l.vw_s + (p == 1 ? OH * VT : 0);
        const int* fv = l.vf_s + (p == 1 ? OH : 0);
        uint2* o8 = reinterpret_cast<uint2*>(a.out[p] + b * opl);
        int yy = tid / OW4, c4 = tid - yy * OW4;
        for (int r = tid; r < per; r += 256) {
            const float4 w = *reinterpret_cast<const float4*>(wv + yy * VT);
            const float* s = tp + fv[yy] * TW + 4 * c4;
            const float4 v0 = *reinterpret_cast<const float4*>(s);
            const float4 v1 = *reinterpret_cast<const float4*>(s + TW);
            const float4 v2 = *reinterpret_cast<const float4*>(s + 2 * TW);
            const float4 v3 = *reinterpret_cast<const float4*>(s + 3 * TW);
            // two outputs per instruction (v_pk_mul_f32 / v_pk_fma_f32): the pairs (x, y) and (z, w) of the four outputs
            const f32x2 w0 = {w.x, w.x}, w1 = {w.y, w.y}, w2 = {w.z, w.z}, w3 = {w.w, w.w};
            f32x2 lo = f32x2{v0.x, v0.y} * w0, hi = f32x2{v0.z, v0.w} * w0;
            lo = __builtin_elementwise_fma(f32x2{v1.x, v1.y}, w1, lo); hi = __builtin_elementwise_fma(f32x2{v1.z, v1.w}, w1, hi);
            lo = __builtin_elementwise_fma(f32x2{v2.x, v2.y}, w2, lo); hi = __builtin_elementwise_fma(f32x2{v2.z, v2.w}, w2, hi);
            lo = __builtin_elementwise_fma(f32x2{v3.x, v3.y}, w3, lo); hi = __builtin_elementwise_fma(f32x2{v3.z, v3.w}, w3, hi);
            o8[r] = make_uint2(pk_bf16(lo.x, lo.y), pk_bf16(hi.x, hi.y));
            yy += vdq; c4 += vdr;
            if (c4 >= OW4) { c4 -= OW4; ++yy; }
        }
    }
}

// the 16 raw codes of one staging unit as float16 image values (exact: integers 0..255)
__device__ __forceinline__ void stage_codes16(_Float16* dst, uint4 w4) {
    const uint32_t ws[4] = {w4.x, w4.y, w4.z, w4.w};
    f16x8* d = reinterpret_cast<f16x8*>(dst);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t w0 = ws[2 * h], w1 = ws[2 * h + 1];
        f16x8 v;
        v[0] = (_Float16)(float)(w0 & 0xFFu); v[1] = (_Float16)(float)((w0 >> 8) & 0xFFu);
        v[2] = (_Float16)(float)((w0 >> 16) & 0xFFu); v[3] = (_Float16)(float)(w0 >> 24);
        v[4] = (_Float16)(float)(w1 & 0xFFu); v[5] = (_Float16)(float)((w1 >> 8) & 0xFFu);
        v[6] = (_Float16)(float)((w1 >> 16) & 0xFFu); v[7] = (_Float16)(float)(w1 >> 24);
        d[h] = v;
    }
}

}  // namespace rmlpre
