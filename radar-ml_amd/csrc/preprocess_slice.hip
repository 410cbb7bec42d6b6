// CNN / SGAN input preprocessing on target slices, straight from the volumes: the reference's samples are the three planes of the radar
// image through one target's voxel -- yz = V[i,:,:], xz = V[:,j,:], xy = V[:,:,k] (predict.py:98-107, ground_truth_samples.py:413-419)
// -- and its live loop classifies every target of every scan that way (predict.py:93-119).  A slice needs (X + Y) * Z + X * Y voxels
// of a frame: k_pre3s gathers them from the volume into the LDS image of k_pre3 (preprocess.hip) and runs k_pre3's passes on it --
// (p - 127.5) / 127.5, Pillow's bicubic windows and weights in float32, bf16 out -- in ONE launch for the B * T targets of a batch:
// no code rows, no row flags, no float rows, no second stream.
//
// Staging type by volume dtype:
//  * uint8 volumes   -> float16 images (a byte is exact in float16; half the LDS bytes, the code-row arithmetic of k_pre3<true>);
//  * float32 volumes -> float32 images (any finite value: no "is the row on the 0..255 grid" test, the arithmetic of k_pre3<false>).
// Float16 -> float32 is exact and the taps are the same fused multiply-adds in the same order, so a float32 volume that holds integers
// 0..255 gives the bits its uint8 copy gives, and both give the bits of rml_dnn_preprocess_rows on the sliced rows.
//
// One 256-thread workgroup per output row r = b * T + t, persistent; the row's planes come from frame r / T:
//  * yz: one contiguous run of Y * Z elements; xz: X runs of Z elements, Y * Z apart -- both as 16-element units (Z % 16 == 0: a unit
//    lies inside one image row), the NEXT row's units loaded into registers while this row is computed;
//  * xy: X * Y single elements, Z apart (element q of the plane is at q * Z + k of the frame): a cache line per element, the first
//    four per thread loaded ahead with the units, the rest (X * Y > 1 024) at staging time.
// Every offset into V is 64-bit.
#include "rml_internal.h"
#include "preprocess_shared.h"
#include <type_traits>

using namespace rmlpre;

namespace {

constexpr int GX = 4;       // xy elements per thread loaded ahead (planes up to 1 024 elements are prefetched whole)

template <typename VOL>
struct SliceArgs {
    PreArgs p;              // geometry, strides, tables, outputs; p.B = B * T rows (rows / codes / flags unused)
    const VOL* V;           // (B, X, Y, Z)
    const int32_t* ijk;     // (B * T, 3)
    int T;
};

template <typename VOL> struct Unit;        // the 16 elements of a staging unit in registers
template <> struct Unit<uint8_t> { uint4 v; };
template <> struct Unit<float> { f32x4u v[4]; };

__device__ __forceinline__ void load_unit(Unit<uint8_t>& u, const uint8_t* s) { u.v = *reinterpret_cast<const uint4*>(s); }
__device__ __forceinline__ void load_unit(Unit<float>& u, const float* s) {
    const f32x4u* p = reinterpret_cast<const f32x4u*>(s);
#pragma unroll
    for (int q = 0; q < 4; ++q) u.v[q] = p[q];
}
__device__ __forceinline__ void store_unit(_Float16* d, const Unit<uint8_t>& u) { stage_codes16(d, u.v); }
__device__ __forceinline__ void store_unit(float* d, const Unit<float>& u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(d + 4 * q) = make_float4(u.v[q].x, u.v[q].y, u.v[q].z, u.v[q].w);
}

template <typename VOL, int WZ, int WY>
__global__ __launch_bounds__(256) void k_pre3s(SliceArgs<VOL> sa) {
    typedef typename std::conditional<std::is_same<VOL, uint8_t>::value, _Float16, float>::type T;
    extern __shared__ __align__(16) unsigned char smem[];
    const PreArgs& a = sa.p;
    const int tid = threadIdx.x;
    const int X = a.X, Y = a.Y, Z = a.Z, SZ = a.SZ;
    const int R1 = X + Y, XY = X * Y;
    const int64_t YZ = (int64_t)Y * Z, XYZ = (int64_t)X * YZ;
    const PreLds<T> l = pre_lds_init<T>(smem, a, tid);
    PreWin<WZ, WY> h;
    pre_win_load(h, a, tid);

    // staging map of this thread (fixed for the launch): unit c covers elements [16 c, 16 c + 16) of the rows [xz | yz], inside
    // one image row.  Its source is at s0 + j * Z (an xz row: frame row x at column j) or s0 + i * Y * Z (a yz row) of the frame.
    const int nA = (R1 * Z) >> 4, nu = (nA + 255) >> 8;
    int dst[PU];
    int64_t s0[PU];
    bool isxz[PU];
#pragma unroll
    for (int u = 0; u < PU; ++u) {
        const int c = u * 256 + tid;
        const int e = 16 * (c < nA ? c : 0);
        const int row = e / Z, col = e - row * Z;
        dst[u] = c < nA ? row * SZ + col : -1;
        isxz[u] = row < X;
        s0[u] = row < X ? row * YZ + col : (int64_t)(row - X) * Z + col;
    }

    Unit<VOL> pa[PU];
    VOL px[GX];
    int kk = 0;                                     // k of the row in flight (the xy elements behind the prefetched ones)
    const VOL* fr = sa.V;                           // its frame
    auto issue = [&](int64_t r) {                   // the units and the first xy elements of row r into registers
        const int32_t* t = sa.ijk + 3 * r;
        int i = t[0], j = t[1], k = t[2];
        i += i < 0 ? X : 0; j += j < 0 ? Y : 0; k += k < 0 ? Z : 0;       // Python's wrap; the range is the caller's
        fr = sa.V + (r / sa.T) * XYZ;
        kk = k;
        const int64_t oj = (int64_t)j * Z, oi = (int64_t)i * YZ;
#pragma unroll
        for (int u = 0; u < PU; ++u)
            if (u < nu && dst[u] >= 0) load_unit(pa[u], fr + (s0[u] + (isxz[u] ? oj : oi)));
#pragma unroll
        for (int g = 0; g < GX; ++g) {
            const int q = g * 256 + tid;
            if (q < XY) px[g] = fr[(int64_t)q * Z + k];
        }
    };
    auto stage = [&]() {                            // ... and from there into the images
#pragma unroll
        for (int u = 0; u < PU; ++u)
            if (u < nu && dst[u] >= 0) store_unit(l.inA + dst[u], pa[u]);
#pragma unroll
        for (int g = 0; g < GX; ++g) {
            const int q = g * 256 + tid;
            if (q < XY) l.inB[q] = (T)(float)px[g];
        }
        for (int q = GX * 256 + tid; q < XY; q += 256) l.inB[q] = (T)(float)fr[(int64_t)q * Z + kk];
    };

    int64_t r = blockIdx.x;
    if (r < a.B) issue(r);
    __syncthreads();                                // LDS initialised (this one may wait for the loads: once)

    for (; r < a.B; r += gridDim.x) {
        stage();
        if (r + gridDim.x < a.B) issue(r + gridDim.x);
        lds_barrier();
        pre_horizontal<T, WZ, WY>(l, h, a);
        lds_barrier();
        pre_vertical<T>(l, a, r, tid);
        lds_barrier();                              // the images and the intermediate are free for the next row
    }
}

template <typename VOL, int WZ, int WY>
void launch_pre3s(const SliceArgs<VOL>& sa, size_t lds, int num_cu, hipStream_t st) {
    RML_MAX_DYN_LDS(160 * 1024, &k_pre3s<VOL, WZ, WY>);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_pre3s<VOL, WZ, WY>, 256, lds) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    const int64_t slots = (int64_t)per_cu * num_cu;
    hipLaunchKernelGGL((k_pre3s<VOL, WZ, WY>), dim3((unsigned)(sa.p.B < slots ? sa.p.B : slots)), dim3(256), lds, st, sa);
}

template <typename VOL>
void launch_pre3s_w(const Plan& p, PreArgs a, const void* V, const int32_t* ijk, int T, int num_cu, hipStream_t st) {
    const int k = std::is_same<VOL, uint8_t>::value ? 1 : 0;         // float16 images for bytes, float32 images for floats
    a.SZ = p.SZ[k];
    SliceArgs<VOL> sa{a, static_cast<const VOL*>(V), ijk, T};
    if (p.wz == 16 && p.wy == 5) launch_pre3s<VOL, 16, 5>(sa, p.lds[k], num_cu, st);
    else if (p.wz == 8 && p.wy == 5) launch_pre3s<VOL, 8, 5>(sa, p.lds[k], num_cu, st);
    else launch_pre3s<VOL, 16, 12>(sa, p.lds[k], num_cu, st);
}

}  // namespace

extern "C" int rml_dnn_preprocess_slices(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, const int32_t* ijk,
                                         int T, int out_h, int out_w, uint16_t* xz, uint16_t* yz, uint16_t* xy, void* stream) {
    RML_REQUIRE(ctx && B >= 0 && T >= 1, RML_ERR_INVALID, "rml_dnn_preprocess_slices: bad arguments");
    const Plan p = make_plan(X, Y, Z, out_h, out_w);
    RML_REQUIRE(p.ok, RML_ERR_UNSUPPORTED, "rml_dnn_preprocess_slices: %dx%dx%d -> %dx%d has no fused kernel (rml_project_slices + rml_resize_bicubic per projection does it)",
                X, Y, Z, out_h, out_w);
    if (B == 0) return RML_OK;
    RML_REQUIRE(B * (int64_t)T < (int64_t)1 << 31 && B < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "rml_dnn_preprocess_slices: B * T too large");
    RML_REQUIRE(V && ijk && xz && yz && xy, RML_ERR_INVALID, "rml_dnn_preprocess_slices: NULL argument");
    RML_REQUIRE(vdtype == RML_VOL_F32 || vdtype == RML_VOL_U8, RML_ERR_INVALID, "rml_dnn_preprocess_slices: unknown volume dtype %d", vdtype);
    RML_REQUIRE((reinterpret_cast<uintptr_t>(V) & (vdtype == RML_VOL_U8 ? 15 : 3)) == 0 && (reinterpret_cast<uintptr_t>(ijk) & 3) == 0, RML_ERR_INVALID,
                "rml_dnn_preprocess_slices: volumes need 16-byte (uint8) / 4-byte (float32) alignment, ijk 4-byte");
    RML_REQUIRE(((reinterpret_cast<uintptr_t>(xz) | reinterpret_cast<uintptr_t>(yz) | reinterpret_cast<uintptr_t>(xy)) & 7) == 0,
                RML_ERR_INVALID, "rml_dnn_preprocess_slices: outputs need 8-byte alignment");
    RML_HIP(hipSetDevice(ctx->device));
    PreArgs a{};
    a.B = B * T;
    a.X = X; a.Y = Y; a.Z = Z; a.OH = out_h; a.OW = out_w; a.TW = p.TW;
    a.out[0] = xz; a.out[1] = yz; a.out[2] = xy;
    int rc = pre_tables(ctx, X, Y, Z, out_h, out_w, p, a);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vdtype == RML_VOL_U8) launch_pre3s_w<uint8_t>(p, a, V, ijk, T, ctx->num_cu, st);
    else launch_pre3s_w<float>(p, a, V, ijk, T, ctx->num_cu, st);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
