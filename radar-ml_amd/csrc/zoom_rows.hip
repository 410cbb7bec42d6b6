// Projection rows of a foreign radar arena zoomed to the model's geometry: the batched sibling of k_zoom (zoom.hip).
//
// The reference classifies a recording whose arena differs from the training arena by spline-zooming every projection to the
// training geometry (predict.py:109-116 -> common.process_samples, common.py:141-148).  k_zoom does that for planes a caller brings
// from the host, one workgroup per (sample, plane).  k_zoom_rows takes the rows the projection kernels write at the SOURCE grid
// (planes concatenated xz|yz|xy; float32, or the uint8 codes of project_u8.hip / the code stage -- uint8 volumes are on the code grid
// by construction) and writes the rows a float-row consumer of svm.hip reads: the model-geometry float row at the model's stride,
// pad columns zeroed, the float64 squared norm of the row and its row flag.
//
// The coefficient image of a plane sits in LDS as float64 at an ODD pitch in doubles (k_zoom walks the axis-1 lines at a pitch of W
// doubles: with W = 160 or 176 every active lane hits the same LDS bank).  Three ways to share a row, measured in DESIGN.md 3.7b:
// one workgroup per (row, plane) -- the default: the most resident waves --, or one workgroup per row with the images of its planes
// together (the lines of all planes filtered side by side: 348 axis-0 and 68 axis-1 lines at 20 x 28 x 160) or one after the other.
// The arithmetic is k_zoom's, operation for operation (prefilter axis 0 then axis 1, 4 x 4 taps, float32 cast, optional
// __fdiv_rn): the rows are the same bits.  The squared norm is summed in the order of k_prepare_rows (svm_rows.h) -- thread t owns
// the columns t, t + 256, ... ascending -- so the SVM behind it computes what rml_svm_decision computes on the same rows.
#include "rml_internal.h"
#include "spline_dev.h"
#include <math.h>
#include <algorithm>

namespace {

using namespace rml_spline;

struct ZoomRowsPlane {
    int H, W, OH, OW, pitch;    // source plane, output plane, pitch of the coefficient image in doubles (odd)
    int in_off, out_off;        // offset of the plane inside the source row / the output row
    int lds_off;                // offset of its coefficient image in LDS (doubles)
};
struct ZoomRowsArgs {
    ZoomRowsPlane pl[3];
    int npl, by_plane;
    const float* src_f; const uint8_t* src_q; int64_t ld_src;   // one of the two: float rows, or biased code rows (value ^ 0x80)
    float* feat; int64_t ld_feat, D, pad_to;
    float scale_div;
    double* row_nsq; int32_t* row_flags;
};

// mirror_idx for the taps of a coordinate inside the plane: i in [-1, n + 1], where no remainder is needed once n > 3 (the same integer)
__device__ __forceinline__ int mirror_near(int i, int n) {
    if (n <= 3) return mirror_idx(i, n);
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// the float64 squared norm of every row in the sum order of k_prepare_rows, and its row flag (0: off the code grid), for rows whose
// planes were written by workgroups of their own
__global__ __launch_bounds__(256) void k_zoom_rows_norms(const float* feat, int64_t ld, int64_t D, double* nsq, int32_t* flags) {
    __shared__ double redn[4];
    const float* __restrict__ src = feat + (int64_t)blockIdx.x * ld;
    double nn = 0.0;
    for (int64_t base = threadIdx.x; base < D; base += 256 * 8) {
        float vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int64_t idx = base + (int64_t)u * 256; vv[u] = idx < D ? src[idx] : 0.0f; }
#pragma unroll
        for (int u = 0; u < 8; ++u) nn += (double)vv[u] * (double)vv[u];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nn += __shfl_xor(nn, off);
    if ((threadIdx.x & 63) == 0) redn[threadIdx.x >> 6] = nn;
    __syncthreads();
    if (threadIdx.x == 0) {
        double NN = 0;
        for (int w = 0; w < 4; ++w) NN += redn[w];
        if (nsq) nsq[blockIdx.x] = NN;
        if (flags) flags[blockIdx.x] = 0;
    }
}

// prefilter_line of spline_dev.h with its floating-point contraction written out.  The source leaves the fusing of multiplies and adds
// to the compiler, and inside k_zoom the compiler settles it per loop: every multiply-add of the causal pass is one fma, and the
// anti-causal recurrence c[i] = z (c[i+1] - c[i]) is left as it is along axis 1, while along axis 0 -- unrolled by eight, the steps
// that are not a multiple of eight first -- a step inside a group takes the previous step's difference d unrounded, fma(d, z, -c[i]),
// where the first step of a group reads z d back rounded.  A line that is filtered here with the lanes of other planes beside it is
// compiled differently, and the rows would differ from k_zoom's in the last place of coefficients that cancel to zero.  So the
// arithmetic of k_zoom is pinned (contraction off, fma where k_zoom has one): tests/test_foreign_arena_gpu.py holds the two kernels to
// the same bits, and fails when a compiler changes k_zoom's.
template <bool AXIS0>
__device__ inline void prefilter_line_pinned(double* c, int n, int stride) {
#pragma clang fp contract(off)
    if (n < 2) return;
    const double z = -0.26794919243112270647;     // sqrt(3) - 2
    const double lam = (1.0 - z) * (1.0 - 1.0 / z);
    for (int i = 0; i < n; ++i) c[i * stride] = c[i * stride] * lam;
    const double zn1 = pow(z, (double)(n - 1));
    double c0 = fma(zn1, c[(n - 1) * stride], c[0]);
    double zi = z, z2 = zn1 * zn1 / z;
    // (the start-up sum: unrolled by four in k_zoom, whole groups first; after the first step of a group the weight z^i + z2 takes
    // the product z^(i-1) z unrounded, while z^i itself stays the chain of rounded products)
    int i1 = 1;
    for (int g = (n - 2) >> 2; g > 0; --g) {
        c0 = fma(zi + z2, c[i1 * stride], c0);
        ++i1;
        for (int u = 1; u < 4; ++u, ++i1) {
            z2 = z2 / z;
            c0 = fma(fma(z, zi, z2), c[i1 * stride], c0);
            zi = zi * z;
        }
        z2 = z2 / z; zi = zi * z;
    }
    for (; i1 < n - 1; ++i1) {
        c0 = fma(zi + z2, c[i1 * stride], c0);
        zi = zi * z; z2 = z2 / z;
    }
    c[0] = c0 / fma(-zn1, zn1, 1.0);
    for (int i = 1; i < n; ++i) c[i * stride] = fma(z, c[(i - 1) * stride], c[i * stride]);
    c[(n - 1) * stride] = fma(z, c[(n - 2) * stride], c[(n - 1) * stride]) * z / (z * z - 1.0);
    if (!AXIS0) {
        for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
        return;
    }
    int i = n - 2;
    for (int r = (n - 1) & 7; r > 0; --r, --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
    while (i >= 0) {
        double d = c[(i + 1) * stride] - c[i * stride];
        c[i * stride] = d * z;
        --i;
        for (int u = 1; u < 8; ++u, --i) {
            d = fma(d, z, -c[i * stride]);
            c[i * stride] = d * z;
        }
    }
}

__global__ __launch_bounds__(256) void k_zoom_rows(ZoomRowsArgs a) {
    extern __shared__ __align__(16) double coef[];
    __shared__ double redn[4];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    float* dst = a.feat + b * a.ld_feat;
    double nn = 0.0;
    // by_plane 0: the planes of the row together; 1: one after the other in one image; 2: this workgroup owns plane blockIdx.y
    const bool split = a.by_plane == 2;
    const int gbeg = split ? (int)blockIdx.y : 0, gend = split ? (int)blockIdx.y + 1 : a.npl;
    const int step = a.by_plane ? 1 : a.npl;
    for (int g0 = gbeg; g0 < gend; g0 += step) {
        const int g1 = g0 + step;
        for (int p = g0; p < g1; ++p) {
            const ZoomRowsPlane P = a.pl[p];
            double* c = coef + P.lds_off;
            if (a.src_q) {
                const uint8_t* s = a.src_q + b * a.ld_src + P.in_off;
                for (int i = tid; i < P.H * P.W; i += 256) { const int h = i / P.W; c[h * P.pitch + (i - h * P.W)] = (double)(s[i] ^ 0x80); }
            } else {
                const float* s = a.src_f + b * a.ld_src + P.in_off;
                for (int i = tid; i < P.H * P.W; i += 256) { const int h = i / P.W; c[h * P.pitch + (i - h * P.W)] = (double)s[i]; }
            }
        }
        __syncthreads();
        int lines = 0;
        for (int p = g0; p < g1; ++p) lines += a.pl[p].W;
        for (int L = tid; L < lines; L += 256) {                    // axis 0: one line per column of every plane
            int l = L, p = g0;
            while (l >= a.pl[p].W) { l -= a.pl[p].W; ++p; }
            prefilter_line_pinned<true>(coef + a.pl[p].lds_off + l, a.pl[p].H, a.pl[p].pitch);
        }
        __syncthreads();
        lines = 0;
        for (int p = g0; p < g1; ++p) lines += a.pl[p].H;
        for (int L = tid; L < lines; L += 256) {                    // axis 1: one line per row of every plane
            int l = L, p = g0;
            while (l >= a.pl[p].H) { l -= a.pl[p].H; ++p; }
            prefilter_line_pinned<false>(coef + a.pl[p].lds_off + (int64_t)l * a.pl[p].pitch, a.pl[p].W, 1);
        }
        __syncthreads();
        // resample the columns [lo, hi) of the output row; thread t takes the columns congruent to t modulo 256
        const int lo = a.pl[g0].out_off, hi = a.pl[g1 - 1].out_off + a.pl[g1 - 1].OH * a.pl[g1 - 1].OW;
        for (int idx = lo + ((tid - lo) & 255); idx < hi; idx += 256) {
            int p = g0;
            while (idx >= a.pl[p].out_off + a.pl[p].OH * a.pl[p].OW) ++p;
            const ZoomRowsPlane P = a.pl[p];
            const double* cf = coef + P.lds_off;
            const int H = P.H, W = P.W;
            const double z0 = P.OH > 1 ? (double)(H - 1) / (double)(P.OH - 1) : 1.0;
            const double z1 = P.OW > 1 ? (double)(W - 1) / (double)(P.OW - 1) : 1.0;
            const int o = idx - P.out_off;
            const int o0 = o / P.OW, o1 = o - o0 * P.OW;
            const double c0 = o0 * z0, c1 = o1 * z1;
            float r = 0.0f;                                    // cval for out-of-range coordinates (mode 'constant')
            if (c0 >= 0.0 && c0 <= (double)(H - 1) && c1 >= 0.0 && c1 <= (double)(W - 1)) {
                const int f0 = (int)floor(c0), f1 = (int)floor(c1);
                double w0[4], w1[4];
                bspline3(c0 - f0, w0);
                bspline3(c1 - f1, w1);
                double s = 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double* row = cf + (int64_t)mirror_near(f0 - 1 + u, H) * P.pitch;
                    double t = 0.0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) t += w1[q] * row[mirror_near(f1 - 1 + q, W)];
                    s += w0[u] * t;
                }
                r = (float)s;
            }
            const float v = a.scale_div > 1.0f ? __fdiv_rn(r, a.scale_div) : r;
            dst[idx] = v;
            nn += (double)v * (double)v;
        }
        __syncthreads();                                            // the next plane takes the image over
    }
    if (split && blockIdx.y != 0) return;
    for (int64_t c = a.D + tid; c < a.pad_to; c += 256) dst[c] = 0.0f;
    if (!a.row_nsq && !a.row_flags) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nn += __shfl_xor(nn, off);
    if ((tid & 63) == 0) redn[tid >> 6] = nn;
    __syncthreads();
    if (tid == 0) {
        double NN = 0;
        for (int w = 0; w < 4; ++w) NN += redn[w];
        if (a.row_nsq) a.row_nsq[b] = NN;
        if (a.row_flags) a.row_flags[b] = 0;                        // off the code grid: k_prepare_rows without code rows
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// pitch of a plane's coefficient image in doubles: odd, unless that alone would push a plane of rml_zoom_features' domain out of LDS
constexpr size_t kZoomRowsLds = 160 * 1024 - 64;
inline int zoom_pitch(int H, int W) { return (size_t)H * (W | 1) * sizeof(double) <= kZoomRowsLds ? (W | 1) : W; }

// the scratch of one chunk: source rows, (code rows: their statistics, as the projection kernels write them), derived (i,j,k), sum planes
struct StageWs { void* rows; int32_t* isum; int64_t* isq; int32_t* flags; int32_t* ijk; float* sums; size_t bytes; };
StageWs stage_carve(const rml_zoom_plan& zp, int64_t frames, unsigned char* base) {
    StageWs w{}; size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align256(bytes); return base && bytes ? base + o : (unsigned char*)nullptr; };
    const bool u8 = zp.codes;
    const size_t rows = (size_t)frames * zp.T;
    w.rows = take(rows * zp.ld_src * (u8 ? 1 : 4));
    w.isum = (int32_t*)take(u8 ? rows * 4 : 0); w.isq = (int64_t*)take(u8 ? rows * 8 : 0); w.flags = (int32_t*)take(u8 ? rows * 4 : 0);
    w.ijk = (int32_t*)take(zp.derive ? rows * 12 : 0);
    w.sums = (float*)take(zp.derive ? (size_t)frames * ((size_t)zp.X * zp.Z + (size_t)zp.Y * zp.Z) * 4 : 0);
    w.bytes = off;
    return w;
}

}  // namespace

int rml_zoom_plan_make(const rml_ctx* ctx, const char* who, int vdtype, int mode, int X, int Y, int Z, int T, bool derive, const int32_t* out_shape,
                       uint32_t mask, rml_zoom_plan* zp) {
    RML_REQUIRE(out_shape && X > 0 && Y > 0 && Z > 0 && T >= 1, RML_ERR_INVALID, "%s: bad arguments", who);
    RML_REQUIRE(vdtype == RML_VOL_F32 || vdtype == RML_VOL_U8, RML_ERR_INVALID, "%s: unknown volume dtype %d", who, vdtype);
    RML_REQUIRE((mask & RML_MASK_ALL) != 0, RML_ERR_INVALID, "%s: empty projection mask", who);
    *zp = rml_zoom_plan{};
    zp->vdtype = vdtype; zp->X = X; zp->Y = Y; zp->Z = Z; zp->T = T; zp->mask = mask & RML_MASK_ALL; zp->derive = derive;
    zp->codes = vdtype == RML_VOL_U8 && mode != RML_MODE_SUM;     // (a sum leaves the code range)
    const int inH[3] = {X, Y, X}, inW[3] = {Z, Z, Y};
    size_t together = 0, largest = 0;
    for (int pl = 0; pl < 3; ++pl) {
        zp->out_shape[2 * pl] = out_shape[2 * pl]; zp->out_shape[2 * pl + 1] = out_shape[2 * pl + 1];
        if (!(mask & (1u << pl))) continue;
        const int OH = out_shape[2 * pl], OW = out_shape[2 * pl + 1];
        RML_REQUIRE(OH > 0 && OW > 0, RML_ERR_INVALID, "%s: empty output plane %d", who, pl);
        zp->Dsrc += (int64_t)inH[pl] * inW[pl];
        zp->Dout += (int64_t)OH * OW;
        // the domain of rml_zoom_features: the plane's float64 image (at its own width) within 150 KB
        RML_REQUIRE((size_t)inH[pl] * inW[pl] * sizeof(double) <= 150 * 1024, RML_ERR_UNSUPPORTED,
                    "%s: plane too large for the LDS-resident spline filter", who);
        const size_t image = (size_t)inH[pl] * zoom_pitch(inH[pl], inW[pl]) * sizeof(double);
        together += image; largest = std::max(largest, image);
    }
    RML_REQUIRE(zp->Dout < (int64_t)1 << 30 && zp->Dsrc < (int64_t)1 << 30, RML_ERR_UNSUPPORTED, "%s: row too long", who);
    zp->ld_src = zp->codes ? (zp->Dsrc + 127) / 128 * 128 : zp->Dsrc;
    // two workgroups per CU while the images of a row fit 80 KB; a row that fits a CU alone may still be forced together
    const int knob = ctx ? ctx->opt.zoom_rows : 0;
    // one workgroup per (row, plane) unless told otherwise: measured, DESIGN.md 3.8 (1: the planes of a row together in one
    // workgroup, where they fit a CU; 2: one workgroup per row, one plane after the other)
    zp->by_plane = (knob == 1 && together <= 150 * 1024) ? 0 : (knob == 2 ? 1 : 2);
    zp->lds = zp->by_plane == 0 ? together : largest;
    return RML_OK;
}

size_t rml_zoom_stage_bytes(const rml_zoom_plan& zp, int64_t frames) { return stage_carve(zp, frames, nullptr).bytes; }

int rml_zoom_stage_run(rml_ctx* ctx, const rml_zoom_plan& zp, void* scratch, const void* V, int64_t frames, int mode, const int32_t* ijk,
                       float scale_div, float* feat, int64_t ld_feat, int64_t pad_to, double* row_nsq, int32_t* row_flags, hipStream_t st) {
    if (frames <= 0) return RML_OK;
    const StageWs w = stage_carve(zp, frames, static_cast<unsigned char*>(scratch));
    const bool u8 = zp.codes;
    const int64_t rows = frames * zp.T;
    const int X = zp.X, Y = zp.Y, Z = zp.Z;
    if (zp.derive) {
        if (int rc = rml_launch_derive(ctx, V, zp.vdtype, frames, X, Y, Z, zp.T, w.ijk, w.sums, st)) return rc;
        ijk = w.ijk;
    }
    // the rows at the source grid, unscaled: float rows as rml_project writes them, or its code rows + statistics
    const int inH[3] = {X, Y, X}, inW[3] = {Z, Z, Y};
    ProjOut o{};
    int64_t off = 0;
    for (int pl = 0; pl < 3; ++pl) {
        if (!(zp.mask & (1u << pl))) continue;
        if (u8) o.q[pl] = static_cast<uint8_t*>(w.rows) + off;
        else { o.p[pl] = static_cast<float*>(w.rows) + off; o.stride[pl] = zp.ld_src; }
        off += (int64_t)inH[pl] * inW[pl];
    }
    o.sel = zp.mask;
    if (u8) { o.qstride = zp.ld_src; o.qrow = static_cast<uint8_t*>(w.rows); o.qD = zp.Dsrc; o.row_isum = w.isum; o.row_isq = w.isq; o.row_flags = w.flags; }
    if (int rc = rml_launch_project(ctx, V, zp.vdtype, rows, X, Y, Z, mode, ijk, o, st, zp.T)) return rc;

    ZoomRowsArgs a{};
    int in_off = 0, out_off = 0, lds_off = 0;
    for (int pl = 0; pl < 3; ++pl) {
        if (!(zp.mask & (1u << pl))) continue;
        const int pitch = zoom_pitch(inH[pl], inW[pl]);
        a.pl[a.npl++] = ZoomRowsPlane{inH[pl], inW[pl], zp.out_shape[2 * pl], zp.out_shape[2 * pl + 1], pitch, in_off, out_off,
                                     zp.by_plane ? 0 : lds_off};      // (an image of its own starts at 0)
        in_off += inH[pl] * inW[pl]; out_off += zp.out_shape[2 * pl] * zp.out_shape[2 * pl + 1]; lds_off += inH[pl] * pitch;
    }
    a.by_plane = zp.by_plane;
    a.src_f = u8 ? nullptr : static_cast<const float*>(w.rows); a.src_q = u8 ? static_cast<const uint8_t*>(w.rows) : nullptr;
    a.ld_src = zp.ld_src;
    a.feat = feat; a.ld_feat = ld_feat; a.D = zp.Dout; a.pad_to = std::max(pad_to, zp.Dout); a.scale_div = scale_div;
    const bool split = zp.by_plane == 2;
    a.row_nsq = split ? nullptr : row_nsq; a.row_flags = split ? nullptr : row_flags;
    RML_MAX_DYN_LDS((int)kZoomRowsLds, &k_zoom_rows);
    hipLaunchKernelGGL(k_zoom_rows, dim3((unsigned)rows, split ? (unsigned)a.npl : 1u), dim3(256), zp.lds, st, a);
    if (split && (row_nsq || row_flags))
        hipLaunchKernelGGL(k_zoom_rows_norms, dim3((unsigned)rows), dim3(256), 0, st, feat, ld_feat, zp.Dout, row_nsq, row_flags);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

// predict.py:98-116 for B frames: the projections of predict.py:102-107 (or mode MAX) at the recording's own grid, then
// common.process_samples with calc_proj_zoom's factors (predict.py:34-54,109-116; common.py:141-148) -- the rows alone
extern "C" int rml_project_zoom(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode, const int32_t* ijk, int T,
                                const int32_t* out_shape, float scale_div, uint32_t mask, float* feat, int64_t ld_feat, void* stream) {
    RML_REQUIRE(ctx && B >= 0, RML_ERR_INVALID, "rml_project_zoom: bad arguments");
    if (mode == RML_MODE_MAX_NAN) mode = RML_MODE_MAX;
    RML_REQUIRE(mode == RML_MODE_MAX || mode == RML_MODE_SLICE || mode == RML_MODE_SUM, RML_ERR_INVALID, "rml_project_zoom: unknown mode %d", mode);
    RML_REQUIRE(T == 1 || (mode == RML_MODE_SLICE && T > 1), RML_ERR_INVALID, "rml_project_zoom: several targets per frame only in mode SLICE");
    const bool derive = mode == RML_MODE_SLICE && !ijk;
    RML_REQUIRE(!derive || (T <= X && T <= Y && T <= Z), RML_ERR_INVALID, "rml_project_zoom: num_targets out of range");
    rml_zoom_plan zp;
    if (int rc = rml_zoom_plan_make(ctx, "rml_project_zoom", vdtype, mode, X, Y, Z, T, derive, out_shape, mask, &zp)) return rc;
    if (B == 0) return RML_OK;
    RML_REQUIRE(V && feat, RML_ERR_INVALID, "rml_project_zoom: NULL argument");
    RML_REQUIRE(ld_feat >= zp.Dout, RML_ERR_INVALID, "rml_project_zoom: ld_feat < D");
    RML_REQUIRE(B * (int64_t)T < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "rml_project_zoom: too many rows");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);           // shared workspace
    // the source-grid rows live for a chunk: 8 192 rows (RML_OPT_CHUNK overrides), whole frames
    const int64_t ch_rows = ctx->opt.chunk >= 128 ? (ctx->opt.chunk + 127) / 128 * 128 : 8192;
    const int64_t CH = std::min<int64_t>(B, std::max<int64_t>(1, ch_rows / T));
    void* ws = nullptr;
    if (int rc = rml_ws_reserve(ctx, rml_zoom_stage_bytes(zp, CH), &ws, st)) return rc;
    const int64_t frame_bytes = (int64_t)X * Y * Z * (vdtype == RML_VOL_U8 ? 1 : 4);
    for (int64_t f0 = 0; f0 < B; f0 += CH) {
        const int64_t n = std::min(CH, B - f0);
        if (int rc = rml_zoom_stage_run(ctx, zp, ws, static_cast<const unsigned char*>(V) + f0 * frame_bytes, n, mode,
                                        ijk ? ijk + f0 * T * 3 : nullptr, scale_div, feat + f0 * T * ld_feat, ld_feat, zp.Dout, nullptr, nullptr, st))
            return rc;
    }
    return RML_OK;
}
