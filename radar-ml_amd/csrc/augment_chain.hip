// The augmentation chain of the two network trainers (dnn.py:94-182 augment_data, the same function at sgan.py:238-326) with the
// scaling in front of it (dnn.py:202-205), one launch per batch of equally shaped projection planes:
//
//   scale   v = (p - sub) / div                                   float32, as NumPy computes it            dnn.py:202-205
//   rotate  ndimage.rotate(p, angle, reshape=False), clamp        order-3 spline, mode 'constant', cval 0  dnn.py:101-105
//   zoom    clipped_zoom(p, factor), clamp                        one factor per plane                     dnn.py:107-156
//   noise   p += draw, clamp                                      ONE draw per plane on EVERY entry        dnn.py:158-161
//
// It differs from augment.hip (train.py's DataGenerator) in what the reference differs in: the stages are applied one after the
// other to the same plane instead of each to the original, the clamp is to [lo, hi] = [-1, 1] (so the corners a rotation leaves
// empty become 0, the MIDDLE of the range, as in the reference), and the noise is added to the zeros too.
//
// One workgroup per plane.  The float32 plane between the stages and the float64 coefficient image of the spline prefilter live in
// LDS (12 bytes per pixel: 65 KB for a 31 x 176 plane); the plane is read from memory once and written once.  The kernel is bound
// by the latency of the recursive prefilter lines (one thread per line, a few hundred dependent float64 operations each), not by
// bandwidth or arithmetic: what it buys is ONE launch per plane shape for a whole data set and SciPy's float64 spline arithmetic.
// The random draws stay on the host (radar-ml_amd/dnn.py makes them in the reference's order).
#include "rml_internal.h"
#include "spline_dev.h"
#include <math.h>

namespace {

using namespace rml_spline;

struct ChainArgs {
    const float* src; int64_t in_stride; float* dst;
    int H, W, stages;
    float sub, div, lo, hi;
    const double* par;      // per plane 8: m00 m01 m10 m11 off0 off1 | zoom factor | noise draw
};

constexpr int NT = 256;

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v > hi ? hi : (v < lo ? lo : v); }     // NaN passes, as in the reference

// coef <- float64 B-spline coefficients of the h x w region of `plane` (H x W) at (top, left)
__device__ __forceinline__ void spline_coefficients(const float* plane, int W, int top, int left, int h, int w, double* coef, int tid) {
    for (int i = tid; i < h * w; i += NT) {
        const int r = i / w, c = i - r * w;
        coef[i] = (double)plane[(top + r) * W + left + c];
    }
    __syncthreads();
    for (int c = tid; c < w; c += NT) prefilter_line(coef + c, h, w);               // axis 0
    __syncthreads();
    for (int r = tid; r < h; r += NT) prefilter_line(coef + (int64_t)r * w, w, 1);  // axis 1
    __syncthreads();
}

__global__ __launch_bounds__(NT) void k_augment_chain(ChainArgs a) {
    extern __shared__ __align__(16) double smem[];
    const int H = a.H, W = a.W, n = H * W;
    double* coef = smem;                                        // [H * W], only with a spline stage
    const bool spline = (a.stages & (RML_CHAIN_ROTATE | RML_CHAIN_ZOOM)) != 0;
    float* plane = reinterpret_cast<float*>(smem + (spline ? n : 0));      // [H * W]
    const int64_t b = blockIdx.x;
    const float* src = a.src + b * a.in_stride;
    const double* par = a.par + b * 8;
    const float lo = a.lo, hi = a.hi;
    const int tid = threadIdx.x;
    {
#pragma clang fp contract(off)
        const bool scaled = a.div != 0.0f;
        for (int i = tid; i < n; i += NT) plane[i] = scaled ? __fdiv_rn(src[i] - a.sub, a.div) : src[i];
    }
    __syncthreads();

    if (a.stages & RML_CHAIN_ROTATE) {
        spline_coefficients(plane, W, 0, 0, H, W, coef, tid);
        for (int o = tid; o < n; o += NT) {
            const int o0 = o / W, o1 = o - o0 * W;
            const double c0 = par[0] * o0 + par[1] * o1 + par[4];
            const double c1 = par[2] * o0 + par[3] * o1 + par[5];
            plane[o] = clampf(sample(coef, H, W, c0, c1), lo, hi);
        }
        __syncthreads();
    }

    if (a.stages & RML_CHAIN_ZOOM) {
        const double zf = par[6];
        if (zf == 1.0) {                                    // clipped_zoom returns the input itself (then clamps it)
            for (int i = tid; i < n; i += NT) plane[i] = clampf(plane[i], lo, hi);
        } else if (!(zf >= 1.0 / 1024 && zf <= 1024.0)) {   // not a factor (NaN, <= 0, absurd): no region to resample
            for (int i = tid; i < n; i += NT) plane[i] = clampf(0.0f, lo, hi);
        } else {
            // source region [top, top+h) x [left, left+w) whose spline is sampled; output window
            int top = 0, left = 0, h = H, w = W;
            int zh = H, zw = W, otop = 0, oleft = 0, trim_top = 0, trim_left = 0, OH = H, OW = W;
            if (zf < 1.0) {                                 // the whole plane, zoomed out into the centre of a zero plane
                zh = (int)rint((double)H * zf); zw = (int)rint((double)W * zf);     // int(np.round(h * zoom_factor)): half to even
                otop = (H - zh) / 2; oleft = (W - zw) / 2;
                OH = zh; OW = zw;
            } else {                                        // the centre crop, zoomed in and trimmed to H x W
                h = (int)ceil((double)H / zf); w = (int)ceil((double)W / zf);
                top = (H - h) / 2; left = (W - w) / 2;
                OH = (int)rint((double)h * zf); OW = (int)rint((double)w * zf);    // ndimage.zoom: int(round(n * zoom))
                trim_top = (OH - H) / 2; trim_left = (OW - W) / 2;
            }
            spline_coefficients(plane, W, top, left, h, w, coef, tid);              // ends with a barrier: the plane is free
            // output index (q0, q1) of the ndimage.zoom result samples q * (n_in - 1) / (n_out - 1)
            const double s0 = OH > 1 ? (double)(h - 1) / (double)(OH - 1) : 1.0;
            const double s1 = OW > 1 ? (double)(w - 1) / (double)(OW - 1) : 1.0;
            for (int o = tid; o < n; o += NT) {
                const int o0 = o / W, o1 = o - o0 * W;
                float v = 0.0f;
                if (zf < 1.0) {
                    const int q0 = o0 - otop, q1 = o1 - oleft;
                    if (q0 >= 0 && q0 < zh && q1 >= 0 && q1 < zw) v = sample(coef, h, w, q0 * s0, q1 * s1);
                } else {
                    v = sample(coef, h, w, (o0 + trim_top) * s0, (o1 + trim_left) * s1);
                }
                plane[o] = clampf(v, lo, hi);
            }
        }
        __syncthreads();
    }

    float* dst = a.dst + b * (int64_t)n;
    if (a.stages & RML_CHAIN_NOISE) {
        const float nz = (float)par[7];                     // float32 array += Python float: NumPy adds in float32
        for (int i = tid; i < n; i += NT) dst[i] = clampf(plane[i] + nz, lo, hi);
    } else {
        for (int i = tid; i < n; i += NT) dst[i] = plane[i];
    }
}

}  // namespace

extern "C" int rml_augment_chain(rml_ctx* ctx, int stages, const float* src, int64_t in_stride, int64_t B, int H, int W, float sub,
                                 float div, float lo, float hi, const double* params, float* dst, void* stream) {
    RML_REQUIRE(ctx && B >= 0 && H > 0 && W > 0, RML_ERR_INVALID, "rml_augment_chain: bad arguments");
    RML_REQUIRE((stages & ~(RML_CHAIN_ROTATE | RML_CHAIN_ZOOM | RML_CHAIN_NOISE)) == 0, RML_ERR_INVALID, "rml_augment_chain: unknown stage in mask %d", stages);
    RML_REQUIRE(lo <= hi, RML_ERR_INVALID, "rml_augment_chain: clamp range [%g, %g]", (double)lo, (double)hi);
    if (B == 0) return RML_OK;
    RML_REQUIRE(src && dst && (params || stages == 0), RML_ERR_INVALID, "rml_augment_chain: NULL argument");
    RML_REQUIRE(B < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "rml_augment_chain: B too large");
    const bool spline = (stages & (RML_CHAIN_ROTATE | RML_CHAIN_ZOOM)) != 0;
    const size_t lds = (size_t)H * W * (sizeof(float) + (spline ? sizeof(double) : 0));
    RML_REQUIRE(lds <= 150 * 1024, RML_ERR_UNSUPPORTED, "rml_augment_chain: plane too large for the LDS-resident chain");
    RML_REQUIRE(in_stride >= (int64_t)H * W, RML_ERR_INVALID, "rml_augment_chain: in_stride %lld < H*W", (long long)in_stride);
    RML_HIP(hipSetDevice(ctx->device));
    RML_MAX_DYN_LDS(160 * 1024, &k_augment_chain);
    ChainArgs a{src, in_stride, dst, H, W, stages, sub, div, lo, hi, params};
    hipLaunchKernelGGL(k_augment_chain, dim3((unsigned)B), dim3(NT), lds, static_cast<hipStream_t>(stream), a);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
