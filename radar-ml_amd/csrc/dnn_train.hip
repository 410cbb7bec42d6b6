// One float32 training (or evaluation) step of the multi-view CNN of dnn.py:45-91 on the device: forward in train mode, weighted
// softmax cross-entropy, gradients of all 18 parameter tensors.  The optimizer is rml_adam_step (optim.hip).
//
// The batch is rows[0..B) of resident planes / labels: no gather copy.  Launches of a TRAIN step, all on the caller's stream:
//   k_prep         rows / labels checked -> status; the second convolution kernels repacked for the two trunk kernels
//   k_trunk_fwd    (conv2 row, branch, sample): conv1 of the 7 plane rows under it into LDS (never stored), conv2 + relu -> feat
//   k_fc1_fwd      Dense 64 over K = (H/4)(W/4)*96 cut into slices of 256: partial sums [slice][b][64]
//   k_head         per sample: slices added in order, relu, dropout, Dense 64, dropout, Dense C, loss, dlogits, back to dz1
//   k_head_wgrad   gradients of the two small dense layers and the first bias: one thread per element, sum over b in order;
//                  one thread adds the batch's loss and correct count to the accumulators
//   k_fc1_bwd      thread per k: dW1[.][k] (sum over b in order) and the masked feature gradient, in place over feat
//   k_trunk_bwd    (row split, branch, sample): conv1 recomputed, conv2 weight gradient in registers, conv2 data gradient by
//                  2x2 blocks of conv1 pixels -> conv1 gradients; partial sums per workgroup
//   k_conv_reduce  the partial sums added in workgroup order -> the convolution gradients
// EVAL runs the first four without dropout and the accumulator thread of the fifth.
// No atomics anywhere: every sum has one owner and one order, so a call repeated on the same inputs gives the same bits.
// All arithmetic is float32 fmaf chains on the vector ALU (the matrix-core form of the two large products is future work:
// DESIGN.md 3.5c).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rml_internal.h"

namespace {

constexpr int kT = 256;             // threads of the trunk / fc1 forward kernels
constexpr int kMaxB = RML_DNN_TRAIN_MAX_BATCH;
constexpr int kW2N = 32 * 576;      // one branch's second convolution kernel
constexpr int kFcSlice = 256;       // K per workgroup of k_fc1_fwd
constexpr int kJB = 5;              // 2x2 conv1 blocks per thread and pass of the conv2 data gradient

struct Params { const float* p[18]; };      // 3 x (k1, b1, k2, b2), fc1 W b, fc2 W b, fc3 W b (torch layouts)
struct Grads { float* g[18]; };

// ---- dropout: a counter-based draw, a function of (seed, step, layer, sample position, unit) only ---------------------------
__host__ __device__ inline uint64_t mix64(uint64_t z) {        // splitmix64's finalizer
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline bool dropout_keep(uint64_t seed, int64_t step, int layer, int b, int j, float rate) {
    uint64_t h = mix64(seed + 0x9E3779B97F4A7C15ull);
    h = mix64(h ^ ((uint64_t)step * 0xD1342543DE82EF95ull + (uint64_t)layer));
    h = mix64(h ^ (((uint64_t)(uint32_t)b << 32) | (uint32_t)j));
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);  // 24 bits: exact in float32, in [0, 1)
    return u >= rate;                                           // Keras: keep where the uniform draw is >= rate
}

struct Geo {
    int B, N, H, W, C, H1, W1, H2, W2, K, NS, S;
    int64_t HW;
};

struct WsLayout {           // offsets in floats
    size_t w2p, w2q, feat, part, act, pc2, pb2, pc1, total;
};
// act: per sample h1 | h2 | g1 | g2 | dz1 | dz2 (64 each), dz3 (16), loss, correct -> 402, padded to 448
constexpr int kAct = 448;
constexpr int A_H1 = 0, A_H2 = 64, A_G1 = 128, A_G2 = 192, A_DZ1 = 256, A_DZ2 = 320, A_DZ3 = 384, A_LOSS = 400, A_CORR = 401;

__host__ inline int row_splits(int B, int H2) {
    int ns = 256 / (3 * B) + 1;
    return ns > H2 ? H2 : ns;
}
__host__ inline Geo make_geo(int B, int N, int H, int W, int C) {
    Geo g;
    g.B = B; g.N = N; g.H = H; g.W = W; g.C = C;
    g.H1 = H / 2; g.W1 = W / 2; g.H2 = H / 4; g.W2 = W / 4;
    g.K = g.H2 * g.W2 * 96;
    g.NS = row_splits(B, g.H2);
    g.S = (g.K + kFcSlice - 1) / kFcSlice;
    g.HW = (int64_t)H * W;
    return g;
}
__host__ inline WsLayout make_layout(const Geo& g) {
    WsLayout l;
    size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
    l.w2p = take(3 * (size_t)kW2N);
    l.w2q = take(3 * (size_t)kW2N);
    l.feat = take((size_t)g.B * g.K);
    l.part = take((size_t)g.S * g.B * 64);
    l.act = take((size_t)g.B * kAct);
    // partial-sum slots for every batch of up to B samples (B * NS is not monotonic in B: a caller that sizes one workspace for its
    // nominal batch passes the partial last batch of an epoch too)
    size_t nb = 0;
    for (int b = 1; b <= g.B; ++b) {
        const size_t n = (size_t)b * row_splits(b, g.H2);
        if (n > nb) nb = n;
    }
    l.pc2 = take(3 * nb * kW2N);
    l.pb2 = take(3 * nb * 32);
    l.pc1 = take(3 * nb * 640);
    l.total = o;
    return l;
}

// ---- k_prep ------------------------------------------------------------------------------------------------------------------
// k2 element (c, cin, tap) of a branch sits at c * 576 + cin * s_cin + tap * s_tap (contiguous OIHW: 9, 1; channels_last: 1, 64).
// w2p [br][k][c] (k = tap * 64 + cin) feeds the forward kernel, lanes over c; w2q [br][c][k] the data gradient, lanes over cin.
__global__ __launch_bounds__(kT) void k_prep(Params P, int s_cin, int s_tap, float* __restrict__ w2p, float* __restrict__ w2q,
                                             const int32_t* __restrict__ rows, const int32_t* __restrict__ labels, int B, int N, int C,
                                             int32_t* status) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i < 3 * kW2N) {
        const int br = i / kW2N, r = i % kW2N, c = r / 576, k = r % 576, tap = k >> 6, cin = k & 63;
        const float v = P.p[4 * br + 2][c * 576 + cin * s_cin + tap * s_tap];
        w2q[i] = v;
        w2p[br * kW2N + k * 32 + c] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < B) {
        const int r = rows[threadIdx.x];
        bool bad = r < 0 || r >= N;
        if (!bad) {
            const int y = labels[r];
            bad = y < 0 || y >= C;
        }
        if (bad) *status = -1;
    }
}

// ---- conv1 of the rows under one conv2 row ---------------------------------------------------------------------------------------
// ps [7][W + 1]: plane rows 4 oy .. 4 oy + 6 (zero beyond the plane: TF 'same' pads bottom / right on even sizes);
// a1s [3][W1 + 1][64]: relu(conv1) rows 2 oy .. 2 oy + 2 (zero at row H1 / column W1: conv2's pad).  Ends with a barrier.
__device__ __forceinline__ void conv1_rows(const float* __restrict__ plane, const Geo& g, int oy, const float* __restrict__ k1,
                                           const float* __restrict__ b1, float* ps, float* a1s) {
    const int PW = g.W + 1, AW = g.W1 + 1;
    for (int i = threadIdx.x; i < 7 * PW; i += kT) {
        const int r = i / PW, x = i - r * PW, y = 4 * oy + r;
        ps[i] = (y < g.H && x < g.W) ? plane[(int64_t)y * g.W + x] : 0.0f;
    }
    __syncthreads();
    const int cin = threadIdx.x & 63;
    float w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = k1[cin * 9 + t];
    const float bb = b1[cin];
    for (int i = threadIdx.x >> 6; i < 3 * AW; i += kT / 64) {
        const int r = i / AW, x = i - r * AW;
        float v = 0.0f;
        if (2 * oy + r < g.H1 && x < g.W1) {
            float a = bb;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) a = fmaf(w[ky * 3 + kx], ps[(2 * r + ky) * PW + 2 * x + kx], a);
            v = fmaxf(a, 0.0f);
        }
        a1s[i * 64 + cin] = v;
    }
    __syncthreads();
}

__host__ inline size_t trunk_lds_floats(const Geo& g) {
    const size_t rows = (size_t)3 * (g.W1 + 1) * 64 + (size_t)2 * (g.W2 + 1) * 32;
    return (size_t)7 * (g.W + 1) + (rows > 2560 ? rows : 2560);       // 2560: k_trunk_bwd's [4][10][64] reduction over the same space
}

// ---- k_trunk_fwd: grid (H2, 3, B) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_trunk_fwd(const float* xz, const float* yz, const float* xy, const int32_t* __restrict__ rows,
                                                  Geo g, Params P, const float* __restrict__ w2p, float* __restrict__ feat,
                                                  const int32_t* __restrict__ status) {
    if (*status != 0) return;
    extern __shared__ float lds[];
    float* ps = lds;
    float* a1s = lds + 7 * (g.W + 1);
    const int oy = blockIdx.x, br = blockIdx.y, b = blockIdx.z;
    const float* plane = (br == 0 ? xz : br == 1 ? yz : xy) + (int64_t)rows[b] * g.HW;
    conv1_rows(plane, g, oy, P.p[4 * br], P.p[4 * br + 1], ps, a1s);
    const int c = threadIdx.x & 31, grp = threadIdx.x >> 5, AW = g.W1 + 1;
    int ox[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) ox[i] = min(grp + 8 * i, g.W2 - 1);
    float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float* wp = w2p + br * kW2N + c;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const float* wk = wp + (ky * 3 + kx) * 64 * 32;
            const float* ak = a1s + (ky * AW + kx) * 64;
#pragma unroll 8
            for (int cin = 0; cin < 64; ++cin) {
                const float w = wk[cin * 32];
#pragma unroll
                for (int i = 0; i < 5; ++i) acc[i] = fmaf(w, ak[2 * ox[i] * 64 + cin], acc[i]);
            }
        }
    const float bb = P.p[4 * br + 3][c];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int o = grp + 8 * i;
        if (o < g.W2) feat[(size_t)b * g.K + (size_t)(oy * g.W2 + o) * 96 + br * 32 + c] = fmaxf(acc[i] + bb, 0.0f);
    }
}

// ---- k_fc1_fwd: grid S; part[s][b][j] = sum over the slice's k of feat[b][k] * W1[j][k], ascending k ------------------------------
__global__ __launch_bounds__(kT) void k_fc1_fwd(const float* __restrict__ feat, const float* __restrict__ W1, Geo g, float* __restrict__ part,
                                                const int32_t* __restrict__ status) {
    if (*status != 0) return;
    __shared__ float fs[64][65], ws[64][65];
    const int t = threadIdx.x, tb = t >> 4, tj = t & 15;
    const int k_begin = blockIdx.x * kFcSlice, k_end = min(g.K, k_begin + kFcSlice);
    float acc[4][4] = {};
    for (int k0 = k_begin; k0 < k_end; k0 += 64) {
        for (int e = t; e < 64 * 64; e += kT) {
            const int r = e >> 6, kk = e & 63, k = k0 + kk;
            fs[r][kk] = (r < g.B && k < k_end) ? feat[(size_t)r * g.K + k] : 0.0f;
            ws[r][kk] = (k < k_end) ? W1[(size_t)r * g.K + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 64; ++kk) {
            float a[4], w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = fs[tb + 16 * i][kk]; w[i] = ws[tj + 16 * i][kk]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], w[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = tb + 16 * i;
        if (b < g.B)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[((size_t)blockIdx.x * g.B + b) * 64 + tj + 16 * j] = acc[i][j];
    }
}

// ---- k_head: grid B, 64 threads ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_head(const float* __restrict__ part, Geo g, Params P, const int32_t* __restrict__ rows,
                                             const int32_t* __restrict__ labels, const float* __restrict__ class_weight, uint64_t seed,
                                             int64_t step, float rate, float keep_scale, int train, float* __restrict__ act,
                                             const int32_t* __restrict__ status) {
    if (*status != 0) return;
    __shared__ float h1[64], h2[64], z3[16], d3[16], d2[64];
    const int j = threadIdx.x, b = blockIdx.x;
    float* A = act + (size_t)b * kAct;
    const float *W2 = P.p[14], *W3 = P.p[16];
    // Dense 64: the K slices in order, bias last
    float z = 0.0f;
    for (int s = 0; s < g.S; ++s) z += part[((size_t)s * g.B + b) * 64 + j];
    z += P.p[13][j];
    float m1 = 1.0f, m2 = 1.0f;
    if (train) {
        m1 = dropout_keep(seed, step, 0, b, j, rate) ? keep_scale : 0.0f;
        m2 = dropout_keep(seed, step, 1, b, j, rate) ? keep_scale : 0.0f;
    }
    const float g1 = z > 0.0f ? m1 : 0.0f;
    h1[j] = fmaxf(z, 0.0f) * m1;
    __syncthreads();
    z = 0.0f;
    for (int i = 0; i < 64; ++i) z = fmaf(W2[j * 64 + i], h1[i], z);
    z += P.p[15][j];
    const float g2 = z > 0.0f ? m2 : 0.0f;
    h2[j] = fmaxf(z, 0.0f) * m2;
    __syncthreads();
    if (j < g.C) {
        z = 0.0f;
        for (int i = 0; i < 64; ++i) z = fmaf(W3[j * 64 + i], h2[i], z);
        z3[j] = z + P.p[17][j];
    }
    __syncthreads();
    const int y = labels[rows[b]];
    const float wy = class_weight ? class_weight[y] : 1.0f;
    // log-softmax on the logits (what Keras' sparse categorical cross-entropy does with a softmax output)
    float mx = z3[0];
    int arg = 0;
    for (int c = 1; c < g.C; ++c)
        if (z3[c] > mx) { mx = z3[c]; arg = c; }
    float se = 0.0f;
    for (int c = 0; c < g.C; ++c) se += expf(z3[c] - mx);
    const float lse = mx + logf(se);
    if (j == 0) {
        A[A_LOSS] = wy * (lse - z3[y]);
        A[A_CORR] = arg == y ? 1.0f : 0.0f;
    }
    if (!train) return;
    if (j < g.C) {
        const float p = expf(z3[j] - lse);
        const float d = wy * (p - (j == y ? 1.0f : 0.0f)) / (float)g.B;
        d3[j] = d;
        A[A_DZ3 + j] = d;
    }
    __syncthreads();
    float d = 0.0f;
    for (int c = 0; c < g.C; ++c) d = fmaf(d3[c], W3[c * 64 + j], d);
    d *= g2;
    d2[j] = d;
    A[A_DZ2 + j] = d;
    A[A_H1 + j] = h1[j];
    A[A_H2 + j] = h2[j];
    __syncthreads();
    d = 0.0f;
    for (int i = 0; i < 64; ++i) d = fmaf(d2[i], W2[i * 64 + j], d);
    A[A_DZ1 + j] = d * g1;
}

// ---- k_head_wgrad: one thread per element of fc3.W, fc3.b, fc2.W, fc2.b, fc1.b, and one for the accumulators ---------------------
__global__ __launch_bounds__(kT) void k_head_wgrad(const float* __restrict__ act, Geo g, Grads G, int train, double* loss_sum, int32_t* correct,
                                                   const int32_t* __restrict__ status) {
    if (*status != 0) return;
    int i = blockIdx.x * kT + threadIdx.x;
    if (i == 0) {
        float l = 0.0f, c = 0.0f;
        for (int b = 0; b < g.B; ++b) { l += act[(size_t)b * kAct + A_LOSS]; c += act[(size_t)b * kAct + A_CORR]; }
        *loss_sum += (double)l;
        *correct += (int32_t)c;
        return;
    }
    if (!train) return;
    i -= 1;
    int xo, yo = -1;             // sum over b of act[b][xo] * (yo < 0 ? 1 : act[b][yo])
    float* out;
    if (i < g.C * 64) { xo = A_DZ3 + i / 64; yo = A_H2 + i % 64; out = G.g[16] + i; }
    else if ((i -= g.C * 64) < g.C) { xo = A_DZ3 + i; out = G.g[17] + i; }
    else if ((i -= g.C) < 4096) { xo = A_DZ2 + i / 64; yo = A_H1 + i % 64; out = G.g[14] + i; }
    else if ((i -= 4096) < 64) { xo = A_DZ2 + i; out = G.g[15] + i; }
    else if ((i -= 64) < 64) { xo = A_DZ1 + i; out = G.g[13] + i; }
    else return;
    float s = 0.0f;
    if (yo < 0) for (int b = 0; b < g.B; ++b) s += act[(size_t)b * kAct + xo];
    else for (int b = 0; b < g.B; ++b) s = fmaf(act[(size_t)b * kAct + xo], act[(size_t)b * kAct + yo], s);
    *out = s;
}

// ---- k_fc1_bwd: grid ceil(K / 128), 128 threads; thread = one k ---------------------------------------------------------------
// dW1[j][k] = sum_b dz1[b][j] feat[b][k] (ascending b); feat[b][k] <- (feat > 0) * sum_j dz1[b][j] W1[j][k]: the gradient of the conv2
// pre-activation, in place (this thread was the last reader of feat[.][k]).
__global__ __launch_bounds__(128) void k_fc1_bwd(float* __restrict__ feat, const float* __restrict__ W1, const float* __restrict__ act, Geo g,
                                                 float* __restrict__ dW1, const int32_t* __restrict__ status) {
    if (*status != 0) return;
    __shared__ float dz[kMaxB * 64];
    for (int i = threadIdx.x; i < g.B * 64; i += 128) dz[i] = act[(size_t)(i >> 6) * kAct + A_DZ1 + (i & 63)];
    __syncthreads();
    const int k = blockIdx.x * 128 + threadIdx.x;
    if (k >= g.K) return;
    float w[64], acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) { w[j] = W1[(size_t)j * g.K + k]; acc[j] = 0.0f; }
    for (int b = 0; b < g.B; ++b) {
        const float f = feat[(size_t)b * g.K + k];
        float d = 0.0f;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const float s = dz[b * 64 + j];
            acc[j] = fmaf(s, f, acc[j]);
            d = fmaf(s, w[j], d);
        }
        feat[(size_t)b * g.K + k] = f > 0.0f ? d : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 64; ++j) dW1[(size_t)j * g.K + k] = acc[j];
}

// ---- k_trunk_bwd: grid (NS, 3, B) -----------------------------------------------------------------------------------------------
// dzf = feat after k_fc1_bwd.  The workgroup walks its conv2 rows; per row oy it holds conv1 rows 2 oy .. 2 oy + 2 (recomputed) and the
// gradient rows oy - 1, oy (dzs, one zero pixel in front of each row).
//   conv2 kernel gradient: thread (cin, 8 channels c) keeps 8 x 9 sums over the pixels of its rows.
//   conv1 pixels (2 oy + r, 2 j + q), r, q in {0, 1}: each of the nine conv2 taps reaches the block exactly once -- tap (ky, kx) from
//   pixel (oy - [ky == 2], j - [kx == 2]) into (r, q) = ([ky == 1], [kx == 1]).  Masked by conv1's relu, the block's gradient goes into
//   this thread's 9 + 1 sums of the first kernel and bias.
__global__ __launch_bounds__(kT) void k_trunk_bwd(const float* xz, const float* yz, const float* xy, const int32_t* __restrict__ rows, Geo g,
                                                  Params P, const float* __restrict__ w2q, const float* __restrict__ dzf,
                                                  float* __restrict__ pc2, float* __restrict__ pb2, float* __restrict__ pc1,
                                                  const int32_t* __restrict__ status) {
    if (*status != 0) return;
    extern __shared__ float lds[];
    const int PW = g.W + 1, AW = g.W1 + 1, DW = g.W2 + 1;
    float* ps = lds;
    float* a1s = ps + 7 * PW;
    float* dzs = a1s + 3 * AW * 64;
    const int sp = blockIdx.x, br = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const float* plane = (br == 0 ? xz : br == 1 ? yz : xy) + (int64_t)rows[b] * g.HW;
    const int oy0 = (int)((int64_t)sp * g.H2 / g.NS), oy1 = (int)((int64_t)(sp + 1) * g.H2 / g.NS);
    const int cin = t & 63, grp = t >> 6;
    float accw[8][9] = {};
    float gk[9] = {};
    float gb = 0.0f, sb2 = 0.0f;
    const float* wq = w2q + br * kW2N + cin;
    for (int oy = oy0; oy < oy1; ++oy) {
        __syncthreads();                            // the previous row's readers are done with the LDS
        for (int i = t; i < 2 * DW * 32; i += kT) {
            const int slot = i / (DW * 32), r = i - slot * DW * 32, px = r >> 5, c = r & 31, row = oy - 1 + slot;
            dzs[i] = (px > 0 && row >= 0) ? dzf[(size_t)b * g.K + (size_t)(row * g.W2 + px - 1) * 96 + br * 32 + c] : 0.0f;
        }
        conv1_rows(plane, g, oy, P.p[4 * br], P.p[4 * br + 1], ps, a1s);
        // conv2 kernel and bias gradient of row oy
        for (int ox = 0; ox < g.W2; ++ox) {
            float a[9];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) a[ky * 3 + kx] = a1s[(ky * AW + 2 * ox + kx) * 64 + cin];
            const float* dp = dzs + (DW + ox + 1) * 32 + grp * 8;
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) {
                const float d = dp[ci];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) accw[ci][tap] = fmaf(d, a[tap], accw[ci][tap]);
            }
            if (t < 32) sb2 += dzs[(DW + ox + 1) * 32 + t];
        }
        // conv2 data gradient of conv1 rows 2 oy, 2 oy + 1 -> conv1 gradients
        for (int jb = grp * kJB; jb < g.W2; jb += 4 * kJB) {
            float da[kJB][4] = {};
            int jc[kJB];
#pragma unroll
            for (int jj = 0; jj < kJB; ++jj) jc[jj] = min(jb + jj, g.W2 - 1);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int slot = ky == 2 ? 0 : 1, rq = (ky == 1 ? 2 : 0) + (kx == 1 ? 1 : 0), sh = kx == 2 ? 0 : 1;
                    const float* wt = wq + (ky * 3 + kx) * 64;
                    const float* dr = dzs + slot * DW * 32;
#pragma unroll 4
                    for (int c = 0; c < 32; ++c) {
                        const float w = wt[c * 576];
#pragma unroll
                        for (int jj = 0; jj < kJB; ++jj) da[jj][rq] = fmaf(dr[(jc[jj] + sh) * 32 + c], w, da[jj][rq]);
                    }
                }
#pragma unroll
            for (int jj = 0; jj < kJB; ++jj) {
                if (jb + jj >= g.W2) continue;
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int r = rq >> 1, x = 2 * (jb + jj) + (rq & 1);
                    const float d = a1s[(r * AW + x) * 64 + cin] > 0.0f ? da[jj][rq] : 0.0f;
                    gb += d;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) gk[ky * 3 + kx] = fmaf(d, ps[(2 * r + ky) * PW + 2 * x + kx], gk[ky * 3 + kx]);
                }
            }
        }
    }
    const size_t slot = (size_t)br * g.B * g.NS + (size_t)b * g.NS + sp;
    float* o2 = pc2 + slot * kW2N;
#pragma unroll
    for (int ci = 0; ci < 8; ++ci)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) o2[(grp * 8 + ci) * 576 + tap * 64 + cin] = accw[ci][tap];
    if (t < 32) pb2[slot * 32 + t] = sb2;
    // the four groups' conv1 sums, added in group order
    __syncthreads();
    float* red = a1s;                               // [4][10][64]
#pragma unroll
    for (int q = 0; q < 9; ++q) red[(grp * 10 + q) * 64 + cin] = gk[q];
    red[(grp * 10 + 9) * 64 + cin] = gb;
    __syncthreads();
    for (int i = t; i < 640; i += kT) pc1[slot * 640 + i] = ((red[i] + red[640 + i]) + red[1280 + i]) + red[1920 + i];
}

// ---- k_conv_reduce: the per-workgroup partial sums in workgroup order -> gradients in the parameters' layouts -----------------------
__global__ __launch_bounds__(kT) void k_conv_reduce(const float* __restrict__ pc2, const float* __restrict__ pb2, const float* __restrict__ pc1,
                                                    Geo g, Grads G, int s_cin, int s_tap, const int32_t* __restrict__ status) {
    if (*status != 0) return;
    const int per = kW2N + 32 + 640;
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= 3 * per) return;
    const int br = i / per;
    int r = i - br * per;
    const int nb = g.B * g.NS;
    const float* src;
    size_t stride;
    float* out;
    if (r < kW2N) {
        const int c = r / 576, k = r % 576, tap = k >> 6, cin = k & 63;
        src = pc2 + (size_t)br * nb * kW2N + r; stride = kW2N;
        out = G.g[4 * br + 2] + c * 576 + cin * s_cin + tap * s_tap;
    } else if ((r -= kW2N) < 32) {
        src = pb2 + (size_t)br * nb * 32 + r; stride = 32;
        out = G.g[4 * br + 3] + r;
    } else {
        r -= 32;
        const int q = r >> 6, cin = r & 63;
        src = pc1 + (size_t)br * nb * 640 + r; stride = 640;
        out = q < 9 ? G.g[4 * br] + cin * 9 + q : G.g[4 * br + 1] + cin;
    }
    float s = 0.0f;
    for (int n = 0; n < nb; ++n) s += src[(size_t)n * stride];
    *out = s;
}

}  // namespace

extern "C" int rml_dnn_train_supported(int H, int W, int C) {
    return H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0 && W <= 128 && H <= 4096 && C >= 2 && C <= 16;
}

extern "C" int64_t rml_dnn_train_workspace_bytes(int B, int H, int W, int C) {
    if (B < 1 || B > kMaxB || !rml_dnn_train_supported(H, W, C)) return 0;
    return (int64_t)make_layout(make_geo(B, 1, H, W, C)).total * 4;
}

extern "C" int rml_dnn_dropout_mask(uint64_t seed, int64_t step, int layer, int b, int n_units, float rate, uint8_t* keep) {
    RML_REQUIRE(keep && n_units >= 0 && b >= 0 && layer >= 0 && rate >= 0.0f && rate < 1.0f, RML_ERR_INVALID, "rml_dnn_dropout_mask: bad arguments");
    for (int j = 0; j < n_units; ++j) keep[j] = dropout_keep(seed, step, layer, b, j, rate) ? 1 : 0;
    return RML_OK;
}

extern "C" int rml_dnn_train_step(rml_ctx* ctx, const float* xz, const float* yz, const float* xy, const int32_t* labels, const int32_t* rows,
                                  int B, int64_t N, int H, int W, const float* class_weight, int C, const void* const* params,
                                  void* const* grads, int k2_layout, uint64_t seed, int64_t step, float rate, int mode, void* workspace,
                                  int64_t workspace_bytes, double* loss_sum, int32_t* correct, int32_t* status, void* stream) {
    RML_REQUIRE(ctx && xz && yz && xy && labels && rows && params && workspace && loss_sum && correct && status, RML_ERR_INVALID,
                "rml_dnn_train_step: NULL argument");
    RML_REQUIRE(mode == RML_DNN_TRAIN || mode == RML_DNN_EVAL, RML_ERR_INVALID, "rml_dnn_train_step: mode %d", mode);
    RML_REQUIRE(rml_dnn_train_supported(H, W, C), RML_ERR_UNSUPPORTED,
                "rml_dnn_train_step: %d x %d planes, %d classes (H, W multiples of 4, W <= 128, 2..16 classes)", H, W, C);
    RML_REQUIRE(B >= 1 && B <= kMaxB, RML_ERR_UNSUPPORTED, "rml_dnn_train_step: batch of %d (1..%d)", B, kMaxB);
    RML_REQUIRE(N >= 1 && N < (int64_t)1 << 31, RML_ERR_INVALID, "rml_dnn_train_step: N = %lld", (long long)N);
    RML_REQUIRE(rate >= 0.0f && rate < 1.0f, RML_ERR_INVALID, "rml_dnn_train_step: dropout rate %g", (double)rate);
    RML_REQUIRE(k2_layout == 0 || k2_layout == 1, RML_ERR_INVALID, "rml_dnn_train_step: k2_layout %d", k2_layout);
    const bool train = mode == RML_DNN_TRAIN;
    RML_REQUIRE(!train || grads, RML_ERR_INVALID, "rml_dnn_train_step: TRAIN needs the gradient tensors");
    const Geo g = make_geo(B, (int)N, H, W, C);
    const WsLayout L = make_layout(g);
    RML_REQUIRE(workspace_bytes >= (int64_t)L.total * 4 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, RML_ERR_INVALID,
                "rml_dnn_train_step: workspace of %lld bytes, 16-byte aligned, needed", (long long)L.total * 4);
    Params P;
    Grads G;
    for (int i = 0; i < 18; ++i) {
        P.p[i] = static_cast<const float*>(params[i]);
        G.g[i] = train ? static_cast<float*>(grads[i]) : nullptr;
        RML_REQUIRE(P.p[i] && (!train || G.g[i]), RML_ERR_INVALID, "rml_dnn_train_step: parameter / gradient %d is NULL", i);
    }
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const int s_cin = k2_layout ? 1 : 9, s_tap = k2_layout ? 64 : 1;
    const size_t lds = trunk_lds_floats(g) * sizeof(float);
    const float keep_scale = 1.0f / (1.0f - rate);
    hipLaunchKernelGGL(k_prep, dim3((3 * kW2N + kT - 1) / kT), dim3(kT), 0, st, P, s_cin, s_tap, ws + L.w2p, ws + L.w2q, rows, labels, B, (int)N,
                       C, status);
    hipLaunchKernelGGL(k_trunk_fwd, dim3(g.H2, 3, B), dim3(kT), lds, st, xz, yz, xy, rows, g, P, ws + L.w2p, ws + L.feat, status);
    hipLaunchKernelGGL(k_fc1_fwd, dim3(g.S), dim3(kT), 0, st, ws + L.feat, P.p[12], g, ws + L.part, status);
    hipLaunchKernelGGL(k_head, dim3(B), dim3(64), 0, st, ws + L.part, g, P, rows, labels, class_weight, seed, step, rate, keep_scale,
                       train ? 1 : 0, ws + L.act, status);
    const int n_head = 1 + C * 64 + C + 4096 + 64 + 64;
    hipLaunchKernelGGL(k_head_wgrad, dim3(train ? (n_head + kT - 1) / kT : 1), dim3(kT), 0, st, ws + L.act, g, G, train ? 1 : 0, loss_sum, correct,
                       status);
    if (train) {
        hipLaunchKernelGGL(k_fc1_bwd, dim3((g.K + 127) / 128), dim3(128), 0, st, ws + L.feat, P.p[12], ws + L.act, g, G.g[12], status);
        hipLaunchKernelGGL(k_trunk_bwd, dim3(g.NS, 3, B), dim3(kT), lds, st, xz, yz, xy, rows, g, P, ws + L.w2q, ws + L.feat, ws + L.pc2,
                           ws + L.pb2, ws + L.pc1, status);
        hipLaunchKernelGGL(k_conv_reduce, dim3((3 * (kW2N + 32 + 640) + kT - 1) / kT), dim3(kT), 0, st, ws + L.pc2, ws + L.pb2, ws + L.pc1, g, G,
                           s_cin, s_tap, status);
    }
    RML_HIP(hipGetLastError());
    return RML_OK;
}
