// Internal declarations shared by the HIP translation units of libradarml_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/radarml.h"

// device copy of Pillow's precompute_coeffs() table for one (in, out) size pair (resize.hip)
struct rml_resize_tab {
    int in, out, ksize;
    const int* bounds;      // [out][2] (points into the allocation that starts at kk)
    const double* kk;       // [out][ksize]
};

// device tables of the CNN preprocessing kernel for one (grid, output size) pair (preprocess.hip)
struct rml_pre_tab {
    int X, Y, Z, OH, OW;
    void* dev;              // one allocation; the six tables start at off[]
    size_t off[6];
};

// rml_ctx_set_option values.  The defaults are the tuned configuration; the others exist for A/B measurements and for the tests
// that pin one kernel family against another (they used to be environment variables read with getenv inside the launch paths:
// a data race beside a caller's setenv, and invisible in the API).
struct rml_opts {
    int project_share_cu = 0;   // RML_OPT_PROJECT_SHARE_CU
    int waveframe = 1;          // RML_OPT_WAVEFRAME: 0 off, 1 on, 2 quarter-plane buffers everywhere, 3 also short rows stand-alone
    int linplane = 1;           // RML_OPT_LINPLANE: k_project_lin for rows of 40 / 44 / 48 / 56 quads
    int stage_codes = 1;        // RML_OPT_STAGE_CODES: per-wave LDS code stage of the wave-per-frame kernels
    int slice_wave = 1;         // RML_OPT_SLICE_WAVE: k_slice_rows (0: the round-1 workgroup-per-row kernel)
    int derive_fused = 1;       // RML_OPT_DERIVE_FUSED: k_derive_slice (0: sum planes + top-k + slices)
    int code_rmw = -1;          // RML_OPT_CODE_RMW: -1 = the measured rule (rml_code_rmw), 0 / 1 forced
    int gemm_big = -1;          // RML_OPT_GEMM_BIG: -1 = whole-round rule (use_big_gemm), 0 never, 1 for every n >= 256
    int c1_pk = 1;              // RML_OPT_C1_PK: packed first-layer kernels of the SGAN branches
    int64_t chunk = 0;          // RML_OPT_CHUNK: rows per chunk of the chunked front doors, 0 = chosen per batch
    int smo_lds_rows = RML_SMO_LDS_ROWS_MAX;   // RML_OPT_SMO_LDS_ROWS: duals of more rows run on the workspace variant of k_smo
    int conv7 = RML_CONV7_DEFAULT;  // RML_OPT_CONV7: bit 0 forward, bit 1 backward of the generator's output layer on csrc/gen.hip
    int sgd_resident_d = RML_SGD_RESIDENT_D_MAX;   // RML_OPT_SGD_RESIDENT_D: wider problems run on the workspace variant of k_sgd
    int sparse_rows = -1;       // RML_OPT_SPARSE_ROWS: -1 = the measured grid rule (rml_sparse_rows), 0 dense, 1 wherever occupancy words can be had (also in place of split-K)
    int sparse_stores = -1;     // RML_OPT_SPARSE_STORES: -1 = the measured rule (rml_sparse_stores), 0 whole rows, 1 wherever the chunk's plan is sparse and the kernel can skip
    int zoom_rows = 0;          // RML_OPT_ZOOM_ROWS: k_zoom_rows 0 = one workgroup per (row, plane), 1 / 2 one per row: planes together / in turn
};

struct rml_ws_retired {         // a workspace block that was outgrown: freed once the work queued before its retirement is done
    void* p;
    hipEvent_t ev;
};

struct rml_ctx {
    int device = 0;
    int num_cu = 256;
    // grow-on-demand device workspace for the fused front doors (owned by the ctx)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    std::vector<rml_ws_retired> ws_retired;
    rml_opts opt;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_proj[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};   // chunk pipeline of rml_project_svm (two workspaces)
    hipStream_t aux_stream = nullptr;   // second stream for overlapping GEMM with projection
    int64_t sparse_store_launches = 0;          // projection launches with ProjOut::skip_clear on a kernel that honours it (rml_ctx_sparse_store_launches)
    mutable int64_t sparse_gemm_launches = 0;  // launches of k_svm_gemm<I8, PT, false, true> issued so far (rml_ctx_sparse_gemm_launches: the tests' witness)
    uint8_t* bg_line = nullptr;         // 128 bytes of 0x80 (a line of background codes): what the sparse GEMM stager fetches for a clear occupancy bit
    // optional in-situ timing of the projection launches issued by rml_project_svm
    bool profiling = false;
    std::vector<hipEvent_t> prof_ev;    // start/stop pairs
    size_t prof_used = 0;
    int64_t prof_frames = 0;
    std::vector<hipEvent_t> prof_ev_g;  // the same for the GEMM + finish of every chunk (aux stream)
    size_t prof_used_g = 0;
    double prof_ops_g = 0.0;
    std::vector<rml_resize_tab> resize_tabs;    // owned; freed with the context
    std::vector<rml_pre_tab> pre_tabs;          // owned; freed with the context
    // Entry points that use the shared workspace / events / caches take `mu` for the duration of the call and order
    // their stream behind the previous user's work (ev_last), so calls from several host threads or on several
    // streams cannot interleave on the workspace (rml_ctx_guard below).
    std::recursive_mutex mu;
    hipEvent_t ev_last = nullptr;
    bool ev_last_valid = false;
    // pinned host buffer for per-call descriptor tables (rml_stage_reserve / rml_stage_upload), and the event behind its last copy
    void* stage = nullptr;
    size_t stage_bytes = 0;
    hipEvent_t ev_stage = nullptr;
    bool ev_stage_valid = false;
};

// RAII serialisation of one entry point on a context: locks ctx->mu, makes `stream` wait for the work the previous
// guarded call queued (on whatever stream), and on destruction records the new "last use" point on `stream`.
struct rml_ctx_guard {
    rml_ctx* ctx;
    hipStream_t st;
    bool capturing = false;
    explicit rml_ctx_guard(rml_ctx* c, hipStream_t stream) : ctx(c), st(stream) {
        ctx->mu.lock();
        // Inside a stream capture (a caller recording the call into a HIP graph) the cross-call ordering is the caller's: an event
        // recorded by an earlier, un-captured call cannot be waited for from a captured stream on every runtime, and an event recorded
        // INSIDE the capture must not become the "last use" that later un-captured calls wait for.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
        capturing = cs != hipStreamCaptureStatusNone;
        if (!capturing && ctx->ev_last_valid) (void)hipStreamWaitEvent(st, ctx->ev_last, 0);
    }
    ~rml_ctx_guard() {
        if (!capturing && ctx->ev_last && hipEventRecord(ctx->ev_last, st) == hipSuccess) ctx->ev_last_valid = true;
        ctx->mu.unlock();
    }
    rml_ctx_guard(const rml_ctx_guard&) = delete;
    rml_ctx_guard& operator=(const rml_ctx_guard&) = delete;
};

// records an event on st when profiling is on (no-op otherwise)
void rml_prof_mark(rml_ctx* ctx, hipStream_t st);
void rml_prof_mark_gemm(rml_ctx* ctx, hipStream_t st);

// "done once per device" for hipFuncSetAttribute: one process may drive several devices (one context each), and the
// attribute belongs to the device's copy of the kernel
struct rml_once_per_device {
    std::atomic<uint64_t> mask{0};
    bool first(int dev) { const uint64_t bit = 1ull << (dev & 63); return !(mask.fetch_or(bit) & bit); }
};
// allow `bytes` of dynamic LDS for kernel (the variadic part: a template-id may hold commas) on the current device
#define RML_MAX_DYN_LDS(bytes, ...)                                                                                     \
    do {                                                                                                                \
        static rml_once_per_device _once;                                                                               \
        int _dev = 0;                                                                                                   \
        (void)hipGetDevice(&_dev);                                                                                      \
        if (_once.first(_dev))                                                                                          \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(__VA_ARGS__), hipFuncAttributeMaxDynamicSharedMemorySize, (bytes)); \
    } while (0)

void rml_set_error(const char* fmt, ...);
int rml_hip_fail(hipError_t e, const char* what, const char* file, int line);

#define RML_HIP(call)                                                        \
    do {                                                                     \
        hipError_t _e = (call);                                              \
        if (_e != hipSuccess) return rml_hip_fail(_e, #call, __FILE__, __LINE__); \
    } while (0)

#define RML_REQUIRE(cond, status, ...)      \
    do {                                    \
        if (!(cond)) {                      \
            rml_set_error(__VA_ARGS__);     \
            return (status);                \
        }                                   \
    } while (0)

// workspace of at least `bytes` (inside an rml_ctx_guard on `st`); growing allocates -- not inside a stream capture: context.hip
int rml_ws_reserve(rml_ctx* ctx, size_t bytes, void** out, hipStream_t st);

// Per-call descriptor tables (inside an rml_ctx_guard): rml_stage_reserve hands out the context's pinned host buffer, grown to
// `bytes`, after the copy of the previous user has completed (a wait for a few KB queued a whole call ago); rml_stage_upload
// copies its first `bytes` to `dst` asynchronously on `st`.
int rml_stage_reserve(rml_ctx* ctx, size_t bytes, void** host);
int rml_stage_upload(rml_ctx* ctx, void* dst, size_t bytes, hipStream_t st);

// ---- projection (project.hip) -------------------------------------------------------------
struct ProjOut {
    // destination of each plane for frame b: p[pl] + b*stride[pl] (float) ; NULL = plane not wanted
    float* p[3];
    int64_t stride[3];
    uint32_t sel;      // bit pl set: plane pl is part of the row (stored and counted in the statistics)
    // uint8 codes of the same values (before scaling); NULL = not wanted
    uint8_t* q[3];
    int64_t qstride;
    uint8_t* qrow;     // base of the code rows (pad columns [qD, qstride) are zeroed), or NULL
    int64_t qD;
    int32_t* row_isum;
    int64_t* row_isq;
    int32_t* row_flags;
    float scale_div;   // 0/1 => none
    // float row bookkeeping for the SVM front door: zero the pad columns [pD, stride) of the
    // float row at prow + b*pstride, and the float64 squared norm of the (scaled) row
    float* prow;
    int64_t pD, pstride;
    double* row_nsq;
    // predication: the whole launch is a no-op when *skip_if_set != 0 (device flag)
    const int32_t* skip_if_set;
    // set by the fused pipeline: an SVM GEMM runs concurrently on another stream, so a persistent projection kernel
    // should leave every CU the registers / LDS for one of its workgroups (k_project_wave: quarter-plane buffers, one
    // workgroup per CU) -- measured +5 % end to end on the Walabot grid against filling the CUs with projection waves
    int share_cu;
    // the predicated (usually skipped) second pass of the fused pipeline: launch without the LDS pad of share_cu, so that its
    // workgroups can start -- and exit at once -- on CUs whose LDS a resident projection workgroup of the next chunk holds
    int no_pad;
    // Read-compare-write of the code rows: read the old 4 / 16 bytes and store only what changed (always correct: whatever the row
    // held before, it holds the new codes afterwards).  Radar projections are mostly background -- 17 % / 9 % of the codes of a
    // Walabot / 64x64x128 frame are non-zero -- and the rows land in buffers that are re-used batch after batch (the chunk workspaces
    // of the fused pipelines, a caller's code buffer), so most of a row's HBM WRITE traffic -- what the streaming kernels pay
    // 3-15 % for, DESIGN.md 3.1b' -- becomes reads.  The kernels put the old words of a region in flight together (Emitter::old_word).
    int q_rmw;
    // Occupancy words of the code rows (the int8 GEMM's sparse stager, mfma_tile.h): row b has one bit per 128-byte line of its code
    // row at occ + b * occ_words (bit k & 31 of word k >> 5), 1 unless all 128 bytes are the background code (0x80) and the line
    // lies wholly inside qD.  NULL: none wanted.  Written by the wave-per-frame kernels with the code stage (Emitter::flush_wave);
    // a launch of any other kernel fills the words with ones (rml_launch_project), which is always right.
    uint32_t* occ;
    int occ_words;
    // Rows with holes: a line whose occupancy bit stays clear need not be stored -- its consumer, the sparse GEMM, takes it from the
    // constant background line and never reads it from the row.  Honoured only by a kernel that writes `occ` itself (a launch that
    // gets words of all ones stores everything); a set bit's line is always fully stored, a clear bit's line holds anything.  Only the
    // producer of a chunk whose plan is sparse may set it (svm.hip front_chunked; ChunkOps::holes).
    int skip_clear;
};
// rml_code_rmw: the default of ProjOut::q_rmw in the fused pipelines, for frames of frame_bytes volume bytes and D codes.  The
// read-back costs its bytes (and, in a per-frame epilogue, its latency) whatever the rows hold; the stores it saves depend on the
// data.  So the rule is what was measured (tools/exp/README.md round 4; synthetic frames with the sparsity above; sessions r4be /
// r4bf: this library against the library of the commit before, three interleaved whole-round runs on one box):
//   64x64x128 uint8 (rows 3.9 % of the frame): 7.41 -> 7.86 M frames/s (+6 %; +11 % on another box)                        on
//   64x64x128 derive -> slice (rows 1 %): 2.193 -> 2.264 M (+3.2 %)                                                          on
//   Walabot grid, uint8 (rows 8.3 %): -2.5 %                                                                                off
//   Walabot grid, derive -> slice (rows 2.1 %): per store 7.94 -> 7.89 M (kernel in situ -7 %); with the old words loaded
//     alongside the gather's batches (slice_emit<., ., true>, session r4bs) 8.33-8.35 -> 8.33-8.39 M, kernel 0.576 -> 0.585;
//     64x64x128 in that form 2.24 -> 2.26 M, kernel 0.618 -> 0.634                                                          on
//   float32 max projections: +0.7 / +1.1 % end to end at the Walabot grid and +-0.5 % at 64x64x128 against the same library
//     without -- but the prefetched old words and the test in front of every store cost k_project_lin 9 % in situ (0.735 -> 0.665)
//     and the headline 1 % against the library before: those kernels store plainly again (Emitter::rmw = false)              off
// The CNN chain's first pass keeps plain stores (5.98 / 5.97 M frames/s without, 5.87 / 5.96 with).
// rml_ctx_set_option(RML_OPT_CODE_RMW, 0 / 1) forces it off / on where a kernel has it (-1: this rule).
inline int rml_code_rmw(int64_t D, int64_t frame_bytes, bool derive, bool u8) {
    // round 5, FRESH frames (bench.py's sliding windows: no workspace row meets its own frame's old codes; sessions r5c / r5d):
    // 64x64x128 uint8 +2.7 % (the +6-10 % above came with a batch re-run 20 times), derive -> slice +1.6 % / +1.3 % -- below the
    // 2 % bar: the derive pipelines store plainly
    if (derive) return 0;
    return u8 && D * 64 >= frame_bytes && D * 16 <= frame_bytes;
}

// rml_sparse_rows: the default of RML_OPT_SPARSE_ROWS (-1) for a grid.  What was measured (same library, option 0 against -1, three
// interleaved rounds of the fused float32 pipeline on one box, tools/exp/README.md): 64x64x128 -- 69 % of the sample lines and 63 %
// of the SV lines are background -- 22.45 / 22.81 / 22.85 -> 21.77 / 21.49 / 21.47 ms per 65 536 frames (+3 ... +6 %); the Walabot
// grid 22x31x176 -- 45 % / 37 %, rows of 176 codes that straddle the 128-byte lines -- 12.45 / 13.11 / 12.28 -> 12.85 / 12.71 /
// 12.72 ms (-3 / +3 / -3.5 %: no gain).  So: on where a line is a whole number of z-rows (or a whole fraction of one) and every
// plane starts on a line -- background then comes in whole lines --, off elsewhere.
inline int rml_sparse_rows(int X, int Y, int Z) {
    return (Z % 128 == 0 || 128 % Z == 0) && ((int64_t)X * Z) % 128 == 0 && ((int64_t)Y * Z) % 128 == 0;
}

// rml_sparse_stores: the default of RML_OPT_SPARSE_STORES (-1) for a grid -- whether the projection in front of a sparse chunk leaves
// the lines whose occupancy bit is clear unstored (ProjOut::skip_clear).  What was measured at 64x64x128 (bench.py --gpus 1 --steps 20
// --warmup 3, 65 536 frames, one box, alternating runs):
//   the ceiling -- a timing-only arm that stores NO codes (tools/exp/sparse_stores_ablation.patch) against the library before, three
//     pairs: 2.933 / 2.941 / 2.939 -> 3.153 / 3.121 / 3.126 M frames/s (+6.1 ... +7.5 %; the parent's max - min: 0.28 %), k_project_wave
//     in situ 0.806 -> 0.857-0.864 of 8 TB/s;
//   the kernel itself -- 69 % of the lines unstored, one burst of occupied lines per frame left -- against the commit before, five
//     pairs: 2.993 / 2.985 / 2.994 / 2.997 / 2.997 -> 3.072 / 3.058 / 3.065 / 3.071 / 3.072 M frames/s (+2.4 ... +2.7 %, median
//     +2.5 %; the parent's max - min: 0.43 %), same bits, 169.2 -> 54.0 MB written per launch (profiles/sparse_stores_bench.json,
//     profiles/sparse_stores_pmc.txt): on.
// A skipped line must be a whole line of ONE plane, so the rule is rml_sparse_rows' (every plane starts on a line; on the Walabot grid
// only xz does and the rows stay dense anyway).
inline int rml_sparse_stores(int X, int Y, int Z) {
    return rml_sparse_rows(X, Y, Z);
}

// true when rml_launch_project would use the persistent wave-per-frame kernel for this shape (the fused pipeline then
// pairs it with the 128x128 GEMM, whose workgroups fit beside it on a CU)
bool rml_project_uses_wave_kernel(const rml_ctx* ctx, int vdtype, int mode, int X, int Y, int Z, bool share_cu, int64_t B);

int rml_launch_project(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode,
                       const int32_t* ijk, const ProjOut& o, hipStream_t st, int targets_per_frame = 1);

// single observations: mode MAX with every frame split into S pieces along x (project.hip); S = rml_project_split_pieces (0: not taken)
constexpr int RML_SMALL_FRAMES = 8;
int rml_project_split_pieces(int X, int Y, int Z);
size_t rml_project_split_scratch_bytes(int64_t B, int X, int Y, int Z, int S);
int rml_launch_project_split(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, const ProjOut& o, float* scratch, int S,
                             hipStream_t st);

// k_derive_slice (project_slice.hip): DerivedTarget.get_derived_targets (common.py:49-80) and the slices at the derived (i,j,k) in one
// pass over the frames; o.sel == 0: derive only.  RML_ERR_UNSUPPORTED (no message set) when the shape has no fused kernel.
int rml_launch_derive_slice(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int num_targets,
                            int32_t* ijk_out, float* profiles, const ProjOut& o, hipStream_t st);

// the strongest targets of B frames (rml_derive_targets) with the sum planes in the caller's scratch: B * (X*Z + Y*Z) floats, touched
// only by shapes without the fused derive kernel.  For callers whose own chunks live in the context's workspace.
int rml_launch_derive(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int num_targets, int32_t* ijk,
                      float* sums, hipStream_t st);

// ---- projection rows zoomed to a model's geometry (zoom_rows.hip) ------------------------
// One validated geometry of rml_project_zoom / rml_project_zoom_svm: the source grid, the output planes, and how a chunk of
// source-grid rows is kept -- float32 rows of stride Dsrc, or (uint8 volumes: codes by construction) code rows of stride round_up(Dsrc, 128).
struct rml_zoom_plan {
    int vdtype, X, Y, Z, T; uint32_t mask; int32_t out_shape[6];
    bool codes;               // the source rows are code rows
    bool derive;              // mode SLICE without ijk: the T strongest targets of every frame, derived at the source grid
    int64_t Dsrc, Dout, ld_src;
    size_t lds; int by_plane; // dynamic LDS of k_zoom_rows; 0: the planes of a row together, 1: one after the other, 2: a workgroup each
};
// RML_ERR_INVALID / RML_ERR_UNSUPPORTED (a plane whose float64 image exceeds 150 KB) with a message that starts with `who`
int rml_zoom_plan_make(const rml_ctx* ctx, const char* who, int vdtype, int mode, int X, int Y, int Z, int T, bool derive, const int32_t* out_shape,
                       uint32_t mask, rml_zoom_plan* zp);
size_t rml_zoom_stage_bytes(const rml_zoom_plan& zp, int64_t frames);      // scratch of one chunk of `frames` frames (a multiple of 256)
// projection of `frames` frames at the source grid into `scratch`, then k_zoom_rows: frames * T float rows at feat (stride ld_feat,
// columns [Dout, pad_to) zeroed), their float64 squared norms (the sum order of k_prepare_rows) and row flags 0 ("not on the code grid")
int rml_zoom_stage_run(rml_ctx* ctx, const rml_zoom_plan& zp, void* scratch, const void* V, int64_t frames, int mode, const int32_t* ijk,
                       float scale_div, float* feat, int64_t ld_feat, int64_t pad_to, double* row_nsq, int32_t* row_flags, hipStream_t st);

// ---- SVM (svm.hip) ------------------------------------------------------------------------
struct rml_svm {
    int64_t M = 0, Mpad = 0, D = 0;
    int64_t Kq = 0;               // code K extent (bytes)   = round_up(D, 128)
    int64_t Kf = 0;               // float K extent (floats) = round_up(D, 32)
    // Row strides: the K extent, plus one 128-byte granule when that makes the stride an ODD multiple of 128 B.
    // With an even multiple (D = 20 480: 160 x 128 B) the same K-slice of every row of a tile maps to the same
    // L2 channel and the LDS-DMA staging of the GEMM serialises on it.
    int64_t Dq = 0;               // code row stride (bytes)
    int64_t Df = 0;               // float row stride (floats)
    int C = 0, P = 0, PT = 0, kernel = 0;
    double gamma = 0, code_scale = 1;
    bool exact = false, has_calib = false;
    // device buffers
    float* sv_f32 = nullptr;      // Mpad x Df, zero padded
    double* sv_nsq = nullptr;     // Mpad  ||sv||^2 (float64)
    uint8_t* sv_q = nullptr;      // Mpad x Dq codes XOR 0x80 (= int8 code-128); pad = 0
    double* sv_term_q = nullptr;  // Mpad  exact-path per-SV term (see svm.hip)
    double* W = nullptr;          // PT x Mpad per-pair SV weights (zero padded)
    double* intercept = nullptr;  // P
    double* calib = nullptr;      // 2*C (a then b)
    double* platt = nullptr;      // libsvm probA | probB (2 x kMaxP), set by rml_svm_set_platt
    // digit path (general rows on the int8 matrix cores, svm.hip "multi-digit"): every value v is the 32-bit fixed-point
    // number u = (v - dig_c0) / dig_s in [-1, 1), split into four balanced int8 digits; plane i of row r lives at
    // sv_dig + (i * Mpad + r) * Dq (plane-major: the row stride stays the odd multiple of 128 B)
    bool dig_ok = false;
    double dig_c0 = 0, dig_s = 1;
    int8_t* sv_dig = nullptr;     // 4 x Mpad x Dq
    double* sv_dig_nsq = nullptr; // Mpad  ||u_sv||^2 of the quantised values
    uint32_t mask_hint = 0;
    uint32_t* sv_occ = nullptr;   // Mpad x occ_words occupancy words of sv_q (ProjOut::occ's rule; rows M..Mpad hold 0x00: occupied)
    int occ_words = 0;            // (Kq / 128 + 31) / 32
};

// host-side packed operands of a model (rml_svm_pack_host fills them, rml_svm_load uploads them)
struct rml_svm_pack {
    std::vector<double> W, nsq, term, dnsq;
    std::vector<float> svf;
    std::vector<uint8_t> svq;
    std::vector<int8_t> svd;
    std::vector<uint32_t> occ;
};
int rml_svm_pack_host(const double* sv, int64_t M, int64_t D, const double* dual_coef, const int32_t* n_support,
                      int n_classes, int kernel, double gamma, double code_scale, bool has_calib, rml_svm* m, rml_svm_pack* pk);
// bytes of the workspace of one chunk of CH rows (no HIP call).  needs: bit 0 code rows, 1 float rows, 2 digit planes, 3 derived (i,j,k)
size_t rml_svm_ws_bytes(const rml_svm* m, int64_t CH, unsigned needs);

struct rml_linear {
    int64_t D = 0;
    int C = 0;
    bool has_calib = false;
    double* coef = nullptr;       // C x D
    double* intercept = nullptr;  // C
    double* calib = nullptr;      // 2*C
};
