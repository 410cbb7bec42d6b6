/*
 * radarml.h -- C ABI of libradarml_hip.so, the MI355X (gfx950) implementation of the
 * radar-ml batched hot path: 3-D radar volume -> (xz, yz, xy) projections -> feature
 * rows -> RBF-SVM / linear decision function -> labels.
 *
 * The reference (goruck/radar-ml) is pure Python and has no FFI of its own; its
 * boundary for this path is three Python call surfaces.  Each entry
 * point below names the reference site it replaces (paths relative to the reference
 * tree; "sk:" = the scikit-learn package the reference calls into).  The Python side
 * binds these with ctypes (radar-ml_amd/_lib.py; INTEGRATION.md shows the stub a
 * maintainer of the reference would add).
 *
 * Conventions
 *   - every function returns RML_OK (0) or a negative rml_status; no exceptions, no
 *     aborts, nothing printed.  rml_last_error() returns a thread-local message.
 *   - all array arguments are CALLER-OWNED DEVICE pointers unless a parameter is
 *     documented "host".  The library never frees caller memory.
 *   - launches are asynchronous on the caller's hipStream_t (passed as void*; NULL =
 *     the default stream).  A context is bound to one device.
 *   - threads and streams: a context may be shared.  The entry points that use the context's workspace, second
 *     stream or caches (rml_svm_decision, rml_svm_kernel_matrix, rml_project_svm, rml_derive_targets,
 *     rml_resize_bicubic) serialise on it: they hold a per-context mutex for the duration of the (asynchronous) call and
 *     make their stream wait for the device work the previous such call queued, whatever stream that was on.  Calls on
 *     different streams are therefore correct but do not overlap on the device; use one context per stream for that.
 *   - layouts: volumes V[b][i][j][k], C-contiguous, (x=theta index i, y=phi index j,
 *     z=range index k); element type float32 (vdtype RML_VOL_F32) or uint8 (RML_VOL_U8: the
 *     radar's native 0..255 magnitudes as stored by the data sets -- a quarter of the HBM
 *     bytes; results are identical to the float32 path on the same values).  Feature rows are [xz | yz | xy] (the tuple
 *     order of common.py:40), each plane C-order, i.e. exactly
 *     np.concatenate((xz, yz, xy), axis=None) of common.py:146.
 */
#ifndef RADARML_H
#define RADARML_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rml_status {
    RML_OK = 0,
    RML_ERR_INVALID = -1,      /* bad argument (NULL pointer, non-positive size, ...) */
    RML_ERR_UNSUPPORTED = -2,  /* shape / mode this build has no kernel for          */
    RML_ERR_HIP = -3,          /* a HIP runtime call failed (see rml_last_error)     */
    RML_ERR_NOMEM = -4,
    RML_ERR_STATE = -5         /* e.g. exact-integer path requested on a model that is not integer valued */
} rml_status;

typedef struct rml_ctx rml_ctx;
typedef struct rml_svm rml_svm;
typedef struct rml_linear rml_linear;

/* projection modes */
#define RML_MODE_MAX   0   /* BASELINE-named max-projection: xz=max_j V, yz=max_i V, xy=max_k V -- np.max, NaN policy included
                              (SURVEY 8 a-1'): a line that holds a NaN gives NaN (round 6: gfx950's IEEE-754-2019 maximum,
                              v_maximum3_f32, in every kernel family at the cost of the maxNum instruction it replaced; rounds 1-5
                              ignored NaNs here).  Radar magnitudes are integers 0..255 (common.py:30-31): the reference path never
                              meets one; tests/test_projection_gpu.py pins the behaviour of every kernel. */
#define RML_MODE_SLICE 1   /* reference-faithful plane slices through (i,j,k): predict.py:102-107       */
#define RML_MODE_SUM   2   /* sum-projection (the reductions of common.py:51-53), float32 accumulation  */
#define RML_MODE_MAX_NAN 3 /* = RML_MODE_MAX since round 6 (kept for callers of rounds 3-5, when NumPy's NaN policy was this opt-in
                              mode on an untuned kernel).
                              Non-finite rows and the SVM: a row with a NaN is off the code grid, so the asynchronous front doors
                              (rml_svm_decision, rml_project_svm) score it on the float64 path, whose RBF epilogue clamps the squared
                              distance with "d2 > 0 ? d2 : 0" -- the row's decision values are finite and meaningless; rows next to
                              it are untouched.  The reference raises instead (predict.py:60 -> sklearn validate_data): the
                              sklearn-protocol classes of radar-ml_amd/svm.py test their input rows and raise the same ValueError
                              (tests/test_svm_gpu.py::test_nan_row_through_the_svm_raises_like_scikit_learn); callers of the bare ABI
                              that may meet NaNs test the row flags / projections themselves. */

/* element type of the volumes */
#define RML_VOL_F32    0
#define RML_VOL_U8     1

/* projection mask bits, positional order of common.ProjMask (common.py:40) */
#define RML_MASK_XZ 1u
#define RML_MASK_YZ 2u
#define RML_MASK_XY 4u
#define RML_MASK_ALL 7u

/* kernel types of the SVC grid in train.py:474-476 */
#define RML_KERNEL_RBF    0
#define RML_KERNEL_LINEAR 1

/* GEMM path selection for rml_svm_decision */
#define RML_PATH_AUTO  0   /* exact-integer path where model and rows are on the code grid, else f64 */
#define RML_PATH_F32   1   /* v_mfma_f32_32x32x2_f32: opt-in, approximate (f32 accumulate, ~1e-4)     */
#define RML_PATH_I8    2   /* v_mfma_i32_32x32x32_i8 on u8 codes, exact int32 dot products            */
#define RML_PATH_F64   3   /* v_mfma_f64_16x16x4_f64 on widened float32 rows: libsvm-class accuracy   */
#define RML_PATH_DIGITS 4  /* general rows as four balanced int8 digits of a 32-bit fixed-point value: ten exact
                              digit-plane products on v_mfma_i32_32x32x32_i8 (|d(u.u)| ~ 1e-8); rows outside the
                              model's fixed-point range take RML_PATH_F64.  RML_PATH_AUTO picks it for large batches */

const char* rml_version(void);
const char* rml_last_error(void);

/* ---- context ------------------------------------------------------------------------- */
int rml_ctx_create(int device, rml_ctx** out);
int rml_ctx_destroy(rml_ctx* ctx);
int rml_ctx_device(const rml_ctx* ctx);

/* Context options (rml_ctx_set_option / rml_ctx_get_option).  The defaults are the tuned configuration and give the documented
 * results; every other value gives THE SAME RESULTS through another kernel family or schedule -- they exist for A/B measurements and
 * for the tests that pin one family against another.  (Until round 5 these were environment variables read inside the launch paths.)
 *   RML_OPT_PROJECT_SHARE_CU (0 / 1, default 0): the stand-alone projection entry points launch their persistent kernels the way
 *     the fused pipeline does beside its GEMM -- one workgroup per CU with a padded LDS request -- so that a kernel the caller runs on
 *     ANOTHER stream finds room on every CU.
 *   RML_OPT_WAVEFRAME (default 1): wave-per-frame projection kernels; 0 off, 2 quarter-plane buffers everywhere, 3 also for short rows
 *     stand-alone.          RML_OPT_LINPLANE (default 1): the linear-plane kernel for rows of 40 / 44 / 48 / 56 quads.
 *   RML_OPT_STAGE_CODES (default 1): per-wave LDS stage of the code rows.   RML_OPT_SLICE_WAVE (default 1): wave-per-row slice kernel.
 *   RML_OPT_DERIVE_FUSED (default 1): one-pass derive -> slice kernel (0: rml_derive_slice runs sum planes + top-k + slices, and
 *     rml_derive_project_svm returns RML_ERR_UNSUPPORTED).
 *   RML_OPT_CODE_RMW (default -1 = the measured rule, rml_code_rmw_default; 0 / 1 forced): read-compare-write code-row stores.
 *   RML_OPT_GEMM_BIG (default -1 = the whole-round rule; 0 never, 1 for every chunk of >= 256 rows): 256 x 256 ring GEMM.
 *   RML_OPT_CHUNK (default 0 = chosen per batch): rows per chunk of the chunked front doors (>= 128; rounded up to 128).
 *   RML_OPT_C1_PK (default 1): packed first-layer kernels of the SGAN branches.
 *   RML_OPT_SMO_LDS_ROWS (default RML_SMO_LDS_ROWS_MAX = 2 768, the 160 KB of a CU at 59 bytes per row): rml_smo_solve keeps the state
 *     of a dual of at most this many rows in LDS; larger duals run the same code on the workspace.  0: every dual on the workspace.
 *   RML_OPT_SGD_RESIDENT_D (default RML_SGD_RESIDENT_D_MAX = 10 240, ten elements per thread of a 1 024-thread workgroup):
 *     rml_sgd_solve and rml_sgd_online keep the weights of a problem of at most this many features in registers; wider rows run the same code with
 *     the weights on the workspace.  0: every problem on the workspace.  The results are the same bits either way.
 *   RML_OPT_CONV7 (default RML_CONV7_DEFAULT; bit 0: forward, bit 1: backward): which passes of the generator's output layer the callers
 *     of rml_conv7_tanh_* (nn_common.conv7_tanh) run on the hand-written kernels; a cleared bit sends that pass to the convolution library.
 *     The entry points themselves always run the kernels: the option is the caller's switch, kept here so that A/B runs share one knob.
 *   RML_OPT_ZOOM_ROWS (default 0): how the workgroups of k_zoom_rows (rml_project_zoom, rml_project_zoom_svm) share a row.  0: one
 *     workgroup per (row, plane) -- the measured choice; 1: one workgroup per row, the float64 images of its planes together in LDS
 *     (where they fit 150 KB); 2: one workgroup per row, one plane after the other.  The rows are the same bits in every mode.
 *   RML_OPT_SPARSE_ROWS (default -1): the 128 x 128 int8 GEMM of the fused pipelines stages operand lines (128 bytes of a code row)
 *     that hold nothing but the background code from one constant line instead of from the row, by the occupancy words the projection's
 *     code stage and rml_svm_load write.  -1: where the chunk's producer is a wave-per-frame max / sum projection of float32 volumes
 *     and the grid's z-rows fill whole 128-byte lines (Z a multiple or a divisor of 128: where it was measured to pay); 0: dense
 *     staging everywhere; 1: wherever the 128 x 128 kernel runs in rml_project_svm, and in place of the split-K kernel of small chunks
 *     (producers without the code stage get words of all ones).  The same bits either way: the operands that reach the matrix cores are identical.
 *   RML_OPT_SPARSE_STORES (default -1): the projection in front of a chunk whose int8 GEMM is the sparse kernel does not store the
 *     lines of a code row whose occupancy bit stays clear -- the GEMM never fetches them -- where the kernel writes the words itself
 *     and the line is a whole line of one plane (a set bit's line is always fully stored; the line that holds padding always is).
 *     Decided chunk by chunk: a chunk that takes the split-K, small, ring or float kernels keeps whole rows.  -1: where
 *     RML_OPT_SPARSE_ROWS' grid rule holds and the stores were measured to cost (csrc/rml_internal.h rml_sparse_stores); 0: whole
 *     rows everywhere; 1: wherever the chunk's plan is sparse and the kernel can skip.  The same bits either way. */
#define RML_OPT_PROJECT_SHARE_CU 1
#define RML_OPT_WAVEFRAME 2
#define RML_OPT_LINPLANE 3
#define RML_OPT_STAGE_CODES 4
#define RML_OPT_SLICE_WAVE 5
#define RML_OPT_DERIVE_FUSED 6
#define RML_OPT_CODE_RMW 7
#define RML_OPT_GEMM_BIG 8
#define RML_OPT_CHUNK 9
#define RML_OPT_C1_PK 10
#define RML_OPT_SMO_LDS_ROWS 11
#define RML_SMO_LDS_ROWS_MAX 2768
#define RML_OPT_SGD_RESIDENT_D 12
#define RML_SGD_RESIDENT_D_MAX 10240
#define RML_OPT_CONV7 13
#define RML_CONV7_DEFAULT 3
#define RML_OPT_ZOOM_ROWS 14
#define RML_OPT_SPARSE_ROWS 15
#define RML_OPT_SPARSE_STORES 16
int rml_ctx_set_option(rml_ctx* ctx, int option, int value);
int rml_ctx_get_option(const rml_ctx* ctx, int option, int* value);

/* The context's workspace (the chunk buffers of rml_project_svm / rml_svm_decision / rml_derive_targets ...) grows on demand: the
 * first call that needs more than any call before it allocates a bigger block with hipMalloc (the outgrown one is released once the
 * work queued before is done) -- a host-side allocation, not capturable into a HIP graph and possibly synchronising.  Every other
 * call is asynchronous on the caller's stream.  rml_ctx_reserve_workspace(ctx, bytes) does the growth up front (and releases
 * outgrown blocks; it synchronises the device); a warm-up call of the same shape does the same.  A call that would have to grow
 * the workspace while its stream is being captured fails with RML_ERR_INVALID and says so. */
int rml_ctx_reserve_workspace(rml_ctx* ctx, int64_t bytes);
int64_t rml_ctx_workspace_bytes(const rml_ctx* ctx);

/* In-situ timing of the projection launches issued by rml_project_svm (bench.py's roofline line):
 * while enabled, a hipEvent pair is recorded around every projection launch on the stream it is
 * launched on.  rml_profile_read synchronises, returns the number of launches, the summed
 * elapsed time and the frames they covered, and resets the counters. */
int rml_profile_enable(rml_ctx* ctx, int on);
int rml_profile_read(rml_ctx* ctx, int64_t* launches, double* total_ms, int64_t* frames);
/* The same for the GEMM + finish kernels of every chunk (the context's second stream): launches, summed
 * milliseconds, and the algorithmic operations 2*D*M per frame they covered. */
int rml_profile_read_gemm(rml_ctx* ctx, int64_t* launches, double* total_ms, double* ops);

/* What a pure streaming READ of `bytes` resident bytes reaches on this device, in GB/s: `reps` launches of a persistent
 * non-temporal 16-byte-load kernel over `buf` (16-byte aligned, >= 1 MiB), timed with a hipEvent pair on `stream`; synchronises.
 * bench.py's second roofline denominator beside the 8 TB/s specification (SURVEY.md 8d "measured copy bandwidth"); replaces no
 * reference interface -- the reference publishes no bandwidth figure. */
int rml_probe_stream(rml_ctx* ctx, const void* buf, int64_t bytes, int reps, double* gb_per_s, void* stream);

/* 1 when the fused pipelines store a frame's code row read-compare-write (read the old words, store what changed) for frames of
 * frame_bytes volume bytes and D codes, 0 for plain stores (the rule and its measurements: csrc/rml_internal.h rml_code_rmw;
 * RML_OPT_CODE_RMW overrides it per context).  Reporting only: bench.py prints it beside the with/without pair. */
int rml_code_rmw_default(int64_t D, int64_t frame_bytes, int derive, int u8);

/* Test hooks of RML_OPT_SPARSE_ROWS.  Occupancy words: one bit per 128-byte line of a code row, bit k & 31 of dword k >> 5, 1 unless
 * all 128 bytes are the background code (0x80) and the line lies wholly inside the D codes; ceil(ceil(D / 128) / 32) dwords per row.
 * rml_svm_sv_occupancy copies the model's words (M rounded up to 128 rows; the added rows are all occupied) to the HOST array `out`
 * (synchronises).  rml_project_occupancy is rml_project's code-row output (128-byte aligned rows, ld_q a multiple of 128) with the
 * rows' words into the device array occ[B][occ_words]: from the projection's own code stage where the kernel has one, all ones
 * elsewhere.  rml_project_sparse_rows is the same launch with RML_OPT_SPARSE_STORES' producer side (skip_clear != 0): a line whose
 * bit stays clear is left as feat_q held it where the kernel can skip it, every set bit's line is stored in full.
 * rml_ctx_sparse_gemm_launches: how many sparse GEMM launches the context has issued so far. */
int rml_svm_sv_occupancy(rml_ctx* ctx, const rml_svm* m, uint32_t* out, int64_t n_words);
int rml_project_occupancy(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode, float scale_div,
                          uint32_t mask, uint8_t* feat_q, int64_t ld_q, int32_t* row_isum, int64_t* row_isq, int32_t* row_flags,
                          uint32_t* occ, int occ_words, void* stream);
int rml_project_sparse_rows(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode, float scale_div,
                            uint32_t mask, uint8_t* feat_q, int64_t ld_q, int32_t* row_isum, int64_t* row_isq, int32_t* row_flags,
                            uint32_t* occ, int occ_words, int skip_clear, void* stream);
int64_t rml_ctx_sparse_gemm_launches(const rml_ctx* ctx);
/* how many projection launches the context has issued with skip_clear set on a kernel that writes its own occupancy words (and
 * therefore leaves clear lines unstored): the witness of RML_OPT_SPARSE_STORES' producer side */
int64_t rml_ctx_sparse_store_launches(const rml_ctx* ctx);

/* Feature-row length for a grid and mask: X*Z + Y*Z + X*Y over the selected planes
 * (train_svc.log:19 "Feature vector length: 10010" at (22,31,176)). */
int64_t rml_feature_len(int X, int Y, int Z, uint32_t mask);

/* ---- projection + feature assembly ---------------------------------------------------
 * Replaces, for a batch of B frames, the inline slicing of predict.py:102-107 /
 * ground_truth_samples.py:413-419 (mode SLICE), the max-projection named by
 * BASELINE.json (mode MAX) and the reductions of common.py:51-53 (mode SUM), followed by
 * common.process_samples at zoom 1 (common.py:141-148): mask-select, ravel, concatenate
 * in (xz,yz,xy) order, optional "/ RADAR_MAX" (scale_div = 255.0f; 0 or 1 = no scaling;
 * a true float32 division, bit-identical to NumPy's).
 *
 *   V        B*X*Y*Z float32
 *   ijk      B*3 int32 (mode SLICE only; negative indices wrap like Python's)
 *   feat     B*ld_feat float32 or NULL, row b at feat + b*ld_feat (ld_feat >= D)
 *   feat_q   B*ld_q uint8 or NULL: the same rows as integer codes c = value (before
 *            scaling), stored biased for the signed i8 MFMA (byte = c XOR 0x80 = int8 c-128),
 *            pad columns [D, ld_q) zeroed; valid for a row iff row_flags[b]==1.
 *            Needs ld_q % 4 == 0 and a 4-byte aligned base.
 *   row_isum / row_isq   B int32 / B int64 or NULL: sum c and sum c^2 of each code row
 *   row_flags            B int32 or NULL: 1 iff every selected value of the row is an
 *            integer in [0,255] (the exact-integer SVM path may then be used)
 */
int rml_project(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode,
                const int32_t* ijk, float scale_div, uint32_t mask,
                float* feat, int64_t ld_feat,
                uint8_t* feat_q, int64_t ld_q, int32_t* row_isum, int64_t* row_isq, int32_t* row_flags,
                void* stream);

/* Mode SLICE with T targets per frame: the reference classifies every target of one raw image
 * (`for target in targets:` over one `image`, predict.py:93-119; ground_truth_samples.py:366-440).  Row r = b*T + t of
 * every output is sliced from frame b at ijk[r] -- the volume is read once per target but never duplicated.
 *   ijk      B*T*3 int32;  feat / feat_q / row_* have B*T rows, otherwise as rml_project. */
int rml_project_slices(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int T,
                       const int32_t* ijk, float scale_div, uint32_t mask,
                       float* feat, int64_t ld_feat,
                       uint8_t* feat_q, int64_t ld_q, int32_t* row_isum, int64_t* row_isq, int32_t* row_flags,
                       void* stream);

/* The three planes as separate arrays (B,X,Z) (B,Y,Z) (B,X,Y); any may be NULL.
 * Same modes; no scaling.  (The tuple a reference caller packs at predict.py:113.) */
int rml_project_planes(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode,
                       const int32_t* ijk, float* xz, float* yz, float* xy, void* stream);

/* DerivedTarget.get_derived_targets, common.py:49-80, batched: the three energy
 * profiles (sum over the other two axes) and their top-num_targets indices, ascending
 * by value (argpartition(-n)[-n:] then argsort).  Ties: the LOWER index ranks lower.
 *   ijk      B*num_targets*3 int32   (t-th row = t-th entry of each of the three index lists,
 *                                     zipped as common.py:80)
 *   profiles B*(X+Y+Z) float32 or NULL: [s_theta | s_phi | s_r] per frame
 */
int rml_derive_targets(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                       int num_targets, int32_t* ijk, float* profiles, void* stream);

/* The reference-faithful path in ONE pass over the volumes: derive the num_targets strongest targets of every frame
 * (common.py:49-80, as rml_derive_targets) and slice the three planes through each of them (predict.py:98-107) into feature
 * rows -- what predict.py does per frame when the SDK reports no target and get_derived_targets stands in
 * (ground_truth_samples.py:357).  Row r = b*num_targets + t of every row output belongs to target t of frame b (ascending by
 * energy, like rml_derive_targets).  The frame is streamed once for the three energy profiles (no sum planes through HBM);
 * the planes of its targets are gathered right behind (4*D more bytes per target).
 *   ijk      B*num_targets*3 int32 or NULL (the derived indices, as rml_derive_targets writes them)
 *   profiles B*(X+Y+Z) float32 or NULL
 *   feat, feat_q, row_*   B*num_targets rows, as rml_project
 * Shapes without the fused kernel (rows that are not whole 16-byte quads, Z > 256, odd part of Z/4 above 15, a misaligned V)
 * run rml_derive_targets + rml_project_slices internally.  rml_derive_slice_supported: 1 when the one-pass kernel takes the
 * shape on this context (ctx may be NULL: default options; V may be NULL: alignment not checked). */
int rml_derive_slice(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int num_targets,
                     int32_t* ijk, float* profiles, float scale_div, uint32_t mask,
                     float* feat, int64_t ld_feat,
                     uint8_t* feat_q, int64_t ld_q, int32_t* row_isum, int64_t* row_isq, int32_t* row_flags,
                     void* stream);
int rml_derive_slice_supported(const rml_ctx* ctx, const void* V, int vdtype, int X, int Y, int Z, int num_targets);

/* Assemble feature rows from already separate projection planes (the list-of-tuples
 * input of common.process_samples, common.py:123-149, stacked per plane), zoom 1.
 * Planes are (B,X,Z),(B,Y,Z),(B,X,Y) float32; NULL for a masked-out plane. */
int rml_assemble_features(rml_ctx* ctx, const float* xz, const float* yz, const float* xy,
                          int64_t B, int X, int Y, int Z, float scale_div, uint32_t mask,
                          float* feat, int64_t ld_feat, void* stream);

/* common.process_samples with NON-UNIT zoom (common.py:141-148 when proj_zoom != 1; predict.py:34-54,109-116):
 * scipy.ndimage.zoom(p, zoom) with SciPy's defaults (order-3 spline, mode 'constant', prefilter) on every
 * selected plane, then ravel + concatenate + optional "/ RADAR_MAX".  out_shape (HOST, 6 ints: xz, yz, xy as
 * (rows, cols)) is round(in * zoom) evaluated by the caller with Python's round().  Planes as in
 * rml_assemble_features; feat rows have D = sum of the selected output planes. */
int rml_zoom_features(rml_ctx* ctx, const float* xz, const float* yz, const float* xy,
                      int64_t B, int X, int Y, int Z, const int32_t* out_shape,
                      float scale_div, uint32_t mask, float* feat, int64_t ld_feat, void* stream);

/* Volumes from a radar arena that differs from the training arena -> feature rows at the MODEL's geometry, on the device:
 * the body of predict.py:98-116 for B frames at once -- the projections (predict.py:102-107, or mode MAX), calc_proj_zoom's
 * factors (predict.py:34-54,109-111) applied by common.process_samples (common.py:141-148: scipy.ndimage.zoom per plane, ravel,
 * concatenate, optional "/ RADAR_MAX").  The projection runs at the source grid X x Y x Z into a chunk of the context's
 * workspace (float32 rows; uint8 volumes: code rows, a quarter of the bytes), k_zoom_rows resamples every row to out_shape
 * (HOST, 6 ints as in rml_zoom_features) -- the arithmetic of rml_zoom_features, bit for bit.  No host synchronisation.
 *   mode   as rml_project; RML_MODE_SLICE with ijk NULL derives the T strongest targets of every frame at the source grid
 *   ijk    B*T*3 int32 (frame-major) or NULL;  T targets per frame (1 unless mode is RML_MODE_SLICE)
 *   feat   B*T rows of D = sum of the selected output planes, stride ld_feat >= D
 * RML_ERR_UNSUPPORTED: a selected plane whose float64 image exceeds 150 KB (the LDS-resident spline filter), as rml_zoom_features. */
int rml_project_zoom(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode, const int32_t* ijk, int T,
                     const int32_t* out_shape, float scale_div, uint32_t mask, float* feat, int64_t ld_feat, void* stream);

/* Quantise float32 feature rows to uint8 codes + row stats, for callers that bring (N,D)
 * features instead of volumes.  A value v is on the code grid iff it is bit-identical to
 * float32(c / scale_div) for an integer c in [0,255] (scale_div = 255: the "p / 255." of
 * train.py:667; scale_div <= 1: v == c).  flags as in rml_project. */
int rml_quantize_rows(rml_ctx* ctx, const float* feat, int64_t N, int64_t D, int64_t ld_feat,
                      float scale_div, uint8_t* feat_q, int64_t ld_q,
                      int32_t* row_isum, int64_t* row_isq, int32_t* row_flags, void* stream);

/* ---- RBF / linear SVC (libsvm C-SVC, one-vs-one) ------------------------------------------
 * rml_svm_load ingests the arrays of a fitted sklearn SVC (HOST pointers, float64, the
 * private libsvm-order attributes): support_vectors_ (M,D), _dual_coef_ (C-1,M),
 * _intercept_ (P=C(C-1)/2), _n_support (C), _gamma; optional sigmoid calibrators
 * a_, b_ (C each) of CalibratedClassifierCV (train.py:722-724).  It builds the device
 * copies both GEMM paths need (float32 centred SVs + norms; uint8 codes when every SV
 * is an integer multiple of 1/code_scale).
 */
int rml_svm_load(rml_ctx* ctx, const double* sv, int64_t M, int64_t D,
                 const double* dual_coef, const double* intercept, const int32_t* n_support,
                 int n_classes, int kernel, double gamma, double code_scale /* e.g. 255, or 1 */,
                 const double* calib_a, const double* calib_b, rml_svm** out);
int rml_svm_free(rml_ctx* ctx, rml_svm* m);
int rml_svm_is_exact(const rml_svm* m);   /* 1 when the uint8-code path is available */
int64_t rml_svm_num_sv(const rml_svm* m);
int64_t rml_svm_dim(const rml_svm* m);

/* SVC.decision_function / SVC.predict / CalibratedClassifierCV.predict_proba / .predict
 * (train.py:217,723-724; predict.py:60) for N feature rows:
 *   sk:svm/src/libsvm/svm.cpp:461-475,514  K = exp(-gamma * ||x - sv||^2)
 *   sk:svm/src/libsvm/svm.cpp:2864-2890    dec[p] = sum coef*K - rho[p]; vote
 *   sk:utils/multiclass.py:542-584         ovr = votes + s/(3(|s|+1))
 *   sk:calibration.py:727-784,928-942      expit(-(a*T+b)), normalise, argmax
 * Inputs: either feat (float32 rows, general path) or feat_q (+row stats, exact path).
 * Outputs (any may be NULL): dec_ovo N*P f64, dec_ovr N*C f64, proba N*C f64,
 * label_vote N int32 (class index of SVC.predict), label_calib N int32 (class index of
 * the calibrated predict; requires calibrators).
 */
int rml_svm_decision(rml_ctx* ctx, const rml_svm* m, int path,
                     const float* feat, int64_t ld_feat,
                     const uint8_t* feat_q, int64_t ld_q, const int32_t* row_isum, const int64_t* row_isq,
                     const int32_t* row_flags,
                     int64_t N,
                     double* dec_ovo, double* dec_ovr, double* proba,
                     int32_t* label_vote, int32_t* label_calib, void* stream);

/* SVC(probability=True).predict_proba (the estimator train.py:478 constructs): libsvm's Platt sigmoid on every
 * pair value followed by pairwise coupling (sk:svm/src/libsvm/svm.cpp:2032-2104, 2918-2952).
 * rml_svm_set_platt: probA/probB HOST, P values each (SVC._probA / _probB); copied to the device once, at load time
 * (synchronous, like rml_svm_load).  rml_svm_pairwise_proba: dec_ovo DEVICE N*P libsvm pair values (dec_ovo of
 * rml_svm_decision); proba DEVICE N*C; an ordinary asynchronous launch on `stream`; RML_ERR_STATE when the model has
 * no Platt coefficients. */
int rml_svm_set_platt(rml_ctx* ctx, rml_svm* m, const double* probA, const double* probB);
int rml_svm_pairwise_proba(rml_ctx* ctx, const rml_svm* m, const double* dec_ovo, int64_t N, double* proba, void* stream);

/* ---- training-time augmentation ---------------------------------------------------------------
 * train.DataGenerator (train.py:84-185) on the GPU, one batch of equally shaped projection planes per call:
 *   RML_AUG_ROTATE  scipy.ndimage.rotate(p, angle, reshape=False) + clamp to [0,1] (train.py:87-94); params: 6 doubles per
 *                   plane, the affine map of ndimage.rotate: m00 m01 m10 m11 off0 off1 with
 *                   [[c, s], [-s, c]], offset = centre - M centre, c/s = cos/sin of the angle in degrees
 *   RML_AUG_ZOOM    clipped_zoom(p, f) + clamp (train.py:96-144); params: 1 double per plane, the zoom factor
 *   RML_AUG_NOISE   sparse_noise: ONE draw per plane added to its non-zero entries + clamp (train.py:146-154); params:
 *                   1 double per plane, the draw
 * src, dst: DEVICE B*H*W float32 (may not alias); params: DEVICE.  The random draws are the caller's (the Python mirror
 * makes them in the reference's order from the reference's generators). */
#define RML_AUG_ROTATE 0
#define RML_AUG_ZOOM   1
#define RML_AUG_NOISE  2
int rml_augment(rml_ctx* ctx, int op, const float* src, int64_t B, int H, int W, const double* params, float* dst, void* stream);

/* The augmentation chain of the network trainers (dnn.py:94-182 augment_data; sgan.py:238-326 is the same function) with the
 * scaling of preprocess_data (dnn.py:202-205) in front, ONE launch for B equally shaped planes; per plane, in this order:
 *   scaling           v = (p - sub) / div in float32 when div != 0 (sub = div = 127.5: [0, 255] -> [-1, 1]); div == 0: v = p
 *   RML_CHAIN_ROTATE  scipy.ndimage.rotate(v, angle, reshape=False) (order 3, mode 'constant', cval 0, float64 prefilter), clamp
 *   RML_CHAIN_ZOOM    clipped_zoom(v, factor) (centre paste below 1, centre crop + trim above 1, the input itself at 1), clamp
 *   RML_CHAIN_NOISE   v += draw on EVERY entry (dnn.py:160; train.py's sparse noise of rml_augment is another function), clamp
 * Each stage of the mask `stages` works on the previous one's result; the clamp is to [lo, hi] ([-1, 1] in the reference) and lets
 * NaN pass; stages == 0 is the scaling alone.  Unlike rml_augment the planes between the stages never leave the workgroup.
 * src: DEVICE, plane b at src + b * in_stride floats (in_stride >= H*W); dst: DEVICE B*H*W float32, dense; may not alias.
 * params: DEVICE 8 doubles per plane: m00 m01 m10 m11 off0 off1 (the affine map of ndimage.rotate, see RML_AUG_ROTATE), the zoom
 * factor, the noise draw -- all eight slots are there whatever `stages` is; NULL only with stages == 0.  A zoom factor outside
 * [1/1024, 1024] (or NaN) has no region to resample and gives a zero plane.  The random draws are the caller's.
 * RML_ERR_UNSUPPORTED: a plane whose float32 copy and float64 coefficient image (12 bytes per pixel, 4 without a spline stage)
 * exceed the 150 KB of LDS that rml_augment allows, too.  B == 0 is a no-op.  Follow it with rml_resize_bicubic(div = 0). */
#define RML_CHAIN_ROTATE 1
#define RML_CHAIN_ZOOM   2
#define RML_CHAIN_NOISE  4
int rml_augment_chain(rml_ctx* ctx, int stages, const float* src, int64_t in_stride, int64_t B, int H, int W, float sub, float div,
                      float lo, float hi, const double* params, float* dst, void* stream);

/* Kernel values against the model's support vectors, K[n][m] = k(x_n, sv_m) for m < M, float64, exact to the
 * same arithmetic as rml_svm_decision (path AUTO / I8 / F64).  With the training rows loaded as the "support vectors"
 * of a model (any coefficients) this is the Gram matrix sklearn's SVC(kernel='precomputed') is fitted on and
 * K(test, train) it predicts with -- the rbf evaluations libsvm would otherwise do one pair at a time
 * (train.py:462-491 grid search).  kmat: N x ld_k doubles, ld_k >= M. */
int rml_svm_kernel_matrix(rml_ctx* ctx, const rml_svm* m, int path, const float* feat, int64_t ld_feat, int64_t N,
                          double* kmat, int64_t ld_k, void* stream);

/* Kernel matrices of ONE set of rows against itself, every requested kernel from one pass over the inner products
 * (the Gram service of an SVC grid search with kernel='precomputed'):
 *   RML_GRAM_LINEAR  K[i][j] = x_i . x_j
 *   RML_GRAM_RBF     K[i][j] = exp(-gamma_k * (x_i.x_i + x_j.x_j - 2 x_i.x_j))   (libsvm's formula, no clamp)
 * float64 products and sums of the float32 rows.  feat: DEVICE N x ld_feat float32.  kinds / gammas: HOST, nk entries
 * (gamma ignored for LINEAR; otherwise finite and >= 0), 1 <= nk <= 8.  out: DEVICE; matrix k at out + k * stride_k, row i at
 * + i * ld_out (ld_out >= N, stride_k >= N * ld_out); only [0,N) x [0,N) of each is written.  Every matrix is bit-exactly
 * symmetric.  Deterministic run to run.  N == 0 is a no-op.  Uses the context's workspace; asynchronous on `stream`. */
#define RML_GRAM_LINEAR 0
#define RML_GRAM_RBF    1
int rml_gram(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int64_t D,
             int nk, const int* kinds, const double* gammas,
             double* out, int64_t ld_out, int64_t stride_k, void* stream);

/* The same service for a search over projection masks: a row is the concatenation of `nseg` column segments (the reference's
 * xz, yz, xy projections), and the inner products and squared norms of any union of segments are the sums of the segments' own.
 * rml_gram_segments forms, in ONE pass over the rows, the float64 inner products G_s and squared row norms of every segment
 * (rml_gram's arithmetic: float32 rows, exact products, float64 accumulation in ascending k within the segment).
 *   feat: DEVICE N x ld_feat float32.  seg_len: HOST, nseg positive lengths, 1 <= nseg <= 8, sum <= ld_feat; segment s is the
 *   columns [sum_{t<s} seg_len[t], + seg_len[s]).  Columns past the last segment are never read.
 *   G: DEVICE; G_s at G + s * stride_s, row i at + i * ld_g (ld_g >= N, stride_s >= N * ld_g); only [0,N) x [0,N) is written.
 *   nsq: DEVICE, nseg * N doubles: the squared norm of segment s of row i at nsq[s * N + i].
 * Every G_s is bit-exactly symmetric.  Uses the context's workspace.
 * rml_gram_compose writes n_out kernel matrices from them (HOST arrays of n_out >= 1 entries, any number): output k is the
 * kernel kinds[k] / gammas[k] (as rml_gram: gamma ignored for LINEAR, otherwise finite and >= 0) of the columns of mask
 * seg_bits[k], a non-zero subset of the nseg segments (bit s = segment s).  With g = sum G_s[i][j] and n_i = sum nsq[s * N + i]
 * over the set bits in ascending s: d2 = (n_i + n_j) - 2 g, K = g (LINEAR) or exp(-gamma_k * d2) (RBF).  The sums associate by
 * segment, so an output is not the bits of rml_gram on the column subset; it obeys the same error bound.  out: matrix k at
 * out + k * stride_k, row i at + i * ld_out (ld_out >= N, stride_k >= N * ld_out).  Every output is bit-exactly symmetric (what
 * rml_smo_solve requires).  Both calls: deterministic run to run, N == 0 is a no-op, asynchronous on `stream`, no environment
 * variable read. */
int rml_gram_segments(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int nseg, const int64_t* seg_len,
                      double* G, int64_t ld_g, int64_t stride_s, double* nsq, void* stream);
int rml_gram_compose(rml_ctx* ctx, const double* G, int64_t ld_g, int64_t stride_s, const double* nsq, int64_t N, int nseg,
                     int n_out, const int* seg_bits, const int* kinds, const double* gammas,
                     double* out, int64_t ld_out, int64_t stride_k, void* stream);

/* ---- SVC duals of a grid search on the device ---------------------------------------------------------------------
 * rml_smo_solve: a batch of independent binary C-SVC duals (one per grid point x fold x class pair), each solved by one
 * workgroup running libsvm's Solver::Solve as scikit-learn ships it (sklearn/svm/src/libsvm/svm.cpp: Solver, lines
 * ~560-1160 -- select_working_set 833-932, do_shrinking 969-1031, reconstruct_gradient 662-709, calculate_rho 1033-1075 --
 * and SVC_Q, ~1423-1470) on Gram matrices in the layout rml_gram writes.  It replaces the host libsvm fits of
 * GridSearchCV(SVC) at train.py:462-491.  Working-set ties, the Qfloat rounding of kernel rows, shrinking with its position
 * permutation, the gradient reconstruction order and the un-fused double arithmetic are libsvm's: on the same matrix n_iter,
 * alpha and rho are the bits of SVC(kernel='precomputed').fit (n_iter_, |dual_coef_|, -intercept_ up to scikit-learn's
 * sign flip of binary models).  The matrices must be bit-exactly symmetric.
 *   gram: DEVICE; matrix k at gram + k * stride_k, row i at + i * ld (ld >= N, stride_k >= N * ld), k < n_mats.
 *   probs: HOST, n_probs descriptors.  rows: DEVICE int32, n_rows_total entries in [0, N): problem p reads its l Gram rows at
 *   rows + rows_off in libsvm's order -- the rows of class i (y = +1, the first n_pos) in original order, then those of class
 *   j (y = -1); problems may share a row list.  Per-row C is Cp for y = +1 and Cn for y = -1 (libsvm's weighted C); eps is
 *   SVC's tol; max_iter -1 = no limit.
 *   Outputs, DEVICE: alpha (n_alpha_total doubles; problem p writes l of them at alpha_off, in the order of its row list),
 *   rho, n_iter, stopped (n_probs each; stopped: 1 = max_iter reached, 0 = converged, -1 = a row index outside [0, N): that
 *   problem is not solved and its alpha is 0).
 * rml_smo_score: libsvm's svm_predict_values + vote (svm.cpp ~2842-2900, SVC.predict on K[test, train]) for n_fits models
 * of n_classes (2..8) classes.  Fit f is made of the n_classes (n_classes - 1) / 2 consecutive problems prob0 .. in libsvm's
 * pair order (0,1), (0,2), .., (1,2), .., all on one matrix; its held-out Gram rows are test_rows + test_off (DEVICE int32,
 * n_test entries), their true class indices test_y + test_off.  Per (row, pair) the decision value is the sequential sum of
 * coef * K[row][sv] over the pair's rows with alpha > 0 (class i then class j, coef = +alpha / -alpha) minus rho -- libsvm's
 * order, so the values are its bits.  Outputs, DEVICE: dec (n_test_total x pairs doubles, row-major per fit at
 * test_off * pairs), labels (n_test_total int32 class indices: dec > 0 votes i, first maximum wins), correct (n_fits int32:
 * labels equal to test_y).  Row indices are checked on the device as in rml_smo_solve: a held-out row, or a row with
 * alpha > 0, outside [0, N) is not read -- its decision values are NaN and the row's label is -1 (never counted correct).
 * Both calls use the context's workspace, are asynchronous on `stream` and read no environment variable. */
typedef struct rml_smo_problem {
    int32_t matrix;             /* which Gram matrix */
    int32_t l;                  /* rows of the dual */
    int32_t n_pos;              /* the first n_pos rows have y = +1 */
    int32_t shrinking;          /* SVC(shrinking=...) */
    int32_t max_iter;           /* SVC(max_iter=...), -1: no limit */
    int32_t reserved;
    int64_t rows_off;           /* into `rows` */
    int64_t alpha_off;          /* into `alpha` */
    double Cp, Cn, eps;
} rml_smo_problem;
typedef struct rml_smo_fit {
    int32_t prob0;              /* first of the fit's pair problems */
    int32_t n_test;             /* held-out rows */
    int64_t test_off;           /* into test_rows / test_y / labels; dec at test_off * pairs */
} rml_smo_fit;
int rml_smo_solve(rml_ctx* ctx, const double* gram, int64_t N, int64_t ld, int64_t stride_k, int n_mats,
                  const rml_smo_problem* probs, int64_t n_probs, const int32_t* rows, int64_t n_rows_total,
                  double* alpha, int64_t n_alpha_total, double* rho, int32_t* n_iter, int32_t* stopped, void* stream);
int rml_smo_score(rml_ctx* ctx, const double* gram, int64_t N, int64_t ld, int64_t stride_k, int n_mats,
                  const rml_smo_problem* probs, int64_t n_probs, const int32_t* rows, int64_t n_rows_total,
                  const double* alpha, int64_t n_alpha_total, const double* rho, int n_classes,
                  const rml_smo_fit* fits, int64_t n_fits, const int32_t* test_rows, const int32_t* test_y,
                  int64_t n_test_total, double* dec, int32_t* labels, int32_t* correct, void* stream);

/* ---- SGDClassifier fits on the device ---------------------------------------------------------------------------------
 * rml_sgd_solve: a batch of independent binary logistic-regression problems (one per grid point x fold x class of a
 * one-vs-rest SGDClassifier), each solved by one workgroup running scikit-learn 1.7.2's _plain_sgd64
 * (sklearn/linear_model/_sgd_fast.pyx.tp:275-603) for loss='log_loss', learning_rate='optimal', dense rows, with its
 * WeightVector (sklearn/utils/_weight_vector.pyx.tp), its shuffle (sklearn/utils/_seq_dataset.pyx.tp:137-145 on the
 * generator of sklearn/utils/_random.pxd:20-34), the half-binomial loss on labels 0 / 1 (sklearn/_loss/_loss.pyx.tp:256-266,
 * 686-725) and the cumulative L1 penalty (_sgd_fast.pyx.tp:631-659).  It replaces the host fits of
 * GridSearchCV(SGDClassifier(loss='log')) at train.py:350-381 and the partial_fit of train.py:432.  Every expression outside the
 * dot product w . x is scikit-learn's, un-fused and in its order.  The dot product is summed in this order:
 *   thread t of 1 024 owns the elements t, t + 1024, ..; it adds its products w[e] * (double)x[e] in ascending order from 0;
 *   the 64 threads of a wave (64 v .. 64 v + 63) combine by a butterfly, s += s of lane ^ m for m = 32, 16, 8, 4, 2, 1;
 *   the 16 wave sums are added in wave order, ((S0 + S1) + S2) + .. + S15.
 * A problem's result does not depend on its place in the batch, on the batch, or on RML_OPT_SGD_RESIDENT_D, and is the same
 * bits run to run.
 *   X: DEVICE float32, row i at X + i * ld (ld >= D), N rows (converted to double exactly, as X.astype(float64)).
 *   probs: HOST, n_probs descriptors.  rows: DEVICE int32, n_rows_total entries in [0, N): problem p trains on the n rows at
 *   rows + rows_off, in that order (the dataset's initial order), with the labels (0 / 1) at y + y_off (DEVICE int32,
 *   n_y_total entries); problems may share either list.  n <= RML_SGD_MAX_ROWS.  seed is the shuffle seed fit_binary draws
 *   (the shuffle runs before every epoch with the same seed on the persisting order, so the permutations compound).
 *   average: 0, or the iteration at which averaging starts.  tol: -INFINITY for tol=None.  t0: 1.0 for a fresh fit.  warm != 0:
 *   the outputs of slot `out` hold the initial coef / avg_coef / intercept / avg_intercept (partial_fit: t0 = est.t_).
 *   Outputs, DEVICE, indexed by the problem's slot `out` < n_out: coef and avg_coef (D doubles at out * D: the standard and the
 *   averaged weights; avg_coef is written only where average > 0), intercept, avg_intercept, n_iter (epochs run), t
 *   (t0 + n_iter * n, as est.t_), status: 0 converged, 1 max_iter reached, 2 non-finite weights (where scikit-learn raises its
 *   "Floating-point under-/overflow" ValueError), -1 a row index outside [0, N): that problem is not run and its other
 *   outputs are untouched.
 * rml_sgd_score: SGDClassifier.predict for n_fits fits of n_classes (2..8) classes.  Fit f is made of the n_classes consecutive
 * problems prob0 .. (class order), or of ONE problem when n_classes == 2 (class 1 positive).  Per held-out row (test_rows +
 * test_off, DEVICE int32; true class indices test_y + test_off) and class, dec = coef . x + intercept in the dot order above;
 * the coefficients are the averaged ones where average > 0 and average <= t - 1 with t the largest t of the fit's problems, as
 * SGDClassifier chooses.  The label is the first maximum over the classes, or dec > 0 for two classes.  It reads the outputs
 * of rml_sgd_solve where they are.  Outputs, DEVICE: dec (n_test_total x n_dec doubles, n_dec = 1 for two classes, row-major
 * per fit at test_off * n_dec), labels (n_test_total int32), correct (n_fits int32).  A held-out row outside [0, N) is not
 * read: its values are NaN and its label -1.
 * rml_sgd_shuffle: HOST helper, one call of SequentialDataset.shuffle(seed) on perm_inout (n int32), no device, no context.
 * The two device calls use the context's workspace, are asynchronous on `stream` and read no environment variable. */
#define RML_SGD_L1 1
#define RML_SGD_L2 2
#define RML_SGD_ELASTICNET 3
#define RML_SGD_MAX_ROWS 8192
typedef struct rml_sgd_problem {
    int32_t n;                  /* training rows */
    int32_t penalty;            /* RML_SGD_L1 / L2 / ELASTICNET */
    int32_t average;            /* 0, or the iteration at which averaging starts */
    int32_t max_iter;
    int32_t n_iter_no_change;
    int32_t shuffle;
    uint32_t seed;              /* the shuffle seed */
    int32_t warm;               /* the outputs hold the initial state */
    int64_t rows_off;           /* into `rows` */
    int64_t y_off;              /* into `y` */
    int64_t out;                /* output slot: coef / avg_coef at out * D, the scalars at out */
    double alpha, l1_ratio, tol, weight_pos, weight_neg, t0;
} rml_sgd_problem;
typedef struct rml_sgd_fit {
    int32_t prob0;              /* first of the fit's class problems */
    int32_t n_test;             /* held-out rows */
    int64_t test_off;           /* into test_rows / test_y / labels; dec at test_off * n_dec */
} rml_sgd_fit;
int rml_sgd_solve(rml_ctx* ctx, const float* X, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int64_t n_probs,
                  const int32_t* rows, int64_t n_rows_total, const int32_t* y, int64_t n_y_total, int64_t n_out, double* coef,
                  double* avg_coef, double* intercept, double* avg_intercept, int32_t* n_iter, double* t, int32_t* status,
                  void* stream);
int rml_sgd_score(rml_ctx* ctx, const float* X, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int64_t n_probs,
                  int64_t n_out, const double* coef, const double* avg_coef, const double* intercept, const double* avg_intercept,
                  const double* t, int n_classes, const rml_sgd_fit* fits, int64_t n_fits, const int32_t* test_rows,
                  const int32_t* test_y, int64_t n_test_total, double* dec, int32_t* labels, int32_t* correct, void* stream);
int rml_sgd_shuffle(uint32_t seed, int64_t n, int32_t* perm_inout);

/* ---- a chain of SGDClassifier.partial_fit calls on the device (train.py:409-416, 418-438) ------------------------------
 * rml_sgd_online: n_steps partial_fit calls of ONE SGDClassifier of n_classes (2..8) classes on resident rows, each followed,
 * where its step asks for it, by predict on the held-out rows, as ONE asynchronous call on `stream`: one persistent
 * workgroup per class problem (k_sgd_online) that keeps the weights where rml_sgd_solve keeps them for all the steps, then
 * k_sgd_online_finish for the labels and counts.  No device synchronisation, no environment variable; it uses the context's
 * workspace and can be captured like rml_sgd_solve.
 *   X, N, D, ld: as for rml_sgd_solve.  probs: HOST, K descriptors, K = n_classes (class order), or ONE when n_classes == 2
 *   (class 1 positive): penalty, average, shuffle, alpha, l1_ratio, weight_pos / weight_neg, the output slot `out` (distinct),
 *   warm, and t0 = est.t_ before the first step; penalty, average, t0 and warm are the same for all K.  n, seed, rows_off,
 *   y_off, max_iter, tol and n_iter_no_change are ignored: a partial_fit call is exactly one epoch and cannot stop early.
 *   steps: HOST, n_steps records.  Step s trains on the n rows at rows + off (DEVICE int32, n_rows_total entries in [0, N), in
 *   the order the partial_fit call would see them) with the class indices at cls + off (DEVICE int32, same offsets): the
 *   problem of class c has the label 1 where cls == c.  Steps may share or overlap ranges.  seed[k]: the shuffle seed of
 *   problem k for this call (scikit-learn draws them per call).  score != 0: the held-out rows are scored after the step.
 *   test_rows / test_y: DEVICE int32, n_test >= 0 held-out rows and their class indices (no step is scored when n_test == 0).
 * Per step and problem: one epoch of _plain_sgd64 from the state the previous step left, with everything a fresh _plain_sgd
 * call starts anew started anew: the index array 0 .. n-1 and ONE shuffle with the step's seed, wscale = 1, the cumulative L1
 * penalty u and q = 0, average_a = 0, average_b = 1; the epoch ends with reset_wscale; t advances by n.  The arithmetic and the
 * dot order are rml_sgd_solve's.  Between steps the intercepts follow the statements of _fit_binary / _fit_multiclass
 * (sklearn/linear_model/_stochastic_gradient.py:753-768, 807-823) with what their aliasing does.  Per problem k the call
 * keeps SI[k] (_standard_intercept), AI[k] (_average_intercept) and, per estimator, the flag A ("intercept_ is
 * _average_intercept").  A step starts problem k from (SI[k], AI[k]) and yields (icpt, aicpt).  With average > 0,
 * AI[k] = aicpt.  Then, for more than two classes: icpt goes to AI[k] if A was set before the step, else to SI[k] (the
 * former overwrites the averaged intercept and leaves SI stale, as scikit-learn does), and A = average > 0 && average <= t - 1.
 * For two classes: if average > 0 && average <= t - 1, A is set and SI stays; else SI[0] = icpt and A is cleared.  coef_ /
 * intercept_ are the averaged arrays iff A, and a scored step uses exactly that view: dec[r][c] = coef_[c] . x_r +
 * intercept_[c] in rml_sgd_score's dot order, the label the first maximum (dec > 0 for two classes).
 *   In and out, DEVICE, per slot `out` < n_out as rml_sgd_solve leaves them: coef, avg_coef (D doubles at out * D; avg_coef only
 *   where average > 0), intercept = SI, avg_intercept = AI, and avg_flag (ONE int32: A); read where warm != 0 (else the state
 *   starts at zero and A clear).  The weights are written once, at the end of the call.  A call split in two (steps 0..j, then
 *   j..n_steps with t0 = t, warm = 1 and the state and flag the first left) gives the bits of the one call.
 *   Out, DEVICE: t (per slot: t0 + the rows of the steps run), status (per slot: 1 all steps run, 2 non-finite weights, -1),
 *   fail_step (ONE int32: the first step at which a problem went non-finite, else -1), correct (n_steps int32: the held-out
 *   rows labelled as test_y says after step s; -1 for a step that was not scored), labels (n_test int32) and dec (n_test x
 *   n_dec doubles, n_dec = 1 for two classes) of the last scored step.
 * A row index outside [0, N), in any step or in test_rows, is found before anything is written: status -1 in every
 * problem's slot, every other output untouched.  If a problem's weights go non-finite at step s (scikit-learn raises
 * there): its status is 2, fail_step = s, correct[s ..] = -1, labels / dec are those of the last scored step before s; the
 * other problems stop at the first step boundary after s at which they see it (they never wait for each other), so their
 * weights are then those of some step >= s: the estimator is to be discarded, as after scikit-learn's exception. */
typedef struct rml_sgd_step {
    int64_t off;                /* into `rows` and `cls` */
    int32_t n;                  /* rows of this partial_fit call, 1 .. RML_SGD_MAX_ROWS */
    int32_t score;              /* != 0: predict on the held-out rows after this step */
    uint32_t seed[8];           /* the shuffle seed of each class problem for this call */
} rml_sgd_step;
int rml_sgd_online(rml_ctx* ctx, const float* X, int64_t N, int64_t D, int64_t ld, const rml_sgd_problem* probs, int n_classes,
                   const rml_sgd_step* steps, int64_t n_steps, const int32_t* rows, const int32_t* cls, int64_t n_rows_total,
                   const int32_t* test_rows, const int32_t* test_y, int64_t n_test, int64_t n_out, double* coef, double* avg_coef,
                   double* intercept, double* avg_intercept, double* t, int32_t* avg_flag, int32_t* status, int32_t* fail_step,
                   int32_t* correct, int32_t* labels, double* dec, void* stream);

/* ---- the host-side steps of SVC(probability=True).fit -------------------------------------------------------------------
 * libsvm's svm_train with probability = 1 runs, per class pair, svm_binary_svc_probability (scikit-learn 1.7.2,
 * sklearn/svm/src/libsvm/svm.cpp:2107-2203) before the pair's own dual: the pair's rows shuffled, five folds of sub-duals
 * (rml_smo_solve / rml_smo_score take them as ordinary problems), and sigmoid_train on the held-out decision values.  The
 * two functions below are the steps around those duals.  They use no device and no context, and are thread-safe.
 * rml_libsvm_shuffle: perm (HOST, l int32) = the Fisher-Yates pass of svm.cpp:2117-2122 over 0 .. l-1, drawn from a
 * std::mt19937 freshly seeded with `seed` through the Lemire post-processor of sklearn/svm/src/newrand/newrand.h:21-53.
 * (The generator IS freshly seeded for every pair: each inner svm_train re-seeds it, svm.cpp:2373-2376.)
 * rml_platt_fit: A, B = sigmoid_train(l, dec, y) of svm.cpp:1919-2030 -- the same operation order and constants, libm's exp /
 * log, no fused multiply-add -- so that they are SVC.probA_ / probB_ bit for bit.  dec, y: HOST, l doubles (y > 0: the
 * pair's first class).  info (may be NULL): RML_PLATT_OK, or which of libsvm's two messages it would have printed. */
#define RML_PLATT_OK 0
#define RML_PLATT_LINE_SEARCH_FAILED 1
#define RML_PLATT_MAX_ITER 2
int rml_libsvm_shuffle(uint32_t seed, int64_t l, int32_t* perm);
int rml_platt_fit(const double* dec, const double* y, int64_t l, double* A, double* B, int* info);

/* Fused front door: volumes -> projection (mode, mask fixed at load: D must match) ->
 * SVM outputs, features never returned to the caller.  Workspace is owned by the ctx and
 * grows on demand. */
int rml_project_svm(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                    int mode, const int32_t* ijk, float scale_div, uint32_t mask,
                    double* dec_ovo, double* dec_ovr, double* proba,
                    int32_t* label_vote, int32_t* label_calib, void* stream);

/* The same front door for the reference-faithful projection with DERIVED targets: per frame the strongest derived target
 * (common.py:49-80, num_targets = 1), the three slices through it (predict.py:98-107) and the SVM outputs, the frame read once
 * (+ 4*D bytes for the slices).  ijk_out: B*3 int32 or NULL (the derived indices).  RML_ERR_UNSUPPORTED when
 * rml_derive_slice_supported(ctx, V, ...) is 0: call rml_derive_targets and rml_project_svm(RML_MODE_SLICE, ijk) then. */
int rml_derive_project_svm(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                           float scale_div, uint32_t mask, int32_t* ijk_out,
                           double* dec_ovo, double* dec_ovr, double* proba,
                           int32_t* label_vote, int32_t* label_calib, void* stream);

/* The front door for a recording from a foreign arena (predict.py:98-119 with calc_proj_zoom != 1, predict.py:34-54): projection
 * at the source grid X x Y x Z, the zoom of rml_project_zoom to out_shape (the selected output planes must sum to the model's D:
 * RML_ERR_INVALID otherwise), the SVM of rml_svm_decision on the zoomed rows -- off the code grid: the float64 kernel, or the
 * multi-digit int8 kernel for batches that fill it, as RML_PATH_AUTO picks for float rows.  One target per frame; mode
 * RML_MODE_SLICE with ijk NULL derives it at the source grid.  Chunked like rml_project_svm (the GEMM of a chunk beside the
 * projection and zoom of the next); at most 128 frames run on the caller's stream alone. */
int rml_project_zoom_svm(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                         int mode, const int32_t* ijk, const int32_t* out_shape, float scale_div, uint32_t mask,
                         double* dec_ovo, double* dec_ovr, double* proba,
                         int32_t* label_vote, int32_t* label_calib, void* stream);

/* ---- linear classifier (SGDClassifier(loss='log'), train.py:350-381; predict 421,433) --- */
int rml_linear_load(rml_ctx* ctx, const double* coef /* host (C,D) */, const double* intercept /* host C */,
                    int n_classes, int64_t D, const double* calib_a, const double* calib_b, rml_linear** out);
int rml_linear_free(rml_ctx* ctx, rml_linear* m);
int rml_linear_decision(rml_ctx* ctx, const rml_linear* m, const float* feat, int64_t ld_feat, int64_t N,
                        double* dec /* N*C */, double* proba /* N*C or NULL */, int32_t* label /* argmax dec */,
                        int32_t* label_calib, void* stream);

/* ---- PIL bicubic resize in front of the dnn / sgan classifiers ----------------------------------------------
 * Image.fromarray(p).resize((out_w, out_h), resample=Image.BICUBIC) of float32 planes (dnn.py:240-245,
 * sgan.py:676-681; Pillow's Resample.c: antialiased, double-precision taps, float32 intermediate), bit-identical
 * to Pillow.  When div != 0 the reference's [-1,1] scaling (dnn.py:202-205) is applied first: v = (p - sub) / div
 * (sub = div = RADAR_MAX/2 = 127.5).  in: B planes of H x W float32, in_stride floats from one sample to the next
 * (a plane inside a feature row [xz|yz|xy] is addressed directly); out: B x out_h x out_w contiguous, float32
 * (out_bf16 = 0) or bf16 (out_bf16 = 1, the operand type of rml_dnn_trunk).  Sizes whose plane and intermediate image do not fit
 * the LDS together (128 x 128 -> 22 x 176, the data product of sgan.py:474-479) run Pillow's two passes as two launches through the
 * float32 intermediate image in the context's workspace: the same bits. */
int rml_resize_bicubic(rml_ctx* ctx, const float* in, int64_t in_stride, int64_t B, int H, int W, int out_h, int out_w,
                       float sub, float div, void* out, int out_bf16, void* stream);
/* ---- the same preprocessing for the bf16 conv trunk, all three projections of a feature row in ONE launch ------------
 * dnn.py:200-254 ((p - 127.5) / 127.5, then the bicubic resize of xz (X x Z), yz (Y x Z) and xy (X x Y) to out_h x out_w) with
 * bf16 outputs (the operand type of rml_dnn_trunk).  Pillow's windows and normalised weights -- the tables of
 * rml_resize_bicubic -- applied in float32 (fused multiply-adds, partial sums): NOT bit-identical to Pillow, within ~1e-6 of it
 * before the bf16 rounding (the bf16 value differs from the rounded exact one by at most one bf16 ulp on a small fraction of
 * the pixels); rml_resize_bicubic stays the Pillow-exact surface.  Input per row: the float32 feature row [xz | yz | xy]
 * (rows, ld floats apart) and / or the biased uint8 code row rml_project writes (codes, ldq bytes apart, 16-byte aligned);
 * flags[b] != 0 selects the code row of row b (the per-row "every value is an integer in [0, 255]" flag of rml_project), 0 its
 * float row; a row whose kind was not passed is left untouched (flags with ONE kind of row: only the rows of that kind are
 * written); flags = NULL: every row, from the one kind given.  Outputs: (B, out_h, out_w) bf16, 8-byte aligned.
 * Shapes: Z % 16 == 0, out_w % 4 == 0, out_w <= 256, out_h >= X and >= Y (no vertical shrink), (X + Y) * Z <= 16 384,
 * X * Y <= 4 096 -- rml_dnn_preprocess_supported says; others: RML_ERR_UNSUPPORTED (rml_resize_bicubic per projection). */
int rml_dnn_preprocess_supported(int X, int Y, int Z, int out_h, int out_w);
int rml_dnn_preprocess_rows(rml_ctx* ctx, const float* rows, int64_t ld, const uint8_t* codes, int64_t ldq, const int32_t* flags,
                            int64_t B, int X, int Y, int Z, int out_h, int out_w, uint16_t* xz, uint16_t* yz, uint16_t* xy,
                            void* stream);
/* Volumes -> trunk inputs (the front of BASELINE configs[3]): projection (mode as rml_project; ijk for RML_MODE_SLICE) into code rows
 * + row flags (no float rows through HBM), for float32 volumes a float-row pass predicated ON THE DEVICE on "some row left the
 * code grid" (it exits at once for radar data, integers 0..255: common.py:30-31) -- queued on the context's second stream beside
 * the code rows' preprocessing, joined before the call returns its stream --, then rml_dnn_preprocess_rows.  Scratch is the
 * caller's: codes B x ldq bytes (ldq >= D, % 16 == 0), flags B + 1 int32 (flags[B]: every row on the grid), rows B x ld float32
 * (float32 volumes only; NULL for uint8 volumes, which cannot leave the grid). */
int rml_dnn_preprocess_volumes(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, int mode, const int32_t* ijk,
                               uint8_t* codes, int64_t ldq, int32_t* flags, float* rows, int64_t ld, int out_h, int out_w,
                               uint16_t* xz, uint16_t* yz, uint16_t* xy, void* stream);
/* Target slices -> trunk inputs in ONE launch.  The reference's samples are the three planes of the radar image through one
 * target's voxel: yz = V[i,:,:], xz = V[:,j,:], xy = V[:,:,k] (predict.py:98-107, ground_truth_samples.py:413-419), and its live loop
 * classifies every target of every scan that way (predict.py:93-119).  V: B volumes (X, Y, Z), float32 (4-byte aligned) or uint8
 * (16-byte aligned); ijk: B * T * 3 int32, frame-major (row b * T + t is target t of frame b), negative indices wrap like Python's,
 * the range is the caller's responsibility (as for rml_project_slices).  The (X + Y) * Z + X * Y voxels of a slice go straight from
 * the volume into the kernel's LDS image -- float16 images for uint8 volumes, float32 images for float32 volumes (any finite value:
 * no on-grid test) -- and through the passes of rml_dnn_preprocess_rows: the planes are those of rml_dnn_preprocess_rows on the rows
 * of rml_project_slices, bit for bit.  Outputs: (B * T, out_h, out_w) bf16, 8-byte aligned.  No scratch, no row flags, no second
 * stream, no synchronisation; the only allocation is the cached table of a new (grid, output size) pair.  Shapes: those of
 * rml_dnn_preprocess_supported, others RML_ERR_UNSUPPORTED; T < 1: RML_ERR_INVALID; B == 0: RML_OK. */
int rml_dnn_preprocess_slices(rml_ctx* ctx, const void* V, int vdtype, int64_t B, int X, int Y, int Z, const int32_t* ijk, int T,
                              int out_h, int out_w, uint16_t* xz, uint16_t* yz, uint16_t* xy, void* stream);
/* ---- dnn.py convolutional trunk (dnn.py:45-52,68-76), fused ----------------------------------------------
 * Per branch Conv2D(1->64,3x3,s2,'same',relu) -> Conv2D(64->32,3x3,s2,'same',relu); the three branches concatenated
 * on channels and flattened NHWC: feat[b][(h*(W/4)+w)*96 + branch*32 + n], bf16.  Inputs (B,H,W) already scaled to
 * [-1,1] and resized (dnn.py:200-254; rml_resize_bicubic), float32 (in_bf16 = 0; H, W multiples of 4; rounded to
 * bf16 on load) or bf16 (in_bf16 = 1; W a multiple of 8): the results are identical.  Weights (DEVICE): w1 [3][64][9] float32
 * (tap = ky*3+kx), b1 [3][64], w2t [3][32][576] bf16 with k = (ky*3+kx)*64 + cin, b2 [3][32]. */
int rml_dnn_trunk(rml_ctx* ctx, const void* xz, const void* yz, const void* xy, int in_bf16, int64_t B, int H, int W,
                  const float* w1, const float* b1, const uint16_t* w2t, const float* b2,
                  uint16_t* feat, void* stream);
/* Host only, no context, no GPU: what rml_dnn_trunk would launch for B >= 1 samples of (H, W) planes on a device of num_cu compute
 * units, answered by the launchers' own predicates.  out[0]: the kernel -- 0 unsupported (rml_dnn_trunk returns RML_ERR_UNSUPPORTED),
 * 1 k_dnn_trunk_rf (conv1 image in registers; conv1 bias to float32 precision), 2 k_dnn_trunk (conv1 image in LDS; conv1 bias as one
 * bf16); out[1], out[2]: k_dnn_trunk's conv2 rows per strip SR and workgroups per CU WPC (0 for rf); out[3]: 1 when k_dnn_trunk
 * prefetches the next plane into registers; out[4]: 1 when k_dnn_trunk_rf gives a sample to a workgroup, 0 to a wave; out[5]:
 * workgroups along the sample axis of the grid.  RML_ERR_INVALID for out == NULL, B outside [1, 2^31) or num_cu < 1. */
int rml_dnn_trunk_path(int H, int W, int in_bf16, int64_t B, int num_cu, int out[6]);
/* The same values in the layout rml_dnn_dense_tail streams best ("K-block"): feat[kb][b][64] bf16 with the K axis ordered (branch,
 * pixel, channel) -- element (branch, pixel, channel) of sample b at block kb = (branch * P + pixel) / 2, offset (pixel & 1) * 32 +
 * channel, P = (H/4) * (W/4) even.  A 128-sample tile of one K-step is then 16 KB of contiguous memory (row-major rows put those
 * 128 pieces of 128 B 76.8 KB apart: every piece its own DRAM page, 3.3-3.6 TB/s for every GEMM that was tried on it).
 * RML_ERR_UNSUPPORTED for planes the register-resident trunk kernel does not take.
 * rml_dnn_trunk_kblock_supported (host only, no device needed): H % 4 == 0, W % 8 == 0, P even and that kernel's LDS layout -- eight
 * wave-private bf16 planes with a 4-pixel border + 36 KB of weights -- within the 160 KB; the 80 x 80 of dnn.py:33 does. */
int rml_dnn_trunk_kblock_supported(int H, int W);
int rml_dnn_trunk_kblock(rml_ctx* ctx, const void* xz, const void* yz, const void* xy, int in_bf16, int64_t B, int H, int W,
                         const float* w1, const float* b1, const uint16_t* w2t, const float* b2,
                         uint16_t* feat, void* stream);

/* The same two convolutions at float32-class accuracy (csrc/dnn_x3.hip, round 6) -- the reference's model.predict is float32 Keras
 * (dnn.py:373-381): every operand is carried as `parts` bf16 numbers and every product as the matrix-core products of the part
 * pairs (i, j) with i + j < parts, float32 accumulation.  parts = 2 ("x3": 16 significant bits, three products, ~2^-16 relative
 * per product where rml_dnn_trunk has bf16's 2^-9; about 3.5 x the time of rml_dnn_trunk per sample) or 3 ("x6": 24 bits, six
 * products, what is dropped is the size of float32's own rounding; about twice x3).  Planes float32 (rml_resize_bicubic's
 * Pillow-bit-identical output), weights float32: w1 [3][64][9], b1 [3][64], w2 [3][32][576] (k = (ky*3+kx)*64 + cin; NOT transposed
 * to bf16), b2 [3][32]; feat[b][(h*(W/4)+w)*96 + branch*32 + n] float32 (Keras' Flatten order).  Planes, w2 and feat 16-byte aligned.
 * The second opinion of the margin guard (radar-ml_amd/dnn.py), not the fast path.
 * rml_dnn_trunk_x3_supported: H, W multiples of 4 and three float32 planes + 72 KB of weight fragments (one plane + 108 KB for
 * parts = 3) within the 160 KB LDS -- the 80 x 80 of dnn.py:33 does; otherwise RML_ERR_UNSUPPORTED. */
int rml_dnn_trunk_x3_supported(int H, int W);
int rml_dnn_trunk_x3(rml_ctx* ctx, const float* xz, const float* yz, const float* xy, int64_t B, int H, int W,
                     const float* w1, const float* b1, const float* w2, const float* b2, int parts, float* feat, void* stream);

/* Volumes -> float32-class features in one call (the re-scoring front of the margin guard): frames rows[0..n) of V (rows = NULL: the
 * first n frames) gathered into scratch, projected exactly (rml_project, float32 rows, mode MAX / SUM / MAX_NAN), scaled to [-1, 1]
 * and resized with rml_resize_bicubic (Pillow-bit-identical float32 planes), then rml_dnn_trunk_x3 with `parts`.  scratch:
 * rml_dnn_exact_features_scratch_bytes(vdtype, n, X, Y, Z, out_h, out_w, rows != NULL) bytes, 256-byte aligned. */
int64_t rml_dnn_exact_features_scratch_bytes(int vdtype, int64_t n, int X, int Y, int Z, int out_h, int out_w, int gathered);
int rml_dnn_exact_features(rml_ctx* ctx, const void* V, int vdtype, const int64_t* rows, int64_t n, int X, int Y, int Z, int mode,
                           int out_h, int out_w, const float* w1, const float* b1, const float* w2, const float* b2, int parts,
                           void* scratch, int64_t scratch_bytes, float* feat, void* stream);

/* ---- the margin guard's device side (radar-ml_amd/dnn.py Classifier._guard; labels of model.predict, dnn.py:373-381) --------------
 * rml_dnn_top2_gap: gap[r] = largest - second largest of proba[r][0..C) (rows ld floats apart, 2 <= C <= 16); 0 for a row that
 * holds a non-finite value (it counts as a tie).
 * rml_dnn_guard_apply: one re-scoring round's bookkeeping in one launch -- proba[rows[i]] <- fresh[i] (fresh: n x C contiguous),
 * stats[0] = atomic max over the rows where both are finite of |old - new| as float32 BITS (non-negative floats order like unsigned
 * integers; zero stats before the call), stats[1] += rows whose new top-2 gap is below thr_close, close[i] = that test,
 * gap[rows[i]] = +inf when gap is given (re-scored: never a candidate again). */
int rml_dnn_top2_gap(rml_ctx* ctx, const float* proba, int64_t ld, int64_t N, int C, float* gap, void* stream);
int rml_dnn_guard_apply(rml_ctx* ctx, float* proba, int64_t ld, int C, const int64_t* rows, int64_t n, const float* fresh,
                        float thr_close, float* gap, uint32_t* stats, uint8_t* close, void* stream);

/* ---- dnn.py dense tail (dnn.py:78-88), fused -----------------------------------------------------------------
 * Dense 64 relu -> Dense 64 relu -> Dense n_classes softmax on the bf16 feature rows of rml_dnn_trunk (Dropout is inactive at
 * inference): proba[b][c] float32.  The first layer runs on the bf16 matrix cores (float32 accumulation, split-K with the partial
 * sums added in a fixed order: deterministic), the two small layers and the softmax in float32.  feat: N rows of K bf16, ld_feat
 * elements apart (kblock = 0; K % 64 == 0, ld_feat % 8 == 0, 16-byte aligned), or the [K/64][N][64] layout of rml_dnn_trunk_kblock
 * (kblock = 1: w1 is then blocked the same way, [K/64][64 out][64], the K axis in the (branch, pixel, channel) order); w1 [64][K]
 * bf16 (kblock = 0: torch Linear layout, out x in), b1 [64];
 * w2t [64 in][64 out] float32 -- the TRANSPOSE of torch's (out, in) = the Keras kernel layout (in, out) --, b2 [64]; w3
 * [n_classes][64] float32 (torch layout), b3 [n_classes]; n_classes <= 16.  workspace: rml_dnn_dense_workspace_bytes(ctx, N, K)
 * bytes of device memory, 16-byte aligned (the split-K partial sums). */
int64_t rml_dnn_dense_workspace_bytes(rml_ctx* ctx, int64_t N, int64_t K);
int rml_dnn_dense_tail(rml_ctx* ctx, const uint16_t* feat, int64_t ld_feat, int kblock, int64_t N, int64_t K, const uint16_t* w1, const float* b1,
                       const float* w2t, const float* b2, const float* w3, const float* b3, int n_classes, float* workspace,
                       int64_t workspace_bytes, float* proba, void* stream);

/* The same tail on FLOAT32 feature rows (feat [N][ld_feat], w1 [64][K] float32 in torch's Linear layout, the other operands as
 * above): the last stage of the margin guard's re-scoring (radar-ml_amd/dnn.py Classifier._tail_float32; Keras runs these layers in
 * float32, dnn.py:78-88).  Its result for a row depends on that row alone -- the K axis is cut into splits that are a function of
 * K only, every partial sum is one fma chain in ascending k, the splits are added in order -- so a row scored alone, inside any
 * candidate set, or twice has the same bits (a library float32 GEMM that splits K with atomics does not).  K and ld_feat multiples
 * of 4; workspace: rml_dnn_dense_tail_f32_workspace_bytes(N, K) bytes, 16-byte aligned. */
int64_t rml_dnn_dense_tail_f32_workspace_bytes(int64_t N, int64_t K);
int rml_dnn_dense_tail_f32(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int64_t K, const float* w1, const float* b1,
                           const float* w2t, const float* b2, const float* w3, const float* b3, int n_classes, float* workspace,
                           int64_t workspace_bytes, float* proba, void* stream);

/* ---- SGAN classifier at inference (sgan.py:132-199, c_model.predict), fused -----------------------------------------------------
 * The trunk: per branch Conv2D(1->128, 3x3, s2, 'same') -> Conv2D(128->64, s2) -> Conv2D(64->32, s2), each followed by BatchNorm and
 * LeakyReLU(slope); in inference mode the BatchNorm is an affine map and the CALLER folds it into the weights: s = gamma /
 * sqrt(moving_variance + eps), w' = w * s, b' = beta + (bias - moving_mean) * s.  Inputs as rml_dnn_trunk: three (B, H, W) planes in
 * [-1, 1], float32 (in_bf16 = 0, rounded to bf16 on load) or bf16 (in_bf16 = 1): identical results.  A window is loaded as
 * aligned pairs; the neighbouring value a pair brings along is masked to zero, so a non-finite plane value reaches only the pixels
 * whose 3x3 window holds it, as in the reference convolution.  Folded weights (DEVICE), k =
 * (ky*3+kx)*Cin + cin: w1 [3][128][9] float32, b1 [3][128]; w2t [3][64][1152] bf16, b2 [3][64] float32; w3t [3][32][576] bf16, b3
 * [3][32] float32.  feat[b][(h*(W/8)+w)*96 + branch*32 + n] bf16 -- Keras' Flatten of the concatenated branches.  bf16 operands on the
 * matrix cores, float32 accumulation; biases and LeakyReLU in float32 before the rounding to bf16; 0 <= slope <= 1.  The layer-1
 * activation is recomputed where layer 2 reads it and never stored; the layer-2 activation goes through the workspace.  No atomics:
 * a sample's features are the same bits alone, at any position of any batch, and on a second call.
 * rml_sgan_trunk_supported (HOST, no device): H and W multiples of 8 (every stride-2 'same' layer then sees an even size and pads
 * bottom / right only), W <= 128, H <= 32 768; anything else: 0, and rml_sgan_trunk returns RML_ERR_UNSUPPORTED without a launch.
 * workspace: rml_sgan_trunk_workspace_bytes(B, H, W) bytes (0 for unsupported planes; non-decreasing in B), 16-byte aligned, as are
 * the planes, w2t, w3t and feat. */
int rml_sgan_trunk_supported(int H, int W);
int64_t rml_sgan_trunk_workspace_bytes(int64_t B, int H, int W);
int rml_sgan_trunk(rml_ctx* ctx, const void* xz, const void* yz, const void* xy, int in_bf16, int64_t B, int H, int W,
                   const float* w1, const float* b1, const uint16_t* w2t, const float* b2, const uint16_t* w3t, const float* b3,
                   float slope, uint16_t* feat, void* workspace, int64_t workspace_bytes, void* stream);
/* rml_dnn_dense_tail (row-major features, kblock = 0) with LeakyReLU(slope) instead of relu behind the two hidden layers: x > 0 ? x :
 * slope * x.  The BatchNorm1d layers behind fc1 / fc2 fold into w1 / b1 and w2t / b2 on the host.  The same split-K first layer
 * (fixed K pieces, summed in order), the same workspace size (rml_dnn_dense_workspace_bytes). */
int rml_dense_tail_lrelu(rml_ctx* ctx, const uint16_t* feat, int64_t ld_feat, int64_t N, int64_t K, const uint16_t* w1, const float* b1,
                         const float* w2t, const float* b2, const float* w3, const float* b3, int n_classes, float slope,
                         float* workspace, int64_t workspace_bytes, float* proba, void* stream);

/* The same trunk at float32-class accuracy (csrc/sgan_x3.hip) -- c_model.predict is float32 Keras (sgan.py:132-199): the arithmetic of
 * rml_dnn_trunk_x3 on the layers of rml_sgan_trunk.  Every operand is carried as `parts` bf16 numbers and every product as the
 * matrix-core products of the part pairs (i, j) with i + j < parts, the smallest terms first, float32 accumulation: parts = 2 ("x3",
 * ~2^-16 relative per product) or 3 ("x6", ~2^-24); anything else RML_ERR_INVALID.  Planes float32; folded weights float32 with k =
 * (ky*3+kx)*Cin + cin: w1 [3][128][9], b1 [3][128], w2 [3][64][1152], b2 [3][64], w3 [3][32][576], b3 [3][32] (NOT rounded to bf16);
 * feat[b][(h*(W/8)+w)*96 + branch*32 + n] float32.  conv1's bias rides in three bf16 K slots, the other biases start the float32
 * accumulators (all exact); LeakyReLU(slope), 0 <= slope <= 1, in float32; the layer-2 activation goes through the workspace as
 * float32.  No atomics, one owner and one order per sum: a sample's features are the same bits alone, at any position of any batch,
 * and on a second call.  The second opinion of the margin guard (radar-ml_amd/sgan.py), not the fast path.
 * rml_sgan_trunk_x3_supported (HOST, no device; sgan.py:132-199 at 128 x 128 does): H and W multiples of 8, at most 4096; anything
 * else: 0, and rml_sgan_trunk_x3 returns RML_ERR_UNSUPPORTED without a launch.
 * workspace: rml_sgan_trunk_x3_workspace_bytes(B, H, W) bytes (the layers of sgan.py:132-199 in operand order for either part count
 * + the layer-2 activation; 0 for unsupported planes; non-decreasing in B), 16-byte aligned, as are the planes, w2, b2, w3, b3 and
 * feat; a shorter one: RML_ERR_INVALID.  B = 0: nothing is launched. */
int rml_sgan_trunk_x3_supported(int H, int W);
int64_t rml_sgan_trunk_x3_workspace_bytes(int64_t B, int H, int W);
int rml_sgan_trunk_x3(rml_ctx* ctx, const float* xz, const float* yz, const float* xy, int64_t B, int H, int W, const float* w1,
                      const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float slope, int parts,
                      float* feat, void* workspace, int64_t workspace_bytes, void* stream);
/* rml_dnn_dense_tail_f32 with LeakyReLU(slope) behind the two hidden layers (sgan.py:187-199 on the float32 rows of
 * rml_sgan_trunk_x3; the BatchNorm1d layers folded into w1 / b1 and w2t / b2 on the host): the same fixed K splits, the same
 * workspace size (rml_dnn_dense_tail_f32_workspace_bytes), a row's result depends on that row alone. */
int rml_dense_tail_lrelu_f32(rml_ctx* ctx, const float* feat, int64_t ld_feat, int64_t N, int64_t K, const float* w1, const float* b1,
                             const float* w2t, const float* b2, const float* w3, const float* b3, int n_classes, float slope,
                             float* workspace, int64_t workspace_bytes, float* proba, void* stream);

/* ---- dnn.py training step (dnn.py:347-390: model.fit on the model of dnn.py:45-91), float32 -----------------------------------
 * One step on the batch rows[0..B) of RESIDENT data: three float32 plane sets xz / yz / xy, [N][H][W] each, already scaled to
 * [-1, 1] and resized (H, W multiples of 4, W <= 128: rml_dnn_train_supported; others RML_ERR_UNSUPPORTED), labels [N] int32 in
 * [0, C), 2 <= C <= 16.  rows: DEVICE int32, B entries in [0, N), 1 <= B <= RML_DNN_TRAIN_MAX_BATCH; no gather copy is made.
 * Forward: per branch conv 1->64 3x3 stride 2 relu, conv 64->32 3x3 stride 2 relu (TF 'same': pad bottom / right), the branches
 * concatenated on the channel axis, Flatten in NHWC order (K = (H/4)(W/4)*96), Dense 64 relu, dropout, Dense 64 relu, dropout,
 * Dense C; loss_b = class_weight[y_b] * (logsumexp(z_b) - z_b[y_b]) (class_weight: DEVICE float32 [C], NULL = ones), the batch
 * loss is sum_b loss_b / B (Keras' class_weight under SUM_OVER_BATCH_SIZE).  All operands and sums are float32.
 *   params: HOST array of 18 DEVICE pointers in the order of the torch module's parameters(): per branch (xz, yz, xy) k1
 *   [64][1][3][3], b1 [64], k2 [32][64][3][3], b2 [32]; then W [64][K], b [64]; W [64][64], b [64]; W [C][64], b [C] (torch Linear:
 *   out x in).  k2_layout 0: k2 dense in (out, in, ky, kx) order; 1: channels_last, (out, ky, kx, in).
 *   grads (mode TRAIN): 18 DEVICE pointers, the same shapes and layouts; every element is overwritten with d(batch loss)/d(param).
 *   Dropout: unit j of dropout layer l (0, 1) of the sample at batch position b is kept iff a uniform draw that is a function of
 *   (seed, step, l, b, j) only -- not of B, not of the launch geometry -- is >= rate; kept units are scaled by 1 / (1 - rate);
 *   0 <= rate < 1.  rml_dnn_dropout_mask (HOST, no device, no context): keep[j] = 1 / 0 for j < n_units, the same function.
 *   mode RML_DNN_EVAL: the same forward without dropout, no gradients (grads may be NULL).
 *   Both modes: *loss_sum (DEVICE double) += sum_b loss_b (not divided by B), *correct (DEVICE int32) += #{b: first argmax_c z_b[c]
 *   == y_b}: zero them where an epoch starts, read them once where it ends.
 *   status (DEVICE int32, zeroed by the caller): set to -1 when a row index is outside [0, N) or a label outside [0, C); the step
 *   then reads no plane, writes no gradient and leaves the accumulators alone.
 *   workspace: rml_dnn_train_workspace_bytes(B, H, W, C) bytes, 16-byte aligned (0 is returned for unsupported arguments); the size
 *   for B covers every batch of up to B samples (non-decreasing in B), so one workspace serves an epoch's partial last batch too.
 * Every sum over the batch or over pixels has one owner and a fixed order (per-workgroup partial sums, then an ordered
 * reduction; no atomics): the same call on the same inputs gives the same bits.  Asynchronous on `stream`.  The update itself is
 * rml_adam_step below (torch.optim.Adam's form: epsilon inside the bias correction of the denominator, where Keras adds it
 * outside -- Keras' epsilon is this one's divided by sqrt(1 - beta2^t), so the two updates differ only where sqrt(v) is itself of the
 * order of eps = 1e-7). */
#define RML_DNN_TRAIN 0
#define RML_DNN_EVAL 1
#define RML_DNN_TRAIN_MAX_BATCH 64
int rml_dnn_train_supported(int H, int W, int C);
int64_t rml_dnn_train_workspace_bytes(int B, int H, int W, int C);
int rml_dnn_train_step(rml_ctx* ctx, const float* xz, const float* yz, const float* xy, const int32_t* labels, const int32_t* rows,
                       int B, int64_t N, int H, int W, const float* class_weight, int C, const void* const* params,
                       void* const* grads, int k2_layout, uint64_t seed, int64_t step, float rate, int mode, void* workspace,
                       int64_t workspace_bytes, double* loss_sum, int32_t* correct, int32_t* status, void* stream);
int rml_dnn_dropout_mask(uint64_t seed, int64_t step, int layer, int b, int n_units, float rate, uint8_t* keep);

/* ---- SGAN discriminator branches: fused BatchNorm(train) + LeakyReLU + 'same' pad (sgan.py:137-158) -------------
 * x: N x H x W x C (NHWC, dense) float16 (dtype 0) or bfloat16 (dtype 1), the convolution output; y: N x (H+pad_h) x
 * (W+pad_w) x C, the zero-padded input of the next stride-2 'same' convolution (pad 0: plain output).  Batch
 * statistics in float32/float64 (deterministic), running estimates updated as torch.nn.BatchNorm2d does
 * (momentum = 1 - Keras momentum).  workspace: rml_bn_workspace_floats(ctx, C) + 2*C floats (all three entry points).  backward: dy has y's
 * layout; returns dx (x's layout) and the float32 parameter gradients. */
int64_t rml_bn_workspace_floats(rml_ctx* ctx, int C);
int rml_bn_lrelu_pad_forward(rml_ctx* ctx, const void* x, int dtype, int64_t N, int H, int W, int C, int pad_h, int pad_w,
                             const float* gamma, const float* beta, float eps, float momentum, float slope,
                             float* running_mean, float* running_var, float* save_mean, float* save_rstd,
                             float* workspace, void* y, void* stream);
int rml_bn_lrelu_pad_backward(rml_ctx* ctx, const void* x, const void* dy, int dtype, int64_t N, int H, int W, int C,
                              int pad_h, int pad_w, const float* gamma, const float* beta, const float* save_mean,
                              const float* save_rstd, float slope, float* workspace, void* dx, float* dgamma, float* dbeta,
                              void* stream);

/* First layer of a branch, [3x3 stride-2 'same' convolution of a 1-channel image] + BatchNorm + LeakyReLU + pad with the
 * convolution folded in (the image needs no gradient): the convolution output is never stored; every pass recomputes
 * it (9 FMAs per element) from the zero-padded half-precision image N x (2H+1) x (2W+1) and the float32 weights
 * weight[tap][c].  forward: image -> y; backward: image, dy -> dweight[tap][c], dgamma, dbeta (rows of at most 340 pixels:
 * RML_ERR_UNSUPPORTED beyond, except for the packed shapes C = 128, W = 16 / 32 / 64). */
int rml_conv1_bn_lrelu_pad_forward(rml_ctx* ctx, const void* image, const float* weight, int dtype, int64_t N, int H, int W,
                                   int C, int pad_h, int pad_w, const float* gamma, const float* beta, float eps,
                                   float momentum, float slope, float* running_mean, float* running_var, float* save_mean,
                                   float* save_rstd, float* img_stats /* 54 floats out: sums of the taps and of their products */,
                                   float* workspace, void* y, void* stream);
int rml_conv1_bn_lrelu_pad_backward(rml_ctx* ctx, const void* image, const float* weight, const void* dy, int dtype, int64_t N,
                                    int H, int W, int C, int pad_h, int pad_w, const float* gamma, const float* beta,
                                    const float* save_mean, const float* save_rstd, const float* img_stats /* from forward */,
                                    float slope, float* workspace, float* dweight, float* dgamma, float* dbeta, void* stream);

/* ---- SGAN generator output layer: Conv2D(1, 7x7, 'same') + tanh (sgan.py:112-114; csrc/gen.hip) ------------------------------------
 * x: N x H x W x C (NHWC, dense, 16-byte aligned) float16 (dtype 0) or bfloat16 (dtype 1); weight: float32 [49][C], tap = ky * 7 + kx (the
 * Keras kernel (7, 7, C, 1) flattened), rounded to x's type on load; bias: 1 float; y, dy: N x H x W float32.  All sums in float32, in an
 * order fixed by (H, W) alone -- no atomics: the same call gives the same bits, and y / dx of a sample do not depend on the batch around
 * it.  backward: dz = dy (1 - y^2); dx (x's layout and type), dweight [49][C], dbias [1]; workspace of
 * rml_conv7_workspace_floats(ctx, N, H, W, C) floats.  rml_conv7_tanh_supported: 1 for C = 128 and 1 <= H, W <= 256. */
int rml_conv7_tanh_supported(int H, int W, int C);
int64_t rml_conv7_workspace_floats(rml_ctx* ctx, int64_t N, int H, int W, int C);
int rml_conv7_tanh_forward(rml_ctx* ctx, const void* x, int dtype, int64_t N, int H, int W, int C, const float* weight,
                           const float* bias, float* y, void* stream);
int rml_conv7_tanh_backward(rml_ctx* ctx, const void* x, const float* y, const float* dy, int dtype, int64_t N, int H, int W, int C,
                            const float* weight, float* workspace, void* dx, float* dweight, float* dbias, void* stream);

/* ---- SGAN generator at inference (sgan.py:57-122 through g_model.predict: sgan.py:450 in generate_fake_samples, sgan.py:462-488 in
 * summarize_performance; csrc/gen_infer.hip) ----------------------------------------------------------------------------------------------
 * rml_gen_up_forward: Conv2DTranspose(C -> C, 4x4, stride 2, 'same') + BatchNormalization (moving statistics) + ReLU (sgan.py:65-87) with
 * the BatchNorm folded by the CALLER.  x: N x H x W x C (NHWC, dense) float16 (dtype 0) or bfloat16 (dtype 1) -> y: N x 2H x 2W x C of the
 * same type.  Output pixel (2m+p, 2n+q), p, q in {0, 1}, reads the 2x2 input window at rows m-1+p+a and columns n-1+q+b (a, b in {0, 1};
 * outside the plane: zero) through the kernel taps ky = 3-p-2a, kx = 3-q-2b (oy = 2 iy + ky - 1).  wt (DEVICE, of x's type):
 * wt[p*2+q][co][(a*2+b)*C + ci] = K[ky][kx][co][ci] * s[co] with K the Keras kernel (4, 4, out, in) and s = gamma / sqrt(moving_variance +
 * eps); bias[co] float32 = beta + (b - moving_mean) * s.  Four implicit GEMMs (K = 4C) on the matrix cores, float32 accumulation, bias and
 * ReLU in float32 before the rounding.  No atomics; the sum order of an output element depends on nothing but (H, W): a sample has the
 * same bits alone, at any position of any batch, and on a second call.  x, wt, bias and y 16-byte aligned.
 * rml_gen_up_supported (HOST, no device): C = 128, H and W multiples of 8 in [8, 128]; anything else: 0, and rml_gen_up_forward returns
 * RML_ERR_UNSUPPORTED without a launch.
 * rml_sgan_generate: the whole generator, g_model.predict(z).  z [N][latent_dim] float32; per branch (xz, yz, xy) Dense + ReLU into the NHWC
 * image [base][base][C] (Keras unit order: no permutation), n_up x rml_gen_up_forward ping-ponging through the workspace, then
 * rml_conv7_tanh_forward into y_xz / y_yz / y_xy, each [N][S][S] float32, S = base * 2^n_up.  dense_w [3][latent_dim][base*base*C] float32
 * (the Keras kernels), dense_b [3][base*base*C]; up_wt [3][n_up][4][C][4C] of `dtype` and up_bias [3][n_up][C] float32 as above; out_w
 * [3][49][C] float32 and out_b [3] as rml_conv7_tanh_forward takes them.  The dense layer runs in float32 FMAs in a fixed order and rounds
 * once.  N is cut into chunks so that the workspace stays bounded (128 MB of activations, one sample at least);
 * workspace: rml_sgan_generate_workspace_bytes(N, base, n_up, C) bytes (0 for unsupported sizes; non-decreasing in N), 16-byte aligned.
 * Asynchronous on `stream`, no device synchronisation.  Unsupported sizes (RML_ERR_UNSUPPORTED) and a workspace that is too small
 * (RML_ERR_INVALID) are reported before anything is launched. */
int rml_gen_up_supported(int H, int W, int C);
int rml_gen_up_forward(rml_ctx* ctx, const void* x, int dtype, int64_t N, int H, int W, int C, const void* wt, const float* bias, void* y,
                       void* stream);
int64_t rml_sgan_generate_workspace_bytes(int64_t N, int base, int n_up, int C);
int rml_sgan_generate(rml_ctx* ctx, const float* z, int64_t N, int latent_dim, int base, int n_up, int C, int dtype, const float* dense_w,
                      const float* dense_b, const void* up_wt, const float* up_bias, const float* out_w, const float* out_b, float* y_xz,
                      float* y_yz, float* y_xy, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- SGAN discriminator in training: the 3x3 stride-2 convolutions of layers 2 and 3 and their gradients (sgan.py:137-158;
 * csrc/conv_train.hip) -------------------------------------------------------------------------------------------------------------
 * A VALID convolution of an already padded tensor, no bias.  x: N x hp x wp x cin (NHWC, dense), hp = 2 Ho + 1, wp = 2 Wo + 1 -- what
 * rml_bn_lrelu_pad_forward / rml_conv1_bn_lrelu_pad_forward write; w: [cout][3][3][cin], the channels_last storage of a (cout, cin, 3, 3)
 * tensor; z: N x Ho x Wo x cout.  All of float16 (dtype 0) or bfloat16 (dtype 1), float32 accumulation on the matrix cores, one rounding.
 *   forward  z[n,oy,ox,co] = sum x[n,2oy+ky,2ox+kx,ci] w[co,ky,kx,ci]
 *   dgrad    dx[n,y,x,ci]  = sum over ky = y, kx = x (mod 2), co of dz[n,(y-ky)/2,(x-kx)/2,co] w[co,ky,kx,ci]: EVERY element of the padded dx
 *            is written (the bottom / right pad row and column too)
 *   wgrad    dw[co,ky,kx,ci] = sum over n, oy, ox of dz[n,oy,ox,co] x[n,2oy+ky,2ox+kx,ci], of the half type, in w's layout
 * No atomics, no zeroed workspace; every output has one summation order that depends on the shapes alone (the same call gives the same
 * bits; a sample's z does not depend on the batch around it).  Asynchronous on `stream`, no allocation, no synchronisation.
 * rml_conv3s2_supported (HOST): cin -> cout of 128 -> 64 or 64 -> 32, hp and wp odd in [3, 8193]; anything else: 0, and the three passes
 * return RML_ERR_UNSUPPORTED before any launch.  workspace: rml_conv3s2_workspace_bytes(..., pass) bytes (0 for unsupported shapes),
 * 16-byte aligned like every tensor; its contents need no initialisation. */
#define RML_CONV3S2_FORWARD 0
#define RML_CONV3S2_DGRAD 1
#define RML_CONV3S2_WGRAD 2
int rml_conv3s2_supported(int cin, int cout, int hp, int wp);
int64_t rml_conv3s2_workspace_bytes(rml_ctx* ctx, int64_t n, int hp, int wp, int cin, int cout, int pass);
int rml_conv3s2_forward(rml_ctx* ctx, const void* x, const void* w, int dtype, int64_t n, int hp, int wp, int cin, int cout, void* z,
                        void* workspace, int64_t workspace_bytes, void* stream);
int rml_conv3s2_dgrad(rml_ctx* ctx, const void* dz, const void* w, int dtype, int64_t n, int hp, int wp, int cin, int cout, void* dx,
                      void* workspace, int64_t workspace_bytes, void* stream);
int rml_conv3s2_wgrad(rml_ctx* ctx, const void* x, const void* dz, int dtype, int64_t n, int hp, int wp, int cin, int cout, void* dw,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- SGAN generator in training: Conv2DTranspose(128 -> 128, 4x4, stride 2, 'same') and its gradients (sgan.py:65-87;
 * csrc/convt_train.hip) ------------------------------------------------------------------------------------------------------------
 * No bias (the batch norm behind the layer cancels it).  h, w are the INPUT plane.  x: N x h x w x cin (NHWC, dense); z, dz: N x 2h x 2w x
 * cout; w: [cin][4][4][cout], the channels_last storage of torch's (cin, cout, 4, 4) ConvTranspose2d weight; dw like w.  All of float16
 * (dtype 0) or bfloat16 (dtype 1), float32 accumulation on the matrix cores, one rounding.  With oy = 2 iy + ky - 1, ox = 2 ix + kx - 1
 * and everything outside a plane zero:
 *   forward  z[n,oy,ox,co]  = sum over iy, ix, ci of x[n,iy,ix,ci] w[ci,ky,kx,co]: at most 2 x 2 taps per output pixel, four phase GEMMs
 *   dgrad    dx[n,iy,ix,ci] = sum over ky, kx, co of dz[n,2iy+ky-1,2ix+kx-1,co] w[ci,ky,kx,co]
 *   wgrad    dw[ci,ky,kx,co] = sum over n, iy, ix of x[n,iy,ix,ci] dz[n,2iy+ky-1,2ix+kx-1,co], of the half type
 * No atomics, no zeroed workspace; every output has one summation order that depends on the shapes alone (the same call gives the same
 * bits; a sample's z and dx do not depend on the batch around it).  Asynchronous on `stream`, no allocation, no synchronisation.
 * rml_convt4s2_supported (HOST): cin = cout = 128, h and w multiples of 8 in [8, 128] (the domain of rml_gen_up_supported); anything
 * else: 0, and the three passes return RML_ERR_UNSUPPORTED before any launch.  workspace: rml_convt4s2_workspace_bytes(..., pass) bytes (0
 * for unsupported shapes; a smaller one: RML_ERR_INVALID), 16-byte aligned like every tensor; its contents need no initialisation. */
#define RML_CONVT4S2_FORWARD 0
#define RML_CONVT4S2_DGRAD 1
#define RML_CONVT4S2_WGRAD 2
int rml_convt4s2_supported(int cin, int cout, int h, int w);
int64_t rml_convt4s2_workspace_bytes(rml_ctx* ctx, int64_t n, int h, int w, int cin, int cout, int pass);
int rml_convt4s2_forward(rml_ctx* ctx, const void* x, const void* w, int dtype, int64_t n, int h, int w_, int cin, int cout, void* z,
                         void* workspace, int64_t workspace_bytes, void* stream);
int rml_convt4s2_dgrad(rml_ctx* ctx, const void* dz, const void* w, int dtype, int64_t n, int h, int w_, int cin, int cout, void* dx,
                       void* workspace, int64_t workspace_bytes, void* stream);
int rml_convt4s2_wgrad(rml_ctx* ctx, const void* x, const void* dz, int dtype, int64_t n, int h, int w_, int cin, int cout, void* dw,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Adam update of the SGAN discriminator (sgan.py:206, 214: Adam(lr=0.0002, beta_1=0.5) inside train_on_batch, sgan.py:525-532) ----
 * ONE pass over all parameters with the loss-scale bookkeeping of a half-precision step on the device (csrc/optim.hip).
 * table: DEVICE array of n_tensors + 1 records of rml_adam_entry_bytes() bytes each,
 *     { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t start; }
 * start = the tensor's first element in the concatenation of all tensors, record n_tensors holds { 0, 0, 0, 0, total }.  The four
 * tensors of a record are dense float32 with identical strides (the update runs over the storage order).
 * step: device float, the number of updates applied so far (incremented here unless the step is skipped).
 * scale: device float loss scale, or NULL (no scaling: gradients taken as they are, inv_scale = 1).  With check != 0 every gradient is
 * tested first; a non-finite one skips the whole update and multiplies the scale by `backoff`, `growth_interval` clean steps in
 * a row multiply it by `growth` (torch.amp.GradScaler's rule).  state: device int32[3] (non-finite count, growth tracker, skip flag
 * of the last call), zero-initialised by the caller once.  inv_scale: device float scratch.
 * The update is torch.optim.Adam's: m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2, p -= lr / (1-b1^t) * m / (sqrt(v) / sqrt(1-b2^t) + eps). */
int rml_adam_entry_bytes(void);
int rml_adam_step(rml_ctx* ctx, const void* table, int n_tensors, int64_t total, float lr, float beta1, float beta2, float eps,
                  float* step, float* scale, int32_t* state, float* inv_scale, int check, float growth, float backoff,
                  int growth_interval, void* stream);

/* ---- synthetic data (bench / tests) --------------------------------------- */
int rml_synth_volumes(rml_ctx* ctx, uint64_t seed, int64_t frame0, int64_t B, int X, int Y, int Z,
                      int n_classes, float* V, int32_t* cls /* B or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RADARML_H */
