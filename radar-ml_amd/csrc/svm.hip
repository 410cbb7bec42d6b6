// C-SVC decision function and linear classifier: the host side (model load, chunk plan, stages, entry points).
// The kernels and the overview of the path: svm_tile.h (128 x 128 tile, split-K), svm_ring.h (256 x 256 ring), svm_small.h
// (single observations), svm_rows.h (row preparation, tile flags), svm_finish.h (vote, Platt, linear).
#include "rml_internal.h"
#include "svm_tile.h"
#include "svm_ring.h"
#include "svm_small.h"
#include "svm_rows.h"
#include "svm_finish.h"
#include <math.h>
#include <vector>
#include <stdlib.h>
#include <type_traits>
#include <algorithm>
#include <new>

namespace {

// the multi-digit kernel for the general tiles of a chunk of n rows?  RML_DIGITS = 0 never, 1 always (when the model allows),
// default: when the launch has tiles for at least half a round of one workgroup per CU (below that the float64 MFMA kernel's
// 128 x 128 tiles fill the machine better)
inline bool use_dig_gemm(const rml_svm* m, int policy, int64_t n, int num_cu) {
    if (!m->dig_ok) return false;
    if (policy == RML_PATH_DIGITS) return true;
    if (policy != RML_PATH_AUTO) return false;
    const int64_t wgs = ((n + kBig - 1) / kBig) * ((m->Mpad + kBig - 1) / kBig);
    return wgs * 2 >= (int64_t)num_cu;
}

// does the 256x256 ring kernel take the exact tiles of a chunk of n rows against this model?  It runs at up to 0.6 of the int8
// peak when its tiles fill whole rounds of one workgroup per CU and proportionally less otherwise; the 128x128 kernel (two
// workgroups per CU, four times as many tiles) sits at 0.40-0.46 whatever the batch.  So: at least three quarters of a round,
// and the last round at least three quarters full.  knob = RML_OPT_GEMM_BIG: 0 turns it off, 1 forces it for every n >= 256.
inline bool use_big_gemm(const rml_svm* m, int64_t n, int num_cu, int knob) {
    if (knob == 0 || m->PT > 6) return false;
    if (knob == 1) return n >= 256;
    const int64_t wgs = ((n + kBig - 1) / kBig) * ((m->Mpad + kBig - 1) / kBig);
    const int64_t rounds = (wgs + num_cu - 1) / num_cu;
    return wgs * 4 >= (int64_t)num_cu * 3 && wgs * 4 >= rounds * num_cu * 3;
}

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

template <typename T> int dev_upload(T** dst, const std::vector<T>& h) {
    RML_HIP(hipMalloc(reinterpret_cast<void**>(dst), h.size() * sizeof(T)));
    RML_HIP(hipMemcpy(*dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return RML_OK;
}

RingArgs ring_args_from(const GemmArgs& ga) {
    RingArgs ra{};
    ra.sv = ga.sv; ra.x = ga.x; ra.ld_sv = ga.ld_sv; ra.ld_x = ga.ld_x; ra.KT = ga.KT;
    ra.N = ga.N; ra.Mpad = ga.Mpad; ra.sv_rows = ga.sv_rows; ra.ST = ga.ST; ra.FT = ga.FT;
    ra.tile_exact = ga.tile_exact; ra.want = ga.want; ra.x_isum = ga.x_isum; ra.x_isq = ga.x_isq;
    ra.sv_term = ga.sv_term; ra.W = ga.W; ra.gs = ga.gs; ra.kernel = ga.kernel; ra.partial = ga.partial; ra.Npart = ga.Npart;
    return ra;
}
int launch_gemm_big(const rml_svm* m, const GemmArgs& ga, hipStream_t st) { return launch_gemm_ring<0>(m, ring_args_from(ga), st); }
// the epilogue half of SmallArgs: dot products at G[m * g_sm + n * g_sn] -> partial sums
SmallArgs small_args_from(const GemmArgs& ga, int32_t* G, int64_t g_sm, int64_t g_sn) {
    SmallArgs sa{};
    sa.N = (int)ga.N; sa.Mpad = ga.Mpad; sa.tile_exact = ga.tile_exact; sa.G = G; sa.g_sm = g_sm; sa.g_sn = g_sn;
    sa.x_isum = ga.x_isum; sa.x_isq = ga.x_isq; sa.sv_term = ga.sv_term; sa.W = ga.W; sa.gs = ga.gs; sa.kernel = ga.kernel;
    sa.partial = ga.partial; sa.Npart = ga.Npart;
    return sa;
}
inline bool ring_takes(const rml_ctx* ctx, const rml_svm* m, int64_t n) { return use_big_gemm(m, n, ctx->num_cu, ctx->opt.gemm_big); }  // (its one caller)

// Rows per chunk of the chunked front doors.  Where the 256x256 ring kernel runs (an exact model, or the multi-digit path) a
// chunk costs ceil(tiles / CUs) rounds of one workgroup per CU, so the chunk size is chosen for the WHOLE batch: among the
// multiples of 256 rows in 4096..32768 the one with the fewest rounds in total (full chunks + the remainder) plus a small charge
// per chunk, the larger chunk on a tie.  Otherwise `fallback`.  RML_OPT_CHUNK overrides.
int64_t pick_chunk_opt(const rml_ctx* ctx, int64_t fallback) { return ctx->opt.chunk >= 128 ? round_up(ctx->opt.chunk, kTile) : fallback; }
int64_t pick_chunk(const rml_ctx* ctx, const rml_svm* m, int64_t rows, int64_t fallback, bool dig) {
    const int64_t env = pick_chunk_opt(ctx, 0);
    const int num_cu = ctx->num_cu;
    int64_t ch = fallback;
    if (env) ch = env;
    else if (dig || (m->exact && ring_takes(ctx, m, 32768))) {
        const int64_t st2 = (m->Mpad + kBig - 1) / kBig;
        auto rounds = [&](int64_t n) { return n <= 0 ? (int64_t)0 : (((n + kBig - 1) / kBig) * st2 + num_cu - 1) / num_cu; };
        // cost in units of a twentieth of a round: a chunk also costs its launches and a fill / drain in which the CUs run in
        // lockstep (measured: 1.97 rounds per launch 0.47-0.51 of peak, 2.99 rounds 0.54-0.58) -- three twentieths per chunk
        const int64_t total = round_up(rows, kBig);
        int64_t best = -1;
        // digit path: every launched workgroup parks two 256 KiB scratch tiles (carve: ring_grid x 512 KiB per workspace, times the
        // workspaces in rotation), so the chunk is also capped by a scratch budget of 1 GiB per workspace: 2048 tiles.  M = 2 560
        // is not touched (32 768 rows = 1 280 tiles); a 20 480-SV model stops at 6 400 rows instead of asking for 5 GiB
        const int64_t cmax = dig ? std::max<int64_t>(4096 / 4, std::min<int64_t>(32768, (2048 / st2) * kBig)) : 32768;
        for (int64_t c = std::min<int64_t>(4096, cmax); c <= cmax; c += kBig) {
            const int64_t nfull = total / c, rem = total % c;
            const int64_t cost = 20 * (nfull * rounds(c) + rounds(rem)) + 3 * (nfull + (rem ? 1 : 0));
            if (best < 0 || cost <= best) { best = cost; ch = c; }
            if (c >= total) break;
        }
    }
    return std::min<int64_t>(round_up(rows, kTile), ch);
}

// Workspace carved from the ctx block for one chunk of CH rows.
struct ChunkWs {
    uint8_t* q; float* f32; int32_t* isum; int64_t* isq; double* nsq; int32_t* flags;
    int32_t* tile_exact; int32_t* all_exact; double* partial;
    int8_t* dig; int64_t dig_plane; double* dnsq; int32_t* dflags;      // multi-digit operand of the general rows (or NULL)
    int32_t* stash;                                                     // scratch tiles of k_svm_gemm_ring<.., 1>
    int32_t* ijk;                                                       // derived (i,j,k) of the chunk's frames (fused derive -> slice), or NULL
    int32_t* gsmall;                                                    // [RML_SMALL_FRAMES][Mpad] dot products of the single-observation path
    int32_t* gsplit;                                                    // [Mpad][CH] of the split-K path (chunks of at most kSplitRows rows), or NULL
    uint32_t* occ;                                                      // [CH][occ_words] occupancy words of the code rows (ProjOut::occ), or NULL
    size_t bytes;
};

// what an entry point wants in a chunk workspace beside statistics, tile predicate and partial sums: code rows (+ the scratch of the
// small / split-K kernels), float rows, their digit planes (+ the ring kernel's scratch tiles), derived (i,j,k) per frame, occupancy
// words of the code rows
struct ChunkNeeds { bool q, f32, dig, ijk, occ; };
constexpr int64_t kSplitRows = 2048;        // the split-K path serves chunks of at most this many rows

// base == NULL: the size only (every pointer NULL).  A part that is not needed takes no bytes and is NULL.
ChunkWs carve(const rml_svm* m, int64_t CH, unsigned char* base, const ChunkNeeds& need) {
    ChunkWs w{}; size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return base && bytes ? base + o : (unsigned char*)nullptr; };
    w.q = (uint8_t*)take(need.q ? (size_t)CH * m->Dq : 0);
    w.f32 = (float*)take(need.f32 ? (size_t)CH * m->Df * 4 : 0);
    w.isum = (int32_t*)take((size_t)CH * 4); w.isq = (int64_t*)take((size_t)CH * 8);
    w.nsq = (double*)take((size_t)CH * 8); w.flags = (int32_t*)take((size_t)CH * 4);
    w.tile_exact = (int32_t*)take((size_t)(CH / kTile + 1) * 4); w.all_exact = (int32_t*)take(256);
    w.partial = (double*)take((size_t)(m->Mpad / kTile) * CH * m->PT * 8);
    w.dig_plane = CH * m->Dq;
    w.dig = (int8_t*)take(need.dig ? (size_t)4 * CH * m->Dq : 0);
    w.dnsq = (double*)take(need.dig ? (size_t)CH * 8 : 0); w.dflags = (int32_t*)take(need.dig ? (size_t)CH * 4 : 0);
    w.stash = (int32_t*)take(need.dig ? (size_t)ring_grid((int)((CH + kBig - 1) / kBig), (int)((m->Mpad + kBig - 1) / kBig)) * 2 * kDigStashBytes : 0);
    w.ijk = (int32_t*)take(need.ijk ? (size_t)CH * 12 : 0);
    w.gsmall = (int32_t*)take(need.q ? (size_t)RML_SMALL_FRAMES * m->Mpad * 4 : 0);
    w.gsplit = (int32_t*)take(need.q && CH <= kSplitRows ? (size_t)m->Mpad * CH * 4 : 0);
    w.occ = (uint32_t*)take(need.q && need.occ ? (size_t)CH * m->occ_words * 4 : 0);
    w.bytes = off;
    return w;
}

// the only caller of carve: size -> rml_ws_reserve -> w[0..nbuf) back to back, then `extra` bytes of the caller's own at *extra_at
int reserve_chunks(rml_ctx* ctx, const rml_svm* m, int64_t CH, const ChunkNeeds& need, hipStream_t st, ChunkWs* w, int nbuf,
                   size_t extra = 0, void** extra_at = nullptr) {
    const size_t each = carve(m, CH, nullptr, need).bytes;
    void* ws = nullptr;
    if (int rc = rml_ws_reserve(ctx, (size_t)nbuf * each + extra, &ws, st)) return rc;
    unsigned char* base = static_cast<unsigned char*>(ws);
    for (int i = 0; i < nbuf; ++i) w[i] = carve(m, CH, base + (size_t)i * each, need);
    if (extra_at) *extra_at = base + (size_t)nbuf * each;
    return RML_OK;
}

struct DecisionOut {
    double* dec_ovo; double* dec_ovr; double* proba; int32_t* label_vote; int32_t* label_calib;
    DecisionOut at(int64_t r0, int C, int P) const {       // the outputs of rows r0...
        auto adv = [r0](auto* p, int64_t per_row) { return p ? p + r0 * per_row : p; };
        return DecisionOut{adv(dec_ovo, P), adv(dec_ovr, C == 2 ? 1 : C), adv(proba, C), adv(label_vote, 1), adv(label_calib, 1)};
    }
};

// The n rows of one chunk, already in place: code rows + their statistics (q NULL: none), per row "on the code grid?" (NULL: not
// known per row), float rows of stride m->Df + squared norms (f32 NULL: none).  ws_rows: the first n rows of a chunk workspace.
// occ: the occupancy words of the code rows (m->occ_words per row) when the chunk's producer wrote them, else NULL.
// holes: the producer did not store the lines whose bit is clear (ProjOut::skip_clear): only a sparse plan may read these rows.
struct ChunkOps { int64_t n; const uint8_t* q; int64_t ld_q; const int32_t* isum; const int64_t* isq; const int32_t* flags; const float* f32; const double* nsq;
                  const uint32_t* occ; bool holes; };
ChunkOps ws_rows(const rml_svm* m, const ChunkWs& w, int64_t n) { return ChunkOps{n, w.q, m->Dq, w.isum, w.isq, w.flags, w.f32, w.nsq, nullptr, false}; }

// What to do with a chunk.  The entry point fills the first group (a ChunkPlan{} asks for nothing: set what is meant, by name);
// plan_chunk derives the second from it, and is the only place that does.
struct ChunkPlan {
    int policy;             // RML_PATH_AUTO (i8 on exact tiles, f64 elsewhere) / _F32 / _I8 / _F64 / _DIGITS (forced)
    bool tiles_done;        // w.tile_exact is already decided (launch_tile_flags at plan_chunk's group): run_chunk launches no flag kernel
    bool all_exact_known;   // every row is on the code grid by construction (uint8 volumes): no tile predicate at all
    bool allow_big;         // the 256x256 ring kernel may take the exact tiles (not beside a persistent projection: it fills a CU)
    bool dig_ready;         // the digit planes of the float rows are in w.dig
    double* kmat; int64_t ld_k;     // kernel values K[n][m] of the chunk's rows instead of decisions (rml_svm_kernel_matrix), or NULL
    int FT, ST, group; bool run_i8, run_gen, gen_f32, big, run_dig, small, split, sparse;      // derived: see plan_chunk
};

// No allocation, no lock, no HIP call: run_chunk is entered with a const ctx and from inside a stream capture.
ChunkPlan plan_chunk(const rml_ctx* ctx, const rml_svm* m, ChunkPlan p, const ChunkOps& x, const ChunkWs& w) {
    p.FT = (int)((x.n + kTile - 1) / kTile); p.ST = (int)(m->Mpad / kTile);             // sample tiles, SV tiles
    p.run_i8 = m->exact && x.q && (p.policy == RML_PATH_AUTO || p.policy == RML_PATH_I8);
    p.run_gen = x.f32 && p.policy != RML_PATH_I8; p.gen_f32 = (p.policy == RML_PATH_F32);
    // large exact batches go to the 256x256 kernel; the tile predicate is then decided per pair of 128-sample tiles
    p.big = p.allow_big && p.run_i8 && !p.kmat && ring_takes(ctx, m, x.n);
    // general tiles whose rows fit the model's fixed-point range go to the multi-digit int8 kernel (digit planes in w.dig)
    p.run_dig = p.dig_ready && w.dig && p.run_gen && !p.gen_f32 && !p.kmat && m->dig_ok;
    p.group = (p.big || p.run_dig) ? 2 : 1;             // sample tiles per entry of the tile predicate
    // a handful of rows: the matrix-vector kernels (the SV codes read once by the whole chip instead of by Mpad / 128 workgroups)
    p.small = p.run_i8 && !p.kmat && x.n <= RML_SMALL_FRAMES && w.gsmall && (m->Mpad % kSmallSv) == 0;
    // ... and batches whose 128 x 128 tiles are fewer than the CUs: the same tiles cut along K (exact: any order)
    p.split = p.run_i8 && !p.kmat && !p.small && !p.big && w.gsplit && x.n <= kSplitRows && (int64_t)p.FT * p.ST < ctx->num_cu &&
              m->Kq / kStepBytes >= 8;
    // the 128 x 128 kernel stages all-background lines from the context's constant line when the chunk's producer wrote occupancy
    // words (the model's come from rml_svm_load).  The ring, split-K and small kernels, the kernel matrix and the float paths are dense.
    // Forced (RML_OPT_SPARSE_ROWS = 1) it also takes the chunks split-K would: the same bits (both are exact), and the tests reach it
    // with a few hundred rows.
    const bool can_sparse = p.run_i8 && !p.kmat && !p.small && !p.big && x.occ && m->sv_occ && ctx->bg_line && ctx->opt.sparse_rows != 0 &&
                            m->occ_words <= kSparseMaxWords;
    if (can_sparse && ctx->opt.sparse_rows > 0) p.split = false;
    p.sparse = can_sparse && !p.split;
    return p;
}

// the tile predicate of a chunk at the plan's granularity; with all_exact ONE MORE block that writes the AND of every row flag there
void launch_tile_flags(const rml_svm* m, const ChunkOps& x, const ChunkPlan& p, const ChunkWs& w, int32_t* all_exact, hipStream_t st) {
    const int blocks = (p.FT + p.group - 1) / p.group + (all_exact ? 1 : 0);
    hipLaunchKernelGGL(k_tile_flags, dim3(blocks), dim3(128 * p.group), 0, st, x.flags, x.n, p.FT, p.run_i8 ? (p.run_gen ? 0 : 2) : 1,
                       (int)m->exact, w.tile_exact, all_exact, p.group);
}
void launch_tile_dig(const ChunkOps& x, const ChunkPlan& p, const ChunkWs& w, hipStream_t st) {
    hipLaunchKernelGGL(k_tile_dig, dim3((p.FT + 1) / 2), dim3(256), 0, st, w.dflags, x.n, p.FT, w.tile_exact, (const int32_t*)nullptr);
}
// digit planes of the n float rows in w.f32
void launch_digit_rows(const rml_svm* m, const ChunkWs& w, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_digit_rows, dim3((unsigned)n), dim3(256), 0, st, w.f32, m->Df, m->D, m->Dq, w.dig_plane, w.dig, w.dnsq,
                       w.dflags, m->dig_c0, 2147483648.0 / m->dig_s, (const int32_t*)nullptr);
}

// the epilogue of a chunk: partial sums of every SV tile -> decision values, votes, calibrated probabilities, labels
int run_finish(const rml_svm* m, const ChunkOps& x, const ChunkPlan& p, const ChunkWs& w, const DecisionOut& out, hipStream_t st) {
    FinishArgs fa{};
    fa.partial = w.partial; fa.Npart = x.n; fa.ST = p.ST; fa.PT = m->PT; fa.N = x.n; fa.C = m->C; fa.P = m->P;
    fa.intercept = m->intercept; fa.calib = m->calib; fa.has_calib = m->has_calib;
    fa.row_flags = p.all_exact_known ? nullptr : x.flags; fa.tile_exact = p.all_exact_known ? nullptr : w.tile_exact;
    fa.forced_i8 = p.run_i8 && !p.run_gen;
    fa.dec_ovo = out.dec_ovo; fa.dec_ovr = out.dec_ovr; fa.proba = out.proba; fa.label_vote = out.label_vote; fa.label_calib = out.label_calib;
    hipLaunchKernelGGL(k_svm_finish, dim3((unsigned)((x.n + 255) / 256)), dim3(256), 0, st, fa);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

int launch_epi(const rml_svm* m, const SmallArgs& sa, int ST, int64_t n, hipStream_t st) {
    const dim3 ge((unsigned)ST, (unsigned)n);
    switch (m->PT) {
        case 1: hipLaunchKernelGGL(k_svm_epi_small<1>, ge, dim3(128), 0, st, sa); break;
        case 3: hipLaunchKernelGGL(k_svm_epi_small<3>, ge, dim3(128), 0, st, sa); break;
        case 6: hipLaunchKernelGGL(k_svm_epi_small<6>, ge, dim3(128), 0, st, sa); break;
        case 10: hipLaunchKernelGGL(k_svm_epi_small<10>, ge, dim3(128), 0, st, sa); break;
        case 15: hipLaunchKernelGGL(k_svm_epi_small<15>, ge, dim3(128), 0, st, sa); break;
        default: RML_REQUIRE(false, RML_ERR_UNSUPPORTED, "svm: unsupported pair count");
    }
    RML_HIP(hipGetLastError());
    return RML_OK;
}

// the exact path for n <= RML_SMALL_FRAMES rows: k_svm_dot_small + k_svm_epi_small (bit-identical partial sums: see the kernels)
int launch_small(const rml_svm* m, const GemmArgs& ga, int32_t* G, hipStream_t st) {
    SmallArgs sa = small_args_from(ga, G, 1, ga.Mpad);
    sa.sv = ga.sv; sa.ld_sv = ga.ld_sv; sa.x = ga.x; sa.ld_x = ga.ld_x; sa.Kb = (int64_t)ga.KT * kStepBytes;
    const dim3 gd((unsigned)(ga.Mpad / kSmallSv));
    if (ga.N <= 1) hipLaunchKernelGGL(k_svm_dot_small<1>, gd, dim3(256), 0, st, sa);
    else if (ga.N <= 2) hipLaunchKernelGGL(k_svm_dot_small<2>, gd, dim3(256), 0, st, sa);
    else if (ga.N <= 4) hipLaunchKernelGGL(k_svm_dot_small<4>, gd, dim3(256), 0, st, sa);
    else hipLaunchKernelGGL(k_svm_dot_small<8>, gd, dim3(256), 0, st, sa);
    return launch_epi(m, sa, ga.ST, ga.N, st);
}

// the exact path for batches whose tiles do not fill the machine: split-K tile kernel + the chain epilogue (see k_svm_gemm_splitk)
int launch_split(const rml_svm* m, const GemmArgs& ga, int32_t* G, int num_cu, hipStream_t st) {
    const int64_t ldg = (int64_t)ga.FT * kTile;
    // (a kernel, not hipMemsetAsync: the memset of a captured stream was not replayed with the graph -- the second replay added
    // onto the first one's sums, tests/test_capi_gpu.py)
    const int64_t n16 = ga.Mpad * ldg / 4;                 // Mpad and ldg are multiples of 128
    hipLaunchKernelGGL(k_zero16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<v4i*>(G), n16);
    SplitArgs sp{};
    sp.sv = ga.sv; sp.ld_sv = ga.ld_sv; sp.x = ga.x; sp.ld_x = ga.ld_x; sp.KT = ga.KT; sp.N = ga.N; sp.FT = ga.FT;
    sp.tile_exact = ga.tile_exact; sp.G = G; sp.ldg = ldg;
    const int tiles = ga.FT * ga.ST;
    int KS = (2 * num_cu + tiles - 1) / tiles;            // about two workgroups per CU
    if (KS > ga.KT / 4) KS = ga.KT / 4;                   // at least four K-steps per range
    if (KS < 1) KS = 1;
    sp.per = (ga.KT + KS - 1) / KS;
    KS = (ga.KT + sp.per - 1) / sp.per;
    hipLaunchKernelGGL(k_svm_gemm_splitk, dim3((unsigned)tiles, (unsigned)KS), dim3(256), 0, st, sp);
    return launch_epi(m, small_args_from(ga, G, ldg, 1), ga.ST, ga.N, st);
}

// the multi-digit operands of a chunk: the model's digit planes against w.dig, general tiles only (tile_exact == 2)
RingArgs digit_args(const rml_svm* m, const ChunkOps& x, const ChunkPlan& p, const ChunkWs& w) {
    RingArgs ra{};
    ra.sv = reinterpret_cast<const uint8_t*>(m->sv_dig); ra.x = reinterpret_cast<const uint8_t*>(w.dig);
    ra.ld_sv = m->Dq; ra.ld_x = m->Dq; ra.sv_plane = m->Mpad * m->Dq; ra.x_plane = w.dig_plane;
    ra.KT = (int)(m->Kq / kStepBytes); ra.N = x.n; ra.Mpad = m->Mpad; ra.sv_rows = m->Mpad; ra.ST = p.ST; ra.FT = p.FT;
    ra.tile_exact = w.tile_exact; ra.want = 2; ra.x_nsq = w.dnsq; ra.sv_term = m->sv_dig_nsq; ra.W = m->W;
    ra.gs = m->gamma * m->dig_s * m->dig_s; ra.kernel = RML_KERNEL_RBF; ra.partial = w.partial; ra.Npart = x.n; ra.stash = w.stash;
    return ra;
}

// GEMM(s) + finish for one chunk whose operands are already in place.
int run_chunk(const rml_ctx* ctx, const rml_svm* m, const ChunkOps& x, const ChunkPlan& asked, const ChunkWs& w, const DecisionOut& out,
              hipStream_t st) {
    const ChunkPlan p = plan_chunk(ctx, m, asked, x, w);
    RML_REQUIRE(p.run_i8 || p.run_gen, RML_ERR_STATE, "svm: no usable operand path (model exact=%d)", (int)m->exact);
    // every kernel but the sparse 128 x 128 GEMM reads whole code rows (tile flags, finish and the float paths read none)
    RML_REQUIRE(!(x.holes && !p.sparse), RML_ERR_STATE, "svm: code rows with unstored background lines reached a dense plan");
    if (!p.tiles_done) {
        launch_tile_flags(m, x, p, w, nullptr, st);
        if (p.run_dig) launch_tile_dig(x, p, w, st);
    }
    GemmArgs ga{};
    ga.N = x.n; ga.ST = p.ST; ga.FT = p.FT; ga.tile_exact = p.all_exact_known ? nullptr : w.tile_exact;
    ga.W = m->W; ga.Mpad = m->Mpad; ga.kernel = m->kernel; ga.partial = w.partial; ga.Npart = x.n;
    ga.kmat = p.kmat; ga.ld_k = p.ld_k; ga.M = m->M; ga.sv_rows = m->Mpad;
    int rc = RML_OK;
    if (p.run_i8) {
        ga.sv = m->sv_q; ga.ld_sv = m->Dq; ga.x = x.q; ga.ld_x = x.ld_q; ga.KT = (int)(m->Kq / kStepBytes);
        ga.want = 1; ga.x_isum = x.isum; ga.x_isq = x.isq; ga.sv_term = m->sv_term_q;
        ga.gs = (m->kernel == RML_KERNEL_RBF ? m->gamma : 1.0) / (m->code_scale * m->code_scale);
        if (p.kmat) rc = launch_gemm<PATH_I8, true>(m, ga, st);
        else if (p.small) rc = launch_small(m, ga, w.gsmall, st);
        else if (p.split) rc = launch_split(m, ga, w.gsplit, ctx->num_cu, st);
        else if (p.big) rc = launch_gemm_big(m, ga, st);
        else if (p.sparse) {
            ga.sv_occ = m->sv_occ; ga.x_occ = x.occ; ga.ow = m->occ_words; ga.bg_line = ctx->bg_line;
            ++ctx->sparse_gemm_launches;
            rc = launch_gemm<PATH_I8, false, true>(m, ga, st);
        } else rc = launch_gemm<PATH_I8>(m, ga, st);
        if (rc) return rc;
    }
    if (p.run_dig && (rc = launch_gemm_ring<1>(m, digit_args(m, x, p, w), st))) return rc;
    if (p.run_gen) {
        ga.sv = reinterpret_cast<const uint8_t*>(m->sv_f32); ga.ld_sv = m->Df * 4;
        ga.x = reinterpret_cast<const uint8_t*>(x.f32); ga.ld_x = m->Df * 4; ga.KT = (int)(m->Kf * 4 / kStepBytes);
        ga.want = 0; ga.x_nsq = x.nsq; ga.sv_term = m->sv_nsq; ga.gs = m->gamma;
        rc = p.gen_f32 ? launch_gemm<PATH_F32>(m, ga, st)
                       : (p.kmat ? launch_gemm<PATH_F64, true>(m, ga, st) : launch_gemm<PATH_F64>(m, ga, st));
        if (rc) return rc;
    }
    if (p.kmat) { RML_HIP(hipGetLastError()); return RML_OK; }      // kernel values only
    return run_finish(m, x, p, w, out, st);
}
}  // namespace

// ---- model load ---------------------------------------------------------------------------
// The host half of rml_svm_load: validation, geometry and every packed operand, no HIP call (the sanitizer build of
// tools/sanitize drives it on a box without a GPU).  Fills the geometry / flags of *m and the arrays of *pk.
int rml_svm_pack_host(const double* sv, int64_t M, int64_t D, const double* dual_coef, const int32_t* n_support,
                      int n_classes, int kernel, double gamma, double code_scale, bool has_calib, rml_svm* m, rml_svm_pack* pk) {
    RML_REQUIRE(sv && dual_coef && n_support && m && pk, RML_ERR_INVALID, "rml_svm_load: NULL argument");
    RML_REQUIRE(M > 0 && D > 0, RML_ERR_INVALID, "rml_svm_load: empty model");
    RML_REQUIRE(n_classes >= 2 && n_classes <= kMaxC, RML_ERR_UNSUPPORTED, "rml_svm_load: %d classes (supported: 2..%d)", n_classes, kMaxC);
    RML_REQUIRE(kernel == RML_KERNEL_RBF || kernel == RML_KERNEL_LINEAR, RML_ERR_UNSUPPORTED, "rml_svm_load: kernel %d", kernel);
    int64_t msum = 0;
    for (int c = 0; c < n_classes; ++c) { RML_REQUIRE(n_support[c] >= 0, RML_ERR_INVALID, "rml_svm_load: negative n_support"); msum += n_support[c]; }
    RML_REQUIRE(msum == M, RML_ERR_INVALID, "rml_svm_load: sum(n_support)=%lld != M=%lld", (long long)msum, (long long)M);
    m->M = M; m->D = D; m->C = n_classes; m->P = n_classes * (n_classes - 1) / 2;
    m->PT = m->P <= 1 ? 1 : (m->P <= 3 ? 3 : (m->P <= 6 ? 6 : (m->P <= 10 ? 10 : 15)));
    m->kernel = kernel; m->gamma = gamma; m->code_scale = code_scale > 1.0 ? code_scale : 1.0;
    m->Mpad = round_up(M, kTile);
    m->Kq = round_up(D, kStepBytes); m->Kf = round_up(D, 32);
    m->Dq = ((m->Kq / 128) & 1) ? m->Kq : m->Kq + 128;
    m->Df = ((m->Kf / 32) & 1) ? m->Kf : m->Kf + 32;
    m->has_calib = has_calib;

    // per-pair SV weights: the pair loop of svm_predict_values (svm.cpp:2864-2883)
    std::vector<double>& W = pk->W;
    W.assign((size_t)m->PT * m->Mpad, 0.0);
    {
        std::vector<int64_t> start(n_classes, 0);
        for (int c = 1; c < n_classes; ++c) start[c] = start[c - 1] + n_support[c - 1];
        int p = 0;
        for (int i = 0; i < n_classes; ++i)
            for (int j = i + 1; j < n_classes; ++j, ++p) {
                for (int64_t k = 0; k < n_support[i]; ++k) W[(size_t)p * m->Mpad + start[i] + k] = dual_coef[(size_t)(j - 1) * M + start[i] + k];
                for (int64_t k = 0; k < n_support[j]; ++k) W[(size_t)p * m->Mpad + start[j] + k] = dual_coef[(size_t)i * M + start[j] + k];
            }
    }
    // float operand + norms
    std::vector<float>& svf = pk->svf;
    std::vector<double>& nsq = pk->nsq;
    svf.assign((size_t)m->Mpad * m->Df, 0.0f);
    nsq.assign(m->Mpad, 0.0);
    // exact codes: every SV must be bit-identical to float32(c/scale) (or to c when unscaled)
    std::vector<uint8_t>& svq = pk->svq;
    std::vector<double>& term = pk->term;
    svq.assign((size_t)m->Mpad * m->Dq, 0);
    term.assign(m->Mpad, 0.0);
    bool exact = true;
    const float fscale = (float)m->code_scale;
    for (int64_t r = 0; r < M; ++r) {
        double nn = 0.0; int64_t isum = 0, isq = 0;
        for (int64_t d = 0; d < D; ++d) {
            const double v = sv[(size_t)r * D + d];
            const float vf = (float)v;
            svf[(size_t)r * m->Df + d] = vf;
            nn += (double)vf * (double)vf;
            if (exact) {
                double c = nearbyint(v * m->code_scale);
                bool good = c >= 0.0 && c <= 255.0;
                if (good) {
                    double back = m->code_scale > 1.0 ? (double)((float)c / fscale) : c;
                    good = (back == v);
                }
                if (!good) exact = false;
                else { int ci = (int)c; svq[(size_t)r * m->Dq + d] = (uint8_t)(ci ^ 0x80); isum += ci; isq += (int64_t)ci * ci; }
            }
        }
        nsq[r] = nn;
        // RBF:    d^2 = (isq_x - 256 isum_x) + [isq_s - 256 isum_s + 32768 D] - 2 G'
        // linear: x.s = G' + 128 isum_x + [128 isum_s - 16384 D]
        term[r] = (kernel == RML_KERNEL_RBF) ? (double)(isq - 256 * isum + 32768 * D) : (double)(128 * isum - 16384 * D);
    }
    // occupancy words of the code rows (ProjOut::occ's rule): a line is clear when all of its 128 bytes are the background code 0x80
    // and it lies wholly inside D.  Rows M .. Mpad hold 0x00 (int8 0, not the background code) and stay occupied.
    m->occ_words = (int)((m->Kq / kStepBytes + 31) / 32);
    std::vector<uint32_t>& occ = pk->occ;
    occ.assign((size_t)m->Mpad * m->occ_words, 0u);
    for (int64_t r = 0; r < m->Mpad; ++r)
        for (int64_t k = 0; k < m->Kq / kStepBytes; ++k) {
            bool bg = r < M && (k + 1) * kStepBytes <= D;
            for (int t = 0; bg && t < kStepBytes; ++t) bg = svq[(size_t)r * m->Dq + k * kStepBytes + t] == 0x80;
            if (!bg) occ[(size_t)r * m->occ_words + (k >> 5)] |= 1u << (k & 31);
        }
    // the int8 MFMA accumulates sum (a-128)(b-128) in int32: |.| <= 128^2 * K must stay below 2^31
    if (m->Kq >= 131072) exact = false;
    m->exact = exact;
    // multi-digit frame for general rows: u = (v - c0) / s with s the power of two >= the SV value range (SVs then sit in
    // [-1/2, 1/2] + rounding of c0; rows may leave the SV range by s/2 on either side before they fall back to float64) and
    // c0 the mid-range on a grid of s/256 (so that v - c0 is exact in float64 for float32 v).  Four digit groups share one
    // int32 accumulator: 4 * 128^2 * K < 2^31.
    std::vector<int8_t>& svd = pk->svd;
    std::vector<double>& dnsq = pk->dnsq;
    svd.clear(); dnsq.clear();
    m->dig_ok = false;
    if (kernel == RML_KERNEL_RBF && m->Kq < 32768 && m->PT <= 6) {
        double lo = sv[0], hi = sv[0];
        bool finite = true;
        for (size_t i = 0; i < (size_t)M * D; ++i) { const double v = sv[i]; finite &= std::isfinite(v); lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        if (finite && hi > lo) {
            int e = 0;
            (void)frexp(hi - lo, &e);                             // hi - lo = f 2^e, f in [0.5, 1)
            double sd = ldexp(1.0, e);
            if (ldexp(1.0, e - 1) == hi - lo) sd = hi - lo;       // an exact power of two is its own scale
            const double c0 = nearbyint(0.5 * (lo + hi) / sd * 256.0) / 256.0 * sd;
            const double k31 = 2147483648.0 / sd;
            svd.assign((size_t)4 * m->Mpad * m->Dq, 0);
            dnsq.assign(m->Mpad, 0.0);
            const size_t plane = (size_t)m->Mpad * m->Dq;
            bool ok = true;
            for (int64_t r = 0; r < M && ok; ++r) {
                double nn = 0.0;
                for (int64_t d = 0; d < D; ++d) {
                    const double t = nearbyint((sv[(size_t)r * D + d] - c0) * k31);
                    if (!(t >= -2147483648.0 && t <= 2139062143.0)) { ok = false; break; }
                    const int32_t I = (int32_t)t;
                    const double u = (double)I * 0x1p-31;
                    nn += u * u;
                    const uint32_t pk4 = ((uint32_t)I + 0x00808080u) ^ 0x00808080u;     // bytes = balanced digits, a0 on top
                    for (int dg = 0; dg < 4; ++dg) svd[(size_t)dg * plane + (size_t)r * m->Dq + d] = (int8_t)((pk4 >> (8 * (3 - dg))) & 255u);
                }
                dnsq[r] = nn;
            }
            if (ok) { m->dig_ok = true; m->dig_c0 = c0; m->dig_s = sd; }
        }
    }
    return RML_OK;
}

extern "C" int rml_svm_load(rml_ctx* ctx, const double* sv, int64_t M, int64_t D,
                            const double* dual_coef, const double* intercept, const int32_t* n_support,
                            int n_classes, int kernel, double gamma, double code_scale,
                            const double* calib_a, const double* calib_b, rml_svm** out) {
    RML_REQUIRE(ctx && sv && dual_coef && intercept && n_support && out, RML_ERR_INVALID, "rml_svm_load: NULL argument");
    RML_REQUIRE((calib_a == nullptr) == (calib_b == nullptr), RML_ERR_INVALID, "rml_svm_load: calib_a/calib_b must both be given");
    *out = nullptr;
    rml_svm* m = new (std::nothrow) rml_svm();
    RML_REQUIRE(m != nullptr, RML_ERR_NOMEM, "rml_svm_load: out of host memory");
    rml_svm_pack pk;
    int rc = rml_svm_pack_host(sv, M, D, dual_coef, n_support, n_classes, kernel, gamma, code_scale, calib_a != nullptr, m, &pk);
    if (rc) { delete m; return rc; }
    {
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) { delete m; RML_HIP(e); }
    }
    const bool exact = m->exact;
    do {
        if ((rc = dev_upload(&m->W, pk.W))) break;
        if ((rc = dev_upload(&m->sv_f32, pk.svf))) break;
        if ((rc = dev_upload(&m->sv_nsq, pk.nsq))) break;
        if (exact) {
            if ((rc = dev_upload(&m->sv_q, pk.svq))) break;
            if ((rc = dev_upload(&m->sv_term_q, pk.term))) break;
            if ((rc = dev_upload(&m->sv_occ, pk.occ))) break;
        }
        if (m->dig_ok) {
            if ((rc = dev_upload(&m->sv_dig, pk.svd))) break;
            if ((rc = dev_upload(&m->sv_dig_nsq, pk.dnsq))) break;
        }
        std::vector<double> ic(intercept, intercept + m->P);
        if ((rc = dev_upload(&m->intercept, ic))) break;
        if (m->has_calib) {
            std::vector<double> cal(2 * n_classes);
            const int ncal = n_classes == 2 ? 1 : n_classes;
            for (int c = 0; c < n_classes; ++c) { cal[c] = c < ncal ? calib_a[c] : 0.0; cal[n_classes + c] = c < ncal ? calib_b[c] : 0.0; }
            if ((rc = dev_upload(&m->calib, cal))) break;
        }
    } while (0);
    if (rc) { rml_svm_free(ctx, m); return rc; }
    *out = m;
    return RML_OK;
}

extern "C" int rml_svm_free(rml_ctx* ctx, rml_svm* m) {
    if (!m) return RML_OK;
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    void* bufs[] = {m->sv_f32, m->sv_nsq, m->sv_q, m->sv_term_q, m->W, m->intercept, m->calib, m->platt, m->sv_dig, m->sv_dig_nsq, m->sv_occ};
    for (void* b : bufs) if (b) (void)hipFree(b);
    delete m;
    return RML_OK;
}

extern "C" int rml_svm_sv_occupancy(rml_ctx* ctx, const rml_svm* m, uint32_t* out, int64_t n_words) {
    RML_REQUIRE(ctx && m && out, RML_ERR_INVALID, "rml_svm_sv_occupancy: NULL argument");
    RML_REQUIRE(m->sv_occ != nullptr, RML_ERR_STATE, "rml_svm_sv_occupancy: the model is not on the code grid");
    RML_REQUIRE(n_words == m->Mpad * m->occ_words, RML_ERR_INVALID, "rml_svm_sv_occupancy: out holds %lld words, the model has %lld",
                (long long)n_words, (long long)(m->Mpad * m->occ_words));
    RML_HIP(hipSetDevice(ctx->device));
    RML_HIP(hipMemcpy(out, m->sv_occ, (size_t)n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RML_OK;
}
extern "C" int64_t rml_ctx_sparse_gemm_launches(const rml_ctx* ctx) { return ctx ? ctx->sparse_gemm_launches : 0; }
extern "C" int64_t rml_ctx_sparse_store_launches(const rml_ctx* ctx) { return ctx ? ctx->sparse_store_launches : 0; }
extern "C" int rml_svm_is_exact(const rml_svm* m) { return m && m->exact ? 1 : 0; }
extern "C" int64_t rml_svm_num_sv(const rml_svm* m) { return m ? m->M : 0; }
extern "C" int64_t rml_svm_dim(const rml_svm* m) { return m ? m->D : 0; }

// the size of one chunk workspace (tools/sanitize pins the layout with it).  needs: bit 0 code rows, 1 float rows, 2 digit planes, 3 ijk,
// 4 occupancy words
size_t rml_svm_ws_bytes(const rml_svm* m, int64_t CH, unsigned needs) {
    return carve(m, CH, nullptr, ChunkNeeds{(needs & 1u) != 0, (needs & 2u) != 0, (needs & 4u) != 0, (needs & 8u) != 0, (needs & 16u) != 0}).bytes;
}

// ---- decision on caller-provided rows -----------------------------------------------------
namespace {
// float rows of a caller, chunk by chunk: k_prepare_rows (and the digit planes, where the workspace has room for them) into w, then
// run_chunk; with plan.kmat the kernel values of the rows instead of decisions
int run_float_rows(const rml_ctx* ctx, const rml_svm* m, const float* feat, int64_t ld_feat, int64_t N, int64_t CH, const ChunkWs& w,
                   const ChunkPlan& plan, const DecisionOut& out, hipStream_t st) {
    for (int64_t r0 = 0; r0 < N; r0 += CH) {
        const int64_t n = std::min(CH, N - r0);
        hipLaunchKernelGGL(k_prepare_rows, dim3((unsigned)n), dim3(256), 0, st, feat + r0 * ld_feat, ld_feat, m->D,
                           (float)m->code_scale, w.f32, m->Df, w.nsq, w.q, m->Dq, w.isum, w.isq, w.flags);
        if (w.dig) launch_digit_rows(m, w, n, st);
        RML_HIP(hipGetLastError());
        ChunkPlan p = plan; if (p.kmat) p.kmat += r0 * p.ld_k;
        if (int rc = run_chunk(ctx, m, ws_rows(m, w, n), p, w, out.at(r0, m->C, m->P), st)) return rc;
    }
    return RML_OK;
}
}  // namespace

extern "C" int rml_svm_decision(rml_ctx* ctx, const rml_svm* m, int path,
                                const float* feat, int64_t ld_feat,
                                const uint8_t* feat_q, int64_t ld_q, const int32_t* row_isum, const int64_t* row_isq,
                                const int32_t* row_flags, int64_t N,
                                double* dec_ovo, double* dec_ovr, double* proba,
                                int32_t* label_vote, int32_t* label_calib, void* stream) {
    RML_REQUIRE(ctx && m && N >= 0, RML_ERR_INVALID, "rml_svm_decision: bad arguments");
    if (N == 0) return RML_OK;
    RML_REQUIRE(feat || feat_q, RML_ERR_INVALID, "rml_svm_decision: need feat or feat_q");
    RML_REQUIRE(!feat || ld_feat >= m->D, RML_ERR_INVALID, "rml_svm_decision: ld_feat < D");
    RML_REQUIRE(path >= RML_PATH_AUTO && path <= RML_PATH_DIGITS, RML_ERR_INVALID, "rml_svm_decision: bad path %d", path);
    RML_REQUIRE(path != RML_PATH_DIGITS || m->dig_ok, RML_ERR_STATE, "rml_svm_decision: multi-digit path requested but the model has no digit frame "
                "(RBF kernel, D < 32768 and at most 6 class pairs)");
    RML_REQUIRE(!(proba || label_calib) || m->has_calib, RML_ERR_STATE, "rml_svm_decision: model has no calibrators");
    RML_REQUIRE(path != RML_PATH_I8 || m->exact, RML_ERR_STATE, "rml_svm_decision: exact path requested but the model is not on the code grid");
    if (!feat) {
        RML_REQUIRE(m->exact, RML_ERR_STATE, "rml_svm_decision: code rows given but the model is not on the code grid");
        RML_REQUIRE(path == RML_PATH_AUTO || path == RML_PATH_I8, RML_ERR_INVALID, "rml_svm_decision: the float paths need float rows");
        RML_REQUIRE(row_isum && row_isq, RML_ERR_INVALID, "rml_svm_decision: code rows need row_isum/row_isq");
        RML_REQUIRE(ld_q >= m->Kq && ld_q % 16 == 0 && (reinterpret_cast<uintptr_t>(feat_q) & 15) == 0, RML_ERR_INVALID,
                    "rml_svm_decision: code rows need ld_q >= %lld, ld_q %% 16 == 0 and 16-byte alignment", (long long)m->Kq);
    }
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);           // shared workspace
    const DecisionOut out{dec_ovo, dec_ovr, proba, label_vote, label_calib};
    // float rows: the multi-digit kernel takes the rows off the code grid when the batch fills enough 256 x 256 tiles (a model on
    // the grid can meet such rows as well -- mixed batches: digit planes then ride along with the codes); a model that is not on
    // the grid then has chunks sized for whole rounds of one workgroup per CU, like the exact 256 x 256 kernel's.
    // The caller's code rows are taken as they are: the workspace holds the tile predicate and the partial sums only
    ChunkNeeds need{};
    need.q = feat && m->exact && (path == RML_PATH_AUTO || path == RML_PATH_I8); need.f32 = feat != nullptr;
    need.dig = feat && use_dig_gemm(m, path, N, ctx->num_cu);
    const bool dig_rounds = need.dig && !m->exact;
    const int64_t CH = (dig_rounds || m->exact) ? pick_chunk(ctx, m, N, 8192, dig_rounds) : std::min<int64_t>(round_up(N, kTile), 8192);
    ChunkWs w; int rc = reserve_chunks(ctx, m, CH, need, st, &w, 1);
    if (rc) return rc;
    ChunkPlan plan{};
    plan.policy = feat ? path : RML_PATH_I8; plan.allow_big = true; plan.dig_ready = need.dig;
    if (feat) return run_float_rows(ctx, m, feat, ld_feat, N, CH, w, plan, out, st);
    for (int64_t r0 = 0; r0 < N && !rc; r0 += CH) {
        const ChunkOps x{std::min(CH, N - r0), feat_q + r0 * ld_q, ld_q, row_isum + r0, row_isq + r0, row_flags ? row_flags + r0 : nullptr,
                         nullptr, nullptr};
        rc = run_chunk(ctx, m, x, plan, w, out.at(r0, m->C, m->P), st);
    }
    return rc;
}

// ---- kernel matrix K(X, SV): the Gram-matrix service for SVC training with kernel='precomputed' -------------
extern "C" int rml_svm_kernel_matrix(rml_ctx* ctx, const rml_svm* m, int path, const float* feat, int64_t ld_feat, int64_t N,
                                     double* kmat, int64_t ld_k, void* stream) {
    RML_REQUIRE(ctx && m && N >= 0, RML_ERR_INVALID, "rml_svm_kernel_matrix: bad arguments");
    if (N == 0) return RML_OK;
    RML_REQUIRE(feat && kmat, RML_ERR_INVALID, "rml_svm_kernel_matrix: NULL argument");
    RML_REQUIRE(ld_feat >= m->D && ld_k >= m->M, RML_ERR_INVALID, "rml_svm_kernel_matrix: ld_feat < D or ld_k < M");
    RML_REQUIRE(path == RML_PATH_AUTO || path == RML_PATH_I8 || path == RML_PATH_F64, RML_ERR_INVALID,
                "rml_svm_kernel_matrix: path must be AUTO, I8 or F64");
    RML_REQUIRE(path != RML_PATH_I8 || m->exact, RML_ERR_STATE, "rml_svm_kernel_matrix: exact path requested but the model is not on the code grid");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, st);           // shared workspace
    const int64_t CH = std::min<int64_t>(round_up(N, kTile), 8192);
    ChunkNeeds need{};
    need.q = m->exact && (path == RML_PATH_AUTO || path == RML_PATH_I8); need.f32 = true;
    ChunkWs w; ChunkPlan plan{};
    if (int rc = reserve_chunks(ctx, m, CH, need, st, &w, 1)) return rc;
    plan.policy = path; plan.kmat = kmat; plan.ld_k = ld_k;
    return run_float_rows(ctx, m, feat, ld_feat, N, CH, w, plan, DecisionOut{}, st);
}

// ---- fused front door: volumes -> projection -> SVM ---------------------------------------
namespace {
// one validated call of the front door (front_chunked fills the last group: what is fixed for its chunks)
struct FrontCall {
    rml_ctx* ctx; const rml_svm* m; hipStream_t caller;
    const void* V; int vdtype; int64_t B; int X, Y, Z; int mode; const int32_t* ijk; bool derive; int32_t* ijk_out;
    float scale_div; uint32_t mask; DecisionOut out;
    bool grid_ok;           // the code grid of the features is the model's: codes are the unscaled values
    int share_cu, q_rmw;    // ProjOut's: a GEMM runs beside the projections; read-compare-write of the code rows
    bool occ;               // the first projection pass also writes occupancy words (ChunkWs::occ) and the GEMM stage hands them on
    bool skip_ok;           // RML_OPT_SPARSE_STORES allows rows with holes for this call; whether a chunk gets them: FrontChunk::holes
    bool use_dig; ChunkPlan plan;   // rows off the code grid go to the multi-digit int8 kernel; the plan of every chunk
    bool u8() const { return vdtype == RML_VOL_U8; }
    int64_t frame_bytes() const { return (int64_t)X * Y * Z * (u8() ? 1 : 4); }
    int64_t plane_len(int pl) const { return pl == 0 ? (int64_t)X * Z : (pl == 1 ? (int64_t)Y * Z : (int64_t)X * Y); }
};

// projection pass 1 of a chunk: code rows + row statistics (uint8 volumes are on the code grid by construction: no row flags)
// (holes: FrontChunk::holes -- every other producer of code rows stores whole rows)
ProjOut code_rows_out(const FrontCall& f, const ChunkWs& w, bool holes = false) {
    ProjOut o{}; int64_t off = 0;
    for (int pl = 0; pl < 3; ++pl)
        if (f.mask & (1u << pl)) { o.q[pl] = w.q + off; off += f.plane_len(pl); }
    o.sel = f.mask & RML_MASK_ALL;
    o.qstride = f.m->Dq; o.qrow = w.q; o.qD = f.m->D;
    o.row_isum = w.isum; o.row_isq = w.isq; o.row_flags = f.u8() ? nullptr : w.flags; o.scale_div = f.scale_div;
    o.share_cu = f.share_cu; o.q_rmw = f.q_rmw;
    if (f.occ && w.occ) { o.occ = w.occ; o.occ_words = f.m->occ_words; o.skip_clear = holes ? 1 : 0; }
    return o;
}
// projection pass 2: float rows + norms, for the rows that left the code grid (or for a model that is not on it)
ProjOut float_rows_out(const FrontCall& f, const ChunkWs& w) {
    ProjOut o{}; int64_t off = 0;
    for (int pl = 0; pl < 3; ++pl)
        if (f.mask & (1u << pl)) { o.p[pl] = w.f32 + off; o.stride[pl] = f.m->Df; off += f.plane_len(pl); }
    o.sel = f.mask & RML_MASK_ALL;
    o.scale_div = f.scale_div; o.prow = w.f32; o.pD = f.m->D; o.pstride = f.m->Df; o.row_nsq = w.nsq;
    o.share_cu = f.share_cu;
    return o;
}

// Single observations -- how the reference calls the surface (predict.py:98-119: one target per call) -- and other batches of
// at most one sample tile (128 frames) on a code-grid model: everything on the caller's stream (no second stream, no events), the
// frame split over the chip (rml_launch_project_split) and the matrix-vector SVM kernels (plan_chunk picks them by the row
// count): 64x64x128 float32 314 -> ~100 us per call on the host clock, GPU work 275 -> ~60 us.
// (slices at given voxels -- the SDK target of predict.py:98-107 -- are one wave per row as they are: k_slice_rows)
int front_single_tile(const FrontCall& f) {
    rml_ctx* ctx = f.ctx; const rml_svm* m = f.m; hipStream_t st = f.caller;
    // (the frames are split while their pieces are fewer than ~4 per CU; byte volumes: k_project_u8_max takes 24 us as it is)
    const int S = (f.vdtype == RML_VOL_F32 && f.mode == RML_MODE_MAX && f.B <= 64) ? rml_project_split_pieces(f.X, f.Y, f.Z) : 0;
    const size_t sbytes = S ? ((rml_project_split_scratch_bytes(f.B, f.X, f.Y, f.Z, S) + 255) & ~(size_t)255) : 0;
    ChunkNeeds need{};
    need.q = true; need.f32 = !f.u8();
    ChunkWs w; void* scratch = nullptr;
    int rc = reserve_chunks(ctx, m, kTile, need, st, &w, 1, sbytes, &scratch);
    if (rc) return rc;
    const ProjOut o = code_rows_out(f, w);
    rc = S ? rml_launch_project_split(ctx, f.V, f.vdtype, f.B, f.X, f.Y, f.Z, o, static_cast<float*>(scratch), S, st)
           : rml_launch_project(ctx, f.V, f.vdtype, f.B, f.X, f.Y, f.Z, f.mode, f.ijk, o, st);
    if (rc) return rc;
    const ChunkOps x = ws_rows(m, w, f.B);
    ChunkPlan plan{};           // allow_big stays off: one sample tile
    plan.policy = f.u8() ? RML_PATH_I8 : RML_PATH_AUTO; plan.tiles_done = true; plan.all_exact_known = f.u8();
    if (f.u8()) return run_chunk(ctx, m, x, plan, w, f.out, st);
    launch_tile_flags(m, x, plan_chunk(ctx, m, plan, x, w), w, w.all_exact, st);
    // float rows + norms for frames that left the code grid (float64 path): a no-op when every frame is on it
    ProjOut of = float_rows_out(f, w);
    of.skip_if_set = w.all_exact;
    rc = rml_launch_project(ctx, f.V, f.vdtype, f.B, f.X, f.Y, f.Z, f.mode, f.ijk, of, st);
    return rc ? rc : run_chunk(ctx, m, x, plan, w, f.out, st);
}

// ---- the chunked pipelines: projection(c + 1) on the caller's stream beside GEMM(c) on ctx->aux_stream, two workspaces in rotation
struct FrontChunk {         // rows [r0, r0 + n) in w; "the rows are in w"; the frames, the given targets, where derived (i,j,k) go
    int64_t r0, n; const ChunkWs& w; hipEvent_t ev_proj; const void* V; const int32_t* ijk; int32_t* ijkd;
    bool holes;             // the first pass leaves the clear-bit lines of the code rows unstored (front_chunked decides, per chunk)
};
// the chunk's rows as its GEMM stage reads them: the one description the producer's decision (front_chunked) and run_chunk share
ChunkOps chunk_ops(const FrontCall& f, const FrontChunk& ck) {
    ChunkOps x = ws_rows(f.m, ck.w, ck.n);
    if (f.occ) x.occ = ck.w.occ;
    x.holes = ck.holes;
    return x;
}

// the caller's stream: a chunk's projection pass between the marks of the in-situ timing (and the digit planes of its float rows:
// run_chunk decides the general tiles from their flags), then the GEMM stream takes the chunk over
int caller_stage(const FrontCall& f, const FrontChunk& ck, const ProjOut& po) {
    rml_prof_mark(f.ctx, f.caller);
    const int rc = f.derive ? rml_launch_derive_slice(f.ctx, ck.V, f.vdtype, ck.n, f.X, f.Y, f.Z, 1, ck.ijkd, nullptr, po, f.caller)
                            : rml_launch_project(f.ctx, ck.V, f.vdtype, ck.n, f.X, f.Y, f.Z, f.mode, ck.ijk, po, f.caller);
    rml_prof_mark(f.ctx, f.caller);
    if (f.ctx->profiling) f.ctx->prof_frames += ck.n;
    if (rc) return rc;
    if (f.use_dig) { launch_digit_rows(f.m, ck.w, ck.n, f.caller); RML_HIP(hipGetLastError()); }
    RML_HIP(hipEventRecord(ck.ev_proj, f.caller));
    RML_HIP(hipStreamWaitEvent(f.ctx->aux_stream, ck.ev_proj, 0));
    return RML_OK;
}
int gemm_stage(const FrontCall& f, const FrontChunk& ck) {
    hipStream_t aux = f.ctx->aux_stream;
    rml_prof_mark_gemm(f.ctx, aux);
    const ChunkOps x = chunk_ops(f, ck);
    const int rc = run_chunk(f.ctx, f.m, x, f.plan, ck.w, f.out.at(ck.r0, f.m->C, f.m->P), aux);
    rml_prof_mark_gemm(f.ctx, aux);
    if (f.ctx->profiling) f.ctx->prof_ops_g += 2.0 * (double)ck.n * (double)f.m->M * (double)f.m->D;
    return rc;
}

// uint8 volumes are on the code grid by construction: one projection pass (codes + statistics), the exact GEMM on
// every tile, no flag kernels, no predicated second pass and no predicated float64 GEMM launch
int chunk_u8(const FrontCall& f, const FrontChunk& ck) {
    const int rc = caller_stage(f, ck, code_rows_out(f, ck.w, ck.holes));
    return rc ? rc : gemm_stage(f, ck);
}

// float32 volumes, model on the code grid: two passes.
// The caller's stream carries NOTHING but the first projection pass of every chunk (codes + statistics: the exact path needs
// nothing else): the tile decision and the predicated second pass (float rows for tiles that left the grid: a no-op otherwise)
// follow on the second stream, in front of the chunk's GEMMs.  (Round 2 had them between the projection launches: three launches
// and their gaps per chunk on the stream the step waits for.)
// (Round 5, session r5j: the exact GEMM deciding its tiles from the row flags itself and starting the moment the projection is
// done, with the tile decision and the predicated general path -- second pass, float64 GEMM -- on a third stream beside it and
// the finish waiting for both: the chain WAS shorter, and the step slower -- 64x64x128 0.716-0.733 end to end against
// 0.752-0.759 on boxes of the same class, Walabot 0.593-0.598 against 0.633; k_project_lin in situ 0.66-0.68 against 0.745.
// A GEMM that starts WITH the next projection puts its workgroups on the CUs first, two per CU where the projection's
// persistent workgroup should go, and the projection pays for the imbalance.  The ~30 us of small kernels in front of the GEMM
// are what lets the projection settle first.)
int chunk_on_grid(const FrontCall& f, const FrontChunk& ck) {
    int rc = caller_stage(f, ck, code_rows_out(f, ck.w, ck.holes));
    if (rc) return rc;
    const ChunkOps x = chunk_ops(f, ck); hipStream_t aux = f.ctx->aux_stream;
    launch_tile_flags(f.m, x, plan_chunk(f.ctx, f.m, f.plan, x, ck.w), ck.w, ck.w.all_exact, aux);      // at the group run_chunk's GEMMs read
    ProjOut of = float_rows_out(f, ck.w);
    of.no_pad = 1; of.skip_if_set = ck.w.all_exact;
    // (fused derive -> slice: the first pass derived (i,j,k) per frame and sliced there in one launch; this one is a plain slice at
    // the indices the first one wrote)
    rc = rml_launch_project(f.ctx, ck.V, f.vdtype, ck.n, f.X, f.Y, f.Z, f.derive ? RML_MODE_SLICE : f.mode, f.derive ? ck.ijkd : ck.ijk, of, aux);
    return rc ? rc : gemm_stage(f, ck);
}

// a model that is not on the code grid has no code rows: ONE pass (float rows, norms, flags; it derives as well) and the digit
// planes on the caller's stream, the float64 or the multi-digit GEMM on the second
int chunk_off_grid(const FrontCall& f, const FrontChunk& ck) {
    ProjOut of = float_rows_out(f, ck.w);
    of.row_flags = ck.w.flags;
    const int rc = caller_stage(f, ck, of);
    return rc ? rc : gemm_stage(f, ck);
}

int front_chunked(FrontCall f) {
    rml_ctx* ctx = f.ctx; const rml_svm* m = f.m;
    // Persistent wave-per-frame projection (Walabot-like grids): one projection workgroup per CU plus 128x128 GEMM workgroups
    // beside it overlap for real (GEMM hidden under the projection: 26.7 vs 28.0 ms per 262 144 frames), which the
    // 256x256 GEMM (205 VGPRs x 8 waves) cannot do -- it does not fit on a CU next to anything.
    // derive -> slice: the persistent k_derive_slice takes the same pairing (one 8-wave workgroup per CU beside 128x128 GEMM
    // workgroups; the ring GEMM in whole-round chunks, the two kernels taking turns, measured 1-2 % slower: DESIGN.md 3.3)
    // Byte volumes (k_project_u8_max): the GEMM is a third of the step there, and since the projection's cross-lane steps left the
    // LDS pipe (round 3: 0.59 -> 0.71 of 8 TB/s alone) each kernel is worth more alone than beside the other: the 256x256 ring
    // kernel in whole-round chunks, the projection between its rounds (64x64x128 uint8, same box: 6.5-6.9 -> 7.4-7.5 M frames/s;
    // Walabot grid 17.9-18.0 -> 18.4).
    // (A CU partition -- the GEMM on g CUs of every XCD, the projection on the other 32 - g, six splits -- was measured in rounds
    // 2-3 and never won: DESIGN.md 3.3; the knob and its masked streams are gone since round 5.)
    const bool wave_proj = f.derive || rml_project_uses_wave_kernel(ctx, f.vdtype, f.mode, f.X, f.Y, f.Z, /*share_cu=*/true, std::min<int64_t>(f.B, 8192));
    // rows off the code grid: the multi-digit int8 kernel (256 x 256 tiles: chunks sized for whole rounds) where the model has a
    // digit frame and the batch is large enough, the float64 MFMA kernel otherwise
    // Only for models off the code grid: with a grid model the rows off the grid are the exception, and the digit kernel's
    // predicated launch -- a whole CU's LDS per workgroup even when it exits at once -- cannot start beside the resident projection
    // and GEMM workgroups: on the GEMM stream it waited for the end of the running projection launch, chunk after chunk
    // (profiles/r03_stats_walabot_f32.txt of session r3o: 224 launches of k_svm_gemm_ring<3,1>, up to 325 us each)
    f.use_dig = !f.grid_ok && !f.u8() && use_dig_gemm(m, RML_PATH_AUTO, f.B, ctx->num_cu);
    f.share_cu = 1;         // a GEMM runs beside every projection
    f.q_rmw = ctx->opt.code_rmw >= 0 ? ctx->opt.code_rmw : rml_code_rmw(m->D, f.frame_bytes(), f.derive, f.u8());
    const bool u8_exact = f.grid_ok && f.u8();
    f.plan.policy = u8_exact ? RML_PATH_I8 : (f.grid_ok ? RML_PATH_AUTO : RML_PATH_F64);
    f.plan.tiles_done = f.grid_ok;              // chunk_on_grid decides the tiles itself; chunk_u8 has none to decide
    f.plan.all_exact_known = u8_exact; f.plan.allow_big = !wave_proj; f.plan.dig_ready = f.use_dig;
    // 8192 frames per chunk; 16384 for small byte frames (same-box A/B: 22x31x176 float32 10.3 vs 9.6 M frames/s at 8192 vs 16384,
    // uint8 17.4 vs 17.7)
    // derive -> slice beside the 128x128 GEMM, frames of at most 1 MiB: 12 288 (six interleaved runs, session r4bk, Walabot grid:
    // 8.05 M frames/s at 8192, 8.21 at 12 288, 8.21 at 16 384; 64x64x128: 2.28 / 2.24 / 2.20 -- stays at 8192)
    const int64_t small_chunk = (f.u8() && (int64_t)f.X * f.Y * f.Z <= 200000) ? 16384
                                : (f.derive && !f.u8() && f.frame_bytes() <= (1 << 20)) ? 12288 : 8192;
    // (the 256 x 256 kernels -- ring GEMM, multi-digit GEMM -- get chunks of whole rounds; RML_OPT_CHUNK overrides)
    const int64_t CH = (f.grid_ok && !wave_proj) ? pick_chunk(ctx, m, f.B, small_chunk, /*dig=*/false)
                       : f.use_dig               ? pick_chunk(ctx, m, f.B, 8192, f.use_dig)
                                                 : std::min<int64_t>(round_up(f.B, kTile), f.grid_ok ? pick_chunk_opt(ctx, small_chunk) : 8192);
    ChunkNeeds need{};
    // Occupancy words (RML_OPT_SPARSE_ROWS): by default where the first pass is a wave-per-frame max / sum projection of float32
    // volumes, whose code stage writes them (Emitter::flush_wave), the 128 x 128 GEMM runs beside it and the grid is one where it
    // was measured to pay (rml_sparse_rows); forced (1): for every chunk the 128 x 128 kernel may take (a producer without the
    // code stage gets words of all ones: rml_launch_project).  The derive / slice emitters and the byte-native kernel never write them.
    f.occ = f.grid_ok && !f.derive && f.mode != RML_MODE_SLICE && ctx->opt.sparse_rows != 0 &&
            (ctx->opt.sparse_rows > 0 || (wave_proj && !f.u8() && rml_sparse_rows(f.X, f.Y, f.Z)));
    // Rows with holes (RML_OPT_SPARSE_STORES): only float32 max / sum projections on the wave-per-frame kernels -- the producers
    // that write their own words -- and, chunk by chunk below, only in front of a sparse plan
    f.skip_ok = f.occ && wave_proj && !f.u8() && ctx->opt.sparse_stores != 0 &&
                (ctx->opt.sparse_stores > 0 || rml_sparse_stores(f.X, f.Y, f.Z));
    need.q = f.grid_ok; need.f32 = true; need.dig = f.use_dig; need.ijk = f.derive && !f.ijk_out; need.occ = f.occ;     // the derived (i,j,k) stay in the chunk's workspace when the caller does not want them
    // workspaces in rotation: 2 (projection of chunk c+1 beside the GEMM of chunk c; a third one -- the projection two chunks
    // ahead -- changed nothing at 64x64x128 and cost 2 % at the Walabot grid: DESIGN.md 3.3)
    // (Three streams -- the small kernels either side of a chunk's GEMM on a third one, RML_PIPE_SPLIT in rounds 3-4 -- were
    // bimodal at the Walabot grid and -5 % at 64x64x128: DESIGN.md 3.3; removed in round 5.)
    constexpr int NBUF = 2;
    ChunkWs w2[NBUF];
    int rc = reserve_chunks(ctx, m, CH, need, f.caller, w2, NBUF);
    if (rc) return rc;
    // aux must start after everything already queued by the caller
    RML_HIP(hipEventRecord(ctx->ev_fork, f.caller));
    RML_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
    // (Round 5, session r5i: tapering the last chunk -- 8 192 -> 4 096, 2 048, 2 048, so that the GEMM left exposed behind the last
    // projection is a quarter of a chunk's -- LOST: end to end / in-situ kernel 0.953 against 0.957-0.958 at 64x64x128 and
    // 0.607 against 0.633 of 8 TB/s at the Walabot grid; a persistent launch over 2 048 frames is two frames per wave.)
    int64_t c = 0;
    for (int64_t r0 = 0; r0 < f.B; r0 += CH, ++c) {
        const int b = (int)(c % NBUF);
        if (c >= NBUF) RML_HIP(hipStreamWaitEvent(f.caller, ctx->ev_done[b], 0));    // workspace reuse
        FrontChunk ck{r0, std::min(CH, f.B - r0), w2[b], ctx->ev_proj[b], static_cast<const unsigned char*>(f.V) + r0 * f.frame_bytes(),
                      f.ijk ? f.ijk + r0 * 3 : nullptr, f.derive ? (f.ijk_out ? f.ijk_out + r0 * 3 : w2[b].ijk) : nullptr, false};
        // per chunk, not per call: a short last chunk takes split-K and RML_OPT_CHUNK can send chunks to the small kernels -- both
        // read every line (plan_chunk makes no HIP call: nothing changes for a stream capture)
        ck.holes = f.skip_ok && plan_chunk(ctx, m, f.plan, chunk_ops(f, ck), ck.w).sparse;
        rc = !f.grid_ok ? chunk_off_grid(f, ck) : (f.u8() ? chunk_u8(f, ck) : chunk_on_grid(f, ck));
        if (rc) return rc;
        RML_HIP(hipEventRecord(ctx->ev_done[b], ctx->aux_stream));
    }
    RML_HIP(hipEventRecord(ctx->ev_join, ctx->aux_stream));
    // join: the caller's stream continues after the last GEMMs and their finish
    RML_HIP(hipStreamWaitEvent(f.caller, ctx->ev_join, 0));
    return RML_OK;
}

// the validating front of rml_project_svm / rml_derive_project_svm
int project_svm_front(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                      int mode, const int32_t* ijk, bool derive, int32_t* ijk_out, float scale_div, uint32_t mask,
                      const DecisionOut& out, void* stream) {
    RML_REQUIRE(ctx && m && B >= 0, RML_ERR_INVALID, "rml_project_svm: bad arguments");
    if (B == 0) return RML_OK;
    RML_REQUIRE(V != nullptr, RML_ERR_INVALID, "rml_project_svm: V is NULL");
    RML_REQUIRE(vdtype == RML_VOL_F32 || vdtype == RML_VOL_U8, RML_ERR_INVALID, "rml_project_svm: unknown volume dtype %d", vdtype);
    RML_REQUIRE(rml_feature_len(X, Y, Z, mask) == m->D, RML_ERR_INVALID, "rml_project_svm: grid/mask give D=%lld, model has D=%lld",
                (long long)rml_feature_len(X, Y, Z, mask), (long long)m->D);
    RML_REQUIRE(!(out.proba || out.label_calib) || m->has_calib, RML_ERR_STATE, "rml_project_svm: model has no calibrators");
    RML_REQUIRE(mode != RML_MODE_SLICE || ijk || derive, RML_ERR_INVALID, "rml_project_svm: mode SLICE needs ijk");
    if (mode == RML_MODE_MAX_NAN) mode = RML_MODE_MAX;         // round 6: mode MAX itself has NumPy's NaN policy
    const bool scaled = scale_div > 1.0f;
    const bool grid_ok = m->exact && ((scaled && (double)scale_div == m->code_scale) || (!scaled && m->code_scale == 1.0));
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t caller = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, caller);       // shared workspaces, aux stream and chunk events (the caller's stream joins at the end)
    const FrontCall f{ctx, m, caller, V, vdtype, B, X, Y, Z, mode, ijk, derive, ijk_out, scale_div, mask, out, grid_ok};
    if (B <= kTile && grid_ok && !derive && (mode == RML_MODE_MAX || (mode == RML_MODE_SLICE && ijk))) return front_single_tile(f);
    return front_chunked(f);
}
}  // namespace

extern "C" int rml_project_svm(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                               int mode, const int32_t* ijk, float scale_div, uint32_t mask,
                               double* dec_ovo, double* dec_ovr, double* proba,
                               int32_t* label_vote, int32_t* label_calib, void* stream) {
    return project_svm_front(ctx, m, V, vdtype, B, X, Y, Z, mode, ijk, /*derive=*/false, nullptr, scale_div, mask,
                             DecisionOut{dec_ovo, dec_ovr, proba, label_vote, label_calib}, stream);
}

extern "C" int rml_derive_project_svm(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                                      float scale_div, uint32_t mask, int32_t* ijk_out,
                                      double* dec_ovo, double* dec_ovr, double* proba,
                                      int32_t* label_vote, int32_t* label_calib, void* stream) {
    RML_REQUIRE(rml_derive_slice_supported(ctx, V, vdtype, X, Y, Z, 1) == 1, RML_ERR_UNSUPPORTED,
                "rml_derive_project_svm: no fused derive kernel for %dx%dx%d (rows of whole quads, Z <= 256, odd part of Z/4 <= 15): "
                "use rml_derive_targets + rml_project_svm(mode SLICE)", X, Y, Z);
    return project_svm_front(ctx, m, V, vdtype, B, X, Y, Z, RML_MODE_SLICE, nullptr, /*derive=*/true, ijk_out, scale_div, mask,
                             DecisionOut{dec_ovo, dec_ovr, proba, label_vote, label_calib}, stream);
}

// ---- the front door for a foreign arena: projection at the source grid -> k_zoom_rows -> SVM -----------------------------
namespace {
// One chunk.  The caller's stream: the projection at the source grid into the chunk's stage, k_zoom_rows into the workspace (float
// rows at the model's stride, norms, flags -- what chunk_off_grid asks a projection for) and the digit planes of the zoomed rows;
// then the GEMM stream takes the chunk over, as in chunk_off_grid.
int chunk_zoom(const FrontCall& f, const FrontChunk& ck, const rml_zoom_plan& zp, void* stage) {
    int rc = rml_zoom_stage_run(f.ctx, zp, stage, ck.V, ck.n, f.mode, ck.ijk, f.scale_div, ck.w.f32, f.m->Df, f.m->Df, ck.w.nsq, ck.w.flags,
                                f.caller);
    if (rc) return rc;
    if (f.use_dig) { launch_digit_rows(f.m, ck.w, ck.n, f.caller); RML_HIP(hipGetLastError()); }
    RML_HIP(hipEventRecord(ck.ev_proj, f.caller));
    RML_HIP(hipStreamWaitEvent(f.ctx->aux_stream, ck.ev_proj, 0));
    return gemm_stage(f, ck);
}

int front_zoom(FrontCall f, const rml_zoom_plan& zp) {
    rml_ctx* ctx = f.ctx; const rml_svm* m = f.m;
    // zoomed rows are off the code grid whatever the model: the float64 kernel, or the multi-digit kernel under the rule of
    // rml_svm_decision for float rows (so that the call computes what rml_project_zoom + rml_svm_decision compute)
    f.use_dig = use_dig_gemm(m, RML_PATH_AUTO, f.B, ctx->num_cu);
    f.plan.policy = RML_PATH_F64; f.plan.dig_ready = f.use_dig;
    ChunkNeeds need{};
    need.f32 = true; need.dig = f.use_dig;
    if (f.B <= kTile) {
        // a single observation (predict.py:98-119) or any batch of one sample tile: everything on the caller's stream, as front_single_tile
        ChunkWs w; void* stage = nullptr;
        int rc = reserve_chunks(ctx, m, kTile, need, f.caller, &w, 1, rml_zoom_stage_bytes(zp, f.B), &stage);
        if (rc) return rc;
        rc = rml_zoom_stage_run(ctx, zp, stage, f.V, f.B, f.mode, f.ijk, f.scale_div, w.f32, m->Df, m->Df, w.nsq, w.flags, f.caller);
        if (rc) return rc;
        if (f.use_dig) { launch_digit_rows(m, w, f.B, f.caller); RML_HIP(hipGetLastError()); }
        return run_chunk(ctx, m, ws_rows(m, w, f.B), f.plan, w, f.out, f.caller);
    }
    const int64_t CH = f.use_dig ? pick_chunk(ctx, m, f.B, 8192, true) : std::min<int64_t>(round_up(f.B, kTile), pick_chunk_opt(ctx, 8192));
    constexpr int NBUF = 2;         // workspaces and stages in rotation, as front_chunked
    ChunkWs w2[NBUF];
    const size_t sbytes = rml_zoom_stage_bytes(zp, CH);
    void* stages = nullptr;
    int rc = reserve_chunks(ctx, m, CH, need, f.caller, w2, NBUF, NBUF * sbytes, &stages);
    if (rc) return rc;
    RML_HIP(hipEventRecord(ctx->ev_fork, f.caller));
    RML_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
    int64_t c = 0;
    for (int64_t r0 = 0; r0 < f.B; r0 += CH, ++c) {
        const int b = (int)(c % NBUF);
        if (c >= NBUF) RML_HIP(hipStreamWaitEvent(f.caller, ctx->ev_done[b], 0));    // workspace reuse
        const FrontChunk ck{r0, std::min(CH, f.B - r0), w2[b], ctx->ev_proj[b], static_cast<const unsigned char*>(f.V) + r0 * f.frame_bytes(),
                            f.ijk ? f.ijk + r0 * 3 : nullptr, nullptr};
        rc = chunk_zoom(f, ck, zp, static_cast<unsigned char*>(stages) + (size_t)b * sbytes);
        if (rc) return rc;
        RML_HIP(hipEventRecord(ctx->ev_done[b], ctx->aux_stream));
    }
    RML_HIP(hipEventRecord(ctx->ev_join, ctx->aux_stream));
    RML_HIP(hipStreamWaitEvent(f.caller, ctx->ev_join, 0));
    return RML_OK;
}
}  // namespace

// predict.py:98-119 for a recording whose arena differs from the training arena (calc_proj_zoom, predict.py:34-54, is not 1):
// slices or max-projections at the source grid, common.process_samples' zoom to the training geometry (common.py:141-148), the
// classifier of predict.py:60 -- B frames per call, nothing through the host
extern "C" int rml_project_zoom_svm(rml_ctx* ctx, const rml_svm* m, const void* V, int vdtype, int64_t B, int X, int Y, int Z,
                                    int mode, const int32_t* ijk, const int32_t* out_shape, float scale_div, uint32_t mask,
                                    double* dec_ovo, double* dec_ovr, double* proba,
                                    int32_t* label_vote, int32_t* label_calib, void* stream) {
    RML_REQUIRE(ctx && m && B >= 0, RML_ERR_INVALID, "rml_project_zoom_svm: bad arguments");
    if (mode == RML_MODE_MAX_NAN) mode = RML_MODE_MAX;
    RML_REQUIRE(mode == RML_MODE_MAX || mode == RML_MODE_SLICE || mode == RML_MODE_SUM, RML_ERR_INVALID, "rml_project_zoom_svm: unknown mode %d", mode);
    rml_zoom_plan zp;
    if (int rc = rml_zoom_plan_make(ctx, "rml_project_zoom_svm", vdtype, mode, X, Y, Z, 1, mode == RML_MODE_SLICE && !ijk, out_shape, mask, &zp)) return rc;
    RML_REQUIRE(zp.Dout == m->D, RML_ERR_INVALID, "rml_project_zoom_svm: the zoomed planes give D=%lld, model has D=%lld",
                (long long)zp.Dout, (long long)m->D);
    if (B == 0) return RML_OK;
    RML_REQUIRE(V != nullptr, RML_ERR_INVALID, "rml_project_zoom_svm: V is NULL");
    RML_REQUIRE(B < (int64_t)1 << 31, RML_ERR_UNSUPPORTED, "rml_project_zoom_svm: B too large");
    RML_REQUIRE(!(proba || label_calib) || m->has_calib, RML_ERR_STATE, "rml_project_zoom_svm: model has no calibrators");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t caller = static_cast<hipStream_t>(stream);
    rml_ctx_guard guard(ctx, caller);       // shared workspaces, aux stream and chunk events (the caller's stream joins at the end)
    const FrontCall f{ctx, m, caller, V, vdtype, B, X, Y, Z, mode, ijk, /*derive=*/false, nullptr, scale_div, mask,
                      DecisionOut{dec_ovo, dec_ovr, proba, label_vote, label_calib}, /*grid_ok=*/false};
    return front_zoom(f, zp);
}

// libsvm's own Platt coefficients (SVC(probability=True): sk:svm/_base.py _probA / _probB, one pair per class pair):
// uploaded once, at load time, so that rml_svm_pairwise_proba is an ordinary asynchronous launch
extern "C" int rml_svm_set_platt(rml_ctx* ctx, rml_svm* m, const double* probA, const double* probB) {
    RML_REQUIRE(ctx && m && probA && probB, RML_ERR_INVALID, "rml_svm_set_platt: NULL argument");
    RML_HIP(hipSetDevice(ctx->device));
    std::vector<double> ab(2 * kMaxP, 0.0);
    for (int p = 0; p < m->P; ++p) { ab[p] = probA[p]; ab[kMaxP + p] = probB[p]; }
    if (!m->platt) RML_HIP(hipMalloc(reinterpret_cast<void**>(&m->platt), ab.size() * sizeof(double)));
    RML_HIP(hipMemcpy(m->platt, ab.data(), ab.size() * sizeof(double), hipMemcpyHostToDevice));
    return RML_OK;
}

extern "C" int rml_svm_pairwise_proba(rml_ctx* ctx, const rml_svm* m, const double* dec_ovo, int64_t N, double* proba, void* stream) {
    RML_REQUIRE(ctx && m && N >= 0, RML_ERR_INVALID, "rml_svm_pairwise_proba: bad arguments");
    if (N == 0) return RML_OK;
    RML_REQUIRE(dec_ovo && proba, RML_ERR_INVALID, "rml_svm_pairwise_proba: NULL array");
    RML_REQUIRE(m->platt != nullptr, RML_ERR_STATE, "rml_svm_pairwise_proba: the model has no Platt coefficients (rml_svm_set_platt)");
    RML_HIP(hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_pairwise_proba, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dec_ovo, N, m->C, m->platt, m->platt + kMaxP, proba);
    RML_HIP(hipGetLastError());
    return RML_OK;
}

// ---- linear classifier --------------------------------------------------------------------
extern "C" int rml_linear_load(rml_ctx* ctx, const double* coef, const double* intercept, int n_classes, int64_t D,
                               const double* calib_a, const double* calib_b, rml_linear** out) {
    RML_REQUIRE(ctx && coef && intercept && out && D > 0, RML_ERR_INVALID, "rml_linear_load: bad arguments");
    RML_REQUIRE(n_classes >= 2 && n_classes <= kMaxC, RML_ERR_UNSUPPORTED, "rml_linear_load: %d classes", n_classes);
    RML_REQUIRE((calib_a == nullptr) == (calib_b == nullptr), RML_ERR_INVALID, "rml_linear_load: calib_a/calib_b must both be given");
    *out = nullptr;
    RML_HIP(hipSetDevice(ctx->device));
    rml_linear* m = new (std::nothrow) rml_linear();
    RML_REQUIRE(m != nullptr, RML_ERR_NOMEM, "rml_linear_load: out of host memory");
    m->D = D; m->C = n_classes; m->has_calib = calib_a != nullptr;
    const int rows = n_classes == 2 ? 1 : n_classes;
    std::vector<double> cf((size_t)n_classes * D, 0.0), ic(n_classes, 0.0);
    std::copy(coef, coef + (size_t)rows * D, cf.begin());
    std::copy(intercept, intercept + rows, ic.begin());
    int rc = dev_upload(&m->coef, cf);
    if (!rc) rc = dev_upload(&m->intercept, ic);
    if (!rc && m->has_calib) {
        std::vector<double> cal(2 * n_classes, 0.0);
        for (int c = 0; c < rows; ++c) { cal[c] = calib_a[c]; cal[n_classes + c] = calib_b[c]; }
        rc = dev_upload(&m->calib, cal);
    }
    if (rc) { rml_linear_free(ctx, m); return rc; }
    *out = m;
    return RML_OK;
}

extern "C" int rml_linear_free(rml_ctx* ctx, rml_linear* m) {
    if (!m) return RML_OK;
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    if (m->coef) (void)hipFree(m->coef);
    if (m->intercept) (void)hipFree(m->intercept);
    if (m->calib) (void)hipFree(m->calib);
    delete m;
    return RML_OK;
}

extern "C" int rml_linear_decision(rml_ctx* ctx, const rml_linear* m, const float* feat, int64_t ld_feat, int64_t N,
                                   double* dec, double* proba, int32_t* label, int32_t* label_calib, void* stream) {
    RML_REQUIRE(ctx && m && N >= 0, RML_ERR_INVALID, "rml_linear_decision: bad arguments");
    if (N == 0) return RML_OK;
    RML_REQUIRE(feat && ld_feat >= m->D, RML_ERR_INVALID, "rml_linear_decision: bad arguments");
    RML_REQUIRE(!(proba || label_calib) || m->has_calib, RML_ERR_STATE, "rml_linear_decision: model has no calibrators");
    RML_HIP(hipSetDevice(ctx->device));
    if (N == 0) return RML_OK;
    hipLaunchKernelGGL(k_linear, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       feat, ld_feat, N, m->D, m->C, m->coef, m->intercept, m->calib, (int)m->has_calib, dec, proba, label, label_calib);
    RML_HIP(hipGetLastError());
    return RML_OK;
}
