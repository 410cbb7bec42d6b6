// Sanitizer driver of libradarml_hip.so (tools/sanitize/build.py): a plain program over the C ABI of include/radarml.h plus the
// host-only internals of csrc/ (model packing, Pillow table builder).  Built with -fsanitize=address,undefined against the
// host-only library it runs on a box without a GPU (phase A: every path that precedes the first HIP call, and the graceful failure
// of that call); linked against the real library on a GPU box it adds phase B: four host threads on two streams sharing ONE
// rml_ctx through the fused projection -> SVM pipeline, rml_project and rml_svm_decision, results compared bit for bit.
// Exit status 0 = every check passed (a sanitizer report aborts the process with its own status).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <thread>
#include <vector>
#include "../../radar-ml_amd/csrc/rml_internal.h"
#include "../../radar-ml_amd/csrc/resize_tables.h"

static int g_fail = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

// ---- phase A ------------------------------------------------------------------------------------------------------------------
static void phase_a_arguments() {
    CHECK(rml_feature_len(22, 31, 176, RML_MASK_ALL) == 10010);
    CHECK(rml_feature_len(64, 64, 128, RML_MASK_ALL) == 20480);
    CHECK(rml_feature_len(22, 31, 176, RML_MASK_XY) == 682);
    CHECK(rml_feature_len(22, 31, 176, 0) == 0);
    CHECK(rml_version() != nullptr && strlen(rml_version()) > 0);
    // NULL context / NULL pointers: a status and a message, never a dereference
    float f = 0; double d = 0; int32_t i3[3] = {0, 0, 0}; int64_t n = 0; rml_svm* m = nullptr; rml_linear* lm = nullptr;
    CHECK(rml_project(nullptr, &f, RML_VOL_F32, 1, 2, 2, 4, RML_MODE_MAX, nullptr, 0.f, RML_MASK_ALL, &f, 16, nullptr, 0, nullptr, nullptr, nullptr, nullptr) < 0);
    CHECK(strlen(rml_last_error()) > 0);
    CHECK(rml_derive_targets(nullptr, &f, RML_VOL_F32, 1, 2, 2, 4, 1, i3, nullptr, nullptr) < 0);
    CHECK(rml_svm_load(nullptr, &d, 1, 1, &d, &d, i3, 3, RML_KERNEL_RBF, 0.1, 255.0, nullptr, nullptr, &m) < 0 && m == nullptr);
    CHECK(rml_svm_decision(nullptr, nullptr, 0, &f, 1, nullptr, 0, nullptr, nullptr, nullptr, 1, &d, nullptr, nullptr, nullptr, nullptr, nullptr) < 0);
    CHECK(rml_project_svm(nullptr, nullptr, &f, RML_VOL_F32, 1, 2, 2, 4, RML_MODE_MAX, nullptr, 255.f, RML_MASK_ALL, &d, nullptr, nullptr, nullptr, nullptr, nullptr) < 0);
    CHECK(rml_linear_load(nullptr, &d, &d, 3, 4, nullptr, nullptr, &lm) < 0);
    {
        const int kd[2] = {RML_GRAM_LINEAR, RML_GRAM_RBF};
        const double gm[2] = {0.0, 0.5};
        CHECK(rml_gram(nullptr, &f, 1, 1, 1, 2, kd, gm, &d, 1, 1, nullptr) == RML_ERR_INVALID && strlen(rml_last_error()) > 0);
    }
    {
        rml_smo_problem sp{};
        rml_smo_fit sf{};
        int32_t i32 = 0;
        CHECK(rml_smo_solve(nullptr, &d, 1, 1, 1, 1, &sp, 1, &i32, 1, &d, 1, &d, &i32, &i32, nullptr) == RML_ERR_INVALID && strlen(rml_last_error()) > 0);
        CHECK(rml_smo_score(nullptr, &d, 1, 1, 1, 1, &sp, 1, &i32, 1, &d, 1, &d, 2, &sf, 1, &i32, &i32, 1, &d, &i32, &i32, nullptr) == RML_ERR_INVALID);
    }
    CHECK(rml_profile_read(nullptr, &n, &d, &n) < 0);
    CHECK(rml_probe_stream(nullptr, &f, 1 << 20, 1, &d, nullptr) < 0);
    CHECK(rml_ctx_set_option(nullptr, RML_OPT_PROJECT_SHARE_CU, 1) < 0);
    {
        int v = 0;
        CHECK(rml_ctx_get_option(nullptr, RML_OPT_CHUNK, &v) < 0 && rml_ctx_reserve_workspace(nullptr, 1 << 20) < 0 && rml_ctx_workspace_bytes(nullptr) == 0);
        CHECK(rml_dnn_trunk_x3_supported(80, 80) == 1 && rml_dnn_trunk_x3_supported(128, 128) == 0 && rml_dnn_trunk_x3_supported(81, 80) == 0);
        CHECK(rml_dnn_trunk_kblock_supported(80, 80) == 1 && rml_dnn_trunk_kblock_supported(96, 80) == 0 && rml_dnn_trunk_kblock_supported(80, 84) == 0);
        {
            int path[6] = {9, 9, 9, 9, 9, 9};
            CHECK(rml_dnn_trunk_path(80, 80, 0, 1, 256, nullptr) == RML_ERR_INVALID && rml_dnn_trunk_path(80, 80, 0, 0, 256, path) == RML_ERR_INVALID &&
                  rml_dnn_trunk_path(80, 80, 0, 1, 0, path) == RML_ERR_INVALID && path[0] == 9);
            CHECK(rml_dnn_trunk_path(80, 80, 1, 512, 256, path) == RML_OK && path[0] == 1 && path[1] == 0 && path[4] == 1 && path[5] == 256);
            CHECK(rml_dnn_trunk_path(80, 80, 1, 513, 256, path) == RML_OK && path[0] == 1 && path[4] == 0 && path[5] == 65);
            CHECK(rml_dnn_trunk_path(124, 64, 1, 1000, 256, path) == RML_OK && path[0] == 2 && path[1] == 4 && path[2] == 2 && path[3] == 1 && path[5] == 170);
            CHECK(rml_dnn_trunk_path(36, 256, 0, 3, 256, path) == RML_OK && path[0] == 2 && path[1] == 1 && path[2] == 1 && path[3] == 0 && path[5] == 3);
            CHECK(rml_dnn_trunk_path(40, 264, 0, 3, 256, path) == RML_OK && path[0] == 0 && path[5] == 0);
            // planes whose layouts would overflow 32-bit arithmetic: refused before any layout is computed
            CHECK(rml_dnn_trunk_path(2147483644, 2147483644, 0, 3, 256, path) == RML_OK && path[0] == 0);
            CHECK(rml_dnn_trunk_kblock_supported(2147483644, 2147483640) == 0 && rml_dnn_trunk_kblock_supported(65536, 65536) == 0);
        }
        CHECK(rml_dnn_trunk_x3(nullptr, &f, &f, &f, 1, 80, 80, &f, &f, &f, &f, 2, &f, nullptr) < 0);
        CHECK(rml_dnn_exact_features_scratch_bytes(RML_VOL_F32, 10, 22, 31, 176, 80, 80, 1) > 10 * 22 * 31 * 176 * 4);
        CHECK(rml_dnn_exact_features(nullptr, &f, RML_VOL_F32, nullptr, 1, 2, 2, 4, RML_MODE_MAX, 80, 80, &f, &f, &f, &f, 2, &f, 1, &f, nullptr) < 0);
        CHECK(rml_dnn_top2_gap(nullptr, &f, 3, 1, 3, &f, nullptr) < 0);
        CHECK(rml_dnn_guard_apply(nullptr, &f, 3, 3, nullptr, 1, &f, 1e-4f, nullptr, nullptr, nullptr, nullptr) < 0);
    }
    CHECK(rml_svm_free(nullptr, nullptr) == RML_OK && rml_linear_free(nullptr, nullptr) == RML_OK && rml_ctx_destroy(nullptr) == RML_OK);
    CHECK(rml_svm_is_exact(nullptr) == 0 && rml_svm_num_sv(nullptr) == 0 && rml_svm_dim(nullptr) == 0);
    CHECK(rml_ctx_device(nullptr) < 0);
    rml_ctx* bad = nullptr;
    CHECK(rml_ctx_create(-5, &bad) < 0 && bad == nullptr);
    CHECK(rml_ctx_create(4099, &bad) < 0 && bad == nullptr);
    // pure-host predicates
    for (int X = 1; X <= 70; X += 7)
        for (int Y = 1; Y <= 70; Y += 9)
            for (int Z = 4; Z <= 260; Z += 36)
                for (int o : {16, 80, 128}) {
                    (void)rml_dnn_preprocess_supported(X, Y, Z, o, o);
                    (void)rml_derive_slice_supported(nullptr, &f, RML_VOL_F32, X, Y, Z, 1);
                    (void)rml_derive_slice_supported(nullptr, &f, RML_VOL_U8, X, Y, Z, 3);
                    (void)rml_code_rmw_default(rml_feature_len(X, Y, Z, RML_MASK_ALL), (int64_t)X * Y * Z, X & 1, Y & 1);
                }
    CHECK(rml_dnn_preprocess_supported(22, 31, 176, 80, 80) == 1);
    CHECK(rml_adam_entry_bytes() > 0);
}

static void phase_a_pillow_tables() {
    for (int in : {1, 2, 3, 22, 31, 64, 176, 500})
        for (int out : {1, 2, 3, 80, 128, 257}) {
            rmlresize::AxisTable t;
            rmlresize::precompute(in, out, t);
            CHECK((int)t.bounds.size() == 2 * out && (int)t.kk.size() == out * t.ksize);
            for (int x = 0; x < out; ++x) {
                const int x0 = t.bounds[2 * x], nt = t.bounds[2 * x + 1];
                CHECK(x0 >= 0 && nt >= 1 && nt <= t.ksize && x0 + nt <= in);
                double s = 0;
                for (int k = 0; k < nt; ++k) s += t.kk[(size_t)x * t.ksize + k];
                CHECK(fabs(s - 1.0) < 1e-12);
            }
        }
}

static void phase_a_model_packing() {
    struct Case { int64_t M, D; int C; int kind; double scale; };      // kind 0: codes/255 on the grid, 1: off the grid, 2: one NaN, 3: unscaled codes
    const Case cases[] = {{5, 7, 2, 0, 255.0}, {300, 1234, 3, 0, 255.0}, {17, 130, 6, 1, 255.0}, {64, 129, 3, 2, 255.0},
                          {128, 128, 4, 3, 1.0}, {129, 127, 5, 0, 255.0}, {1, 1, 2, 0, 255.0}};
    for (const Case& c : cases) {
        std::vector<double> sv((size_t)c.M * c.D), dc((size_t)(c.C - 1) * c.M);
        for (double& v : sv) {
            const int code = (int)(rnd() % 256);
            v = c.kind == 3 ? (double)code : (double)((float)code / 255.0f);
            if (c.kind == 1) v += 1e-3 * (double)(rnd() % 100);
        }
        if (c.kind == 2) sv[sv.size() / 2] = NAN;
        for (double& v : dc) v = ((double)(rnd() % 2001) - 1000.0) / 100.0;
        std::vector<int32_t> ns(c.C, 0);
        for (int64_t r = 0; r < c.M; ++r) ns[r % c.C]++;
        if (c.M < c.C) { std::fill(ns.begin(), ns.end(), 0); ns[0] = (int32_t)c.M; }
        rml_svm m;
        rml_svm_pack pk;
        int rc = rml_svm_pack_host(sv.data(), c.M, c.D, dc.data(), ns.data(), c.C, RML_KERNEL_RBF, 0.01, c.scale, true, &m, &pk);
        CHECK(rc == RML_OK);
        CHECK(m.Mpad >= c.M && m.Mpad % 128 == 0 && m.Dq >= c.D && m.Df >= c.D && ((m.Dq / 128) & 1) == 1);
        CHECK((int64_t)pk.W.size() == m.PT * m.Mpad && (int64_t)pk.svf.size() == m.Mpad * m.Df && (int64_t)pk.svq.size() == m.Mpad * m.Dq);
        CHECK(m.exact == (c.kind == 0 || c.kind == 3));
        CHECK(m.dig_ok ? ((int64_t)pk.svd.size() == 4 * m.Mpad * m.Dq && (int64_t)pk.dnsq.size() == m.Mpad) : pk.svd.empty());
        if (c.kind == 2) CHECK(!m.dig_ok);
        // linear kernel, no calibrators
        rc = rml_svm_pack_host(sv.data(), c.M, c.D, dc.data(), ns.data(), c.C, RML_KERNEL_LINEAR, 0.0, c.scale, false, &m, &pk);
        CHECK(rc == RML_OK && !m.dig_ok);
        // validation
        ns[0] += 1;
        CHECK(rml_svm_pack_host(sv.data(), c.M, c.D, dc.data(), ns.data(), c.C, RML_KERNEL_RBF, 0.01, c.scale, true, &m, &pk) == RML_ERR_INVALID);
        CHECK(strstr(rml_last_error(), "n_support") != nullptr);
        ns[0] -= 1;
        CHECK(rml_svm_pack_host(sv.data(), c.M, c.D, dc.data(), ns.data(), 7, RML_KERNEL_RBF, 0.01, c.scale, true, &m, &pk) == RML_ERR_UNSUPPORTED);
        CHECK(rml_svm_pack_host(sv.data(), c.M, c.D, dc.data(), ns.data(), c.C, 9, 0.01, c.scale, true, &m, &pk) == RML_ERR_UNSUPPORTED);
    }
}

// The byte size of a chunk workspace (rml_svm_ws_bytes: svm.hip's carve) for seven model geometries x two chunk sizes x the 16
// combinations of ChunkNeeds {code rows, float rows, digit planes, derived ijk} against kWsBytes: the sizes the layout had when
// the table was printed (`driver --print-ws-table` on a commit whose layout is trusted).  The fused front doors carve two such
// workspaces back to back from one block, so a part that grows or moves unnoticed is an overrun, not an error.
struct WsCase { int64_t M, D; int C; };
static const WsCase kWsCases[] = {{5, 7, 2}, {300, 1234, 3}, {17, 130, 6}, {64, 129, 3}, {128, 128, 4}, {129, 127, 5}, {2562, 20480, 3}};
static const int64_t kWsChunks[] = {2048, 8192};        // with and without the split-K scratch
static const size_t kWsBytes[7][2][16] = {
    {{66048, 1380864, 328192, 1643008, 5333504, 6648320, 5595648, 6910464, 90624, 1405440, 352768, 1667584, 5358080, 6672896, 5620224, 6935040},
     {262912, 1315584, 1311488, 2364160, 21332736, 22385408, 22381312, 23433984, 361216, 1413888, 1409792, 2462464, 21431040, 22483712, 22479616, 23532288}},
    {{197120, 6238720, 10420736, 16462336, 20144640, 26186240, 30368256, 36409856, 221696, 6263296, 10445312, 16486912, 20169216, 26210816, 30392832, 36434432},
     {787200, 12333824, 41681664, 53228288, 80577280, 92123904, 121471744, 133018368, 885504, 12432128, 41779968, 53326592, 80675584, 92222208, 121570048, 133116672}},
    {{295424, 2134528, 1606144, 3445248, 7660032, 9499136, 8970752, 10809856, 320000, 2159104, 1630720, 3469824, 7684608, 9523712, 8995328, 10834432},
     {1180416, 4330240, 6423296, 9573120, 30638848, 33788672, 35881728, 39031552, 1278720, 4428544, 6521600, 9671424, 30737152, 33886976, 35980032, 39129856}},
    {{98816, 1937920, 1409536, 3248640, 7463424, 9302528, 8774144, 10613248, 123392, 1962496, 1434112, 3273216, 7488000, 9327104, 8798720, 10637824},
     {393984, 3543808, 5636864, 8786688, 29852416, 33002240, 35095296, 38245120, 492288, 3642112, 5735168, 8884992, 29950720, 33100544, 35193600, 38343424}},
    {{147968, 1462784, 1458688, 2773504, 5415424, 6730240, 6726144, 8040960, 172544, 1487360, 1483264, 2798080, 5440000, 6754816, 6750720, 8065536},
     {590592, 1643264, 5833472, 6886144, 21660416, 22713088, 26903296, 27955968, 688896, 1741568, 5931776, 6984448, 21758720, 22811392, 27001600, 28054272}},
    {{377344, 2744832, 1688064, 4055552, 5644800, 8012288, 6955520, 9323008, 401920, 2769408, 1712640, 4080128, 5669376, 8036864, 6980096, 9347584},
     {1508096, 2564864, 6750976, 7807744, 22577920, 23634688, 27820800, 28877568, 1606400, 2663168, 6849280, 7906048, 22676224, 23732992, 27919104, 28975872}},
    {{1081856, 65393152, 169116160, 233427456, 216064512, 280375808, 384098816, 448410112, 1106432, 65417728, 169140736, 233452032, 216089088, 280400384, 384123392, 448434688},
     {4326144, 173232896, 676463360, 845370112, 864256768, 1033163520, 1536393984, 1705300736, 4424448, 173331200, 676561664, 845468416, 864355072, 1033261824, 1536492288, 1705399040}},
};

static void phase_a_workspace_layout(bool print) {
    for (int ci = 0; ci < 7; ++ci) {
        const WsCase& c = kWsCases[ci];
        std::vector<double> sv((size_t)c.M * c.D, 0.0), dc((size_t)(c.C - 1) * c.M, 0.0);
        std::vector<int32_t> ns(c.C, 0);
        ns[0] = (int32_t)c.M;
        rml_svm m;
        rml_svm_pack pk;
        CHECK(rml_svm_pack_host(sv.data(), c.M, c.D, dc.data(), ns.data(), c.C, RML_KERNEL_RBF, 0.01, 255.0, false, &m, &pk) == RML_OK);
        if (print) printf("    {");
        for (int hi = 0; hi < 2; ++hi) {
            if (print) printf("%s{", hi ? ",\n     " : "");
            for (unsigned needs = 0; needs < 16; ++needs) {
                const size_t b = rml_svm_ws_bytes(&m, kWsChunks[hi], needs);
                if (print) printf("%zu%s", b, needs < 15 ? ", " : "}");
                else CHECK(b == kWsBytes[ci][hi][needs]);
            }
        }
        if (print) printf("},\n");
    }
}

static void phase_a_thread_local_errors() {
    // rml_last_error is thread-local: four threads fail differently at the same time and each reads its own message
    std::vector<std::thread> ts;
    int ok[4] = {0, 0, 0, 0};
    for (int t = 0; t < 4; ++t)
        ts.emplace_back([t, &ok] {
            float f = 0; double d = 0; int32_t i3[3] = {1, 1, 1}; rml_svm* m = nullptr; rml_svm sm; rml_svm_pack pk;
            int good = 1;
            for (int it = 0; it < 200; ++it) {
                const char* want = nullptr;
                if (t == 0) { (void)rml_svm_pack_host(&d, 3, 1, &d, i3, 9, RML_KERNEL_RBF, 0.1, 255.0, false, &sm, &pk); want = "classes"; }
                else if (t == 1) { (void)rml_svm_pack_host(&d, 5, 1, &d, i3, 3, RML_KERNEL_RBF, 0.1, 255.0, false, &sm, &pk); want = "n_support"; }
                else if (t == 2) { (void)rml_svm_load(nullptr, &d, 1, 1, &d, &d, i3, 3, RML_KERNEL_RBF, 0.1, 255.0, nullptr, nullptr, &m); want = "NULL"; }
                else { (void)rml_probe_stream(nullptr, &f, 4, 1, &d, nullptr); want = "rml_probe_stream"; }
                good &= strstr(rml_last_error(), want) != nullptr;
            }
            ok[t] = good;
        });
    for (auto& th : ts) th.join();
    CHECK(ok[0] && ok[1] && ok[2] && ok[3]);
}

// the two host-side steps of SVC(probability=True).fit: every length from 0 (exact-size heap buffers: an index one past the end is a
// report), a permutation out, finite A / B on separable, constant, empty and huge decision values, bad arguments as statuses
static void phase_a_platt() {
    for (int64_t l : {0, 1, 2, 3, 5, 118, 4860}) {
        std::vector<int32_t> perm((size_t)l);
        std::vector<char> seen((size_t)l, 0);
        CHECK(rml_libsvm_shuffle(1234u + (uint32_t)l, l, perm.data()) == RML_OK);
        bool is_perm = true;
        for (int64_t i = 0; i < l; ++i) {
            is_perm &= perm[(size_t)i] >= 0 && perm[(size_t)i] < l && !seen[(size_t)perm[(size_t)i]];
            if (perm[(size_t)i] >= 0 && perm[(size_t)i] < l) seen[(size_t)perm[(size_t)i]] = 1;
        }
        CHECK(is_perm);
        std::vector<int32_t> again((size_t)l);
        CHECK(rml_libsvm_shuffle(1234u + (uint32_t)l, l, again.data()) == RML_OK && perm == again);
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<double> dec((size_t)l), y((size_t)l);
            for (int64_t i = 0; i < l; ++i) {
                y[(size_t)i] = (i & 1) ? -1.0 : 1.0;
                const double noise = (double)(rnd() % 2001) / 1000.0 - 1.0;
                dec[(size_t)i] = kind == 0 ? y[(size_t)i] + 0.5 * noise : kind == 1 ? 1.0 : kind == 2 ? 1e6 * y[(size_t)i] : noise;
            }
            double A = NAN, B = NAN;
            int info = -1;
            CHECK(rml_platt_fit(dec.data(), y.data(), l, &A, &B, &info) == RML_OK);
            CHECK(isfinite(A) && isfinite(B) && info >= RML_PLATT_OK && info <= RML_PLATT_MAX_ITER);
            CHECK(rml_platt_fit(dec.data(), y.data(), l, &A, &B, nullptr) == RML_OK);
        }
    }
    double d = 0;
    int32_t i32 = 0;
    CHECK(rml_libsvm_shuffle(1, -1, &i32) == RML_ERR_INVALID && strlen(rml_last_error()) > 0);
    CHECK(rml_libsvm_shuffle(1, 3, nullptr) == RML_ERR_INVALID && rml_libsvm_shuffle(1, 0, nullptr) == RML_OK);
    CHECK(rml_platt_fit(nullptr, &d, 1, &d, &d, nullptr) == RML_ERR_INVALID && rml_platt_fit(&d, &d, 1, nullptr, &d, nullptr) == RML_ERR_INVALID);
    CHECK(rml_platt_fit(&d, &d, -1, &d, &d, nullptr) == RML_ERR_INVALID);
}

// ---- phase B (a device is present) -----------------------------------------------------------------------------------------
#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); ++g_fail; return; } } while (0)

// rml_gram's argument validation on a live context: every bad argument is a status and a message, before any device work
static void phase_b_gram_arguments(rml_ctx* ctx) {
    float f = 0; double d = 0;
    const int kd[2] = {RML_GRAM_LINEAR, RML_GRAM_RBF}, bad_kind[2] = {RML_GRAM_LINEAR, 7};
    const double gm[2] = {0.0, 0.5}, g_nan[2] = {0.0, NAN}, g_inf[2] = {0.0, INFINITY}, g_neg[2] = {0.0, -1.0};
    const int64_t N = 4, D = 8;
    CHECK(rml_gram(ctx, nullptr, D, N, D, 2, kd, gm, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, gm, nullptr, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, nullptr, gm, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, nullptr, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D - 1, N, D, 2, kd, gm, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, gm, &d, N - 1, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, gm, &d, N, N * N - 1, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 0, kd, gm, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 9, kd, gm, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, bad_kind, gm, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, g_nan, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, g_inf, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(rml_gram(ctx, &f, D, N, D, 2, kd, g_neg, &d, N, N * N, nullptr) == RML_ERR_INVALID);
    CHECK(strlen(rml_last_error()) > 0);
    CHECK(rml_gram(ctx, nullptr, D, 0, D, 2, kd, gm, nullptr, 0, 0, nullptr) == RML_OK);       // N == 0: a no-op
}

// rml_smo_solve / rml_smo_score: every bad descriptor is a status and a message, before any device work
static void phase_b_smo_arguments(rml_ctx* ctx) {
    double d = 0;
    int32_t i32 = 0;
    const int64_t N = 4;
    rml_smo_problem ok{};
    ok.matrix = 0; ok.l = 4; ok.n_pos = 2; ok.shrinking = 1; ok.max_iter = -1; ok.rows_off = 0; ok.alpha_off = 0; ok.Cp = 1.0; ok.Cn = 1.0; ok.eps = 1e-3;
    auto solve = [&](const rml_smo_problem& p, int64_t n_rows = 4, int64_t n_alpha = 4, int n_mats = 1) {
        return rml_smo_solve(ctx, &d, N, N, N * N, n_mats, &p, 1, &i32, n_rows, &d, n_alpha, &d, &i32, &i32, nullptr);
    };
    rml_smo_problem p = ok;
    p.matrix = 1; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.l = 0; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.n_pos = 5; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.rows_off = 1; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.alpha_off = -1; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.Cp = 0.0; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.Cn = NAN; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.eps = -1e-3; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    p.max_iter = -2; CHECK(solve(p) == RML_ERR_INVALID); p = ok;
    CHECK(solve(ok, 3) == RML_ERR_INVALID && solve(ok, 4, 3) == RML_ERR_INVALID && solve(ok, 4, 4, 0) == RML_ERR_INVALID);
    CHECK(strlen(rml_last_error()) > 0);
    CHECK(rml_smo_solve(ctx, &d, N, N - 1, N * N, 1, &ok, 1, &i32, 4, &d, 4, &d, &i32, &i32, nullptr) == RML_ERR_INVALID);
    CHECK(rml_smo_solve(ctx, nullptr, N, N, N * N, 1, &ok, 1, &i32, 4, &d, 4, &d, &i32, &i32, nullptr) == RML_ERR_INVALID);
    CHECK(rml_smo_solve(ctx, nullptr, N, N, N * N, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == RML_OK);   // no problems: a no-op
    rml_smo_fit f{};
    f.prob0 = 0; f.n_test = 2; f.test_off = 0;
    auto score = [&](const rml_smo_fit& ff, int n_classes, int64_t n_test_total) {
        return rml_smo_score(ctx, &d, N, N, N * N, 1, &ok, 1, &i32, 4, &d, 4, &d, n_classes, &ff, 1, &i32, &i32, n_test_total, &d, &i32, &i32, nullptr);
    };
    CHECK(score(f, 1, 2) == RML_ERR_INVALID && score(f, 9, 2) == RML_ERR_INVALID);
    CHECK(score(f, 3, 2) == RML_ERR_INVALID);          // three classes need three pair problems, one given
    CHECK(score(f, 2, 1) == RML_ERR_INVALID);          // held-out rows past the list
    rml_smo_fit g = f;
    g.prob0 = 1; CHECK(score(g, 2, 2) == RML_ERR_INVALID);
    int32_t cnt[1];
    CHECK(rml_smo_score(ctx, &d, N, N, N * N, 1, &ok, 1, &i32, 4, &d, 4, &d, 2, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, cnt, nullptr) == RML_OK);
}

static void phase_b(rml_ctx* ctx) {
    const int X = 22, Y = 31, Z = 176, C = 3;
    const int64_t B = 9000, M = 300;                   // two pipeline chunks (8192 + 808)
    const int64_t D = rml_feature_len(X, Y, Z, RML_MASK_ALL), vox = (int64_t)X * Y * Z;
    std::vector<float> vol((size_t)B * vox, 0.f);
    for (int64_t b = 0; b < B; ++b)
        for (int k = 0; k < 40; ++k) vol[(size_t)b * vox + rnd() % vox] = (float)(13 + rnd() % 243);
    std::vector<double> sv((size_t)M * D), dc((size_t)(C - 1) * M), ic(3), ca(3, -1.5), cb(3, 0.1);
    for (double& v : sv) v = (rnd() % 8) ? 0.0 : (double)((float)(rnd() % 256) / 255.0f);
    for (double& v : dc) v = ((double)(rnd() % 2001) - 1000.0) / 100.0;
    for (double& v : ic) v = ((double)(rnd() % 2001) - 1000.0) / 1000.0;
    int32_t ns[3] = {100, 100, 100};
    rml_svm* m = nullptr;
    CHECK(rml_svm_load(ctx, sv.data(), M, D, dc.data(), ic.data(), ns, C, RML_KERNEL_RBF, 0.01, 255.0, ca.data(), cb.data(), &m) == RML_OK);
    if (!m) return;
    CHECK(rml_svm_is_exact(m) == 1);
    float* dV = nullptr;
    HIPCK(hipMalloc(&dV, vol.size() * sizeof(float)));
    HIPCK(hipMemcpy(dV, vol.data(), vol.size() * sizeof(float), hipMemcpyHostToDevice));
    const int NT = 4;
    std::vector<std::vector<double>> dec(NT, std::vector<double>((size_t)B * 3));
    std::vector<std::vector<int32_t>> lab(NT, std::vector<int32_t>((size_t)B));
    hipStream_t st[2];
    HIPCK(hipStreamCreate(&st[0]));
    HIPCK(hipStreamCreate(&st[1]));
    int bad[NT] = {0, 0, 0, 0};
    std::vector<std::thread> ts;
    for (int t = 0; t < NT; ++t)
        ts.emplace_back([&, t] {
            double* d_dec = nullptr; double* d_pr = nullptr; int32_t* d_lv = nullptr; int32_t* d_lc = nullptr;
            if (hipSetDevice(rml_ctx_device(ctx)) != hipSuccess || hipMalloc(&d_dec, B * 3 * 8) != hipSuccess || hipMalloc(&d_pr, B * 3 * 8) != hipSuccess ||
                hipMalloc(&d_lv, B * 4) != hipSuccess || hipMalloc(&d_lc, B * 4) != hipSuccess) { bad[t] = 1; return; }
            for (int it = 0; it < 6; ++it) {
                int rc = rml_project_svm(ctx, m, dV, RML_VOL_F32, B, X, Y, Z, RML_MODE_MAX, nullptr, 255.f, RML_MASK_ALL, d_dec, nullptr, d_pr, d_lv, d_lc, st[t & 1]);
                if (rc != RML_OK) { fprintf(stderr, "thread %d: %s\n", t, rml_last_error()); bad[t] = 1; break; }
            }
            if (hipStreamSynchronize(st[t & 1]) != hipSuccess) bad[t] = 1;
            if (hipMemcpy(dec[t].data(), d_dec, B * 3 * 8, hipMemcpyDeviceToHost) != hipSuccess) bad[t] = 1;
            if (hipMemcpy(lab[t].data(), d_lc, B * 4, hipMemcpyDeviceToHost) != hipSuccess) bad[t] = 1;
            (void)hipFree(d_dec); (void)hipFree(d_pr); (void)hipFree(d_lv); (void)hipFree(d_lc);
        });
    for (auto& th : ts) th.join();
    for (int t = 0; t < NT; ++t) {
        CHECK(!bad[t]);
        CHECK(memcmp(dec[t].data(), dec[0].data(), dec[0].size() * 8) == 0);
        CHECK(memcmp(lab[t].data(), lab[0].data(), lab[0].size() * 4) == 0);
    }
    int hist[3] = {0, 0, 0};
    for (int32_t l : lab[0]) { CHECK(l >= 0 && l < 3); if (l >= 0 && l < 3) hist[l]++; }
    printf("phase B: %lld frames x %d threads on 2 streams, one context: identical results (labels %d/%d/%d)\n", (long long)B, NT, hist[0], hist[1], hist[2]);
    (void)hipStreamDestroy(st[0]); (void)hipStreamDestroy(st[1]);
    (void)hipFree(dV);
    CHECK(rml_svm_free(ctx, m) == RML_OK);
}

int main(int argc, char** argv) {
    const bool need_device = argc > 1 && strcmp(argv[1], "--need-device") == 0;
    if (argc > 1 && strcmp(argv[1], "--print-ws-table") == 0) { phase_a_workspace_layout(true); return 0; }
    phase_a_arguments();
    phase_a_pillow_tables();
    phase_a_model_packing();
    phase_a_workspace_layout(false);
    phase_a_thread_local_errors();
    phase_a_platt();
    printf("phase A: %s\n", g_fail ? "FAILED" : "ok");
    rml_ctx* ctx = nullptr;
    const int rc = rml_ctx_create(0, &ctx);
    if (rc != RML_OK) {
        // no GPU (or a host-only library): the failure must be a status with a message, and leave nothing behind
        CHECK(ctx == nullptr && strlen(rml_last_error()) > 0);
        printf("phase B: skipped, rml_ctx_create(0) = %d (%s)\n", rc, rml_last_error());
        if (need_device) { fprintf(stderr, "a device was required\n"); ++g_fail; }
    } else {
        phase_b_gram_arguments(ctx);
        phase_b_smo_arguments(ctx);
        phase_b(ctx);
        CHECK(rml_ctx_destroy(ctx) == RML_OK);
    }
    printf("%s (%d failed checks)\n", g_fail ? "FAILED" : "ALL OK", g_fail);
    return g_fail ? 1 : 0;
}
