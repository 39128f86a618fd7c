// shape_mlp_grad and check_bgemm alone (csrc/launch.cpp + plan.cpp, no HIP, no library), built
// with the address and undefined-behaviour sanitizers and run as an ordinary process
// (tests/test_mlp_eval_abi.py).  One defect per call in otherwise valid arguments, with the status
// and the text dl_mlp_grad and dl_bgemm gave when their checks stood in capi.hip; operands that
// touch without overlapping pass.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "launch.h"

static int fails = 0, calls = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static char err[dl::kErrLen];

// 3 agents of the 32-16-16-16-4 network, row-major rows of ld floats; never dereferenced
constexpr int64_t P = 16 * 32 + 16 + 2 * (16 * 16 + 16) + 4 * 16 + 4, LD = (P + 3) / 4 * 4 + 8;
static char *const XP = (char *)(1ull << 40), *const GP = (char *)(1ull << 41);
static dl_mlp_args mlp() {
    dl_mlp_args a;
    std::memset(&a, 0, sizeof a);
    a.n_agents = 3; a.batch = 64; a.input_dim = 32; a.hidden_dim = 16; a.output_dim = 4;
    a.X = (const float *)XP; a.ldx = LD;
    a.data = (const float *)(1ull << 42); a.s_data = 64 * 32;
    a.labels = (const int32_t *)(1ull << 43); a.s_labels = 64;
    a.G = (float *)GP; a.ldg = LD;
    a.loss = (float *)(1ull << 44);
    return a;
}
template <class F>
static void mlp_refused(int rc, const char *text, F defect) {
    dl_mlp_args a = mlp();
    defect(a);
    err[0] = 0;
    ++calls;
    const int got = dl::shape_mlp_grad(&a, err);
    if (got != rc || std::strcmp(err, text)) {
        std::printf("FAILED: want %d %s\n        got %d %s\n", rc, text, got, err);
        ++fails;
    }
}
template <class F>
static void mlp_passes(F change) {
    dl_mlp_args a = mlp();
    change(a);
    ++calls;
    EXPECT(dl::shape_mlp_grad(&a, err) == DL_OK);
}

static dl_bgemm_args gemm() {
    dl_bgemm_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = 3; a.M = 5; a.N = 7; a.K = 9;
    a.A = (const float *)(1ull << 40); a.lda = 9; a.sA = 45;
    a.B = (const float *)(1ull << 41); a.ldb = 7; a.sB = 0;
    a.C = (float *)(1ull << 42); a.ldc = 7; a.sC = 35;
    return a;
}
template <class F>
static void gemm_refused(const char *text, F defect) {
    dl_bgemm_args a = gemm();
    defect(a);
    err[0] = 0;
    ++calls;
    const int got = dl::check_bgemm(&a, err);
    if (got != DL_ERR_INVALID || std::strcmp(err, text)) {
        std::printf("FAILED: want %s\n        got %d %s\n", text, got, err);
        ++fails;
    }
}
template <class F>
static void gemm_passes(F change) {
    dl_bgemm_args a = gemm();
    change(a);
    ++calls;
    EXPECT(dl::check_bgemm(&a, err) == DL_OK);
}

int main() {
    using A = dl_mlp_args;
    const int INV = DL_ERR_INVALID, UNS = DL_ERR_UNSUPPORTED;
    static_assert(dl::mlp_fused_supported(64, 32, 16, 4) && dl::mlp_fused_supported(64, 4, 152, 16) &&
                      !dl::mlp_fused_supported(63, 32, 16, 4) &&
                      !dl::mlp_fused_supported(64, 30, 16, 4) &&
                      !dl::mlp_fused_supported(64, 32, 154, 4) &&
                      !dl::mlp_fused_supported(64, 32, 15, 4) &&
                      !dl::mlp_fused_supported(64, 32, 16, 17) &&
                      !dl::mlp_fused_supported(64, 0, 16, 4) && !dl::mlp_fused_supported(64, 32, 0, 4) &&
                      !dl::mlp_fused_supported(64, 32, 16, 0), "the fused path's gate");
    static_assert(dl::mlp_workspace_floats(3) == 3 * 64 * 156, "one activation buffer per agent");

    ++calls;
    EXPECT(dl::shape_mlp_grad(nullptr, err) == INV && !std::strcmp(err, "dl_mlp_grad: null args"));
    mlp_passes([](A &) {});
    mlp_passes([](A &a) { a.n_agents = 0; a.X = nullptr; a.batch = 1; });   // nothing to launch
    mlp_passes([](A &a) { a.out_mode = 1; a.lr = 0.1f; a.loss = nullptr; });
    mlp_passes([](A &a) { a.tile_cols = 64; a.ldx = a.ldg = 0; });
    mlp_passes([](A &a) { a.tile_cols = 64; a.ldx = 0; a.ldg = 8; a.out_mode = 1; });
    mlp_refused(UNS, "dl_mlp_grad: fused path needs batch 64, input_dim % 4 == 0, even hidden_dim "
                     "<= 152, output_dim <= 16 (got 63, 32, 16, 4)", [](A &a) { a.batch = 63; });
    mlp_refused(UNS, "dl_mlp_grad: fused path needs batch 64, input_dim % 4 == 0, even hidden_dim "
                     "<= 152, output_dim <= 16 (got 64, 30, 16, 4)", [](A &a) { a.input_dim = 30; });
    mlp_refused(UNS, "dl_mlp_grad: fused path needs batch 64, input_dim % 4 == 0, even hidden_dim "
                     "<= 152, output_dim <= 16 (got 64, 32, 154, 4)",
                [](A &a) { a.hidden_dim = 154; });
    mlp_refused(UNS, "dl_mlp_grad: fused path needs batch 64, input_dim % 4 == 0, even hidden_dim "
                     "<= 152, output_dim <= 16 (got 64, 32, 16, 17)",
                [](A &a) { a.output_dim = 17; });
    const char *tile = "dl_mlp_grad: tile_cols must be 0 or a power of two >= 4";
    mlp_refused(INV, tile, [](A &a) { a.tile_cols = -4; });
    mlp_refused(INV, tile, [](A &a) { a.tile_cols = 2; });
    mlp_refused(INV, tile, [](A &a) { a.tile_cols = 48; });
    mlp_refused(INV, tile, [](A &a) { a.tile_cols = 1 << 30; });
    char bad[160];
    std::snprintf(bad, sizeof bad, "dl_mlp_grad: bad arguments (agents 3, params %lld, ldx %lld, "
                                   "ldg %lld)", (long long)P, (long long)LD, (long long)LD);
    mlp_refused(INV, bad, [](A &a) { a.X = nullptr; });
    mlp_refused(INV, bad, [](A &a) { a.data = nullptr; });
    mlp_refused(INV, bad, [](A &a) { a.labels = nullptr; });
    mlp_refused(INV, bad, [](A &a) { a.G = nullptr; });
    mlp_refused(INV, bad, [](A &a) { a.s_data = 64 * 32 - 4; });
    mlp_refused(INV, bad, [](A &a) { a.s_labels = 63; });
    std::snprintf(bad, sizeof bad, "dl_mlp_grad: bad arguments (agents 3, params %lld, ldx %lld, "
                                   "ldg %lld)", (long long)P, (long long)P - 4, (long long)LD);
    mlp_refused(INV, bad, [](A &a) { a.ldx = P - 4; });
    std::snprintf(bad, sizeof bad, "dl_mlp_grad: bad arguments (agents 65536, params %lld, ldx "
                                   "%lld, ldg %lld)", (long long)P, (long long)LD, (long long)LD);
    mlp_refused(INV, bad, [](A &a) { a.n_agents = 65536; });
    std::snprintf(bad, sizeof bad, "dl_mlp_grad: bad arguments (agents -1, params %lld, ldx %lld, "
                                   "ldg %lld)", (long long)P, (long long)LD, (long long)LD);
    mlp_refused(INV, bad, [](A &a) { a.n_agents = -1; });
    const char *al = "dl_mlp_grad: X, data, G must be 16-byte aligned with row strides % 4 == 0";
    mlp_refused(INV, al, [](A &a) { a.X = (const float *)(XP + 4); });
    mlp_refused(INV, al, [](A &a) { a.data = (const float *)((const char *)a.data + 8); });
    mlp_refused(INV, al, [](A &a) { a.G = (float *)(GP + 4); });
    mlp_refused(INV, al, [](A &a) { a.ldx = LD + 1; });
    mlp_refused(INV, al, [](A &a) { a.ldg = LD + 2; });
    mlp_refused(INV, al, [](A &a) { a.s_data = 64 * 32 + 2; });
    mlp_refused(UNS, "dl_mlp_grad: tiled X too large for 32-bit offsets",
                [](A &a) { a.tile_cols = 32768; a.n_agents = 65535; a.input_dim = 8192;
                           a.hidden_dim = 152; a.s_data = 64 * 8192; });
    // G against X: the bytes of 3 rows; touching passes, one float further in does not
    const int64_t xb = (2 * LD + P) * 4;
    mlp_passes([&](A &a) { a.G = (float *)(XP + (xb + 15) / 16 * 16); });
    mlp_passes([&](A &a) { a.G = (float *)(XP - (xb + 15) / 16 * 16); });
    static_assert((2 * LD + P) % 4 == 0, "the rows end on a 16-byte boundary: touching is exact");
    mlp_refused(INV, "dl_mlp_grad: G overlaps X", [&](A &a) { a.G = (float *)(XP + xb - 16); });
    mlp_refused(INV, "dl_mlp_grad: G overlaps X", [&](A &a) { a.G = (float *)(XP - xb + 16); });
    mlp_refused(INV, "dl_mlp_grad: G overlaps X", [](A &a) { a.G = (float *)XP; });
    // column-tiled: ceil(P / T) tiles of 3 agents x T floats
    const int64_t tb = (P + 63) / 64 * 64 * 3 * 4;
    mlp_passes([&](A &a) { a.tile_cols = 64; a.G = (float *)(XP + tb); });
    mlp_refused(INV, "dl_mlp_grad: G overlaps X",
                [&](A &a) { a.tile_cols = 64; a.G = (float *)(XP + tb - 16); });
    mlp_refused(INV, "dl_mlp_grad: out_mode must be 0 (gradient) or 1 (step)",
                [](A &a) { a.out_mode = 2; });
    mlp_refused(INV, "dl_mlp_grad: out_mode 1 needs ldg == ldx",
                [](A &a) { a.out_mode = 1; a.ldg = LD + 4; });
    // the split path's workspace: 3 activation buffers, against X and against G
    const int64_t wb = (int64_t)dl::mlp_workspace_floats(3) * 4;
    const char *wt = "dl_mlp_grad: workspace must be 16-byte aligned and disjoint from X and G";
    mlp_passes([](A &a) { a.workspace = (float *)(1ull << 45); });
    mlp_passes([&](A &a) { a.workspace = (float *)(XP - wb); });
    mlp_passes([&](A &a) { a.workspace = (float *)(XP + xb); });
    mlp_passes([&](A &a) { a.workspace = (float *)(GP - wb); });
    mlp_passes([&](A &a) { a.workspace = (float *)(GP + xb); });
    mlp_refused(INV, wt, [&](A &a) { a.workspace = (float *)(XP - wb + 16); });
    mlp_refused(INV, wt, [&](A &a) { a.workspace = (float *)(XP + xb - 16); });
    mlp_refused(INV, wt, [&](A &a) { a.workspace = (float *)(GP - wb + 16); });
    mlp_refused(INV, wt, [&](A &a) { a.workspace = (float *)(GP + xb - 16); });
    mlp_refused(INV, wt, [](A &a) { a.workspace = (float *)((1ull << 45) + 4); });
    // two defects: the earlier check wins
    mlp_refused(UNS, "dl_mlp_grad: fused path needs batch 64, input_dim % 4 == 0, even hidden_dim "
                     "<= 152, output_dim <= 16 (got 1, 32, 16, 4)",
                [](A &a) { a.batch = 1; a.X = nullptr; });
    mlp_refused(INV, tile, [](A &a) { a.tile_cols = 3; a.G = (float *)XP; });

    using B = dl_bgemm_args;
    const char *sz = "dl_bgemm: bad sizes/pointers/epilogue";
    ++calls;
    EXPECT(dl::check_bgemm(nullptr, err) == INV && !std::strcmp(err, sz));
    gemm_passes([](B &) {});
    gemm_refused(sz, [](B &a) { a.batch = 0; });
    gemm_refused(sz, [](B &a) { a.batch = 65536; });
    gemm_refused(sz, [](B &a) { a.M = 0; });
    gemm_refused(sz, [](B &a) { a.N = -1; });
    gemm_refused(sz, [](B &a) { a.K = 0; });
    gemm_refused(sz, [](B &a) { a.A = nullptr; });
    gemm_refused(sz, [](B &a) { a.B = nullptr; });
    gemm_refused(sz, [](B &a) { a.C = nullptr; });
    gemm_refused(sz, [](B &a) { a.epi = -1; });
    gemm_refused(sz, [](B &a) { a.epi = DL_EPI_BIAS_XENT + 1; });
    const char *ld = "dl_bgemm: leading dimension too small";
    gemm_refused(ld, [](B &a) { a.lda = 8; });
    gemm_refused(ld, [](B &a) { a.ta = 1; a.lda = 4; });
    gemm_passes([](B &a) { a.ta = 1; a.lda = 5; });
    gemm_refused(ld, [](B &a) { a.ldb = 6; });
    gemm_refused(ld, [](B &a) { a.tb = 1; a.ldb = 8; });
    gemm_passes([](B &a) { a.tb = 1; a.ldb = 9; });
    gemm_refused(ld, [](B &a) { a.ldc = 6; a.sC = 40; });
    const char *der = "dl_bgemm: derivative epilogue needs H with ldh >= N";
    for (int epi : {DL_EPI_DRELU, DL_EPI_DTANH, DL_EPI_DELU}) {
        gemm_refused(der, [&](B &a) { a.epi = epi; });
        gemm_refused(der, [&](B &a) { a.epi = epi; a.H = (const float *)(1ull << 43); a.ldh = 6; });
        gemm_passes([&](B &a) { a.epi = epi; a.H = (const float *)(1ull << 43); a.ldh = 7; });
    }
    const char *xe = "dl_bgemm: cross-entropy epilogue needs M <= 64 rows, N <= 64 classes and "
                     "labels";
    gemm_refused(xe, [](B &a) { a.epi = DL_EPI_BIAS_XENT; });
    const int32_t *lab = (const int32_t *)(1ull << 44);
    gemm_passes([&](B &a) { a.epi = DL_EPI_BIAS_XENT; a.labels = lab; });
    gemm_refused(xe, [&](B &a) { a.epi = DL_EPI_BIAS_XENT; a.labels = lab; a.M = 65;
                                 a.sC = 65 * 7; });
    gemm_refused(xe, [&](B &a) { a.epi = DL_EPI_BIAS_XENT; a.labels = lab; a.N = 65; a.ldb = 65;
                                 a.ldc = 65; a.sC = 5 * 65; });
    const char *st = "dl_bgemm: output batch stride smaller than one batch (sC >= (M-1)*ldc + N, "
                     "s_rowsum >= M)";
    gemm_refused(st, [](B &a) { a.sC = 34; });
    gemm_passes([](B &a) { a.sC = 34; a.batch = 1; });
    gemm_passes([](B &a) { a.ldc = 10; a.sC = 47; });
    gemm_refused(st, [](B &a) { a.ldc = 10; a.sC = 46; });
    gemm_refused(st, [](B &a) { a.rowsum = (float *)(1ull << 45); a.s_rowsum = 4; });
    gemm_passes([](B &a) { a.rowsum = (float *)(1ull << 45); a.s_rowsum = 5; });
    // two defects: the earlier check wins
    gemm_refused(sz, [](B &a) { a.M = 0; a.lda = 1; });
    gemm_refused(ld, [](B &a) { a.lda = 1; a.sC = 1; });
    // the kernel's parameter carries every field over
    {
        B a = gemm();
        a.epi = DL_EPI_BIAS_XENT; a.bias = (const float *)(1ull << 46); a.s_bias = 11;
        a.H = (const float *)(1ull << 43); a.ldh = 7; a.sH = 35;
        a.rowsum = (float *)(1ull << 45); a.s_rowsum = 5;
        a.labels = lab; a.s_labels = 5; a.loss = (float *)(1ull << 47);
        const dl::BgemmArgs p = dl::bgemm_args(a);
        EXPECT(p.batch == 3 && p.M == 5 && p.N == 7 && p.K == 9 && p.A == a.A && p.lda == 9 &&
               p.sA == 45 && p.ta == 0 && p.B == a.B && p.ldb == 7 && p.sB == 0 && p.tb == 0 &&
               p.C == a.C && p.ldc == 7 && p.sC == 35 && p.epi == a.epi && p.bias == a.bias &&
               p.sBias == 11 && p.H == a.H && p.ldh == 7 && p.sH == 35 && p.rowsum == a.rowsum &&
               p.sR == 5 && p.labels == lab && p.sLab == 5 && p.loss == a.loss);
    }
    std::printf("%d calls, %d failures\n", calls, fails);
    return fails != 0;
}
