// shape_lenet alone (csrc/launch.cpp + plan.cpp, no HIP, no library), built with the address and
// undefined-behaviour sanitizers and run as an ordinary process (tests/test_lenet_abi.py).  Over
// n_agents x batch x compute units x {gradient, forward-only} it checks what must hold of any
// shaped call: every pass and every group of every agent is walked exactly once by the
// workgroups of its kernel, the grids are n_agents * wpa, the workspace regions are disjoint,
// large enough for what the kernels keep in them and inside dl_lenet_workspace_bytes, and the
// launch count follows the outputs; and of its steps: every GEMM passes dl_bgemm's own check,
// every operand a step reads is an input or lies in what an earlier step wrote, every extent a
// step writes lies inside one workspace region or inside G, loss or logits, and with G the
// written extents of an agent's row tile the parameters [0, P).  Then the refusals that need a
// plausible workspace, and tests/golden/lenet_launches.txt (format: test_lenet_abi.py) replayed
// step for step and field for field.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <utility>
#include <vector>

#include "launch.h"
#include "launch_table.h"

static int fails = 0, calls = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static dl_lenet_args base(int32_t n, int32_t b, int32_t nc) {
    dl_lenet_args a;
    std::memset(&a, 0, sizeof a);
    const int64_t P = dl::lenet_param_count(nc), ld = (P + 63) / 64 * 64;
    a.n_agents = n; a.batch = b; a.num_classes = nc;
    a.X = (const float *)(1ull << 40); a.ldx = ld;
    a.data = (const float *)(1ull << 44); a.s_data = (int64_t)b * 3072;
    a.labels = (const int32_t *)(1ull << 48); a.s_labels = b;
    a.G = (float *)(1ull << 50); a.ldg = ld;
    a.loss = (float *)(1ull << 52);
    return a;
}
static void *const WS = (void *)(1ull << 54);

// workgroup w of an agent walks items w, w + wpa, ...: every item exactly once
static bool walked_once(int32_t items, int32_t wpa) {
    if (wpa < 1 || wpa > items) return false;
    std::vector<int> seen((size_t)items, 0);
    for (int32_t w = 0; w < wpa; ++w)
        for (int32_t i = w; i < items; i += wpa) ++seen[(size_t)i];
    return std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; });
}

// the workspace regions and what the kernels keep in each
struct R { size_t off, bytes; };
static std::vector<R> regions(const dl::LenetWs &w, int64_t n, int64_t b, int64_t nc) {
    const int64_t nb = n * b, groups = (b + dl::kLenetGroup - 1) / dl::kLenetGroup;
    return {{w.pool1, (size_t)nb * 1176 * 4}, {w.code1, (size_t)nb * 1176},
            {w.pool2, (size_t)nb * 400 * 4},  {w.code2, (size_t)nb * 400},
            {w.h1, (size_t)nb * 120 * 4},     {w.h2, (size_t)nb * 84 * 4},
            {w.z, (size_t)(nb * nc) * 4},     {w.dz3, (size_t)(nb * nc) * 4},
            {w.dz2, (size_t)nb * 84 * 4},     {w.dz1, (size_t)nb * 120 * 4},
            {w.da, (size_t)nb * 400 * 4},     {w.part, (size_t)(n * groups) * 2872 * 4}};
}

static void check_workspace(const dl::LenetWs &w, int64_t n, int64_t b, int64_t nc) {
    const std::vector<R> r = regions(w, n, b, nc);
    for (int i = 0; i < 12; ++i) {
        EXPECT(r[i].off % 16 == 0 && r[i].bytes > 0 && r[i].off + r[i].bytes <= w.total);
        for (int j = i + 1; j < 12; ++j)
            EXPECT(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off);
    }
}

// A span of bytes an operand covers.
struct Span { uintptr_t at; size_t n; };
static Span span(const void *p, size_t bytes) { return Span{(uintptr_t)p, bytes}; }
static bool inside(const Span &s, const Span &o) { return o.at <= s.at && s.at + s.n <= o.at + o.n; }
// a GEMM operand of `rows` x `cols` floats: (batch - 1) stride + (rows - 1) ld + cols floats
static Span mat(const float *p, int64_t batch, int64_t stride, int64_t rows, int64_t ld,
                int64_t cols) {
    return span(p, (size_t)((batch - 1) * stride + (rows - 1) * ld + cols) * 4);
}

static dl_bgemm_args abi(const dl::BgemmArgs &g) {
    dl_bgemm_args a;
    std::memset(&a, 0, sizeof a);
    a.batch = g.batch; a.M = g.M; a.N = g.N; a.K = g.K;
    a.A = g.A; a.lda = g.lda; a.sA = g.sA; a.ta = g.ta;
    a.B = g.B; a.ldb = g.ldb; a.sB = g.sB; a.tb = g.tb;
    a.C = g.C; a.ldc = g.ldc; a.sC = g.sC;
    a.epi = g.epi; a.bias = g.bias; a.s_bias = g.sBias;
    a.H = g.H; a.ldh = g.ldh; a.sH = g.sH;
    a.rowsum = g.rowsum; a.s_rowsum = g.sR;
    a.labels = g.labels; a.s_labels = g.sLab; a.loss = g.loss;
    return a;
}

// what must hold of the steps of any shaped call
static void check_steps(const dl_lenet_args &a, void *ws, const dl::LenetPlan &p) {
    char err[dl::kErrLen];
    const int64_t N = a.n_agents, B = a.batch, nc = a.num_classes;
    const int64_t P = dl::lenet_param_count(a.num_classes);
    EXPECT(p.n_launches >= 3 && p.n_launches <= dl::kLenetMaxLaunches - 1);
    const std::vector<Span> inputs = {
        span(a.X, (size_t)((N - 1) * a.ldx + P) * 4),
        span(a.data, (size_t)((N - 1) * a.s_data + B * dl::kLenetImage) * 4),
        span(a.labels, a.labels ? (size_t)((N - 1) * a.s_labels + B) * 4 : 0)};
    std::vector<Span> homes;   // where a step may write: one workspace region, G, loss, logits
    for (const R &r : regions(p.ws, N, B, nc)) homes.push_back(span((char *)ws + r.off, r.bytes));
    if (a.G) homes.push_back(span(a.G, (size_t)((N - 1) * a.ldg + P) * 4));
    if (a.loss) homes.push_back(span(a.loss, (size_t)N * 4));
    if (a.logits)
        homes.push_back(span(a.logits, (size_t)((N - 1) * a.s_logits + (B - 1) * a.ldz + nc) * 4));
    std::vector<Span> written;
    std::vector<std::pair<int64_t, int64_t>> grow;   // agent 0's written floats of G: [from, to)
    auto in_any = [](const Span &s, const std::vector<Span> &of) {
        return std::any_of(of.begin(), of.end(), [&](const Span &o) { return inside(s, o); });
    };
    auto g_block = [&](const float *at, int64_t rows, int64_t ld, int64_t cols) {
        for (int64_t r = 0; r < rows; ++r) grow.push_back({at - a.G + r * ld, at - a.G + r * ld + cols});
    };
    const dl::LenetConvArgs &cv = p.conv;
    const int64_t groups = p.groups;
    for (int i = 0; i < p.n_launches; ++i) {
        const dl::LenetStep &st = p.step[i];
        std::vector<Span> reads, writes;
        switch (st.kind) {
            case dl::kLenetConvFwd:
                EXPECT(i == 0);
                reads = {span(cv.X, (size_t)((N - 1) * cv.ldx + dl::kLenetConvParams) * 4),
                         span(cv.data, (size_t)((N - 1) * cv.s_data + B * dl::kLenetImage) * 4)};
                writes = {span(cv.pool2, (size_t)(N * B) * 400 * 4)};
                if (cv.train) {
                    writes.push_back(span(cv.pool1, (size_t)(N * B) * 1176 * 4));
                    writes.push_back(span(cv.code1, (size_t)(N * B) * 1176));
                    writes.push_back(span(cv.code2, (size_t)(N * B) * 400));
                }
                break;
            case dl::kLenetGemm: {
                const dl::BgemmArgs &g = st.gemm;
                const dl_bgemm_args ga = abi(g);
                EXPECT(dl::check_bgemm(&ga, err) == DL_OK);
                EXPECT(g.batch == N);
                reads = {mat(g.A, N, g.sA, g.ta ? g.K : g.M, g.lda, g.ta ? g.M : g.K),
                         mat(g.B, N, g.sB, g.tb ? g.N : g.K, g.ldb, g.tb ? g.K : g.N)};
                if (g.epi >= dl::EPI_BIAS && g.epi <= dl::EPI_BIAS_ELU) EXPECT(g.bias != nullptr);
                if (g.epi == dl::EPI_BIAS_XENT) EXPECT(g.bias != nullptr);
                if (g.bias) reads.push_back(mat(g.bias, N, g.sBias, 1, 0, g.N));
                if (g.H) reads.push_back(mat(g.H, N, g.sH, g.M, g.ldh, g.N));
                if (g.labels) reads.push_back(span(g.labels, (size_t)((N - 1) * g.sLab + g.M) * 4));
                writes = {mat(g.C, N, g.sC, g.M, g.ldc, g.N)};
                if (g.rowsum) writes.push_back(mat(g.rowsum, N, g.sR, 1, 0, g.M));
                if (g.loss) writes.push_back(span(g.loss, (size_t)N * 4));
                if (a.G && inside(writes[0], homes[12])) {   // a weight gradient and its bias's
                    EXPECT(g.sC == a.ldg && g.rowsum && g.sR == a.ldg);
                    g_block(g.C, g.M, g.ldc, g.N);
                    g_block(g.rowsum, 1, 0, g.M);
                }
                break;
            }
            case dl::kLenetHead: {
                const dl::XentArgs &h = st.head;
                EXPECT(h.batch == N && h.rows == B && h.classes == nc && nc <= 64);
                EXPECT(N == 1 || h.sD >= B * nc);
                reads = {mat(h.Z, N, h.sZ, 1, 0, B * nc),
                         span(h.y, (size_t)((N - 1) * h.sY + B) * 4)};
                writes = {mat(h.dZ, N, h.sD, 1, 0, B * nc)};
                if (h.loss) writes.push_back(span(h.loss, (size_t)N * 4));
                break;
            }
            case dl::kLenetConvBwd:
                EXPECT(cv.train && i == p.n_launches - 2);
                reads = {span(cv.X, (size_t)((N - 1) * cv.ldx + dl::kLenetConvParams) * 4),
                         span(cv.data, (size_t)((N - 1) * cv.s_data + B * dl::kLenetImage) * 4),
                         span(cv.pool1, (size_t)(N * B) * 1176 * 4),
                         span(cv.code1, (size_t)(N * B) * 1176),
                         span(cv.code2, (size_t)(N * B) * 400),
                         span(cv.da, (size_t)(N * B) * 400 * 4)};
                writes = {span(cv.part, (size_t)(N * groups) * dl::kLenetConvParams * 4)};
                break;
            case dl::kLenetConvReduce:
                EXPECT(cv.train && i == p.n_launches - 1 && cv.G == a.G && cv.ldg == a.ldg);
                reads = {span(cv.part, (size_t)(N * groups) * dl::kLenetConvParams * 4)};
                writes = {mat(cv.G, N, cv.ldg, 1, 0, dl::kLenetConvParams)};
                g_block(cv.G, 1, 0, dl::kLenetConvParams);
                break;
            default: EXPECT(!"a step kind");
        }
        for (const Span &r : reads) EXPECT(r.n > 0 && (in_any(r, inputs) || in_any(r, written)));
        for (const Span &w : writes) EXPECT(w.n > 0 && in_any(w, homes));
        written.insert(written.end(), writes.begin(), writes.end());
    }
    if (a.G) {   // the row's blocks [0, P), every float once
        std::sort(grow.begin(), grow.end());
        int64_t end = 0;
        for (const auto &b : grow) {
            EXPECT(b.first == end);
            end = b.second;
        }
        EXPECT(end == P);
    } else {
        EXPECT(grow.empty());
    }
}

static std::string fmt_steps(const dl::LenetPlan &p) {
    using namespace launch_table;
    std::string s = "0 " + std::to_string(p.n_launches) + " ";
    for (int i = 0; i < p.n_launches; ++i) {
        const dl::LenetStep &st = p.step[i];
        const dl::XentArgs &h = st.head;
        s += fmt_event(i);
        switch (st.kind) {
            case dl::kLenetConvFwd: s += fmt_conv("fwd", p.conv, p.fwd_grid); break;
            case dl::kLenetGemm: s += fmt_gemm(st.gemm); break;
            case dl::kLenetHead:
                s += fmt_head(h.Z, h.sZ, h.y, h.sY, h.dZ, h.sD, h.loss, h.batch, h.rows, h.classes);
                break;
            case dl::kLenetConvBwd: s += fmt_conv("bwd", p.conv, p.bwd_grid); break;
            default: s += fmt_conv("reduce", p.conv, p.n_agents);
        }
    }
    return s + fmt_event(p.n_launches);
}

// the table: every call's steps as the commit before the step list launched them
static void replay(const char *path) {
    std::ifstream in(path);
    std::string line;
    int n = 0;
    for (; std::getline(in, line); ++n) {
        launch_table::LenetCase c;
        launch_table::parse(line, &c);
        EXPECT(c.ok);
        const dl_lenet_args &a = c.a;
        void *ws = launch_table::at<void>(launch_table::WS);
        char err[dl::kErrLen] = "";
        dl::LenetPlan p;
        ++calls;
        const int rc = dl::shape_lenet(&a, 256, ws,
                                       dl::lenet_workspace(a.n_agents, a.batch, a.num_classes).total,
                                       &p, err);
        const std::string got = rc ? std::to_string(rc) + " " + err : fmt_steps(p);
        if (rc == 0) check_steps(a, ws, p);
        if (got != c.want) {
            std::printf("FAILED table line %d: got %s\n", n + 1, got.c_str());
            ++fails;
        }
    }
    EXPECT(n >= 72);   // the lines of the committed table
}

int main(int argc, char **argv) {
    char err[dl::kErrLen];
    const int32_t agents[] = {1, 2, 63, 64, 257, 65535}, batches[] = {1, 5, 64, 80, 1000};
    const int cus[] = {1, 256};
    for (int32_t n : agents)
        for (int32_t b : batches)
            for (int cu : cus)
                for (int mode = 0; mode < 3; ++mode) {   // gradient, loss only, logits only
                    const int32_t nc = 10;
                    dl_lenet_args a = base(n, b, nc);
                    if (mode >= 1) a.G = nullptr;
                    if (mode == 2) {
                        a.loss = nullptr; a.labels = nullptr;
                        a.logits = (float *)(1ull << 53); a.ldz = 16; a.s_logits = (int64_t)b * 16;
                        a.s_data = 0;
                    }
                    const size_t need = dl::lenet_workspace(n, b, nc).total;
                    dl::LenetPlan p;
                    ++calls;
                    EXPECT(dl::shape_lenet(&a, cu, WS, need, &p, err) == DL_OK);
                    EXPECT(p.train == (mode == 0));
                    EXPECT(p.head == (mode == 2 ? 0 : (b <= 64 ? 1 : 2)));
                    EXPECT(p.n_launches == 3 + (mode == 2) + p.head + (mode == 0 ? 8 : 0));
                    EXPECT(p.n_launches + 1 <= dl::kLenetMaxLaunches);
                    check_steps(a, WS, p);
                    EXPECT(p.passes == (b + dl::kLenetFwdImages - 1) / dl::kLenetFwdImages);
                    EXPECT(p.groups == (b + dl::kLenetGroup - 1) / dl::kLenetGroup);
                    EXPECT(walked_once(p.passes, p.fwd_wpa) && walked_once(p.groups, p.bwd_wpa));
                    EXPECT((int64_t)p.fwd_grid == (int64_t)n * p.fwd_wpa && p.fwd_grid > 0);
                    EXPECT((int64_t)p.bwd_grid == (int64_t)n * p.bwd_wpa && p.bwd_grid > 0);
                    // enough workgroups for the compute units where the work allows it
                    const int64_t want = ((int64_t)dl::kLenetWgPerCu * cu + n - 1) / n;
                    EXPECT(p.fwd_wpa == std::min<int64_t>(want, p.passes));
                    EXPECT(p.bwd_wpa == std::min<int64_t>(want, p.groups));
                    EXPECT(p.ws.total == need && need == dl::lenet_workspace(n, b, nc).total);
                    check_workspace(p.ws, n, b, nc);
                    // one byte short, a null and a misaligned workspace
                    EXPECT(dl::shape_lenet(&a, cu, WS, need - 1, &p, err) == DL_ERR_WORKSPACE);
                    EXPECT(dl::shape_lenet(&a, cu, nullptr, need, &p, err) == DL_ERR_WORKSPACE);
                    EXPECT(dl::shape_lenet(&a, cu, (char *)WS + 8, need + 8, &p, err) ==
                           DL_ERR_WORKSPACE);
                }
    // the class range: 1 and 64 shape, the workspace follows num_classes
    for (int32_t nc : {1, 3, 64}) {
        dl_lenet_args a = base(3, 7, nc);
        dl::LenetPlan p;
        const size_t need = dl::lenet_workspace(3, 7, nc).total;
        EXPECT(dl::shape_lenet(&a, 256, WS, need, &p, err) == DL_OK);
        check_workspace(p.ws, 3, 7, nc);
        check_steps(a, WS, p);
    }
    // n_cus = 0 counts as one compute unit; the check alone (no plan)
    {
        dl_lenet_args a = base(2, 64, 10);
        dl::LenetPlan p;
        const size_t need = dl::lenet_workspace(2, 64, 10).total;
        EXPECT(dl::shape_lenet(&a, 0, WS, need, &p, err) == DL_OK && p.fwd_wpa == 2);
        EXPECT(dl::shape_lenet(&a, 256, WS, need, nullptr, err) == DL_OK);
        // touching operands do not overlap; one element further they do
        const size_t gb = ((size_t)a.ldg + (size_t)dl::lenet_param_count(10)) * 4;
        a.loss = (float *)((char *)a.G + gb);
        EXPECT(dl::shape_lenet(&a, 256, WS, need, &p, err) == DL_OK);
        a.loss = (float *)((char *)a.G + gb - 4);
        EXPECT(dl::shape_lenet(&a, 256, WS, need, &p, err) == DL_ERR_INVALID &&
               std::strstr(err, "G overlaps loss"));
        a = base(2, 64, 10);
        EXPECT(dl::shape_lenet(&a, 256, (char *)a.X - need, need, &p, err) == DL_OK);
        EXPECT(dl::shape_lenet(&a, 256, (char *)a.X - need + 16, need, &p, err) ==
                   DL_ERR_INVALID && std::strstr(err, "workspace overlaps X"));
        EXPECT(dl::shape_lenet(&a, 256, (char *)a.loss, need, &p, err) == DL_ERR_INVALID &&
               std::strstr(err, "loss overlaps workspace"));
    }
    replay(argc > 1 ? argv[1] : "tests/golden/lenet_launches.txt");
    std::printf("%d calls, %d failures\n", calls, fails);
    return fails != 0;
}
