// shape_lenet alone (csrc/launch.cpp + plan.cpp, no HIP, no library), built with the address and
// undefined-behaviour sanitizers and run as an ordinary process (tests/test_lenet_abi.py).  Over
// n_agents x batch x compute units x {gradient, forward-only} it checks what must hold of any
// shaped call: every pass and every group of every agent is walked exactly once by the
// workgroups of its kernel, the grids are n_agents * wpa, the workspace regions are disjoint,
// large enough for what the kernels keep in them and inside dl_lenet_workspace_bytes, and the
// launch count follows the outputs.  Then the refusals that need a plausible workspace.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "launch.h"

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

static void check_workspace(const dl::LenetWs &w, int64_t n, int64_t b, int64_t nc) {
    const int64_t nb = n * b, groups = (b + dl::kLenetGroup - 1) / dl::kLenetGroup;
    struct R { size_t off, bytes; };
    const R r[12] = {{w.pool1, (size_t)nb * 1176 * 4}, {w.code1, (size_t)nb * 1176},
                     {w.pool2, (size_t)nb * 400 * 4},  {w.code2, (size_t)nb * 400},
                     {w.h1, (size_t)nb * 120 * 4},     {w.h2, (size_t)nb * 84 * 4},
                     {w.z, (size_t)(nb * nc) * 4},     {w.dz3, (size_t)(nb * nc) * 4},
                     {w.dz2, (size_t)nb * 84 * 4},     {w.dz1, (size_t)nb * 120 * 4},
                     {w.da, (size_t)nb * 400 * 4},     {w.part, (size_t)(n * groups) * 2872 * 4}};
    for (int i = 0; i < 12; ++i) {
        EXPECT(r[i].off % 16 == 0 && r[i].bytes > 0 && r[i].off + r[i].bytes <= w.total);
        for (int j = i + 1; j < 12; ++j)
            EXPECT(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off);
    }
}

int main() {
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
    std::printf("%d calls, %d failures\n", calls, fails);
    return fails != 0;
}
