// shape_lenet_eval alone (csrc/launch.cpp + plan.cpp, no HIP, no library), built with the address
// and undefined-behaviour sanitizers and run as an ordinary process
// (tests/test_lenet_eval_abi.py).  Over n_agents x rows x compute units x row_splits hints it
// checks what must hold of any shaped call: every block of every agent is walked exactly once
// by the agent's workgroups, the grid is n_agents * row_splits and never exceeds n_agents *
// blocks, and part and hit are disjoint, large enough and inside
// dl_lenet_eval_workspace_bytes.  Then the refusals that need a plausible workspace, and
// touching operands.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "launch.h"

static int fails = 0, calls = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static dl_lenet_eval_args base(int32_t n, int32_t rows, int32_t nc) {
    dl_lenet_eval_args a;
    std::memset(&a, 0, sizeof a);
    const int64_t P = dl::lenet_param_count(nc), ld = (P + 63) / 64 * 64;
    a.n_agents = n; a.rows = rows; a.num_classes = nc;
    a.X = (const float *)(1ull << 40); a.ldx = ld;
    a.data = (const float *)(1ull << 44); a.s_data = 0;
    a.labels = (const int32_t *)(1ull << 50); a.s_labels = 0;
    a.loss = (float *)(1ull << 52);
    a.correct = (int32_t *)(1ull << 53);
    return a;
}
static void *const WS = (void *)(1ull << 54);

// the kernel's walk: workgroup (agent, split) takes blocks split, split + row_splits, ...
static bool walked_once(int32_t blocks, int32_t splits) {
    if (splits < 1 || splits > blocks) return false;
    std::vector<int> seen((size_t)blocks, 0);
    for (int32_t s = 0; s < splits; ++s)
        for (int32_t b = s; b < blocks; b += splits) ++seen[(size_t)b];
    return std::all_of(seen.begin(), seen.end(), [](int v) { return v == 1; });
}

int main() {
    char err[dl::kErrLen];
    const int32_t agents[] = {1, 2, 3, 63, 64, 257, 600, 65535};
    const int32_t rows[] = {1, 63, 64, 65, 129, 130, 1000, 10000, 1 << 20};
    const int cus[] = {0, 1, 8, 256, 304};
    const int32_t hints[] = {0, 1, 2, 3, 7, 64, 1 << 20};
    for (int32_t n : agents)
        for (int32_t r : rows)
            for (int cu : cus)
                for (int32_t hint : hints) {
                    dl_lenet_eval_args a = base(n, r, 10);
                    a.row_splits = hint;
                    const dl::LenetEvalWs w = dl::lenet_eval_workspace(n, r);
                    const int64_t blocks = ((int64_t)r + 63) / 64;
                    dl_lenet_eval_plan p;
                    ++calls;
                    EXPECT(dl::shape_lenet_eval(&a, cu, WS, w.total, true, &p, err) == DL_OK);
                    EXPECT(p.blocks == blocks && p.lds_bytes == dl::kLenetEvalLdsBytes);
                    EXPECT(p.lds_bytes * dl::kLenetEvalWgPerCu <= 160 * 1024);
                    EXPECT(walked_once(p.blocks, p.row_splits));
                    EXPECT((int64_t)p.grid == (int64_t)n * p.row_splits && p.grid > 0);
                    EXPECT((int64_t)p.grid <= (int64_t)n * blocks);
                    if (hint > 0) {
                        EXPECT(p.row_splits == std::min<int64_t>(hint, blocks));
                    } else {   // enough workgroups for the compute units where the work allows it
                        const int64_t want =
                            ((int64_t)dl::kLenetEvalWgPerCu * std::max(cu, 1) + n - 1) / n;
                        EXPECT(p.row_splits == std::min(want, blocks));
                    }
                    // part [n][blocks] floats, hit [n][blocks] int32: aligned, disjoint, inside
                    const size_t cells = (size_t)n * (size_t)blocks * 4;
                    EXPECT(w.part % 16 == 0 && w.hit % 16 == 0);
                    EXPECT(w.part + cells <= w.hit && w.hit + cells <= w.total);
                    EXPECT(w.total == dl::lenet_eval_workspace(n, r).total && w.total > 0);
                    // the same plan without a workspace (the plan query)
                    dl_lenet_eval_plan q;
                    EXPECT(dl::shape_lenet_eval(&a, cu, nullptr, 0, false, &q, err) == DL_OK);
                    EXPECT(std::memcmp(&p, &q, sizeof p) == 0);
                    // one byte short, a null and a misaligned workspace
                    EXPECT(dl::shape_lenet_eval(&a, cu, WS, w.total - 1, true, &p, err) ==
                           DL_ERR_WORKSPACE);
                    EXPECT(dl::shape_lenet_eval(&a, cu, nullptr, w.total, true, &p, err) ==
                           DL_ERR_WORKSPACE);
                    EXPECT(dl::shape_lenet_eval(&a, cu, (char *)WS + 8, w.total + 8, true, &p,
                                                err) == DL_ERR_WORKSPACE);
                }
    // the class range and per-agent operands; the workspace does not follow num_classes
    for (int32_t nc : {1, 3, 64}) {
        dl_lenet_eval_args a = base(3, 150, nc);
        a.s_data = 150 * 3072; a.s_labels = 150;
        a.logits = (float *)(1ull << 55); a.ldz = 64; a.s_logits = 150 * 64;
        dl_lenet_eval_plan p;
        const size_t need = dl::lenet_eval_workspace(3, 150).total;
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_OK);
        EXPECT(p.blocks == 3 && p.row_splits == 3 && p.grid == 9);
    }
    {
        // touching operands do not overlap; one element further they do
        dl_lenet_eval_args a = base(2, 130, 10);
        dl_lenet_eval_plan p;
        const size_t need = dl::lenet_eval_workspace(2, 130).total;
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, nullptr, err) == DL_OK);
        a.correct = (int32_t *)((char *)a.loss + 8);
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_OK);
        a.correct = (int32_t *)((char *)a.loss + 4);
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_ERR_INVALID &&
               std::strstr(err, "loss overlaps correct"));
        a = base(2, 130, 10);
        const size_t db = (size_t)130 * 3072 * 4, lb = (size_t)130 * 4;   // shared: one agent's
        a.loss = (float *)((char *)a.data + db);
        a.correct = (int32_t *)((char *)a.labels + lb);
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_OK);
        a.loss = (float *)((char *)a.data + db - 4);
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_ERR_INVALID &&
               std::strstr(err, "loss overlaps data"));
        a = base(2, 130, 10);
        EXPECT(dl::shape_lenet_eval(&a, 256, (char *)a.X - need, need, true, &p, err) == DL_OK);
        EXPECT(dl::shape_lenet_eval(&a, 256, (char *)a.X - need + 16, need, true, &p, err) ==
                   DL_ERR_INVALID && std::strstr(err, "workspace overlaps X"));
        EXPECT(dl::shape_lenet_eval(&a, 256, (char *)a.loss + 16, need, true, &p, err) == DL_OK);
        EXPECT(dl::shape_lenet_eval(&a, 256, (char *)a.loss, need, true, &p, err) ==
                   DL_ERR_INVALID && std::strstr(err, "loss overlaps workspace"));
    }
    {
        // only a hint can ask for 2^31 workgroups: refused, not wrapped
        dl_lenet_eval_args a = base(65535, 1 << 30, 10);
        a.row_splits = 1 << 20;
        dl_lenet_eval_plan p;
        const size_t need = dl::lenet_eval_workspace(65535, 1 << 30).total;
        EXPECT(need > ((size_t)1 << 32));
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_ERR_INVALID &&
               std::strstr(err, "grid too large"));
        a.row_splits = 0;
        EXPECT(dl::shape_lenet_eval(&a, 256, WS, need, true, &p, err) == DL_OK &&
               p.blocks == (1 << 24) && p.row_splits == 1 && p.grid == 65535);
    }
    std::printf("%d calls, %d failures\n", calls, fails);
    return fails != 0;
}
