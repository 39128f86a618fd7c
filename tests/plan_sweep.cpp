// The mix planner alone (csrc/plan.cpp, no HIP, no library): replays tests/golden/mix_plans.txt
// (format: test_plan_table_cpu.py) through the pure planner at 256 compute units, compares every
// answer with the line, and checks the plan fields the C ABI does not show.  Built with the
// address and undefined-behaviour sanitizers by test_plan_sweep_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../distributed-learning_amd/csrc/plan.h"

namespace {

int n_bad = 0;
const std::string *g_line;
void expect(bool ok, const char *what) {
    if (ok) return;
    if (++n_bad <= 20) std::cerr << what << ": " << *g_line << "\n";
}
#define EXPECT(c) expect((c), #c)

dl::Knobs parse_knob(const std::string &s) {
    dl::Knobs k;
    if (s == "-") return k;
    const std::string name = s.substr(0, s.find('='));
    const int v = atoi(s.c_str() + s.find('=') + 1);
    if (name == "DLAMD_GRID_MULT") k.grid_mult = v, k.grid_mult_set = true;
    else if (name == "DLAMD_WG_PER_CU") k.wg_per_cu = v;
    else if (name == "DLAMD_BALANCE_GRID") k.balance_grid = v != 0;
    else if (name == "DLAMD_FORCE_REG") k.force_reg = v != 0;
    else if (name == "DLAMD_FORCE_GATHER") k.force_gather = v != 0;
    else if (name == "DLAMD_MAX_TILE_CHUNKS") k.max_tile_chunks = v;
    else if (name == "DLAMD_TILE_GROUP") k.tile_group = v;
    else if (name == "DLAMD_TRACE_PLANES") k.trace_planes = true;
    else expect(false, "unknown knob");
    return k;
}

// the fields behind dl_mix_plan: LDS offsets, grid and tile cover, the kernels' row-pass limit
void check_hidden(const dl_mix_args &a, const dl::Plan &pl, int images) {
    const dl_mix_plan &p = pl.pub;
    if (p.path == 2) return;   // the gather kernel: no tile, no LDS
    const int64_t R = dl::local_src(a) + a.n_halo;
    const int64_t tile = R * pl.chunks * 16;
    const int grp = pl.grp > 1 ? pl.grp : 1;
    EXPECT(pl.csr_off % 16 == 0 && pl.scratch_off % 16 == 0 && p.lds_bytes % 16 == 0);
    EXPECT(p.lds_bytes <= dl::kLdsBytes);
    EXPECT(1 <= p.grid && p.grid <= p.n_tiles);
    EXPECT(pl.chunks == p.tile_cols / 4 * grp);
    EXPECT((int64_t)p.n_tiles * p.tile_cols * grp >= a.n_params);
    EXPECT((int64_t)(p.n_tiles - 1) * p.tile_cols * grp < a.n_params);
    EXPECT(R * pl.chunks <= (a.n_halo > 0 && a.tile_cols > 0 ? 4 : dl::kRowsPerThread) *
                                dl::kTileThreads);
    const int64_t scratch = pl.dev ? 16 * pl.chunks * 16 : 0;
    if (p.path == 4 || p.path == 5) {   // tile, scratch, then path 5's tail
        EXPECT(pl.scratch_off == tile && pl.csr_off == tile + scratch);
        EXPECT(p.path == 5 ? p.lds_bytes >= (int64_t)pl.csr_off
                           : p.lds_bytes == (int64_t)pl.csr_off);
        return;
    }
    const dl::CsrShape S = dl::csr_shape(a.W);
    EXPECT(pl.csr_off == tile * images);
    EXPECT(pl.scratch_off == pl.csr_off + S.lds ||
           (images == 2 && S.in_regs && pl.scratch_off == pl.csr_off));   // CSR in registers
    EXPECT(p.lds_bytes == pl.scratch_off + scratch);
}

}  // namespace

int main(int argc, char **argv) {
    std::ifstream in(argc > 1 ? argv[1] : "tests/golden/mix_plans.txt");
    std::string line;
    int n = 0;
    float f;   // operands are never read: any non-null address does
    for (; std::getline(in, line); ++n) {
        g_line = &line;
        std::istringstream s(line);
        std::string name, entry, knob, arrow, want;
        dl_mix_args a{};
        int dev, lag;
        s >> name >> entry >> a.W.n_rows >> a.W.nnz >> a.W.uniform_row_nnz >>
            a.W.doubly_stochastic >> a.W.shared_row_weights >> a.W.min_row_nnz >> a.n_params >>
            a.tile_cols >> a.n_halo >> a.n_local_src >> dev >> lag >> knob >> arrow;
        std::getline(s >> std::ws, want);
        EXPECT(s && arrow == "->");
        const dl::Knobs k = parse_knob(knob);
        if (dev) a.dev_sq = a.dev_max = &f;
        if (lag) a.mean_prev = a.colsum_out = &f;
        char err[dl::kErrLen] = "";
        char got[dl::kErrLen + 16];
        int rc;
        if (entry == "trace") {
            dl::TracePlan tp;
            rc = dl::plan_trace(a, 256, k, &tp, err);
            snprintf(got, sizeof got, "0 %d", tp.max_rounds);
            if (rc == 0) {
                EXPECT(tp.n_steps * tp.chunks * (tp.narrow ? 2 : 4) == a.n_params);
                EXPECT(tp.lds <= (uint32_t)dl::kLdsBytes && tp.scratch_off % 16 == 0 &&
                       tp.csr_off % 16 == 0 && tp.csr_off <= tp.scratch_off);
                EXPECT(1 <= tp.grid && tp.grid <= tp.n_steps);
            }
        } else {
            dl::Plan pl;
            if (entry == "csr") {   // dl_mix_plan_csr: shapes only, the width chosen
                if (!a.W.uniform_row_nnz) a.W.shared_row_weights = 0;
                a.tile_cols = dl::choose_tile_cols(a.W, a.n_halo, a.n_params, dev != 0, k);
            }
            rc = entry == "rounds" ? dl::plan_rounds(a, 256, k, &pl, err)
                                   : dl::plan_mix(a, 256, k, &pl, err);
            const dl_mix_plan &p = pl.pub;
            snprintf(got, sizeof got, "0 %d %d %d %d %d %d %d %d", p.path, p.tile_cols, p.grid,
                     p.lds_bytes, p.n_tiles, p.regular, p.head, p.tail_fmt);
            if (rc == 0) check_hidden(a, pl, entry == "rounds" ? 2 : 1);
        }
        if (rc) snprintf(got, sizeof got, "%d %s", rc, err);
        if (want != got) {
            if (++n_bad <= 20) std::cerr << "got " << got << ": " << line << "\n";
        }
    }
    std::cout << n << " plans, " << n_bad << " failures\n";
    return n_bad || n < 1500 ? 1 : 0;
}
