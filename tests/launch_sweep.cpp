// The launch shaping alone (csrc/launch.cpp + plan.cpp, no HIP, no library): replays
// tests/golden/mix_launches.txt (format: test_launch_sweep_cpu.py) through the pure functions at
// 256 compute units, compares every launch, follow-up and refusal with the line, and checks what
// must hold of any launch list; a momentum round's plan query (shape_sgd_round without a launch
// list) must refuse what the round refuses.  Built with the address and undefined-behaviour sanitizers by
// test_launch_sweep_cpu.py.
#include <fstream>
#include <iostream>

#include "../distributed-learning_amd/csrc/launch.h"
#include "launch_table.h"

namespace {

using namespace launch_table;

int n_bad = 0;
const std::string *g_line;
void expect(bool ok, const char *what) {
    if (ok) return;
    if (++n_bad <= 20) std::cerr << what << ": " << *g_line << "\n";
}
#define EXPECT(c) expect((c), #c)

// the environment variable of a line's knob field (`-` or NAME=value) as Knobs fields
dl::Knobs parse_knob(const std::string &s) {
    dl::Knobs k;
    if (s == "-") return k;
    const std::string name = s.substr(0, s.find('=')), val = s.substr(s.find('=') + 1);
    const char c = val[0];
    const int v = atoi(val.c_str());
    if (name == "DLAMD_NT_STORE") k.nt_store = c == '0' ? 0 : 1;
    else if (name == "DLAMD_NT_LOAD") k.nt_load = c == '0' ? 0 : c == 'x' ? 1 : c == 'g' ? 2 : 3;
    else if (name == "DLAMD_LDS_MIN") k.lds_min = v;
    else if (name == "DLAMD_TILE_RUN") k.tile_run = c == '1' ? 1 : 0;
    else if (name == "DLAMD_GATHER_ORDER") k.gather_order_columns = c == 'c';
    else if (name == "DLAMD_FORCE_REG") k.force_reg = v != 0;
    else if (name == "DLAMD_FORCE_GATHER") k.force_gather = v != 0;
    else if (name == "DLAMD_GRID_MULT") k.grid_mult = v, k.grid_mult_set = true;
    else if (name == "DLAMD_TILE_GROUP") k.tile_group = v;
    else if (name == "DLAMD_MAX_TILE_CHUNKS") k.max_tile_chunks = v;
    else if (name == "DLAMD_WG_PER_CU") k.wg_per_cu = v;
    else if (name == "DLAMD_BALANCE_GRID") k.balance_grid = v != 0;
    else if (name == "DLAMD_TRACE_PLANES") k.trace_planes = true;
    else expect(false, "unknown knob");
    return k;
}

std::string fmt(const dl::Launch &l) {
    switch (l.kind) {
        case dl::kLaunchTile:
            return fmt_launch("tile", {l.chunks, l.sgd, l.dev, l.mix, l.fast, l.grid, l.lds}, l.t);
        case dl::kLaunchSgdTile:
            return fmt_sgd_launch(l.chunks, l.dev, l.fast, l.grid, l.lds, l.t, l.q);
        case dl::kLaunchTileReg:
            return fmt_launch("reg", {l.chunks, l.head, l.tail_fmt, l.sgd, l.dev, l.grid, l.lds},
                              l.t);
        case dl::kLaunchGather: return fmt_launch("gather", {l.sgd, l.columns}, l.t);
        case dl::kLaunchMulti:
            return fmt_launch("multi", {l.chunks, l.rounds, l.sgd, l.dev, l.grid, l.lds}, l.t);
        case dl::kLaunchTrace:
            return fmt_launch("trace", {l.chunks, l.planes, l.rounds, l.grid, l.lds}, l.t);
        default:
            return fmt_launch("irr", {l.head, l.gm, l.narrow, l.rounds, l.grid, l.lds}, l.t);
    }
}

std::string fmt(const dl::Launches &L, bool traced) {
    std::string s = "0 ";
    for (int i = 0; i < L.n; ++i) s += fmt(L.l[i]);
    switch (L.after) {
        case dl::kAfterZero: return s + "; zero";
        case dl::kAfterReduce:
            return s + "; reduce " + ptr(L.partial, WS) + " " + std::to_string(L.parts) + " " +
                   std::to_string(L.rows) + " " + std::to_string(L.max_zeroed);
        case dl::kAfterPartialRows: return s + "; partial_rows " + std::to_string(L.parts);
        case dl::kAfterTwoPass: return s + "; two_pass";
        default: return s + (traced ? "; trace_reduce" : "; none");
    }
}

// what holds of every launch list: partial rows disjoint and inside the workspace, no idle
// workgroup, every column covered exactly once, the hub rows' heads inside LDS
void check_launches(const Case &c, const dl::Launches &L) {
    EXPECT(1 <= L.n && L.n <= 2);
    int64_t ws_end = 0, col_end = 0, parts = 0;
    for (int i = 0; i < L.n; ++i) {
        const dl::Launch &l = L.l[i];
        const dl::TileArgs &t = l.t;
        for (int b = t.n_hblk + 1; b < 17; ++b) EXPECT(t.hblk_row0[b] == 0);
        for (int b = t.n_hblk; b < 16; ++b) EXPECT(t.hblk_off[b] == 0);
        if (l.kind == dl::kLaunchGather) {
            EXPECT(L.n == 1 && !t.dev_partial);
            return;
        }
        EXPECT(1 <= l.grid && l.grid <= t.n_tiles);
        EXPECT(16 <= l.lds && l.lds <= dl::kLdsBytes);
        EXPECT(t.n_hub == 0 ||
               (t.hub_off % 16 == 0 && (int64_t)t.hub_off + (int64_t)t.n_hub * l.head * 8 == l.lds));
        const bool traced = l.kind == dl::kLaunchTrace || l.kind == dl::kLaunchTraceIrr;
        // columns of a kernel tile: a traced step walks chunks of 4 (narrow: 2) columns
        const int64_t T = traced ? (int64_t)l.chunks * (l.narrow ? 2 : 4) : 4 * (int64_t)l.chunks;
        EXPECT(t.col_base == col_end);
        col_end += (int64_t)t.n_tiles * T;
        if (i + 1 == L.n) EXPECT(col_end >= t.n_params && col_end - T < t.n_params);
        if (t.dev_partial) {
            const int64_t rows = dl::tile_lag(t) ? t.n_loc : t.n_rows;
            const int64_t off = reinterpret_cast<uintptr_t>(t.dev_partial) -
                                reinterpret_cast<uintptr_t>(c.ws);
            EXPECT(off == ws_end);
            ws_end = off + (int64_t)l.grid * (traced ? l.rounds : 1) * rows * 4;
            EXPECT(ws_end <= (int64_t)c.ws_bytes);
            parts += l.grid;
        } else {
            EXPECT(L.after != dl::kAfterReduce && L.after != dl::kAfterPartialRows);
        }
    }
    if (L.after == dl::kAfterReduce)
        EXPECT(L.partial == c.ws && L.parts == parts && (int64_t)L.parts * L.rows * 4 == ws_end);
    if (L.after == dl::kAfterPartialRows) EXPECT(L.parts == parts && c.a.partial_rows_out);
}

}  // namespace

int main(int argc, char **argv) {
    std::ifstream in(argc > 1 ? argv[1] : "tests/golden/mix_launches.txt");
    const int floor = 792;   // the lines of the committed table
    std::string line;
    int n = 0;
    for (; std::getline(in, line); ++n) {
        g_line = &line;
        Case c;
        parse(line, &c);
        EXPECT(c.ok);
        const dl::Knobs k = parse_knob(c.knob);
        const dl_mix_args &a = c.a;
        char err[dl::kErrLen] = "";
        dl::Launches L{};
        int rc;
        if (c.entry == "dev" || c.entry == "devtiled") {
            rc = dl::shape_deviation(a.x, a.ldx, a.tile_cols, a.W.n_rows, a.n_params, a.mean, 256,
                                     c.ws, c.ws_bytes, &L, err);
            // no one-pass kernel: dl_deviation runs the two passes, dl_deviation_tiled refuses
            if (rc == DL_ERR_UNSUPPORTED && !*err) {
                if (c.entry == "dev") rc = DL_OK, L.after = dl::kAfterTwoPass;
                else snprintf(err, sizeof err, "dl_deviation_tiled: %d rows exceed one tile",
                              a.W.n_rows);
            }
        } else if (c.entry == "sgdround") {
            const dl_sgd_round_args q = c.sgd();
            rc = dl::shape_sgd_round(c.null_args ? nullptr : &q, 256, k, c.ws, c.ws_bytes, nullptr,
                                     &L, err);
            // the plan query: the same refusal, or the plan of a call that is shaped (and of one
            // that only the workspace or the launch list stops)
            char perr[dl::kErrLen] = "";
            dl_mix_plan pub{};
            const int prc = dl::shape_sgd_round(c.null_args ? nullptr : &q, 256, k, nullptr, 0, &pub,
                                                nullptr, perr);
            if (rc == 0) {
                EXPECT(prc == 0 && pub.path == 1);
                for (int i = 0; i < L.n; ++i) {
                    const dl::Launch &l = L.l[i];
                    EXPECT(l.kind == dl::kLaunchSgdTile && l.sgd && l.mix);
                    EXPECT(l.q.p.lr == a.lr && (l.q.buf != nullptr) == (q.momentum != 0.f));
                }
            } else if (prc) {
                EXPECT(prc == rc && std::string(perr) == err);
            } else {
                EXPECT(rc == DL_ERR_WORKSPACE || std::string(err).find("tiled operands") !=
                                                     std::string::npos);
            }
        } else {
            rc = dl::check_mix_args(c.null_args ? nullptr : &a, err);
            if (rc) {}
            else if (c.entry == "round") rc = dl::shape_round(a, 256, k, c.ws, c.ws_bytes, &L, err);
            else if (c.entry == "rounds")
                rc = dl::shape_rounds(a, c.rounds, 256, k, c.ws, c.ws_bytes, &L, err);
            else if (c.entry == "trace")
                rc = dl::shape_trace(a, c.rounds, 256, k, c.ws, c.ws_bytes, &L, err);
            else expect(false, "unknown entry");
        }
        if (rc == 0 && L.n) check_launches(c, L);
        const std::string got = rc ? std::to_string(rc) + " " + err : fmt(L, c.entry == "trace");
        if (c.want != got && ++n_bad <= 20) std::cerr << "got " << got << ": " << line << "\n";
    }
    std::cout << n << " calls, " << n_bad << " failures\n";
    return n_bad || n < floor ? 1 : 0;
}
