// The gradient-tracking round's launch shaping alone (csrc/launch.cpp + plan.cpp, no HIP, no
// library): drives shape_track_round at 256 compute units over a grid of shapes -- agents x
// parameters x layout x row stride x deviation x graph kind x where x' and d' live -- and checks
// every launch list against shape_round's for the same dl_mix_args: the same launches in grid,
// LDS, chunks, fast and TileArgs, every one a kLaunchTrackTile whose tracker and gradient strides
// are x's, every column covered once; then the refusals of plan paths 2, 4 and 5 and of every
// illegal overlap with the header's text.  Built with the address and undefined-behaviour
// sanitizers by test_track_sweep_cpu.py.
#include <iostream>

#include "../distributed-learning_amd/csrc/launch.h"
#include "launch_table.h"

namespace {

using namespace launch_table;

int n_bad = 0;
std::string g_case;
void expect(bool ok, const char *what) {
    if (ok) return;
    if (++n_bad <= 20) std::cerr << what << ": " << g_case << "\n";
}
#define EXPECT(c) expect((c), #c)

constexpr size_t kWsBytes = (size_t)1 << 24;
// dummy address spaces of the tracker, its output and last step's gradient
constexpr int D = BUF, DOUT = N_BASES, Q = N_BASES + 1;

// regular: 5 entries a row, one shared weight sequence, doubly stochastic (the tests' circulant
// graph); else an irregular row-stochastic graph of 3 to 9 entries a row
dl_csr csr(int32_t n, bool regular) {
    dl_csr W{};
    W.row_ptr = at<int32_t>(ROWPTR);
    W.col = at<int32_t>(COL);
    W.w = at<float>(WEIGHTS);
    W.n_rows = n;
    if (regular) {
        W.nnz = 5 * n;
        W.uniform_row_nnz = 5;
        W.doubly_stochastic = 1;
        W.shared_row_weights = 1;
        W.min_row_nnz = 5;
    } else {
        W.nnz = 6 * n;
        W.min_row_nnz = n >= 10 ? 3 : 1;
    }
    return W;
}

// alias bit 0: x' = x, bit 1: d' = d
dl_track_round_args args(int32_t n, int64_t P, bool regular, int32_t tile_cols, int64_t pad,
                         bool dev, int alias) {
    dl_track_round_args q{};
    dl_mix_args &m = q.mix;
    m.W = csr(n, regular);
    m.n_params = P;
    m.tile_cols = tile_cols;
    m.x = at<float>(X);
    m.y = at<float>((alias & 1) ? X : Y);
    m.g = at<float>(G);
    m.lr = 0.125f;
    q.d = at<float>(D);
    q.d_out = at<float>((alias & 2) ? D : DOUT);
    q.g_old = at<float>(Q);
    const int64_t ld = tile_cols > 0 ? 0 : P + pad;
    m.ldx = m.ldy = m.ldg = q.ldd = q.lddo = q.ldq = ld;
    if (dev) {
        m.dev_sq = at<float>(DEV_SQ);
        m.dev_max = at<float>(DEV_MAX);
        m.mean = at<float>(MEAN);
    }
    return q;
}

int n_ok = 0;

// a call that must be shaped: compare with shape_round's launches for the same dl_mix_args
void check_shaped(const dl_track_round_args &q, const dl::Knobs &k) {
    const dl_mix_args &m = q.mix;
    char err[dl::kErrLen] = "", rerr[dl::kErrLen] = "", perr[dl::kErrLen] = "";
    dl::Launches L{}, Lr{};
    dl_mix_plan pub{}, qpub{};
    void *ws = at<void>(WS);
    const int rc = dl::shape_track_round(&q, 256, k, ws, kWsBytes, &pub, &L, err);
    EXPECT(rc == DL_OK);
    if (rc != DL_OK) {
        if (n_bad <= 20) std::cerr << "  " << rc << " " << err << "\n";
        return;
    }
    ++n_ok;
    // the plan query alone answers the same plan: the planner's for the same dl_mix_args
    EXPECT(dl::shape_track_round(&q, 256, k, nullptr, 0, &qpub, nullptr, perr) == DL_OK);
    dl::Plan pl;
    EXPECT(dl::plan_mix(m, 256, k, &pl, perr) == DL_OK && pl.pub.path == 1);
    for (const dl_mix_plan *p : {&pub, &qpub})
        EXPECT(p->path == 1 && p->tile_cols == pl.pub.tile_cols && p->grid == pl.pub.grid &&
               p->lds_bytes == pl.pub.lds_bytes && p->n_tiles == pl.pub.n_tiles);
    // shape_round takes no in-place y: the same round with y elsewhere, y put back to compare
    dl_mix_args mr = m;
    if (m.y == m.x) mr.y = at<float>(Y);
    const int rrc = dl::shape_round(mr, 256, k, ws, kWsBytes, &Lr, rerr);
    EXPECT(rrc == DL_OK && Lr.n == L.n);
    if (rrc != DL_OK || Lr.n != L.n) return;
    EXPECT(L.after == Lr.after && L.partial == Lr.partial && L.parts == Lr.parts &&
           L.rows == Lr.rows && L.max_zeroed == Lr.max_zeroed);
    const bool dev = m.dev_sq != nullptr;
    EXPECT(L.after == (!dev ? dl::kAfterNothing : m.W.n_rows <= 1 ? dl::kAfterZero
                                                                   : dl::kAfterReduce));
    EXPECT(1 <= L.n && L.n <= 2);
    int64_t col_end = 0, ws_end = 0;
    for (int i = 0; i < L.n; ++i) {
        const dl::Launch &l = L.l[i];
        dl::Launch r = Lr.l[i];
        r.t.y = l.t.y;
        EXPECT(l.kind == dl::kLaunchTrackTile && r.kind == dl::kLaunchTile);
        EXPECT(l.grid == r.grid && l.lds == r.lds && l.chunks == r.chunks && l.fast == r.fast &&
               l.dev == r.dev && l.dev == dev && l.sgd && l.mix);
        EXPECT(fmt(l.t) == fmt(r.t));
        const dl::TileArgs &t = l.t;
        // the tracker, its output and both gradients: the call's, laid out as x
        EXPECT(l.k.d == q.d && l.k.ldd == q.ldd && l.k.d_out == q.d_out && l.k.lddo == q.lddo &&
               l.k.q == q.g_old && l.k.ldq == q.ldq && t.g == m.g && t.ldg == m.ldg &&
               t.lr == m.lr);
        EXPECT(l.k.dts == t.xts && l.k.dots == t.xts && l.k.qts == t.xts && t.gts == t.xts);
        EXPECT(l.k.drs == t.xrs && l.k.dors == t.xrs && l.k.qrs == t.xrs && t.grs == t.xrs);
        int64_t ts;
        uint32_t rs;
        dl::tile_stride(t.tiled, q.ldd, t.n_rows, 4 * l.chunks, &ts, &rs);
        EXPECT(l.k.dts == ts && l.k.drs == rs);
        // the float4 kernel only where every row of every operand is 16-byte aligned
        if (l.fast) EXPECT(t.vec && (t.tiled || (m.ldx % 4 == 0 && q.ldd % 4 == 0)));
        EXPECT(1 <= l.grid && l.grid <= t.n_tiles);
        EXPECT(16 <= l.lds && l.lds <= dl::kLdsBytes);
        // every column once
        const int64_t T = 4 * (int64_t)l.chunks;
        EXPECT(t.col_base == col_end);
        col_end += (int64_t)t.n_tiles * T;
        if (i + 1 == L.n) EXPECT(col_end >= t.n_params && col_end - T < t.n_params);
        if (dev && m.W.n_rows > 1) {
            const int64_t off = reinterpret_cast<uintptr_t>(t.dev_partial) -
                                reinterpret_cast<uintptr_t>(ws);
            EXPECT(off == ws_end);
            ws_end = off + (int64_t)l.grid * t.n_rows * 4;
            EXPECT(ws_end <= (int64_t)kWsBytes);
        }
    }
    if (L.after == dl::kAfterReduce) EXPECT((int64_t)L.parts * L.rows * 4 == ws_end);
}

// a call the round refuses: status and text, from the round and from the plan query
void check_refused(const dl_track_round_args &q, const dl::Knobs &k, int status, const char *text,
                   bool plan_too = true) {
    char err[dl::kErrLen] = "", perr[dl::kErrLen] = "";
    dl::Launches L{};
    dl_mix_plan pub{};
    const int rc = dl::shape_track_round(&q, 256, k, at<void>(WS), kWsBytes, nullptr, &L, err);
    EXPECT(rc == status && std::string(err).find(text) != std::string::npos);
    if ((rc != status || std::string(err).find(text) == std::string::npos) && n_bad <= 20)
        std::cerr << "  got " << rc << " " << err << ", want " << status << " ..." << text << "\n";
    if (!plan_too) return;
    const int prc = dl::shape_track_round(&q, 256, k, nullptr, 0, &pub, nullptr, perr);
    EXPECT(prc == rc && std::string(perr) == err);
}

}  // namespace

int main() {
    const dl::Knobs k0;
    const int32_t ns[] = {2, 33, 64, 300, 1024, 1500};
    const int64_t Ps[] = {7, 129, 777, 4096, 4100};
    int n_cases = 0, n_fast = 0, n_guarded = 0;
    for (int32_t n : ns)
        for (int64_t P : Ps)
            for (int tiled = 0; tiled < 2; ++tiled)
                for (int64_t pad : {0, 4})
                    for (int dev = 0; dev < 2; ++dev)
                        for (int regular = 0; regular < 2; ++regular)
                            for (int alias = 0; alias < 4; ++alias) {
                                if (tiled && pad) continue;   // a tiled operand has no row stride
                                int32_t T = 0;
                                if (tiled) {
                                    T = dl::choose_tile_cols(csr(n, regular), 0, P, dev, k0);
                                    if (T <= 0) continue;
                                }
                                g_case = "n=" + std::to_string(n) + " P=" + std::to_string(P) +
                                         " T=" + std::to_string(T) + " pad=" + std::to_string(pad) +
                                         " dev=" + std::to_string(dev) + " regular=" +
                                         std::to_string(regular) + " alias=" + std::to_string(alias);
                                const dl_track_round_args q = args(n, P, regular, T, pad, dev, alias);
                                dl::Plan pl;
                                char err[dl::kErrLen] = "";
                                ++n_cases;
                                if (dl::plan_mix(q.mix, 256, k0, &pl, err) == DL_OK &&
                                    pl.pub.path != 1) {
                                    const std::string want = "path " + std::to_string(pl.pub.path);
                                    check_refused(q, k0, DL_ERR_UNSUPPORTED, want.c_str());
                                    continue;
                                }
                                check_shaped(q, k0);
                                dl::Launches L{};
                                if (dl::shape_track_round(&q, 256, k0, at<void>(WS), kWsBytes,
                                                          nullptr, &L, err) == DL_OK)
                                    for (int i = 0; i < L.n; ++i)
                                        (L.l[i].fast ? n_fast : n_guarded)++;
                            }
    g_case = "grid totals";
    EXPECT(n_ok >= n_cases * 3 / 4);
    EXPECT(n_fast > 0 && n_guarded > 0);

    // d, d_out or g_old off 16 bytes, or a row stride of theirs that is no multiple of 4: the
    // guarded kernel alone (row-major), a refusal in the column-tiled layout
    for (int which = 0; which < 3; ++which) {
        g_case = "operand " + std::to_string(which) + " misaligned";
        auto put = [&](dl_track_round_args &q, int64_t off) {
            if (which == 0) q.d = at<float>(D, off);
            if (which == 1) q.d_out = at<float>(DOUT, off);
            if (which == 2) q.g_old = at<float>(Q, off);
        };
        dl_track_round_args q = args(64, 4096, true, 0, 0, false, 0);
        put(q, 4);
        dl::Launches L{};
        char err[dl::kErrLen] = "";
        EXPECT(dl::shape_track_round(&q, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err) == DL_OK);
        for (int i = 0; i < L.n; ++i) EXPECT(!L.l[i].fast && !L.l[i].t.vec);
        q = args(64, 4096, true, 0, 0, false, 0);
        (which == 0 ? q.ldd : which == 1 ? q.lddo : q.ldq) = 4098;
        EXPECT(dl::shape_track_round(&q, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err) == DL_OK);
        for (int i = 0; i < L.n; ++i) {
            const dl::TrackTileArgs &t = L.l[i].k;
            EXPECT(!L.l[i].fast && (which == 0 ? t.drs : which == 1 ? t.dors : t.qrs) == 4098 * 4);
        }
        q = args(64, 4096, true, 64, 0, false, 0);
        put(q, 4);
        check_refused(q, k0, DL_ERR_INVALID, "tiled operands must be 16-byte aligned", false);
    }

    // every illegal overlap, row-major and column-tiled: an output on another operand, or partly
    // on the one it may be
    for (int32_t T : {0, 64}) {
        const int64_t bytes = 64 * 4096 * 4;
        auto base = [&]() { return args(64, 4096, true, T, 0, false, 0); };
        auto refused = [&](const char *name, dl_track_round_args q, const char *text) {
            g_case = std::string(name) + (T ? " (tiled)" : "");
            check_refused(q, k0, DL_ERR_INVALID, text);
        };
        dl_track_round_args q = base();
        q.d_out = at<float>(X);
        refused("d_out = x", q, "dl_track_round: d_out overlaps x");
        q = base();
        q.d_out = at<float>(Y, bytes - 256);
        refused("d_out into y", q, "dl_track_round: d_out overlaps y");
        q = base();
        q.d_out = at<float>(G);
        refused("d_out = g", q, "dl_track_round: d_out overlaps g");
        q = base();
        q.d_out = at<float>(Q, 256);
        refused("d_out into g_old", q, "dl_track_round: d_out overlaps g_old");
        q = base();
        q.d_out = at<float>(D, 256);
        refused("d_out partly on d", q, "dl_track_round: d_out overlaps d (d_out may be d itself");
        if (!T) {
            q = base();
            q.d_out = at<float>(D);
            q.lddo = 4100;
            refused("d_out = d, another stride", q, "dl_track_round: d_out overlaps d");
        }
        q = base();
        q.mix.y = at<float>(D);
        refused("y = d", q, "dl_track_round: y overlaps d");
        q = base();
        q.mix.y = at<float>(Q, bytes - 256);
        refused("y into g_old", q, "dl_track_round: y overlaps g_old");
        q = base();
        q.mix.y = at<float>(G);
        refused("y = g", q, "dl_mix_round: y overlaps g");
        q = base();
        q.mix.y = at<float>(X, 256);
        refused("y partly on x", q, "dl_mix_round: y overlaps x");
        q = base();
        q.mix.y = at<float>(X);
        q.d_out = at<float>(X);
        refused("y = d_out = x", q, "dl_track_round: d_out overlaps x");
    }

    // plan paths 2, 4 and 5 are refused with the header's text: forced by the knobs, and where
    // the planner chooses them (4096 agents with per-edge weights, an irregular graph of 3000)
    bool seen[6] = {};
    auto refused_path = [&](const char *name, dl_track_round_args q, const dl::Knobs &k) {
        g_case = name;
        dl::Plan pl;
        char err[dl::kErrLen] = "";
        EXPECT(dl::plan_mix(q.mix, 256, k, &pl, err) == DL_OK);
        EXPECT(pl.pub.path == 2 || pl.pub.path == 4 || pl.pub.path == 5);
        if (pl.pub.path < 0 || pl.pub.path > 5) return;
        seen[pl.pub.path] = true;
        const std::string want = "dl_track_round: the fused gradient-tracking round runs on the "
                                 "LDS tile kernel (plan path 1); this round plans path " +
                                 std::to_string(pl.pub.path);
        check_refused(q, k, DL_ERR_UNSUPPORTED, want.c_str());
    };
    dl::Knobs kg, kr;
    kg.force_gather = true;
    kr.force_reg = true;
    for (int dev = 0; dev < 2; ++dev) {
        refused_path("forced gather", args(64, 4096, true, 0, 0, dev, 3), kg);
        refused_path("forced gather, irregular", args(300, 777, false, 0, 4, dev, 0), kg);
        refused_path("forced reg, tiled regular", args(1500, 64, true, 4, 0, dev, 2), kr);
        refused_path("forced reg, tiled irregular", args(1500, 64, false, 4, 0, dev, 1), kr);
        dl_track_round_args big = args(4096, 1 << 16, true, 0, 0, dev, 0);
        big.mix.W.shared_row_weights = 0;
        refused_path("4096 agents, per-edge weights", big, k0);
        dl_track_round_args irr = args(3000, 1 << 16, false, 0, 0, dev, 0);
        irr.mix.W.nnz = 9000;
        irr.mix.W.doubly_stochastic = 1;
        irr.mix.W.min_row_nnz = 3;
        refused_path("3000 agents, irregular", irr, k0);
    }
    g_case = "paths seen";
    EXPECT(seen[2] && seen[4] && seen[5]);

    std::cout << n_cases << " cases, " << n_ok << " shaped, " << n_bad << " failures\n";
    return n_bad ? 1 : 0;
}
