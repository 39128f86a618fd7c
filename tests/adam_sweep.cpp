// The Adam round's launch shaping alone (csrc/launch.cpp + plan.cpp, no HIP, no library): drives
// shape_adam_round at 256 compute units over a grid of shapes -- agents x parameters x layout x
// row stride x deviation x graph kind x where x' lives x where the coefficients come from -- and
// checks every launch list against shape_round's for the same dl_mix_args: the same launches in
// grid, LDS, chunks, fast and TileArgs, every one a kLaunchAdamTile whose moment strides are x's
// and whose AdamParams are the call's, every column covered once; then the refusals of plan paths
// 2, 4 and 5, of every illegal overlap and of every bad parameter with the header's text.  Built
// with the address and undefined-behaviour sanitizers by test_adam_sweep_cpu.py.
#include <cmath>
#include <iostream>
#include <limits>

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
// dummy address spaces of the two moments and the device coefficients
constexpr int M = BUF, V = N_BASES, COEF = N_BASES + 1;

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

// mode bit 0: x' = x, bit 1: the coefficients from the device; the option set cycles with `opt`
// (0 plain, 1 L2 weight decay, 2 decoupled)
dl_adam_round_args args(int32_t n, int64_t P, bool regular, int32_t tile_cols, int64_t pad,
                        bool dev, int mode, int opt = 0) {
    dl_adam_round_args q{};
    dl_mix_args &m = q.mix;
    m.W = csr(n, regular);
    m.n_params = P;
    m.tile_cols = tile_cols;
    m.x = at<float>(X);
    m.y = at<float>((mode & 1) ? X : Y);
    m.g = at<float>(G);
    m.lr = 0.125f;
    q.m = at<float>(M);
    q.v = at<float>(V);
    const int64_t ld = tile_cols > 0 ? 0 : P + pad;
    m.ldx = m.ldy = m.ldg = q.ldm = q.ldv = ld;
    q.beta1 = 0.9;
    q.beta2 = 0.999;
    q.eps = 1e-8f;
    q.weight_decay = opt == 1 ? 5e-4f : opt == 2 ? 1e-2f : 0.f;
    q.decoupled = opt == 2;
    if (mode & 2) {
        q.coef = at<float>(COEF);
        // ignored with coef: anything goes
        q.step_size = std::numeric_limits<float>::quiet_NaN();
    } else {
        q.step_size = 0.01f;
        q.bias2_sqrt = 0.0316f;
    }
    if (dev) {
        m.dev_sq = at<float>(DEV_SQ);
        m.dev_max = at<float>(DEV_MAX);
        m.mean = at<float>(MEAN);
    }
    return q;
}

int n_ok = 0;

// a call that must be shaped: compare with shape_round's launches for the same dl_mix_args
void check_shaped(const dl_adam_round_args &q, const dl::Knobs &k) {
    const dl_mix_args &m = q.mix;
    char err[dl::kErrLen] = "", rerr[dl::kErrLen] = "", perr[dl::kErrLen] = "";
    dl::Launches L{}, Lr{};
    dl_mix_plan pub{}, qpub{};
    void *ws = at<void>(WS);
    const int rc = dl::shape_adam_round(&q, 256, k, ws, kWsBytes, &pub, &L, err);
    EXPECT(rc == DL_OK);
    if (rc != DL_OK) {
        if (n_bad <= 20) std::cerr << "  " << rc << " " << err << "\n";
        return;
    }
    ++n_ok;
    // the plan query alone answers the same plan: the planner's for the same dl_mix_args
    EXPECT(dl::shape_adam_round(&q, 256, k, nullptr, 0, &qpub, nullptr, perr) == DL_OK);
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
        EXPECT(l.kind == dl::kLaunchAdamTile && r.kind == dl::kLaunchTile);
        EXPECT(l.grid == r.grid && l.lds == r.lds && l.chunks == r.chunks && l.fast == r.fast &&
               l.dev == r.dev && l.dev == dev && l.sgd && l.mix);
        EXPECT(fmt(l.t) == fmt(r.t));
        const dl::TileArgs &t = l.t;
        // the moments and the gradient: the call's, laid out as x
        EXPECT(l.a.m == q.m && l.a.ldm == q.ldm && l.a.v == q.v && l.a.ldv == q.ldv &&
               t.g == m.g && t.ldg == m.ldg);
        EXPECT(l.a.mts == t.xts && l.a.vts == t.xts && t.gts == t.xts);
        EXPECT(l.a.mrs == t.xrs && l.a.vrs == t.xrs && t.grs == t.xrs);
        int64_t ts;
        uint32_t rs;
        dl::tile_stride(t.tiled, q.ldm, t.n_rows, 4 * l.chunks, &ts, &rs);
        EXPECT(l.a.mts == ts && l.a.mrs == rs);
        // the optimizer's constants: formed in fp64 from the call's
        const dl::AdamParams &p = l.a.p;
        EXPECT(p.b2 == (float)q.beta2 && p.omb1 == (float)(1.0 - q.beta1) &&
               p.omb2 == (float)(1.0 - q.beta2) && p.eps == q.eps && p.wd == q.weight_decay &&
               p.decay == (float)(1.0 - (double)m.lr * (double)q.weight_decay) &&
               p.decoupled == (q.decoupled ? 1 : 0) && p.coef == q.coef);
        if (!q.coef) EXPECT(p.ss == q.step_size && p.bs == q.bias2_sqrt);
        // the float4 kernel only where every row of every operand is 16-byte aligned
        if (l.fast) EXPECT(t.vec && (t.tiled || (m.ldx % 4 == 0 && q.ldm % 4 == 0)));
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
void check_refused(const dl_adam_round_args &q, const dl::Knobs &k, int status, const char *text,
                   bool plan_too = true) {
    char err[dl::kErrLen] = "", perr[dl::kErrLen] = "";
    dl::Launches L{};
    dl_mix_plan pub{};
    const int rc = dl::shape_adam_round(&q, 256, k, at<void>(WS), kWsBytes, nullptr, &L, err);
    EXPECT(rc == status && std::string(err).find(text) != std::string::npos);
    if ((rc != status || std::string(err).find(text) == std::string::npos) && n_bad <= 20)
        std::cerr << "  got " << rc << " " << err << ", want " << status << " ..." << text << "\n";
    if (!plan_too) return;
    const int prc = dl::shape_adam_round(&q, 256, k, nullptr, 0, &pub, nullptr, perr);
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
                            for (int mode = 0; mode < 4; ++mode) {
                                if (tiled && pad) continue;   // a tiled operand has no row stride
                                int32_t T = 0;
                                if (tiled) {
                                    T = dl::choose_tile_cols(csr(n, regular), 0, P, dev, k0);
                                    if (T <= 0) continue;
                                }
                                const int opt = n_cases % 3;
                                g_case = "n=" + std::to_string(n) + " P=" + std::to_string(P) +
                                         " T=" + std::to_string(T) + " pad=" + std::to_string(pad) +
                                         " dev=" + std::to_string(dev) + " regular=" +
                                         std::to_string(regular) + " mode=" + std::to_string(mode) +
                                         " opt=" + std::to_string(opt);
                                const dl_adam_round_args q =
                                    args(n, P, regular, T, pad, dev, mode, opt);
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
                                if (dl::shape_adam_round(&q, 256, k0, at<void>(WS), kWsBytes,
                                                         nullptr, &L, err) == DL_OK)
                                    for (int i = 0; i < L.n; ++i)
                                        (L.l[i].fast ? n_fast : n_guarded)++;
                            }
    g_case = "grid totals";
    EXPECT(n_ok >= n_cases * 3 / 4);
    EXPECT(n_fast > 0 && n_guarded > 0);

    // m or v off 16 bytes, or a row stride of theirs that is no multiple of 4: the guarded kernel
    // alone (row-major), a refusal in the column-tiled layout
    for (int which = 0; which < 2; ++which) {
        g_case = "operand " + std::to_string(which) + " misaligned";
        auto put = [&](dl_adam_round_args &q, int64_t off) {
            if (which == 0) q.m = at<float>(M, off);
            if (which == 1) q.v = at<float>(V, off);
        };
        dl_adam_round_args q = args(64, 4096, true, 0, 0, false, 0);
        put(q, 4);
        dl::Launches L{};
        char err[dl::kErrLen] = "";
        EXPECT(dl::shape_adam_round(&q, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err) == DL_OK);
        for (int i = 0; i < L.n; ++i) EXPECT(!L.l[i].fast && !L.l[i].t.vec);
        q = args(64, 4096, true, 0, 0, false, 0);
        (which == 0 ? q.ldm : q.ldv) = 4098;
        EXPECT(dl::shape_adam_round(&q, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err) == DL_OK);
        for (int i = 0; i < L.n; ++i) {
            const dl::AdamTileArgs &t = L.l[i].a;
            EXPECT(!L.l[i].fast && (which == 0 ? t.mrs : t.vrs) == 4098 * 4);
        }
        q = args(64, 4096, true, 64, 0, false, 0);
        put(q, 4);
        check_refused(q, k0, DL_ERR_INVALID, "tiled operands must be 16-byte aligned", false);
    }

    // every illegal overlap, every missing operand, every stride and every parameter out of range,
    // row-major and column-tiled
    for (int32_t T : {0, 64}) {
        const int64_t bytes = 64 * 4096 * 4;
        auto base = [&]() { return args(64, 4096, true, T, 0, false, 0); };
        auto refused = [&](const char *name, dl_adam_round_args q, const char *text,
                           int status = DL_ERR_INVALID) {
            g_case = std::string(name) + (T ? " (tiled)" : "");
            check_refused(q, k0, status, text);
        };
        dl_adam_round_args q = base();
        q.m = at<float>(X);
        refused("m = x", q, "dl_adam_round: m overlaps x");
        q = base();
        q.m = at<float>(Y, bytes - 256);
        refused("m into y", q, "dl_adam_round: m overlaps y");
        q = base();
        q.m = at<float>(G, 256);
        refused("m into g", q, "dl_adam_round: m overlaps g");
        q = base();
        q.m = at<float>(V);
        refused("m = v", q, "dl_adam_round: m overlaps v");
        q = base();
        q.v = at<float>(M, bytes - 256);
        refused("v into m", q, "dl_adam_round: m overlaps v");
        q = base();
        q.v = at<float>(X, 256);
        refused("v into x", q, "dl_adam_round: v overlaps x");
        q = base();
        q.v = at<float>(Y);
        refused("v = y", q, "dl_adam_round: v overlaps y");
        q = base();
        q.v = at<float>(G);
        refused("v = g", q, "dl_adam_round: v overlaps g");
        q = base();
        q.mix.y = at<float>(X);
        q.v = at<float>(X);
        refused("y = v = x", q, "dl_adam_round: v overlaps x");
        q = base();
        q.mix.y = at<float>(G);
        refused("y = g", q, "dl_mix_round: y overlaps g");
        q = base();
        q.mix.y = at<float>(X, 256);
        refused("y partly on x", q, "dl_mix_round: y overlaps x");
        // missing operands
        for (int which = 0; which < 5; ++which) {
            q = base();
            if (which == 0) q.mix.x = nullptr;
            if (which == 1) q.mix.y = nullptr;
            if (which == 2) q.mix.g = nullptr;
            if (which == 3) q.m = nullptr;
            if (which == 4) q.v = nullptr;
            refused("a NULL operand", q, "dl_adam_round: null x/y/g/m/v");
        }
        // strides
        q = base();
        q.ldm = T ? 63 : 4095;
        refused("ldm too small", q, "dl_adam_round: m and v laid out as x");
        q = base();
        q.ldv = T ? -1 : 4095;
        refused("ldv too small", q, "dl_adam_round: m and v laid out as x");
        // the optimizer's parameters
        const float inf = std::numeric_limits<float>::infinity();
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (double b : {-0.1, 1.0, 1.5, (double)nan}) {
            q = base();
            q.beta1 = b;
            refused("beta1 out of range", q, "dl_adam_round: beta1 and beta2 must be in [0, 1)");
            q = base();
            q.beta2 = b;
            refused("beta2 out of range", q, "dl_adam_round: beta1 and beta2 must be in [0, 1)");
        }
        for (float e : {-1e-8f, nan}) {
            q = base();
            q.eps = e;
            refused("eps negative", q, "dl_adam_round: eps must be >= 0");
        }
        for (float c : {inf, -inf, nan}) {
            q = base();
            q.step_size = c;
            refused("step_size not finite", q,
                    "dl_adam_round: step_size and bias2_sqrt must be finite when coef is NULL");
            q = base();
            q.bias2_sqrt = c;
            refused("bias2_sqrt not finite", q,
                    "dl_adam_round: step_size and bias2_sqrt must be finite when coef is NULL");
        }
        // halo, partition and lagged-deviation fields
        const char *whole = "dl_adam_round: no halo rows, partition row sets or lagged deviation";
        q = base();
        q.mix.halo = at<float>(HALO);
        refused("halo", q, whole, DL_ERR_UNSUPPORTED);
        q = base();
        q.mix.n_halo = 3;
        refused("n_halo", q, whole, DL_ERR_UNSUPPORTED);
        q = base();
        q.mix.mean_prev = at<float>(MEAN_PREV);
        refused("mean_prev", q, whole, DL_ERR_UNSUPPORTED);
        q = base();
        q.mix.colsum_out = at<float>(COLSUM);
        refused("colsum_out", q, whole, DL_ERR_UNSUPPORTED);
        q = base();
        q.mix.n_local_src = 64;
        refused("n_local_src", q, whole, DL_ERR_UNSUPPORTED);
        q = base();
        q.mix.n_halo_blocks = 1;
        refused("n_halo_blocks", q, whole, DL_ERR_UNSUPPORTED);
        int32_t parts = 0;
        q = base();
        q.mix.partial_rows_out = &parts;
        refused("partial_rows_out", q, whole, DL_ERR_UNSUPPORTED);
    }
    {
        g_case = "args NULL";
        char err[dl::kErrLen] = "";
        dl::Launches L{};
        dl_mix_plan pub{};
        EXPECT(dl::shape_adam_round(nullptr, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err) ==
                   DL_ERR_INVALID && std::string(err) == "dl_adam_round: args is NULL");
        EXPECT(dl::shape_adam_round(nullptr, 256, k0, nullptr, 0, &pub, nullptr, err) ==
               DL_ERR_INVALID);
        g_case = "plan NULL";
        const dl_adam_round_args q = args(64, 4096, true, 0, 0, false, 0);
        EXPECT(dl::shape_adam_round(&q, 256, k0, nullptr, 0, nullptr, nullptr, err) ==
                   DL_ERR_INVALID && std::string(err) == "dl_adam_round_plan: plan is NULL");
    }

    // plan paths 2, 4 and 5 are refused with the header's text: forced by the knobs, and where
    // the planner chooses them (4096 agents with per-edge weights, an irregular graph of 3000)
    bool seen[6] = {};
    auto refused_path = [&](const char *name, dl_adam_round_args q, const dl::Knobs &k) {
        g_case = name;
        dl::Plan pl;
        char err[dl::kErrLen] = "";
        EXPECT(dl::plan_mix(q.mix, 256, k, &pl, err) == DL_OK);
        EXPECT(pl.pub.path == 2 || pl.pub.path == 4 || pl.pub.path == 5);
        if (pl.pub.path < 0 || pl.pub.path > 5) return;
        seen[pl.pub.path] = true;
        const std::string want = "dl_adam_round: the fused Adam round runs on the LDS tile kernel "
                                 "(plan path 1); this round plans path " +
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
        dl_adam_round_args big = args(4096, 1 << 16, true, 0, 0, dev, 0);
        big.mix.W.shared_row_weights = 0;
        refused_path("4096 agents, per-edge weights", big, k0);
        dl_adam_round_args irr = args(3000, 1 << 16, false, 0, 0, dev, 0);
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
