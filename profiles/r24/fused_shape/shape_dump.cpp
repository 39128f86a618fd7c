// Differential of the fused rounds' launch shaping between two trees (README.md): links only
// csrc/launch.cpp and csrc/plan.cpp of the tree named by the include path (no HIP, no library),
// calls shape_sgd_round, shape_cheb_round and shape_track_round at 256 compute units and prints
// one line per call: status, the whole error text, the plan and every field of every launch.
//   shape_dump                 the call list below
//   shape_dump time ROUND N    nanoseconds per shaping call of one shaped case, N calls
#include <chrono>
#include <iostream>

#include "launch.h"
#include "launch_table.h"

namespace {

using namespace launch_table;

constexpr size_t kWsBytes = (size_t)1 << 24;
// dummy address spaces beside launch_table's: BUF is the momentum buffer, z and the tracker d
constexpr int DOUT = N_BASES, Q = N_BASES + 1, FAR = N_BASES + 2;

std::string any(const void *p) {   // a pointer of any address space: space:offset
    if (!p) return "-";
    const uintptr_t v = reinterpret_cast<uintptr_t>(p);
    return std::to_string(v >> 40) + ":" + std::to_string((int64_t)(v & (((uintptr_t)1 << 40) - 1)));
}

int n_calls = 0, n_refused = 0;

void print(const std::string &name, const char *mode, int rc, const char *err,
           const dl_mix_plan &p, const dl::Launches &L) {
    ++n_calls;
    if (rc) ++n_refused;
    std::ostringstream o;
    o << name << ' ' << mode << " -> " << rc << " \"" << err << "\" plan{" << p.path << ' '
      << p.tile_cols << ' ' << p.grid << ' ' << p.lds_bytes << ' ' << p.n_tiles << ' ' << p.regular
      << ' ' << p.head << ' ' << p.tail_fmt << "} L{" << L.n << ' ' << L.after << ' '
      << any(L.partial) << ' ' << L.parts << ' ' << L.rows << ' ' << L.max_zeroed << "}";
    for (int i = 0; i < L.n && i < 2; ++i) {
        const dl::Launch &l = L.l[i];
        dl::TileArgs t = l.t;
        o << " [" << l.kind << ' ' << l.grid << ' ' << l.lds << ' ' << l.chunks << ' ' << l.head
          << ' ' << l.tail_fmt << ' ' << l.rounds << ' ' << l.sgd << l.dev << l.mix << l.fast
          << l.columns << l.planes << l.gm << l.narrow << " y=" << any(t.y) << ' ';
        if (reinterpret_cast<uintptr_t>(t.y) >> 40 != Y) t.y = nullptr;   // fmt prints Y offsets
        o << fmt(t) << " q{" << any(l.q.buf) << ' ' << l.q.ldb << ' ' << l.q.bts << ' ' << l.q.brs
          << ' ' << l.q.p.lr << ' ' << l.q.p.mu << ' ' << l.q.p.damp << ' ' << l.q.p.wd << ' '
          << l.q.p.first << ' ' << l.q.p.nesterov << "} c{" << any(l.c.z) << ' ' << l.c.ldz << ' '
          << l.c.zts << ' ' << l.c.zrs << ' ' << l.c.a << ' ' << l.c.b << "} k{" << any(l.k.d)
          << ' ' << l.k.ldd << ' ' << any(l.k.d_out) << ' ' << l.k.lddo << ' ' << any(l.k.q) << ' '
          << l.k.ldq << ' ' << l.k.dts << ' ' << l.k.dots << ' ' << l.k.qts << ' ' << l.k.drs
          << ' ' << l.k.dors << ' ' << l.k.qrs << "}]";
    }
    std::cout << o.str() << "\n";
}

// One case through an entry point's three call forms: the plan query (with a NULL plan when
// null_plan), the launching call as the C ABI makes it (no plan) and as the sweeps do (plan too).
template <class Args>
void emit(const std::string &name,
          int (*shape)(const Args *, int, const dl::Knobs &, void *, size_t, dl_mix_plan *,
                       dl::Launches *, char *),
          const Args *a, const dl::Knobs &k, bool null_plan = false, bool no_ws = false) {
    void *ws = no_ws ? nullptr : at<void>(WS);
    const size_t wb = no_ws ? 0 : kWsBytes;
    for (int mode = 0; mode < 3; ++mode) {
        char err[dl::kErrLen] = "";
        dl_mix_plan pub{};
        dl::Launches L{};
        int rc;
        if (mode == 0)
            rc = shape(a, 256, k, nullptr, 0, null_plan ? nullptr : &pub, nullptr, err);
        else
            rc = shape(a, 256, k, ws, wb, mode == 2 ? &pub : nullptr, &L, err);
        print(name, mode == 0 ? "plan" : mode == 1 ? "run" : "run+plan", rc, err, pub, L);
    }
}

// the sweeps' graphs: 5 entries a row, shared weights, doubly stochastic; or irregular
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

dl_mix_args mix(int32_t n, int64_t P, bool regular, int32_t tile_cols, int64_t pad, bool dev,
                bool g, bool in_place) {
    dl_mix_args m{};
    m.W = csr(n, regular);
    m.n_params = P;
    m.tile_cols = tile_cols;
    m.x = at<float>(X);
    m.y = at<float>(in_place ? X : Y);
    if (g) m.g = at<float>(G), m.lr = 0.125f;
    m.ldx = m.ldy = tile_cols > 0 ? 0 : P + pad;
    if (g) m.ldg = m.ldx;
    if (dev) {
        m.dev_sq = at<float>(DEV_SQ);
        m.dev_max = at<float>(DEV_MAX);
        m.mean = at<float>(MEAN);
    }
    return m;
}

// variant: 0 no momentum and no buffer, 1 momentum, 2 Nesterov, 3 first step, 4 dampening
dl_sgd_round_args sgd(int32_t n, int64_t P, bool regular, int32_t T, int64_t pad, bool dev,
                      bool in_place, int variant) {
    dl_sgd_round_args q{};
    q.mix = mix(n, P, regular, T, pad, dev, true, in_place);
    q.weight_decay = 5e-4f;
    if (variant > 0) {
        q.buf = at<float>(BUF);
        q.ldb = q.mix.ldx;
        q.momentum = 0.9f;
    }
    q.nesterov = variant == 2;
    q.first = variant == 3;
    if (variant == 4) q.dampening = 0.1f;
    return q;
}
// y_at: 0 apart, 1 z itself, 2 x itself
dl_cheb_round_args cheb(int32_t n, int64_t P, bool regular, int32_t T, int64_t pad, bool dev,
                        int y_at) {
    dl_cheb_round_args q{};
    q.mix = mix(n, P, regular, T, pad, dev, false, y_at == 2);
    q.z = at<float>(BUF);
    q.ldz = q.mix.ldx;
    if (y_at == 1) q.mix.y = at<float>(BUF);
    q.a = 1.25f;
    q.b = -0.25f;
    return q;
}
// alias bit 0: x' = x, bit 1: d' = d
dl_track_round_args track(int32_t n, int64_t P, bool regular, int32_t T, int64_t pad, bool dev,
                          int alias) {
    dl_track_round_args q{};
    q.mix = mix(n, P, regular, T, pad, dev, true, alias & 1);
    q.d = at<float>(BUF);
    q.d_out = at<float>((alias & 2) ? BUF : DOUT);
    q.g_old = at<float>(Q);
    q.ldd = q.lddo = q.ldq = q.mix.ldx;
    return q;
}

// The three base cases of the refusals, 64 agents x 4096 parameters on the regular graph, and a
// change applied to one of them.
struct Three {
    dl_sgd_round_args s;
    dl_cheb_round_args c;
    dl_track_round_args t;
};
Three base(int32_t T, bool dev = false) {
    return {sgd(64, 4096, true, T, 0, dev, false, 1), cheb(64, 4096, true, T, 0, dev, 0),
            track(64, 4096, true, T, 0, dev, 0)};
}
void emit3(const std::string &name, const Three &b, const dl::Knobs &k, bool null_plan = false,
           bool no_ws = false) {
    emit("sgd:" + name, dl::shape_sgd_round, &b.s, k, null_plan, no_ws);
    emit("cheb:" + name, dl::shape_cheb_round, &b.c, k, null_plan, no_ws);
    emit("track:" + name, dl::shape_track_round, &b.t, k, null_plan, no_ws);
}
// f(mix) applied to all three
template <class F>
Three with_mix(Three b, F f) {
    f(b.s.mix);
    f(b.c.mix);
    f(b.t.mix);
    return b;
}
// the extra operand `which` (sgd: buf; cheb: z; track: 0 d, 1 d_out, 2 g_old) moved / re-strided
Three with_extra(Three b, int which, float *p, bool set_p, int64_t ld, bool set_ld) {
    if (set_p) {
        b.s.buf = p;
        b.c.z = p;
        if (which == 0) b.t.d = p;
        if (which == 1) b.t.d_out = p;
        if (which == 2) b.t.g_old = p;
    }
    if (set_ld) {
        b.s.ldb = b.c.ldz = ld;
        (which == 0 ? b.t.ldd : which == 1 ? b.t.lddo : b.t.ldq) = ld;
    }
    return b;
}

void grids(const dl::Knobs &k0) {
    const int32_t ns[] = {2, 33, 64, 300, 1024, 1500};
    const int64_t Ps[] = {7, 129, 777, 4096, 4100};
    for (int32_t n : ns)
        for (int64_t P : Ps)
            for (int tiled = 0; tiled < 2; ++tiled)
                for (int64_t pad : {0, 4})
                    for (int dev = 0; dev < 2; ++dev)
                        for (int regular = 0; regular < 2; ++regular) {
                            if (tiled && pad) continue;
                            int32_t T = 0;
                            if (tiled) {
                                T = dl::choose_tile_cols(csr(n, regular), 0, P, dev, k0);
                                if (T <= 0) continue;
                            }
                            const std::string at = "n=" + std::to_string(n) + ",P=" +
                                std::to_string(P) + ",T=" + std::to_string(T) + ",pad=" +
                                std::to_string(pad) + ",dev=" + std::to_string(dev) + ",reg=" +
                                std::to_string(regular);
                            for (int y_at = 0; y_at < 3; ++y_at) {
                                const auto q = cheb(n, P, regular, T, pad, dev, y_at);
                                emit("cheb:grid," + at + ",y=" + std::to_string(y_at),
                                     dl::shape_cheb_round, &q, k0);
                            }
                            for (int alias = 0; alias < 4; ++alias) {
                                const auto q = track(n, P, regular, T, pad, dev, alias);
                                emit("track:grid," + at + ",alias=" + std::to_string(alias),
                                     dl::shape_track_round, &q, k0);
                            }
                            for (int in_place = 0; in_place < 2; ++in_place)
                                for (int v = 0; v < 5; ++v) {
                                    const auto q = sgd(n, P, regular, T, pad, dev, in_place, v);
                                    emit("sgd:grid," + at + ",inplace=" + std::to_string(in_place) +
                                             ",v=" + std::to_string(v),
                                         dl::shape_sgd_round, &q, k0);
                                }
                        }
}

// every refusal of the three ABI tests and the sweeps, row-major and column-tiled
void refusals(const dl::Knobs &k0) {
    const int64_t N = 64, P = 4096, bytes = N * P * 4;
    emit<dl_sgd_round_args>("sgd:nullargs", dl::shape_sgd_round, nullptr, k0);
    emit<dl_cheb_round_args>("cheb:nullargs", dl::shape_cheb_round, nullptr, k0);
    emit<dl_track_round_args>("track:nullargs", dl::shape_track_round, nullptr, k0);
    for (int32_t T : {0, 64}) {
        const std::string lay = T ? "tiled," : "rows,";
        const Three b = base(T);
        emit3(lay + "valid", b, k0);
        emit3(lay + "valid,dev", base(T, true), k0);
        emit3(lay + "dev,no_ws", base(T, true), k0, false, true);
        emit3(lay + "nullplan", b, k0, true);
        emit3(lay + "nullx", with_mix(b, [](dl_mix_args &m) { m.x = nullptr; }), k0);
        emit3(lay + "nully", with_mix(b, [](dl_mix_args &m) { m.y = nullptr; }), k0);
        emit3(lay + "nullg", with_mix(b, [](dl_mix_args &m) { m.g = nullptr; }), k0);
        emit3(lay + "g_set", with_mix(b, [](dl_mix_args &m) { m.g = at<float>(G); m.ldg = m.ldx; }),
              k0);
        for (int w = 0; w < 3; ++w)
            emit3(lay + "nullextra" + std::to_string(w),
                  with_extra(b, w, (float *)nullptr, true, 0, false), k0);
        emit3(lay + "nullrowptr", with_mix(b, [](dl_mix_args &m) { m.W.row_ptr = nullptr; }), k0);
        emit3(lay + "ldx_small", with_mix(b, [](dl_mix_args &m) { m.ldx = m.tile_cols ? -1 : 4095; }),
              k0);
        emit3(lay + "ldg_small", with_mix(b, [](dl_mix_args &m) { m.ldg = m.tile_cols ? 63 : 4095; }),
              k0);
        emit3(lay + "n_params0", with_mix(b, [](dl_mix_args &m) { m.n_params = 0; }), k0);
        emit3(lay + "tile_cols48", with_mix(b, [](dl_mix_args &m) { m.tile_cols = 48; }), k0);
        // an extra operand not laid out as x, misaligned, or with rows no multiple of 16 bytes
        for (int w = 0; w < 3; ++w) {
            const std::string ws = std::to_string(w);
            for (int64_t ld : {P - 1, N - 1, (int64_t)-1, (int64_t)65535 * 4 + 1, P + 2,
                               (int64_t)1 << 26})
                emit3(lay + "extra" + ws + ",ld=" + std::to_string(ld),
                      with_extra(b, w, (float *)nullptr, false, ld, true), k0);
            const int space = w == 1 ? DOUT : w == 2 ? Q : BUF;
            emit3(lay + "extra" + ws + ",off4", with_extra(b, w, at<float>(space, 4), true, 0, false),
                  k0);
        }
        emit3(lay + "x_off4", with_mix(b, [](dl_mix_args &m) { m.x = at<float>(X, 4); }), k0);
        emit3(lay + "g_off4",
              with_mix(b, [](dl_mix_args &m) { if (m.g) m.g = at<float>(G, 4); }), k0);
        // overlaps: the extra operands on x, y, g and each other, y on everything
        for (int w = 0; w < 3; ++w)
            for (int space : {(int)X, (int)Y, (int)G, (int)BUF, DOUT, Q})
                for (int64_t off : {(int64_t)0, (int64_t)64, bytes - 4, -bytes + 4, bytes})
                    emit3(lay + "extra" + std::to_string(w) + "=" + std::to_string(space) + "+" +
                              std::to_string(off),
                          with_extra(b, w, at<float>(space, off), true, 0, false), k0);
        for (int space : {(int)X, (int)G, (int)BUF, DOUT, Q})
            for (int64_t off : {(int64_t)0, (int64_t)64, bytes - 4, -bytes + 4, bytes})
                emit3(lay + "y=" + std::to_string(space) + "+" + std::to_string(off),
                      with_mix(b, [&](dl_mix_args &m) { m.y = at<float>(space, off); }), k0);
        if (!T) {
            emit3(lay + "y=x,ldy+4",
                  with_mix(b, [&](dl_mix_args &m) { m.y = at<float>(X); m.ldy = P + 4; }), k0);
            emit3(lay + "extra1=d,ld+4", with_extra(b, 1, at<float>(BUF), true, P + 4, true), k0);
            emit3(lay + "y=z,ldy+4",
                  with_mix(b, [&](dl_mix_args &m) { m.y = at<float>(BUF); m.ldy = P + 4; }), k0);
            emit3(lay + "strides", [&] {
                Three t = with_mix(b, [&](dl_mix_args &m) {
                    m.ldx = P + 4; m.ldy = P + 8; if (m.g) m.ldg = P + 12; });
                t.s.ldb = t.c.ldz = t.t.ldd = P + 16;
                t.t.lddo = P + 20;
                t.t.ldq = P + 24;
                return t;
            }(), k0);
        } else {
            emit3(lay + "extra1=d+tile", with_extra(b, 1, at<float>(BUF, 64 * 4 * N), true, 0, false),
                  k0);
        }
        emit3(lay + "y=d_out=x", with_extra(with_mix(b, [](dl_mix_args &m) { m.y = at<float>(X); }),
                                            1, at<float>(X), true, 0, false), k0);
        emit3(lay + "y=d_out=d", with_extra(with_mix(b, [](dl_mix_args &m) { m.y = at<float>(BUF); }),
                                            1, at<float>(BUF), true, 0, false), k0);
        // the optimizer's rules
        Three o = b;
        o.s.nesterov = 1, o.s.momentum = 0.f, o.s.buf = nullptr;
        emit("sgd:" + lay + "nesterov,mu=0", dl::shape_sgd_round, &o.s, k0);
        o = b;
        o.s.nesterov = 1, o.s.momentum = -0.5f;
        emit("sgd:" + lay + "nesterov,mu<0", dl::shape_sgd_round, &o.s, k0);
        o = b;
        o.s.nesterov = 1, o.s.dampening = 0.1f;
        emit("sgd:" + lay + "nesterov,damp", dl::shape_sgd_round, &o.s, k0);
        o = b;
        o.s.mix.y = at<float>(X), o.s.mix.g = at<float>(X, 4096);
        emit("sgd:" + lay + "inplace,g_on_x", dl::shape_sgd_round, &o.s, k0);
        // whole rounds only
        static int32_t rows1[1] = {4}, parts = 0;
        emit3(lay + "halo", with_mix(b, [](dl_mix_args &m) { m.halo = at<float>(HALO); }), k0);
        emit3(lay + "n_halo", with_mix(b, [](dl_mix_args &m) { m.n_halo = 4; }), k0);
        emit3(lay + "halo+n_halo", with_mix(b, [&](dl_mix_args &m) {
                  m.halo = at<float>(HALO); m.n_halo = 4; m.ldh = P; }), k0);
        emit3(lay + "mean_prev", with_mix(b, [](dl_mix_args &m) { m.mean_prev = at<float>(MEAN_PREV); }),
              k0);
        emit3(lay + "colsum", with_mix(b, [](dl_mix_args &m) { m.colsum_out = at<float>(COLSUM); }),
              k0);
        emit3(lay + "n_local=N", with_mix(b, [](dl_mix_args &m) { m.n_local_src = 64; }), k0);
        emit3(lay + "n_local=N+8", with_mix(b, [](dl_mix_args &m) { m.n_local_src = 72; }), k0);
        emit3(lay + "halo_blocks", with_mix(b, [](dl_mix_args &m) {
                  m.n_halo_blocks = 1; m.halo_block_rows = rows1; }), k0);
        emit3(lay + "partial_rows_out", with_mix(b, [](dl_mix_args &m) { m.partial_rows_out = &parts; }),
              k0);
    }
}

// plan paths 2, 4 and 5: forced by the knobs, and where the planner chooses them
Three far(int32_t n, int64_t P, bool regular, int32_t T, int64_t pad, bool dev, int alias) {
    return {sgd(n, P, regular, T, pad, dev, alias & 1, 1), cheb(n, P, regular, T, pad, dev, alias % 3),
            track(n, P, regular, T, pad, dev, alias)};
}
void paths(const dl::Knobs &k0, const dl::Knobs &kg, const dl::Knobs &kr) {
    for (int dev = 0; dev < 2; ++dev) {
        const std::string d = dev ? "dev," : "";
        emit3(d + "forced_gather", far(64, 4096, true, 0, 0, dev, 3), kg);
        emit3(d + "forced_gather,irregular", far(300, 777, false, 0, 4, dev, 0), kg);
        emit3(d + "forced_reg,tiled", far(1500, 64, true, 4, 0, dev, 2), kr);
        emit3(d + "forced_reg,tiled,irregular", far(1500, 64, false, 4, 0, dev, 1), kr);
        emit3(d + "4096,per_edge", with_mix(far(4096, 1 << 16, true, 0, 0, dev, 0),
                                            [](dl_mix_args &m) { m.W.shared_row_weights = 0; }), k0);
        emit3(d + "3000,irregular", with_mix(far(3000, 1 << 16, false, 0, 0, dev, 0),
                                             [](dl_mix_args &m) {
                                                 m.W.nnz = 9000;
                                                 m.W.doubly_stochastic = 1;
                                                 m.W.min_row_nnz = 3;
                                             }), k0);
    }
}

// two defects in one call: which refusal wins
void pairs(const dl::Knobs &k0, const dl::Knobs &kg, const dl::Knobs &kr) {
    const int64_t P = 4096;
    auto halo = [](dl_mix_args &m) { m.n_halo = 4; };
    for (int32_t T : {0, 64}) {
        const std::string lay = T ? "pair,tiled," : "pair,rows,";
        const Three b = base(T);
        for (int w = 0; w < 3; ++w)
            emit3(lay + "nullextra" + std::to_string(w) + "+halo",
                  with_mix(with_extra(b, w, (float *)nullptr, true, 0, false), halo), k0);
        emit3(lay + "nullg+halo", with_mix(b, [](dl_mix_args &m) { m.g = nullptr; m.n_halo = 4; }), k0);
        emit3(lay + "g_set+halo", with_mix(b, [](dl_mix_args &m) {
                  m.g = at<float>(G); m.ldg = m.ldx; m.n_halo = 4; }), k0);
        emit3(lay + "g_set+nullz", with_extra(with_mix(b, [](dl_mix_args &m) {
                  m.g = at<float>(G); m.ldg = m.ldx; }), 0, (float *)nullptr, true, 0, false), k0);
        emit3(lay + "halo+ldx_small", with_mix(b, [](dl_mix_args &m) { m.n_halo = 4; m.ldx = -1; }), k0);
        emit3(lay + "ldx_small+bad_extra_ld",
              with_extra(with_mix(b, [](dl_mix_args &m) { m.ldx = m.tile_cols ? -1 : 4095; }), 0,
                         (float *)nullptr, false, -1, true), k0);
        // a bad extra ld + an illegal overlap of that operand, of another one, and of y
        for (int w = 0; w < 3; ++w) {
            const std::string ws = std::to_string(w);
            emit3(lay + "bad_ld" + ws + "+on_x", with_extra(b, w, at<float>(X), true, -1, true), k0);
            emit3(lay + "bad_ld" + ws + "+y_on_extra",
                  with_extra(with_mix(b, [](dl_mix_args &m) { m.y = at<float>(BUF, 64); }), w,
                             (float *)nullptr, false, -1, true), k0);
            emit3(lay + "bad_ld" + ws + "+y_on_x",
                  with_extra(with_mix(b, [](dl_mix_args &m) { m.y = at<float>(X, 64); }), w,
                             (float *)nullptr, false, -1, true), k0);
        }
        // the optimizer's order: buffer layout, Nesterov, the buffer's overlap
        Three o = b;
        o.s.ldb = -1, o.s.nesterov = 1, o.s.dampening = 0.1f, o.s.buf = at<float>(X);
        emit("sgd:" + lay + "bad_ldb+nesterov+buf_on_x", dl::shape_sgd_round, &o.s, k0);
        o.s.ldb = b.s.ldb;
        emit("sgd:" + lay + "nesterov+buf_on_x", dl::shape_sgd_round, &o.s, k0);
        o.s.buf = nullptr;
        emit("sgd:" + lay + "nullbuf+nesterov", dl::shape_sgd_round, &o.s, k0);
        o = b;
        o.s.buf = at<float>(X), o.s.mix.y = at<float>(G);
        emit("sgd:" + lay + "y_on_g+buf_on_x", dl::shape_sgd_round, &o.s, k0);
        // the tracking round's order: d_out vs d, d_out vs x, y, g, g_old, y vs d, g_old
        Three t = b;
        t.t.d_out = at<float>(BUF, 64), t.t.mix.y = at<float>(Q);
        emit("track:" + lay + "d_out_on_d+y_on_g_old", dl::shape_track_round, &t.t, k0);
        t.t.d_out = at<float>(Q, 64);
        emit("track:" + lay + "d_out_on_g_old+y_on_g_old", dl::shape_track_round, &t.t, k0);
        t.t.mix.y = at<float>(BUF);
        emit("track:" + lay + "d_out_on_g_old+y_on_d", dl::shape_track_round, &t.t, k0);
        t = b;
        t.t.d_out = at<float>(X, 64), t.t.d = at<float>(X);
        emit("track:" + lay + "d_out_on_d_and_x", dl::shape_track_round, &t.t, k0);
        t = b;
        t.t.d_out = at<float>(Y, 64), t.t.g_old = at<float>(Y);
        emit("track:" + lay + "d_out_on_y_and_g_old", dl::shape_track_round, &t.t, k0);
        t = b;
        t.t.mix.y = at<float>(BUF), t.t.g_old = at<float>(BUF, 64);
        emit("track:" + lay + "y_on_d_and_g_old", dl::shape_track_round, &t.t, k0);
        // an illegal overlap + a NULL plan; a NULL plan + forced path 2
        for (int w = 0; w < 3; ++w)
            emit3(lay + "extra" + std::to_string(w) + "_on_x+nullplan",
                  with_extra(b, w, at<float>(X), true, 0, false), k0, true);
        emit3(lay + "y_on_extra+nullplan",
              with_mix(b, [](dl_mix_args &m) { m.y = at<float>(BUF, 64); }), k0, true);
        emit3(lay + "nullplan+gather", b, kg, true);
        emit3(lay + "bad_ld+gather", with_extra(b, 0, (float *)nullptr, false, -1, true), kg);
        emit3(lay + "halo+gather", with_mix(b, halo), kg);
        // a misaligned operand + a forced path, a missing workspace + a misaligned operand
        for (int w = 0; w < 3; ++w) {
            const int space = w == 1 ? DOUT : w == 2 ? Q : BUF;
            emit3(lay + "extra" + std::to_string(w) + ",off4+gather",
                  with_extra(b, w, at<float>(space, 4), true, 0, false), kg);
            emit3(lay + "extra" + std::to_string(w) + ",off4+dev,no_ws",
                  with_extra(base(T, true), w, at<float>(space, 4), true, 0, false), k0, false, true);
        }
        emit3(lay + "x_off4+dev,no_ws",
              with_mix(base(T, true), [](dl_mix_args &m) { m.x = at<float>(X, 4); }), k0, false, true);
    }
    // a misaligned column-tiled operand + forced path 4
    const Three r = far(1500, 64, true, 4, 0, false, 0);
    for (int w = 0; w < 3; ++w) {
        const int space = w == 1 ? DOUT : w == 2 ? Q : BUF;
        emit3("pair,extra" + std::to_string(w) + ",off4+forced_reg",
              with_extra(r, w, at<float>(space, 4), true, 0, false), kr);
    }
    emit3("pair,x_off4+forced_reg", with_mix(r, [](dl_mix_args &m) { m.x = at<float>(X, 4); }), kr);
    emit3("pair,nullplan+forced_reg", r, kr, true);
    (void)P;
}

// Host cost of one shaping call: 64 agents x 4096 parameters, regular graph, with deviation.
int time_calls(const std::string &round, long n) {
    const dl::Knobs k0;
    const Three b = base(0, true);
    dl::Launches L{};
    char err[dl::kErrLen] = "";
    long sink = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (long i = 0; i < n; ++i) {
        int rc;
        if (round == "sgd")
            rc = dl::shape_sgd_round(&b.s, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err);
        else if (round == "cheb")
            rc = dl::shape_cheb_round(&b.c, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err);
        else
            rc = dl::shape_track_round(&b.t, 256, k0, at<void>(WS), kWsBytes, nullptr, &L, err);
        if (rc != DL_OK || L.n < 1) return 1;
        sink += L.l[0].grid + L.l[L.n - 1].kind;
    }
    const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0)
                          .count();
    std::cout << round << ' ' << ns / n << " ns/call (" << sink % 7 << ")\n";
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && std::string(argv[1]) == "time") return time_calls(argv[2], atol(argv[3]));
    dl::Knobs k0, kg, kr;
    kg.force_gather = true;
    kr.force_reg = true;
    grids(k0);
    refusals(k0);
    paths(k0, kg, kr);
    pairs(k0, kg, kr);
    std::cerr << n_calls << " calls, " << n_refused << " refused\n";
    return 0;
}
