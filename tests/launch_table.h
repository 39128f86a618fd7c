// tests/golden/mix_launches.txt: one call of a round entry point per line and what it launched
// (format: test_launch_sweep_cpu.py), and tests/golden/lenet_launches.txt: one dl_lenet_grad call
// per line with its steps (format: test_lenet_abi.py).  Parsing of a line's left side into the
// call's arguments and printing of a launch, shared by launch_sweep.cpp, lenet_sweep.cpp and by
// the recorders that wrote the tables from the launch_* calls of the commit before that entry
// point's launch shaping became host-only code.
// Include after dl::TileArgs, dl::SgdTileArgs, dl::BgemmArgs, dl::LenetConvArgs and the args
// structs of dlamd.h are declared.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <sstream>
#include <string>

namespace launch_table {

// The operands are never read: each gets an address of its own, 1 TiB apart, and the table
// prints a pointer as its offset from there.
enum Base { X = 1, Y, G, HALO, MEAN, MEAN_PREV, COLSUM, DEV_SQ, DEV_MAX, WS, ROWPTR, COL, WEIGHTS,
            BUF, DATA, LABELS, LOSS, LOGITS, N_BASES };
inline uintptr_t base(int b) { return (uintptr_t)b << 40; }
template <class T>
T *at(int b, int64_t off = 0) { return reinterpret_cast<T *>(base(b) + off); }

struct Case {
    std::string name, entry, flags, knob, want;
    dl_mix_args a{};
    int32_t hblk_rows[32] = {};
    int32_t partial_rows = 0;
    int32_t rounds = 0;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    bool null_args = false;
    bool ok = false;
    // entry sgdround: the momentum buffer and the optimizer (flags mu=, ldb=, damp=, wd=, nest,
    // first, nullbuf, buf=x / buf=y / buf=g; the misalignment's fifth number is buf's offset)
    float *buf = nullptr;
    bool has(const char *flag) const {
        return ("," + flags + ",").find(std::string(",") + flag + ",") != std::string::npos;
    }
    // the number of a `key=number` flag
    double val(const char *key, double dflt) const {
        const size_t at = ("," + flags).find(std::string(",") + key + "=");
        return at == std::string::npos ? dflt : atof(flags.c_str() + at + strlen(key) + 1);
    }
    dl_sgd_round_args sgd() const {
        dl_sgd_round_args q{};
        q.mix = a;
        q.buf = buf;
        q.ldb = (int64_t)val("ldb", 0);
        q.momentum = (float)val("mu", 0);
        q.dampening = (float)val("damp", 0);
        q.weight_decay = (float)val("wd", 0);
        q.nesterov = has("nest");
        q.first = has("first");
        return q;
    }
};

inline void parse(const std::string &line, Case *c) {
    std::istringstream s(line);
    std::string mis, hblk, arrow;
    int dev, lag;
    int64_t ws_mis, ws_bytes;
    dl_mix_args &a = c->a;
    s >> c->name >> c->entry >> a.W.n_rows >> a.W.nnz >> a.W.uniform_row_nnz >>
        a.W.doubly_stochastic >> a.W.shared_row_weights >> a.W.min_row_nnz >> a.n_params >>
        a.tile_cols >> a.n_halo >> a.n_local_src >> dev >> lag >> a.ldx >> a.ldy >> a.ldg >>
        a.ldh >> mis >> hblk >> a.n_hub_rows >> ws_mis >> ws_bytes >> c->rounds >> c->flags >>
        c->knob >> arrow;
    std::getline(s >> std::ws, c->want);
    c->ok = s && arrow == "->";
    int64_t m[5] = {0, 0, 0, 0, 0};   // byte misalignment of x : y : g : halo [: buf]
    sscanf(mis.c_str(), "%ld:%ld:%ld:%ld:%ld", &m[0], &m[1], &m[2], &m[3], &m[4]);
    const int64_t mm = c->has("meanmis") ? 4 : 0;
    a.x = c->has("nullx") ? nullptr : at<float>(X, m[0]);
    a.y = c->has("nully") ? nullptr : c->has("y=x") ? at<float>(X, m[1])
          : c->has("y=g") ? at<float>(G, m[1]) : c->has("y=h") ? at<float>(HALO, m[1])
                                                                : at<float>(Y, m[1]);
    if (c->has("g")) a.g = at<float>(G, m[2]), a.lr = 0.5f;
    if (c->has("g=x")) a.g = at<float>(X, m[2]), a.lr = 0.5f;
    if (!c->has("nullbuf"))
        c->buf = at<float>(c->has("buf=x") ? X : c->has("buf=y") ? Y : c->has("buf=g") ? G : BUF,
                           m[4]);
    if (a.n_halo > 0 && !c->has("nullhalo")) a.halo = at<float>(HALO, m[3]);
    a.W.row_ptr = c->has("nullrp") ? nullptr : at<int32_t>(ROWPTR);
    a.W.col = c->has("nullcol") ? nullptr : at<int32_t>(COL);
    a.W.w = at<float>(WEIGHTS);
    if (dev && !c->has("nodevsq")) a.dev_sq = at<float>(DEV_SQ);
    if (dev && !c->has("nomax")) a.dev_max = at<float>(DEV_MAX);
    if (c->has("mean")) a.mean = at<float>(MEAN, mm);
    if (lag && !c->has("noprev")) a.mean_prev = at<float>(MEAN_PREV, mm);
    if (lag && !c->has("nocolsum")) a.colsum_out = at<float>(COLSUM, mm);
    if (c->has("pro")) a.partial_rows_out = &c->partial_rows;
    // halo blocks: 0, or n:rows:rows:...
    std::istringstream h(hblk);
    char colon;
    h >> a.n_halo_blocks;
    for (int b = 0; b < 32 && h >> colon >> c->hblk_rows[b]; ++b) {}
    if (a.n_halo_blocks != 0 && !c->has("nohbr")) a.halo_block_rows = c->hblk_rows;
    c->ws = ws_bytes < 0 ? nullptr : at<void>(WS, ws_mis);
    c->ws_bytes = ws_bytes < 0 ? 0 : (size_t)ws_bytes;
    c->null_args = c->has("nullargs");
}

inline std::string ptr(const void *p, int b) {
    return p ? std::to_string((int64_t)(reinterpret_cast<uintptr_t>(p) - base(b))) : "-";
}

// every scalar field of the kernels' parameter, in declaration order; the halo block tables up
// to n_hblk
inline std::string fmt(const dl::TileArgs &t) {
    std::ostringstream o;
    // y may have been put on another operand (the overlap refusals): those calls launch nothing
    o << "{" << ptr(t.x, X) << ' ' << t.ldx << ' ' << ptr(t.halo, HALO) << ' ' << t.ldh << ' '
      << ptr(t.g, G) << ' ' << t.ldg << ' ' << ptr(t.y, Y) << ' ' << t.ldy << ' '
      << ptr(t.rowptr, ROWPTR) << ' ' << ptr(t.col, COL) << ' ' << ptr(t.w, WEIGHTS) << ' '
      << t.n_rows << ' ' << t.n_src << ' ' << t.n_loc << ' ' << t.nnz << ' ' << t.regular << ' '
      << t.n_w << ' ' << t.mean_from_inputs << ' ' << t.nt_store << ' ' << t.nt_load << ' '
      << t.n_params << ' ' << t.n_tiles << ' ' << t.col_base << ' ' << t.lr << ' ' << t.vec << ' '
      << t.csr_off << ' ' << t.scratch_off << ' ' << t.tiled << ' ' << t.xts << ' ' << t.gts
      << ' ' << t.yts << ' ' << t.xrs << ' ' << t.grs << ' ' << t.yrs << ' ' << t.hrs << ' '
      << t.lchunks << ' ' << ptr(t.dev_partial, WS) << ' ' << ptr(t.mean, MEAN) << ' '
      << ptr(t.dev_max_zero, DEV_MAX) << ' ' << ptr(t.mean_prev, MEAN_PREV) << ' '
      << ptr(t.colsum_out, COLSUM) << ' ' << t.n_hblk << " [";
    for (int b = 0; b <= t.n_hblk && b <= 16; ++b) o << (b ? " " : "") << t.hblk_row0[b];
    o << "] [";
    for (int b = 0; b < t.n_hblk && b < 16; ++b) o << (b ? " " : "") << t.hblk_off[b];
    o << "] " << t.n_hub << ' ' << t.hub_off << ' ' << t.grp << ' ' << t.cd_sh << ' '
      << t.tile_run << "}";
    return o.str();
}

// one launch: the family, its selectors in the launch_* function's order, the kernel's parameter
inline std::string fmt_launch(const char *family, std::initializer_list<int> sel,
                              const dl::TileArgs &t) {
    std::string s = family;
    for (int v : sel) s += " " + std::to_string(v);
    return s + " " + fmt(t) + " ";
}

// the fused momentum round's launch: launch_mix_sgd_tile's selectors, the kernel's parameter and
// the momentum buffers' {buf ldb bts brs lr mu damp wd first nesterov}
inline std::string fmt_sgd_launch(int chunks, bool dev, bool fast, int grid, int lds,
                                  const dl::TileArgs &t, const dl::SgdTileArgs &q) {
    std::ostringstream o;
    o << fmt_launch("sgdtile", {chunks, dev, fast, grid, lds}, t) << "{" << ptr(q.buf, BUF) << ' '
      << q.ldb << ' ' << q.bts << ' ' << q.brs << ' ' << q.p.lr << ' ' << q.p.mu << ' '
      << q.p.damp << ' ' << q.p.wd << ' ' << q.p.first << ' ' << q.p.nesterov << "} ";
    return o.str();
}

// lenet_launches.txt.  A pointer prints as its operand's name and the byte offset from it.
inline std::string named(const void *p) {
    static const char *const name[N_BASES] = {"?", "X", "Y", "G", "HALO", "MEAN", "MEAN_PREV",
                                              "COLSUM", "DEV_SQ", "DEV_MAX", "WS", "ROWPTR", "COL",
                                              "WEIGHTS", "BUF", "DATA", "LABELS", "LOSS", "LOGITS"};
    if (!p) return "-";
    const uintptr_t v = reinterpret_cast<uintptr_t>(p), b = v >> 40;
    return std::string(b < N_BASES ? name[b] : "?") + "+" + std::to_string(v - (b << 40));
}

// A line's left side: name n_agents batch num_classes ldx_pad ldg_pad flags; ldx and ldg are the
// parameter count rounded up to 4 plus the pad, ldz = num_classes + 2 and s_logits = batch * ldz
// + 5; flags of g (G given), loss, logits, nolabels, sdata0 and slab0 (the shared strides).
struct LenetCase {
    std::string name, flags, want;
    dl_lenet_args a{};
    bool ok = false;
    bool has(const char *flag) const {
        return ("," + flags + ",").find(std::string(",") + flag + ",") != std::string::npos;
    }
};
inline void parse(const std::string &line, LenetCase *c) {
    std::istringstream s(line);
    std::string arrow;
    int64_t xpad, gpad;
    dl_lenet_args &a = c->a;
    s >> c->name >> a.n_agents >> a.batch >> a.num_classes >> xpad >> gpad >> c->flags >> arrow;
    std::getline(s >> std::ws, c->want);
    c->ok = s && arrow == "->";
    const int64_t P4 = (dl::lenet_param_count(a.num_classes) + 3) / 4 * 4;
    a.X = at<float>(X);
    a.ldx = P4 + xpad;
    a.data = at<float>(DATA);
    a.s_data = c->has("sdata0") ? 0 : (int64_t)a.batch * 3072;
    if (!c->has("nolabels")) a.labels = at<int32_t>(LABELS);
    a.s_labels = c->has("slab0") ? 0 : a.batch + 1;
    if (c->has("g")) a.G = at<float>(G);
    a.ldg = P4 + gpad;
    if (c->has("loss")) a.loss = at<float>(LOSS);
    if (c->has("logits")) a.logits = at<float>(LOGITS);
    a.ldz = a.num_classes + 2;
    a.s_logits = (int64_t)a.batch * a.ldz + 5;
}

// every field in declaration order
inline std::string fmt(const dl::BgemmArgs &p) {
    std::ostringstream o;
    o << "{" << p.batch << ' ' << p.M << ' ' << p.N << ' ' << p.K << ' ' << named(p.A) << ' '
      << p.lda << ' ' << p.sA << ' ' << p.ta << ' ' << named(p.B) << ' ' << p.ldb << ' ' << p.sB
      << ' ' << p.tb << ' ' << named(p.C) << ' ' << p.ldc << ' ' << p.sC << ' ' << p.epi << ' '
      << named(p.bias) << ' ' << p.sBias << ' ' << named(p.H) << ' ' << p.ldh << ' ' << p.sH
      << ' ' << named(p.rowsum) << ' ' << p.sR << ' ' << named(p.labels) << ' ' << p.sLab << ' '
      << named(p.loss) << "}";
    return o.str();
}
inline std::string fmt(const dl::LenetConvArgs &p) {
    std::ostringstream o;
    o << "{" << named(p.X) << ' ' << p.ldx << ' ' << named(p.data) << ' ' << p.s_data << ' '
      << named(p.pool1) << ' ' << named(p.code1) << ' ' << named(p.pool2) << ' '
      << named(p.code2) << ' ' << named(p.da) << ' ' << named(p.part) << ' ' << named(p.G) << ' '
      << p.ldg << ' ' << p.batch << ' ' << p.train << ' ' << p.passes << ' ' << p.fwd_wpa << ' '
      << p.groups << ' ' << p.bwd_wpa << "}";
    return o.str();
}
// the steps of a call as the launch_* functions take them
inline std::string fmt_conv(const char *which, const dl::LenetConvArgs &p, int grid_or_agents) {
    return std::string(which) + " " + std::to_string(grid_or_agents) + " " + fmt(p) + " ";
}
inline std::string fmt_gemm(const dl::BgemmArgs &p) { return "gemm " + fmt(p) + " "; }
inline std::string fmt_head(const float *Z, int64_t sZ, const int32_t *y, int64_t sY, float *dZ,
                            int64_t sD, float *loss, int batch, int rows, int classes) {
    std::ostringstream o;
    o << "head {" << named(Z) << ' ' << sZ << ' ' << named(y) << ' ' << sY << ' ' << named(dZ)
      << ' ' << sD << ' ' << named(loss) << ' ' << batch << ' ' << rows << ' ' << classes << "} ";
    return o.str();
}
inline std::string fmt_event(int k) { return "e" + std::to_string(k) + " "; }

}  // namespace launch_table
