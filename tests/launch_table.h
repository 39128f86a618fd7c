// tests/golden/mix_launches.txt: one call of a round entry point per line and what it launched
// (format: test_launch_sweep_cpu.py).  Parsing of a line's left side into the call's arguments
// and printing of a launch, shared by launch_sweep.cpp and by the recorder that wrote the table
// from the launch_* calls of the commit before the launch shaping became host-only code.
// Include after dl::TileArgs and dl_mix_args are declared.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <sstream>
#include <string>

namespace launch_table {

// The operands are never read: each gets an address of its own, 1 TiB apart, and the table
// prints a pointer as its offset from there.
enum Base { X = 1, Y, G, HALO, MEAN, MEAN_PREV, COLSUM, DEV_SQ, DEV_MAX, WS, ROWPTR, COL, WEIGHTS };
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
    bool has(const char *flag) const {
        return ("," + flags + ",").find(std::string(",") + flag + ",") != std::string::npos;
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
    int64_t m[4] = {0, 0, 0, 0};   // byte misalignment of x : y : g : halo
    sscanf(mis.c_str(), "%ld:%ld:%ld:%ld", &m[0], &m[1], &m[2], &m[3]);
    const int64_t mm = c->has("meanmis") ? 4 : 0;
    a.x = c->has("nullx") ? nullptr : at<float>(X, m[0]);
    a.y = c->has("nully") ? nullptr : c->has("y=x") ? at<float>(X, m[1])
          : c->has("y=g") ? at<float>(G, m[1]) : c->has("y=h") ? at<float>(HALO, m[1])
                                                                : at<float>(Y, m[1]);
    if (c->has("g")) a.g = at<float>(G, m[2]), a.lr = 0.5f;
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

}  // namespace launch_table
