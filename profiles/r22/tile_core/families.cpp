// Which instantiation families of mix_sgd_tile_kernel / mix_cheb_tile_kernel a round launches:
// shapes the round in host-only code (csrc/launch.cpp + plan.cpp, 256 compute units) and prints,
// per launch, FAST or guarded, C, KV, DEV, mean_from_inputs and reg5.  One case per input line:
//   name kind(sgd|cheb) n nnz uniform_row_nnz doubly_stochastic shared_row_weights min_row_nnz
//   P tile_cols(0 = row-major, -1 = the planner's tiled choice) ld dev
// Build: g++ -std=c++17 -I tests families.cpp csrc/launch.cpp csrc/plan.cpp (families.py does it).
#include <iostream>
#include <sstream>

#include "../../../distributed-learning_amd/csrc/launch.h"
#include "launch_table.h"

using namespace launch_table;

int main() {
    const dl::Knobs k;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream s(line);
        std::string name, kind;
        dl_mix_args m{};
        int64_t ld;
        int dev, tc;
        s >> name >> kind >> m.W.n_rows >> m.W.nnz >> m.W.uniform_row_nnz >> m.W.doubly_stochastic >>
            m.W.shared_row_weights >> m.W.min_row_nnz >> m.n_params >> tc >> ld >> dev;
        if (!s) continue;
        m.W.row_ptr = at<int32_t>(ROWPTR);
        m.W.col = at<int32_t>(COL);
        m.W.w = at<float>(WEIGHTS);
        m.x = at<float>(X);
        m.y = at<float>(Y);
        if (tc < 0) tc = dl::choose_tile_cols(m.W, 0, m.n_params, dev != 0, k);
        m.tile_cols = tc;
        m.ldx = m.ldy = tc > 0 ? 0 : ld;
        if (dev) {
            m.dev_sq = at<float>(DEV_SQ);
            m.dev_max = at<float>(DEV_MAX);
            m.mean = at<float>(MEAN);
        }
        dl::Launches L{};
        char err[dl::kErrLen] = "";
        int rc;
        if (kind == "sgd") {
            dl_sgd_round_args q{};
            m.g = at<float>(G);
            m.ldg = m.ldx;
            m.lr = 0.05f;
            q.mix = m;
            q.buf = at<float>(BUF);
            q.ldb = m.ldx;
            q.momentum = 0.9f;
            rc = dl::shape_sgd_round(&q, 256, k, at<void>(WS), (size_t)1 << 26, nullptr, &L, err);
        } else {
            dl_cheb_round_args q{};
            q.mix = m;
            q.z = at<float>(BUF);
            q.ldz = m.ldx;
            q.a = 1.5f;
            q.b = -0.5f;
            rc = dl::shape_cheb_round(&q, 256, k, at<void>(WS), (size_t)1 << 26, nullptr, &L, err);
        }
        if (rc != DL_OK) {
            std::cout << name << " " << kind << " refused: " << err << "\n";
            continue;
        }
        for (int i = 0; i < L.n; ++i) {
            const dl::Launch &l = L.l[i];
            const int kv = dl::tile_passes(l.chunks, l.t.n_src, l.fast);
            const bool reg5 = kv <= 4 && l.t.regular == 5 && l.t.n_w != l.t.nnz;
            std::cout << name << " " << kind << " " << (l.fast ? "FAST" : "guarded") << " C=" << l.chunks
                      << " KV=" << kv << " DEV=" << l.dev << " mfi=" << (l.dev && l.t.mean_from_inputs)
                      << " reg5=" << reg5 << " tiles=" << l.t.n_tiles << " grid=" << l.grid << "\n";
        }
    }
    return 0;
}
