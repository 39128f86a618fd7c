// Fused momentum-SGD consensus round for gfx950 (MI355X): X' = W sgd(X, G, M), M updated in
// the same pass -- torch.optim.SGD's step (sgd_elem.h) of every agent and the Mixer round that
// follows it (mixer.py:43-49), which dl_sgd_step + dl_mix_round run as two launches through a
// scratch matrix.
//
// Design (path 1): as mix_tile.hip.  Persistent 1024-thread workgroups each own
// column tiles of T = 4*C floats for all agents; the CSR is staged once per workgroup in LDS; the
// geometry (chunks, LDS offsets, grid, tiles) is the planner's for the same dl_mix_args.  Per
// tile a thread loads its rows' chunk of x, g and (unless `first`) buf, steps it with sgd_elem,
// writes buf back -- the thread that read an element writes it -- and puts the stepped value in
// the LDS image; after the barrier every output row is folded from LDS in CSR order (products and
// sums separate fp32 operations: the reference's left fold) and written to y.  20 B per element
// cross HBM (read x, g, buf; write buf, y) against 28 B for the two launches, and there is no
// scratch matrix.  y may be x itself: a workgroup stages all rows of its columns before it writes
// them, and no other workgroup touches those columns.
//
// The next tile's loads are in flight while the current one is mixed.  Three streams cost 12*KV
// VGPRs of prefetch per thread: all three ride the prefetch up to KV = 4 rows per thread (48
// VGPRs); at KV = 8 only x does, and g and buf are loaded while the tile is staged, four rows at
// a time -- prefetching g as well spills.  The guarded kernel (a row-major tail tile, unaligned
// operands; always 8 rows per thread, scalar accesses with 64-bit addresses) prefetches nothing
// and stages one row at a time in a rolled loop, for the same reason.
#include <type_traits>

#include "sgd_elem.h"
#include "tile_core.h"

namespace dl {
namespace {

__device__ __forceinline__ float4 sgd4(float4 x, float4 g, float4 &b, const SgdParams &p) {
    float4 t;
    t.x = sgd_elem(x.x, g.x, b.x, p);
    t.y = sgd_elem(x.y, g.y, b.y, p);
    t.z = sgd_elem(x.z, g.z, b.z, p);
    t.w = sgd_elem(x.w, g.w, b.w, p);
    return t;
}

// C, KV, DEV, FAST as mix_tile_kernel's (no halo rows, no row sets: every source row is an
// output row); MOM: momentum != 0, the momentum buffers are read (unless `first`) and written.
template <int C, int KV, bool MOM, bool DEV, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, kTileThreads)))
mix_sgd_tile_kernel(TileArgs a, SgdTileArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *tile = reinterpret_cast<float4 *>(smem);
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;  // rows covered per pass
    constexpr int T = 4 * C;
    constexpr bool PFG = FAST && KV <= 4;   // g and buf ride the prefetch
    constexpr bool PFB = MOM && PFG;
    constexpr int HB = 4;                   // FAST, KV = 8: rows of g and buf per staging step
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int R = a.n_rows;
    const int64_t P = a.n_params;
    const SgdParams p = q.p;
    const bool rd_buf = MOM && !p.first;

    // FAST-path byte offsets: lane row s / chunk c; pass k adds k * step
    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t og = (uint32_t)s * a.grs + lc;
    const uint32_t sg = (uint32_t)SLOTS * a.grs;
    uint32_t ob = MOM ? (uint32_t)s * q.brs + lc : 0u;
    const uint32_t sb = MOM ? (uint32_t)SLOTS * q.brs : 0u;
    uint32_t oy = (uint32_t)s * a.yrs + lc;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);

    float4 px[FAST ? KV : 1], pg[PFG ? KV : 1], pb[PFB ? KV : 1];
    DevAcc<C, KV, DEV && dev_per_lane(C, KV)> dv;   // per-agent ||y - mean||^2
    dev_zero(dv);

    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;

    auto prefetch = [&](int tile_id) {
        if (FAST) {
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
            const __amdgpu_buffer_rsrc_t rg = buf_rsrc(tile_base(a, a.g, a.gts, tile_id));
            // one straight-line loop per load policy (bit 0: x and buf non-temporal, bit 1: g)
            auto loads = [&](auto ax, auto ag) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = s + k * SLOTS < R;
                    px[k] = buf_ld4<decltype(ax)::value>(rx, ok ? ox + k * sx : lc);
                    if (PFG)
                        pg[PFG ? k : 0] = buf_ld4<decltype(ag)::value>(rg, ok ? og + k * sg : lc);
                }
                if (PFB && rd_buf) {
                    const __amdgpu_buffer_rsrc_t rb = buf_rsrc(tile_base(a, q.buf, q.bts, tile_id));
#pragma unroll
                    for (int k = 0; k < KV; ++k) {
                        const bool ok = s + k * SLOTS < R;
                        pb[PFB ? k : 0] = buf_ld4<decltype(ax)::value>(rb, ok ? ob + k * sb : lc);
                    }
                }
            };
            if (a.nt_load == 3) loads(PNT{}, PNT{});
            else if (a.nt_load == 1) loads(PNT{}, PPL{});
            else if (a.nt_load == 2) loads(PPL{}, PNT{});
            else loads(PPL{}, PPL{});
        }
    };

    // the fold of a row reads only LDS (reg5: at <= 4 rows per thread)
    const LdsCsr L = lds_csr(smem, a, KV <= 4);

    TileWalk tw = tile_walk(a);
    if (tw.id < tw.end) prefetch(tw.id);
    // the LDS CSR is staged behind the first tile's loads; the first staging barrier publishes it
    stage_csr(L, a, tid);
    for (; tw.id < tw.end; tw.id += tw.step) {
        const int tile_id = tw.id;
        // opaque per tile: keeps LICM from hoisting one offset register per pass
        asm volatile("" : "+v"(ox), "+v"(og), "+v"(ob), "+v"(oy));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tw.step;
        // this tile's momentum buffers (the prefetch holds only their values) and gradients
        const __amdgpu_buffer_rsrc_t rbc =
            buf_rsrc(MOM ? tile_base(a, q.buf, q.bts, tile_id) : tile_base(a, a.x, a.xts, tile_id));
        const __amdgpu_buffer_rsrc_t rgc = buf_rsrc(tile_base(a, a.g, a.gts, tile_id));
        auto load_x = [&](int k) {   // (guarded kernel)
            const int r = s + k * SLOTS;
            return ld4(a.x + (int64_t)(r < R ? r : 0) * a.ldx, col0 + 4 * c, P, false);
        };
        auto load_g = [&](int k) {
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t o = r < R ? og + (uint32_t)k * sg : lc;
                return (a.nt_load & 2) ? buf_ld4<kBufNT>(rgc, o) : buf_ld4<0>(rgc, o);
            }
            return ld4(a.g + (int64_t)(r < R ? r : 0) * a.ldg, col0 + 4 * c, P, false);
        };
        auto load_b = [&](int k) {
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t o = r < R ? ob + (uint32_t)k * sb : lc;
                return (a.nt_load & 1) ? buf_ld4<kBufNT>(rbc, o) : buf_ld4<0>(rbc, o);
            }
            return ld4(q.buf + (int64_t)(r < R ? r : 0) * q.ldb, col0 + 4 * c, P, false);
        };
        auto store_b = [&](int k, const float4 &b) {   // row s + k * SLOTS < R
            if (FAST) {
                if (a.nt_store)
                    buf_st4<kBufNT>(b, rbc, ob + (uint32_t)k * sb);
                else
                    buf_st4<0>(b, rbc, ob + (uint32_t)k * sb);
            } else {
                st4(q.buf + (int64_t)(s + k * SLOTS) * q.ldb, col0 + 4 * c, P, false, b);
            }
        };
        // step every source row and stage the stepped tile in LDS
        float4 cst = zero4();  // column partial sums of t (doubly stochastic W only)
        auto stage = [&](int k, float4 x, float4 g, float4 b) {
            const int r = s + k * SLOTS;
            const float4 t = sgd4(x, g, b, p);
            if (r < R) {
                if (MOM) store_b(k, b);
                tile[r * C + c] = t;
                if (DEV) add4(cst, t);
            }
        };
        if constexpr (PFG) {
#pragma unroll
            for (int k = 0; k < KV; ++k)
                stage(k, px[k], pg[PFG ? k : 0], (PFB && rd_buf) ? pb[PFB ? k : 0] : zero4());
        } else if constexpr (FAST) {
#pragma unroll
            for (int k0 = 0; k0 < KV; k0 += HB) {
                float4 hg[HB], hb[HB];
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    hg[j] = k0 + j < KV ? load_g(k0 + j) : zero4();
                    hb[j] = (rd_buf && k0 + j < KV) ? load_b(k0 + j) : zero4();
                }
#pragma unroll
                for (int j = 0; j < HB; ++j)
                    if (k0 + j < KV) stage(k0 + j, px[(k0 + j) % KV], hg[j], hb[j]);
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < KV; ++k)
                stage(k, load_x(k), load_g(k), rd_buf ? load_b(k) : zero4());
        }
        // mean(W t) = mean(t) when W is doubly stochastic: reduce the column sums of the inputs
        // under the staging barrier instead of re-mixing the tile afterwards
        const bool mfi = DEV && a.mean_from_inputs;
        if (mfi) col_sums_to_scratch<C>(cst, scratch, tid);
        __syncthreads();
        // the next tile's loads go out first: they land while we mix from LDS
        if (nxt < tw.end) prefetch(nxt);
        float4 mean_t = zero4();
        if (mfi) mean_t = div4(col_sums_from_scratch<C>(scratch, c), (float)R);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(tile_base(a, a.y, a.yts, tile_id));
        float4 cs = zero4();
        // passes stay rolled: interleaving them would hold KV accumulators at once on top of the
        // prefetch registers
#pragma unroll 1
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS;
            if (ag < R) {
                const float4 acc = csr_fold<C>(L, tile, ag, c);
                store_y<FAST>(a, ry, oy + (uint32_t)k * sy, ag, col0 + 4 * c, acc);
                if (DEV) {
                    if (mfi)
                        dev_add(dv, k, acc, mean_t, c);
                    else
                        add4(cs, acc);
                }
            }
        }
        if (mfi && a.mean != nullptr && s == 0) st4(a.mean, col0 + 4 * c, P, FAST, mean_t);
        if (DEV && !mfi) {
            const float4 mean = tile_mean<C>(cs, scratch, tid, c, R);
            if (a.mean != nullptr && s == 0) st4(a.mean, col0 + 4 * c, P, FAST, mean);
            // second LDS pass: recompute y (same order, same bits) instead of holding it
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                const int ag = s + k * SLOTS;
                if (ag < R) dev_add(dv, k, csr_fold<C>(L, tile, ag, c), mean, c);
            }
        }
        __syncthreads();  // tile and scratch are rewritten by the next iteration
    }
    if (DEV) dev_epilogue(dv, a, tid, R);
}

template <int C, int KV, bool FAST>
hipError_t launch_kv(const TileArgs &a, const SgdTileArgs &q, bool mom, bool dev, int grid,
                     int lds, hipStream_t s) {
    if (mom)
        return dev ? launch_lds(mix_sgd_tile_kernel<C, KV, true, true, FAST>, grid, lds, s, a, q)
                   : launch_lds(mix_sgd_tile_kernel<C, KV, true, false, FAST>, grid, lds, s, a, q);
    return dev ? launch_lds(mix_sgd_tile_kernel<C, KV, false, true, FAST>, grid, lds, s, a, q)
               : launch_lds(mix_sgd_tile_kernel<C, KV, false, false, FAST>, grid, lds, s, a, q);
}

}  // namespace

hipError_t launch_mix_sgd_tile(const TileArgs &a, const SgdTileArgs &q, int chunks, bool dev,
                               int grid, int lds, bool fast, hipStream_t s) {
    // no halo rows and no row sets: every staged row is a local source row and an output row
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows || a.g == nullptr) return hipErrorInvalidValue;
    const bool mom = q.p.mu != 0.f;
    if (mom && q.buf == nullptr) return hipErrorInvalidValue;
    // FAST kernels: every C x KV in {2, 4, 8}; guarded kernels: every C, KV = 8 (plan.h
    // tile_passes)
    return with_chunks(chunks, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        if (!fast) return launch_kv<C, kRowsPerThread, false>(a, q, mom, dev, grid, lds, s);
        return with_passes(tile_passes(C, a.n_src, true), [&](auto kv) {
            return launch_kv<C, decltype(kv)::value, true>(a, q, mom, dev, grid, lds, s);
        });
    });
}

}  // namespace dl
