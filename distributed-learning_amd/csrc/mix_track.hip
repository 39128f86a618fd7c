// Gradient-tracking consensus round for gfx950 (MI355X): D' = W ((D + G) - G_old), X' = W (X - lr
// D') in one HBM pass -- each agent's tracker of the network-average gradient is updated and
// mixed, and the parameters step along the freshly mixed tracker and are mixed in turn, which two
// element-wise torch kernels and two dl_mix_round launches run through a scratch matrix.
//
// Design (path 1): as mix_sgd.hip.  Persistent 1024-thread workgroups each own
// column tiles of T = 4*C floats for all agents; the CSR is staged once per workgroup in LDS; the
// geometry (chunks, LDS offsets, grid, tiles) is the planner's for the same dl_mix_args.  A
// workgroup holds every agent of its columns, so the mixed tracker of every neighbour is inside
// it when the parameter mix needs it: both mixes of a round share ONE LDS image, used twice per
// tile --
//   1. t = fl(fl(d + g) - q) is staged; barrier; every row of d' is folded from LDS in CSR order
//      (products and sums separate fp32 operations: the reference's left fold) and written;
//   2. barrier; s = fl(x - fl(lr d')) is staged over t, from x and the d' the SAME thread just
//      folded: the thread that stages a (row, chunk) is the one that outputs it, so d' stays in
//      registers (4*KV VGPRs) and is never read back;
//   3. barrier; every row of x' is folded, written, and its deviation accumulated.
// 24 B per element cross HBM (read x, d, g, q; write d', x') against 36 B or more for the
// composed launches.  d' may be d itself and x' may be x itself: a workgroup stages all rows of
// its columns before it writes them, and no other workgroup touches those columns.
//
// Four input streams; vmcnt retires in order, so each is issued where the next thing waited for
// was issued before it.  Up to KV = 4 rows per thread: behind phase 1's barrier x of THIS tile
// goes out first, then d of the next tile; they land under the first fold (8 B per element in
// flight beside the d' stores).  Behind phase 2's barrier g and q of the next tile go out and
// land under the second fold (8 B beside the x' stores).  The staging of s waits on x alone,
// the staging of the next t on everything.  At most 12*KV VGPRs are live at once: x, d' and the
// next d under the first fold, the next d, g and q under the second.  At KV = 8 only d rides
// ahead, issued behind phase 2's barrier; g and q are loaded while t is staged, four rows at a
// time (x, d' under the first fold: 8*KV VGPRs).  The folds' passes stay rolled loops, which
// cannot index registers by the pass: a pass pushes its d' into the last register of a rotating
// set (4*KV moves a pass), so KV passes leave row k's value in register k.  The guarded kernel (a
// row-major tail tile, unaligned operands; always 8 rows per thread, scalar accesses with 64-bit
// addresses) prefetches nothing and stages one row at a time in rolled loops.
//
// Cache policy: the four inputs are streamed once and load non-temporally (TileArgs::nt_load: bit
// 0 x and d, bit 1 g and q); x' follows the round's rule (TileArgs::nt_store: plain below the
// MALL size so the next gradient launch finds it, non-temporal above), and d' follows the same
// flag: below the MALL size the next round, one gradient launch later, reads it back.
#include <type_traits>

#include "tile_core.h"

namespace dl {
namespace {

// fl(fl(d + g) - q): two separately rounded operations (-ffp-contract=off)
__device__ __forceinline__ float4 track4(float4 d, float4 g, float4 q) {
    float4 t;
    t.x = (d.x + g.x) - q.x;
    t.y = (d.y + g.y) - q.y;
    t.z = (d.z + g.z) - q.z;
    t.w = (d.w + g.w) - q.w;
    return t;
}

// fl(x - fl(lr d)): dl_mix_round's fused step
__device__ __forceinline__ float4 step4(float4 x, float lr, float4 d) {
    float4 s;
    s.x = x.x - lr * d.x;
    s.y = x.y - lr * d.y;
    s.z = x.z - lr * d.z;
    s.w = x.w - lr * d.w;
    return s;
}

// C, KV, DEV, FAST as mix_sgd_tile_kernel's (no halo rows, no row sets)
template <int C, int KV, bool DEV, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, kTileThreads)))
mix_track_tile_kernel(TileArgs a, TrackTileArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *tile = reinterpret_cast<float4 *>(smem);
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;  // rows covered per pass
    constexpr int T = 4 * C;
    constexpr bool PFG = FAST && KV <= 4;   // g and q ride ahead as well as d
    constexpr int HB = 4;                   // FAST, KV = 8: rows of g and q per staging step
    constexpr int KF = FAST ? KV : 1;
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int R = a.n_rows;
    const int64_t P = a.n_params;
    const float lr = a.lr;

    // FAST-path byte offsets: lane row s / chunk c; pass k adds k * step
    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t og = (uint32_t)s * a.grs + lc;
    const uint32_t sg = (uint32_t)SLOTS * a.grs;
    uint32_t od = (uint32_t)s * q.drs + lc;
    const uint32_t sd = (uint32_t)SLOTS * q.drs;
    uint32_t oq = (uint32_t)s * q.qrs + lc;
    const uint32_t sq = (uint32_t)SLOTS * q.qrs;
    uint32_t oo = (uint32_t)s * q.dors + lc;
    const uint32_t so = (uint32_t)SLOTS * q.dors;
    uint32_t oy = (uint32_t)s * a.yrs + lc;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;
    // staged element of pass k: tile[(s + k * SLOTS) * C + c] = tile[tid + k * NT]
    uint32_t ot = (uint32_t)tid;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);

    float4 pd[KF], pg[PFG ? KV : 1], pq[PFG ? KV : 1];
    DevAcc<C, KV, DEV && dev_per_lane(C, KV)> dv;   // per-agent ||x' - mean||^2
    dev_zero(dv);

    // KV rows of one stream, one straight-line loop per load policy
    auto load_rows = [&](float4 *dst, const void *p, int64_t ts, int tile_id, uint32_t o,
                         uint32_t st, bool nt) {
        const __amdgpu_buffer_rsrc_t r = buf_rsrc(tile_base(a, p, ts, tile_id));
        if (nt) {
#pragma unroll
            for (int k = 0; k < KV; ++k)
                dst[k] = buf_ld4<kBufNT>(r, s + k * SLOTS < R ? o + k * st : lc);
        } else {
#pragma unroll
            for (int k = 0; k < KV; ++k)
                dst[k] = buf_ld4<0>(r, s + k * SLOTS < R ? o + k * st : lc);
        }
    };
    auto prefetch_d = [&](int tile_id) {
        if constexpr (FAST) load_rows(pd, q.d, q.dts, tile_id, od, sd, a.nt_load & 1);
    };
    auto prefetch_gq = [&](int tile_id) {
        if constexpr (PFG) {
            load_rows(pg, a.g, a.gts, tile_id, og, sg, a.nt_load & 2);
            load_rows(pq, q.q, q.qts, tile_id, oq, sq, a.nt_load & 2);
        }
    };

    auto clear_d = [&]() {
#pragma unroll
        for (int k = 0; k < KF; ++k) pd[k] = zero4();
    };
    auto clear_gq = [&]() {
#pragma unroll
        for (int k = 0; k < (PFG ? KV : 1); ++k) pg[k] = pq[k] = zero4();
    };

    // the fold of a row reads only LDS (reg5: at <= 4 rows per thread)
    const LdsCsr L = lds_csr(smem, a, KV <= 4);

    TileWalk tw = tile_walk(a);
    if (tw.id < tw.end) {
        prefetch_d(tw.id);
        prefetch_gq(tw.id);
    }
    // the LDS CSR is staged behind the first tile's loads; the first staging barrier publishes it
    stage_csr(L, a, tid);
    for (; tw.id < tw.end; tw.id += tw.step) {
        const int tile_id = tw.id;
        // opaque per tile: keeps LICM from hoisting one offset register per pass
        asm volatile("" : "+v"(ox), "+v"(og), "+v"(od), "+v"(oq), "+v"(oo), "+v"(oy), "+v"(ot));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tw.step;
        // a guarded load of row s + k * SLOTS of a row-major operand
        auto load_s = [&](const float *p, int64_t ld, int k) {
            const int r = s + k * SLOTS;
            return ld4(p + (int64_t)(r < R ? r : 0) * ld, col0 + 4 * c, P, false);
        };

        // ---- phase 1: stage t = (d + g) - q
        if constexpr (PFG) {
#pragma unroll
            for (int k = 0; k < KV; ++k)
                if (s + k * SLOTS < R)
                    tile[ot + (uint32_t)k * NT] = track4(pd[k], pg[PFG ? k : 0], pq[PFG ? k : 0]);
        } else if constexpr (FAST) {
            const __amdgpu_buffer_rsrc_t rgc = buf_rsrc(tile_base(a, a.g, a.gts, tile_id));
            const __amdgpu_buffer_rsrc_t rqc = buf_rsrc(tile_base(a, q.q, q.qts, tile_id));
#pragma unroll
            for (int k0 = 0; k0 < KV; k0 += HB) {
                float4 hg[HB], hq[HB];
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    const int k = k0 + j;
                    const bool ok = k < KV && s + k * SLOTS < R;
                    const uint32_t ofg = ok ? og + (uint32_t)k * sg : lc;
                    const uint32_t ofq = ok ? oq + (uint32_t)k * sq : lc;
                    hg[j] = (a.nt_load & 2) ? buf_ld4<kBufNT>(rgc, ofg) : buf_ld4<0>(rgc, ofg);
                    hq[j] = (a.nt_load & 2) ? buf_ld4<kBufNT>(rqc, ofq) : buf_ld4<0>(rqc, ofq);
                }
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    const int k = k0 + j;
                    if (k < KV && s + k * SLOTS < R)
                        tile[ot + (uint32_t)k * NT] = track4(pd[k % KF], hg[j], hq[j]);
                }
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                const int r = s + k * SLOTS;
                const float4 t = track4(load_s(q.d, q.ldd, k), load_s(a.g, a.ldg, k),
                                        load_s(q.q, q.ldq, k));
                if (r < R) tile[r * C + c] = t;
            }
        }
        __syncthreads();
        // x of this tile first (phase 2 waits on it alone), then the next tile's d
        float4 cx[KF];
        if constexpr (FAST) load_rows(cx, a.x, a.xts, tile_id, ox, sx, a.nt_load & 1);
        // (a last tile clears the registers instead: the values staged above are then dead here,
        // not carried round the loop beside x and d')
        if (PFG) {
            if (nxt < tw.end) prefetch_d(nxt);
            else clear_d();
        }
        // fold d' and write it; the pass's value is pushed into dn's last register and the rows
        // rotate by one, so KV passes leave row k's d' in dn[k]
        float4 dn[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) dn[k] = zero4();
        const __amdgpu_buffer_rsrc_t ro = buf_rsrc(tile_base(a, q.d_out, q.dots, tile_id));
#pragma unroll 1
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS;
            float4 v = zero4();
            if (ag < R) {
                v = csr_fold<C>(L, tile, ag, c);
                if (FAST) {
                    if (a.nt_store)
                        buf_st4<kBufNT>(v, ro, oo + (uint32_t)k * so);
                    else
                        buf_st4<0>(v, ro, oo + (uint32_t)k * so);
                } else {
                    st4(q.d_out + (int64_t)ag * q.lddo, col0 + 4 * c, P, false, v);
                }
            }
#pragma unroll
            for (int j = 0; j + 1 < KV; ++j) dn[j] = dn[j + 1];
            dn[KV - 1] = v;
        }
        __syncthreads();   // every row of d' is folded: the image is rewritten

        // ---- phase 2: stage s = x - lr d'
        // mean(W s) = mean(s) when W is doubly stochastic: reduce the column sums of s under the
        // staging barrier instead of re-mixing the tile afterwards
        bool mfi = DEV && a.mean_from_inputs;
        float4 cst = zero4();
        if constexpr (FAST) {
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                if (s + k * SLOTS < R) {
                    const float4 sv = step4(cx[k % KF], lr, dn[k]);
                    tile[ot + (uint32_t)k * NT] = sv;
                    if (DEV) add4(cst, sv);
                }
            }
        } else {
            // rolled: the row's d' is dn[0] and the rows rotate by one after it, so KV steps
            // leave dn as they found it
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                const int r = s + k * SLOTS;
                const float4 sv = step4(load_s(a.x, a.ldx, k), lr, dn[0]);
                if (r < R) {
                    tile[r * C + c] = sv;
                    if (DEV) add4(cst, sv);
                }
                const float4 d0 = dn[0];
#pragma unroll
                for (int j = 0; j + 1 < KV; ++j) dn[j] = dn[j + 1];
                dn[KV - 1] = d0;
            }
        }
        if (mfi) col_sums_to_scratch<C>(cst, scratch, tid);
        __syncthreads();
        // the next tile's remaining loads go out first: they land while we mix from LDS
        if (nxt < tw.end) {
            if (!PFG) prefetch_d(nxt);
            prefetch_gq(nxt);
        } else {
            if (!PFG) clear_d();
            clear_gq();
        }
        float4 mean_t = zero4();
        if (mfi) {
            mean_t = div4(col_sums_from_scratch<C>(scratch, c), (float)R);
            // s can hold +inf and -inf where x' and its mean are finite or one-signed (a diverged
            // run): a tile with a mean that is not finite takes the two-pass form, the mean
            // summed from x' itself as numpy does; a tile of finite means keeps this one, bit for
            // bit (mix_cheb.hip: t - t is 0 for a finite t and NaN otherwise; every wave holds
            // all C columns, so the vote of one wave is the workgroup's)
            const float t = (mean_t.x + mean_t.y) + (mean_t.z + mean_t.w);
            if (__any(t - t != 0.f)) {
                __syncthreads();   // every wave has read scratch before tile_mean rewrites it
                mfi = false;
                mean_t = zero4();
            }
        }
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
            // second LDS pass: recompute x' (same order, same bits) instead of holding it
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
hipError_t launch_kv(const TileArgs &a, const TrackTileArgs &q, bool dev, int grid, int lds,
                     hipStream_t s) {
    return dev ? launch_lds(mix_track_tile_kernel<C, KV, true, FAST>, grid, lds, s, a, q)
               : launch_lds(mix_track_tile_kernel<C, KV, false, FAST>, grid, lds, s, a, q);
}

}  // namespace

hipError_t launch_mix_track_tile(const TileArgs &a, const TrackTileArgs &q, int chunks, bool dev,
                                 int grid, int lds, bool fast, hipStream_t s) {
    // no halo rows and no row sets: every staged row is a local source row and an output row
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows || a.g == nullptr || q.d == nullptr ||
        q.d_out == nullptr || q.q == nullptr)
        return hipErrorInvalidValue;
    // FAST kernels: every C x KV in {2, 4, 8}; guarded kernels: every C, KV = 8 (plan.h
    // tile_passes)
    return with_chunks(chunks, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        if (!fast) return launch_kv<C, kRowsPerThread, false>(a, q, dev, grid, lds, s);
        return with_passes(tile_passes(C, a.n_src, true), [&](auto kv) {
            return launch_kv<C, decltype(kv)::value, true>(a, q, dev, grid, lds, s);
        });
    });
}

}  // namespace dl
