// Fused Adam consensus round for gfx950 (MI355X): X' = W adam(X, G, M, V), M and V updated in the
// same pass -- torch.optim.Adam's / AdamW's step (adam_elem.h) of every agent and the Mixer round
// that follows it, which dl_adam_step + dl_mix_round run as two launches through a scratch matrix.
//
// Design (path 1): as mix_sgd.hip.  Persistent 1024-thread workgroups each own
// column tiles of T = 4*C floats for all agents; the CSR is staged once per workgroup in LDS; the
// geometry (chunks, LDS offsets, grid, tiles) is the planner's for the same dl_mix_args.  Per
// tile a thread loads its rows' chunk of x, g, m and v, steps it with adam_elem, writes m' and v'
// back -- the thread that read an element writes it -- and puts the stepped value in the LDS
// image; after the barrier every output row is folded from LDS in CSR order (products and sums
// separate fp32 operations: the reference's left fold) and written to y.  28 B per element cross
// HBM (read x, g, m, v; write m', v', y) against 36 B for the two launches, and there is no
// scratch matrix.  y may be x itself: a workgroup stages all rows of its columns before it writes
// them, and no other workgroup touches those columns.  The bias-correction coefficients come by
// value or, with AdamParams::coef, from two ordinary loads per workgroup (dl_adam_tick's outputs:
// a captured graph then advances the step count itself).
//
// The next tile's loads are in flight while the current one is mixed.  Four streams would cost
// 16*KV VGPRs of prefetch per thread.  From the compiler's resource report (no scratch, no
// spills, at most 128 VGPRs in every instantiation; profiles/r25/adam_round/vgprs.txt): at KV = 2
// rows per thread all four ride the prefetch (32 VGPRs); at KV = 4 x and g do (32 VGPRs) and m and
// v are loaded while the tile is staged, four rows at once; at KV = 8 only x does (32 VGPRs), and
// g, m and v are loaded while the tile is staged, two rows at a time (four rows of three streams
// spilled one register at C = 2).  43-118 VGPRs over the 48 instantiations.  The guarded kernel (a row-major tail
// tile, unaligned operands; always 8 rows per thread, scalar accesses with 64-bit addresses)
// prefetches nothing and stages one row at a time in a rolled loop.
//
// Cache policy, reasoned and not A/B-measured: x, g, m and v are streamed once and load
// non-temporally (TileArgs::nt_load: bit 0 x, m and v, bit 1 g); y follows the round's rule
// (TileArgs::nt_store: plain below the MALL size so the next gradient launch finds it,
// non-temporal above), and m' and v' follow the same flag, as dl_track_round's d' does: below the
// MALL size the next round, one gradient launch later, reads them back.
#include <type_traits>

#include "adam_elem.h"
#include "tile_core.h"

namespace dl {
namespace {

__device__ __forceinline__ float4 adam4(float4 x, float4 g, float4 &m, float4 &v,
                                        const AdamParams &p, float ss, float bs) {
    float4 t;
    t.x = adam_elem(x.x, g.x, m.x, v.x, p, ss, bs);
    t.y = adam_elem(x.y, g.y, m.y, v.y, p, ss, bs);
    t.z = adam_elem(x.z, g.z, m.z, v.z, p, ss, bs);
    t.w = adam_elem(x.w, g.w, m.w, v.w, p, ss, bs);
    return t;
}

// rows per thread up to which g, and m and v, ride the cross-tile prefetch beside x
constexpr int kAdamPrefetchG = 4;
constexpr int kAdamPrefetchMV = 2;

// C, KV, DEV, FAST as mix_sgd_tile_kernel's (no halo rows, no row sets: every source row is an
// output row)
template <int C, int KV, bool DEV, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, kTileThreads)))
mix_adam_tile_kernel(TileArgs a, AdamTileArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *tile = reinterpret_cast<float4 *>(smem);
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;  // rows covered per pass
    constexpr int T = 4 * C;
    constexpr bool PFG = FAST && KV <= kAdamPrefetchG;    // g rides the prefetch
    constexpr bool PFS = FAST && KV <= kAdamPrefetchMV;   // m and v ride the prefetch
    // FAST: rows of the other streams per staging step (two streams at KV = 4, three at KV = 8)
    constexpr int HB = KV <= 4 ? KV : 2;
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int R = a.n_rows;
    const int64_t P = a.n_params;
    const AdamParams p = q.p;
    // once per workgroup (uniform addresses: ordinary loads)
    const float ss = adam_step_size(p);
    const float bs = adam_bias2_sqrt(p);

    // FAST-path byte offsets: lane row s / chunk c; pass k adds k * step
    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t og = (uint32_t)s * a.grs + lc;
    const uint32_t sg = (uint32_t)SLOTS * a.grs;
    uint32_t om = (uint32_t)s * q.mrs + lc;
    const uint32_t sm = (uint32_t)SLOTS * q.mrs;
    uint32_t ov = (uint32_t)s * q.vrs + lc;
    const uint32_t sv = (uint32_t)SLOTS * q.vrs;
    uint32_t oy = (uint32_t)s * a.yrs + lc;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);

    float4 px[FAST ? KV : 1], pg[PFG ? KV : 1], pm[PFS ? KV : 1], pv[PFS ? KV : 1];
    DevAcc<C, KV, DEV && dev_per_lane(C, KV)> dv;   // per-agent ||y - mean||^2
    dev_zero(dv);

    // KV rows of one stream, one straight-line loop per load policy
    auto load_rows = [&](float4 *dst, const void *ptr, int64_t ts, int tile_id, uint32_t o,
                         uint32_t st, bool nt) {
        const __amdgpu_buffer_rsrc_t r = buf_rsrc(tile_base(a, ptr, ts, tile_id));
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
    auto prefetch = [&](int tile_id) {
        if constexpr (FAST) load_rows(px, a.x, a.xts, tile_id, ox, sx, a.nt_load & 1);
        if constexpr (PFG) load_rows(pg, a.g, a.gts, tile_id, og, sg, a.nt_load & 2);
        if constexpr (PFS) {
            load_rows(pm, q.m, q.mts, tile_id, om, sm, a.nt_load & 1);
            load_rows(pv, q.v, q.vts, tile_id, ov, sv, a.nt_load & 1);
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
        asm volatile("" : "+v"(ox), "+v"(og), "+v"(om), "+v"(ov), "+v"(oy));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tw.step;
        // this tile's moments (the prefetch holds only their values) and gradients
        const __amdgpu_buffer_rsrc_t rgc = buf_rsrc(tile_base(a, a.g, a.gts, tile_id));
        const __amdgpu_buffer_rsrc_t rmc = buf_rsrc(tile_base(a, q.m, q.mts, tile_id));
        const __amdgpu_buffer_rsrc_t rvc = buf_rsrc(tile_base(a, q.v, q.vts, tile_id));
        // row s + k * SLOTS of an operand: a FAST load at byte offset o + k * st of the tile's
        // resource, or a guarded load of the row-major operand
        auto load_k = [&](__amdgpu_buffer_rsrc_t rc, uint32_t o, uint32_t st, bool nt,
                          const float *ptr, int64_t ld, int k) {
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t off = r < R ? o + (uint32_t)k * st : lc;
                return nt ? buf_ld4<kBufNT>(rc, off) : buf_ld4<0>(rc, off);
            }
            return ld4(ptr + (int64_t)(r < R ? r : 0) * ld, col0 + 4 * c, P, false);
        };
        auto load_x = [&](int k) { return load_k(rgc, 0u, 0u, false, a.x, a.ldx, k); };  // guarded
        auto load_g = [&](int k) { return load_k(rgc, og, sg, a.nt_load & 2, a.g, a.ldg, k); };
        auto load_m = [&](int k) { return load_k(rmc, om, sm, a.nt_load & 1, q.m, q.ldm, k); };
        auto load_v = [&](int k) { return load_k(rvc, ov, sv, a.nt_load & 1, q.v, q.ldv, k); };
        auto store_k = [&](__amdgpu_buffer_rsrc_t rc, uint32_t o, uint32_t st, float *ptr,
                           int64_t ld, int k, const float4 &val) {   // row s + k * SLOTS < R
            if (FAST) {
                if (a.nt_store)
                    buf_st4<kBufNT>(val, rc, o + (uint32_t)k * st);
                else
                    buf_st4<0>(val, rc, o + (uint32_t)k * st);
            } else {
                st4(ptr + (int64_t)(s + k * SLOTS) * ld, col0 + 4 * c, P, false, val);
            }
        };
        // step every source row and stage the stepped tile in LDS
        float4 cst = zero4();  // column partial sums of t (doubly stochastic W only)
        auto stage = [&](int k, float4 x, float4 g, float4 m, float4 v) {
            const int r = s + k * SLOTS;
            const float4 t = adam4(x, g, m, v, p, ss, bs);
            if (r < R) {
                store_k(rmc, om, sm, q.m, q.ldm, k, m);
                store_k(rvc, ov, sv, q.v, q.ldv, k, v);
                tile[r * C + c] = t;
                if (DEV) add4(cst, t);
            }
        };
        if constexpr (PFG && PFS) {
#pragma unroll
            for (int k = 0; k < KV; ++k) stage(k, px[k], pg[k], pm[k], pv[k]);
        } else if constexpr (FAST) {
#pragma unroll
            for (int k0 = 0; k0 < KV; k0 += HB) {
                float4 hg[PFG ? 1 : HB], hm[HB], hv[HB];
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    if (!PFG) hg[PFG ? 0 : j] = load_g(k0 + j);
                    hm[j] = load_m(k0 + j);
                    hv[j] = load_v(k0 + j);
                }
#pragma unroll
                for (int j = 0; j < HB; ++j)
                    stage(k0 + j, px[(k0 + j) % (FAST ? KV : 1)],
                          PFG ? pg[PFG ? k0 + j : 0] : hg[PFG ? 0 : j], hm[j], hv[j]);
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < KV; ++k) stage(k, load_x(k), load_g(k), load_m(k), load_v(k));
        }
        // mean(W t) = mean(t) when W is doubly stochastic: reduce the column sums of the inputs
        // under the staging barrier instead of re-mixing the tile afterwards
        bool mfi = DEV && a.mean_from_inputs;
        if (mfi) col_sums_to_scratch<C>(cst, scratch, tid);
        __syncthreads();
        // the next tile's loads go out first: they land while we mix from LDS
        if (nxt < tw.end) prefetch(nxt);
        float4 mean_t = zero4();
        if (mfi) {
            mean_t = div4(col_sums_from_scratch<C>(scratch, c), (float)R);
            // t can hold +inf and -inf where y and its mean are finite or one-signed (a diverged
            // run): a tile with a mean that is not finite takes the two-pass form, the mean
            // summed from y itself as numpy does; a tile of finite means keeps this one, bit for
            // bit (mix_track.hip: u - u is 0 for a finite u and NaN otherwise; every wave holds
            // all C columns, so the vote of one wave is the workgroup's)
            const float u = (mean_t.x + mean_t.y) + (mean_t.z + mean_t.w);
            if (__any(u - u != 0.f)) {
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
hipError_t launch_kv(const TileArgs &a, const AdamTileArgs &q, bool dev, int grid, int lds,
                     hipStream_t s) {
    return dev ? launch_lds(mix_adam_tile_kernel<C, KV, true, FAST>, grid, lds, s, a, q)
               : launch_lds(mix_adam_tile_kernel<C, KV, false, FAST>, grid, lds, s, a, q);
}

}  // namespace

hipError_t launch_mix_adam_tile(const TileArgs &a, const AdamTileArgs &q, int chunks, bool dev,
                                int grid, int lds, bool fast, hipStream_t s) {
    // no halo rows and no row sets: every staged row is a local source row and an output row
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows || a.g == nullptr || q.m == nullptr ||
        q.v == nullptr)
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
