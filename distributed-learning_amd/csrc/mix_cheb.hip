// Chebyshev-accelerated gossip round for gfx950 (MI355X): Y = a W X + b Z in one HBM pass -- the
// semi-iteration x_{k+1} = w_{k+1} W x_k + (1 - w_{k+1}) x_{k-1} with X = x_k, Z = x_{k-1}, a =
// w_{k+1}, b = 1 - w_{k+1}, which dl_mix_round + dl_axpby run as two launches through a third
// matrix.
//
// Design (path 1): as mix_sgd.hip.  Persistent 1024-thread workgroups each own
// column tiles of T = 4*C floats for all agents; the CSR is staged once per workgroup in LDS; the
// geometry (chunks, LDS offsets, grid, tiles) is the planner's for the same dl_mix_args.  Per
// tile a thread puts its rows' chunk of x in the LDS image; after the barrier every output row
// is folded from LDS in CSR order (products and sums separate fp32 operations: the reference's
// left fold, dl_mix_round's bits with g = NULL) and y = fl(fl(a acc) + fl(b z)) is written.  12 B
// per element cross HBM (read x, z; write y) against 20 B for the two launches.
//
// The element of z belongs to the thread that stages and outputs that (row, chunk): the thread
// that reads z writes y, so y may be z itself -- the engine's ping-pong then needs no third
// matrix.  y may also be x: a workgroup stages all rows of its columns before it writes them,
// and no other workgroup touches those columns.
//
// The next tile's x is in flight while the current one is mixed.  The fold needs this tile's z,
// and vmcnt retires in order, so z must have been issued before the next tile's prefetch: up to
// KV = 4 rows per thread z rides the prefetch one tile ahead (x, z of the next tile and z of the
// current one: 12*KV VGPRs); at KV = 8 only x does and the current tile's z is loaded while the
// tile is staged, in groups of four rows, and held through the fold (8*KV VGPRs).  The fold's
// passes stay a rolled loop, which cannot index registers by the pass: the FAST kernels rotate
// z's rows through the first one instead (4*KV moves a pass; unrolled passes cost a hoisted
// offset per pass and spilled with the deviation).  The guarded
// kernel (a row-major tail tile, unaligned operands; always 8 rows per thread, scalar accesses
// with 64-bit addresses) prefetches nothing and reads z in the pass that writes y.
#include <type_traits>

#include "tile_core.h"

namespace dl {
namespace {

// fl(fl(a s) + fl(b z)): three separately rounded operations (-ffp-contract=off), dl_axpby's
__device__ __forceinline__ float4 axpby4(float a, float4 s, float b, float4 z) {
    float4 y;
    y.x = a * s.x + b * z.x;
    y.y = a * s.y + b * z.y;
    y.z = a * s.z + b * z.z;
    y.w = a * s.w + b * z.w;
    return y;
}

// C, KV, DEV, FAST as mix_sgd_tile_kernel's (no halo rows, no row sets, no gradient)
template <int C, int KV, bool DEV, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, kTileThreads)))
mix_cheb_tile_kernel(TileArgs a, ChebTileArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *tile = reinterpret_cast<float4 *>(smem);
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;  // rows covered per pass
    constexpr int T = 4 * C;
    constexpr bool PFZ = FAST && KV <= 4;   // z rides the prefetch
    constexpr int HB = 4;                   // FAST, KV = 8: rows of z per load group
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int R = a.n_rows;
    const int64_t P = a.n_params;
    const float ca = q.a, cb = q.b;

    // FAST-path byte offsets: lane row s / chunk c; pass k adds k * step
    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t oz = (uint32_t)s * q.zrs + lc;
    const uint32_t sz = (uint32_t)SLOTS * q.zrs;
    uint32_t oy = (uint32_t)s * a.yrs + lc;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;
    // staged element of pass k: tile[(s + k * SLOTS) * C + c] = tile[tid + k * NT]
    uint32_t ot = (uint32_t)tid;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);

    float4 px[FAST ? KV : 1], pz[PFZ ? KV : 1];
    DevAcc<C, KV, DEV && dev_per_lane(C, KV)> dv;   // per-agent ||y - mean||^2
    dev_zero(dv);

    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;

    auto prefetch = [&](int tile_id) {
        if (FAST) {
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
            const __amdgpu_buffer_rsrc_t rz = buf_rsrc(tile_base(a, q.z, q.zts, tile_id));
            // one straight-line loop per load policy (bit 0: x and z non-temporal); x first, so
            // the staging waits on x alone
            auto loads = [&](auto ax) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = s + k * SLOTS < R;
                    px[k] = buf_ld4<decltype(ax)::value>(rx, ok ? ox + k * sx : lc);
                }
                if (PFZ) {
#pragma unroll
                    for (int k = 0; k < KV; ++k) {
                        const bool ok = s + k * SLOTS < R;
                        pz[PFZ ? k : 0] = buf_ld4<decltype(ax)::value>(rz, ok ? oz + k * sz : lc);
                    }
                }
            };
            if (a.nt_load & 1) loads(PNT{});
            else loads(PPL{});
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
        asm volatile("" : "+v"(ox), "+v"(oz), "+v"(oy), "+v"(ot));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tw.step;
        const __amdgpu_buffer_rsrc_t rzc = buf_rsrc(tile_base(a, q.z, q.zts, tile_id));
        auto load_x = [&](int k) {   // (guarded kernel)
            const int r = s + k * SLOTS;
            return ld4(a.x + (int64_t)(r < R ? r : 0) * a.ldx, col0 + 4 * c, P, false);
        };
        auto load_z = [&](int k) {   // (guarded kernel, and FAST at KV = 8)
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t o = r < R ? oz + (uint32_t)k * sz : lc;
                return (a.nt_load & 1) ? buf_ld4<kBufNT>(rzc, o) : buf_ld4<0>(rzc, o);
            }
            return ld4(q.z + (int64_t)(r < R ? r : 0) * q.ldz, col0 + 4 * c, P, false);
        };
        // mean(W x) = mean(x) when W is doubly stochastic, so mean(y) = mean(a x + b z): reduce
        // the column sums of the inputs under the staging barrier instead of re-mixing the tile
        bool mfi = DEV && a.mean_from_inputs;
        float4 cst = zero4();
        // this tile's z, held until its rows are written (FAST)
        float4 cz[FAST ? KV : 1];
        if constexpr (PFZ) {
#pragma unroll
            for (int k = 0; k < KV; ++k) cz[k] = pz[PFZ ? k : 0];
        } else if constexpr (FAST) {
#pragma unroll
            for (int k0 = 0; k0 < KV; k0 += HB)
#pragma unroll
                for (int j = 0; j < HB; ++j)
                    if (k0 + j < KV) cz[k0 + j] = load_z(k0 + j);
        }
        // stage the tile of x in LDS
        if constexpr (FAST) {
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int r = s + k * SLOTS;
                if (r < R) {
                    tile[ot + (uint32_t)k * NT] = px[k];
                    if (mfi) add4(cst, axpby4(ca, px[k], cb, cz[k]));
                }
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                const int r = s + k * SLOTS;
                const float4 x = load_x(k);
                if (r < R) {
                    tile[r * C + c] = x;
                    if (mfi) add4(cst, axpby4(ca, x, cb, load_z(k)));
                }
            }
        }
        if (mfi) col_sums_to_scratch<C>(cst, scratch, tid);
        __syncthreads();
        // the next tile's loads go out first: they land while we mix from LDS
        if (nxt < tw.end) prefetch(nxt);
        float4 mean_t = zero4();
        if (mfi) {
            mean_t = div4(col_sums_from_scratch<C>(scratch, c), (float)R);
            // a x can overflow where a (W x) does not (|x| above FLT_MAX / |a|: a diverged run),
            // and then +inf meets -inf here though y and its mean are finite.  A tile with a
            // mean that is not finite takes the two-pass form, the mean summed from y itself
            // as numpy does; a tile of finite means keeps this one, bit for bit.
            // (t - t is 0 for a finite t and NaN for inf or NaN; an inf or NaN component makes t
            // one, and four finite components whose sum overflows only take the slower form)
            // Every wave holds all C columns (lane & (C - 1), C divides 64), so the vote of one
            // wave is the workgroup's: the same in every wave, with no barrier and no LDS.
            const float t = (mean_t.x + mean_t.y) + (mean_t.z + mean_t.w);
            if (__any(t - t != 0.f)) {
                __syncthreads();   // every wave has read scratch before tile_mean rewrites it
                mfi = false;
                mean_t = zero4();
            }
        }
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(tile_base(a, a.y, a.yts, tile_id));
        auto put_y = [&](int k, int ag, const float4 &y) {
            store_y<FAST>(a, ry, oy + (uint32_t)k * sy, ag, col0 + 4 * c, y);
        };
        // The two-pass deviation (W not doubly stochastic) needs y twice.  FAST: z is in
        // registers, y is written in the first pass and recomputed in the second.  Guarded: z is
        // read from memory and y may be z itself, so the first pass only sums and the second
        // writes.
        const bool two = DEV && !mfi;
        float4 ms = mean_t;   // mfi: the tile's column mean; two: the column sums of y (from 0)
        // one output pass: `first` the pass under the prefetch, else the two-pass form's second
        auto pass = [&](int k, float4 z, bool first) {
            const int ag = s + k * SLOTS;
            if (ag < R) {
                const float4 y = axpby4(ca, csr_fold<C>(L, tile, ag, c), cb, z);
                if (first) {
                    if (FAST || !two) put_y(k, ag, y);
                    if (mfi) dev_add(dv, k, y, ms, c);
                    if (two) add4(ms, y);
                } else {
                    if (!FAST) put_y(k, ag, y);
                    dev_add(dv, k, y, ms, c);
                }
            }
        };
        // passes stay rolled: interleaving them would hold KV accumulators at once on top of the
        // prefetch registers.  FAST: the pass's z is cz[0] and the rows rotate by one after it (a
        // rolled loop cannot index registers), so KV passes leave cz as they found it.
        auto rotate = [&]() {
            const float4 z0 = cz[0];
#pragma unroll
            for (int j = 0; j + 1 < (FAST ? KV : 1); ++j) cz[j] = cz[j + 1];
            cz[(FAST ? KV : 1) - 1] = z0;
        };
#pragma unroll 1
        for (int k = 0; k < KV; ++k) {
            pass(k, FAST ? cz[0] : load_z(k), true);
            if (FAST) rotate();
        }
        if (mfi && a.mean != nullptr && s == 0) st4(a.mean, col0 + 4 * c, P, FAST, ms);
        if (two) {
            ms = tile_mean<C>(ms, scratch, tid, c, R);
            if (a.mean != nullptr && s == 0) st4(a.mean, col0 + 4 * c, P, FAST, ms);
            // second LDS pass: recompute y (same order, same bits) instead of holding it
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                pass(k, FAST ? cz[0] : load_z(k), false);
                if (FAST) rotate();
            }
        }
        __syncthreads();  // tile and scratch are rewritten by the next iteration
    }
    if (DEV) dev_epilogue(dv, a, tid, R);
}

template <int C, int KV, bool FAST>
hipError_t launch_kv(const TileArgs &a, const ChebTileArgs &q, bool dev, int grid, int lds,
                     hipStream_t s) {
    return dev ? launch_lds(mix_cheb_tile_kernel<C, KV, true, FAST>, grid, lds, s, a, q)
               : launch_lds(mix_cheb_tile_kernel<C, KV, false, FAST>, grid, lds, s, a, q);
}

}  // namespace

hipError_t launch_mix_cheb_tile(const TileArgs &a, const ChebTileArgs &q, int chunks, bool dev,
                                int grid, int lds, bool fast, hipStream_t s) {
    // no halo rows, no row sets, no gradient: every staged row is a local source row and an
    // output row
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows || a.g != nullptr || q.z == nullptr)
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
