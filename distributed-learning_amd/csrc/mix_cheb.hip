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

#include "dl_internal.h"
#include "tile_ops.h"

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
    const int nnz = a.nnz;
    const float ca = q.a, cb = q.b;

    float *lw = reinterpret_cast<float *>(smem + a.csr_off);
    uint16_t *lcol = reinterpret_cast<uint16_t *>(smem + a.csr_off + 4u * (uint32_t)a.n_w);
    uint16_t *lrp = lcol + nnz;
    const int reg = a.regular;

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
    // byte address of tile t's first element (row 0) in x / z / y
    auto tile_base = [&](const void *ptr, int64_t ts, int tile_id) {
        return reinterpret_cast<const char *>(ptr) + (a.tiled ? 0 : a.col_base * 4) +
               (int64_t)tile_id * ts;
    };
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);

    float4 px[FAST ? KV : 1], pz[PFZ ? KV : 1];
    // per-agent ||y - mean||^2 accumulators, as mix_tile_kernel keeps them
    constexpr int ND = KV <= C ? 1 : KV / C;
    float dacc[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) dacc[k] = 0.f;
    constexpr bool LD = DEV && C > 1 && KV <= 4;
    float ldev[LD ? KV : 1];
#pragma unroll
    for (int k = 0; k < (LD ? KV : 1); ++k) ldev[k] = 0.f;

    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;

    auto prefetch = [&](int tile_id) {
        if (FAST) {
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a.x, a.xts, tile_id));
            const __amdgpu_buffer_rsrc_t rz = buf_rsrc(tile_base(q.z, q.zts, tile_id));
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

    // acc_a = sum_e w_e * x_{col_e} for agent ag, chunk c: left fold in CSR order from +0.0
    // (mixer.py:47); reads only LDS.  reg5: mix_tile_kernel's form for regular rows of 5 entries
    // sharing one weight sequence (the same products and sums in the same order).
    const bool wshared = a.n_w != nnz;
    const bool reg5 = KV <= 4 && reg == 5 && wshared;
    float w5[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) w5[e] = reg5 ? a.w[e] : 0.f;
    auto mix_row = [&](int ag) {
        if (reg5) {
            uint32_t ci[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) ci[e] = lcol[ag * 5 + e];
            float4 v[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) v[e] = tile[ci[e] * C + c];
            float4 acc = zero4();
#pragma unroll
            for (int e = 0; e < 5; ++e) axpy4(acc, w5[e], v[e]);
            return acc;
        }
        int e0, e1;
        if (reg) {
            e0 = ag * reg;
            e1 = e0 + reg;
        } else {
            e0 = lrp[ag];
            e1 = lrp[ag + 1];
        }
        const float *wr = wshared ? lw - e0 : lw;
        float4 acc = zero4();
        for (int e = e0; e < e1; ++e) axpy4(acc, wr[e], tile[lcol[e] * C + c]);
        return acc;
    };

    // column mean of the tile over all agents from per-thread partial sums (mix_tile_kernel's)
    auto tile_mean = [&](float4 cs) {
#pragma unroll
        for (int m = C; m < 64; m <<= 1) cs = shfl_xor4(cs, m);
        const int wave = tid >> 6, lane = tid & 63;
        if (lane < C) scratch[wave * C + lane] = cs;
        __syncthreads();
        float4 mean = zero4();
#pragma unroll
        for (int wv = 0; wv < NT / 64; ++wv) add4(mean, scratch[wv * C + c]);
        const float n = (float)R;
        mean.x = mean.x / n;
        mean.y = mean.y / n;
        mean.z = mean.z / n;
        mean.w = mean.w / n;
        return mean;
    };

    auto dev_add = [&](int k, float4 y, float4 mean) {  // k may be a runtime pass index
        const float dx = y.x - mean.x, dy = y.y - mean.y;
        const float dz = y.z - mean.z, dw = y.w - mean.w;
        float v = (dx * dx + dy * dy) + (dz * dz + dw * dw);
        if constexpr (LD) {
#pragma unroll
            for (int j = 0; j < KV; ++j) ldev[j] += j == k ? v : 0.f;
            return;
        }
#pragma unroll
        for (int m = 1; m < C; m <<= 1) v = xor_add(v, m);  // sum over the row group
        const bool mine = (k % C) == c;
#pragma unroll
        for (int j = 0; j < ND; ++j) dacc[j] += (mine && j == k / C) ? v : 0.f;
    };

    const int trun = a.tile_run;
    int tile_id = trun ? (int)blockIdx.x * trun : (int)blockIdx.x;
    const int tile_end = trun ? min(tile_id + trun, a.n_tiles) : a.n_tiles;
    const int tstep = trun ? 1 : (int)gridDim.x;
    if (tile_id < tile_end) prefetch(tile_id);
    // the LDS CSR is staged behind the first tile's loads; the first staging barrier publishes it
    for (int i = tid; i < a.n_w; i += NT) lw[i] = a.w[i];
    for (int i = tid; i < nnz; i += NT) lcol[i] = (uint16_t)a.col[i];
    if (!a.regular)
        for (int i = tid; i <= R; i += NT) lrp[i] = (uint16_t)a.rowptr[i];
    for (; tile_id < tile_end; tile_id += tstep) {
        // opaque per tile: keeps LICM from hoisting one offset register per pass
        asm volatile("" : "+v"(ox), "+v"(oz), "+v"(oy), "+v"(ot));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tstep;
        const __amdgpu_buffer_rsrc_t rzc = buf_rsrc(tile_base(q.z, q.zts, tile_id));
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
        if (mfi) {
#pragma unroll
            for (int m = C; m < 64; m <<= 1) cst = shfl_xor4(cst, m);
            if ((tid & 63) < C) scratch[(tid >> 6) * C + (tid & 63)] = cst;
        }
        __syncthreads();
        // the next tile's loads go out first: they land while we mix from LDS
        if (nxt < tile_end) prefetch(nxt);
        float4 mean_t = zero4();
        if (mfi) {
#pragma unroll
            for (int wv = 0; wv < NT / 64; ++wv) add4(mean_t, scratch[wv * C + c]);
            const float n = (float)R;
            mean_t.x = mean_t.x / n;
            mean_t.y = mean_t.y / n;
            mean_t.z = mean_t.z / n;
            mean_t.w = mean_t.w / n;
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
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(tile_base(a.y, a.yts, tile_id));
        auto store_y = [&](int k, int ag, const float4 &y) {
            if (FAST) {
                if (a.nt_store)
                    buf_st4<kBufNT>(y, ry, oy + (uint32_t)k * sy);
                else
                    buf_st4<0>(y, ry, oy + (uint32_t)k * sy);
            } else {
                st4(a.y + (int64_t)ag * a.ldy, col0 + 4 * c, P, false, y);
            }
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
                const float4 y = axpby4(ca, mix_row(ag), cb, z);
                if (first) {
                    if (FAST || !two) store_y(k, ag, y);
                    if (mfi) dev_add(k, y, ms);
                    if (two) add4(ms, y);
                } else {
                    if (!FAST) store_y(k, ag, y);
                    dev_add(k, y, ms);
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
            ms = tile_mean(ms);
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
    if (LD) {
#pragma unroll
        for (int k = 0; k < (LD ? KV : 1); ++k) {
            float v = ldev[k];
#pragma unroll
            for (int m = 1; m < C; m <<= 1) v = xor_add(v, m);   // over the row group
            const int ag = s + k * SLOTS;
            if (c == 0 && ag < R) a.dev_partial[(int64_t)blockIdx.x * R + ag] = v;
        }
        if (a.dev_max_zero != nullptr && blockIdx.x == 0 && tid == 0) *a.dev_max_zero = 0u;
    } else if (DEV) {
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const int k = j * C + c;  // the pass this lane's slot j holds
            const int ag = s + k * SLOTS;
            if (k < KV && ag < R) a.dev_partial[(int64_t)blockIdx.x * R + ag] = dacc[j];
        }
        if (a.dev_max_zero != nullptr && blockIdx.x == 0 && tid == 0) *a.dev_max_zero = 0u;
    }
}

template <int C, int KV, bool FAST>
hipError_t launch_kv(const TileArgs &a, const ChebTileArgs &q, bool dev, int grid, int lds,
                     hipStream_t s) {
    return dev ? launch_lds(mix_cheb_tile_kernel<C, KV, true, FAST>, grid, lds, s, a, q)
               : launch_lds(mix_cheb_tile_kernel<C, KV, false, FAST>, grid, lds, s, a, q);
}

// FAST kernels: every C x KV in {2, 4, 8}; guarded kernels: every C, KV = 8 (plan.h tile_passes)
template <int C>
hipError_t launch_c(const TileArgs &a, const ChebTileArgs &q, bool dev, int grid, int lds,
                    bool fast, hipStream_t s) {
    if (!fast) return launch_kv<C, kRowsPerThread, false>(a, q, dev, grid, lds, s);
    switch (tile_passes(C, a.n_src, true)) {
        case 2: return launch_kv<C, 2, true>(a, q, dev, grid, lds, s);
        case 4: return launch_kv<C, 4, true>(a, q, dev, grid, lds, s);
        default: return launch_kv<C, 8, true>(a, q, dev, grid, lds, s);
    }
}

}  // namespace

hipError_t launch_mix_cheb_tile(const TileArgs &a, const ChebTileArgs &q, int chunks, bool dev,
                                int grid, int lds, bool fast, hipStream_t s) {
    // no halo rows, no row sets, no gradient: every staged row is a local source row and an
    // output row
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows || a.g != nullptr || q.z == nullptr)
        return hipErrorInvalidValue;
    switch (chunks) {
        case 1: return launch_c<1>(a, q, dev, grid, lds, fast, s);
        case 2: return launch_c<2>(a, q, dev, grid, lds, fast, s);
        case 4: return launch_c<4>(a, q, dev, grid, lds, fast, s);
        case 8: return launch_c<8>(a, q, dev, grid, lds, fast, s);
        case 16: return launch_c<16>(a, q, dev, grid, lds, fast, s);
        case 32: return launch_c<32>(a, q, dev, grid, lds, fast, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dl
