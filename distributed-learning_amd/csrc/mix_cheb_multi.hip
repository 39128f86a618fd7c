// K Chebyshev-accelerated gossip rounds in one HBM pass (gfx950): u_{r+1} = a_r W u_r + b_r
// u_{r-1} for r = 0..K-1 with u_0 = X, u_{-1} = Z, on LDS-resident column tiles.
//
// mix_cheb.hip runs the recurrence one round a launch (12 B per element per round across HBM);
// mix_multi.hip keeps a column tile of all agents in LDS for K plain rounds (8 B per element per K
// rounds).  The recurrence is column-independent as the plain mix is and needs exactly the two
// tile images mix_multi.hip ping-pongs, so this kernel takes mix_multi.hip's geometry (persistent
// 1024-thread workgroups, a column tile of ALL agents, two images, the CSR in LDS or in
// registers, FAST tiles only) and moves 16 B per element per K rounds: x and z in, y = u_K and
// z_out = u_{K-1} out.
//
// Data movement.  Staging writes u_0 to image A and u_{-1} to image B.  Round r folds every row
// from the image that holds u_r (the CSR-order left fold of dl_mix_round, products and sums
// separate fp32 operations), and the thread that owns (row, chunk) combines the fold with ITS OWN
// element of the other image -- u_{r-1}, which no other thread reads any more -- and writes the
// result over it: y = fl(fl(a acc) + fl(b old)), dl_axpby's three roundings.  Then the images swap
// roles: one barrier a round, as the plain pass.  With the CSR in registers (RE = 5: degree-4
// regular graphs with shared weights) a thread also keeps its own elements of u_r (own[k]: the
// fold's self operand, as mix_multi.hip) and, where the registers allow, of u_{r-1} (old[k]), so a
// round reads only the four neighbours from LDS and rotates new -> own -> old in registers; the
// LDS-CSR form reads its own element of the older image from LDS (contiguous, conflict-free).
// The last round stores y from registers and z_out from own[k] (or from the current image).
//
// x and z of the next tile are prefetched in registers while the current tile's rounds run
// (buffer loads, the rounds' non-temporal policy), in mix_multi.hip's rotated tile loop, so the
// image fill waits on loads only.  Where that does not fit beside the rotating registers
// (prefetch_z below, decided from the compiler's resource report: no instantiation may use
// scratch) z is loaded while the tile is staged instead.  A call without z (the first pass of a
// run: round 0 is the plain fold) is handed x in z's place by the host, so the loads -- and the
// wait counts -- are the same; image B and old[k] are then not read before they are rewritten.
//
// Any of y, z_out may be x or z themselves: a workgroup has staged all rows of its columns before
// it writes any of them, and no other workgroup touches those columns.
//
// Deviation (OUT 1) and per-round trace (OUT 2), for a doubly stochastic W: the column means m_0,
// m_{-1} of the two staged images are reduced under the staging barrier, and m_{r+1} = fl(fl(a_r
// m_r) + fl(b_r m_{r-1})) follows the iterates in registers (mean(W u) = mean(u) whatever a and b
// are).  Each lane accumulates its own chunk's squared distance per row -- and per round in the
// traced form, whose round loop is unrolled so the round indexes registers -- and the C lanes of a
// row are summed once, after the last tile.
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

// The register choices per instantiation, from `make resource RES_SRC=mix_cheb_multi.hip`
// (profiles/r30/cheb_rounds/vgprs.txt): 128 VGPRs a thread at 1024 threads.
// old[k] in registers (8 x KV VGPRs with own[k]): the register CSR only.  Beside the traced
// form's KV x kChebTraceRounds partial sums it is dropped first.
constexpr bool old_in_regs(int KV, int OUT, int RE) { return RE > 0 && KV <= 2 && OUT < 2; }
// z rides the prefetch one tile ahead (4 x KV VGPRs more); else it is loaded at staging
constexpr bool prefetch_z(int KV, int OUT, int RE) {
    return KV <= 2 || (KV <= 4 && OUT < 2 && RE == 0);
}
// The traced register-CSR form at 4 rows per thread keeps 32 partial sums and 20 neighbour
// offsets and is built guarded only (traced_full); it, the guarded register-CSR form at 4 rows
// (the ragged guards' registers) and every form at 8 rows give up own[k] too (the self operand
// and z_out from LDS) and load x at staging like z (no prefetch).
constexpr bool traced_full(int KV, int OUT, int RE) { return !(RE > 0 && KV > 2 && OUT == 2); }
constexpr bool lean(int KV, int OUT, int RE, int MODE) {
    return KV > 4 || (RE > 0 && KV > 2 && (OUT == 2 || MODE == 0));
}

// C: float4 chunks per tile row; KV: rows per thread (agents s + k * SLOTS); OUT: 1 the final
// deviation (its partial rows written when a.dev_partial is given: a call without deviation
// outputs runs this kernel too, the column sums and the last round's distances being a few
// operations a tile), 2 the per-round trace (rounds <= kChebTraceRounds; the final deviation too
// when q.dev_final); RE, MODE: as mix_multi_kernel's (register CSR of RE entries a row; 1 / 2:
// every slot an agent, unguarded, plain / non-temporal stores; 0: guarded, store kind at run time)
template <int C, int KV, int OUT, int RE, int MODE>
__global__ void __launch_bounds__(kTileThreads)
mix_cheb_multi_kernel(TileArgs a, ChebMultiArgs q, int rounds) {
    static_assert(OUT == 1 || OUT == 2, "the column means are formed in every instantiation");
    constexpr bool FULL = MODE > 0;
    constexpr bool OLD = old_in_regs(KV, OUT, RE);
    constexpr bool PFZ = prefetch_z(KV, OUT, RE);
    constexpr bool PFX = !lean(KV, OUT, RE, MODE);   // x rides the prefetch
    constexpr bool OWN = RE > 0 && PFX;        // own[k] in registers
    constexpr int KR = OUT == 2 ? kChebTraceRounds : 1;
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int Nr = a.n_rows;
    float4 *img0 = reinterpret_cast<float4 *>(smem);
    float4 *img1 = img0 + (size_t)Nr * C;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);
    float4 *scratch2 = reinterpret_cast<float4 *>(smem + q.scratch2_off);
    const LdsCsr L = lds_csr(smem, a, false);
    if constexpr (RE == 0) stage_csr(L, a, tid);   // RE > 0 keeps its CSR in registers

    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t oz = (uint32_t)s * q.zrs + lc;
    const uint32_t sz = (uint32_t)SLOTS * q.zrs;
    uint32_t oy = (uint32_t)s * a.yrs + lc;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;
    uint32_t oo = (uint32_t)s * q.zors + lc;
    const uint32_t so = (uint32_t)SLOTS * q.zors;

    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;
    const bool ntl = (a.nt_load & 1) != 0;

    // ragged slots re-read row 0 (an L1 hit), so every thread issues the same loads
    float4 px[PFX ? KV : 1], pz[PFZ ? KV : 1];
    auto prefetch = [&](int tile_id) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
        const __amdgpu_buffer_rsrc_t rz = buf_rsrc(tile_base(a, q.z, q.zts, tile_id));
        auto loads = [&](auto ax) {
            if constexpr (PFX) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = FULL || s + k * SLOTS < Nr;
                    px[k] = buf_ld4<decltype(ax)::value>(rx, ok ? ox + k * sx : lc);
                }
            }
            if constexpr (PFZ) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = FULL || s + k * SLOTS < Nr;
                    pz[k] = buf_ld4<decltype(ax)::value>(rz, ok ? oz + k * sz : lc);
                }
            }
        };
        if (ntl) loads(PNT{});
        else loads(PPL{});
    };

    // register-cached CSR (RE > 0): byte offset of each neighbour's chunk c inside an image
    uint32_t coff[KV][RE > 0 ? RE : 1];
    float wreg[RE > 0 ? RE : 1];
    bool self_ok = true;   // every row of this thread lists itself first (the diagonal of W)
    if constexpr (RE > 0) {
#pragma unroll
        for (int e = 0; e < RE; ++e) wreg[e] = a.w[e];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int ag = FULL || s + k * SLOTS < Nr ? s + k * SLOTS : 0;
            self_ok = self_ok && a.col[ag * RE] == ag;
#pragma unroll
            for (int e = 0; e < RE; ++e)
                coff[k][e] = ((uint32_t)a.col[ag * RE + e] * C + c) * 16u;
        }
    }
    // the fold's self operand from own[k] instead of LDS, decided per wave (mix_multi.hip)
    const bool self0 = OWN && __all(self_ok ? 1 : 0) != 0;
    float4 own[OWN ? KV : 1], old[OLD ? KV : 1];
#pragma unroll
    for (int k = 0; k < (OWN ? KV : 1); ++k) own[k] = zero4();
#pragma unroll
    for (int k = 0; k < (OLD ? KV : 1); ++k) old[k] = zero4();

    auto fold_reg = [&](const float4 *src, int k) __attribute__((always_inline)) {
        const char *base = reinterpret_cast<const char *>(src);
        float4 acc = zero4();
#pragma unroll
        for (int e = 0; e < (RE > 0 ? RE : 1); ++e) {
            float4 v;
            if (e == 0 && self0)   // wave-uniform: the skipped read is not issued
                v = own[OWN ? k : 0];
            else
                v = *reinterpret_cast<const float4 *>(base + coff[k][e]);
            axpy4(acc, wreg[e], v);
        }
        return acc;
    };
    auto fold = [&](const float4 *src, int k, int ag) __attribute__((always_inline)) {
        if constexpr (RE > 0) return fold_reg(src, k);
        return csr_fold<C>(L, src, ag, c);
    };

    // per-lane partial ||u_a - m||^2 of this thread's rows, per traced round (OUT 1: the last)
    float dacc[KV][KR];
#pragma unroll
    for (int k = 0; k < KV; ++k)
#pragma unroll
        for (int r = 0; r < KR; ++r) dacc[k][r] = 0.f;

    // column means of the current and the previous iterate (this thread's chunk)
    float4 mcur = zero4(), mprev = zero4();
    const int last = a.n_tiles - 1;
    auto stage = [&](int tile_id) __attribute__((always_inline)) {
        float4 cx = zero4(), cz = zero4();
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
        const __amdgpu_buffer_rsrc_t rz = buf_rsrc(tile_base(a, q.z, q.zts, tile_id));
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int r = s + k * SLOTS;
            const bool ok = FULL || r < Nr;
            float4 u;
            if constexpr (PFZ) {
                u = pz[k];
            } else {
                const uint32_t o = ok ? oz + (uint32_t)k * sz : lc;
                u = ntl ? buf_ld4<kBufNT>(rz, o) : buf_ld4<0>(rz, o);
            }
            float4 t;
            if constexpr (PFX) {
                t = px[k];
            } else {
                const uint32_t o = ok ? ox + (uint32_t)k * sx : lc;
                t = ntl ? buf_ld4<kBufNT>(rx, o) : buf_ld4<0>(rx, o);
            }
            if (OWN) own[OWN ? k : 0] = t;
            if (OLD) old[OLD ? k : 0] = u;
            if (ok) {
                img0[r * C + c] = t;
                img1[r * C + c] = u;
                add4(cx, t);
                add4(cz, u);
            }
        }
        col_sums_to_scratch<C>(cx, scratch, tid);
        col_sums_to_scratch<C>(cz, scratch2, tid);
        __syncthreads();
        float4 sx4 = zero4(), sz4 = zero4();
#pragma unroll 2   // (fully unrolled, the reads are hoisted: 128 VGPRs at once)
        for (int wv = 0; wv < NT / 64; ++wv) {
            add4(sx4, scratch[wv * C + c]);
            add4(sz4, scratch2[wv * C + c]);
        }
        mcur = div4(sx4, (float)Nr);
        mprev = div4(sz4, (float)Nr);
    };

    int tile_id = blockIdx.x;
    if (tile_id < a.n_tiles) {
        prefetch(tile_id);
        stage(tile_id);
        prefetch(min(tile_id + (int)gridDim.x, last));
    }
    for (; tile_id < a.n_tiles; tile_id += gridDim.x) {
        asm volatile("" : "+v"(ox), "+v"(oz), "+v"(oy), "+v"(oo));
        const int nxt = min(tile_id + (int)gridDim.x, last);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(tile_base(a, a.y, a.yts, tile_id));
        const __amdgpu_buffer_rsrc_t ro =
            buf_rsrc(tile_base(a, q.z_out ? q.z_out : a.y, q.z_out ? q.zots : a.yts, tile_id));
        const bool nts = MODE == 2 || (MODE == 0 && a.nt_store);
        // round r: src holds u_r, dst holds u_{r-1} and receives u_{r+1}; fin: the last round,
        // which writes HBM instead; dk: this round's partial sums
        auto round = [&](int r, bool fin, const float4 *src, float4 *dst, auto &&dk) __attribute__((always_inline)) {
            const bool plain = q.plain0 && r == 0;
            float ca = 1.f, cb = 0.f;
            if (!plain) {
                ca = q.coef[2 * r];
                cb = q.coef[2 * r + 1];
            }
            float4 mnew = mcur;
            if (!plain) mnew = axpby4(ca, mcur, cb, mprev);
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int ag = s + k * SLOTS;
                if (FULL || ag < Nr) {
                    const uint32_t idx = (uint32_t)ag * C + c;
                    float4 nw = fold(src, k, ag);
                    if (!plain) nw = axpby4(ca, nw, cb, OLD ? old[OLD ? k : 0] : dst[idx]);
                    if (!fin) {
                        dst[idx] = nw;
                    } else {
                        if (nts) buf_st4<kBufNT>(nw, ry, oy + (uint32_t)k * sy);
                        else buf_st4<0>(nw, ry, oy + (uint32_t)k * sy);
                        if (q.z_out != nullptr) {
                            const float4 prev = OWN ? own[OWN ? k : 0] : src[idx];
                            if (nts) buf_st4<kBufNT>(prev, ro, oo + (uint32_t)k * so);
                            else buf_st4<0>(prev, ro, oo + (uint32_t)k * so);
                        }
                    }
                    if (OUT == 2 || fin) {
                        const float dx = nw.x - mnew.x, dy = nw.y - mnew.y;
                        const float dz = nw.z - mnew.z, dw = nw.w - mnew.w;
                        dk(k) += (dx * dx + dy * dy) + (dz * dz + dw * dw);
                    }
                    if (OLD) old[OLD ? k : 0] = own[OWN ? k : 0];
                    if (OWN) own[OWN ? k : 0] = nw;
                }
                // one output row at a time (register pressure at 1024 threads, mix_multi.hip)
                __builtin_amdgcn_sched_barrier(0);
            }
            mprev = mcur;
            mcur = mnew;
        };
        const float4 *src = img0;
        float4 *dst = img1;
        if constexpr (OUT == 2) {
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                if (r < rounds) {
                    round(r, r + 1 == rounds, src, dst, [&](int k) -> float & { return dacc[k][r]; });
                    if (r + 1 < rounds) __syncthreads();
                    const float4 *t = src;
                    src = dst;
                    dst = const_cast<float4 *>(t);
                }
            }
        } else {
            for (int r = 0; r < rounds; ++r) {
                round(r, r + 1 == rounds, src, dst,
                      [&](int k) -> float & { return dacc[k][0]; });
                if (r + 1 < rounds) __syncthreads();
                const float4 *t = src;
                src = dst;
                dst = const_cast<float4 *>(t);
            }
        }
        if (a.mean != nullptr && s == 0)
            st4(a.mean, a.col_base + (int64_t)tile_id * 4 * C + 4 * c, a.n_params, true, mcur);
        __syncthreads();   // both images and the scratches are rewritten by the next tile
        stage(nxt);        // (past the end: a re-read of the last tile, then unused)
        prefetch(min(nxt + (int)gridDim.x, last));   // lands while the next tile's rounds run
    }
    {
        // the C lanes of a row group summed once; lane 0 writes the workgroup's partial rows:
        // the trace's [grid][rounds][N] and / or the final deviation's [grid][N]
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const float v = row_group_sum<C>(dacc[k][r]);
                if (c != 0 || !(FULL || ag < Nr)) continue;
                if (OUT == 2) {
                    if (r < rounds)
                        a.dev_partial[((int64_t)blockIdx.x * rounds + r) * Nr + ag] = v;
                    if (r + 1 == rounds && q.dev_final != nullptr)
                        q.dev_final[(int64_t)blockIdx.x * Nr + ag] = v;
                } else if (a.dev_partial != nullptr) {
                    a.dev_partial[(int64_t)blockIdx.x * Nr + ag] = v;
                }
            }
        }
        if (a.dev_max_zero != nullptr && blockIdx.x == 0 && tid == 0) *a.dev_max_zero = 0u;
    }
}

template <int C, int KV, int OUT, int RE, int MODE>
hipError_t launch_mode(const TileArgs &a, const ChebMultiArgs &q, int rounds, int grid, int lds,
                       hipStream_t s) {
    return launch_lds(mix_cheb_multi_kernel<C, KV, OUT, RE, MODE>, grid, lds, s, a, q, rounds);
}

template <int C, int KV, int OUT, int RE>
hipError_t launch_one(const TileArgs &a, const ChebMultiArgs &q, int rounds, int grid, int lds,
                      hipStream_t s) {
    // the unguarded variant for the register-CSR graphs whose N fills every slot (c2, c4)
    if constexpr (RE > 0 && traced_full(KV, OUT, RE)) {
        if (a.n_rows == KV * (kTileThreads / C))
            return a.nt_store ? launch_mode<C, KV, OUT, RE, 2>(a, q, rounds, grid, lds, s)
                              : launch_mode<C, KV, OUT, RE, 1>(a, q, rounds, grid, lds, s);
    }
    return launch_mode<C, KV, OUT, RE, 0>(a, q, rounds, grid, lds, s);
}

template <int C, int KV, int OUT>
hipError_t launch_re(const TileArgs &a, const ChebMultiArgs &q, int rounds, int grid, int lds,
                     hipStream_t s) {
    // the same test as csr_in_registers() on the host, which then reserves no LDS for the CSR
    if constexpr (KV <= 4) {
        if (a.regular == 5 && a.n_w == 5)
            return launch_one<C, KV, OUT, 5>(a, q, rounds, grid, lds, s);
    }
    return launch_one<C, KV, OUT, 0>(a, q, rounds, grid, lds, s);
}

template <int C, int KV>
hipError_t launch_kv(const TileArgs &a, const ChebMultiArgs &q, int rounds, int out, int grid,
                     int lds, hipStream_t s) {
    if (out < 2) return launch_re<C, KV, 1>(a, q, rounds, grid, lds, s);
    // the traced form keeps KV x kChebTraceRounds sums: up to cheb_trace_max_kv rows a thread
    if constexpr (KV <= kChebTraceMaxKv) return launch_re<C, KV, 2>(a, q, rounds, grid, lds, s);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_mix_cheb_multi(const TileArgs &a, const ChebMultiArgs &q, int chunks, int rounds,
                                 int out, int grid, int lds, hipStream_t s) {
    if (rounds < 1 || out < 0 || out > 2 || (out == 2 && rounds > kChebTraceRounds) ||
        q.z == nullptr || (q.coef == nullptr && !(q.plain0 && rounds == 1)) ||
        a.n_src != a.n_rows || a.n_loc != a.n_rows || a.g != nullptr)
        return hipErrorInvalidValue;
    hipError_t e = with_chunks(chunks, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        return with_passes(tile_passes(C, a.n_rows, true), [&](auto kv) {
            return launch_kv<C, decltype(kv)::value>(a, q, rounds, out, grid, lds, s);
        });
    });
    if (e != hipSuccess || out != 2) return e;
    return launch_trace_reduce(a.dev_partial, grid, rounds, a.n_rows, q.trace, s);
}

}  // namespace dl
