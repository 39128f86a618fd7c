// K gossip rounds over failing links in one HBM pass (gfx950): X <- W_t (X - lr G) for the rounds
// t = t0 .. t0 + K - 1, W_t the fixed W with round t's failed links removed and their weight
// returned to the diagonal (include/dlamd.h dl_drop_rounds: the rule, bit for bit).
//
// Geometry.  mix_multi.hip's: a persistent 1024-thread workgroup holds a column tile of ALL agents
// in LDS, two images ping-pong (one barrier a round), the last round goes to HBM from registers,
// the next tile's rows are prefetched into registers while the current tile's rounds run, and the
// final deviation is taken against the staged tile's column mean (the mask is symmetric, so a
// symmetric doubly stochastic W stays doubly stochastic).  Thread (s, c) owns chunk c (one float4)
// of the rows s + k * SLOTS, k < KV; the C lanes of a row are contiguous lanes of one wave.
//
// Moving the mask.  Whether a link is up depends on (seed, round, link) only -- not on the column
// -- so hashing every entry in all C lanes of a row would spend C times the work, and one hash
// (two fmix rounds: four 32-bit multiplies) costs about what a whole 5-entry fold of one float4
// does.  Instead lane c of the row hashes entry c (then c + C, ...: ceil(len / C) hashes a lane a
// row a round), and ONE wave ballot hands every lane of the row the bit field of all its entries:
// the row's C bits sit at the row group's lane offset in the 64-bit ballot.  No LDS, no barrier
// and no state between rounds, so the kernel keeps mix_multi's one barrier a round, and the c4
// shape (4096 agents: two images leave 32 KiB, less than its CSR) is served.  At C = 1 there is
// nothing to share: the lane hashes its row's entries itself.  The per-round part of the hash is
// uniform (scalar registers); the row's diagonal entry is never hashed for the link draw.  With
// thr_node != 0 (a uniform branch) an entry's lane also draws both ends' node hashes.
//
// The fold.  wd = w[e0] plus, in CSR order, the weight of every down entry; acc = +0.0 + wd x_i,
// then + w[e] x_col[e] for every up entry: separate fp32 products and sums.  A down entry's term
// is formed and dropped by a select (no divergent branch), which is a skip: its operand -- Inf
// and NaN included -- never reaches acc.  With no link down these are dl_mix_round's operations
// in its order.
//
// Two forms, as mix_multi.hip: the CSR staged in LDS (any graph whose CSR fits beside the images;
// rows of any length: the down bits of a row's first 64 entries are kept, those beyond are drawn
// again by the fold), and RE = 5 (degree-4 regular graphs with shared weights: c2, c4) with the
// neighbours' LDS offsets and the five weights in registers.  One guarded instantiation each
// (ragged rows, store kind at run time): mix_multi.hip's unguarded MODE 1 / 2 copies and its
// own-operand register are an optimisation left out.  The deviation is a run-time (uniform)
// choice, the local step a template one (it costs the prefetch 4 KV registers).
#include <type_traits>

#include "link_hash.h"
#include "tile_core.h"

namespace dl {
namespace {

__device__ __forceinline__ const float4 *md_at(const void *base, uint32_t off) {
    return reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(base) + off);
}

// the C bits of this lane's row group in a wave ballot (gsh: the group's first lane)
template <int C>
__device__ __forceinline__ uint32_t group_bits(bool down, int gsh) {
    if constexpr (C == 1) return down ? 1u : 0u;   // one lane a row: nothing to share
    const uint64_t b = __ballot(down ? 1 : 0);
    constexpr uint32_t m = C >= 32 ? 0xffffffffu : (1u << C) - 1u;
    return (uint32_t)(b >> gsh) & m;
}

// acc + w v where the entry is up, acc where it is down
__device__ __forceinline__ void axpy4_up(float4 &acc, float w, float4 v, bool down) {
    float4 t = acc;
    axpy4(t, w, v);
    acc.x = down ? acc.x : t.x;
    acc.y = down ? acc.y : t.y;
    acc.z = down ? acc.z : t.z;
    acc.w = down ? acc.w : t.w;
}

// The round's mask parameters: the round key (uniform) and the two thresholds.
struct DropKey {
    uint32_t key, thr_edge, thr_node;
};

// Row ag of round k from the LDS-staged CSR: lane c draws entries c, c + C, ... of the row.
template <int C>
__device__ __forceinline__ float4 drop_fold_csr(const LdsCsr &L, const float4 *src, int ag, int c,
                                                int gsh, const DropKey &k) {
    int e0, e1;
    if (L.reg) {
        e0 = ag * L.reg;
        e1 = e0 + L.reg;
    } else {
        e0 = L.lrp[ag];
        e1 = L.lrp[ag + 1];
    }
    const int len = e1 - e0;
    const float *wr = (L.wshared ? L.lw : L.lw + e0);   // wr[e]: weight of the row's entry e
    const uint16_t *cr = L.lcol + e0;
    // down bits of entries [b, b + C): entry 0 is the row's self entry, never down
    auto draw = [&](int b) __attribute__((always_inline)) {
        const int e = b + c;
        bool down = false;
        if (e >= 1 && e < len) down = link_down(k.key, (uint32_t)ag, cr[e], k.thr_edge, k.thr_node);
        return group_bits<C>(down, gsh);
    };
    uint64_t bits = 0;   // entries [0, 64)
    float wd = wr[0];
    for (int b = 0; b < len; b += C) {
        uint32_t m = draw(b);
        if (b < 64) bits |= (uint64_t)m << b;
        while (m) {   // ascending: CSR order
            wd = wd + wr[b + __builtin_ctz(m)];
            m &= m - 1;
        }
    }
    float4 acc = zero4();
    axpy4(acc, wd, src[cr[0] * C + c]);
    uint32_t m = 0;
    for (int e = 1; e < len; ++e) {
        bool down;
        if (e < 64) {
            down = (bits >> e) & 1;
        } else {
            if ((e & (C - 1)) == 0) m = draw(e);   // (C divides 64: chunks start where b did)
            down = (m >> (e & (C - 1))) & 1;
        }
        axpy4_up(acc, wr[e], src[cr[e] * C + c], down);
    }
    return acc;
}

// g rides the prefetch one tile ahead beside x (4 KV VGPRs more) where that fits the 128 VGPRs of
// a 1024-thread workgroup; else it is loaded while the tile is staged.  From `make resource
// RES_SRC=mix_drop.hip`: no instantiation may use scratch.
constexpr bool prefetch_g(int C, int KV, bool SGD, int RE) {
    return SGD && KV < 8 && !(RE > 0 && KV == 4 && C <= 2);
}
// ... and x too where the lane draws its whole row itself beside 4 rows' registers (the register
// CSR at C = 1, KV = 4: the c4 shape), which with the prefetch kept 8 bytes of scratch
constexpr bool prefetch_x(int C, int KV, int RE) { return !(RE > 0 && KV == 4 && C == 1); }

// C: float4 chunks per tile row (T = 4C columns); KV: rows per thread (agents s + k * SLOTS);
// SGD: local step x - lr g applied once, before the first round; RE: 5 = the register CSR (five
// entries a row, the weights shared), 0 = the CSR from LDS.  FAST tiles only.
template <int C, int KV, bool SGD, int RE>
__global__ void __launch_bounds__(kTileThreads) mix_drop_kernel(TileArgs a, DropArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;
    constexpr int LOGC = C == 1 ? 0 : C == 2 ? 1 : C == 4 ? 2 : C == 8 ? 3 : C == 16 ? 4 : 5;
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int gsh = tid & 63 & ~(C - 1);
    const int Nr = a.n_rows;
    const int rounds = q.rounds;
    const bool dev = a.dev_partial != nullptr;
    float4 *img0 = reinterpret_cast<float4 *>(smem);
    float4 *img1 = img0 + (size_t)Nr * C;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);
    const LdsCsr L = lds_csr(smem, a, false);
    if constexpr (RE == 0) stage_csr(L, a, tid);   // published by the first staging barrier

    const uint32_t t0 = q.round0_dev ? *q.round0_dev : q.round0;   // uniform; never written here

    uint32_t ox = (uint32_t)s * a.xrs + 16u * c;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t og = SGD ? (uint32_t)s * a.grs + 16u * c : 0u;
    const uint32_t sg = SGD ? (uint32_t)SLOTS * a.grs : 0u;
    uint32_t oy = (uint32_t)s * a.yrs + 16u * c;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;

    constexpr bool PFG = prefetch_g(C, KV, SGD, RE);
    constexpr bool PFX = prefetch_x(C, KV, RE);
    float4 px[PFX ? KV : 1], pg[PFG ? KV : 1];
    auto prefetch = [&](int tile_id) __attribute__((always_inline)) {
        const char *xt = PFX ? tile_base(a, a.x, a.xts, tile_id) : nullptr;
        const char *gt = PFG ? tile_base(a, a.g, a.gts, tile_id) : nullptr;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const bool ok = s + k * SLOTS < Nr;   // ragged: re-read row 0 (an L1 hit)
            if (PFX) px[PFX ? k : 0] = nt_load4(md_at(xt, ok ? ox + k * sx : 16u * c));
            if (PFG) pg[PFG ? k : 0] = nt_load4(md_at(gt, ok ? og + k * sg : 16u * c));
        }
    };

    // register CSR (RE > 0): byte offset of each neighbour's chunk c inside an image (the column
    // id is the offset >> (4 + log2 C)) and the shared weights
    uint32_t coff[KV][RE > 0 ? RE : 1];
    float wreg[RE > 0 ? RE : 1];
    if constexpr (RE > 0) {
#pragma unroll
        for (int e = 0; e < RE; ++e) wreg[e] = a.w[e];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS < Nr ? s + k * SLOTS : 0;
#pragma unroll
            for (int e = 0; e < RE; ++e)
                coff[k][e] = ((uint32_t)a.col[ag * RE + e] * C + c) * 16u;
        }
    }
    auto fold_reg = [&](const float4 *src, int k, int ag, const DropKey &dk)
                        __attribute__((always_inline)) {
        constexpr int R = RE > 0 ? RE : 1;
        // lane c draws entries c, c + C, ... (entry 0: self, never down)
        uint32_t bits = 0;
#pragma unroll
        for (int b = 0; b < R; b += C) {
            const int e = b + c;
            uint32_t off = coff[k][b];
#pragma unroll
            for (int i = 1; i < C && b + i < R; ++i) off = c == i ? coff[k][b + i] : off;
            bool down = false;
            if (e >= 1 && e < R)
                down = link_down(dk.key, (uint32_t)ag, off >> (4 + LOGC), dk.thr_edge, dk.thr_node);
            bits |= group_bits<C>(down, gsh) << b;
        }
        float wd = wreg[0];
#pragma unroll
        for (int e = 1; e < R; ++e) {
            const float t = wd + wreg[e];
            wd = (bits >> e) & 1 ? t : wd;
        }
        const char *base = reinterpret_cast<const char *>(src);
        float4 acc = zero4();
        axpy4(acc, wd, *reinterpret_cast<const float4 *>(base + coff[k][0]));
#pragma unroll
        for (int e = 1; e < R; ++e)
            axpy4_up(acc, wreg[e], *reinterpret_cast<const float4 *>(base + coff[k][e]),
                     (bits >> e) & 1);
        return acc;
    };
    auto out_row = [&](const float4 *src, int k, int ag, const DropKey &dk)
                       __attribute__((always_inline)) {
        if constexpr (RE > 0) return fold_reg(src, k, ag, dk);
        return drop_fold_csr<C>(L, src, ag, c, gsh, dk);
    };

    DevAcc<C, KV, false> dv;   // per-agent ||y - mean||^2, slot k / C of lane k % C
    dev_zero(dv);

    // mix_multi.hip's rotated tile loop: the next tile is staged after this tile's stores and its
    // successor's prefetch issued right after
    int tile_id = blockIdx.x;
    float4 mean = zero4();
    auto stage = [&](int tile) __attribute__((always_inline)) {
        float4 cst = zero4();
        const char *xt = PFX ? nullptr : tile_base(a, a.x, a.xts, tile);
        const char *gt = SGD && !PFG ? tile_base(a, a.g, a.gts, tile) : nullptr;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int r = s + k * SLOTS;
            float4 t;
            if constexpr (PFX)
                t = px[k];
            else
                t = nt_load4(md_at(xt, r < Nr ? ox + k * sx : 16u * c));
            if (SGD) {
                float4 g;
                if constexpr (PFG)
                    g = pg[k];
                else
                    g = nt_load4(md_at(gt, r < Nr ? og + k * sg : 16u * c));
                t.x = t.x - a.lr * g.x;
                t.y = t.y - a.lr * g.y;
                t.z = t.z - a.lr * g.z;
                t.w = t.w - a.lr * g.w;
            }
            if (r < Nr) {
                img0[r * C + c] = t;
                add4(cst, t);
            }
        }
        if (dev) col_sums_to_scratch<C>(cst, scratch, tid);
        __syncthreads();
        mean = zero4();
        if (dev) {
            float4 sum = zero4();
#pragma unroll 2
            for (int wv = 0; wv < NT / 64; ++wv) add4(sum, scratch[wv * C + c]);
            mean = div4(sum, (float)Nr);
        }
    };
    const int last = a.n_tiles - 1;
    if (tile_id < a.n_tiles) {
        prefetch(tile_id);
        stage(tile_id);
        prefetch(min(tile_id + (int)gridDim.x, last));
    }
    for (; tile_id < a.n_tiles; tile_id += gridDim.x) {
        asm volatile("" : "+v"(ox), "+v"(og), "+v"(oy));
        const int nxt = min(tile_id + (int)gridDim.x, last);
        const float4 *src = img0;
        float4 *dst = img1;
        for (int r = 0; r + 1 < rounds; ++r) {
            const DropKey dk{link_round_key(q.seed, t0 + (uint32_t)r), q.thr_edge, q.thr_node};
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int ag = s + k * SLOTS;
                if (ag < Nr) dst[ag * C + c] = out_row(src, k, ag, dk);
                // one output row at a time (register pressure at 1024 threads, mix_multi.hip)
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            const float4 *t = src;
            src = dst;
            dst = const_cast<float4 *>(t);
        }
        const DropKey dk{link_round_key(q.seed, t0 + (uint32_t)(rounds - 1)), q.thr_edge,
                         q.thr_node};
        const char *yt = tile_base(a, a.y, a.yts, tile_id);
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS;
            if (ag < Nr) {
                const float4 y = out_row(src, k, ag, dk);
                float4 *py = const_cast<float4 *>(md_at(yt, oy + (uint32_t)k * sy));
                if (a.nt_store)
                    nt_store4(y, py);
                else
                    *py = y;
                if (dev) dev_add(dv, k, y, mean, c);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (dev && a.mean != nullptr && s == 0) {
            const int64_t col0 = a.col_base + (int64_t)tile_id * 4 * C + 4 * c;
            *reinterpret_cast<float4 *>(a.mean + col0) = mean;
        }
        __syncthreads();   // both images and the scratch are rewritten by the next tile
        stage(nxt);        // (past the end: a re-read of the last tile, then unused)
        prefetch(min(nxt + (int)gridDim.x, last));   // lands while the next tile's rounds run
    }
    if (dev) dev_epilogue(dv, a, tid, Nr);
}

template <int C, int KV, int RE>
hipError_t launch_re(const TileArgs &a, const DropArgs &q, bool sgd, int grid, int lds,
                     hipStream_t s) {
    return sgd ? launch_lds(mix_drop_kernel<C, KV, true, RE>, grid, lds, s, a, q)
               : launch_lds(mix_drop_kernel<C, KV, false, RE>, grid, lds, s, a, q);
}

template <int C, int KV>
hipError_t launch_kv(const TileArgs &a, const DropArgs &q, bool sgd, int grid, int lds,
                     hipStream_t s) {
    // the same test as csr_in_registers() on the host, which then reserves no LDS for the CSR
    if constexpr (KV <= 4) {
        if (a.regular == 5 && a.n_w == 5) return launch_re<C, KV, 5>(a, q, sgd, grid, lds, s);
    }
    return launch_re<C, KV, 0>(a, q, sgd, grid, lds, s);
}

}  // namespace

hipError_t launch_mix_drop(const TileArgs &a, const DropArgs &q, int chunks, bool sgd, int grid,
                           int lds, hipStream_t s) {
    if (q.rounds < 1 || a.n_src != a.n_rows || a.n_loc != a.n_rows || (sgd && a.g == nullptr))
        return hipErrorInvalidValue;
    return with_chunks(chunks, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        return with_passes(tile_passes(C, a.n_rows, true), [&](auto kv) {
            return launch_kv<C, decltype(kv)::value>(a, q, sgd, grid, lds, s);
        });
    });
}

}  // namespace dl
