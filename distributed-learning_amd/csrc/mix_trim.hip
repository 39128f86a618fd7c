// Trimmed-mean consensus round for gfx950 (MI355X): the screened counterpart of dl_mix_round
// (BRIDGE-T / ByRDiE).  Per column every agent drops the b largest and the b smallest of its
// neighbours' values and averages what is left with its own:
//   s_j = x_j, or fl(x_j - fl(lr g_j)) with g            (dl_mix_round's local step)
//   u_1 <= ... <= u_n = the n neighbours' s_j[p], ascending
//   y_a[p] = fl((((+0.0 + u_{b+1}) + ...) + u_{n-b} + s_a[p]) / (float)(n - 2b + 1))
// every operation rounded separately (-ffp-contract=off).  Only W's sparsity pattern is read: a
// row lists the closed neighbourhood, its one entry with col == row is the agent itself.  The
// result for NaN inputs is unspecified (fminf / fmaxf drop a NaN where a comparison sort moves it).
//
// Design (path 1): the sixth LDS tile kernel, as mix_tile.hip / mix_sgd.hip.
// Persistent 1024-thread workgroups each own column tiles of T = 4*C floats for all agents; the
// CSR is staged once per workgroup in LDS; the geometry (chunks, LDS offsets, grid, tiles) is the
// planner's for the same dl_mix_args.  Per tile a thread steps its rows' chunk of x with g and
// puts it in the LDS image; after the barrier every output row is folded from LDS and written.
// 12 B per element cross HBM with g (8 B without), whatever the graph.  y may be x itself: a
// workgroup stages all rows of its columns before it writes them.
//
// The fold of a row replaces the siblings' weighted sum.  The row's column ids come from the LDS
// CSR (at most the promised max_nbrs + 1 of them); the position of the self entry is found among
// them and the other ids close up over it, so the row's up-to-NW neighbour float4s are gathered
// from the LDS image into statically indexed registers.  Slots beyond the row's n neighbours hold
// +Inf: pads sort behind every true value (ties with a true +Inf are indistinguishable), so the
// first n outputs of the network are u_1..u_n whatever the row's length.  Each of the four
// components then runs one fixed Batcher odd-even merge network of fminf / fmaxf exchanges (5
// at NW = 4, 19 at 8, 63 at 16; branch-free), outputs b..n-b-1 are added under a predicate on the
// runtime b and n, self -- tile[row], no search -- is added and the sum divided.  The fold starts
// from +0.0, so the order among values that compare equal (-0.0 and +0.0 included) cannot change
// a bit of the sum.  NW in {4, 8, 16} is the host's choice from the promised longest row; a
// regular graph has n as a constant of the launch (TrimTileArgs::uniform_nbrs).
//
// A caller that breaks the degree promises gets wrong values and no out-of-range access: a row is
// read for at most max_nbrs + 1 entries at indices clamped into the CSR, slots past the row read
// the agent's own element, and the column ids are used as the other tile kernels use them.
//
// Prefetch as mix_sgd.hip: x and g ride the prefetch one tile ahead up to KV = 4 rows per thread;
// at KV = 8 only x does and g is loaded while the tile is staged, four rows at a time.  The
// passes stay a rolled loop; the NW slot addresses and NW float4 (NW float2 at NW = 16, where the
// four components are gathered and sorted two at a time: all four at once spilled with the
// deviation) are live beside the prefetch registers.
// The deviation is always the two-pass form (a trimmed mean does not preserve the column mean;
// mean_from_inputs is not read): y is recomputed in the second LDS pass instead of being held --
// 4*KV more registers beside the network's do not fit under 128 at NW = 16.
// VGPRs (make resource RES_SRC=mix_trim.hip; every instantiation without scratch), lowest without
// the deviation to highest with it, over C and KV: FAST NW = 4: 46-95, NW = 8: 62-113, NW = 16:
// 85-126; guarded (KV = 8) NW = 4: 42-59, NW = 8: 62-76, NW = 16: 73-93.
#include <type_traits>
#include <utility>

#include "tile_core.h"

namespace dl {
namespace {

// x - lr*g with two roundings (mix_tile.hip's local step)
__device__ __forceinline__ float4 local_step(float4 x, float4 g, float lr) {
    float4 t;
    t.x = x.x - lr * g.x;
    t.y = x.y - lr * g.y;
    t.z = x.z - lr * g.z;
    t.w = x.w - lr * g.w;
    return t;
}

// Batcher's odd-even merge sort of N = 2^k keys as a list of compare-exchanges (lo, hi), lo < hi
template <int N>
struct Network {
    int n;
    int lo[64], hi[64];
};
template <int N>
constexpr Network<N> batcher() {
    Network<N> w{};
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < N; j += 2 * k)
                for (int i = 0; i < k && i + j + k < N; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        w.lo[w.n] = i + j;
                        w.hi[w.n] = i + j + k;
                        ++w.n;
                    }
    return w;
}
template <int N>
struct Net {
    static constexpr Network<N> w = batcher<N>();
};
static_assert(Net<4>::w.n == 5 && Net<8>::w.n == 19 && Net<16>::w.n == 63, "minimal networks");

template <int N, int I>
__device__ __forceinline__ void exchange(float (&v)[N]) {
    constexpr int lo = Net<N>::w.lo[I], hi = Net<N>::w.hi[I];
    const float a = v[lo], b = v[hi];
    v[lo] = fminf(a, b);
    v[hi] = fmaxf(a, b);
}
template <int N, size_t... I>
__device__ __forceinline__ void sort_net(float (&v)[N], std::index_sequence<I...>) {
    (exchange<N, (int)I>(v), ...);
}

// A row's shape for the fold: entries [e0, e0 + len) of the LDS CSR, len clipped to the promise
struct TrimRow {
    int b;          // trim
    int cap;        // max_nbrs + 1: entries read per row
    int uni;        // > 0: every row has uni neighbours
    int elast;      // last valid CSR index
};

// The trimmed mean of row ag, chunk c, from the LDS image src ([rows][C] float4); reads only LDS.
template <int C, int NW>
__device__ __forceinline__ float4 trim_fold(const LdsCsr &L, const TrimRow &r, const float4 *src,
                                            int ag, int c) {
    int e0, len;
    if (L.reg) {
        e0 = ag * L.reg;
        len = L.reg;
    } else {
        e0 = L.lrp[ag];
        len = (int)L.lrp[ag + 1] - e0;
    }
    len = min(max(len, 0), r.cap);
    // the row's ids and the self entry's position among them
    uint32_t id[NW + 1];
#pragma unroll
    for (int i = 0; i <= NW; ++i) id[i] = L.lcol[min(e0 + i, r.elast)];
    int sp = NW + 1;
#pragma unroll
    for (int i = NW; i >= 0; --i) sp = (id[i] == (uint32_t)ag && i < len) ? i : sp;
    const int n = r.uni > 0 ? min(r.uni, r.cap - 1) : max(len - 1, 0);
    // slot i is entry i, or i + 1 from the self entry on; slots beyond the n neighbours read the
    // agent's own element and hold +Inf
    uint32_t at[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i)
        at[i] = (i < n ? (i >= sp ? id[i + 1] : id[i]) : (uint32_t)ag) * C + c;
    const float4 self = src[ag * C + c];
    const int hi = n - r.b;
    // V components per gather: all four of a float4 up to NW = 8; at NW = 16 two halves of two
    // (ds_read_b64) in a rolled loop, so 32 values are live instead of 64
    constexpr int V = NW == 16 ? 2 : 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int h = 0; h < 4 / V; ++h) {
        if (V < 4) asm volatile("" : "+s"(h));   // opaque: the halves are not interleaved
        float v[V][NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const bool ok = i < n;
            if constexpr (V == 4) {
                const float4 t = src[at[i]];
                v[0][i] = ok ? t.x : __builtin_inff();
                v[1][i] = ok ? t.y : __builtin_inff();
                v[2][i] = ok ? t.z : __builtin_inff();
                v[3][i] = ok ? t.w : __builtin_inff();
            } else {
                const float2 t = reinterpret_cast<const float2 *>(src + at[i])[h];
                v[0][i] = ok ? t.x : __builtin_inff();
                v[1][i] = ok ? t.y : __builtin_inff();
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            sort_net<NW>(v[j], std::make_index_sequence<Net<NW>::w.n>{});
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < NW; ++i) t = (i >= r.b && i < hi) ? t + v[j][i] : t;
            // (h is a run-time value in the rolled loop: a select per result register)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[o] = o == h * V + j ? t : acc[o];
        }
    }
    const float cnt = (float)(n - 2 * r.b + 1);
    return div4(make_float4(acc[0] + self.x, acc[1] + self.y, acc[2] + self.z, acc[3] + self.w),
                cnt);
}

// C, KV, DEV, FAST as mix_sgd_tile_kernel's (no halo rows, no row sets; g optional, a run-time
// choice); NW: slots of the sorting network, >= the longest row's neighbours
template <int C, int KV, int NW, bool DEV, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, kTileThreads)))
mix_trim_tile_kernel(TileArgs a, TrimTileArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *tile = reinterpret_cast<float4 *>(smem);
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;  // rows covered per pass
    constexpr int T = 4 * C;
    constexpr bool PFG = FAST && KV <= 4;   // g rides the prefetch
    constexpr int HB = 4;                   // FAST, KV = 8: rows of g per staging step
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int R = a.n_rows;
    const int64_t P = a.n_params;
    const bool sgd = a.g != nullptr;
    const float lr = a.lr;
    const TrimRow row{q.b, min(q.max_nbrs, NW) + 1, q.uniform_nbrs, max(a.nnz - 1, 0)};

    // FAST-path byte offsets: lane row s / chunk c; pass k adds k * step
    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t og = sgd ? (uint32_t)s * a.grs + lc : 0u;
    const uint32_t sg = sgd ? (uint32_t)SLOTS * a.grs : 0u;
    uint32_t oy = (uint32_t)s * a.yrs + lc;
    const uint32_t sy = (uint32_t)SLOTS * a.yrs;
    float4 *scratch = reinterpret_cast<float4 *>(smem + a.scratch_off);

    float4 px[FAST ? KV : 1], pg[PFG ? KV : 1];
    DevAcc<C, KV, DEV && dev_per_lane(C, KV)> dv;   // per-agent ||y - mean||^2
    dev_zero(dv);

    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;

    auto prefetch = [&](int tile_id) {
        if (FAST) {
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
            const __amdgpu_buffer_rsrc_t rg =
                buf_rsrc(sgd ? tile_base(a, a.g, a.gts, tile_id) : tile_base(a, a.x, a.xts, tile_id));
            // one straight-line loop per load policy (bit 0: x non-temporal, bit 1: g)
            auto loads = [&](auto ax, auto ag) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = s + k * SLOTS < R;
                    px[k] = buf_ld4<decltype(ax)::value>(rx, ok ? ox + k * sx : lc);
                }
                if (PFG && sgd) {
#pragma unroll
                    for (int k = 0; k < KV; ++k) {
                        const bool ok = s + k * SLOTS < R;
                        pg[PFG ? k : 0] = buf_ld4<decltype(ag)::value>(rg, ok ? og + k * sg : lc);
                    }
                }
            };
            if (a.nt_load == 3) loads(PNT{}, PNT{});
            else if (a.nt_load == 1) loads(PNT{}, PPL{});
            else if (a.nt_load == 2) loads(PPL{}, PNT{});
            else loads(PPL{}, PPL{});
        }
    };

    // the fold of a row reads only LDS; the weights are staged with the ids (the planner's LDS
    // layout) and never read
    const LdsCsr L = lds_csr(smem, a, false);

    TileWalk tw = tile_walk(a);
    if (tw.id < tw.end) prefetch(tw.id);
    // the LDS CSR is staged behind the first tile's loads; the first staging barrier publishes it
    stage_csr(L, a, tid);
    for (; tw.id < tw.end; tw.id += tw.step) {
        const int tile_id = tw.id;
        // opaque per tile: keeps LICM from hoisting one offset register per pass
        asm volatile("" : "+v"(ox), "+v"(og), "+v"(oy));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tw.step;
        const __amdgpu_buffer_rsrc_t rgc =
            buf_rsrc(sgd ? tile_base(a, a.g, a.gts, tile_id) : tile_base(a, a.x, a.xts, tile_id));
        auto load_x = [&](int k) {   // (guarded kernel)
            const int r = s + k * SLOTS;
            return ld4(a.x + (int64_t)(r < R ? r : 0) * a.ldx, col0 + 4 * c, P, false);
        };
        auto load_g = [&](int k) {   // (guarded kernel, and FAST at KV = 8); sgd only
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t o = r < R ? og + (uint32_t)k * sg : lc;
                return (a.nt_load & 2) ? buf_ld4<kBufNT>(rgc, o) : buf_ld4<0>(rgc, o);
            }
            return ld4(a.g + (int64_t)(r < R ? r : 0) * a.ldg, col0 + 4 * c, P, false);
        };
        // step every source row and stage the stepped tile in LDS
        auto stage = [&](int k, float4 x, float4 g) {
            const int r = s + k * SLOTS;
            if (r < R) tile[r * C + c] = sgd ? local_step(x, g, lr) : x;
        };
        if constexpr (PFG) {
#pragma unroll
            for (int k = 0; k < KV; ++k) stage(k, px[k], sgd ? pg[PFG ? k : 0] : zero4());
        } else if constexpr (FAST) {
#pragma unroll
            for (int k0 = 0; k0 < KV; k0 += HB) {
                float4 hg[HB];
#pragma unroll
                for (int j = 0; j < HB; ++j)
                    hg[j] = (sgd && k0 + j < KV) ? load_g(k0 + j) : zero4();
#pragma unroll
                for (int j = 0; j < HB; ++j)
                    if (k0 + j < KV) stage(k0 + j, px[(k0 + j) % KV], hg[j]);
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < KV; ++k) stage(k, load_x(k), sgd ? load_g(k) : zero4());
        }
        __syncthreads();
        // the next tile's loads go out first: they land while we sort from LDS
        if (nxt < tw.end) prefetch(nxt);
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(tile_base(a, a.y, a.yts, tile_id));
        float4 cs = zero4();
        // passes stay rolled: one row's network is live at a time beside the prefetch registers
#pragma unroll 1
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS;
            if (ag < R) {
                const float4 y = trim_fold<C, NW>(L, row, tile, ag, c);
                store_y<FAST>(a, ry, oy + (uint32_t)k * sy, ag, col0 + 4 * c, y);
                if (DEV) add4(cs, y);
            }
        }
        if (DEV) {
            const float4 mean = tile_mean<C>(cs, scratch, tid, c, R);
            if (a.mean != nullptr && s == 0) st4(a.mean, col0 + 4 * c, P, FAST, mean);
            // second LDS pass: recompute y (same network, same order, same bits)
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                const int ag = s + k * SLOTS;
                if (ag < R) dev_add(dv, k, trim_fold<C, NW>(L, row, tile, ag, c), mean, c);
            }
        }
        __syncthreads();  // tile and scratch are rewritten by the next iteration
    }
    if (DEV) dev_epilogue(dv, a, tid, R);
}

template <int C, int KV, int NW, bool FAST>
hipError_t launch_nw(const TileArgs &a, const TrimTileArgs &q, bool dev, int grid, int lds,
                     hipStream_t s) {
    return dev ? launch_lds(mix_trim_tile_kernel<C, KV, NW, true, FAST>, grid, lds, s, a, q)
               : launch_lds(mix_trim_tile_kernel<C, KV, NW, false, FAST>, grid, lds, s, a, q);
}

template <int C, int KV, bool FAST>
hipError_t launch_kv(const TileArgs &a, const TrimTileArgs &q, bool dev, int grid, int lds,
                     hipStream_t s) {
    if (q.max_nbrs <= 4) return launch_nw<C, KV, 4, FAST>(a, q, dev, grid, lds, s);
    if (q.max_nbrs <= 8) return launch_nw<C, KV, 8, FAST>(a, q, dev, grid, lds, s);
    return launch_nw<C, KV, 16, FAST>(a, q, dev, grid, lds, s);
}

}  // namespace

hipError_t launch_mix_trim_tile(const TileArgs &a, const TrimTileArgs &q, int chunks, bool dev,
                                int grid, int lds, bool fast, hipStream_t s) {
    // no halo rows and no row sets: every staged row is a local source row and an output row
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows) return hipErrorInvalidValue;
    if (q.b < 0 || q.b > 7 || q.max_nbrs < 1 || q.max_nbrs > 16 || q.uniform_nbrs < 0 ||
        q.uniform_nbrs > q.max_nbrs)
        return hipErrorInvalidValue;
    // FAST kernels: every C x KV in {2, 4, 8} x NW in {4, 8, 16}; guarded kernels: every C x NW,
    // KV = 8 (plan.h tile_passes)
    return with_chunks(chunks, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        if (!fast) return launch_kv<C, kRowsPerThread, false>(a, q, dev, grid, lds, s);
        return with_passes(tile_passes(C, a.n_src, true), [&](auto kv) {
            return launch_kv<C, decltype(kv)::value, true>(a, q, dev, grid, lds, s);
        });
    });
}

}  // namespace dl
