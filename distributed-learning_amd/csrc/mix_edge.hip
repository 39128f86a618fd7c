// Per-edge squared distances for gfx950 (MI355X), and the clipped-gossip weights made from them
// (self-centred clipping; He, Karimireddy, Jaggi: "Byzantine-robust decentralized learning via
// ClippedGossip").  For every CSR entry e of row a with column j
//   s_j  = x_j, or fl(x_j - fl(lr g_j)) with g            (dl_mix_round's local step)
//   E[e] = sum_p fl(fl(s_j[p] - s_a[p])^2)                 (+0.0 on the diagonal entry)
// by direct differences: near consensus |s_a|^2 + |s_j|^2 - 2 <s_a, s_j> cancels to noise.  The
// sum's order is fixed by the plan (below), not by the caller: any order is within (P + 3) ulp/2
// of the exact sum of the rounded squares, since every term is >= 0.
//
// Design (path 1): the seventh LDS tile kernel, as mix_trim.hip.  Persistent
// 1024-thread workgroups each own column tiles of T = 4*C floats for all agents; the CSR is staged
// once per workgroup in LDS; the geometry is the planner's for the same dl_mix_args.  Per tile a
// thread steps its rows' chunk of x with g and puts it in the LDS image; after the barrier every
// row gathers its up-to-NW neighbour float4s from the image (ids, self position and the closing
// over it exactly as mix_trim.hip's fold; slots past the row's neighbours read the agent's own
// element and add +0.0), and adds (dx dx + dy dy) + (dz dz + dw dw) of the difference to the slot's
// accumulator.  Nothing is written per tile: 8 B per element cross HBM with g, 4 B without.
//
// Accumulators: acc[KV][NW] per lane, statically indexed (the pass loop is unrolled), the lane's
// own chunk's partial of every (row, slot) pair, carried across all of the workgroup's tiles;
// the row group's C lanes are summed once, after the last tile (tile_core.h dev_per_lane is the
// precedent), and lane 0 of the group writes the row's NW sums to the workgroup's partial row
// [n_rows][NW] in the workspace.  edge_reduce_kernel then adds the workgroups' partial rows in
// workgroup order -- the same bits from run to run for one plan --, maps slot i of row a back to
// its CSR entry and writes +0.0 on the diagonal.
// KV * NW <= 64 is instantiated, for the FAST and the guarded kernels alike (the guarded ones run
// the rows per thread the shape needs here, not always 8: they hold no prefetch registers, and 8
// rows x 16 slots cannot be held); launch.cpp refuses a shape beyond it.  VGPRs (make resource
// RES_SRC=mix_edge.hip): profiles/r27/clip_round/vgprs.txt has the table; no instantiation uses
// scratch.
//
// A caller that breaks the row-length promises gets wrong values and no out-of-range access: a
// row is read for at most max_nbrs + 1 entries at indices clamped into the CSR, and the entries
// of a longer row beyond them are written as +0.0.
#include <type_traits>

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

// A row's shape for the gather: entries [e0, e0 + len) of the CSR, len clipped to the promise
struct EdgeRow {
    int cap;        // max_nbrs + 1: entries read per row
    int uni;        // > 0: every row has uni neighbours
    int elast;      // last valid CSR index
};

// The neighbour count n and the self entry's position sp (NW + 1: none) of a row of `len` entries
// whose first NW + 1 column ids are id[]; shared by the tile kernel and the reduce, so slot i is
// entry i, or i + 1 from the self entry on, in both.
template <int NW>
__device__ __forceinline__ void row_slots(const uint32_t (&id)[NW + 1], int ag, int len,
                                          const EdgeRow &r, int &n, int &sp) {
    sp = NW + 1;
#pragma unroll
    for (int i = NW; i >= 0; --i) sp = (id[i] == (uint32_t)ag && i < len) ? i : sp;
    n = r.uni > 0 ? min(r.uni, r.cap - 1) : max(len - 1, 0);
}

// Adds row ag's chunk c of every slot's squared difference to acc[]; reads only LDS.
template <int C, int NW>
__device__ __forceinline__ void edge_row(const LdsCsr &L, const EdgeRow &r, const float4 *src,
                                         int ag, int c, float (&acc)[NW]) {
    int e0, len;
    if (L.reg) {
        e0 = ag * L.reg;
        len = L.reg;
    } else {
        e0 = L.lrp[ag];
        len = (int)L.lrp[ag + 1] - e0;
    }
    len = min(max(len, 0), r.cap);
    uint32_t id[NW + 1];
#pragma unroll
    for (int i = 0; i <= NW; ++i) id[i] = L.lcol[min(e0 + i, r.elast)];
    int n, sp;
    row_slots<NW>(id, ag, len, r, n, sp);
    const float4 self = src[ag * C + c];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t at = (i < n ? (i >= sp ? id[i + 1] : id[i]) : (uint32_t)ag) * C + c;
        const float4 t = src[at];
        const float dx = t.x - self.x, dy = t.y - self.y;
        const float dz = t.z - self.z, dw = t.w - self.w;
        acc[i] += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
}

// C, KV, FAST as mix_trim_tile_kernel's (no halo rows, no row sets; g optional, a run-time
// choice; the guarded kernel too runs KV rows per thread); NW: slots per row, >= the longest
// row's neighbours
template <int C, int KV, int NW, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, kTileThreads)))
mix_edge_tile_kernel(TileArgs a, EdgeTileArgs q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *tile = reinterpret_cast<float4 *>(smem);
    constexpr int NT = kTileThreads;
    constexpr int SLOTS = NT / C;  // rows covered per pass
    constexpr int T = 4 * C;
    // x rides the prefetch one tile ahead, except at KV * NW = 64: those accumulators, the
    // prefetch registers and a row's gather do not fit 128 VGPRs together (44-72 bytes of scratch
    // a lane), so there x and g are loaded while the tile is staged
    constexpr bool PFX = FAST && KV * NW < kEdgeAccumulators;
    constexpr bool PFG = PFX && KV <= 4;    // g rides the prefetch too
    constexpr int HB = PFX ? 4 : 2;         // FAST, g or both loaded here: rows per staging step
    const int tid = threadIdx.x;
    const int c = tid & (C - 1);
    const int s = tid / C;
    const int R = a.n_rows;
    const int64_t P = a.n_params;
    const bool sgd = a.g != nullptr;
    const float lr = a.lr;
    const EdgeRow row{min(q.max_nbrs, NW) + 1, q.uniform_nbrs, max(a.nnz - 1, 0)};

    // FAST-path byte offsets: lane row s / chunk c; pass k adds k * step
    const uint32_t lc = 16u * (uint32_t)c;
    uint32_t ox = (uint32_t)s * a.xrs + lc;
    const uint32_t sx = (uint32_t)SLOTS * a.xrs;
    uint32_t og = sgd ? (uint32_t)s * a.grs + lc : 0u;
    const uint32_t sg = sgd ? (uint32_t)SLOTS * a.grs : 0u;

    float4 px[PFX ? KV : 1], pg[PFG ? KV : 1];
    float acc[KV][NW];
#pragma unroll
    for (int k = 0; k < KV; ++k)
#pragma unroll
        for (int i = 0; i < NW; ++i) acc[k][i] = 0.f;

    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;

    auto prefetch = [&](int tile_id) {
        if (PFX) {
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
            const __amdgpu_buffer_rsrc_t rg =
                buf_rsrc(sgd ? tile_base(a, a.g, a.gts, tile_id) : tile_base(a, a.x, a.xts, tile_id));
            // one straight-line loop per load policy (bit 0: x non-temporal, bit 1: g)
            auto loads = [&](auto ax, auto ag) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = s + k * SLOTS < R;
                    px[PFX ? k : 0] = buf_ld4<decltype(ax)::value>(rx, ok ? ox + k * sx : lc);
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

    // the weights are staged with the ids (the planner's LDS layout) and never read
    const LdsCsr L = lds_csr(smem, a, false);

    TileWalk tw = tile_walk(a);
    if (tw.id < tw.end) prefetch(tw.id);
    // the LDS CSR is staged behind the first tile's loads; the first staging barrier publishes it
    stage_csr(L, a, tid);
    for (; tw.id < tw.end; tw.id += tw.step) {
        const int tile_id = tw.id;
        // opaque per tile: keeps LICM from hoisting one offset register per pass
        asm volatile("" : "+v"(ox), "+v"(og));
        const int64_t col0 = a.col_base + (int64_t)tile_id * T;
        const int nxt = tile_id + tw.step;
        const __amdgpu_buffer_rsrc_t rgc =
            buf_rsrc(sgd ? tile_base(a, a.g, a.gts, tile_id) : tile_base(a, a.x, a.xts, tile_id));
        const __amdgpu_buffer_rsrc_t rxc = buf_rsrc(tile_base(a, a.x, a.xts, tile_id));
        // (guarded kernel: columns >= P read as 0 in every row; and FAST without a prefetch)
        auto load_x = [&](int k) {
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t o = r < R ? ox + (uint32_t)k * sx : lc;
                return (a.nt_load & 1) ? buf_ld4<kBufNT>(rxc, o) : buf_ld4<0>(rxc, o);
            }
            return ld4(a.x + (int64_t)(r < R ? r : 0) * a.ldx, col0 + 4 * c, P, false);
        };
        auto load_g = [&](int k) {   // (likewise, and FAST at KV = 8); sgd only
            const int r = s + k * SLOTS;
            if (FAST) {
                const uint32_t o = r < R ? og + (uint32_t)k * sg : lc;
                return (a.nt_load & 2) ? buf_ld4<kBufNT>(rgc, o) : buf_ld4<0>(rgc, o);
            }
            return ld4(a.g + (int64_t)(r < R ? r : 0) * a.ldg, col0 + 4 * c, P, false);
        };
        // step every source row and stage the stepped tile in LDS
        // (a column-tiled operand's last tile is padded to T columns: the padding must not enter
        // E, whatever it holds)
        const bool ragged = FAST && col0 + T > P;
        auto stage = [&](int k, float4 x, float4 g) {
            const int r = s + k * SLOTS;
            float4 v = sgd ? local_step(x, g, lr) : x;
            if (ragged) {
                const int64_t p0 = col0 + 4 * c;
                v.x = p0 < P ? v.x : 0.f;
                v.y = p0 + 1 < P ? v.y : 0.f;
                v.z = p0 + 2 < P ? v.z : 0.f;
                v.w = p0 + 3 < P ? v.w : 0.f;
            }
            if (r < R) tile[r * C + c] = v;
        };
        if constexpr (PFG) {
#pragma unroll
            for (int k = 0; k < KV; ++k) stage(k, px[k], sgd ? pg[PFG ? k : 0] : zero4());
        } else if constexpr (FAST) {
#pragma unroll
            for (int k0 = 0; k0 < KV; k0 += HB) {
                float4 hx[HB], hg[HB];
#pragma unroll
                for (int j = 0; j < HB; ++j) {
                    hx[j] = PFX ? px[PFX ? (k0 + j) % KV : 0] : load_x(k0 + j);
                    hg[j] = (sgd && k0 + j < KV) ? load_g(k0 + j) : zero4();
                }
#pragma unroll
                for (int j = 0; j < HB; ++j)
                    if (k0 + j < KV) stage(k0 + j, hx[j], hg[j]);
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < KV; ++k) stage(k, load_x(k), sgd ? load_g(k) : zero4());
        }
        __syncthreads();
        // the next tile's loads go out first: they land while we gather from LDS
        if (PFX && nxt < tw.end) prefetch(nxt);
        // unrolled: acc[k][] stays in statically indexed registers
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int ag = s + k * SLOTS;
            if (ag < R) edge_row<C, NW>(L, row, tile, ag, c, acc[k]);
        }
        __syncthreads();  // the tile is rewritten by the next iteration
    }
    // once per workgroup: the row group's C lanes summed, the row's NW sums to the partial row
    float *part = q.partial + (int64_t)blockIdx.x * R * NW;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
        const int ag = s + k * SLOTS;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const float v = row_group_sum<C>(acc[k][i]);
            if (c == 0 && ag < R) part[ag * NW + i] = v;
        }
    }
}

// E[e] of entry i of row a = the sum over the workgroups' partial rows, in workgroup order, of the
// entry's slot; +0.0 on the diagonal entry and on entries beyond the promised row length.  One
// thread per (row, i <= NW).
template <int NW>
__global__ void __launch_bounds__(256)
edge_reduce_kernel(const float *__restrict__ partial, int parts, int n_rows, int nnz, int regular,
                   EdgeRow r, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                   float *__restrict__ E) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int ag = t / (NW + 1), i = t % (NW + 1);
    if (ag >= n_rows) return;
    const int e0 = regular ? ag * regular : rowptr[ag];
    const int full = regular ? regular : rowptr[ag + 1] - e0;
    if (e0 < 0 || full <= 0) return;
    const int len = min(full, r.cap);
    uint32_t id[NW + 1];
#pragma unroll
    for (int j = 0; j <= NW; ++j) id[j] = (uint32_t)col[min(e0 + j, r.elast)];
    int n, sp;
    row_slots<NW>(id, ag, len, r, n, sp);
    if (i == NW)   // a row longer than promised
        for (int e = e0 + NW + 1; e < min(e0 + full, nnz); ++e) E[e] = 0.f;
    if (i >= full || e0 + i >= nnz) return;
    const int slot = i < sp ? i : i - 1;
    float sum = 0.f;
    if (i != sp && slot < n) {
        const float *p = partial + (int64_t)ag * NW + slot;
        const int64_t stride = (int64_t)n_rows * NW;
#pragma unroll 16
        for (int b = 0; b < parts; ++b) sum += p[b * stride];
    }
    E[e0 + i] = sum;
}

// The clipped row of W (include/dlamd.h dl_clip_weights): one thread per row, entries in CSR order.
// sqrtf and / are the correctly rounded ones under this Makefile's flags (hipcc's default for
// fp32); __fsqrt_rn is not: without OCML_BASIC_ROUNDED_OPERATIONS it is the native approximation.
__global__ void __launch_bounds__(256)
clip_weights_kernel(int n_rows, int nnz, int cap, const int32_t *__restrict__ rowptr,
                    const int32_t *__restrict__ col, const float *w, const float *__restrict__ E,
                    const float *__restrict__ tau_in, int drop, float *w_out,
                    float *__restrict__ tau_out) {
    const int ag = blockIdx.x * 256 + threadIdx.x;
    if (ag >= n_rows) return;
    const int e0 = max(rowptr[ag], 0);
    const int e1 = min(rowptr[ag + 1], nnz);
    const int ec = min(e1, e0 + cap);   // the promised row length
    int diag = -1;
    for (int e = ec - 1; e >= e0; --e) diag = col[e] == ag ? e : diag;
    float tau;
    if (tau_in != nullptr) {
        tau = tau_in[ag];
    } else {
        // the (drop + 1)-th largest E among the neighbour entries, by rank count (ties by index)
        float pick = 0.f;
        for (int e = e0; e < ec; ++e) {
            if (e == diag) continue;
            const float v = E[e];
            int rank = 0;
            for (int f = e0; f < ec; ++f)
                rank += (f != diag && (E[f] > v || (E[f] == v && f < e))) ? 1 : 0;
            pick = rank == drop ? v : pick;
        }
        tau = sqrtf(pick);
    }
    if (tau_out != nullptr) tau_out[ag] = tau;
    float t = diag >= 0 ? w[diag] : 0.f;
    for (int e = e0; e < e1; ++e) {
        if (e == diag) continue;
        const float we = w[e];
        float wc = we;
        if (e < ec) {
            const float d = sqrtf(E[e]);
            const float ce = d == 0.f ? 1.f : fminf(1.f, tau / d);
            wc = we * ce;
            t = t + (we - wc);
        }
        w_out[e] = wc;
    }
    if (diag >= 0) w_out[diag] = t;
}

template <int C, int KV, bool FAST>
hipError_t launch_kv(const TileArgs &a, const EdgeTileArgs &q, int grid, int lds, hipStream_t s) {
    constexpr int NWMAX = 64 / KV;   // KV * NW <= 64 accumulators
    if (q.max_nbrs <= 4) return launch_lds(mix_edge_tile_kernel<C, KV, 4, FAST>, grid, lds, s, a, q);
    if constexpr (NWMAX >= 8)
        if (q.max_nbrs <= 8)
            return launch_lds(mix_edge_tile_kernel<C, KV, 8, FAST>, grid, lds, s, a, q);
    if constexpr (NWMAX >= 16)
        return launch_lds(mix_edge_tile_kernel<C, KV, 16, FAST>, grid, lds, s, a, q);
    return hipErrorInvalidValue;   // (launch.cpp edge_slots_fit refused it)
}

}  // namespace

hipError_t launch_mix_edge_tile(const TileArgs &a, const EdgeTileArgs &q, int chunks, int grid,
                                int lds, bool fast, hipStream_t s) {
    // no halo rows and no row sets: every staged row is a local source row and a row of E
    if (a.n_src != a.n_rows || a.n_loc != a.n_rows) return hipErrorInvalidValue;
    if (q.partial == nullptr || q.max_nbrs < 1 || q.max_nbrs > 16 || q.uniform_nbrs < 0 ||
        q.uniform_nbrs > q.max_nbrs)
        return hipErrorInvalidValue;
    return with_chunks(chunks, [&](auto cc) {
        constexpr int C = decltype(cc)::value;
        return with_passes(tile_passes(C, a.n_src, true), [&](auto kv) {
            constexpr int KV = decltype(kv)::value;
            return fast ? launch_kv<C, KV, true>(a, q, grid, lds, s)
                        : launch_kv<C, KV, false>(a, q, grid, lds, s);
        });
    });
}

hipError_t launch_edge_reduce(const TileArgs &a, const EdgeTileArgs &q, const float *partial,
                              int parts, float *edge_sq, hipStream_t s) {
    const int nw = edge_slots(q.max_nbrs);
    const EdgeRow r{min(q.max_nbrs, nw) + 1, q.uniform_nbrs, max(a.nnz - 1, 0)};
    const int grid = (int)(((int64_t)a.n_rows * (nw + 1) + 255) / 256);
    auto go = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, partial, parts, a.n_rows, a.nnz,
                           a.regular, r, a.rowptr, a.col, edge_sq);
    };
    if (nw == 4) go(edge_reduce_kernel<4>);
    else if (nw == 8) go(edge_reduce_kernel<8>);
    else go(edge_reduce_kernel<16>);
    return hipGetLastError();
}

hipError_t launch_clip_weights(int n_rows, int nnz, int max_row_nnz, const int32_t *rowptr,
                               const int32_t *col, const float *w, const float *edge_sq,
                               const float *tau, int drop, float *w_out, float *tau_out,
                               hipStream_t s) {
    hipLaunchKernelGGL(clip_weights_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, s, n_rows,
                       nnz, max_row_nnz, rowptr, col, w, edge_sq, tau, drop, w_out, tau_out);
    return hipGetLastError();
}

}  // namespace dl
