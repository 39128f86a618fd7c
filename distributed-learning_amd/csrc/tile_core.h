// The per-tile pieces that the LDS mixing kernels share (mix_tile.hip, mix_sgd.hip, mix_cheb.hip,
// mix_multi.hip; mix_trace.hip takes the CSR staging): the staged CSR and its row fold, the tile
// mean, the deviation accumulators, the tile walk and the output store, and the host-side
// dispatch of `chunks` to a compile-time C.  Each is defined here once; the kernels keep their
// own prefetch, staging and pass loops and call these between them.  As in tile_ops.h every
// device function is force-inlined, in an unnamed namespace: each kernel file gets its own copy.
#pragma once
#include <type_traits>

#include "dl_internal.h"
#include "tile_ops.h"

namespace dl {
namespace {

// The CSR staged in LDS at a.csr_off: n_w weights (all nnz, or one row's when every row shares
// them), u16 columns, u16 row_ptr unless the graph is regular.
struct LdsCsr {
    float *lw;
    uint16_t *lcol;
    uint16_t *lrp;
    int reg;        // a.regular
    bool wshared;   // weight of entry e is lw[e - e0]
    // regular rows of 5 entries sharing one weight sequence (a degree-4 graph with uniform
    // weights: c2, c3, c4): the 5 weights in scalar registers from row 0's CSR, the row's 5
    // column ids and then its 5 tile values read back to back -- 6 LDS round trips a row
    // become 2 (the same products and sums in the same order: the same bits)
    bool reg5;
    float w5[5];
};

// reg5_ok: the kernel folds from this CSR at <= 4 rows per thread (beyond, the five values per
// row do not fit beside the prefetch registers)
__device__ __forceinline__ LdsCsr lds_csr(unsigned char *smem, const TileArgs &a, bool reg5_ok) {
    LdsCsr L;
    L.lw = reinterpret_cast<float *>(smem + a.csr_off);
    L.lcol = reinterpret_cast<uint16_t *>(smem + a.csr_off + 4u * (uint32_t)a.n_w);
    L.lrp = L.lcol + a.nnz;
    L.reg = a.regular;
    L.wshared = a.n_w != a.nnz;
    L.reg5 = reg5_ok && L.reg == 5 && L.wshared;
#pragma unroll
    for (int e = 0; e < 5; ++e) L.w5[e] = L.reg5 ? a.w[e] : 0.f;
    return L;
}

// Copy the CSR into LDS, the workgroup's threads striding; the caller's next barrier publishes it.
__device__ __forceinline__ void stage_csr(const LdsCsr &L, const TileArgs &a, int tid) {
    constexpr int NT = kTileThreads;
    for (int i = tid; i < a.n_w; i += NT) L.lw[i] = a.w[i];
    for (int i = tid; i < a.nnz; i += NT) L.lcol[i] = (uint16_t)a.col[i];
    if (!a.regular)
        for (int i = tid; i <= a.n_rows; i += NT) L.lrp[i] = (uint16_t)a.rowptr[i];
}

// y_a = sum_e w_e * src_{col_e} for agent ag, chunk c of the LDS image src ([rows][C] float4):
// left fold in CSR order from +0.0 (mixer.py:47); reads only LDS.
template <int C>
__device__ __forceinline__ float4 csr_fold(const LdsCsr &L, const float4 *src, int ag, int c) {
    if (L.reg5) {
        uint32_t ci[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) ci[e] = L.lcol[ag * 5 + e];
        float4 v[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) v[e] = src[ci[e] * C + c];
        float4 acc = zero4();
#pragma unroll
        for (int e = 0; e < 5; ++e) axpy4(acc, L.w5[e], v[e]);
        return acc;
    }
    int e0, e1;
    if (L.reg) {
        e0 = ag * L.reg;
        e1 = e0 + L.reg;
    } else {
        e0 = L.lrp[ag];
        e1 = L.lrp[ag + 1];
    }
    const float *wr = L.wshared ? L.lw - e0 : L.lw;
    float4 acc = zero4();
    for (int e = e0; e < e1; ++e) axpy4(acc, wr[e], src[L.lcol[e] * C + c]);
    return acc;
}

// Column mean of the tile over all agents from per-thread partial sums: thread -> wave (lanes
// with the same c) -> LDS scratch -> every thread sums the 16 wave partials in order (reading
// them once per wave and adding across the wave's slot lanes with shuffles instead measured no
// faster, profiles/r12).  In two halves, because the mean-from-inputs path puts the staging
// barrier and the next tile's prefetch between them.
template <int C>
__device__ __forceinline__ void col_sums_to_scratch(float4 cs, float4 *scratch, int tid) {
#pragma unroll
    for (int m = C; m < 64; m <<= 1) cs = shfl_xor4(cs, m);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane < C) scratch[wave * C + lane] = cs;
}

template <int C>
__device__ __forceinline__ float4 col_sums_from_scratch(const float4 *scratch, int c) {
    float4 sum = zero4();
#pragma unroll
    for (int wv = 0; wv < kTileThreads / 64; ++wv) add4(sum, scratch[wv * C + c]);
    return sum;
}

__device__ __forceinline__ float4 div4(float4 v, float n) {
    v.x = v.x / n;
    v.y = v.y / n;
    v.z = v.z / n;
    v.w = v.w / n;
    return v;
}

template <int C>
__device__ __forceinline__ float4 tile_mean(float4 cs, float4 *scratch, int tid, int c, int n) {
    col_sums_to_scratch<C>(cs, scratch, tid);
    __syncthreads();
    return div4(col_sums_from_scratch<C>(scratch, c), (float)n);
}

// Per-agent ||y - mean||^2 accumulators of a thread's KV passes, spread over the C lanes of a
// row group: lane c keeps the passes k with k % C == c (slot k / C), so ceil(KV / C) registers
// instead of KV.
// LD (dev_per_lane): each lane instead keeps its own chunk's partial of every pass's row, and the
// row group's C lanes are summed ONCE, after the last tile -- no cross-lane reduction per pass
// and tile (log2 C ds_bpermutes per pass: at c3's 256 x 164,608 round they were 20-30 us of a
// 117-us launch, scripts/c3_scale_probe.py)
constexpr bool dev_per_lane(int C, int KV) { return C > 1 && KV <= 4; }
constexpr int dev_slots(int C, int KV) { return KV <= C ? 1 : KV / C; }

template <int C, int KV, bool LD>
struct DevAcc {
    float dacc[dev_slots(C, KV)];
    float ldev[LD ? KV : 1];
};

template <int C, int KV, bool LD>
__device__ __forceinline__ void dev_zero(DevAcc<C, KV, LD> &d) {
#pragma unroll
    for (int k = 0; k < dev_slots(C, KV); ++k) d.dacc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < (LD ? KV : 1); ++k) d.ldev[k] = 0.f;
}

// sum over the C lanes of a row group
template <int C>
__device__ __forceinline__ float row_group_sum(float v) {
#pragma unroll
    for (int m = 1; m < C; m <<= 1) v = xor_add(v, m);
    return v;
}

// k may be a runtime pass index (a select per register)
template <int C, int KV, bool LD>
__device__ __forceinline__ void dev_add(DevAcc<C, KV, LD> &d, int k, float4 y, float4 mean, int c) {
    const float dx = y.x - mean.x, dy = y.y - mean.y;
    const float dz = y.z - mean.z, dw = y.w - mean.w;
    float v = (dx * dx + dy * dy) + (dz * dz + dw * dw);
    if constexpr (LD) {
#pragma unroll
        for (int j = 0; j < KV; ++j) d.ldev[j] += j == k ? v : 0.f;
        return;
    }
    v = row_group_sum<C>(v);
    const bool mine = (k % C) == c;
#pragma unroll
    for (int j = 0; j < dev_slots(C, KV); ++j) d.dacc[j] += (mine && j == k / C) ? v : 0.f;
}

// After the last tile: this workgroup's partials of rows [skip, n_rows) to a.dev_partial (rows
// below `skip` belong to other lanes: mix_tile.hip's hub rows), and workgroup 0 clears
// a.dev_max_zero.
template <int C, int KV, bool LD>
__device__ __forceinline__ void dev_epilogue(const DevAcc<C, KV, LD> &d, const TileArgs &a,
                                             int tid, int n_rows, int skip = 0) {
    constexpr int SLOTS = kTileThreads / C;
    const int c = tid & (C - 1), s = tid / C;
    if constexpr (LD) {
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const float v = row_group_sum<C>(d.ldev[k]);
            const int ag = s + k * SLOTS;
            if (c == 0 && ag < n_rows && !(ag < skip))
                a.dev_partial[(int64_t)blockIdx.x * n_rows + ag] = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < dev_slots(C, KV); ++j) {
            const int k = j * C + c;  // the pass this lane's slot j holds
            const int ag = s + k * SLOTS;
            if (k < KV && ag < n_rows && !(ag < skip))
                a.dev_partial[(int64_t)blockIdx.x * n_rows + ag] = d.dacc[j];
        }
    }
    if (a.dev_max_zero != nullptr && blockIdx.x == 0 && tid == 0) *a.dev_max_zero = 0u;
}

// byte address of tile t's first element (row 0) in an operand of tile stride ts; grp: data tiles
// per kernel tile (TileArgs::grp)
__device__ __forceinline__ const char *tile_base(const TileArgs &a, const void *p, int64_t ts,
                                                 int tile_id, int grp = 1) {
    return reinterpret_cast<const char *>(p) + (a.tiled ? 0 : a.col_base * 4) +
           (int64_t)tile_id * grp * ts;
}

// A workgroup's tiles: id, id + step, ... below end (TileArgs::tile_run)
struct TileWalk {
    int id, end, step;
};

__device__ __forceinline__ TileWalk tile_walk(const TileArgs &a) {
    const int trun = a.tile_run;
    TileWalk t;
    t.id = trun ? (int)blockIdx.x * trun : (int)blockIdx.x;
    t.end = trun ? min(t.id + trun, a.n_tiles) : a.n_tiles;
    t.step = trun ? 1 : (int)gridDim.x;
    return t;
}

// One output chunk of row ag.  FAST: a buffer store at byte offset `off` of the tile's resource
// ry, its cache policy a.nt_store; else guarded scalar stores at column `col` of a.y's row.
template <bool FAST>
__device__ __forceinline__ void store_y(const TileArgs &a, __amdgpu_buffer_rsrc_t ry, uint32_t off,
                                        int ag, int64_t col, const float4 &y) {
    if (FAST) {
        if (a.nt_store)
            buf_st4<kBufNT>(y, ry, off);
        else
            buf_st4<0>(y, ry, off);
    } else {
        st4(a.y + (int64_t)ag * a.ldy, col, a.n_params, false, y);
    }
}

// Host side: f(std::integral_constant<int, C>{}) for chunks = C in {1, 2, 4, ..., kMaxChunks}
template <class F>
hipError_t with_chunks(int chunks, F &&f) {
    switch (chunks) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        default: return hipErrorInvalidValue;
    }
}

// ... and f(std::integral_constant<int, KV>{}) for plan.h tile_passes' 2, 4 or 8 rows per thread
template <class F>
hipError_t with_passes(int kv, F &&f) {
    if (kv <= 2) return f(std::integral_constant<int, 2>{});
    if (kv <= 4) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 8>{});
}

}  // namespace
}  // namespace dl
