// Banded consensus round for gfx950 (MI355X): Y = W (X - lr G) for a sparse W with locality and
// ANY row count -- the graphs whose column tile of all agents does not fit one workgroup's LDS
// (more than 8192 agents: 128 x 128 tori, long rings, geometric graphs), which dl_mix_round hands
// to the L2 gather kernel.  dl_mix_round's rule, so its bits: for every column p
//   t_j[p] = x_j[p], or fl(x_j[p] - fl(lr g_j[p])) with g
//   acc = +0.0;  acc = fl(acc + fl(w_e t_col(e)[p])) over row a's entries in CSR order;  y_a[p] = acc
// (-ffp-contract=off: a separate multiply and add).
//
// Design.  Not a tile_core.h kernel: a block of consecutive rows reads only a window of source
// rows (include/dlamd.h dl_band_round_args: blocks, window segments, a u16 window slot per CSR
// entry, all made on the host by graph.band_blocks), so a workgroup stages a WINDOW, not all
// agents.
//   Work: an item is (block, tile of 4C columns).  Persistent 1024-thread workgroups; workgroup k
//     walks the k-th of gridDim.x equal contiguous runs of items in block-major order, so a run
//     stays in one block while its tiles last and the block's tables are staged once per run of
//     tiles, not once per item.
//   LDS (launch.h band_lds, the budget the host plan was grown against): the window image
//     [window rows][C] float4; the window's row map (global row of every slot); the block's CSR
//     slice -- weights, u16 slots, u16 row pointers relative to the slice, or with shared row
//     weights one weight sequence and the slots alone (10 B a row on a torus).
//   Staging: the image is linear in i = slot x C + chunk; thread tid takes i = tid + 1024 k.  FAST:
//     float4 buffer loads of x and g with the rounds' non-temporal policy (tile_ops.h), kBandPrefetch
//     passes at a time; the local step is applied on the way into LDS.  The next item's first
//     kBandPrefetch passes go out right behind the staging barrier and land under the fold; they
//     are cleared when no item of the same block follows (a new block's row map is not staged yet).
//   Fold: LDS only.  Thread tid owns (row, chunk) pairs i = tid + 1024 k of the block, walks the
//     row's entries in CSR order -- slot and weight from the slice, one ds_read_b128 of the image
//     per entry -- and stores one float4 of y.
//   Layouts: one kernel through two byte strides per operand (row-major: row stride 4 ld, tile
//     stride 16 C; column-tiled: row stride 16 C, tile stride rows x 16 C -- a window segment is
//     then one contiguous HBM run).  FAST: 16-byte aligned operands, whole tiles, row offsets in
//     32 bits.  Guarded: scalar accesses with 64-bit addresses, columns past the end zero in LDS
//     and never written; no prefetch.
//   Safety: every value read from the block table is clamped to the promises the LDS was sized by
//     and to W's sizes, so a wrong table gives wrong results, never an access out of bounds.
//   The deviation is NOT fused: a block does not see all agents.  dl_deviation(_tiled) runs after
//     the round (GossipEngine.deviation()).  Left undone: a sliding window that carries the rows two
//     consecutive blocks share, banded forms of the fused optimizer rounds.
//
// VGPRs (make resource RES_SRC=mix_band.hip; no instantiation uses scratch), shared row weights /
// general slice: FAST 95 / 87, guarded 52 / 59 (profiles/r29/band_round/vgprs.txt).
#include "dl_internal.h"
#include "tile_ops.h"

namespace dl {
namespace {

constexpr int KV = kBandPrefetch;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// x - lr*g with two roundings (mix_tile.hip's local step)
__device__ __forceinline__ float4 local_step(float4 x, float4 g, float lr) {
    float4 t;
    t.x = x.x - lr * g.x;
    t.y = x.y - lr * g.y;
    t.z = x.z - lr * g.z;
    t.w = x.w - lr * g.w;
    return t;
}

// 4 floats at p, element e read only when col + e < end (else 0); 4-byte aligned accesses
__device__ __forceinline__ float4 ld4_guard(const char *p, int64_t col, int64_t end) {
    const float *f = reinterpret_cast<const float *>(p);
    float4 v = zero4();
    if (col < end) v.x = f[0];
    if (col + 1 < end) v.y = f[1];
    if (col + 2 < end) v.z = f[2];
    if (col + 3 < end) v.w = f[3];
    return v;
}

template <bool FAST, bool SHARED>
__global__ void __attribute__((amdgpu_flat_work_group_size(kBandThreads, kBandThreads)))
mix_band_kernel(BandArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *img = reinterpret_cast<float4 *>(smem);
    int32_t *wmap = reinterpret_cast<int32_t *>(smem + a.map_off);
    float *wts = reinterpret_cast<float *>(smem + a.w_off);
    uint16_t *slots = reinterpret_cast<uint16_t *>(smem + a.slot_off);
    uint16_t *rp = reinterpret_cast<uint16_t *>(smem + a.rp_off);

    const int tid = threadIdx.x;
    const int lc = a.log2c, cm = (1 << lc) - 1;
    const int N = a.n_rows;
    const bool sgd = a.g != nullptr;
    const float lr = a.lr;
    const uint32_t xrs = (uint32_t)a.xrs, grs = (uint32_t)a.grs;   // FAST: they fit

    // this workgroup's run of items (the host launches gridDim.x <= n_items workgroups)
    const int64_t per = a.n_items / gridDim.x, rem = a.n_items % gridDim.x;
    const int64_t bid = blockIdx.x;
    int64_t it = bid * per + (bid < rem ? bid : rem);
    const int64_t end = it + per + (bid < rem ? 1 : 0);

    float4 px[FAST ? KV : 1], pg[FAST ? KV : 1];
    // FAST: passes [base, base + KV) of tile t's window into px / pg; a lane without an element
    // reads the tile's first 16 bytes
    auto issue = [&](int64_t t, int base, int wn) {
        if constexpr (FAST) {
            const __amdgpu_buffer_rsrc_t rx =
                buf_rsrc(reinterpret_cast<const char *>(a.x) + t * a.xts);
            uint32_t row[KV], ch[KV];
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int i = base + tid + k * kBandThreads;
                const bool ok = (i >> lc) < wn;
                row[k] = ok ? (uint32_t)wmap[i >> lc] : 0u;
                ch[k] = ok ? 16u * (uint32_t)(i & cm) : 0u;
            }
            // (two instructions per policy: tile_ops.h)
            if (a.nt_load & 1) {
#pragma unroll
                for (int k = 0; k < KV; ++k) px[k] = buf_ld4<kBufNT>(rx, row[k] * xrs + ch[k]);
            } else {
#pragma unroll
                for (int k = 0; k < KV; ++k) px[k] = buf_ld4<0>(rx, row[k] * xrs + ch[k]);
            }
            if (sgd) {
                const __amdgpu_buffer_rsrc_t rg =
                    buf_rsrc(reinterpret_cast<const char *>(a.g) + t * a.gts);
                if (a.nt_load & 2) {
#pragma unroll
                    for (int k = 0; k < KV; ++k) pg[k] = buf_ld4<kBufNT>(rg, row[k] * grs + ch[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < KV; ++k) pg[k] = buf_ld4<0>(rg, row[k] * grs + ch[k]);
                }
            }
        }
    };
    auto clear = [&]() {
#pragma unroll
        for (int k = 0; k < (FAST ? KV : 1); ++k) px[k] = pg[k] = zero4();
    };
    clear();

    int cur = -1, r0 = 0, nr = 0, wn = 0;
    bool have = false;
    for (; it < end; ++it) {
        const int b = (int)(it / a.n_tiles);
        const int tl = (int)(it - (int64_t)b * a.n_tiles);
        const int64_t t = a.tile0 + tl;
        if (b != cur) {
            // a new block (the barrier that ended the last item freed the tables): its rows, its
            // window's row map, its CSR slice.  Every table value is clamped.
            cur = b;
            have = false;
            r0 = clampi(a.block_row[b], 0, N);
            const int r1 = clampi(a.block_row[b + 1], r0,
                                  (int)min((int64_t)N, (int64_t)r0 + a.max_block));
            nr = r1 - r0;
            const int s0 = clampi(a.seg_ptr[b], 0, a.n_segments);
            const int s1 = clampi(a.seg_ptr[b + 1], s0, a.n_segments);
            wn = 0;
            for (int s = s0; s < s1 && wn < a.max_window; ++s) {
                const int first = a.seg_row[s];
                const int len = clampi(a.seg_len[s], 0, a.max_window - wn);
                for (int j = tid; j < len; j += kBandThreads)
                    wmap[wn + j] = clampi(first + j, 0, N - 1);
                wn += len;
            }
            const int top = wn > 0 ? wn - 1 : 0;   // (an empty window: slot 0 of a stale image)
            int e0, nn;
            if constexpr (SHARED) {
                e0 = (int)min((int64_t)r0 * a.degree, (int64_t)a.nnz);
                nn = (int)min((int64_t)nr * a.degree, (int64_t)min(a.max_slice, a.nnz - e0));
                nr = min(nr, nn / a.degree);
                for (int j = tid; j < a.degree; j += kBandThreads) wts[j] = a.w[j];
            } else {
                e0 = clampi(a.rowptr[r0], 0, a.nnz);
                nn = clampi(a.rowptr[r1] - e0, 0, min(a.max_slice, a.nnz - e0));
                for (int j = tid; j <= nr; j += kBandThreads)
                    rp[j] = (uint16_t)clampi(a.rowptr[r0 + j] - e0, 0, nn);
                for (int j = tid; j < nn; j += kBandThreads) wts[j] = a.w[e0 + j];
            }
            for (int j = tid; j < nn; j += kBandThreads)
                slots[j] = (uint16_t)min((int)a.slot[e0 + j], top);
            __syncthreads();   // the row map, before the staging reads it
        }
        const int cells = wn << lc;   // float4s of the image
        // stage the stepped window
        if constexpr (FAST) {
            for (int base = 0; base < cells; base += KV * kBandThreads) {
                if (base > 0 || !have) issue(t, base, wn);
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const int i = base + tid + k * kBandThreads;
                    if (i < cells) img[i] = sgd ? local_step(px[k], pg[k], lr) : px[k];
                }
            }
        } else {
            const char *xt = reinterpret_cast<const char *>(a.x) + t * a.xts;
            const char *gt = reinterpret_cast<const char *>(a.g) + t * a.gts;
            const int64_t col0 = t << (lc + 2);
            for (int i = tid; i < cells; i += kBandThreads) {
                const int64_t row = wmap[i >> lc];
                const int c = i & cm;
                const int64_t col = col0 + 4 * c;
                const float4 x = ld4_guard(xt + row * a.xrs + 16 * c, col, a.col_end);
                img[i] = sgd ? local_step(x, ld4_guard(gt + row * a.grs + 16 * c, col, a.col_end),
                                          lr)
                             : x;
            }
        }
        __syncthreads();
        // the next item's first loads go out now and land while the fold runs from LDS
        if constexpr (FAST) {
            have = it + 1 < end && tl + 1 < a.n_tiles;
            if (have) issue(t + 1, 0, wn);
            else clear();
        }
        // fold the block's rows
        char *yt = reinterpret_cast<char *>(a.y) + t * a.yts;
        const __amdgpu_buffer_rsrc_t ry = buf_rsrc(yt);
        const int outs = nr << lc;
        for (int i = tid; i < outs; i += kBandThreads) {
            const int row = i >> lc, c = i & cm;
            float4 acc = zero4();
            if constexpr (SHARED) {
                const uint16_t *sl = slots + row * a.degree;
                for (int e = 0; e < a.degree; ++e)
                    axpy4(acc, wts[e], img[((int)sl[e] << lc) + c]);
            } else {
                const int e1 = rp[row + 1];
                for (int e = rp[row]; e < e1; ++e)
                    axpy4(acc, wts[e], img[((int)slots[e] << lc) + c]);
            }
            if constexpr (FAST) {
                const uint32_t off = (uint32_t)(r0 + row) * (uint32_t)a.yrs + 16u * (uint32_t)c;
                if (a.nt_store) buf_st4<kBufNT>(acc, ry, off);
                else buf_st4<0>(acc, ry, off);
            } else {
                float *f = reinterpret_cast<float *>(yt + (int64_t)(r0 + row) * a.yrs + 16 * c);
                const int64_t col = (t << (lc + 2)) + 4 * c;
                if (col < a.col_end) f[0] = acc.x;
                if (col + 1 < a.col_end) f[1] = acc.y;
                if (col + 2 < a.col_end) f[2] = acc.z;
                if (col + 3 < a.col_end) f[3] = acc.w;
            }
        }
        __syncthreads();   // the image (and, at a block change, the tables) are rewritten next
    }
}

}  // namespace

hipError_t launch_mix_band(const BandArgs &a, bool fast, int grid, int lds, hipStream_t s) {
    if (grid < 1 || grid > a.n_items || a.n_tiles < 1 || a.n_blocks < 1 || a.max_window < 1 ||
        a.max_block < 1 || a.max_slice < 1 || lds < (int)a.rp_off || lds > kLdsBytes ||
        a.log2c < 0 || a.log2c > 5)
        return hipErrorInvalidValue;
    const bool shared = a.degree > 0;
    if (fast)
        return shared ? launch_lds(mix_band_kernel<true, true>, grid, lds, s, a)
                      : launch_lds(mix_band_kernel<true, false>, grid, lds, s, a);
    return shared ? launch_lds(mix_band_kernel<false, true>, grid, lds, s, a)
                  : launch_lds(mix_band_kernel<false, false>, grid, lds, s, a);
}

}  // namespace dl
