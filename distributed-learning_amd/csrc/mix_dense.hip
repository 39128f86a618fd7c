// Dense-W consensus round for gfx950 (MI355X) on the fp32 matrix cores: X' = Wd S for a dense
// row-major Wd[N][N], 2 <= N <= 256 -- complete graphs, powers and products of W, learned weights.
// For every column p:
//   s_j[p] = x_j[p], or fl(x_j[p] - fl(lr g_j[p])) with g      (dl_mix_round's local step)
//   acc = +0.0;  for k = 0 .. N-1: acc = fmaf(Wd[a][k], s_k[p], acc);  y_a[p] = acc
// which is oracle/mix_ref.c ref_bgemm(1, N, P, N, Wd, S): v_mfma_f32_16x16x4_f32 is a k-ordered
// fp32 fma chain (tests/test_bgemm_gpu.py) and k ascends within every accumulator here.
// Every Wd[a][k] takes part, a zero included: a non-finite s_k reaches every row as NaN (the
// sparse rounds skip non-neighbours).  The sign of a sum that underflows to zero and subnormal
// operands are unspecified.
//
// Design.  Not a tile_core.h kernel: no CSR, 512 threads (8 waves, 2 a SIMD, so a wave may hold
// 256 VGPRs).  N is padded to NP in {32, 64, 128, 256}.  Persistent workgroups walk column tiles
// of TMAX = 128 columns (64 at NP = 256); a tile of all N rows of S lives in LDS as
// [NP][TMAX + 16] fp32.
//   W in registers: the NP / 16 row blocks are dealt to WR = min(NP / 16, 8) waves, RB = 1 or 2
//     blocks each; a wave loads its blocks' fragments for ALL k (RB x NP / 4 registers a lane,
//     128 at NP = 256) once, before its first tile, and keeps them: per tile only x, g and y
//     cross HBM.  Pad rows and pad columns of W are zero registers, pad rows of the LDS image are
//     zeroed once, so a pad term is fma(0, 0, acc); pad rows are never stored.
//   Column split: with fewer than 8 row blocks the 8 / WR wave groups take every (8 / WR)-th
//     16-column block of the tile, so all waves have work at N <= 64.
//   Operand order: S is the MFMA's A operand and W its B operand (products commute, the chain is
//     the same), so the accumulator of lane l holds row l % 16 x columns 4 (l / 16) .. + 3: one
//     float4 store a lane, 64 contiguous bytes a row and column block.
//   LDS banks: the S fragment is lane (k = l / 16, n = l % 16) reading row k0 + k, column n0 + n.
//     At a pitch of T = 64 or 128 floats the four k groups of a wave fall on the same 16 banks
//     (a 4-way conflict on every read); the pitch TMAX + 16 = 16 (mod 64) puts them on banks
//     [0,16) [16,32) [32,48) [48,64): none left.  The staging writes are float4s along a row.
//   Staging: float4 buffer loads of x and g go out one tile ahead, right behind the staging
//     barrier, with the round kernels' non-temporal policy (tile_ops.h); the local step is applied
//     as the tile is written to LDS.  When no tile follows the prefetch registers are cleared
//     (mix_track.hip: dead values are then not carried round the loop).
//   Layouts: a column-tiled operand's data tile of T = 16 m <= 128 columns is walked as
//     ceil(T / TMAX) kernel tiles (two at NP = 256, T > 64); row-major operands of any ld.  FAST:
//     16-byte aligned operands, whole tiles, 32-bit offsets.  Guarded: scalar accesses with
//     64-bit addresses, columns past the end zero in LDS and never written; no prefetch.
//   Left undone: two column blocks a wave at a time (independent chains at RB = 1), 128-byte
//     store segments, a fused deviation.
//
// VGPRs (make resource RES_SRC=mix_dense.hip; no instantiation uses scratch), FAST / guarded:
// NP = 32: 43 / 37, 64: 81 / 49, 128: 152 / 65, 256: 251 / 164; LDS 18, 36, 72, 80 KiB.
#include <type_traits>

#include "dl_internal.h"
#include "tile_ops.h"

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

template <int NP, bool FAST>
__global__ void __attribute__((amdgpu_flat_work_group_size(kDenseThreads, kDenseThreads)))
mix_dense_kernel(DenseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *img = reinterpret_cast<float *>(smem);
    constexpr int TMAX = dense_tmax(NP);
    constexpr int PITCH = dense_pitch(NP);
    constexpr int C4 = TMAX / 4;                 // float4 chunks of a tile row
    constexpr int SLOTS = kDenseThreads / C4;    // rows staged per pass
    constexpr int KV = NP / SLOTS;               // passes: float4s of x (and of g) a thread holds
    constexpr int KS = NP / 4;                   // MFMA k steps
    constexpr int NRB = NP / 16;                 // row blocks
    constexpr int WR = NRB < 8 ? NRB : 8;        // waves along the rows
    constexpr int RB = NRB / WR;                 // row blocks a wave
    constexpr int CG = 8 / WR;                   // wave groups along the columns
    static_assert(KV * SLOTS == NP && RB * WR == NRB && CG * WR == 8, "geometry");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave % WR, wc = wave / WR;
    const int N = a.n_rows;
    const int c = tid % C4, s = tid / C4;
    const bool sgd = a.g != nullptr;
    const float lr = a.lr;
    const int T = a.tile_cols, sub = a.sub;

    // this wave's W fragments: lane (j = l % 16, k = l / 16) of row block b, k step ks holds
    // Wd[16 b + j][4 ks + k], zero outside N x N
    float af[RB][KS];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        const int row = 16 * (wr * RB + i) + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = 4 * ks + (lane >> 4);
            af[i][ks] = (row < N && k < N) ? a.w[(int64_t)row * a.ldw + k] : 0.f;
        }
    }
    // pad rows of the image, once: staging writes rows < N only
    for (int i = tid; i < (NP - N) * PITCH; i += kDenseThreads) img[N * PITCH + i] = 0.f;

    // FAST byte offsets inside a tile: lane row s / chunk c; pass k adds k * step
    const uint32_t ox = (uint32_t)s * (uint32_t)a.xrs + 16u * (uint32_t)c;
    const uint32_t sx = (uint32_t)SLOTS * (uint32_t)a.xrs;
    const uint32_t og = (uint32_t)s * (uint32_t)a.grs + 16u * (uint32_t)c;
    const uint32_t sg = (uint32_t)SLOTS * (uint32_t)a.grs;

    // kernel tile kt of this launch: data tile dt, sub-tile h of TMAX columns
    auto tile_off = [&](int kt, int64_t ts, int &width) {
        const int64_t gk = a.tile0 + kt;
        const int64_t dt = gk / sub;
        const int h = (int)(gk - dt * sub);
        width = min(TMAX, T - h * TMAX);
        return dt * ts + (int64_t)h * TMAX * 4;
    };

    float4 px[FAST ? KV : 1], pg[FAST ? KV : 1];
    using PNT = std::integral_constant<int, kBufNT>;
    using PPL = std::integral_constant<int, 0>;
    auto prefetch = [&](int kt) {
        if constexpr (FAST) {
            int width;
            const int64_t xo = tile_off(kt, a.xts, width);
            const int64_t go = tile_off(kt, a.gts, width);
            const bool cok = 4 * c < width;
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(reinterpret_cast<const char *>(a.x) + xo);
            const __amdgpu_buffer_rsrc_t rg = buf_rsrc(
                sgd ? reinterpret_cast<const char *>(a.g) + go
                    : reinterpret_cast<const char *>(a.x) + xo);
            // one straight-line loop per load policy (bit 0: x non-temporal, bit 1: g); a lane
            // without an element reads the tile's first 16 bytes
            auto loads = [&](auto ax, auto ag) {
#pragma unroll
                for (int k = 0; k < KV; ++k) {
                    const bool ok = cok && s + k * SLOTS < N;
                    px[k] = buf_ld4<decltype(ax)::value>(rx, ok ? ox + k * sx : 0u);
                }
                if (sgd) {
#pragma unroll
                    for (int k = 0; k < KV; ++k) {
                        const bool ok = cok && s + k * SLOTS < N;
                        pg[k] = buf_ld4<decltype(ag)::value>(rg, ok ? og + k * sg : 0u);
                    }
                }
            };
            if (a.nt_load == 3) loads(PNT{}, PNT{});
            else if (a.nt_load == 1) loads(PNT{}, PPL{});
            else if (a.nt_load == 2) loads(PPL{}, PNT{});
            else loads(PPL{}, PPL{});
        }
    };
    auto clear = [&]() {
#pragma unroll
        for (int k = 0; k < (FAST ? KV : 1); ++k) px[k] = pg[k] = zero4();
    };
    clear();

    const int n_tiles = a.n_tiles;
    int kt = blockIdx.x;
    if (kt < n_tiles) prefetch(kt);
    for (; kt < n_tiles; kt += gridDim.x) {
        int width;
        const int64_t yo = tile_off(kt, a.yts, width);
        const int64_t gk = a.tile0 + kt;
        const int64_t col0 = (gk / sub) * T + (gk % sub) * TMAX;   // the tile's first column
        // columns of this tile that exist (guarded: a ragged last tile), in 16-column blocks
        const int live = FAST ? width : (int)min((int64_t)width, a.col_end - col0);
        const int ncb = (live + 15) >> 4;
        // stage the stepped tile
        if constexpr (FAST) {
#pragma unroll
            for (int k = 0; k < KV; ++k) {
                const int r = s + k * SLOTS;
                if (r < N && 4 * c < width)
                    *reinterpret_cast<float4 *>(img + r * PITCH + 4 * c) =
                        sgd ? local_step(px[k], pg[k], lr) : px[k];
            }
        } else {
            int w2;
            const int64_t xo = tile_off(kt, a.xts, w2), go = tile_off(kt, a.gts, w2);
#pragma unroll 1
            for (int k = 0; k < KV; ++k) {
                const int r = s + k * SLOTS;
                if (r < N && 4 * c < width) {
                    const int64_t col = col0 + 4 * c;
                    const float4 x = ld4_guard(reinterpret_cast<const char *>(a.x) + xo +
                                                   (int64_t)r * a.xrs + 16 * c, col, a.col_end);
                    const float4 g = sgd ? ld4_guard(reinterpret_cast<const char *>(a.g) + go +
                                                         (int64_t)r * a.grs + 16 * c, col, a.col_end)
                                         : zero4();
                    *reinterpret_cast<float4 *>(img + r * PITCH + 4 * c) =
                        sgd ? local_step(x, g, lr) : x;
                }
            }
        }
        __syncthreads();
        // the next tile's loads go out first: they land while the matrix cores run from LDS
        const int nxt = kt + (int)gridDim.x;
        if (nxt < n_tiles) prefetch(nxt);
        else clear();

        if (16 * wr * RB < N) {   // (a wave whose row blocks are all padding has nothing to store)
            char *yt = reinterpret_cast<char *>(a.y) + yo;
            const __amdgpu_buffer_rsrc_t ry = buf_rsrc(yt);
#pragma unroll 1
            for (int cb = wc; cb < ncb; cb += CG) {
                f32x4 acc[RB];
#pragma unroll
                for (int i = 0; i < RB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                const float *bp = img + (lane >> 4) * PITCH + 16 * cb + (lane & 15);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const float b = bp[ks * 4 * PITCH];
#pragma unroll
                    for (int i = 0; i < RB; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b, af[i][ks], acc[i], 0, 0, 0);
                }
                // lane l: row 16 b + l % 16, columns 16 cb + 4 (l / 16) .. + 3
                const int cc = 16 * cb + 4 * (lane >> 4);
#pragma unroll
                for (int i = 0; i < RB; ++i) {
                    const int row = 16 * (wr * RB + i) + (lane & 15);
                    if (row >= N) continue;
                    const float4 y = make_float4(acc[i].x, acc[i].y, acc[i].z, acc[i].w);
                    if constexpr (FAST) {
                        const uint32_t off = (uint32_t)row * (uint32_t)a.yrs + 4u * (uint32_t)cc;
                        if (a.nt_store) buf_st4<kBufNT>(y, ry, off);
                        else buf_st4<0>(y, ry, off);
                    } else {
                        float *f = reinterpret_cast<float *>(yt + (int64_t)row * a.yrs + 4 * cc);
                        const int64_t col = col0 + cc;
                        if (col < a.col_end) f[0] = y.x;
                        if (col + 1 < a.col_end) f[1] = y.y;
                        if (col + 2 < a.col_end) f[2] = y.z;
                        if (col + 3 < a.col_end) f[3] = y.w;
                    }
                }
            }
        }
        __syncthreads();  // the image is rewritten by the next iteration
    }
}

template <int NP>
hipError_t launch_np(const DenseArgs &a, bool fast, int grid, hipStream_t s) {
    auto go = [&](auto k) {
        hipError_t e = allow_full_lds(reinterpret_cast<const void *>(k));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(grid), dim3(kDenseThreads), dense_lds_bytes(NP), s, a);
        return hipGetLastError();
    };
    return fast ? go(mix_dense_kernel<NP, true>) : go(mix_dense_kernel<NP, false>);
}

}  // namespace

hipError_t launch_mix_dense(const DenseArgs &a, int n_pad, bool fast, int grid, hipStream_t s) {
    if (a.n_rows < 2 || a.n_rows > n_pad || grid < 1 || a.n_tiles < 1 || a.sub < 1 ||
        a.tile_cols < 16 || a.tile_cols % 16 || a.tile_cols > a.sub * dense_tmax(n_pad))
        return hipErrorInvalidValue;
    switch (n_pad) {
        case 32: return launch_np<32>(a, fast, grid, s);
        case 64: return launch_np<64>(a, fast, grid, s);
        case 128: return launch_np<128>(a, fast, grid, s);
        case 256: return launch_np<256>(a, fast, grid, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dl
