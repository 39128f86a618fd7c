// Kernel-configuration planner of the gossip rounds: host-only C++17, no HIP.  Pure functions of
// (args, compute units, knobs); the C ABI (capi.hip) supplies the device's CU count and the
// environment, the kernel files share the geometry helpers, so host and kernel cannot disagree.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dlamd.h"

namespace dl {

constexpr int kTileThreads = 1024;      // 16 waves: one workgroup per CU owns a column tile
constexpr int kRowsPerThread = 8;       // prefetch depth: rows x chunks <= 8 * 1024 float4
constexpr int kLdsBytes = 163840;       // 160 KiB LDS per CU on gfx950
constexpr int kMaxChunks = 32;          // T <= 128 columns per tile
constexpr int kErrLen = 512;            // bytes of the planners' error text buffer

// Every environment knob the planner and the launch shaping (launch.h) read.  read_knobs() fills
// it once per ABI call (not cached: tests and scripts set the variables after the library is
// loaded).
struct Knobs {
    int grid_mult = 2;            // DLAMD_GRID_MULT, clamped to 1..8
    bool grid_mult_set = false;   // ... was given: it then applies to short launches too
    int wg_per_cu = 2;            // DLAMD_WG_PER_CU=1: one workgroup per CU
    bool balance_grid = true;     // DLAMD_BALANCE_GRID=0: keep the full grid
    bool force_reg = false;       // DLAMD_FORCE_REG=1 (tests): paths 4 / 5 wherever they apply
    bool force_gather = false;    // DLAMD_FORCE_GATHER=1 (tests): path 2; wins over force_reg
    int max_tile_chunks = 0;      // DLAMD_MAX_TILE_CHUNKS=c: row-major tiles of <= 4c columns
    int tile_group = 8;           // DLAMD_TILE_GROUP=g: halo tile groups of <= g tiles (1: off)
    bool trace_planes = false;    // DLAMD_TRACE_PLANES set: the chunk-major traced kernel
    int nt_store = -1;            // DLAMD_NT_STORE=0 / other: plain / non-temporal stores of y
    int nt_load = 3;              // DLAMD_NT_LOAD=0 / x / g / other: nt_load 0 / 1 / 2 / 3
    int lds_min = 0;              // DLAMD_LDS_MIN=b: at least b bytes of LDS per tile workgroup
    int tile_run = -1;            // DLAMD_TILE_RUN=1 / other: contiguous tile runs on / off
    bool gather_order_columns = false;   // DLAMD_GATHER_ORDER=c...: the column-fastest gather grid
};
Knobs read_knobs();
// Writes the dl_last_error() text of a refusal into err[kErrLen] and returns code.
int fail(char *err, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

struct Plan {
    dl_mix_plan pub;
    int chunks;
    bool dev;
    uint32_t csr_off, scratch_off;
    int head;       // path 5: CSR entries per row in registers (the rest in LDS)
    int tail_fmt;   // path 5: LDS tail entries of 8 B (2) or 6 B (1)
    int grp;        // path 1, column-tiled: data tiles per kernel tile (0 / 1: one)
};

// dl_mix_rounds_trace configuration: one agent per thread, C float4 column chunks per step.
struct TracePlan {
    int32_t max_rounds;  // rounds per traced pass (the per-round deviations live in VGPRs)
    int32_t grid, chunks;
    int64_t n_steps;
    uint32_t csr_off, scratch_off, lds;
    int32_t irr;   // 1: mix_trace_irr_kernel (one image, register head + LDS tail)
    int32_t head;  // irr: CSR entries per row in registers
    int32_t gm;    // irr: W not doubly stochastic, every round's mean from its outputs
    int32_t narrow;  // irr: 2-column steps, 6-byte tail entries
};

// The planners return a dl_status and, on failure, the dl_last_error() text in err[kErrLen].
int plan_mix(const dl_mix_args &a, int n_cus, const Knobs &k, Plan *pl, char *err);
int plan_rounds(const dl_mix_args &a, int n_cus, const Knobs &k, Plan *pl, char *err);
int plan_trace(const dl_mix_args &a, int n_cus, const Knobs &k, TracePlan *tp, char *err);
// Column-tiled width (4 x chunks, 0: not tileable) for R = every source row, local + halo.
int choose_tile_cols(const dl_csr &W, int32_t n_halo, int64_t n_params, bool want_dev,
                     const Knobs &k);
// Upper bound of per-workgroup partial rows any path writes.
int max_parts(int n_cus, const Knobs &k);
int next_pow2_chunks(int64_t n_params);

// Local source rows of a round: n_local_src, or n_rows when 0 (dlamd.h).
inline int32_t local_src(const dl_mix_args &a) {
    return a.n_local_src > 0 ? a.n_local_src : a.W.n_rows;
}

// LDS of a tile workgroup: `images` tile images of rows x chunks float4, then the staged CSR,
// then the 16 x chunks float4 mean scratch (want_dev).  The register-CSR kernels (paths 4 / 5)
// keep the scratch right behind the tile and path 5's LDS tail, at csr_off, behind that.
struct LdsLayout {
    int64_t tile;                  // bytes of one image
    int64_t csr_off, scratch_off;  // byte offsets
    int64_t total;
};
constexpr LdsLayout lds_layout(int64_t rows, int chunks, int64_t csr_bytes, bool want_dev,
                               int images = 1) {
    const int64_t tile = rows * chunks * 16;
    const int64_t scratch = want_dev ? (int64_t)(kTileThreads / 64) * chunks * 16 : 0;
    return {tile, images * tile, images * tile + csr_bytes, images * tile + csr_bytes + scratch};
}

// LDS bytes the staged CSR needs (0 if it cannot be staged: > 65535 rows/entries); n_w = weights
// staged (nnz, or the row degree when all rows share one weight sequence).
constexpr uint32_t csr_lds_bytes(int32_t n_rows, int32_t nnz, int32_t regular, int32_t n_w) {
    if (nnz > 65535 || n_rows > 65535) return 0;
    const uint32_t b = 4u * (uint32_t)n_w + 2u * (uint32_t)nnz +
                       (regular ? 0u : 2u * (uint32_t)(n_rows + 1));
    return (b + 15u) & ~15u;
}
struct CsrShape {
    int regular;    // 1: every row has uniform_row_nnz entries (row_ptr not staged)
    int32_t n_w;    // weights staged: nnz, or the row degree with shared row weights
    uint32_t lds;   // csr_lds_bytes of it
    bool in_regs;   // degree-4 regular with shared weights: the multi-round kernels' register CSR
};
constexpr CsrShape csr_shape(const dl_csr &W) {
    const int reg = W.uniform_row_nnz > 0 ? 1 : 0;
    const int32_t n_w = (reg && W.shared_row_weights) ? W.uniform_row_nnz : W.nnz;
    return {reg, n_w, csr_lds_bytes(W.n_rows, W.nnz, reg, n_w), W.uniform_row_nnz == 5 && n_w == 5};
}

// Row passes n_src rows need at `chunks` float4 per row, and the rows per thread (KV) the FAST
// tile kernels run for them (the guarded kernels always run kRowsPerThread).
constexpr int row_passes(int chunks, int n_src) {
    return (n_src + kTileThreads / chunks - 1) / (kTileThreads / chunks);
}
constexpr int tile_passes(int chunks, int n_src, bool fast) {
    const int need = row_passes(chunks, n_src);
    return !fast ? kRowsPerThread : need <= 2 ? 2 : need <= 4 ? 4 : 8;
}
// ... and of launch_mix_tile: a column-tiled halo mix of exactly 3 row passes (c4 at 8 GPUs: 512
// + 96 rows at C = 4; at 2 GPUs 2048 + 128 rows at C = 1) runs three passes instead of four, up
// to C = 8: the fourth would only re-read row 0 (45 % of the staging loads dead at 608 rows,
// 47 % at 2176)
constexpr int tile_kv(int chunks, int n_src, bool fast, bool tiled_halo_mix) {
    return fast && tiled_halo_mix && chunks <= 8 && row_passes(chunks, n_src) == 3
               ? 3 : tile_passes(chunks, n_src, fast);
}
// Two 1024-thread workgroups share a CU only at <= 64 VGPRs.  Of the column-tiled halo (HALO =
// 2) instantiations, those of C >= 8 at <= 3 rows per thread without the lagged deviation are
// compiled to that (53-64 VGPRs, no spills); every other one takes 66-123
// (profiles/r13/vgprs.txt), so a grid sized for two would only queue them (rank-of 4 / 2 halo
// mix 1.5 / 2 % slower, profiles/r12/halo_grid/).
constexpr bool halo_two_per_cu(int C, int KV, bool lag) { return C >= 8 && KV <= 3 && !lag; }

// Tile kernel with the CSR in registers (regular graphs of 5 entries per row whose CSR does not
// fit LDS beside the tile): FAST path only, no halo, chunks 1, <= 4 rows per thread.
constexpr bool reg_csr_supported(int chunks, int n_rows, int regular, int n_halo) {
    return regular == 5 && n_halo == 0 && chunks == 1 && tile_passes(chunks, n_rows, true) <= 4;
}
// ... and its irregular form: every row has >= min_row_nnz entries; the first reg_head_rows()
// of each row in registers, the remaining nnz - head * n_rows entries in LDS
constexpr int reg_head_rows(int min_row_nnz) {   // 5, 3, 2 or 0 (no register head)
    return min_row_nnz >= 5 ? 5 : min_row_nnz >= 3 ? 3 : min_row_nnz >= 2 ? 2 : 0;
}
constexpr bool reg_tail_supported(int chunks, int n_rows, int head, int n_halo) {
    return head > 0 && n_halo == 0 && chunks == 1 && tile_passes(chunks, n_rows, true) <= 4;
}

// Rounds per traced pass (the per-round deviations live in VGPRs): 32 on the planes kernel;
// mix_trace_rows_kernel at 4 agents per thread keeps 4 agents' CSR offsets and prefetch
// registers, so 24 (122 VGPRs, no spills); mix_trace_wide_kernel (1024 < N <= 4096 agents, one
// chunk per step, KV = 2 or 4 agents per thread) keeps KV x rounds: 16 at KV = 2, 8 at KV = 4
// (12 spilled 20-30 VGPRs there)
constexpr int kTraceRounds = 32;
constexpr int kRowsTraceRounds = 24;
constexpr int kWideTraceRounds2 = 16;
constexpr int kWideTraceRounds4 = 8;
constexpr int wide_trace_rounds(int n_rows) {
    return n_rows > 2 * kTileThreads ? kWideTraceRounds4 : kWideTraceRounds2;
}
// the agent-major traced kernel serves register-cached regular graphs at C = 4; `planes`
// (Knobs::trace_planes) keeps the chunk-major planes kernel (comparison runs)
constexpr bool trace_uses_rows(int n_rows, bool in_regs, int chunks, bool planes) {
    return in_regs && chunks == 4 && n_rows <= kTileThreads && !planes;
}
constexpr int trace_max_rounds(int n_rows, bool in_regs, int chunks, bool planes) {
    if (n_rows > kTileThreads) return wide_trace_rounds(n_rows);
    return trace_uses_rows(n_rows, in_regs, chunks, planes) && n_rows > kTileThreads / 2
               ? kRowsTraceRounds : kTraceRounds;
}
// mix_trace_irr_kernel: KV agents per thread, irr_trace_rounds(KV) rounds per pass
constexpr int irr_trace_kv(int n_rows) {
    return n_rows <= kTileThreads ? 1 : n_rows <= 2 * kTileThreads ? 2 : 4;
}
constexpr int irr_trace_rounds(int kv) { return kv == 1 ? 24 : kv == 2 ? 12 : 4; }

}  // namespace dl
