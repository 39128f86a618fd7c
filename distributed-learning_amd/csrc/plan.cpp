// The mix planner (plan.h): which kernel, tile width, grid and LDS layout a round gets.
#include "plan.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dl {

Knobs read_knobs() {
    auto is = [](const char *name, char c) {
        const char *v = getenv(name);
        return v && v[0] == c;
    };
    Knobs k;
    if (const char *m = getenv("DLAMD_GRID_MULT")) {
        const int v = atoi(m);
        k.grid_mult = v < 1 ? 1 : (v > 8 ? 8 : v);
        k.grid_mult_set = true;
    }
    k.wg_per_cu = is("DLAMD_WG_PER_CU", '1') ? 1 : 2;
    k.balance_grid = !is("DLAMD_BALANCE_GRID", '0');
    k.force_gather = is("DLAMD_FORCE_GATHER", '1');
    k.force_reg = is("DLAMD_FORCE_REG", '1') && !k.force_gather;
    if (const char *v = getenv("DLAMD_MAX_TILE_CHUNKS")) k.max_tile_chunks = atoi(v);
    if (const char *v = getenv("DLAMD_TILE_GROUP")) k.tile_group = atoi(v);
    k.trace_planes = getenv("DLAMD_TRACE_PLANES") != nullptr;
    if (const char *v = getenv("DLAMD_NT_STORE")) k.nt_store = v[0] == '0' ? 0 : 1;
    if (const char *v = getenv("DLAMD_NT_LOAD"))
        k.nt_load = v[0] == '0' ? 0 : v[0] == 'x' ? 1 : v[0] == 'g' ? 2 : 3;
    if (const char *v = getenv("DLAMD_LDS_MIN")) k.lds_min = atoi(v);
    if (const char *v = getenv("DLAMD_TILE_RUN")) k.tile_run = v[0] == '1' ? 1 : 0;
    k.gather_order_columns = is("DLAMD_GATHER_ORDER", 'c');
    return k;
}

int fail(char *err, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, kErrLen, fmt, ap);
    va_end(ap);
    return code;
}

int max_parts(int n_cus, const Knobs &k) {
    const int p = 2 * n_cus * k.grid_mult;
    return p < 256 ? 256 : p;
}

int next_pow2_chunks(int64_t n_params) {
    const int64_t need = (n_params + 3) / 4;
    int c = 1;
    while (c < kMaxChunks && c < need) c <<= 1;
    return c;
}

namespace {

uint32_t align256(size_t v) { return (uint32_t)((v + 255) & ~(size_t)255); }

// Workgroups per CU of a kernel using `lds` bytes (<= kLdsBytes): 1024 threads, so at most 2.
int wg_per_cu(int64_t lds, const Knobs &k) {
    const int bpc = (int)(kLdsBytes / lds);
    return bpc > k.wg_per_cu ? k.wg_per_cu : bpc;
}

// Workgroups of the one-round tile kernel per resident slot on the column-tiled layout: its
// persistent grid is oversubscribed 2x, the second half of the workgroups starting as the first
// ones retire.  Measured on MI355X (scripts/grid_sweep.py, profiles/r05/grid_sweep.log): the c2
// and c4 rounds stream at 5.90-5.93 TB/s with 2x against 5.28-5.41 TB/s with exactly one
// workgroup per CU, on the same box (3x: 5.74-5.80, 4x: 5.75-5.84).  Forcing one resident
// workgroup per CU through LDS changes nothing, so the gain is not co-residency.  Row-major
// operands (c3's N = 256 rows) keep one slot's grid (3247 vs 3206 steps/s).  The 2x grid pays on
// long persistent launches (c2 / c4: 128 tile passes per slot); on short ones (c3 column-tiled:
// 2572 tiles of 64 columns on 512 slots, 5 passes) the second wave of workgroups only adds its
// ramp: 105.3 vs 110.1 us with one slot's grid (scripts/c3_round_probe.py,
// profiles/r12/c3_round).  An explicit DLAMD_GRID_MULT=k (1..8) applies everywhere.
int grid_mult_for(int64_t n_tiles, int64_t slots, const Knobs &k) {
    return !k.grid_mult_set && n_tiles < 16 * slots ? 1 : k.grid_mult;
}

// Persistent grid for n_tiles tiles and at most gmax workgroups: the fewest workgroups that
// still finish in the same number of passes, so every workgroup walks ceil(n_tiles/gmax) or one
// fewer tiles.  The time of a persistent HBM-bound launch is its longest workgroup's tile
// count; with gmax workgroups and a ragged last pass (c3: 1286 tiles on 256 CUs = 6 passes for
// an average of 5.02) the idle CUs of that pass are pure tail.  Fewer, evenly loaded workgroups
// keep the same number of passes while each one gets a larger share of HBM.
// DLAMD_BALANCE_GRID=0 (a measurement knob) keeps gmax.
int64_t balanced_grid(int64_t n_tiles, int64_t gmax, const Knobs &k) {
    if (gmax <= 0) return 1;
    if (n_tiles <= gmax) return n_tiles;
    if (!k.balance_grid) return gmax;
    const int64_t passes = (n_tiles + gmax - 1) / gmax;
    return (n_tiles + passes - 1) / passes;
}

void fill(Plan *pl, int path, int64_t tile_cols, int64_t grid, int64_t n_tiles, int regular,
          int chunks, const LdsLayout &L) {
    pl->pub.path = path;
    pl->pub.tile_cols = (int32_t)tile_cols;
    pl->pub.grid = (int32_t)grid;
    pl->pub.lds_bytes = (int32_t)L.total;
    pl->pub.n_tiles = (int32_t)n_tiles;
    pl->pub.regular = regular;
    pl->chunks = chunks;
    pl->csr_off = (uint32_t)L.csr_off;
    pl->scratch_off = (uint32_t)L.scratch_off;
}

// LDS bytes of the register-head + LDS-tail tile kernel (path 5) for R rows at c chunks, or 0
// when it does not apply: the nnz - head * R tail entries behind the tile and the mean scratch,
// 8 B per entry ({weight, row} pairs, *fmt = 2) when that fits, else 6 B (weights + u16 rows,
// *fmt = 1; the only form at a 5-entry head, whose registers leave no room for the pairs'
// unrolled loop); the tail's u16 row map (setup only) must fit the tile area.
int64_t reg_tail_lds(const dl_csr &W, int32_t R, int c, bool want_dev, int *head_out = nullptr,
                     int *fmt_out = nullptr) {
    const int head = reg_head_rows(W.min_row_nnz);
    if (W.uniform_row_nnz == 5 || !reg_tail_supported(c, R, head, 0)) return 0;
    const int64_t ntail = (int64_t)W.nnz - (int64_t)head * R;
    if (ntail < 0 || ntail > 65535) return 0;
    const LdsLayout L = lds_layout(R, c, 0, want_dev);
    if (L.tile > 65536 || 2 * ntail > L.tile) return 0;
    for (int fmt = head < 5 ? 2 : 1; fmt >= 1; --fmt) {
        const int64_t lds = L.total + (((fmt == 2 ? 8 : 6) * ntail + 15) & ~(int64_t)15);
        if (lds > kLdsBytes) continue;
        if (head_out) *head_out = head;
        if (fmt_out) *fmt_out = fmt;
        return lds;
    }
    return 0;
}

// R = every source row (local + halo); halo rounds have no register-CSR kernels
int choose_tiled_chunks(const dl_csr &W, int32_t R, uint32_t csr, bool want_dev, bool halo,
                        const Knobs &k) {
    if (R > 65535) return 0;
    const bool reg_csr = reg_csr_supported(1, R, W.uniform_row_nnz, 0);
    const bool reg_tail = reg_tail_lds(W, R, 1, want_dev) > 0;
    if (k.force_reg && !halo && (reg_csr || reg_tail)) return 1;
    if (csr > 0) {
        for (int c = kMaxChunks; c >= 1; c >>= 1) {
            // (the column-tiled halo kernel runs at most 4 row passes per thread)
            if ((int64_t)R * c > (int64_t)(halo ? 4 : kRowsPerThread) * kTileThreads) continue;
            const LdsLayout L = lds_layout(R, c, csr, want_dev);
            if (L.tile > 65536 && c > 1) continue;
            if (L.total <= kLdsBytes) return c;
        }
    }
    if (halo) return 0;
    // the CSR does not fit beside any tile: the register-CSR kernels need LDS for the tile (and
    // path 5 for the CSR entries past each row's register head)
    const LdsLayout L = lds_layout(R, 1, 0, want_dev);
    return (reg_csr && L.tile <= 65536 && L.total <= kLdsBytes) || reg_tail ? 1 : 0;
}

// An irregular graph of more than 2048 agents takes the register-head + LDS-tail kernel (path 5)
// even when its whole CSR fits LDS beside the tile: above 2048 agents the tile is one 4-column
// chunk either way, and path 1's per-lane CSR loop from LDS (row pointers, weights and rows read
// per entry, a wave as long as its longest row) runs Barabasi-Albert m = 1 at 250 rounds/s
// against 430 for path 5 (4096 x 2^18, `bench.py --workload c4-ba --irregular ba1`).
bool prefer_reg_tail(const dl_csr &W, int32_t R, int c) {
    return c == 1 && R > 2048 && W.uniform_row_nnz == 0 && reg_head_rows(W.min_row_nnz) > 0;
}

// Register-CSR plan for c chunks -- path 4 (regular, 5 entries per row, all in registers) or
// path 5 (rows of >= min_row_nnz entries: register head + LDS tail) -- or false when neither
// applies.
bool plan_reg(const dl_mix_args &a, int c, bool want_dev, int n_cus, const Knobs &k, Plan *pl) {
    const int32_t R = a.W.n_rows;
    if (a.n_halo > 0 || local_src(a) != R) return false;
    const LdsLayout T = lds_layout(R, c, 0, want_dev);
    int head = 0;
    int64_t lds = T.total;
    if (reg_csr_supported(c, R, a.W.uniform_row_nnz, 0)) {
        if (lds > kLdsBytes) return false;
    } else {
        lds = reg_tail_lds(a.W, R, c, want_dev, &head, &pl->tail_fmt);
        if (lds == 0) return false;
    }
    const int64_t n_tiles = (a.n_params + 4 * c - 1) / (4 * c);
    if (n_tiles > 0x7fffffff) return false;
    const int64_t slots = (int64_t)n_cus * wg_per_cu(lds, k);
    const int mult = a.tile_cols > 0 ? grid_mult_for(n_tiles, slots, k) : 1;
    // the tile, the scratch, then path 5's LDS tail (csr_off)
    fill(pl, head > 0 ? 5 : 4, 4 * c, balanced_grid(n_tiles, slots * mult, k), n_tiles,
         head > 0 ? 0 : 1, c, LdsLayout{T.tile, T.total, T.tile, lds});
    pl->pub.head = head > 0 ? head : 5;
    pl->pub.tail_fmt = head > 0 ? pl->tail_fmt : 0;
    pl->head = head;
    return true;
}

// mix_trace_irr_kernel's configuration: one [N] float4 image, each row's first `head` entries in
// registers and the rest as 8-byte {weight, row} pairs behind it, a 16 x float4 mean scratch.
// The tail's u16 row map (setup only) lives in the image area.
int plan_trace_irr(const dl_mix_args &a, int n_cus, const Knobs &k, TracePlan *tp, char *err) {
    const dl_csr &W = a.W;
    const int32_t N = W.n_rows;
    if (N < 2 || N > 4 * kTileThreads || W.nnz > 65535 + 5 * (int64_t)N)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: no traced kernel for %d agents "
                                             "with %d CSR entries", N, W.nnz);
    int head = reg_head_rows(W.min_row_nnz);
    int64_t ntail = (int64_t)W.nnz - (int64_t)head * N;
    if (ntail > 65535 || ntail < 0) {
        head = 0;
        ntail = W.nnz;
    }
    if (ntail > 65535)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: %lld CSR entries past the "
                                             "register heads (> 65535)", (long long)ntail);
    // 4-column steps with 8-byte {weight, row} tail pairs (the tail's row map in the image), or
    // 2-column steps with 6-byte tail entries when that does not fit
    bool narrow = false;
    uint32_t img = (uint32_t)N * 16u;
    uint32_t tail = align256((size_t)ntail * 8);
    if (2 * ntail > (int64_t)img || img + tail + 256u > (uint32_t)kLdsBytes) {
        narrow = true;
        img = align256((size_t)N * 8u);
        tail = align256((size_t)ntail * 6);
        if (img + tail + 256u > (uint32_t)kLdsBytes)
            return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: the CSR of %d agents (%d "
                                                 "entries) does not fit LDS beside one image",
                        N, W.nnz);
    }
    tp->irr = 1;
    tp->head = head;
    tp->gm = W.doubly_stochastic ? 0 : 1;
    tp->narrow = narrow ? 1 : 0;
    tp->chunks = 1;
    tp->csr_off = img;
    tp->scratch_off = img + tail;
    tp->lds = img + tail + 256u;
    tp->max_rounds = irr_trace_rounds(irr_trace_kv(N));
    tp->n_steps = a.n_params / (narrow ? 2 : 4);
    tp->grid = (int32_t)balanced_grid(tp->n_steps, n_cus, k);
    return DL_OK;
}

}  // namespace

int choose_tile_cols(const dl_csr &W, int32_t n_halo, int64_t n_params, bool want_dev,
                     const Knobs &k) {
    const int64_t R = (int64_t)W.n_rows + n_halo;
    // a tile of every source row in LDS; 0: not tileable, report the row-major plan
    int tile_cols = R > 65535 ? 0 : 4 * choose_tiled_chunks(W, (int32_t)R, csr_shape(W).lds,
                                                            want_dev, n_halo > 0, k);
    // a tiled halo round needs whole tiles (check_mix_args)
    if (n_halo > 0 && tile_cols > 0) {
        while (tile_cols > 4 && n_params % tile_cols) tile_cols >>= 1;
        if (n_params % tile_cols) tile_cols = 0;
    }
    return tile_cols;
}

// Pick the kernel configuration for a mix round.
int plan_mix(const dl_mix_args &a, int n_cus, const Knobs &k, Plan *pl, char *err) {
    std::memset(pl, 0, sizeof *pl);
    const int32_t R = local_src(a) + a.n_halo;
    const bool halo = a.n_halo > 0;
    const bool lag = a.mean_prev || a.colsum_out;
    // the halo round's column sums use the same LDS scratch as the fused deviation
    const bool want_dev = a.dev_sq || a.dev_max || a.mean || a.colsum_out;
    pl->dev = want_dev;
    const CsrShape S = csr_shape(a.W);
    const uint32_t csr = S.lds;
    int cmax = next_pow2_chunks(a.n_params);
    while (k.max_tile_chunks >= 1 && cmax > k.max_tile_chunks) cmax >>= 1;
    if (a.tile_cols > 0) {  // column-tiled layout: the tile width is fixed by the data
        const int c = a.tile_cols / 4;
        const LdsLayout L = lds_layout(R, c, csr, want_dev);
        if ((csr == 0 || L.total > kLdsBytes || k.force_reg || prefer_reg_tail(a.W, R, c)) &&
            R <= 65535 && plan_reg(a, c, want_dev, n_cus, k, pl))
            return DL_OK;
        // (the column-tiled halo kernel runs at most 4 row passes per thread)
        const int64_t row_cap = (int64_t)(halo ? 4 : kRowsPerThread) * kTileThreads;
        if (csr == 0 || R > 65535 || (int64_t)R * c > row_cap || L.total > kLdsBytes)
            return fail(err, DL_ERR_INVALID, "dl_mix_round: tile_cols %d does not fit this graph "
                                             "(%d rows); query dl_mix_plan_query on row-major args",
                        a.tile_cols, R);
        int64_t n_tiles = (a.n_params + a.tile_cols - 1) / a.tile_cols;
        // tile groups: a halo round of few source rows (the split scheme's boundary launch,
        // 276 rows at 16 columns: 18 KB a tile, latency-bound) walks g <= 8 consecutive data tiles
        // as one kernel tile of 4cg columns, within the halo kernel's row passes;
        // DLAMD_TILE_GROUP=g caps g (1: off, a measurement knob)
        int g = 1;
        LdsLayout Lg = L;
        for (int gg = 8; halo && gg >= 2; gg >>= 1) {
            const LdsLayout Lc = lds_layout(R, c * gg, csr, want_dev);
            if (gg > k.tile_group || c * gg > kMaxChunks || n_tiles % gg ||
                (int64_t)R * c * gg > row_cap || Lc.total > kLdsBytes)
                continue;
            g = gg;
            Lg = Lc;
            break;
        }
        const int cg = c * g;
        n_tiles /= g;
        // two 1024-thread workgroups per CU when LDS allows, except at C = 4, where the second
        // workgroup's LDS traffic (4 rows of 64 B per 16 lanes: the most bank conflicts of any
        // C) costs more than its extra loads in flight (measured 5.5 vs 5.8 TB/s at N = 1024;
        // the c4 rank of 8's 608-row halo round: 69.1 vs 70.1 % of spec, profiles/r11/session_c)
        // and except for the halo kernels compiled past 64 VGPRs (halo_two_per_cu)
        int bpc = wg_per_cu(Lg.total, k);
        if (cg == 4 || (halo && !halo_two_per_cu(cg, tile_kv(cg, R, true, true), lag))) bpc = 1;
        const int64_t slots = (int64_t)n_cus * bpc;
        fill(pl, 1, a.tile_cols,
             balanced_grid(n_tiles, slots * grid_mult_for(n_tiles, slots, k), k), n_tiles,
             S.regular, cg, Lg);
        pl->grp = g;
        return DL_OK;
    }
    if ((k.force_reg || (prefer_reg_tail(a.W, R, 1) && !k.force_gather)) && R <= 65535 &&
        a.n_params % 4 == 0 && plan_reg(a, 1, want_dev, n_cus, k, pl))
        return DL_OK;
    // with the fused deviation, prefer the widest tile at <= 4 row passes per thread: the
    // kernel then keeps each lane's deviation partials in registers and reduces them once per
    // launch (mix_tile.hip LD); c3's 256 agents: 64-column tiles, 116 -> 105 us a round
    // (scripts/c3_round_probe.py, profiles/r12/c3_round)
    int cdev = 0;
    for (int c = cmax; want_dev && c >= 2 && !cdev; c >>= 1)
        if ((int64_t)R * c <= 4 * (int64_t)kTileThreads) cdev = c;
    // ... and one workgroup per CU there: c3 3704-3729 against 3589-3610 steps/s with two
    // (same box, profiles/r12/c3_round/c3_rows_wg*.log)
    bool one_per_cu = false;
    if (cdev > 0 && cdev < cmax && a.n_params % (4 * cdev) == 0) {
        cmax = cdev;
        one_per_cu = true;
    }
    for (int c = cmax; csr > 0 && R <= 65535 && !k.force_gather && c >= 1; c >>= 1) {
        const LdsLayout L = lds_layout(R, c, csr, want_dev);
        const int64_t n_tiles = (a.n_params + 4 * c - 1) / (4 * c);
        if ((int64_t)R * c > (int64_t)kRowsPerThread * kTileThreads || L.total > kLdsBytes ||
            n_tiles > 0x7fffffff)
            continue;
        const int bpc = one_per_cu && c == cmax ? 1 : wg_per_cu(L.total, k);
        fill(pl, 1, 4 * c, balanced_grid(n_tiles, (int64_t)n_cus * bpc, k), n_tiles, S.regular,
             c, L);
        return DL_OK;
    }
    if (R <= 65535 && !k.force_gather && a.n_params % 4 == 0 &&
        plan_reg(a, 1, want_dev, n_cus, k, pl))
        return DL_OK;
    if (a.W.n_rows > 4 * 65535)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_round: %d rows exceed the gather path limit",
                    a.W.n_rows);
    if (lag)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_round: the lagged halo deviation needs the "
                                             "LDS tile kernel; this graph takes the gather path");
    if (local_src(a) != a.W.n_rows)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_round: n_local_src != n_rows needs the LDS "
                                             "tile kernel; this graph takes the gather path");
    pl->pub.path = 2;
    pl->pub.grid = (int32_t)(((a.n_params + 255) / 256) * ((a.W.n_rows + 3) / 4));
    pl->pub.regular = S.regular;
    return DL_OK;
}

// Configuration of the multi-round kernel: two tile images of all agents in LDS beside the CSR.
int plan_rounds(const dl_mix_args &a, int n_cus, const Knobs &k, Plan *pl, char *err) {
    std::memset(pl, 0, sizeof *pl);
    const int32_t R = a.W.n_rows;
    const bool want_dev = a.dev_sq || a.dev_max || a.mean;
    pl->dev = want_dev;
    if (a.n_halo > 0 || local_src(a) != R)
        return fail(err, DL_ERR_UNSUPPORTED,
                    "dl_mix_rounds: halo rows need one exchange per round");
    if (want_dev && !a.W.doubly_stochastic)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds: the fused final deviation needs a "
                                             "doubly stochastic W");
    const CsrShape S = csr_shape(a.W);
    if (S.lds == 0 || R > 65535)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds: CSR too large");
    // degree-4 regular graphs with shared weights keep the CSR in registers (mix_multi.hip
    // launch_kv: uniform_row_nnz 5, 5 weights, <= 4 rows per thread): no LDS for it
    auto layout = [&](int c) {
        const bool in_regs = S.in_regs && tile_passes(c, R, true) <= 4;
        return lds_layout(R, c, in_regs ? 0u : S.lds, want_dev, 2);
    };
    auto fits = [&](int c) {
        return (int64_t)R * c <= (int64_t)kRowsPerThread * kTileThreads &&
               layout(c).total <= kLdsBytes;
    };
    int c = 0;
    if (a.tile_cols > 0) {
        c = a.tile_cols / 4;
        if (!fits(c))
            return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds: two %d-column tiles of %d rows do "
                                                 "not fit LDS", a.tile_cols, R);
    } else {
        for (int cc = next_pow2_chunks(a.n_params); cc >= 1 && !c; cc >>= 1)
            if (fits(cc) && a.n_params % (4 * cc) == 0) c = cc;
        if (c == 0)
            return fail(err, DL_ERR_UNSUPPORTED,
                        "dl_mix_rounds: no full-tile row-major configuration");
    }
    const int64_t n_tiles = (a.n_params + 4 * c - 1) / (4 * c);
    fill(pl, 3, 4 * c, balanced_grid(n_tiles, n_cus, k), n_tiles, S.regular, c, layout(c));
    return DL_OK;
}

int plan_trace(const dl_mix_args &a, int n_cus, const Knobs &k, TracePlan *tp, char *err) {
    const int32_t N = a.W.n_rows;
    std::memset(tp, 0, sizeof *tp);
    if (a.n_halo > 0 || local_src(a) != N)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: halo rows need one exchange per "
                                             "round");
    if (a.g)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: no local step (g must be NULL)");
    if (a.n_params % 4)
        return fail(err, DL_ERR_UNSUPPORTED,
                    "dl_mix_rounds_trace: n_params must be a multiple of 4");
    // a W that is not doubly stochastic (every round's mean from its outputs), or an irregular
    // graph above 2048 agents: the one-image kernel with the register head + LDS tail CSR
    const CsrShape S = csr_shape(a.W);
    if (!a.W.doubly_stochastic || (N > 2 * kTileThreads && !S.in_regs))
        return plan_trace_irr(a, n_cus, k, tp, err);
    // one agent per thread up to 1024 agents; above, mix_trace_wide_kernel (one column chunk per
    // step, up to 4 agents per thread; the CSR in registers above 2048 agents)
    if (N < 2 || N > 4 * kTileThreads)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: needs 2..%d agents, got %d",
                    4 * kTileThreads, N);
    const uint32_t csr = S.in_regs ? 0u : S.lds;
    if (!S.in_regs && csr == 0) return plan_trace_irr(a, n_cus, k, tp, err);
    const bool wide = N > kTileThreads;
    const int64_t nq = a.n_params / 4;
    const int64_t lc = a.tile_cols > 0 ? a.tile_cols / 4 : 0;   // 0: row-major
    // widest chunk count whose two images fit LDS (a round then does C outputs per thread)
    for (int c = wide ? 1 : 4; c >= 1 && !tp->chunks; c >>= 1) {
        const uint32_t img = 2u * (uint32_t)N * 16u * (uint32_t)c;
        const uint32_t scr = align256(img + csr);
        const uint32_t lds = scr + (kTileThreads / 64) * 16u * (uint32_t)c;
        // a step's chunks must be whole (nq % c) and lie in one operand tile (lc % c)
        if (lds <= (uint32_t)kLdsBytes && nq % c == 0 && (lc == 0 || lc % c == 0)) {
            tp->chunks = c;
            tp->csr_off = img;
            tp->scratch_off = scr;
            tp->lds = lds;
        }
    }
    if (tp->chunks == 0) return plan_trace_irr(a, n_cus, k, tp, err);   // one image instead
    tp->max_rounds = trace_max_rounds(N, S.in_regs, tp->chunks, k.trace_planes);
    tp->n_steps = nq / tp->chunks;
    tp->grid = (int32_t)balanced_grid(tp->n_steps, n_cus, k);
    return DL_OK;
}

}  // namespace dl
