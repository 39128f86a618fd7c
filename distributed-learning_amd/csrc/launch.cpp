// Launch shaping (launch.h): argument validation, the kernels' TileArgs, and what every round
// entry point launches.
#include "launch.h"

#include <cstring>

namespace dl {

void tile_stride(bool tiled, int64_t ld, int64_t rows, int64_t T, int64_t *ts, uint32_t *rs) {
    *ts = tiled ? (ld ? ld : rows) * T * 4 : T * 4;
    *rs = (uint32_t)(tiled ? T * 4 : ld * 4);
}

namespace {

// MI355X Infinity Cache (MALL), shared by all XCDs
constexpr size_t kMallBytes = (size_t)256 << 20;

void set_tile_strides(TileArgs &t, int64_t T) {
    tile_stride(t.tiled, t.ldx, t.n_loc, T, &t.xts, &t.xrs);
    tile_stride(t.tiled, t.ldg, t.n_loc, T, &t.gts, &t.grs);
    tile_stride(t.tiled, t.ldy, t.n_rows, T, &t.yts, &t.yrs);
    if (!t.tiled) t.hrs = (uint32_t)(t.ldh * 4);
}

// Full tiles on the branch-free float4 kernel, the ragged tail tile (and unaligned operands) on
// the guarded one, each on at most gmax workgroups.
struct Split {
    int64_t n_full, n_tail;  // n_tail: 0 or 1 when vec, else all tiles
    int grid_full, grid_tail;
    int parts() const { return grid_full + grid_tail; }
};
Split split_tiles(const TileArgs &t, int64_t T, int64_t n_tiles, int64_t gmax) {
    Split s;
    s.n_full = t.tiled ? n_tiles : (t.vec ? t.n_params / T : 0);
    s.n_tail = n_tiles - s.n_full;
    s.grid_full = (int)(s.n_full < gmax ? s.n_full : gmax);
    s.grid_tail = (int)(s.n_tail < gmax ? s.n_tail : gmax);
    return s;
}
// The tile launches of a split from the prototype in out->l[0]; each writes its own deviation
// partial rows ([grid][part_rows] floats at `partial`, the tail's behind the full tiles').
// runs: the full launch's workgroups walk contiguous runs of tiles.
void push_split(Launches *out, const Split &s, int64_t T, float *partial, int32_t part_rows,
                bool runs) {
    Launch &full = out->l[0];
    if (s.grid_tail > 0) {
        Launch &tail = out->l[s.grid_full > 0 ? 1 : 0];
        if (s.grid_full > 0) tail = full;
        tail.kind = kLaunchTile;
        tail.fast = false;
        tail.grid = s.grid_tail;
        tail.t.n_tiles = (int32_t)s.n_tail;
        tail.t.col_base = s.n_full * T;
        tail.t.dev_partial = partial ? partial + (size_t)s.grid_full * part_rows : nullptr;
    }
    if (s.grid_full > 0) {
        full.fast = true;
        full.grid = s.grid_full;
        full.t.n_tiles = (int32_t)s.n_full;
        if (runs) full.t.tile_run = (int32_t)((s.n_full + s.grid_full - 1) / s.grid_full);
        full.t.dev_partial = partial;
    }
    out->n = (s.grid_full > 0) + (s.grid_tail > 0);
}

// an empty list whose first launch is zeroed (the second is a copy of it when there is one)
void reset(Launches *out) {
    out->n = 0;
    out->after = kAfterNothing;
    out->partial = nullptr;
    out->parts = out->rows = 0;
    out->max_zeroed = false;
    std::memset(&out->l[0], 0, sizeof out->l[0]);
}

// No output (o) may share a byte with an input or another output; a span of 0 bytes is absent.
struct Span { const void *p; size_t n; };
int check_disjoint(const char *who, const Span *o, const char *const *o_name, int n_out,
                   const Span *in, const char *const *in_name, int n_in, char *err) {
    for (int i = 0; i < n_out; ++i) {
        if (!o[i].n) continue;
        for (int j = 0; j < n_in; ++j)
            if (in[j].n && overlaps(o[i].p, o[i].n, in[j].p, in[j].n))
                return fail(err, DL_ERR_INVALID, "%s: %s overlaps %s", who, o_name[i], in_name[j]);
        for (int j = i + 1; j < n_out; ++j)
            if (o[j].n && overlaps(o[i].p, o[i].n, o[j].p, o[j].n))
                return fail(err, DL_ERR_INVALID, "%s: %s overlaps %s", who, o_name[i], o_name[j]);
    }
    return DL_OK;
}

void after_reduce(Launches *out, const float *partial, int parts, int rows, bool max_zeroed) {
    out->after = kAfterReduce;
    out->partial = partial;
    out->parts = parts;
    out->rows = rows;
    out->max_zeroed = max_zeroed;
}

// The operand layout of a round whose tile_cols passed check_mix_args: row-major rows of
// n_params floats, or column tiles of Tc columns.  The rules an operand of n rows "laid out as x"
// obeys are the fused rounds' (their extra operands all have the round's n_rows rows).
struct Layout {
    bool tiled;
    int64_t n, n_params, Tc, ntl;
    explicit Layout(const dl_mix_args &a)
        : tiled(a.tile_cols > 0), n(a.W.n_rows), n_params(a.n_params), Tc(a.tile_cols),
          ntl(tiled ? (a.n_params + Tc - 1) / Tc : 0) {}
    // bytes spanned: a tiled operand of `rows` used rows inside blocks of `ld` rows (0 = its own
    // rows) spans (tiles - 1) block strides plus its used rows of the last tile
    size_t span(int64_t ld, int64_t rows) const {
        return tiled ? (size_t)(((ntl - 1) * (ld ? ld : rows) + rows) * Tc * 4)
                     : ((size_t)(rows - 1) * ld + n_params) * 4;
    }
    size_t span(int64_t ld) const { return span(ld, n); }
    // not laid out as x: row-major ld < n_params; column-tiled block rows neither 0 (its own
    // rows) nor at least n, or beyond the kernels' block-row bound
    bool bad_ld(int64_t ld) const {
        return tiled ? ld < 0 || (ld > 0 && ld < n) || ld > 65535 * 4 : ld < n_params;
    }
    // do the float4 kernels reach the operand: 16-byte aligned, and row-major rows too, within
    // the 32-bit offsets of a tile base (as tile_args asks of x, g and y)
    bool reach(const void *p, int64_t ld) const {
        return aligned16(p) &&
               (tiled || (ld % 4 == 0 && ((n - 1) * ld + 128) * 4 < ((int64_t)1 << 32)));
    }
};

}  // namespace

int check_mix_args(const dl_mix_args *a, char *err, bool y_may_be_x) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_mix_round: args is NULL");
    const dl_csr &W = a->W;
    if (W.n_rows <= 0)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: n_rows must be > 0 (got %d)", W.n_rows);
    if (a->n_params <= 0) return fail(err, DL_ERR_INVALID, "dl_mix_round: n_params must be > 0");
    if (a->n_halo < 0) return fail(err, DL_ERR_INVALID, "dl_mix_round: n_halo < 0");
    if (a->n_local_src < 0) return fail(err, DL_ERR_INVALID, "dl_mix_round: n_local_src < 0");
    const int32_t NL = local_src(*a);
    // an interior / boundary row set of an agent partition (outputs need not be source rows)
    const bool part = mix_partitioned(*a);
    if ((int64_t)W.n_rows > (int64_t)NL + a->n_halo)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: n_rows %d > n_local_src + n_halo %lld",
                    W.n_rows, (long long)NL + a->n_halo);
    if (W.nnz < 0) return fail(err, DL_ERR_INVALID, "dl_mix_round: nnz < 0");
    if (a->n_hub_rows < 0) return fail(err, DL_ERR_INVALID, "dl_mix_round: n_hub_rows < 0");
    if (!a->x || !a->y || !W.row_ptr || (W.nnz > 0 && (!W.col || !W.w)))
        return fail(err, DL_ERR_INVALID, "dl_mix_round: null x/y/row_ptr/col/w");
    if (a->tile_cols < 0 || (a->tile_cols > 0 && (a->tile_cols % 4 || a->tile_cols < 4 ||
                                                   a->tile_cols > 4 * kMaxChunks ||
                                                   (a->tile_cols & (a->tile_cols - 1)))))
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: tile_cols must be 0 or a power of two in [4, %d]",
                    4 * kMaxChunks);
    const bool tiled = a->tile_cols > 0;
    if (!tiled && (a->ldx < a->n_params || a->ldy < a->n_params))
        return fail(err, DL_ERR_INVALID, "dl_mix_round: ldx/ldy smaller than n_params");
    if (!tiled && a->g && a->ldg < a->n_params)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: ldg < n_params");
    // column-tiled: ld* = rows of each operand's tiled blocks (0 = the operand's own rows)
    if (tiled && (a->ldx < 0 || a->ldy < 0 || a->ldg < 0 || (a->ldx > 0 && a->ldx < NL) ||
                  (a->ldy > 0 && a->ldy < W.n_rows) || (a->g && a->ldg > 0 && a->ldg < NL) ||
                  a->ldx > 65535 * 4 || a->ldy > 65535 * 4 || a->ldg > 65535 * 4))
        return fail(err, DL_ERR_INVALID, "dl_mix_round: tiled ldx/ldg (>= n_local_src) or "
                                         "ldy (>= n_rows) out of range");
    if (a->n_halo > 0 && !a->halo)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: n_halo > 0 needs a halo buffer");
    if (!tiled && a->n_halo > 0 && a->ldh < a->n_params)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: n_halo > 0 needs halo with ldh >= n_params");
    if (!tiled && a->n_halo_blocks != 0)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: n_halo_blocks is for the column-tiled layout");
    if (tiled && a->n_halo > 0) {
        if (a->n_halo_blocks < 0 || a->n_halo_blocks > kMaxHaloBlocks ||
            (a->n_halo_blocks > 0 && !a->halo_block_rows))
            return fail(err, DL_ERR_INVALID, "dl_mix_round: n_halo_blocks must be 0..%d with "
                                             "halo_block_rows", kMaxHaloBlocks);
        int64_t sum = 0;
        for (int b = 0; b < a->n_halo_blocks; ++b) {
            if (a->halo_block_rows[b] <= 0)
                return fail(err, DL_ERR_INVALID, "dl_mix_round: halo_block_rows[%d] <= 0", b);
            sum += a->halo_block_rows[b];
        }
        if (a->n_halo_blocks > 0 && sum != a->n_halo)
            return fail(err, DL_ERR_INVALID,
                        "dl_mix_round: halo_block_rows sum to %lld, n_halo %d", (long long)sum,
                        a->n_halo);
        const int64_t ntl = (a->n_params + a->tile_cols - 1) / a->tile_cols;
        if (ntl * a->n_halo * a->tile_cols * 4 >= ((int64_t)1 << 32))
            return fail(err, DL_ERR_INVALID, "dl_mix_round: the tiled halo must span < 4 GiB");
    }
    // a column-tiled partition round reads mean_prev / colsum_out a float4 per chunk, tiles whole
    if (tiled && part && a->n_params % a->tile_cols)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: a column-tiled partition round needs "
                                         "n_params %% tile_cols == 0");
    if (W.uniform_row_nnz < 0 ||
        (W.uniform_row_nnz > 0 && (int64_t)W.uniform_row_nnz * W.n_rows != W.nnz))
        return fail(err, DL_ERR_INVALID, "dl_mix_round: uniform_row_nnz * n_rows != nnz");
    if (W.shared_row_weights && W.uniform_row_nnz <= 0)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: shared_row_weights needs uniform_row_nnz > 0");
    if (W.min_row_nnz < 0 || (int64_t)W.min_row_nnz * W.n_rows > W.nnz)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: min_row_nnz * n_rows > nnz");
    if ((a->mean_prev || a->colsum_out) && !part)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: mean_prev / colsum_out are for halo rounds "
                    "(n_halo > 0 or n_local_src != n_rows); local rounds fuse "
                    "the exact deviation");
    if (a->mean && part)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: the column mean of a halo round is global: "
                    "use colsum_out and an all-reduce");
    if ((a->dev_sq || a->dev_max || a->mean_prev || a->colsum_out) && part &&
        !(a->mean_prev && a->colsum_out))
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: a halo round's deviation is the lagged one: mean_prev, "
                    "colsum_out and dev_sq together, or both without dev_sq (partial rows left "
                    "in the workspace), or dl_column_sum + dl_deviation after it");
    if (part && a->mean_prev && !a->dev_sq && a->tile_cols <= 0)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: partial rows without dev_sq need the "
                    "column-tiled layout (one launch, plan grid rows)");
    if (part && a->mean_prev && !a->dev_sq && !a->partial_rows_out)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_round: a lagged halo round without dev_sq leaves its "
                    "deviation as partial rows: pass partial_rows_out (ABI 9) to "
                    "receive their count, or dev_sq for the reduced deviation");
    const Layout lay(*a);
    const size_t yb = lay.span(a->ldy, W.n_rows);
    const bool in_place = y_may_be_x && a->y == a->x && a->ldy == a->ldx;
    if (!in_place && overlaps(a->x, lay.span(a->ldx, NL), a->y, yb))
        return fail(err, DL_ERR_INVALID, "dl_mix_round: y overlaps x");
    if (a->g && overlaps(a->g, lay.span(a->ldg, NL), a->y, yb))
        return fail(err, DL_ERR_INVALID, "dl_mix_round: y overlaps g");
    if (a->n_halo > 0) {
        const size_t hb = tiled ? (size_t)(lay.ntl * a->n_halo * lay.Tc * 4)
                                : lay.span(a->ldh, a->n_halo);
        if (overlaps(a->halo, hb, a->y, yb))
            return fail(err, DL_ERR_INVALID, "dl_mix_round: y overlaps halo");
    }
    return DL_OK;
}

TileArgs tile_args(const dl_mix_args &a, const Knobs &k) {
    TileArgs t{};
    t.x = a.x;
    t.ldx = a.ldx;
    t.halo = a.halo;
    t.ldh = a.ldh;
    t.g = a.g;
    t.ldg = a.ldg;
    t.y = a.y;
    t.ldy = a.ldy;
    t.rowptr = a.W.row_ptr;
    t.col = a.W.col;
    t.w = a.W.w;
    t.n_rows = a.W.n_rows;
    t.n_loc = local_src(a);
    t.n_src = t.n_loc + a.n_halo;
    t.nnz = a.W.nnz;
    t.regular = a.W.uniform_row_nnz;
    t.n_w = (a.W.uniform_row_nnz > 0 && a.W.shared_row_weights) ? a.W.uniform_row_nnz : a.W.nnz;
    t.mean_from_inputs = (a.W.doubly_stochastic && t.n_src == t.n_rows) ? 1 : 0;
    // X, G and X' are streamed exactly once per round: non-temporal loads and stores keep them
    // out of L2/MALL (measured +1.5 % on c2).  An X' that fits the 256-MB MALL is stored plainly
    // instead, so the next kernel's reads of it (the c3 gradient launch reading X' as its
    // parameters) can hit there: c3 +2 % steps/s (3743 vs 3668) -- but not in a partitioned
    // round, whose next launch is the next column chunk's pack and mix (other columns): plain
    // stores there left the following launch 16 % slower (one rank of 8, two chunks of 256 MB:
    // 421.7 against 383.5-387.5 us a round with them non-temporal, profiles/r13/c4rank_env/).
    // Knobs::nt_store / nt_load force them.
    const size_t y_bytes = (size_t)a.W.n_rows * (size_t)a.n_params * 4;
    t.nt_store = k.nt_store >= 0 ? k.nt_store
                                 : (y_bytes > kMallBytes || mix_partitioned(a) ? 1 : 0);
    t.nt_load = k.nt_load;
    t.n_params = a.n_params;
    t.lr = a.lr;
    // float4 access: every operand given 16-byte aligned, and row-major rows too (ld % 4)
    bool vec = aligned16(a.x) && aligned16(a.y) && aligned16(a.g) && aligned16(a.halo) &&
               aligned16(a.mean) && aligned16(a.mean_prev) && aligned16(a.colsum_out);
    if (a.tile_cols <= 0)
        vec = vec && a.ldx % 4 == 0 && a.ldy % 4 == 0 && (!a.g || a.ldg % 4 == 0) &&
              (!a.halo || a.ldh % 4 == 0);
    t.mean_prev = a.mean_prev;
    t.colsum_out = a.colsum_out;
    // the float4 kernel addresses rows with 32-bit byte offsets from the tile base
    const int64_t lim = (int64_t)1 << 32;
    const int64_t R = t.n_loc > t.n_rows ? t.n_loc : t.n_rows;
    if (a.tile_cols > 0) {
        t.tiled = 1;
        // per-peer halo blocks (check_mix_args: <= kMaxHaloBlocks, rows summing to n_halo, the
        // whole halo < 4 GiB)
        const int64_t Tc = a.tile_cols;
        const int64_t ntl = (a.n_params + Tc - 1) / Tc;
        const int nb = a.n_halo > 0 ? (a.n_halo_blocks > 0 ? a.n_halo_blocks : 1) : 0;
        t.n_hblk = nb;
        int32_t r0 = 0;
        for (int b = 0; b < nb; ++b) {
            t.hblk_row0[b] = r0;
            t.hblk_off[b] = (uint32_t)(ntl * r0 * Tc * 4);
            r0 += a.n_halo_blocks > 0 ? a.halo_block_rows[b] : a.n_halo;
        }
        t.hblk_row0[nb] = r0;
    } else if (((R - 1) * a.ldx + 128) * 4 >= lim || ((R - 1) * a.ldy + 128) * 4 >= lim ||
               (a.g && ((R - 1) * a.ldg + 128) * 4 >= lim) ||
               // a halo row's offset (row and column) is one 32-bit value
               (a.n_halo > 0 && (int64_t)a.n_halo * a.ldh * 4 >= lim)) {
        vec = false;
    }
    t.vec = vec ? 1 : 0;
    t.mean = a.mean;
    return t;
}

int shape_round(const dl_mix_args &a, int n_cus, const Knobs &k, void *ws, size_t ws_bytes,
                Launches *out, char *err, bool vec_ok) {
    reset(out);
    Plan pl;
    int rc = plan_mix(a, n_cus, k, &pl, err);
    if (rc) return rc;
    const int32_t Nr = a.W.n_rows;
    Launch &l = out->l[0];
    l.t = tile_args(a, k);
    TileArgs &t = l.t;
    if (!vec_ok) t.vec = 0;
    l.sgd = a.g != nullptr;
    l.dev = pl.dev;   // a lagged halo round always writes its deviation partials
    l.mix = true;
    // lagged halo rounds: one partial row per local source row
    const bool lag = tile_lag(t);
    const int32_t Np = lag ? t.n_loc : Nr;
    if (pl.dev && !ws_holds(ws, ws_bytes, 0))
        return fail(err, DL_ERR_WORKSPACE, "dl_mix_round: deviation outputs need a 16-byte "
                                           "aligned workspace of dl_mix_workspace_bytes()");
    // the register-CSR kernels (paths 4 / 5) are FAST-only and the gather kernel reads row-major
    // operands only: unaligned column-tiled operands are refused, unaligned row-major ones of
    // paths 4 / 5 take the gather path
    if (t.tiled && !t.vec)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: tiled operands must be 16-byte aligned");
    if (pl.pub.path == 2 || (pl.pub.path != 1 && !t.vec)) {
        l.kind = kLaunchGather;
        l.columns = k.gather_order_columns;
        out->n = 1;
        if (pl.dev) out->after = Nr <= 1 ? kAfterZero : kAfterTwoPass;
        return DL_OK;
    }
    const bool reg_csr = pl.pub.path != 1;
    const int64_t T = pl.pub.tile_cols;
    set_tile_strides(t, T);
    const Split s = split_tiles(t, T, pl.pub.n_tiles, pl.pub.grid);
    const size_t need = partial_bytes(s.parts(), Np);
    if (pl.dev && ws_bytes < need)
        return fail(err, DL_ERR_WORKSPACE, "dl_mix_round: workspace %zu < %zu bytes", ws_bytes,
                    need);
    if (reg_csr && s.grid_tail > 0)
        return fail(err, DL_ERR_INVALID, "dl_mix_round: register-CSR plan with a tail");
    t.csr_off = pl.csr_off;
    t.scratch_off = pl.scratch_off;
    if (pl.grp > 1) {   // tile groups: chunk c of a kernel row -> data tile c / (T / 4)
        t.grp = pl.grp;
        t.cd_sh = __builtin_ctz((unsigned)(T / 4));
    }
    float *partial = pl.dev ? static_cast<float *>(ws) : nullptr;
    if (pl.dev) t.dev_max_zero = reinterpret_cast<unsigned int *>(a.dev_max);
    int lds = pl.pub.lds_bytes;
    // Knobs::lds_min, a measurement knob: LDS per workgroup bounds workgroups per CU
    if (k.lds_min > lds) lds = k.lds_min < kLdsBytes ? k.lds_min : kLdsBytes;
    if (pl.pub.path == 5 && pl.head < 5 && a.n_hub_rows > 0) {
        // hub rows' register heads behind the LDS tail: as many as fit, <= 256
        const int hb = pl.head * 8;
        const int room = (kLdsBytes - lds) / hb;
        int nh = a.n_hub_rows < 256 ? a.n_hub_rows : 256;
        if (nh > Nr) nh = Nr;
        if (nh > room) nh = room;
        if (nh > 0) {
            t.n_hub = nh;
            t.hub_off = (uint32_t)((lds + 15) & ~15);
            lds = (int)t.hub_off + nh * hb;
            if (lds > kLdsBytes) {   // (alignment) fall back to no hub lanes
                t.n_hub = 0;
                lds = pl.pub.lds_bytes;
            }
        }
    }
    l.kind = reg_csr ? kLaunchTileReg : kLaunchTile;
    l.chunks = pl.chunks;
    l.head = pl.head;
    l.tail_fmt = pl.tail_fmt;
    l.lds = lds;
    // row-major operands: each workgroup walks one contiguous run of tiles instead of every
    // grid-th tile, so its row segments follow each other in every row (c3's 256 x 164,608
    // round: 103.8 against 105.3-107.3 us between events, profiles/r13/c3_env/); the
    // column-tiled layout keeps the grid stride (+0.4 % with runs on c2, within noise).
    // Knobs::tile_run forces it off / on.
    push_split(out, s, T, partial, Np, k.tile_run >= 0 ? k.tile_run == 1 : !t.tiled);
    if (!pl.dev) return DL_OK;
    // a lagged round without dev_sq leaves its partial rows to the caller (column chunks reduced
    // once, dl_row_sums) and says how many; its dev_max, if any, the kernel zeroed
    if (Nr <= 1 && !lag) {
        out->after = kAfterZero;
    } else if (lag && !a.dev_sq) {
        out->after = kAfterPartialRows;
        out->parts = s.parts();
    } else {
        after_reduce(out, partial, s.parts(), Np, true);
    }
    return DL_OK;
}

namespace {

// A fused round on the LDS tile kernel, as the steps its entry points share see it: the entry
// point's name and the word for the round in the texts, what its launches are, and the operands
// it adds to the round's, each laid out as x.
struct Operand { const void *p; int64_t ld; };
struct FusedRound {
    const char *name, *word;
    LaunchKind kind;
    const Operand *extra;
    int n_extra;
};

// Whole rounds only, then the round's own checks (y == x allowed).
int whole_round(const FusedRound &r, const dl_mix_args &m, char *err) {
    if (m.halo || m.n_halo != 0 || m.mean_prev || m.colsum_out || m.n_local_src != 0 ||
        m.n_halo_blocks != 0 || m.partial_rows_out)
        return fail(err, DL_ERR_UNSUPPORTED,
                    "%s: no halo rows, partition row sets or lagged deviation (halo, "
                    "n_halo, mean_prev, colsum_out, n_local_src, n_halo_blocks, partial_rows_out "
                    "must be NULL / 0)", r.name);
    return check_mix_args(&m, err, true);
}

// After the operand checks: the plan, refused unless path 1 and copied to *plan when given; then,
// unless this is the plan query (out NULL, which needs `plan`), shape_round with the float4
// kernels ruled out when they cannot reach an extra operand, every launch re-tagged r.kind.  The
// caller fills the launches' extra args.
int plan_and_shape(const FusedRound &r, const dl_mix_args &m, int n_cus, const Knobs &k, void *ws,
                   size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err) {
    if (!out && !plan) return fail(err, DL_ERR_INVALID, "%s_plan: plan is NULL", r.name);
    Plan pl;
    int rc = plan_mix(m, n_cus, k, &pl, err);
    if (rc) return rc;
    if (pl.pub.path != 1)
        return fail(err, DL_ERR_UNSUPPORTED, "%s: the fused %s round runs on the LDS tile kernel "
                                             "(plan path 1); this round plans path %d", r.name,
                    r.word, pl.pub.path);
    if (plan) *plan = pl.pub;
    if (!out) return DL_OK;
    const Layout lay(m);
    bool vec_ok = true;
    for (int i = 0; i < r.n_extra; ++i) vec_ok = vec_ok && lay.reach(r.extra[i].p, r.extra[i].ld);
    rc = shape_round(m, n_cus, k, ws, ws_bytes, out, err, vec_ok);
    if (rc) return rc;
    for (int i = 0; i < out->n; ++i) {
        if (out->l[i].kind != kLaunchTile)
            return fail(err, DL_ERR_UNSUPPORTED, "%s: the fused %s round runs on the LDS tile "
                                                 "kernel (plan path 1) only", r.name, r.word);
        out->l[i].kind = r.kind;
    }
    return DL_OK;
}

// FAST-path strides of an extra operand of launch l
void extra_stride(const Launch &l, int64_t ld, int64_t *ts, uint32_t *rs) {
    tile_stride(l.t.tiled, ld, l.t.n_rows, 4 * l.chunks, ts, rs);
}

}  // namespace

int shape_sgd_round(const dl_sgd_round_args *a, int n_cus, const Knobs &k, void *ws,
                    size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_sgd_round: args is NULL");
    const dl_mix_args &m = a->mix;
    if (!m.x || !m.y || !m.g) return fail(err, DL_ERR_INVALID, "dl_sgd_round: null x/y/g");
    // the momentum buffers are an operand only with a momentum
    const bool mom = a->momentum != 0.f;
    const Operand buf{a->buf, a->ldb};
    const FusedRound r{"dl_sgd_round", "momentum", kLaunchSgdTile, &buf, mom ? 1 : 0};
    int rc = whole_round(r, m, err);
    if (rc) return rc;
    const Layout lay(m);
    if (mom && (!a->buf || lay.bad_ld(a->ldb)))
        return fail(err, DL_ERR_INVALID, "dl_sgd_round: momentum needs a buffer laid out as x "
                                         "(row-major ldb >= n_params; column-tiled ldb 0 or >= "
                                         "n_rows)");
    if (a->nesterov && (a->momentum <= 0.f || a->dampening != 0.f))
        return fail(err, DL_ERR_INVALID, "dl_sgd_round: Nesterov momentum requires a momentum and "
                                         "zero dampening");
    if (mom) {
        const size_t bb = lay.span(a->ldb);
        if (overlaps(a->buf, bb, m.x, lay.span(m.ldx)) ||
            overlaps(a->buf, bb, m.y, lay.span(m.ldy)) ||
            overlaps(a->buf, bb, m.g, lay.span(m.ldg)))
            return fail(err, DL_ERR_INVALID, "dl_sgd_round: buf overlaps x, y or g");
    }
    rc = plan_and_shape(r, m, n_cus, k, ws, ws_bytes, plan, out, err);
    if (rc || !out) return rc;
    for (int i = 0; i < out->n; ++i) {
        Launch &l = out->l[i];
        l.q.p = SgdParams{m.lr, a->momentum, a->dampening, a->weight_decay,
                          a->first ? 1 : 0, a->nesterov ? 1 : 0};
        if (mom) {
            l.q.buf = a->buf;
            l.q.ldb = a->ldb;
            extra_stride(l, a->ldb, &l.q.bts, &l.q.brs);
        }
    }
    return DL_OK;
}

int shape_cheb_round(const dl_cheb_round_args *a, int n_cus, const Knobs &k, void *ws,
                     size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_cheb_round: args is NULL");
    const dl_mix_args &m = a->mix;
    if (!m.x || !m.y || !a->z) return fail(err, DL_ERR_INVALID, "dl_cheb_round: null x/y/z");
    if (m.g)
        return fail(err, DL_ERR_INVALID, "dl_cheb_round: g must be NULL (no local step inside the "
                                         "accelerated round)");
    const Operand z{a->z, a->ldz};
    const FusedRound r{"dl_cheb_round", "Chebyshev", kLaunchChebTile, &z, 1};
    int rc = whole_round(r, m, err);
    if (rc) return rc;
    const Layout lay(m);
    if (lay.bad_ld(a->ldz))
        return fail(err, DL_ERR_INVALID, "dl_cheb_round: z laid out as x (row-major ldz >= "
                                         "n_params; column-tiled ldz 0 or >= n_rows)");
    const bool y_is_z = m.y == a->z && m.ldy == a->ldz;
    if (!y_is_z && overlaps(a->z, lay.span(a->ldz), m.y, lay.span(m.ldy)))
        return fail(err, DL_ERR_INVALID, "dl_cheb_round: y overlaps z (y may be z itself "
                                         "with ldy == ldz)");
    rc = plan_and_shape(r, m, n_cus, k, ws, ws_bytes, plan, out, err);
    if (rc || !out) return rc;
    for (int i = 0; i < out->n; ++i) {
        Launch &l = out->l[i];
        l.c.z = a->z;
        l.c.ldz = a->ldz;
        l.c.a = a->a;
        l.c.b = a->b;
        extra_stride(l, a->ldz, &l.c.zts, &l.c.zrs);
    }
    return DL_OK;
}

int shape_track_round(const dl_track_round_args *a, int n_cus, const Knobs &k, void *ws,
                      size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_track_round: args is NULL");
    const dl_mix_args &m = a->mix;
    if (!m.x || !m.y || !a->d || !a->d_out || !m.g || !a->g_old)
        return fail(err, DL_ERR_INVALID, "dl_track_round: null x/y/d/d_out/g/g_old");
    const Operand extra[] = {{a->d, a->ldd}, {a->d_out, a->lddo}, {a->g_old, a->ldq}};
    const FusedRound r{"dl_track_round", "gradient-tracking", kLaunchTrackTile, extra, 3};
    int rc = whole_round(r, m, err);
    if (rc) return rc;
    const Layout lay(m);
    if (lay.bad_ld(a->ldd) || lay.bad_ld(a->lddo) || lay.bad_ld(a->ldq))
        return fail(err, DL_ERR_INVALID, "dl_track_round: d, d_out and g_old laid out as x "
                                         "(row-major ld >= n_params; column-tiled ld 0 or >= "
                                         "n_rows)");
    const Span d{a->d, lay.span(a->ldd)}, d_out{a->d_out, lay.span(a->lddo)};
    const Span y{m.y, lay.span(m.ldy)}, g_old{a->g_old, lay.span(a->ldq)};
    const bool in_place = a->d_out == a->d && a->lddo == a->ldd;
    if (!in_place && overlaps(d_out.p, d_out.n, d.p, d.n))
        return fail(err, DL_ERR_INVALID, "dl_track_round: d_out overlaps d (d_out may be d "
                                         "itself with lddo == ldd)");
    const Span in[] = {{m.x, lay.span(m.ldx)}, y, {m.g, lay.span(m.ldg)}, g_old};
    const char *const in_name[] = {"x", "y", "g", "g_old"};
    const char *const d_out_name = "d_out";
    rc = check_disjoint(r.name, &d_out, &d_out_name, 1, in, in_name, 4, err);
    if (rc) return rc;
    // (y against x and g: check_mix_args)
    const Span yin[] = {d, g_old};
    const char *const yin_name[] = {"d", "g_old"};
    const char *const y_name = "y";
    rc = check_disjoint(r.name, &y, &y_name, 1, yin, yin_name, 2, err);
    if (rc) return rc;
    rc = plan_and_shape(r, m, n_cus, k, ws, ws_bytes, plan, out, err);
    if (rc || !out) return rc;
    for (int i = 0; i < out->n; ++i) {
        Launch &l = out->l[i];
        TrackTileArgs &q = l.k;
        q.d = a->d;
        q.ldd = a->ldd;
        q.d_out = a->d_out;
        q.lddo = a->lddo;
        q.q = a->g_old;
        q.ldq = a->ldq;
        extra_stride(l, a->ldd, &q.dts, &q.drs);
        extra_stride(l, a->lddo, &q.dots, &q.dors);
        extra_stride(l, a->ldq, &q.qts, &q.qrs);
    }
    return DL_OK;
}

AdamParams adam_params(double beta1, double beta2, float eps, float lr, float wd, int decoupled,
                       float ss, float bs, const float *coef) {
    AdamParams p;
    p.b2 = (float)beta2;
    p.omb1 = (float)(1.0 - beta1);
    p.omb2 = (float)(1.0 - beta2);
    p.eps = eps;
    p.wd = wd;
    p.decay = (float)(1.0 - (double)lr * (double)wd);
    p.ss = ss;
    p.bs = bs;
    p.decoupled = decoupled ? 1 : 0;
    p.coef = coef;
    return p;
}

int check_adam_params(const char *who, double beta1, double beta2, float eps, float ss, float bs,
                      const float *coef, char *err) {
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(err, DL_ERR_INVALID, "%s: beta1 and beta2 must be in [0, 1) (got %g, %g)", who,
                    beta1, beta2);
    if (!(eps >= 0.f)) return fail(err, DL_ERR_INVALID, "%s: eps must be >= 0", who);
    // (x - x is 0 for a finite x and NaN otherwise)
    if (!coef && (ss - ss != 0.f || bs - bs != 0.f))
        return fail(err, DL_ERR_INVALID, "%s: step_size and bias2_sqrt must be finite when coef "
                                         "is NULL", who);
    return DL_OK;
}

int shape_adam_round(const dl_adam_round_args *a, int n_cus, const Knobs &k, void *ws,
                     size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_adam_round: args is NULL");
    const dl_mix_args &m = a->mix;
    if (!m.x || !m.y || !m.g || !a->m || !a->v)
        return fail(err, DL_ERR_INVALID, "dl_adam_round: null x/y/g/m/v");
    const Operand extra[] = {{a->m, a->ldm}, {a->v, a->ldv}};
    const FusedRound r{"dl_adam_round", "Adam", kLaunchAdamTile, extra, 2};
    int rc = whole_round(r, m, err);
    if (rc) return rc;
    const Layout lay(m);
    if (lay.bad_ld(a->ldm) || lay.bad_ld(a->ldv))
        return fail(err, DL_ERR_INVALID, "dl_adam_round: m and v laid out as x (row-major ld >= "
                                         "n_params; column-tiled ld 0 or >= n_rows)");
    rc = check_adam_params(r.name, a->beta1, a->beta2, a->eps, a->step_size, a->bias2_sqrt,
                           a->coef, err);
    if (rc) return rc;
    // m and v are read and written: neither shares a byte with the other or with x, y or g
    const Span mv[] = {{a->m, lay.span(a->ldm)}, {a->v, lay.span(a->ldv)}};
    const char *const mv_name[] = {"m", "v"};
    const Span in[] = {{m.x, lay.span(m.ldx)}, {m.y, lay.span(m.ldy)}, {m.g, lay.span(m.ldg)}};
    const char *const in_name[] = {"x", "y", "g"};
    rc = check_disjoint(r.name, mv, mv_name, 2, in, in_name, 3, err);
    if (rc) return rc;
    rc = plan_and_shape(r, m, n_cus, k, ws, ws_bytes, plan, out, err);
    if (rc || !out) return rc;
    for (int i = 0; i < out->n; ++i) {
        Launch &l = out->l[i];
        AdamTileArgs &q = l.a;
        q.m = a->m;
        q.ldm = a->ldm;
        q.v = a->v;
        q.ldv = a->ldv;
        extra_stride(l, a->ldm, &q.mts, &q.mrs);
        extra_stride(l, a->ldv, &q.vts, &q.vrs);
        q.p = adam_params(a->beta1, a->beta2, a->eps, m.lr, a->weight_decay, a->decoupled,
                          a->step_size, a->bias2_sqrt, a->coef);
    }
    return DL_OK;
}

int shape_rounds(const dl_mix_args &a, int32_t rounds, int n_cus, const Knobs &k, void *ws,
                 size_t ws_bytes, Launches *out, char *err) {
    reset(out);
    if (rounds < 1) return fail(err, DL_ERR_INVALID, "dl_mix_rounds: rounds must be >= 1");
    Plan pl;
    int rc = plan_rounds(a, n_cus, k, &pl, err);
    if (rc) return rc;
    const int32_t Nr = a.W.n_rows;
    Launch &l = out->l[0];
    l.t = tile_args(a, k);
    TileArgs &t = l.t;
    if (!t.vec)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds: operands must be 16-byte aligned "
                                             "float4 rows");
    set_tile_strides(t, pl.pub.tile_cols);
    t.n_tiles = pl.pub.n_tiles;
    t.col_base = 0;
    t.csr_off = pl.csr_off;
    t.scratch_off = pl.scratch_off;
    if (pl.dev) {
        const size_t need = partial_bytes(pl.pub.grid, Nr);
        if (!ws_holds(ws, ws_bytes, need))
            return fail(err, DL_ERR_WORKSPACE, "dl_mix_rounds: deviation outputs need a "
                                               "16-byte aligned workspace of %zu bytes", need);
        t.dev_partial = static_cast<float *>(ws);
        t.dev_max_zero = reinterpret_cast<unsigned int *>(a.dev_max);
    }
    l.kind = kLaunchMulti;
    l.chunks = pl.chunks;
    l.rounds = rounds;
    l.sgd = a.g != nullptr;
    l.dev = pl.dev;
    l.grid = pl.pub.grid;
    l.lds = pl.pub.lds_bytes;
    out->n = 1;
    if (pl.dev) {
        if (Nr <= 1) out->after = kAfterZero;
        else after_reduce(out, t.dev_partial, pl.pub.grid, Nr, true);
    }
    return DL_OK;
}

int shape_trace(const dl_mix_args &a, int32_t rounds, int n_cus, const Knobs &k, void *ws,
                size_t ws_bytes, Launches *out, char *err) {
    reset(out);
    TracePlan tp;
    int rc = plan_trace(a, n_cus, k, &tp, err);
    if (rc) return rc;
    if (rounds < 1 || rounds > tp.max_rounds)
        return fail(err, DL_ERR_INVALID, "dl_mix_rounds_trace: rounds must be in [1, %d] (one "
                                         "traced pass), got %d", tp.max_rounds, rounds);
    Launch &l = out->l[0];
    l.t = tile_args(a, k);
    TileArgs &t = l.t;
    if (!t.vec)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mix_rounds_trace: operands must be 16-byte "
                                             "aligned float4 rows");
    if (tp.irr && t.tiled && a.tile_cols % 4)
        return fail(err, DL_ERR_INVALID,
                    "dl_mix_rounds_trace: tile_cols must be a multiple of 4");
    // a step walks float4 chunks: of an operand tile when column-tiled, else of the row itself
    t.lchunks = t.tiled ? a.tile_cols / 4 : 1;
    set_tile_strides(t, t.tiled ? a.tile_cols : 4);
    t.n_tiles = (int32_t)tp.n_steps;
    t.csr_off = tp.csr_off;
    t.scratch_off = tp.scratch_off;
    const size_t need = partial_bytes((int64_t)tp.grid * rounds, a.W.n_rows);
    if (!ws_holds(ws, ws_bytes, need))
        return fail(err, DL_ERR_WORKSPACE, "dl_mix_rounds_trace: needs a 16-byte aligned "
                                           "workspace of %zu bytes "
                                           "(dl_mix_trace_workspace_bytes)", need);
    t.dev_partial = static_cast<float *>(ws);
    l.kind = tp.irr ? kLaunchTraceIrr : kLaunchTrace;
    l.chunks = tp.chunks;
    l.head = tp.head;
    l.gm = tp.gm != 0;
    l.narrow = tp.narrow != 0;
    l.planes = k.trace_planes;
    l.rounds = rounds;
    l.grid = tp.grid;
    l.lds = (int32_t)tp.lds;
    out->n = 1;
    return DL_OK;
}

int shape_deviation(const float *x, int64_t ldx, int32_t tile_cols, int32_t n_rows,
                    int64_t n_params, float *mean_out, int n_cus, void *ws, size_t ws_bytes,
                    Launches *out, char *err) {
    reset(out);
    int c = tile_cols > 0 ? tile_cols / 4 : next_pow2_chunks(n_params);
    for (; c >= 1; c >>= 1) {
        if ((int64_t)n_rows * c <= (int64_t)kRowsPerThread * kTileThreads) break;
        if (tile_cols > 0) return DL_ERR_UNSUPPORTED;
    }
    if (c < 1) return DL_ERR_UNSUPPORTED;
    const int64_t T = 4 * c;
    bool vec = aligned16(x) && (!mean_out || aligned16(mean_out));
    if (tile_cols == 0)
        vec = vec && ldx % 4 == 0 && ((int64_t)(n_rows - 1) * ldx + 128) * 4 < ((int64_t)1 << 32);
    else if (!vec)
        return fail(err, DL_ERR_INVALID, "dl_deviation_tiled: x must be 16-byte aligned");
    Launch &l = out->l[0];
    TileArgs &t = l.t;
    t.x = x;
    t.ldx = ldx;
    t.n_rows = n_rows;
    t.n_src = n_rows;
    t.n_loc = n_rows;
    t.n_params = n_params;
    t.vec = vec ? 1 : 0;
    t.mean = mean_out;
    t.tiled = tile_cols > 0 ? 1 : 0;
    tile_stride(t.tiled, ldx, n_rows, T, &t.xts, &t.xrs);
    const Split s = split_tiles(t, T, (n_params + T - 1) / T, (int64_t)n_cus * 2);
    if (ws_bytes < partial_bytes(s.parts(), n_rows))
        return fail(err, DL_ERR_WORKSPACE, "dl_deviation: workspace too small");
    l.kind = kLaunchTile;
    l.chunks = c;
    l.dev = true;
    l.lds = (kTileThreads / 64) * c * 16;
    float *partial = static_cast<float *>(ws);
    push_split(out, s, T, partial, n_rows, false);
    after_reduce(out, partial, s.parts(), n_rows, false);
    return DL_OK;
}

int shape_mlp_grad(const dl_mlp_args *a, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_mlp_grad: null args");
    if (a->n_agents == 0) return DL_OK;
    if (!mlp_fused_supported(a->batch, a->input_dim, a->hidden_dim, a->output_dim))
        return fail(err, DL_ERR_UNSUPPORTED,
                    "dl_mlp_grad: fused path needs batch 64, input_dim %% 4 == 0, even hidden_dim "
                    "<= 152, output_dim <= 16 (got %d, %d, %d, %d)", a->batch, a->input_dim,
                    a->hidden_dim, a->output_dim);
    const int64_t din = a->input_dim, dh = a->hidden_dim, dout = a->output_dim;
    const int64_t P = dh * din + dh + 2 * (dh * dh + dh) + dout * dh + dout;
    const int32_t T = a->tile_cols;
    if (T < 0 || (T > 0 && (T < 4 || (T & (T - 1)) || (int64_t)T * a->n_agents > 0x7fffffff)))
        return fail(err, DL_ERR_INVALID, "dl_mlp_grad: tile_cols must be 0 or a power of two >= 4");
    if (a->n_agents < 0 || a->n_agents > 65535 || !a->X || !a->data || !a->labels || !a->G ||
        (T == 0 && (a->ldx < P || a->ldg < P)) || a->s_data < (int64_t)a->batch * din ||
        a->s_labels < a->batch)
        return fail(err, DL_ERR_INVALID, "dl_mlp_grad: bad arguments (agents %d, params %lld, ldx "
                                         "%lld, ldg %lld)", a->n_agents, (long long)P,
                    (long long)a->ldx, (long long)a->ldg);
    if (!aligned16(a->X) || !aligned16(a->data) || !aligned16(a->G) ||
        (T == 0 && ((a->ldx & 3) || (a->ldg & 3))) || (a->s_data & 3))
        return fail(err, DL_ERR_INVALID, "dl_mlp_grad: X, data, G must be 16-byte aligned with row "
                                         "strides %% 4 == 0");
    const size_t tb = T ? (size_t)((P + T - 1) / T) * T * a->n_agents * 4 : 0;
    if (T && tb / 4 > 0x7fffffff)   // the kernel addresses an agent's tiled row with 32-bit offsets
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mlp_grad: tiled X too large for 32-bit offsets");
    const size_t xb = T ? tb : ((size_t)a->n_agents - 1) * a->ldx * 4 + P * 4;
    const size_t gb = T ? tb : ((size_t)a->n_agents - 1) * a->ldg * 4 + P * 4;
    if (overlaps(a->X, xb, a->G, gb)) return fail(err, DL_ERR_INVALID, "dl_mlp_grad: G overlaps X");
    if (a->out_mode != 0 && a->out_mode != 1)
        return fail(err, DL_ERR_INVALID, "dl_mlp_grad: out_mode must be 0 (gradient) or 1 (step)");
    if (a->out_mode == 1 && T == 0 && a->ldg != a->ldx)
        return fail(err, DL_ERR_INVALID, "dl_mlp_grad: out_mode 1 needs ldg == ldx");
    const size_t wb = mlp_workspace_floats(a->n_agents) * sizeof(float);
    if (a->workspace && (!aligned16(a->workspace) || overlaps(a->workspace, wb, a->X, xb) ||
                         overlaps(a->workspace, wb, a->G, gb)))
        return fail(err, DL_ERR_INVALID, "dl_mlp_grad: workspace must be 16-byte aligned and "
                                         "disjoint from X and G");
    return DL_OK;
}

int check_bgemm(const dl_bgemm_args *a, char *err) {
    if (!a || a->batch <= 0 || a->M <= 0 || a->N <= 0 || a->K <= 0 || !a->A || !a->B || !a->C ||
        a->batch > 65535 || a->epi < DL_EPI_NONE || a->epi > DL_EPI_BIAS_XENT)
        return fail(err, DL_ERR_INVALID, "dl_bgemm: bad sizes/pointers/epilogue");
    if ((a->ta ? a->lda < a->M : a->lda < a->K) || (a->tb ? a->ldb < a->K : a->ldb < a->N) ||
        a->ldc < a->N)
        return fail(err, DL_ERR_INVALID, "dl_bgemm: leading dimension too small");
    if (a->epi >= DL_EPI_DRELU && a->epi <= DL_EPI_DELU && (!a->H || a->ldh < a->N))
        return fail(err, DL_ERR_INVALID, "dl_bgemm: derivative epilogue needs H with ldh >= N");
    if (a->epi == DL_EPI_BIAS_XENT && (a->M > 64 || a->N > 64 || !a->labels))
        return fail(err, DL_ERR_INVALID, "dl_bgemm: cross-entropy epilogue needs M <= 64 rows, "
                                         "N <= 64 classes and labels");
    // output batches must not overlap: two workgroups would write the same floats (input
    // strides may be 0, a shared operand)
    if (a->batch > 1 && (a->sC < (int64_t)(a->M - 1) * a->ldc + a->N ||
                         (a->rowsum && a->s_rowsum < a->M)))
        return fail(err, DL_ERR_INVALID, "dl_bgemm: output batch stride smaller than one batch "
                                         "(sC >= (M-1)*ldc + N, s_rowsum >= M)");
    return DL_OK;
}

BgemmArgs bgemm_args(const dl_bgemm_args &a) {   // the same fields in the same order
    return BgemmArgs{a.batch, a.M, a.N, a.K, a.A, a.lda, a.sA, a.ta, a.B, a.ldb, a.sB, a.tb, a.C,
                     a.ldc, a.sC, a.epi, a.bias, a.s_bias, a.H, a.ldh, a.sH, a.rowsum, a.s_rowsum,
                     a.labels, a.s_labels, a.loss};
}

int shape_mlp_eval(const dl_mlp_eval_args *a, int n_cus, const void *ws, size_t ws_bytes,
                   bool check_ws, dl_mlp_eval_plan *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_mlp_eval: args is NULL");
    const int64_t din = a->input_dim, dh = a->hidden_dim, dout = a->output_dim, R = a->rows;
    // dl_mlp_grad's shape gate without the batch clause
    if (!mlp_fused_supported(kMlpBatch, a->input_dim, a->hidden_dim, a->output_dim) || R < 1)
        return fail(err, DL_ERR_UNSUPPORTED,
                    "dl_mlp_eval: needs input_dim %% 4 == 0, even hidden_dim <= 152, output_dim "
                    "<= 16, rows >= 1 (got %d, %d, %d, rows %d)", a->input_dim, a->hidden_dim,
                    a->output_dim, a->rows);
    const int64_t P = dh * din + dh + 2 * (dh * dh + dh) + dout * dh + dout;
    const int32_t T = a->tile_cols;
    const int64_t N = a->n_agents;
    if (T < 0 || (T > 0 && (T < 4 || (T & (T - 1)) || (int64_t)T * N > 0x7fffffff)))
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: tile_cols must be 0 or a power of two >= 4");
    if (!a->X || !a->data) return fail(err, DL_ERR_INVALID, "dl_mlp_eval: null X or data");
    if ((a->loss || a->correct) && !a->labels)
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: loss and correct need labels");
    if (!a->loss && !a->correct && !a->logits)
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: no output (loss, correct, logits all NULL)");
    if (N < 1 || N > 65535 || (T == 0 && a->ldx < P))
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: bad arguments (agents %d, params %lld, ldx "
                                         "%lld)", a->n_agents, (long long)P, (long long)a->ldx);
    if (a->s_data != 0 && (a->s_data < R * din || (a->s_data & 3)))
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: s_data must be 0 (shared) or a multiple of "
                                         "4 >= rows * input_dim (got %lld)", (long long)a->s_data);
    if (a->labels && a->s_labels != 0 && a->s_labels < R)
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: s_labels must be 0 (shared) or >= rows "
                                         "(got %lld)", (long long)a->s_labels);
    if (!aligned16(a->X) || !aligned16(a->data) || (T == 0 && (a->ldx & 3)))
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: X and data must be 16-byte aligned with row "
                                         "strides %% 4 == 0");
    const size_t tb = T ? (size_t)((P + T - 1) / T) * T * N * 4 : 0;
    if (T && tb / 4 > 0x7fffffff)   // the kernel addresses an agent's tiled row with 32-bit offsets
        return fail(err, DL_ERR_UNSUPPORTED, "dl_mlp_eval: tiled X too large for 32-bit offsets");
    if (a->logits && (a->ldz < dout || (N > 1 && a->s_logits < R * a->ldz)))
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: logits need ldz >= output_dim and s_logits "
                                         ">= rows * ldz (got ldz %lld, s_logits %lld)",
                    (long long)a->ldz, (long long)a->s_logits);
    const size_t xb = T ? tb : ((size_t)(N - 1) * a->ldx + P) * 4;
    const size_t db = ((size_t)(N - 1) * a->s_data + (size_t)(R * din)) * 4;
    auto hits_input = [&](const void *p, size_t n) {
        return p && (overlaps(p, n, a->X, xb) || overlaps(p, n, a->data, db));
    };
    const size_t zb = a->logits ? ((size_t)(N - 1) * a->s_logits + (size_t)((R - 1) * a->ldz + dout)) * 4
                                : 0;
    if (hits_input(a->logits, zb) || hits_input(a->loss, (size_t)N * 4) ||
        hits_input(a->correct, (size_t)N * 4))
        return fail(err, DL_ERR_INVALID, "dl_mlp_eval: logits, loss or correct overlaps X or data");
    const int32_t blocks = eval_blocks(a->rows);
    int64_t rs = a->row_splits > 0 ? a->row_splits : (n_cus + N - 1) / N;
    if (rs > blocks) rs = blocks;
    if (rs < 1) rs = 1;
    if (N * rs > 0x7fffffff) return fail(err, DL_ERR_INVALID, "dl_mlp_eval: grid too large");
    if (check_ws) {
        const size_t need = eval_workspace_bytes(a->n_agents, a->rows);
        if (!ws_holds(ws, ws_bytes, need))
            return fail(err, DL_ERR_WORKSPACE, "dl_mlp_eval: needs a 16-byte aligned workspace of "
                                               "%zu bytes (dl_mlp_eval_workspace_bytes)", need);
        if (hits_input(ws, need))
            return fail(err, DL_ERR_INVALID, "dl_mlp_eval: the workspace overlaps X or data");
    }
    if (out) *out = dl_mlp_eval_plan{blocks, (int32_t)rs, (int32_t)(N * rs), kMlpLdsBytes};
    return DL_OK;
}

int shape_batch_gather(const dl_batch_gather_args *a, int n_cus, BatchGatherPlan *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_batch_gather: args is NULL");
    const int64_t N = a->n_agents, B = a->batch, S = a->steps, D = a->dim, M = a->n_samples;
    if (N < 1 || B < 1 || S < 1 || M < 1)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: n_agents, batch, steps and n_samples "
                                         "must be >= 1 (got %d, %d, %d, %d)", a->n_agents,
                    a->batch, a->steps, a->n_samples);
    if (D < 4 || D % 4 || D > (1 << 28))   // a row's bytes are a 32-bit offset in the kernel
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: dim must be a positive multiple of 4, "
                                         "at most 2^28 (got %d)", a->dim);
    if (N * B > 0x7fffffff || S * B > 0x7fffffff)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: n_agents * batch and steps * batch "
                                         "must be < 2^31");
    if (!a->samples || !a->index || !a->data)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: null samples, index or data");
    if (a->ld_samples < D || (a->ld_samples & 3))
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: ld_samples must be a multiple of 4 >= "
                                         "dim (got %lld)", (long long)a->ld_samples);
    if (a->s_data < B * D || (a->s_data & 3))
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: s_data must be a multiple of 4 >= "
                                         "batch * dim (got %lld)", (long long)a->s_data);
    if (a->s_index != 0 && a->s_index < S * B)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: s_index must be 0 (shared) or >= steps "
                                         "* batch (got %lld)", (long long)a->s_index);
    if (!aligned16(a->samples) || !aligned16(a->data))
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: samples and data must be 16-byte "
                                         "aligned");
    if (a->labels && !a->targets)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: labels need targets");
    if (a->labels && a->s_labels < B)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: s_labels must be >= batch (got %lld)",
                    (long long)a->s_labels);
    if (a->advance != 0 && a->advance != 1)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: advance must be 0 or 1");
    if (a->advance && !a->cursor)
        return fail(err, DL_ERR_INVALID, "dl_batch_gather: advance needs a cursor");
    const Span in[3] = {{a->samples, (size_t)((M - 1) * a->ld_samples + D) * 4},
                        {a->targets, a->targets ? (size_t)M * 4 : 0},
                        {a->index, (size_t)((N - 1) * a->s_index + S * B) * 4}};
    const Span o[3] = {{a->data, (size_t)((N - 1) * a->s_data + B * D) * 4},
                       {a->labels, a->labels ? (size_t)((N - 1) * a->s_labels + B) * 4 : 0},
                       {a->cursor, a->cursor ? (size_t)4 : 0}};
    static const char *const in_name[3] = {"samples", "targets", "index"};
    static const char *const out_name[3] = {"data", "labels", "cursor"};
    if (const int rc = check_disjoint("dl_batch_gather", o, out_name, 3, in, in_name, 3, err))
        return rc;
    if (!out) return DL_OK;
    BatchGatherPlan &p = *out;
    const int32_t dim4 = (int32_t)(D / 4);
    p.wide = dim4 >= 64;
    int sh = 6;
    if (!p.wide)
        for (sh = 0; (1 << sh) < dim4; ++sh) {}
    p.wave_rows = kGatherRowsInFlight * (64 >> sh);
    const int64_t rows = N * B;
    const int64_t passes = (rows + p.wave_rows - 1) / p.wave_rows;
    const int64_t wmax = (int64_t)(n_cus > 0 ? n_cus : 1) * kGatherWavesPerCu;
    const int64_t waves = passes < wmax ? passes : wmax;
    const int wpg = kGatherThreads / 64;
    p.grid = (int32_t)((waves + wpg - 1) / wpg);
    int64_t st = a->step % S;   // the host step, non-negative
    if (st < 0) st += S;
    p.k = BatchGatherArgs{a->samples, a->ld_samples, a->targets, a->index, a->s_index, a->cursor,
                          a->data, a->s_data, a->labels, a->s_labels, a->n_samples, dim4,
                          a->batch, a->steps, (int32_t)st, (int32_t)rows, sh};
    return DL_OK;
}

int shape_image_batch(const dl_image_batch_args *a, int n_cus, ImageBatchPlan *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_image_batch: args is NULL");
    const int64_t N = a->n_agents, B = a->batch, S = a->steps, M = a->n_samples;
    const int64_t C = a->channels, H = a->height, W = a->width;
    if (!a->samples || !a->index || !a->data || !a->lut)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: null samples, index, data or lut");
    if (N < 1 || B < 1 || S < 1 || M < 1)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: n_agents, batch, steps and n_samples "
                                         "must be >= 1 (got %d, %d, %d, %d)", a->n_agents,
                    a->batch, a->steps, a->n_samples);
    if (H < 1 || W < 1)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: height and width must be >= 1 (got %d, "
                                         "%d)", a->height, a->width);
    if (C < 1 || C > kImageMaxChannels)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: channels must lie in [1, %d] (got %d)",
                    kImageMaxChannels, a->channels);
    if (W % 4)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: width must be a multiple of 4 (got %d)",
                    a->width);
    // an image's bytes and floats are 32-bit offsets in the kernel (H * W < 2^62: no overflow)
    if (H * W > (1 << 28) || C * H * W > (1 << 28))
        return fail(err, DL_ERR_INVALID, "dl_image_batch: channels * height * width must be at "
                                         "most 2^28");
    const int64_t D = C * H * W;
    if (a->pad < 0 || a->pad > 127)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: pad must lie in [0, 127] (got %d)",
                    a->pad);
    if (a->fill < 0 || a->fill > 255)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: fill must lie in [0, 255] (got %d)",
                    a->fill);
    if (N * B > 0x7fffffff || S * B > 0x7fffffff)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: n_agents * batch and steps * batch "
                                         "must be < 2^31");
    if (reinterpret_cast<uintptr_t>(a->samples) & 3u)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: samples must be 4-byte aligned");
    if (a->ld_samples < D || (a->ld_samples & 3))
        return fail(err, DL_ERR_INVALID, "dl_image_batch: ld_samples must be a multiple of 4 >= "
                                         "channels * height * width (got %lld)",
                    (long long)a->ld_samples);
    if (!aligned16(a->data) || !aligned16(a->lut))
        return fail(err, DL_ERR_INVALID, "dl_image_batch: data and lut must be 16-byte aligned");
    if (a->s_data < B * D || (a->s_data & 3))
        return fail(err, DL_ERR_INVALID, "dl_image_batch: s_data must be a multiple of 4 >= "
                                         "batch * channels * height * width (got %lld)",
                    (long long)a->s_data);
    if (a->s_index != 0 && a->s_index < S * B)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: s_index must be 0 (shared) or >= steps "
                                         "* batch (got %lld)", (long long)a->s_index);
    if (a->aug && a->s_aug != 0 && a->s_aug < S * B)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: s_aug must be 0 (shared) or >= steps "
                                         "* batch (got %lld)", (long long)a->s_aug);
    if (a->labels && !a->targets)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: labels need targets");
    if (a->labels && a->s_labels < B)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: s_labels must be >= batch (got %lld)",
                    (long long)a->s_labels);
    if (a->advance != 0 && a->advance != 1)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: advance must be 0 or 1");
    if (a->advance && !a->cursor)
        return fail(err, DL_ERR_INVALID, "dl_image_batch: advance needs a cursor");
    const Span in[5] = {{a->samples, (size_t)((M - 1) * a->ld_samples + D)},
                        {a->targets, a->targets ? (size_t)M * 4 : 0},
                        {a->index, (size_t)((N - 1) * a->s_index + S * B) * 4},
                        {a->aug, a->aug ? (size_t)((N - 1) * a->s_aug + S * B) * 4 : 0},
                        {a->lut, (size_t)C * 256 * 4}};
    const Span o[3] = {{a->data, (size_t)((N - 1) * a->s_data + B * D) * 4},
                       {a->labels, a->labels ? (size_t)((N - 1) * a->s_labels + B) * 4 : 0},
                       {a->cursor, a->cursor ? (size_t)4 : 0}};
    static const char *const in_name[5] = {"samples", "targets", "index", "aug", "lut"};
    static const char *const out_name[3] = {"data", "labels", "cursor"};
    if (const int rc = check_disjoint("dl_image_batch", o, out_name, 3, in, in_name, 5, err))
        return rc;
    if (!out) return DL_OK;
    ImageBatchPlan &p = *out;
    int sh = 0;
    while (sh < 6 && (1 << sh) < W / 4) ++sh;
    p.pass_rows = kImageRowsInFlight * (64 >> sh);
    p.lds_bytes = (int32_t)(C * 256 * 4);
    const int64_t images = N * B;
    const int64_t wmax = (int64_t)(n_cus > 0 ? n_cus : 1) * kImageWavesPerCu;
    const int64_t waves = images < wmax ? images : wmax;
    const int wpg = kImageThreads / 64;
    p.grid = (int32_t)((waves + wpg - 1) / wpg);
    int64_t st = a->step % S;   // the host step, non-negative
    if (st < 0) st += S;
    p.k = ImageBatchArgs{a->samples, a->ld_samples, a->targets, a->lut, a->index, a->s_index,
                         a->aug, a->s_aug, a->cursor, a->data, a->s_data, a->labels, a->s_labels,
                         a->n_samples, a->channels, a->height, a->width, a->pad,
                         (uint32_t)a->fill * 0x01010101u, a->batch, a->steps, (int32_t)st,
                         (int32_t)images, sh};
    return DL_OK;
}

LenetWs lenet_workspace(int32_t n_agents, int32_t batch, int32_t num_classes) {
    LenetWs w{};
    if (n_agents < 1 || batch < 1 || num_classes < 1) return w;
    const size_t nb = (size_t)n_agents * (size_t)batch;
    const size_t groups = ((size_t)batch + kLenetGroup - 1) / kLenetGroup;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes);
        return at;
    };
    w.pool1 = take(nb * kLenetPool1 * 4);
    w.code1 = take(nb * kLenetPool1);
    w.pool2 = take(nb * kLenetPool2 * 4);
    w.code2 = take(nb * kLenetPool2);
    w.h1 = take(nb * kLenetFc1 * 4);
    w.h2 = take(nb * kLenetFc2 * 4);
    w.z = take(nb * (size_t)num_classes * 4);
    w.dz3 = take(nb * (size_t)num_classes * 4);
    w.dz2 = take(nb * kLenetFc2 * 4);
    w.dz1 = take(nb * kLenetFc1 * 4);
    w.da = take(nb * kLenetPool2 * 4);
    w.part = take((size_t)n_agents * groups * kLenetConvParams * 4);
    w.total = off;
    return w;
}

namespace {
// One operand of a per-agent GEMM: the matrix, its leading dimension, the agent stride and whether
// it enters transposed.
struct Mat {
    const float *p;
    int64_t ld, stride;
    int t;
};

// dl_lenet_grad's launches in order, from the plan's geometry and workspace regions.
void lenet_steps(const dl_lenet_args &a, char *ws, LenetPlan *out) {
    LenetPlan &p = *out;
    const int32_t N = a.n_agents, B = a.batch, nc = a.num_classes;
    const int F1 = kLenetFc1, F2 = kLenetFc2, P2 = kLenetPool2;
    const int fc3b = kLenetFc3W + F2 * nc;   // fc3.bias follows fc3.weight [nc][84]
    auto region = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    float *pool2 = region(p.ws.pool2), *h1 = region(p.ws.h1), *h2 = region(p.ws.h2);
    float *z = region(p.ws.z), *dz3 = region(p.ws.dz3), *dz2 = region(p.ws.dz2);
    float *dz1 = region(p.ws.dz1), *da = region(p.ws.da);
    p.conv = LenetConvArgs{a.X, a.ldx, a.data, a.s_data, region(p.ws.pool1),
                           reinterpret_cast<uint8_t *>(ws + p.ws.code1), pool2,
                           reinterpret_cast<uint8_t *>(ws + p.ws.code2), da, region(p.ws.part),
                           a.G, a.ldg, B, p.train, p.passes, p.fwd_wpa, p.groups, p.bwd_wpa};
    // the operands: an activation or its gradient [batch][cols] per agent in the workspace; a
    // weight [rows][cols] at its offset in the parameter row, as stored (x . W) or transposed
    // (x . W^T: a Linear layer's forward); the same block of the gradient row
    auto act = [&](float *m, int cols) { return Mat{m, cols, (int64_t)B * cols, 0}; };
    auto actT = [&](float *m, int cols) { return Mat{m, cols, (int64_t)B * cols, 1}; };
    auto weight = [&](int off, int cols) { return Mat{a.X + off, cols, a.ldx, 0}; };
    auto weightT = [&](int off, int cols) { return Mat{a.X + off, cols, a.ldx, 1}; };
    auto grad = [&](int off, int cols) { return Mat{a.G + off, cols, a.ldg, 0}; };
    p.n_launches = 0;
    auto step = [&](int32_t kind) -> LenetStep & {
        LenetStep &s = p.step[p.n_launches++];
        s = LenetStep{};
        s.kind = kind;
        return s;
    };
    // C (M x Nn) = op(A) op(Bm) per agent, then the epilogue
    auto gemm = [&](int M, int Nn, int K, Mat A, Mat Bm, Mat C, int epi) -> BgemmArgs & {
        BgemmArgs &g = step(kLenetGemm).gemm;
        g.batch = N; g.M = M; g.N = Nn; g.K = K;
        g.A = A.p; g.lda = A.ld; g.sA = A.stride; g.ta = A.t;
        g.B = Bm.p; g.ldb = Bm.ld; g.sB = Bm.stride; g.tb = Bm.t;
        g.C = const_cast<float *>(C.p); g.ldc = C.ld; g.sC = C.stride;
        g.epi = epi;
        g.sBias = a.ldx;   // a bias is a block of the parameter row, a row sum of the gradient row
        g.sR = a.ldg;
        return g;
    };
    auto relu_of = [&](BgemmArgs &g, const float *h, int cols) {   // EPI_DRELU's activations
        g.H = h; g.ldh = cols; g.sH = (int64_t)B * cols;
    };

    step(kLenetConvFwd);
    gemm(B, F1, P2, act(pool2, P2), weightT(kLenetFc1W, P2), act(h1, F1), EPI_BIAS_RELU).bias =
        a.X + kLenetFc1B;
    gemm(B, F2, F1, act(h1, F1), weightT(kLenetFc2W, F1), act(h2, F2), EPI_BIAS_RELU).bias =
        a.X + kLenetFc2B;
    const Mat fc3 = weightT(kLenetFc3W, F2);
    if (a.logits)
        gemm(B, nc, F2, act(h2, F2), fc3, Mat{a.logits, a.ldz, a.s_logits, 0}, EPI_BIAS).bias =
            a.X + fc3b;
    if (p.head == 1) {
        BgemmArgs &g = gemm(B, nc, F2, act(h2, F2), fc3, act(dz3, nc), EPI_BIAS_XENT);
        g.bias = a.X + fc3b;
        g.labels = a.labels; g.sLab = a.s_labels; g.loss = a.loss;   // dZ3 and the loss in one
    } else if (p.head == 2) {
        gemm(B, nc, F2, act(h2, F2), fc3, act(z, nc), EPI_BIAS).bias = a.X + fc3b;
        step(kLenetHead).head = XentArgs{z, (int64_t)B * nc, a.labels, a.s_labels, dz3,
                                         (int64_t)B * nc, a.loss, N, B, nc};
    }
    if (!p.train) return;
    // weight gradients dZ^T . (layer input) straight into G, bias gradients as row sums; dZ of
    // the layer below through the weights, times ReLU's derivative
    gemm(nc, F2, B, actT(dz3, nc), act(h2, F2), grad(kLenetFc3W, F2), EPI_NONE).rowsum = a.G + fc3b;
    relu_of(gemm(B, F2, nc, act(dz3, nc), weight(kLenetFc3W, F2), act(dz2, F2), EPI_DRELU), h2, F2);
    gemm(F2, F1, B, actT(dz2, F2), act(h1, F1), grad(kLenetFc2W, F1), EPI_NONE).rowsum =
        a.G + kLenetFc2B;
    relu_of(gemm(B, F1, F2, act(dz2, F2), weight(kLenetFc2W, F1), act(dz1, F1), EPI_DRELU), h1, F1);
    gemm(F1, P2, B, actT(dz1, F1), act(pool2, P2), grad(kLenetFc1W, P2), EPI_NONE).rowsum =
        a.G + kLenetFc1B;
    // the gradient entering the second pooling: dZ1 . fc1.weight
    gemm(B, P2, F1, act(dz1, F1), weight(kLenetFc1W, P2), act(da, P2), EPI_NONE);
    step(kLenetConvBwd);
    step(kLenetConvReduce);
}
}  // namespace

int shape_lenet(const dl_lenet_args *a, int n_cus, void *ws, size_t ws_bytes, LenetPlan *out,
                char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_lenet_grad: args is NULL");
    const int64_t N = a->n_agents, B = a->batch, nc = a->num_classes;
    if (!a->X || !a->data) return fail(err, DL_ERR_INVALID, "dl_lenet_grad: null X or data");
    if (!a->G && !a->loss && !a->logits)
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: no output (G, loss and logits all NULL)");
    if ((a->G || a->loss) && !a->labels)
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: G and loss need labels");
    if (N < 1 || B < 1)
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: n_agents and batch must be >= 1 (got "
                                         "%d, %d)", a->n_agents, a->batch);
    if (N > 65535)
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: at most 65535 agents (got %d)",
                    a->n_agents);
    if (nc < 1)
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: num_classes must be >= 1 (got %d)",
                    a->num_classes);
    if (nc > kLenetMaxClasses)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_lenet_grad: the cross-entropy head takes at most "
                                             "%d classes (got %d)", kLenetMaxClasses,
                    a->num_classes);
    const int64_t P = lenet_param_count(a->num_classes);
    if (!aligned16(a->X) || !aligned16(a->data) || (a->G && !aligned16(a->G)))
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: X, data and G must be 16-byte aligned");
    if (a->ldx < P || (a->ldx & 3))
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: ldx must be a multiple of 4 >= %lld "
                                         "parameters (got %lld)", (long long)P, (long long)a->ldx);
    if (a->G && (a->ldg < P || (a->ldg & 3)))
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: ldg must be a multiple of 4 >= %lld "
                                         "parameters (got %lld)", (long long)P, (long long)a->ldg);
    if (a->s_data != 0 && (a->s_data < B * kLenetImage || (a->s_data & 3)))
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: s_data must be 0 (shared) or a multiple "
                                         "of 4 >= batch * 3072 (got %lld)", (long long)a->s_data);
    if (a->labels && a->s_labels != 0 && a->s_labels < B)
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: s_labels must be 0 (shared) or >= batch "
                                         "(got %lld)", (long long)a->s_labels);
    if (a->logits && (a->ldz < nc || (N > 1 && a->s_logits < (B - 1) * a->ldz + nc)))
        return fail(err, DL_ERR_INVALID, "dl_lenet_grad: logits need ldz >= num_classes and "
                                         "s_logits >= (batch - 1) * ldz + num_classes (got ldz "
                                         "%lld, s_logits %lld)", (long long)a->ldz,
                    (long long)a->s_logits);
    const LenetWs w = lenet_workspace(a->n_agents, a->batch, a->num_classes);
    if (!ws_holds(ws, ws_bytes, w.total))
        return fail(err, DL_ERR_WORKSPACE, "dl_lenet_grad: needs a 16-byte aligned workspace of "
                                           "%zu bytes (dl_lenet_workspace_bytes)", w.total);
    const Span in[3] = {{a->X, (size_t)((N - 1) * a->ldx + P) * 4},
                        {a->data, (size_t)((N - 1) * a->s_data + B * kLenetImage) * 4},
                        {a->labels, a->labels ? (size_t)((N - 1) * a->s_labels + B) * 4 : 0}};
    const Span o[4] = {{a->G, a->G ? (size_t)((N - 1) * a->ldg + P) * 4 : 0},
                       {a->loss, a->loss ? (size_t)N * 4 : 0},
                       {a->logits, a->logits ? (size_t)((N - 1) * a->s_logits + (B - 1) * a->ldz +
                                                        nc) * 4 : 0},
                       {ws, w.total}};
    static const char *const in_name[3] = {"X", "data", "labels"};
    static const char *const out_name[4] = {"G", "loss", "logits", "workspace"};
    if (const int rc = check_disjoint("dl_lenet_grad", o, out_name, 4, in, in_name, 3, err))
        return rc;
    if (!out) return DL_OK;
    LenetPlan &p = *out;
    p.train = a->G ? 1 : 0;
    p.head = (a->G || a->loss) ? (B <= 64 ? 1 : 2) : 0;
    p.passes = (int32_t)((B + kLenetFwdImages - 1) / kLenetFwdImages);
    p.groups = (int32_t)((B + kLenetGroup - 1) / kLenetGroup);
    const int64_t want = ((int64_t)kLenetWgPerCu * (n_cus > 0 ? n_cus : 1) + N - 1) / N;
    p.fwd_wpa = (int32_t)(want < p.passes ? want : p.passes);
    p.bwd_wpa = (int32_t)(want < p.groups ? want : p.groups);
    p.fwd_grid = (int32_t)(N * p.fwd_wpa);   // <= 65535 + 4 * n_cus
    p.bwd_grid = (int32_t)(N * p.bwd_wpa);
    p.ws = w;
    p.n_agents = a->n_agents;
    lenet_steps(*a, static_cast<char *>(ws), &p);
    return DL_OK;
}

LenetEvalWs lenet_eval_workspace(int32_t n_agents, int32_t rows) {
    LenetEvalWs w{};
    if (n_agents < 1 || rows < 1) return w;
    w.hit = eval_part_bytes(n_agents, rows);
    w.total = 2 * w.hit;
    return w;
}

int shape_lenet_eval(const dl_lenet_eval_args *a, int n_cus, const void *ws, size_t ws_bytes,
                     bool check_ws, dl_lenet_eval_plan *out, char *err) {
    if (!a) return fail(err, DL_ERR_INVALID, "dl_lenet_eval: args is NULL");
    const int64_t N = a->n_agents, R = a->rows, nc = a->num_classes;
    if (!a->X || !a->data) return fail(err, DL_ERR_INVALID, "dl_lenet_eval: null X or data");
    if (!a->loss && !a->correct && !a->logits)
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: no output (loss, correct and logits all "
                                         "NULL)");
    if ((a->loss || a->correct) && !a->labels)
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: loss and correct need labels");
    if (N < 1) return fail(err, DL_ERR_INVALID, "dl_lenet_eval: n_agents must be >= 1 (got %d)",
                           a->n_agents);
    if (N > 65535)
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: at most 65535 agents (got %d)",
                    a->n_agents);
    if (R < 1) return fail(err, DL_ERR_INVALID, "dl_lenet_eval: rows must be >= 1 (got %d)",
                           a->rows);
    if (nc < 1)
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: num_classes must be >= 1 (got %d)",
                    a->num_classes);
    if (nc > kLenetMaxClasses)
        return fail(err, DL_ERR_UNSUPPORTED, "dl_lenet_eval: the cross-entropy head takes at most "
                                             "%d classes (got %d)", kLenetMaxClasses,
                    a->num_classes);
    const int64_t P = lenet_param_count(a->num_classes);
    if (!aligned16(a->X) || !aligned16(a->data))
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: X and data must be 16-byte aligned");
    if (a->ldx < P || (a->ldx & 3))
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: ldx must be a multiple of 4 >= %lld "
                                         "parameters (got %lld)", (long long)P, (long long)a->ldx);
    if (a->s_data != 0 && (a->s_data < R * kLenetImage || (a->s_data & 3)))
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: s_data must be 0 (shared) or a multiple "
                                         "of 4 >= rows * 3072 (got %lld)", (long long)a->s_data);
    if (a->labels && a->s_labels != 0 && a->s_labels < R)
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: s_labels must be 0 (shared) or >= rows "
                                         "(got %lld)", (long long)a->s_labels);
    if (a->logits && (a->ldz < nc || (N > 1 && a->s_logits < (R - 1) * a->ldz + nc)))
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: logits need ldz >= num_classes and "
                                         "s_logits >= (rows - 1) * ldz + num_classes (got ldz "
                                         "%lld, s_logits %lld)", (long long)a->ldz,
                    (long long)a->s_logits);
    if (a->row_splits < 0)
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: row_splits must be >= 0 (got %d)",
                    a->row_splits);
    const LenetEvalWs w = lenet_eval_workspace(a->n_agents, a->rows);
    if (check_ws && !ws_holds(ws, ws_bytes, w.total))
        return fail(err, DL_ERR_WORKSPACE, "dl_lenet_eval: needs a 16-byte aligned workspace of "
                                           "%zu bytes (dl_lenet_eval_workspace_bytes)", w.total);
    const Span in[3] = {{a->X, (size_t)((N - 1) * a->ldx + P) * 4},
                        {a->data, (size_t)((N - 1) * a->s_data + R * kLenetImage) * 4},
                        {a->labels, a->labels ? (size_t)((N - 1) * a->s_labels + R) * 4 : 0}};
    const Span o[4] = {{a->loss, a->loss ? (size_t)N * 4 : 0},
                       {a->correct, a->correct ? (size_t)N * 4 : 0},
                       {a->logits, a->logits ? (size_t)((N - 1) * a->s_logits + (R - 1) * a->ldz +
                                                        nc) * 4 : 0},
                       {ws, check_ws ? w.total : 0}};
    static const char *const in_name[3] = {"X", "data", "labels"};
    static const char *const out_name[4] = {"loss", "correct", "logits", "workspace"};
    if (const int rc = check_disjoint("dl_lenet_eval", o, out_name, 4, in, in_name, 3, err))
        return rc;
    const int32_t blocks = eval_blocks(a->rows);
    int64_t rs = a->row_splits > 0
                     ? a->row_splits
                     : ((int64_t)kLenetEvalWgPerCu * (n_cus > 0 ? n_cus : 1) + N - 1) / N;
    if (rs > blocks) rs = blocks;
    if (rs < 1) rs = 1;
    if (N * rs > 0x7fffffff)   // only a hint can ask for this: the chosen rs is <= 2 n_cus
        return fail(err, DL_ERR_INVALID, "dl_lenet_eval: grid too large (n_agents * row_splits "
                                         "must be < 2^31)");
    if (out)
        *out = dl_lenet_eval_plan{blocks, (int32_t)rs, (int32_t)(N * rs), kLenetEvalLdsBytes};
    return DL_OK;
}

}  // namespace dl
