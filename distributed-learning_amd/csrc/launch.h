// Launch shaping: host-only C++17, no HIP, like the planner beside it.  Pure functions of (args,
// compute units, knobs, workspace pointer and size) that validate a call and describe what it
// launches -- every kernel's parameter, grid, LDS bytes and selectors, and the step after the
// launches; the C ABI (capi.hip) turns the description into launch_* calls.  Shaped here: the
// rounds (dl_mix_round, dl_mix_rounds, dl_mix_rounds_trace, dl_sgd_round, dl_cheb_round,
// dl_track_round, dl_adam_round and their plan queries),
// the one-pass deviation, dl_mlp_grad, dl_mlp_eval, dl_bgemm, dl_batch_gather, dl_image_batch,
// dl_lenet_grad and dl_lenet_eval.  Not shaped here (capi.hip checks them itself, their LDS-size
// functions live in kernel files): dl_mix_until, dl_consensus_gd, dl_perron_round, the two-pass
// deviation, the conversions and the step-rows functions.
#pragma once
#include "plan.h"

namespace dl {

struct TileArgs {
    const float *x;
    int64_t ldx;
    const float *halo;
    int64_t ldh;
    const float *g;
    int64_t ldg;
    float *y;
    int64_t ldy;
    const int32_t *rowptr;
    const int32_t *col;
    const float *w;
    int32_t n_rows;   // output rows (local agents)
    int32_t n_src;    // rows staged in LDS = n_loc + n_halo
    int32_t n_loc;    // source rows read from x (and stepped with g); n_rows unless the round
                      // mixes one row set of an agent partition from a wider local window
    int32_t nnz;
    int32_t regular;  // >0: every row has exactly `regular` entries (row_ptr not staged)
    int32_t n_w;      // weights staged in LDS: nnz, or `regular` when every row shares row 0's
    int32_t mean_from_inputs;  // 1: W doubly stochastic -> tile mean taken from the staged t
    int32_t nt_store;          // 1: non-temporal stores of y (FAST path)
    int32_t nt_load;           // non-temporal loads (FAST path): bit 0 x / halo, bit 1 g
    int64_t n_params;
    int32_t n_tiles;
    int64_t col_base; // first column of tile 0
    float lr;
    int32_t vec;      // 1: x/g/y/halo 16-byte aligned and ld % 4 == 0
    uint32_t csr_off; // byte offset of the staged CSR in LDS
    uint32_t scratch_off; // byte offset of the 16 x C float4 mean scratch in LDS
    // FAST-path strides in bytes: tile stride (next tile's row 0) and row stride.
    //   row-major:      xts = T*4,          xrs = ldx*4   (tile base also offset by col_base)
    //   column-tiled:   xts = n_rows*T*4,   xrs = T*4     (block [n_rows][T] per tile)
    int32_t tiled;
    int64_t xts, gts, yts;
    uint32_t xrs, grs, yrs;
    uint32_t hrs;     // halo row stride in bytes (ldh*4)
    int32_t lchunks;     // mix_trace_kernel: float4 chunks per operand tile (1 = row-major)
    float *dev_partial;  // [gridDim.x][n_rows] per-workgroup partial ||y_a - mean||^2
                         // (lagged halo deviation: [gridDim.x][n_loc], one per source row)
    float *mean;         // [n_params] nullable
    unsigned int *dev_max_zero;  // nullable: workgroup 0 zeroes it (dev_reduce's atomicMax target,
                                 // so that launch needs no memset of its own)
    const float *mean_prev;      // halo rounds: global column mean of x (lagged deviation)
    float *colsum_out;           // halo rounds: this rank's column sums of y
    // column-tiled halo (tiled != 0, n_src > n_loc): n_hblk per-peer blocks back to back; block
    // b holds halo rows [hblk_row0[b], hblk_row0[b + 1]) as [n_tiles][rows_b][T], starting
    // hblk_off[b] bytes into `halo`
    int32_t n_hblk;
    int32_t hblk_row0[17];
    uint32_t hblk_off[16];
    // path 5: rows [0, n_hub) folded by four column lanes each; their register heads as
    // {weight, row} pairs at LDS byte offset hub_off
    int32_t n_hub;
    uint32_t hub_off;
    // column-tiled partition rounds (FAST): one kernel tile = `grp` consecutive data tiles of T
    // columns (chunk c of a kernel row is chunk c & (2^cd_sh - 1) of data tile c >> cd_sh), so a
    // short launch moves grp times the bytes per pass; grp = 1 (the default) is the plain tile
    int32_t grp;
    int32_t cd_sh;
    int32_t tile_run;          // 0: workgroup b walks tiles b, b + grid, ...; > 0: the run
                               // [b * tile_run, (b + 1) * tile_run) (Knobs::tile_run)
};
constexpr int kMaxHaloBlocks = 16;

// a round of an agent partition: halo source rows, or output rows that are not the source rows
inline bool mix_partitioned(const dl_mix_args &a) {
    return a.n_halo > 0 || local_src(a) != a.W.n_rows;
}
inline bool tile_partitioned(const TileArgs &a) {
    return a.n_src != a.n_rows || a.n_loc != a.n_rows;
}
// ... with the lagged deviation (the halo instantiations' LAG)
inline bool tile_lag(const TileArgs &a) {
    return tile_partitioned(a) && (a.mean_prev != nullptr || a.colsum_out != nullptr);
}

constexpr size_t kWsAlign = 256;
constexpr size_t align_up(size_t v) { return (v + kWsAlign - 1) & ~(kWsAlign - 1); }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// do the an bytes at a and the bn bytes at b share a byte
inline bool overlaps(const void *a, size_t an, const void *b, size_t bn) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bn && y < x + an;
}
// workspace bytes of `parts` partial rows of `rows` floats, and whether ws holds `need` of them
constexpr size_t partial_bytes(int64_t parts, int64_t rows) {
    return align_up((size_t)parts * (size_t)rows * 4);
}
inline bool ws_holds(const void *ws, size_t ws_bytes, size_t need) {
    return ws && aligned16(ws) && ws_bytes >= need;
}

// The optimizer of dl_sgd_step and the fused momentum round (sgd_elem.h), and the round's momentum
// buffers: laid out as x, with their FAST-path strides (tile_stride).  buf is read only when mu
// != 0.
struct SgdParams {
    float lr, mu, damp, wd;
    int first, nesterov;
};
struct SgdTileArgs {
    float *buf;
    int64_t ldb;
    int64_t bts;    // FAST-path tile stride in bytes
    uint32_t brs;   // FAST-path row stride in bytes
    SgdParams p;
};

// The Chebyshev round's second operand (mix_cheb.hip): z laid out as x, with its FAST-path
// strides (tile_stride), and the two coefficients of y = fl(fl(a * W x) + fl(b * z)).
struct ChebTileArgs {
    const float *z;
    int64_t ldz;
    int64_t zts;    // FAST-path tile stride in bytes
    uint32_t zrs;   // FAST-path row stride in bytes
    float a, b;
};

// The gradient-tracking round's operands beside x, g and y (mix_track.hip): the tracker d, its
// output d_out (d itself or apart) and last step's gradient q, each laid out as x, with their
// FAST-path strides (tile_stride).  This step's gradient and lr travel in TileArgs (g, lr) as the
// plain round's do.
struct TrackTileArgs {
    const float *d;
    int64_t ldd;
    float *d_out;
    int64_t lddo;
    const float *q;
    int64_t ldq;
    int64_t dts, dots, qts;   // FAST-path tile strides in bytes
    uint32_t drs, dors, qrs;  // FAST-path row strides in bytes
};

// Adam's element arithmetic (adam_elem.h), shared by dl_adam_step and the fused Adam round: the
// host-prepared fp32 constants omb1 = fl32(1 - beta1), omb2 = fl32(1 - beta2) and decay = fl32(1 -
// lr wd), each formed in fp64, and the bias-correction coefficients ss = fl32(lr / (1 - beta1^t))
// and bs = fl32(sqrt(1 - beta2^t)) -- by value, or when coef != NULL read from coef[0] and
// coef[1] on the device (dl_adam_tick's outputs).
struct AdamParams {
    float b2, omb1, omb2, eps, wd, decay;
    float ss, bs;
    int decoupled;
    const float *coef;
};
AdamParams adam_params(double beta1, double beta2, float eps, float lr, float wd, int decoupled,
                       float ss, float bs, const float *coef);
// beta1, beta2 in [0, 1), eps >= 0, and finite coefficients when they are passed by value; a
// text for `who` in err and DL_ERR_INVALID otherwise
int check_adam_params(const char *who, double beta1, double beta2, float eps, float ss, float bs,
                      const float *coef, char *err);
// The Adam round's moments (mix_adam.hip): m and v laid out as x, each read and written in place,
// with their FAST-path strides (tile_stride).
struct AdamTileArgs {
    float *m;
    int64_t ldm;
    float *v;
    int64_t ldv;
    int64_t mts, vts;    // FAST-path tile strides in bytes
    uint32_t mrs, vrs;   // FAST-path row strides in bytes
    AdamParams p;
};

// One kernel launch.  `t` is the kernel's parameter; the selectors pick the instantiation as the
// launch_* functions of dl_internal.h take them.
enum LaunchKind : int32_t {
    kLaunchTile,      // launch_mix_tile(t, chunks, sgd, dev, mix, grid, lds, fast)
    kLaunchSgdTile,   // launch_mix_sgd_tile(t, q, chunks, dev, grid, lds, fast)
    kLaunchTileReg,   // launch_mix_tile_reg(t, chunks, head, tail_fmt, sgd, dev, grid, lds)
    kLaunchGather,    // launch_mix_gather(t, sgd, columns)
    kLaunchMulti,     // launch_mix_multi(t, chunks, rounds, sgd, dev, grid, lds)
    kLaunchTrace,     // launch_mix_trace(t, chunks, planes, rounds, grid, lds, trace): + its reduce
    kLaunchTraceIrr,  // launch_mix_trace_irr(t, head, gm, narrow, rounds, grid, lds, trace): same
    kLaunchChebTile,  // launch_mix_cheb_tile(t, c, chunks, dev, grid, lds, fast)
    kLaunchTrackTile, // launch_mix_track_tile(t, k, chunks, dev, grid, lds, fast)
    kLaunchAdamTile,  // launch_mix_adam_tile(t, a, chunks, dev, grid, lds, fast)
};
struct Launch {
    int32_t kind;
    int32_t grid, lds;
    int32_t chunks, head, tail_fmt, rounds;
    bool sgd, dev, mix, fast;
    bool columns;              // gather: Knobs::gather_order_columns
    bool planes, gm, narrow;   // traced passes
    TileArgs t;
    SgdTileArgs q;             // kLaunchSgdTile
    ChebTileArgs c;            // kLaunchChebTile
    TrackTileArgs k;           // kLaunchTrackTile
    AdamTileArgs a;            // kLaunchAdamTile
};
// What follows the launches on the stream.
enum After : int32_t {
    kAfterNothing,
    kAfterZero,         // zero dev_sq / dev_max (one agent: no deviation)
    kAfterReduce,       // launch_dev_reduce(partial, parts, rows, dev_sq, dev_max, max_zeroed)
    kAfterPartialRows,  // leave the partial rows in the workspace, *partial_rows_out = parts
    kAfterTwoPass,      // the two-pass deviation of y (the gather path)
};
struct Launches {
    int32_t n;
    Launch l[2];
    int32_t after;
    const float *partial;   // kAfterReduce
    int32_t parts, rows;    // kAfterReduce, kAfterPartialRows (parts)
    bool max_zeroed;
};

// Argument check of every round entry point; the texts say dl_mix_round for all of them.
// y_may_be_x: y == x with ldy == ldx is accepted (the fused momentum round mixes in place).
int check_mix_args(const dl_mix_args *a, char *err, bool y_may_be_x = false);
// The kernels' view of a round's operands: sizes, float4 eligibility, cache policy, halo blocks.
TileArgs tile_args(const dl_mix_args &a, const Knobs &k);
// FAST-path strides in bytes of one operand for tiles of T columns: the next tile's row 0 (*ts)
// and the next row (*rs).  A column-tiled operand's tile stride is its block rows (ld, 0 = its
// own `rows`) x T floats.
void tile_stride(bool tiled, int64_t ld, int64_t rows, int64_t T, int64_t *ts, uint32_t *rs);

// The entry points, after check_mix_args: plan (plan.h) and shape.  Each returns a dl_status
// and, on failure, the dl_last_error() text in err[kErrLen].
// vec_ok = false: an operand the args do not describe (the fused momentum round's buffers) rules
// the float4 kernels out
int shape_round(const dl_mix_args &a, int n_cus, const Knobs &k, void *ws, size_t ws_bytes,
                Launches *out, char *err, bool vec_ok = true);
// The fused rounds (dl_X_round / dl_X_round_plan), one sequence in the header's order: the
// entry point's own null checks, whole rounds only (no halo, partition or lagged field) and the
// round's checks with y == x allowed, the layouts and overlaps of the operands the round adds,
// the plan (refused unless path 1; copied to *plan when given), then shape_round with the float4
// kernels ruled out when they cannot reach an added operand, every launch re-tagged with the
// round's kind and given its extra args.  out NULL: the plan query, which stops after the plan
// and needs `plan`.  What each adds:
// momentum buffers when momentum != 0, the Nesterov rule; kLaunchSgdTile with SgdTileArgs
int shape_sgd_round(const dl_sgd_round_args *a, int n_cus, const Knobs &k, void *ws,
                    size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err);
// z (y may be z itself), g refused before anything else; kLaunchChebTile with ChebTileArgs
int shape_cheb_round(const dl_cheb_round_args *a, int n_cus, const Knobs &k, void *ws,
                     size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err);
// d, d_out (may be d itself) and g_old, every other overlap of an output refused;
// kLaunchTrackTile with TrackTileArgs
int shape_track_round(const dl_track_round_args *a, int n_cus, const Knobs &k, void *ws,
                      size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err);
// m and v (each in place), every overlap of either refused, the optimizer's parameter ranges;
// kLaunchAdamTile with AdamTileArgs
int shape_adam_round(const dl_adam_round_args *a, int n_cus, const Knobs &k, void *ws,
                     size_t ws_bytes, dl_mix_plan *plan, Launches *out, char *err);
int shape_rounds(const dl_mix_args &a, int32_t rounds, int n_cus, const Knobs &k, void *ws,
                 size_t ws_bytes, Launches *out, char *err);
int shape_trace(const dl_mix_args &a, int32_t rounds, int n_cus, const Knobs &k, void *ws,
                size_t ws_bytes, Launches *out, char *err);
// One-pass deviation of x on the tile kernel (MIX = false): every agent of a column tile in one
// workgroup, column mean in LDS scratch.  tile_cols > 0: x in the column-tiled layout (ldx 0).
// DL_ERR_UNSUPPORTED without a text: the agents do not fit one tile.
int shape_deviation(const float *x, int64_t ldx, int32_t tile_cols, int32_t n_rows,
                    int64_t n_params, float *mean_out, int n_cus, void *ws, size_t ws_bytes,
                    Launches *out, char *err);

// dl_mlp_eval: rows per block, the LDS of one workgroup (mlp_fused.hip asserts it), and the
// workspace: [n_agents][blocks] float loss parts, then as many int32 correct counts.
constexpr int kEvalBlockRows = 64;
constexpr int kMlpLdsBytes = 156480;
constexpr int32_t eval_blocks(int32_t rows) {
    return (int32_t)(((int64_t)rows + kEvalBlockRows - 1) / kEvalBlockRows);
}
constexpr size_t eval_part_bytes(int32_t n_agents, int32_t rows) {
    return align_up((size_t)n_agents * (size_t)eval_blocks(rows) * 4);
}
constexpr size_t eval_workspace_bytes(int32_t n_agents, int32_t rows) {
    return n_agents > 0 && rows > 0 ? 2 * eval_part_bytes(n_agents, rows) : 0;
}
// dl_mlp_grad's gate and the split gradient path's workspace (dl_mlp_args.workspace: one
// activation buffer per agent), from the fused kernels' geometry (mlp_fused.hip asserts each).
constexpr int kMlpBatch = 64;         // batch rows per agent
constexpr int kMlpMaxHidden = 152;    // hidden width the five K slices and an LDS row hold
constexpr int kMlpMaxOutput = 16;
constexpr int kMlpActStride = 156;    // floats of an activation row in LDS
constexpr bool mlp_fused_supported(int batch, int din, int dh, int dout) {
    return batch == kMlpBatch && din > 0 && din % 4 == 0 && dh > 0 && dh <= kMlpMaxHidden &&
           dh % 2 == 0 && dout > 0 && dout <= kMlpMaxOutput;
}
constexpr size_t mlp_workspace_floats(int n_agents) {
    return (size_t)n_agents * kMlpBatch * kMlpActStride;
}
// Every check of dl_mlp_grad (n_agents == 0 passes: the caller launches nothing).
int shape_mlp_grad(const dl_mlp_args *a, char *err);

// Checks a dl_mlp_eval call and shapes its grid: blocks = ceil(rows / 64); row_splits so that
// n_agents * row_splits workgroups cover the compute units, at most `blocks`; the caller's hint
// (args.row_splits > 0) instead, clamped to [1, blocks].  check_ws: the workspace too
// (dl_mlp_eval; the plan query has none).
int shape_mlp_eval(const dl_mlp_eval_args *a, int n_cus, const void *ws, size_t ws_bytes,
                   bool check_ws, dl_mlp_eval_plan *out, char *err);

// dl_batch_gather: the kernel's parameter (batch_gather.hip) and the launch around it.
struct BatchGatherArgs {
    const float *samples;
    int64_t ld_samples;
    const int32_t *targets;   // nullable with labels
    const int32_t *index;
    int64_t s_index;
    const int32_t *cursor;    // nullable: `step` instead
    float *data;
    int64_t s_data;
    int32_t *labels;          // nullable
    int64_t s_labels;
    int32_t n_samples, dim4;  // dim4: float4 chunks per row
    int32_t batch, steps, step;
    int32_t rows;             // n_agents * batch destination rows
    int32_t lane_sh;          // packed rows: log2 of the lanes that share a row (>= dim4 lanes)
};
constexpr int kGatherThreads = 256;   // four waves
constexpr int kGatherRowsInFlight = 4;
constexpr int kGatherWavesPerCu = 16;
struct BatchGatherPlan {
    int32_t wide;      // 1: one wave per row, scalar row base (dim >= 256); 0: rows packed
    int32_t grid;      // workgroups of kGatherThreads
    int32_t wave_rows; // destination rows one wave has in flight per pass
    BatchGatherArgs k;
};
// Checks a dl_batch_gather call and shapes its launch.  Rows are dealt to waves in passes of
// wave_rows = kGatherRowsInFlight rows (wide: one 256-float piece of a row per wave-instruction)
// or kGatherRowsInFlight * (64 >> lane_sh) rows (packed: dim < 256, 2^lane_sh >= dim / 4 lanes
// per row), grid-strided over min(passes, n_cus * kGatherWavesPerCu) waves.
int shape_batch_gather(const dl_batch_gather_args *a, int n_cus, BatchGatherPlan *out, char *err);

// dl_image_batch: the kernel's parameter (image_batch.hip) and the launch around it.
struct ImageBatchArgs {
    const uint8_t *samples;
    int64_t ld_samples;       // bytes
    const int32_t *targets;   // nullable with labels
    const float *lut;         // [channels][256]
    const int32_t *index;
    int64_t s_index;
    const int32_t *aug;       // nullable: the centre crop, no flip
    int64_t s_aug;
    const int32_t *cursor;    // nullable: `step` instead
    float *data;
    int64_t s_data;
    int32_t *labels;          // nullable
    int64_t s_labels;
    int32_t n_samples, channels, height, width;
    int32_t pad;
    uint32_t fill4;           // the fill byte in all four bytes of a dword
    int32_t batch, steps, step;
    int32_t images;           // n_agents * batch destination images
    int32_t lane_sh;          // log2 of the lanes that share an output row (>= width / 4, <= 64)
};
constexpr int kImageThreads = 256;   // four waves
constexpr int kImageRowsInFlight = 4;
constexpr int kImageWavesPerCu = 16;
constexpr int kImageMaxChannels = 16;
struct ImageBatchPlan {
    int32_t grid;       // workgroups of kImageThreads
    int32_t lds_bytes;  // the staged table: channels * 256 floats
    int32_t pass_rows;  // output rows of one channel a wave has in flight per pass
    ImageBatchArgs k;
};
// Checks a dl_image_batch call and shapes its launch.  A wave owns whole destination images (the
// sample id and the draws are wave-uniform); 2^lane_sh >= width / 4 lanes (at most 64) share an
// output row, four output pixels each, so a wave-instruction covers 64 >> lane_sh rows and a
// pass kImageRowsInFlight times as many.  Images are grid-strided over min(images, n_cus *
// kImageWavesPerCu) waves.
int shape_image_batch(const dl_image_batch_args *a, int n_cus, ImageBatchPlan *out, char *err);

// dl_bgemm's kernel parameter (bgemm.hip) and epilogues (DL_EPI_* of dlamd.h).
enum Epi {
    EPI_NONE = 0,
    EPI_BIAS = 1,
    EPI_BIAS_RELU = 2,
    EPI_BIAS_TANH = 3,
    EPI_BIAS_ELU = 4,
    EPI_DRELU = 5,
    EPI_DTANH = 6,
    EPI_DELU = 7,
    EPI_BIAS_XENT = 8
};
struct BgemmArgs {
    int32_t batch, M, N, K;
    const float *A;
    int64_t lda, sA;
    int32_t ta;
    const float *B;
    int64_t ldb, sB;
    int32_t tb;
    float *C;
    int64_t ldc, sC;
    int32_t epi;
    const float *bias;
    int64_t sBias;
    const float *H;
    int64_t ldh, sH;
    float *rowsum;
    int64_t sR;
    const int32_t *labels;
    int64_t sLab;
    float *loss;
};
// Every check of dl_bgemm, and the kernel's parameter of a call that passed.
int check_bgemm(const dl_bgemm_args *a, char *err);
BgemmArgs bgemm_args(const dl_bgemm_args &a);

// dl_lenet_grad: LeNet's fixed geometry, the workspace regions, the grids of the two
// convolution kernels (lenet.hip) and the launches in order.
constexpr int kLenetImage = 3 * 32 * 32;     // floats of one input image
constexpr int kLenetPool1 = 6 * 14 * 14;     // relu(conv1) pooled: conv2's input
constexpr int kLenetPool2 = 16 * 5 * 5;      // relu(conv2) pooled: fc1's input, index c*25 + y*5 + x
constexpr int kLenetFc1 = 120, kLenetFc2 = 84;
constexpr int kLenetMaxClasses = 64;         // the cross-entropy head's limit
// element offsets of the parameter blocks in a row (Mixer flatten order)
constexpr int kLenetConv1W = 0, kLenetConv1B = 450, kLenetConv2W = 456, kLenetConv2B = 2856;
constexpr int kLenetFc1W = 2872, kLenetFc1B = 50872, kLenetFc2W = 50992, kLenetFc2B = 61072;
constexpr int kLenetFc3W = 61156;
constexpr int kLenetConvParams = kLenetFc1W;   // the 2872 convolution parameters lead the row
constexpr int32_t lenet_param_count(int32_t nc) { return nc < 1 ? 0 : kLenetFc3W + 85 * nc; }
constexpr int kLenetThreads = 256;
constexpr int kLenetFwdImages = 2;   // images a forward workgroup holds in LDS per pass
constexpr int kLenetGroup = 4;       // images of one backward group: fixed, it sets the sum order
// Workgroups per compute unit the grids aim at.  Either kernel holds three a compute unit
// (forward: 51.8 KB of LDS, 130 VGPRs; backward: 143 VGPRs); 4 was chosen because at 64 agents x
// 64 images it gives every workgroup exactly two passes / one group (no uneven split); 3 was
// not measured against it.  Any value gives the same bits.
constexpr int kLenetWgPerCu = 4;
constexpr int kLenetMaxLaunches = 16;
// Byte offsets of the workspace regions, each [n_agents][batch][...] with agent stride batch x
// the per-image size, 256-byte aligned: the pooled activations and their winner codes (one byte
// per pooled output: 0-3 = the window's first maximum in row-major order, 4 = none positive),
// the Linear layers' activations and gradients, the gradient entering the second pooling, and
// the convolution gradients' group partials [n_agents][groups][2872].
struct LenetWs {
    size_t pool1, code1, pool2, code2, h1, h2, z, dz3, dz2, dz1, da, part, total;
};
LenetWs lenet_workspace(int32_t n_agents, int32_t batch, int32_t num_classes);
// The convolution kernels' parameter.  The workspace pointers are the regions of LenetWs (agent
// stride batch x the per-image size).
struct LenetConvArgs {
    const float *X;          // parameter rows; the 2872 convolution parameters lead each
    int64_t ldx;
    const float *data;       // [batch][3][32][32] per agent
    int64_t s_data;
    float *pool1;            // [batch][1176]: written by the forward with train, read by the backward
    uint8_t *code1;          // [batch][1176] winner codes, likewise
    float *pool2;            // [batch][400]: fc1's input, always written
    uint8_t *code2;          // [batch][400]
    const float *da;         // [batch][400]: d loss / d pool2 (backward)
    float *part;             // [groups][2872] per agent: the backward's group partials
    float *G;                // the reduce's destination
    int64_t ldg;
    int32_t batch, train;
    int32_t passes, fwd_wpa, groups, bwd_wpa;
};
// The stand-alone cross-entropy head (launch_xent_grad's arguments).
struct XentArgs {
    const float *Z;
    int64_t sZ;
    const int32_t *y;
    int64_t sY;
    float *dZ;
    int64_t sD;
    float *loss;
    int32_t batch, rows, classes;
};
enum LenetStepKind : int32_t {
    kLenetConvFwd,      // launch_lenet_conv_fwd(conv, fwd_grid)
    kLenetGemm,         // launch_bgemm(gemm)
    kLenetHead,         // launch_xent_grad(head ...)
    kLenetConvBwd,      // launch_lenet_conv_bwd(conv, bwd_grid)
    kLenetConvReduce,   // launch_lenet_conv_reduce(conv, n_agents)
};
struct LenetStep {
    int32_t kind;
    BgemmArgs gemm;   // kLenetGemm
    XentArgs head;    // kLenetHead
};
struct LenetPlan {
    int32_t train;                // G given: the backward runs
    int32_t head;                 // 0: no loss (logits only), 1: fused into fc3's GEMM, 2: fc3 +
                                  // the stand-alone head (batch > 64)
    int32_t passes, fwd_wpa;      // forward: ceil(batch / kLenetFwdImages) passes per agent;
                                  // workgroup w of an agent walks passes w, w + fwd_wpa, ...
    int32_t groups, bwd_wpa;      // backward: ceil(batch / kLenetGroup) groups, walked likewise
    int32_t fwd_grid, bwd_grid;   // n_agents * wpa workgroups of kLenetThreads
    LenetWs ws;
    LenetConvArgs conv;           // the convolution steps' parameter
    int32_t n_agents;
    int32_t n_launches;           // the steps: what dl_lenet_grad launches, in order
    LenetStep step[kLenetMaxLaunches];
};
// Checks a dl_lenet_grad call and shapes it.  Either kernel runs wpa = ceil(kLenetWgPerCu *
// n_cus / n_agents) workgroups per agent, at least 1 and at most the agent's passes / groups.
int shape_lenet(const dl_lenet_args *a, int n_cus, void *ws, size_t ws_bytes, LenetPlan *out,
                char *err);

// dl_lenet_eval: blocks of kEvalBlockRows rows as dl_mlp_eval's, the LDS of one workgroup
// (lenet_eval.hip asserts it: two workgroups a compute unit), and the workspace: [n_agents]
// [blocks] float loss parts at `part`, then as many int32 correct counts at `hit`.
constexpr int kLenetEvalLdsBytes = 72128;
constexpr int kLenetEvalWgPerCu = 2;
struct LenetEvalWs {
    size_t part, hit, total;
};
LenetEvalWs lenet_eval_workspace(int32_t n_agents, int32_t rows);
// Checks a dl_lenet_eval call and shapes its grid: blocks = ceil(rows / 64); row_splits =
// ceil(kLenetEvalWgPerCu * n_cus / n_agents), at least 1 and at most `blocks`; the caller's hint
// (args.row_splits > 0) instead, clamped to [1, blocks].  check_ws: the workspace too
// (dl_lenet_eval; the plan query has none).
int shape_lenet_eval(const dl_lenet_eval_args *a, int n_cus, const void *ws, size_t ws_bytes,
                     bool check_ws, dl_lenet_eval_plan *out, char *err);

}  // namespace dl
