/* dlamd.h -- C ABI of the MI355X consensus-mixing engine (libdlamd.so).
 *
 * The reference (Malkovsky/distributed-learning) is pure Python; it has no native/FFI boundary.
 * Each entry point below replaces one reference Python routine on the gossip hot path and is
 * what a binding (ctypes here) calls in its place:
 *
 *   dl_mix_round        <- Mixer._mix_params_once        utils/consensus_simple/mixer.py:43-49
 *                          (+ the local step x -= lr*g that a training loop runs before mixing,
 *                           Titanic Consensus GD test.ipynb:903-907, and the deviation pass of
 *                           Mixer._get_deviation_dict mixer.py:57-66, fused)
 *   dl_deviation        <- Mixer._get_deviation_dict / _get_max_deviation   mixer.py:51-66
 *   dl_max_column_std   <- Mixer.get_max_parameters_std                     mixer.py:82-84
 *   dl_perron_round     <- ConsensusAgent.run_round mixing loop             consensus_asyncio.py:231-310
 *                          (synchronous Jacobi form: every agent at the same iteration)
 *   dl_async_load / dl_async_update / dl_async_read
 *                       <- ConsensusAgent.run_round's per-agent arithmetic under the reference's
 *                          own message schedule: pre-scale :231, step :295, verdict :297
 *   dl_step_rows        <- (multi-GPU) boundary rows x - lr*g packed for the halo exchange that
 *                          replaces the per-neighbour value messages of consensus_asyncio.py:236-284
 *   dl_column_sum       <- the np.mean numerator of mixer.py:61 (multi-GPU global mean)
 *   dl_mix_rounds       <- Mixer.mix(times=K) with eps=None: K rounds in one HBM pass  mixer.py:18-38
 *   dl_mix_rounds_trace <- Mixer.mix(times, eps) when X does not fit one workgroup: K rounds in
 *                          one HBM pass plus the K per-round max deviations  mixer.py:18-41, 51-66
 *   dl_mix_until        <- Mixer.mix(times, eps): loop, deviation and stop rule in one launch
 *                          mixer.py:18-41
 *   dl_consensus_gd     <- the Titanic notebook's consensus GD run (local logreg steps,
 *                          networks/logreg_model_titanic.py:16-20, + run_round per iteration)
 *   dl_sgd_step, dl_mlp_grad, dl_bgemm, dl_xent_grad <- the per-agent training steps of configs
 *                          c3/c5 (torch.optim.SGD, ANNModel autograd)
 *   dl_sgd_round        <- torch.optim.SGD.step of every agent and the Mixer._mix_params_once
 *                          that follows it (Man_Colab.ipynb cells 19-23), in one pass over HBM
 *   dl_cheb_round, dl_axpby <- (no reference counterpart) Mixer.mix's rounds accelerated by the
 *                          Chebyshev semi-iteration with gamma of fast_averaging.find_optimal_weights
 *   dl_track_round      <- (no reference counterpart) the local step and Mixer.mix's round of
 *                          the consensus notebooks with gradient tracking: exact at a constant lr
 *   dl_adam_step, dl_adam_tick, dl_adam_round <- (no reference counterpart) torch.optim.Adam /
 *                          AdamW as the agents' optimizer, alone or fused into the round
 *   dl_mlp_eval         <- MasterNode's per-node test statistics (accuracy and loss of every
 *                          node on the shared test_loader, Man_Colab.ipynb cells 21-23) through
 *                          ANNModel.forward (networks/ann_model.py:27-45), all agents at once
 *   dl_batch_gather     <- every node's next(train_loader) over its random_split shard
 *                          (Man_Colab.ipynb cells 16, 19-21), from a dataset resident in HBM
 *   dl_image_batch      <- transform_train / transform_test of Man_Colab.ipynb cell 16
 *                          (RandomCrop(32, padding=4), RandomHorizontalFlip, ToTensor, Normalize)
 *                          on every node's next uint8 mini-batch, draws supplied by the caller
 *   dl_lenet_grad       <- every node's LeNet forward, CrossEntropyLoss and backward
 *                          (Man_Colab.ipynb cell 19, model_name = 'lenet'), all agents per call
 *   dl_lenet_eval       <- MasterNode's per-node test statistics through LeNet, Man_Colab.ipynb
 *                          cells 21-23
 *
 * Conventions
 *   - Every pointer argument is a DEVICE pointer owned by the caller; nothing is allocated inside.
 *     Scratch comes from the caller's workspace (size from the *_workspace_bytes query).
 *   - Calls are stream-ordered and asynchronous (no host synchronisation) unless stated.
 *   - Matrices are row-major: row a = agent a, `ld*` = row stride in elements.
 *   - No exceptions cross the ABI. Return value: 0 on success, otherwise a dl_status code;
 *     dl_last_error() returns a thread-local message for the last failure on this thread.
 *   - Reentrant across streams; the only process-wide state is a per-device property cache.
 */
#ifndef DLAMD_H
#define DLAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLAMD_ABI_VERSION 10

typedef void *dl_stream_t; /* hipStream_t; NULL = the legacy default stream */

enum dl_status {
    DL_OK = 0,
    DL_ERR_INVALID = 1,   /* bad argument (shape, null pointer, alias, range) */
    DL_ERR_WORKSPACE = 2, /* workspace too small or misaligned */
    DL_ERR_HIP = 3,       /* a HIP runtime call failed; message has the hipError string */
    DL_ERR_UNSUPPORTED = 4
};

/* Mixing matrix W in CSR form (device pointers).  Row a lists its (source row, weight) pairs in
 * the reference's dict insertion order (mixer.py:47) -- that order is the fp32 summation order,
 * and the result is bit-identical to the reference's left fold when it is kept.  Source rows
 * index [0, n_rows) = local agents, [n_rows, n_rows + n_halo) = halo rows (with
 * dl_mix_args.n_local_src = L: [0, L) local, [L, L + n_halo) halo). */
typedef struct dl_csr {
    const int32_t *row_ptr; /* [n_rows + 1] */
    const int32_t *col;     /* [nnz] */
    const float *w;         /* [nnz] fp32 (the reference casts the Python float to fp32) */
    int32_t n_rows;
    int32_t nnz;
    int32_t uniform_row_nnz; /* > 0 promises row_ptr[a] == a * uniform_row_nnz for every row
                                (regular graphs); lets the LDS kernel skip staging row_ptr.
                                0 = general CSR.  Checked: nnz == n_rows * uniform_row_nnz. */
    int32_t doubly_stochastic; /* 1 promises every column of W sums to 1 (as rows do for the
                                  reference's mixing matrices), so mean(W t) = mean(t): the fused
                                  deviation then takes the column mean from the staged inputs and
                                  needs one LDS pass instead of two.  0 = general W. */
    int32_t shared_row_weights; /* 1 promises (with uniform_row_nnz > 0) that every row's weight
                                   sequence equals row 0's, w[a*d + k] == w[k] bit for bit (a
                                   uniform edge weight: best-constant or analytic FA weights on a
                                   regular graph).  The LDS kernel then stages d weights instead
                                   of nnz, which fits ~2x more agents per tile.  w is still the
                                   full [nnz] array.  0 = per-entry weights. */
    int32_t min_row_nnz; /* (ABI 6) > 0 promises every row has at least this many entries (any
                            graph with a self weight per row: >= 1; Barabasi-Albert m = 2 with
                            self weights: 3).  When the CSR does not fit LDS beside a tile of all
                            agents (thousands of agents, per-edge weights), the tile kernel then
                            keeps each row's first min(min_row_nnz, 5) entries in registers and
                            only the remaining nnz - head * n_rows entries in LDS (plan path 5)
                            instead of taking the gather path.  Checked: min_row_nnz * n_rows <=
                            nnz; a wrong promise gives wrong (never out-of-bounds) results.
                            0 = unknown. */
} dl_csr;

typedef struct dl_mix_args {
    const float *x;     /* [n_rows, ldx] parameters before the round */
    int64_t ldx;
    float *y;           /* [n_rows, ldy] parameters after the round; must not overlap x */
    int64_t ldy;
    int64_t n_params;   /* columns per agent */
    dl_csr W;
    const float *g;     /* nullable [n_rows, ldg]: fused local step x <- x - lr*g first */
    int64_t ldg;
    float lr;
    const float *halo;  /* nullable [n_halo, ldh]: remote rows, already stepped */
    int64_t ldh;
    int32_t n_halo;
    float *dev_sq;      /* nullable [n_rows]: ||y_a - mean_b(y_b)||^2  (n_halo > 0: see mean_prev) */
    float *dev_max;     /* nullable [1]: max_a sqrt(dev_sq[a])          (n_halo > 0: see mean_prev) */
    float *mean;        /* nullable [n_params]: mean_b(y_b)              (needs n_halo == 0) */
    int32_t tile_cols;  /* 0: x, g, y row-major with ld*.  T > 0: x, g, y in the column-tiled
                           layout [ceil(n_params/T)][rows][T] (each tile one contiguous block,
                           last tile zero-padded); T must be the plan's tile_cols
                           (dl_mix_plan_query on the row-major args).  (ABI 8) In this layout
                           ldx / ldg / ldy are the ROWS of each operand's tiled blocks (tile
                           stride ld*T floats), 0 = the default (n_local_src for x and g, n_rows
                           for y): a partition row set passes x / g / y offset by whole rows into
                           wider blocks.  ldh is ignored; the halo is n_halo_blocks tiled blocks
                           (below). */
    /* Agent-partitioned rounds (n_halo > 0) with the deviation pipelined one round behind: the
     * global column mean of y needs every rank's rows, so this round's kernel publishes its
     * share of it and measures the PREVIOUS round's iterate -- its input x, staged anyway --
     * against the previous mean.  No HBM pass beyond the round's own. */
    const float *mean_prev; /* nullable [n_params] (n_halo > 0 or n_local_src > n_rows only; with
                               colsum_out and dev_sq):
                               the global column mean of x (the previous round's all-reduced
                               colsum_out / N): dev_sq[a] = ||x_a - mean_prev||^2, dev_max =
                               max sqrt (nullable).  With dev_sq NULL the round leaves its
                               partial sums in the workspace instead -- rows [0, R) of
                               n_local_src floats, column-tiled layout only, R written to
                               *partial_rows_out (ABI 9: required in this mode) -- for the caller
                               to reduce (one dl_row_sums over several column chunks' partial
                               rows placed back to back); a dev_max is then only set to 0, for
                               that dl_row_sums (max_zeroed = 1). */
    float *colsum_out;      /* nullable [n_params] (as mean_prev): sum over the local source rows of
                               the stepped inputs t = x - lr*g, in a fixed order.  Summed over all
                               ranks it is the column sum of the round's output when the global W
                               is doubly stochastic (the numerator of the next mean_prev). */
    /* Row sets of an agent partition (sharding.py, interior/boundary split): 0 = n_rows.
     * Otherwise source rows [0, n_local_src) come from x (and g, stepped), [n_local_src,
     * n_local_src + n_halo) from halo, and the n_rows OUTPUT rows follow the CSR -- they need
     * not be the first source rows: an interior launch mixes rows [0, n_I) of a rank's window
     * from all its local rows while the halo is in flight; a boundary launch passes x (and g)
     * offset to the first local row the boundary rows read, and y offset to the first boundary
     * row.  Needs n_rows <= n_local_src + n_halo, the LDS tile kernel, no fused exact deviation
     * (dev_sq / dev_max / mean only as the lagged deviation, which is then per SOURCE row:
     * dev_sq[n_local_src]; workspace dl_mix_workspace_bytes(max(n_rows, n_local_src), ...)). */
    int32_t n_local_src;
    /* (ABI 8) Halo rows in the column-tiled layout (tile_cols > 0, n_halo > 0): `halo` holds
     * n_halo_blocks blocks back to back (0 = one block of n_halo rows), block b of
     * halo_block_rows[b] rows laid out [ceil(n_params/T)][halo_block_rows[b]][T] -- one block per
     * peer, so that each peer's halo is ONE contiguous receive buffer of the exchange.  Halo row
     * h of the CSR (source row n_local_src + h) is row h - (rows of blocks before b) of block b.
     * halo_block_rows is a HOST array of n_halo_blocks <= 16 positive counts summing to n_halo.
     * The whole halo must span < 4 GiB.  Row-major layout: n_halo_blocks must be 0. */
    int32_t n_halo_blocks;
    const int32_t *halo_block_rows;
    /* (ABI 8) Plan path 5 only (ignored elsewhere), a performance hint: the first n_hub_rows rows
     * (<= 256; the longest ones first, as in a descending row-length order) are each folded by
     * four lanes, one column each, instead of by one lane.  A Barabasi-Albert hub's CSR row is
     * a serial fp32 fold (the reference's order); split by column it is four shorter scalar
     * chains.  Any value gives the same y bits (each column keeps its left fold), and with a
     * doubly stochastic W the same dev_sq / dev_max / mean bits (the hub lanes add a tile's
     * squared deviations in the owner's order).  With a general W (two-pass deviation) the
     * column mean gathers the hub rows in another lane order, so dev_sq and mean may differ in
     * the last bits across n_hub_rows values.  The kernel uses fewer rows when their register
     * heads do not fit LDS. */
    int32_t n_hub_rows;
    /* (ABI 9) nullable HOST pointer; REQUIRED in the partial-rows mode (a halo round with mean_prev
     * and colsum_out but no dev_sq, see mean_prev), which is refused without it, so a caller that
     * forgets dev_sq gets an error instead of a round with no deviation.  dl_mix_round writes the
     * number of deviation partial rows the launch left in the workspace (0 when it wrote none)
     * before it returns -- on the host, no synchronisation: a caller placing several column
     * chunks' rows back to back starts the next chunk's slice there. */
    int32_t *partial_rows_out;
} dl_mix_args;

/* Which kernel configuration dl_mix_round picks (introspection for tests and the bench). */
typedef struct dl_mix_plan {
    int32_t path;       /* 1 = LDS tile kernel (all agents x T columns per tile), 2 = gather kernel,
                           3 = multi-round LDS kernel (dl_mix_rounds), 4 = tile kernel with the
                           CSR in registers (regular graphs of 5 entries per row whose CSR does
                           not fit LDS beside the tile), 5 = tile kernel with each row's first
                           entries in registers and the rest in LDS (irregular graphs with
                           W.min_row_nnz >= 2 whose CSR does not fit LDS beside the tile) */
    int32_t tile_cols;  /* T: columns per tile (path 1) */
    int32_t grid;       /* workgroups launched */
    int32_t lds_bytes;  /* dynamic LDS per workgroup */
    int32_t n_tiles;    /* tiles one launch walks.  (ABI 9) A column-tiled halo round of few
                           source rows walks groups of 2, 4 or 8 consecutive data tiles as one
                           kernel tile, so n_tiles = n_params / (tile_cols x group) and
                           n_tiles x tile_cols < n_params there; tile_cols stays the data
                           layout's width */
    int32_t regular;    /* 1 if every row has the same entry count (CSR row_ptr not staged) */
    int32_t head;       /* (ABI 8) path 5: CSR entries per row kept in registers (2, 3 or 5);
                           path 4: 5; else 0 */
    int32_t tail_fmt;   /* (ABI 8) path 5: LDS tail entries of 8 B {weight, row} (2) or 6 B (1) */
} dl_mix_plan;

int dl_abi_version(void);
const char *dl_last_error(void);

size_t dl_mix_workspace_bytes(int32_t n_rows, int32_t n_halo, int64_t n_params);
/* Plan from shapes only (no pointers): what dl_mix_round would pick for these sizes, with
 * (deviation) / without the fused deviation.  tile_cols: 0 = row-major operands; > 0 = operands
 * in the column-tiled layout of that width; -1 = choose the width for a column-tiled layout
 * (plan->tile_cols; 0 with the row-major plan if no tile of all rows fits LDS). */
int dl_mix_plan_shape(int32_t n_rows, int32_t n_halo, int64_t n_params, int32_t nnz,
                      int32_t uniform_row_nnz, int32_t shared_row_weights, int32_t deviation,
                      int32_t tile_cols, dl_mix_plan *plan);
/* (ABI 6) The same from a CSR descriptor (only its sizes and flags are read, pointers may be
 * NULL): min_row_nnz included, which dl_mix_plan_shape cannot express (it assumes
 * uniform_row_nnz). */
int dl_mix_plan_csr(const dl_csr *W, int32_t n_halo, int64_t n_params, int32_t deviation,
                    int32_t tile_cols, dl_mix_plan *plan);
int dl_mix_plan_query(const dl_mix_args *args, dl_mix_plan *plan);
int dl_mix_round(const dl_mix_args *args, void *workspace, size_t ws_bytes, dl_stream_t stream);

/* `rounds` consecutive mixing rounds in ONE pass over HBM:  y = W^rounds (x - lr g).
 * Replaces `Mixer.mix(times=rounds)` with eps=None (mixer.py:18-38: `times` calls of
 * _mix_params_once, :43-49, nothing in between) and pure gossip averaging (BASELINE c2).  The
 * mix is column-independent, so each workgroup runs every round on an LDS-resident tile of all
 * agents before writing it back: HBM traffic is that of one round, whatever `rounds` is.  Bit-
 * identical to `rounds` calls of dl_mix_round (same fold order each round).  g (nullable): the
 * local step is applied once, before the first round.  dev_sq / dev_max / mean describe the
 * final iterate and need a doubly stochastic W.  Needs two tile images of all agents in LDS, no
 * halo rows, 16-byte aligned operands and (row-major) n_params a multiple of the tile width;
 * otherwise returns DL_ERR_UNSUPPORTED and the caller loops dl_mix_round.  Workspace:
 * dl_mix_workspace_bytes (deviation only).  dl_mix_rounds_plan reports the configuration
 * (path 3) or DL_ERR_UNSUPPORTED. */
int dl_mix_rounds_plan(const dl_mix_args *args, dl_mix_plan *plan);
/* The same from sizes alone (no operands): the configuration dl_mix_rounds would use for
 * row-major (tile_cols 0) or column-tiled operands of n_rows x n_params, or
 * DL_ERR_UNSUPPORTED.  Lets a caller decide on an LDS slot order before X exists. */
int dl_mix_rounds_plan_shape(int32_t n_rows, int64_t n_params, int32_t nnz,
                             int32_t uniform_row_nnz, int32_t shared_row_weights,
                             int32_t doubly_stochastic, int32_t deviation, int32_t tile_cols,
                             dl_mix_plan *plan);
int dl_mix_rounds(const dl_mix_args *args, int32_t rounds, void *workspace, size_t ws_bytes,
                  dl_stream_t stream);

/* `rounds` mixing rounds in one HBM pass, y = W^rounds x, with the per-round disagreement
 * trace[r] = max_a ||x_a^(r+1) - mean(x^(r+1))||_2 (device float[rounds]) for r < rounds -- what
 * Mixer.mix(times, eps) (mixer.py:18-41) evaluates after every round (_get_max_deviation,
 * :51-55, 57-66).  The caller finds the first round whose value is below eps (and >= times); if
 * it lies inside the pass it re-runs that many rounds from x with dl_mix_rounds / dl_mix_round
 * (x is not modified).  Rounds are the dl_mix_round fold (bit-identical).
 *   W: any CSR.  A doubly stochastic W (W.doubly_stochastic = 1) takes the column mean of x
 *     once (mean(W x) = mean(x)); any other W -- row-stochastic or general -- gets every round's
 *     column mean reduced from that round's own outputs before its deviations (the one-image
 *     kernel, "GM").  Irregular graphs above 2048 agents also take the one-image kernel.
 *   Sizes: 2 <= n_rows <= 4096; no halo rows (n_halo == 0, n_local_src 0 or n_rows); g must be
 *     NULL; n_params % 4 == 0; 16-byte aligned operands, row-major or column-tiled (tile_cols, a
 *     multiple of 4 on the one-image kernel).  Rounds per pass (dl_mix_trace_plan): two-image
 *     kernels 32, or 24 above 512 agents of a register-cached regular graph (degree 4, shared
 *     weights), 16 / 8 above 1024 / 2048 agents; the one-image kernel 24 / 12 / 4 at <= 1024 /
 *     <= 2048 / <= 4096 agents.
 *   LDS: two column images of all agents beside the CSR, or else one image [n_rows] float4 plus
 *     the CSR past each row's register head (min(min_row_nnz, 5) entries) as 8-byte pairs; when
 *     that does not fit, a narrow image [n_rows] float2 with 6-byte tail entries.  Limits: at
 *     most 65535 CSR entries past the register heads, and image + tail + 256 B <= 160 KiB.
 *     Otherwise DL_ERR_UNSUPPORTED (the caller loops dl_mix_round).
 * Workspace: dl_mix_trace_workspace_bytes(n_rows, rounds). */
int dl_mix_trace_plan(const dl_mix_args *args, int32_t *max_rounds);
size_t dl_mix_trace_workspace_bytes(int32_t n_rows, int32_t rounds);
int dl_mix_rounds_trace(const dl_mix_args *args, int32_t rounds, float *trace, void *workspace,
                        size_t ws_bytes, dl_stream_t stream);

/* Mixer.mix(times, eps) (utils/consensus_simple/mixer.py:18-41) as ONE launch: the loop
 *     stop = (!use_eps || max_a ||x_a - mean|| < eps) && done >= times
 *     while (!stop && done < max_rounds) { x <- W x; ++done; }
 * runs on one workgroup with x resident in LDS (two images of n_rows x ceil(n_params/4)*4 fp32
 * plus the CSR: dl_mix_until_fits).  Rounds are the dl_mix_round fold (bit-identical); the
 * deviation is evaluated before the first round and after each one, as the reference does; the
 * test is float32 against float32(eps) (numpy >= 2 semantics of np.float32 < float).
 * status (device int32[2]) receives {rounds done, 1 if the stop rule held / 0 if max_rounds cut
 * the loop / 2 if the max deviation of the last evaluation is NaN}; a caller continues a cut loop
 * with times' = times - done on y.  A NaN max deviation (any NaN parameter, or inf - inf against
 * the column mean; the maximum keeps a NaN as numpy's does) can never pass `< eps`: the loop
 * ends at that evaluation, y is the iterate it was taken on, and re-entering would only repeat
 * it.  An infinite deviation is a number: just not below eps.  dev_trace (nullable,
 * device float[max_rounds + 1], use_eps only) receives the max deviation of every evaluation in
 * order (index 0 = before the first round) for the reference's per-round debug log.  y may be x
 * itself (same ld); otherwise it must not overlap x.  W must be square (col < n_rows). */
typedef struct dl_mix_until_args {
    const float *x;     /* [n_rows, ldx] */
    int64_t ldx;
    float *y;           /* [n_rows, ldy]: x after the last round */
    int64_t ldy;
    int64_t n_params;
    dl_csr W;
    int32_t times;      /* minimum rounds (mixer.py:18 `times`, >= 0) */
    int32_t use_eps;    /* 0 = eps None: exactly `times` rounds */
    float eps;          /* float32(eps) */
    int32_t max_rounds; /* >= 1: rounds this launch may run */
    int32_t *status;    /* device int32[2] */
    float *dev_trace;   /* nullable device float[max_rounds + 1] */
} dl_mix_until_args;

/* BASELINE config c1 as one launch: `iterations` rounds of the Titanic notebook's consensus GD
 * (cells 12-14) for every agent, fp64 -- per agent a local step on its shard of the L2-regularised
 * logistic loss (networks/logreg_model_titanic.py:16-20)
 *     w <- w - steps[it] * ( -(sum_i y_i sigmoid(-y_i x_i.w) x_i) / n_a + tau w )
 * then one asyncio consensus round (consensus_asyncio.py:209-312) weighted by the shard sizes n_a:
 * the dl_perron_round Jacobi (pre-scale w n_a / mean_weight, y <- y (1 - eps deg) + eps sum_nbr y,
 * until every agent's one-sided test against its neighbours' previous values holds, at most
 * max_iter iterations).  Agent a owns rows [shard_ptr[a], shard_ptr[a+1]) of X [rows][n_features]
 * and y; row_ptr/col list each agent's neighbours in its socket order (no self loops).  w (device,
 * [n_agents][n_features]) holds the start weights and receives the final ones; iters_out
 * (nullable, device int32[iterations]) the Jacobi iterations of each round.  One workgroup:
 * n_features <= 16, and the agents' values, shards (if they fit LDS, else read from L2) and the
 * step sizes (host-computed, e.g. alpha (it+1)^-0.5) are device memory. */
typedef struct dl_consensus_gd_args {
    const double *X;
    const double *y;
    const int32_t *shard_ptr;   /* [n_agents + 1], shard_ptr[0] == 0 */
    int32_t n_agents;
    int32_t n_features;
    const int32_t *row_ptr;     /* [n_agents + 1] neighbour lists */
    const int32_t *col;
    double eps;                 /* 0.95 / max degree (consensus_asyncio.py:78-86) */
    double conv_eps;
    double mean_weight;         /* mean shard size */
    double tau;
    const double *steps;        /* [iterations] */
    int32_t iterations;
    int32_t max_iter;
    double *w;
    int32_t *iters_out;
} dl_consensus_gd_args;
int dl_consensus_gd(const dl_consensus_gd_args *args, int32_t total_rows, dl_stream_t stream);

/* 1 when dl_mix_until takes these sizes in one workgroup's LDS, else 0. */
int dl_mix_until_fits(int32_t n_rows, int64_t n_params, int32_t nnz);
int dl_mix_until(const dl_mix_until_args *args, dl_stream_t stream);

/* Deviation of x from its column mean: dev_sq[a] = ||x_a - mean||^2, dev_max = max sqrt(dev_sq).
 * mean_in nullable: when given (e.g. a global mean all-reduced across GPUs) it is used instead
 * of the local column mean.  mean_out nullable.  Returns zeros when n_rows <= 1 (mixer.py:58-59). */
size_t dl_deviation_workspace_bytes(int32_t n_rows, int64_t n_params);
int dl_deviation(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params,
                 const float *mean_in, float *dev_sq, float *dev_max, float *mean_out,
                 void *workspace, size_t ws_bytes, dl_stream_t stream);

/* Deviation of x held in the column-tiled layout (see dl_mix_args.tile_cols). */
int dl_deviation_tiled(const float *x, int32_t n_rows, int64_t n_params, int32_t tile_cols,
                       float *dev_sq, float *dev_max, float *mean_out, void *workspace,
                       size_t ws_bytes, dl_stream_t stream);

/* Layout conversion between row-major [n_rows][ld] and column-tiled [ceil(P/T)][n_rows][T]
 * (the resident layout of the engine: one HBM-contiguous block per LDS tile). */
int dl_to_tiled(const float *src, int64_t ld, int32_t n_rows, int64_t n_params, int32_t tile_cols,
                float *dst, dl_stream_t stream);
int dl_from_tiled(const float *src, int32_t n_rows, int64_t n_params, int32_t tile_cols, float *dst,
                  int64_t ld, dl_stream_t stream);

/* colsum[p] = sum_a x[a, p], rows added in order (numerator of np.mean, mixer.py:61). */
int dl_column_sum(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params, float *colsum,
                  dl_stream_t stream);

/* (ABI 9) sums[a] = sum_b parts[b][a] over n_parts rows of n_rows floats (fixed order, fp64), max_sqrt[0]
 * = max_a sqrt(sums[a]); either output nullable.  The per-agent ||x_a - mean||^2 of a round run
 * as several column chunks (their partial rows back to back in parts, see mean_prev), and their
 * max -- the _get_max_deviation of mixer.py:51-55 over the whole round -- in one launch.
 * max_zeroed = 1: max_sqrt already holds 0 (a dl_mix_round given it as dev_max without dev_sq
 * zeroes it), so no memset is queued before the reduce. */
int dl_row_sums(const float *parts, int32_t n_parts, int32_t n_rows, float *sums, float *max_sqrt,
                int32_t max_zeroed, dl_stream_t stream);

/* out[0] = max_p std_a(x[a, p]) (population std, the intent of mixer.py:82-84). */
int dl_max_column_std(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params, float *out,
                      dl_stream_t stream);

/* Host-only (no device work): agent -> LDS image row-slot order for the multi-round kernels'
 * neighbour gathers.  col: [n_rows][degree] neighbour agent ids in CSR entry order (the
 * reference's topology dict order, mixer.py:43-49); chunks: float4 chunks per image row and lane
 * (4 = dl_mix_rounds' agent-major rows at 16 columns, 1 = dl_mix_rounds_trace's chunk-major
 * planes).  A greedy random-swap search over `moves` moves (seeded) that lowers the number of
 * ds_read_b128 16-lane groups' repeated 16-byte bank slots; order[slot] = agent (out, n_rows);
 * conflicts[0] / [1] = extra LDS cycles per round before / after.  Relabelling keeps every row's
 * entry order, so the iterates are bit-identical per agent.  Same objective and move rule as
 * graph.lds_slot_order (Python), with incremental counts.  Not in the reference: it has no
 * device layout to order. */
int dl_lds_slot_order(int32_t n_rows, int32_t degree, const int32_t *col, int32_t chunks,
                      int64_t moves, uint64_t seed, int32_t *order, int64_t *conflicts);

/* out[i, :] = x[rows[i], :] - lr * g[rows[i], :]  (g nullable: plain copy).  Packs the boundary
 * rows a GPU sends to its neighbours in the multi-GPU halo exchange. */
int dl_step_rows(const float *x, int64_t ldx, const float *g, int64_t ldg, float lr,
                 const int32_t *rows, int32_t n_sel, int64_t n_params, float *out, int64_t ldo,
                 dl_stream_t stream);

/* (ABI 8) The same in the column-tiled layout: x [ceil(n_params/T)][x_rows][T] and g (nullable)
 * [..][g_rows][T] -> out [ceil(n_params/T)][n_sel][T] (one peer's halo block of dl_mix_args,
 * padded columns included).  Packs a rank's boundary rows for one peer of the exchange; a column
 * chunk of whole tiles is x / g / out offset to its first tile.  16-byte aligned pointers. */
int dl_step_rows_tiled(const float *x, int32_t x_rows, const float *g, int32_t g_rows, float lr,
                       const int32_t *rows, int32_t n_sel, int64_t n_params, int32_t tile_cols,
                       float *out, dl_stream_t stream);
/* (ABI 8) The same for every peer of an exchange in ONE launch: peer b's rows are
 * rows[row0[b] .. row0[b+1]) and its block [ceil(n_params/T)][row0[b+1] - row0[b]][T] goes to
 * outs[b].  row0 (n_peers + 1 entries, row0[0] = 0) and outs (n_peers device pointers) are HOST
 * arrays; n_peers <= 16.  Both tiled packs store non-temporally (the blocks are read once, by the
 * peers' receives). */
int dl_step_rows_tiled_peers(const float *x, int32_t x_rows, const float *g, int32_t g_rows,
                             float lr, const int32_t *rows, int32_t n_peers, const int32_t *row0,
                             float *const *outs, int64_t n_params, int32_t tile_cols,
                             dl_stream_t stream);

/* Local optimizer step of config c5 (Man_Colab.ipynb cell 19: optimizer = optim.SGD,
 * {'momentum': 0.9, 'weight_decay': 5e-4}, lr 0.02), i.e. torch.optim.SGD.step (torch/optim/sgd.py,
 * single-tensor form) applied to every agent row at once, with torch's rounding (one fma per
 * add-with-alpha):
 *   d = g + wd*x;  buf = first ? d : mu*buf + (1-dampening)*d;  d = nesterov ? d + mu*buf : buf;
 *   out = x - lr*d
 * out may be x itself (in place, as optimizer.step) or a separate buffer, e.g. the input of the
 * following dl_mix_round (the parameters stay put and the round writes them back).  buf
 * (momentum buffer) is read unless `first` and always written when momentum != 0. */
typedef struct dl_sgd_args {
    const float *x; int64_t ldx;    /* [n_rows, ldx] parameters */
    const float *g; int64_t ldg;    /* [n_rows, ldg] gradients */
    float *buf; int64_t ldb;        /* [n_rows, ldb] momentum buffers (nullable if momentum == 0) */
    float *out; int64_t ldo;        /* [n_rows, ldo] stepped parameters (== x or disjoint) */
    int32_t n_rows;
    int64_t n_params;
    float lr, momentum, dampening, weight_decay;
    int32_t nesterov;
    int32_t first;                  /* 1: buf = d (torch's first step: clone of the gradient) */
} dl_sgd_args;
int dl_sgd_step(const dl_sgd_args *args, dl_stream_t stream);

/* The optimizer step above fused into the consensus round that follows it (config c5: every agent
 * steps with momentum SGD, then Mixer.mix):  y = W sgd(x, g, buf), buf updated in the same pass.
 * Bit for bit dl_sgd_step(out = S) followed by dl_mix_round(x = S, g = NULL), for every parameter
 * setting -- with momentum 0 and weight decay 0 the step is fma(-lr, g, x), dl_sgd_step's
 * rounding, not dl_mix_round's own fl(x - fl(lr g)) -- but one launch that moves 20 B per element
 * (read x, g, buf; write buf, y) instead of two that move 28 B, and no scratch matrix S.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   y may be x itself with ldy == ldx (the round in place: a workgroup stages all rows of its
 *     columns before it writes them); otherwise y must not overlap x.  buf must not overlap x, y
 *     or g.  Row-major: any n_params >= 1, columns [n_params, ld) of y and buf are never written.
 *     Column-tiled (mix.tile_cols > 0): buf in the same layout as x, ldb its block rows (0 =
 *     n_rows), 16-byte aligned operands.
 *   dev_sq / dev_max / mean describe y as dl_mix_round's do; workspace dl_mix_workspace_bytes.
 *   LDS tile kernel only: rounds that plan path 2, 4 or 5 return DL_ERR_UNSUPPORTED (the caller
 *     runs dl_sgd_step + dl_mix_round), as does any halo, partition or lagged-deviation field.
 *   Stream-ordered, no host synchronisation, no allocation: capturable in a hipGraph.
 * dl_sgd_round_plan: DL_OK and the configuration the round would run, or the refusal, without
 * touching the device. */
typedef struct dl_sgd_round_args {
    dl_mix_args mix;   /* x, y, W, g (required), lr, n_params, ld*, tile_cols, dev_sq, dev_max, mean;
                          halo, n_halo, mean_prev, colsum_out, n_local_src, n_halo_blocks,
                          partial_rows_out must be NULL / 0 */
    float *buf; int64_t ldb;   /* momentum buffers laid out as x (nullable if momentum == 0) */
    float momentum, dampening, weight_decay;
    int32_t nesterov, first;   /* as dl_sgd_args */
} dl_sgd_round_args;
int dl_sgd_round_plan(const dl_sgd_round_args *args, dl_mix_plan *plan);
int dl_sgd_round(const dl_sgd_round_args *args, void *workspace, size_t ws_bytes,
                 dl_stream_t stream);

/* One round of Chebyshev-accelerated gossip in one HBM pass:  y = a W x + b z, the semi-iteration
 *   x_1 = W x_0;  x_{k+1} = w_{k+1} W x_k + (1 - w_{k+1}) x_{k-1}
 *   w_1 = 1, w_2 = 2 / (2 - gamma^2), w_{k+1} = 4 / (4 - gamma^2 w_k)
 * with x = x_k, z = x_{k-1}, a = w_{k+1}, b = 1 - w_{k+1}.  For a symmetric W whose spectral radius
 * off the mean is gamma it contracts by gamma / (1 + sqrt(1 - gamma^2)) a round instead of gamma,
 * and keeps the mean (a + b = 1).  Rounding, per agent row r and column:
 *   acc = sum_e w_e x[col_e]          left fold from +0.0 in CSR order, product and sum separate
 *                                     fp32 operations: dl_mix_round's bits with g = NULL
 *   y   = fl(fl(a acc) + fl(b z[r]))  three separately rounded fp32 operations
 * i.e. bit for bit dl_mix_round(y = S) followed by dl_axpby(S, z, a, b, out = y), but one launch
 * that moves 12 B per element (read x, z; write y) instead of two that move 20 B, and no matrix S.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   y may be z itself with ldy == ldz (the intended mode: the thread that reads an element of z
 *     writes that element of y, so a ping-pong pair holds x_k and x_{k-1} and the round overwrites
 *     the older one), or x itself with ldy == ldx (a workgroup stages all rows of its columns
 *     before it writes them), or overlap neither.  x and z are only read.
 *   z is laid out as x: row-major [n_rows, ldz >= n_params]; column-tiled (mix.tile_cols > 0) ldz
 *     its block rows (0 = n_rows), 16-byte aligned operands.  Row-major: any n_params >= 1,
 *     columns [n_params, ld) of y are never written.
 *   dev_sq / dev_max / mean describe y as dl_mix_round's do, for any W and any z; workspace
 *     dl_mix_workspace_bytes.  A doubly stochastic W takes mean(y) as mean(a x + b z) of the
 *     staged inputs.  Where a x[r] overflows fp32 (|x| above FLT_MAX / |a|: a diverged run) that
 *     mean can be inf or NaN though y is finite; a tile with such a mean is measured in two
 *     passes instead, its mean summed from y as for any other W.  Tiles of finite means are
 *     not affected.
 *   DL_ERR_INVALID: args NULL; x, y or z NULL ("null x/y/z"); mix.g != NULL ("g must be NULL");
 *     every argument dl_mix_round itself refuses (W's arrays, strides, tile_cols, alignment of
 *     tiled operands; the texts say dl_mix_round); ldz out of range ("z laid out as x"); y
 *     overlapping x or z in any way other than being it ("y overlaps x", "y overlaps z");
 *     dl_cheb_round_plan with plan NULL.
 *   DL_ERR_UNSUPPORTED: any halo, partition or lagged-deviation field (halo, n_halo, mean_prev,
 *     colsum_out, n_local_src, n_halo_blocks, partial_rows_out); rounds that plan path 2, 4 or 5
 *     (LDS tile kernel only: the caller runs dl_mix_round + dl_axpby).
 *   DL_ERR_WORKSPACE: as dl_mix_round (deviation outputs without a 16-byte aligned workspace of
 *     dl_mix_workspace_bytes).
 *   Stream-ordered, no host synchronisation, no allocation: capturable in a hipGraph.
 * dl_cheb_round_plan: DL_OK and the configuration the round would run, or the refusal, without
 * touching the device. */
typedef struct dl_cheb_round_args {
    dl_mix_args mix;   /* x, y, W, n_params, ld*, tile_cols, dev_sq, dev_max, mean; g must be NULL;
                          halo, n_halo, mean_prev, colsum_out, n_local_src, n_halo_blocks,
                          partial_rows_out must be NULL / 0 */
    const float *z; int64_t ldz;   /* laid out as x (column-tiled: ldz = its block rows, 0 = n_rows) */
    float a, b;
} dl_cheb_round_args;
int dl_cheb_round_plan(const dl_cheb_round_args *args, dl_mix_plan *plan);
int dl_cheb_round(const dl_cheb_round_args *args, void *workspace, size_t ws_bytes,
                  dl_stream_t stream);
/* One gradient-tracking round in one HBM pass (no reference counterpart: the reference's loops run
 * decentralized gradient descent, X <- W (X - lr G), which with a constant step stalls at a bias
 * proportional to lr x the heterogeneity of the agents' gradients).  Each agent carries a tracker
 * d of the network-average gradient and steps along it (adapt-then-combine):
 *   t  = fl(fl(d + g) - g_old)         element-wise; g this step's gradient, g_old the last one's
 *   d' = sum_e w_e t[col_e]            dl_mix_round's fold: left fold from +0.0 in CSR order,
 *                                      product and sum separate fp32 operations
 *   s  = fl(x - fl(lr d'))             dl_mix_round's fused step with g = d'
 *   x' = sum_e w_e s[col_e]            the same fold
 * i.e. bit for bit  T = (D + G) - G_old element-wise, dl_mix_round(x = T, y = D'), dl_mix_round(x =
 * X, g = D', lr, y = X'),  but one launch that moves 24 B per element (read x, d, g, g_old; write
 * d', x') instead of at least 36 B and a scratch matrix.  Start from d = 0 and g_old = 0: the
 * first round then gives d' = W g.  The caller keeps two gradient buffers and swaps them every
 * step; the round writes neither.  For a doubly stochastic W, mean_a d' = mean_a g at every step
 * up to rounding, and with a constant lr the iterates reach the optimum of sum_a f_a.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   mix.x / mix.y are x / x', mix.g is g (required), mix.lr is lr.  y may be x itself with ldy ==
 *     ldx, and d_out may be d itself with lddo == ldd (a workgroup stages all rows of its columns
 *     before it writes them); otherwise no output overlaps any operand.  g and g_old are only
 *     read.
 *   d, d_out and g_old are laid out as x: row-major [n_rows, ld >= n_params]; column-tiled
 *     (mix.tile_cols > 0) ld their block rows (0 = n_rows), 16-byte aligned operands.  Row-major:
 *     any n_params >= 1, columns [n_params, ld) of y and d_out are never written.
 *   dev_sq / dev_max / mean describe x' exactly as dl_mix_round's do; workspace
 *     dl_mix_workspace_bytes.  A doubly stochastic W takes mean(x') as the mean of the staged s;
 *     a tile whose mean is then not finite is measured in two passes, as for any other W.
 *   DL_ERR_INVALID: args NULL; x, y, d, d_out, g or g_old NULL ("null x/y/d/d_out/g/g_old");
 *     every argument dl_mix_round itself refuses (W's arrays, strides, tile_cols, alignment of
 *     tiled operands, y overlapping x other than being it, y overlapping g; the texts say
 *     dl_mix_round); ldd, lddo or ldq out of range ("d, d_out and g_old laid out as x"); d_out
 *     overlapping d other than being it ("d_out overlaps d"); d_out overlapping x, y, g or g_old
 *     ("d_out overlaps x" ...); y overlapping d or g_old ("y overlaps d", "y overlaps g_old");
 *     dl_track_round_plan with plan NULL.
 *   DL_ERR_UNSUPPORTED: any halo, partition or lagged-deviation field (halo, n_halo, mean_prev,
 *     colsum_out, n_local_src, n_halo_blocks, partial_rows_out); rounds that plan path 2, 4 or 5
 *     (LDS tile kernel only: the caller runs the three steps above).
 *   DL_ERR_WORKSPACE: as dl_mix_round (deviation outputs without a 16-byte aligned workspace of
 *     dl_mix_workspace_bytes).
 *   Stream-ordered, no host synchronisation, no allocation: capturable in a hipGraph.
 * dl_track_round_plan: DL_OK and the configuration the round would run, or the refusal, without
 * touching the device. */
typedef struct dl_track_round_args {
    dl_mix_args mix;   /* x, y, W, g (required), lr, n_params, ld*, tile_cols, dev_sq, dev_max, mean;
                          halo, n_halo, mean_prev, colsum_out, n_local_src, n_halo_blocks,
                          partial_rows_out must be NULL / 0 */
    float *d; int64_t ldd;              /* the tracker, laid out as x (read) */
    float *d_out; int64_t lddo;         /* the new tracker: d itself or apart */
    const float *g_old; int64_t ldq;    /* last step's gradient, laid out as x */
} dl_track_round_args;
int dl_track_round_plan(const dl_track_round_args *args, dl_mix_plan *plan);
int dl_track_round(const dl_track_round_args *args, void *workspace, size_t ws_bytes,
                   dl_stream_t stream);
/* Adam (no reference counterpart: the reference's loops step with torch.optim.SGD).  The step of
 * torch.optim.Adam / AdamW (single-tensor form; no amsgrad, no maximize, no tensor lr) over every
 * agent row, each line ONE separately rounded fp32 operation per fl() -- no fma -- so a numpy fp32
 * restatement gives the same bits; the square root and the divides are the correctly rounded
 * ones:
 *   g  = fl(fl(wd x) + g)                     weight_decay != 0, decoupled == 0   (Adam's L2)
 *   x  = fl(x decay)                          weight_decay != 0, decoupled != 0   (AdamW)
 *   m' = fl(m + fl(omb1 fl(g - m)))
 *   v' = fl(fl(beta2 v) + fl(fl(omb2 g) g))
 *   den = fl(fl(fl(sqrt(v')) / bias2_sqrt) + eps)
 *   s  = fl(x - fl(step_size fl(m' / den)))
 * with the constants omb1 = fl32(1 - beta1), omb2 = fl32(1 - beta2), decay = fl32(1 - lr
 * weight_decay) formed in fp64 by the library (beta1 and beta2 are doubles so that 1 - beta is
 * torch's), beta2 = fl32(beta2), and the bias corrections of step t = 1, 2, ...
 *   step_size = fl32(lr / (1 - beta1^t)),  bias2_sqrt = fl32(sqrt(1 - beta2^t))     (fp64)
 * There is no first-step flag: m = v = 0 is the first step.  lr enters the arithmetic only
 * through step_size and decay.
 *
 * The coefficients come by value (step_size, bias2_sqrt; coef NULL), or from the device: coef
 * points at two floats {step_size, bias2_sqrt} that every workgroup reads once with ordinary
 * loads, and the by-value fields are ignored.  dl_adam_tick keeps them in a caller-owned device
 * state of DL_ADAM_STATE_LEN doubles (a torch float64 tensor serves):
 *   [DL_ADAM_T] the step t (0 before the first tick)    [DL_ADAM_B1T], [DL_ADAM_B2T] beta1^t, beta2^t
 *   [DL_ADAM_LR], [DL_ADAM_BETA1], [DL_ADAM_BETA2]      the caller's lr, beta1, beta2
 *   [DL_ADAM_COEF]  two floats in the slot's 8 bytes: step_size, then bias2_sqrt
 *   [7] reserved
 * The caller initialises {0, 1, 1, lr, beta1, beta2, 0, 0}.  One tick is: t += 1, each running
 * product times its beta (one fp64 multiply a step, not pow: a Python float loop gives the same
 * bits), then the two coefficients by the formulas above.  coef = (const float *)(state +
 * DL_ADAM_COEF).  With dl_adam_tick and dl_adam_round (or dl_adam_step) captured in one hipGraph
 * every replay is the next Adam step; the host may overwrite [DL_ADAM_LR] between replays (a
 * schedule without re-capture; an AdamW decay still uses the lr of the captured args).
 * Additive: callers detect these by the symbols; DLAMD_ABI_VERSION is unchanged. */
#define DL_ADAM_T 0
#define DL_ADAM_B1T 1
#define DL_ADAM_B2T 2
#define DL_ADAM_LR 3
#define DL_ADAM_BETA1 4
#define DL_ADAM_BETA2 5
#define DL_ADAM_COEF 6
#define DL_ADAM_STATE_LEN 8
/* Stream-ordered, one thread.  DL_ERR_INVALID: state NULL or not 8-byte aligned. */
int dl_adam_tick(double *state, dl_stream_t stream);

/* The Adam step over [n_rows, n_params] row-major operands (row strides as dl_sgd_step's: every
 * ld >= n_params, n_rows <= 65535).  m and v are updated in place; out may be x itself (in place,
 * as optimizer.step) or a separate buffer, e.g. the input of the following dl_mix_round.  float4
 * accesses when every pointer is 16-byte aligned and n_params and every ld are multiples of 4.
 *   DL_ERR_INVALID: args NULL; a NULL operand, a bad size or stride ("bad arguments"); beta1 or
 *     beta2 outside [0, 1) ("beta1 and beta2 must be in [0, 1)"); eps < 0 ("eps must be >= 0");
 *     coef NULL and a step_size or bias2_sqrt that is not finite ("must be finite when coef is
 *     NULL"); out overlapping x other than being it; m or v overlapping x, g, out or each other
 *     ("m overlaps x" ...). */
typedef struct dl_adam_args {
    const float *x; int64_t ldx;    /* [n_rows, ldx] parameters */
    const float *g; int64_t ldg;    /* [n_rows, ldg] gradients */
    float *m; int64_t ldm;          /* [n_rows, ldm] first moments (exp_avg), in place */
    float *v; int64_t ldv;          /* [n_rows, ldv] second moments (exp_avg_sq), in place */
    float *out; int64_t ldo;        /* [n_rows, ldo] stepped parameters (== x or disjoint) */
    int32_t n_rows;
    int64_t n_params;
    double beta1, beta2;
    float lr;                       /* only in AdamW's decay = 1 - lr weight_decay */
    float eps, weight_decay;
    int32_t decoupled;              /* 0: Adam (L2 into the gradient), 1: AdamW */
    float step_size, bias2_sqrt;    /* by value (coef NULL) */
    const float *coef;              /* nullable: device {step_size, bias2_sqrt} */
} dl_adam_args;
int dl_adam_step(const dl_adam_args *args, dl_stream_t stream);

/* The Adam step above fused into the consensus round that follows it:  y = W adam(x, g, m, v),
 * m and v updated in the same pass.  Bit for bit dl_adam_step(out = S) followed by
 * dl_mix_round(x = S, g = NULL), but one launch that moves 28 B per element (read x, g, m, v;
 * write m', v', y) instead of two that move 36 B, and no scratch matrix S.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   mix.x / mix.y are x / x', mix.g is g (required), mix.lr is the lr of AdamW's decay (the step
 *     itself takes lr through step_size).  y may be x itself with ldy == ldx (a workgroup stages
 *     all rows of its columns before it writes them).  m and v are read and written in place.
 *   m and v are laid out as x: row-major [n_rows, ld >= n_params]; column-tiled (mix.tile_cols >
 *     0) ld their block rows (0 = n_rows), 16-byte aligned operands.  Row-major: any n_params >=
 *     1, columns [n_params, ld) of y, m and v are never written.
 *   dev_sq / dev_max / mean describe y exactly as dl_mix_round's do; workspace
 *     dl_mix_workspace_bytes.  A doubly stochastic W takes mean(y) as the mean of the staged s;
 *     a tile whose mean is then not finite is measured in two passes, as for any other W.
 *   DL_ERR_INVALID: args NULL; x, y, g, m or v NULL ("null x/y/g/m/v"); every argument
 *     dl_mix_round itself refuses (W's arrays, strides, tile_cols, alignment of tiled operands, y
 *     overlapping x other than being it, y overlapping g; the texts say dl_mix_round); ldm or ldv
 *     out of range ("m and v laid out as x"); beta1 or beta2 outside [0, 1) ("beta1 and beta2
 *     must be in [0, 1)"); eps < 0 ("eps must be >= 0"); coef NULL and a step_size or bias2_sqrt
 *     that is not finite ("must be finite when coef is NULL"); m or v overlapping x, y, g or each
 *     other ("m overlaps x", ... "m overlaps v"); dl_adam_round_plan with plan NULL.
 *   DL_ERR_UNSUPPORTED: any halo, partition or lagged-deviation field (halo, n_halo, mean_prev,
 *     colsum_out, n_local_src, n_halo_blocks, partial_rows_out); rounds that plan path 2, 4 or 5
 *     (LDS tile kernel only: the caller runs dl_adam_step + dl_mix_round).
 *   DL_ERR_WORKSPACE: as dl_mix_round (deviation outputs without a 16-byte aligned workspace of
 *     dl_mix_workspace_bytes).
 *   Stream-ordered, no host synchronisation, no allocation: capturable in a hipGraph.
 * dl_adam_round_plan: DL_OK and the configuration the round would run, or the refusal, without
 * touching the device. */
typedef struct dl_adam_round_args {
    dl_mix_args mix;   /* x, y, W, g (required), lr, n_params, ld*, tile_cols, dev_sq, dev_max, mean;
                          halo, n_halo, mean_prev, colsum_out, n_local_src, n_halo_blocks,
                          partial_rows_out must be NULL / 0 */
    float *m; int64_t ldm;          /* first moments, laid out as x, in place */
    float *v; int64_t ldv;          /* second moments, laid out as x, in place */
    double beta1, beta2;
    float eps, weight_decay;
    int32_t decoupled;              /* as dl_adam_args */
    float step_size, bias2_sqrt;    /* by value (coef NULL) */
    const float *coef;              /* nullable: device {step_size, bias2_sqrt} */
} dl_adam_round_args;
int dl_adam_round_plan(const dl_adam_round_args *args, dl_mix_plan *plan);
int dl_adam_round(const dl_adam_round_args *args, void *workspace, size_t ws_bytes,
                  dl_stream_t stream);
/* out[r, j] = fl(fl(a s[r, j]) + fl(b z[r, j])) over n_rows x n_params (row strides lds_, ldz, ldo
 * >= n_params): dl_cheb_round's second line, so dl_mix_round into s and this call give the fused
 * round's bits -- the two-launch form, and the fallback where the round does not plan path 1.  out
 * may be s or z themselves (same stride) or overlap neither; n_rows or n_params 0 is a no-op.
 * float4 accesses when every pointer is 16-byte aligned and every stride a multiple of 4, with a
 * scalar tail.  DL_ERR_INVALID: a NULL pointer, negative sizes, n_rows > 65535, a stride below
 * n_params, out overlapping s or z other than being it. */
int dl_axpby(const float *s, int64_t lds_, const float *z, int64_t ldz, float a, float b,
             float *out, int64_t ldo, int32_t n_rows, int64_t n_params, dl_stream_t stream);

/* dst[i] = src[i] for n_floats floats (float4 streaming copy; variant 0: one load in flight
 * per thread, 1: eight, 2: eight + non-temporal stores, 3: four + non-temporal loads and
 * stores on a 8192-workgroup grid).  Variants 4 and 5 are the triad
 * dst[i] = src[i] - 1e-3 * src[n_floats + i] (src holds 2 * n_floats floats): two read streams
 * and one write stream, the traffic of the fused local step + mix round (12 B per element);
 * 4: one float4 per stream in flight, 512-thread workgroups x 256; 5: four, 256 x 1024; 6: the
 * round's own shape (persistent 1024-thread workgroups on 2 x CUs, 64-KiB blocks per stream,
 * next block loaded before the current one is stored; n_floats % 16384 == 0); all
 * non-temporal.  Not on the reference path: the bench uses them to measure the HBM streaming
 * ceilings next to the mix kernel's achieved bandwidth. */
int dl_stream_copy(const float *src, float *dst, int64_t n_floats, int32_t variant,
                   dl_stream_t stream);

/* One asyncio consensus round (consensus_asyncio.py:209-312) restated as synchronous Jacobi:
 *   y0_a = v_a * weight_a / mean_weight                              (:231)
 *   y_a <- y_a * (1 - eps*deg_a) + eps * sum_{j in N(a)} y_j           (:295, sum then scale;
 *          the sum is np.sum(list, axis=0): a left fold from +0.0 in socket order, so a
 *          coordinate where every neighbour holds -0.0 sums to +0.0; 0 for an agent without
 *          neighbours)
 *   flag_a = all_j all_p (y_a - y_j_previous <= conv_eps)              (:297, one-sided)
 * iterated until every flag is set (master DONE, :170-174) or max_iter.  `y` holds the values on
 * entry and the result on exit; iters_out (device int32[1]) receives the iteration count.
 * The adjacency (no self loops) lists neighbours in the agent's socket order (:104-114).
 * When all columns fit one tile the loop runs inside one launch; otherwise this call iterates on
 * the host and SYNCHRONISES the stream once per iteration. */
typedef struct dl_perron_args {
    int32_t dtype;            /* 0 = fp32, 1 = fp64 */
    void *y;                  /* [n_rows, ldy] */
    int64_t ldy;
    int32_t n_rows;
    int64_t n_params;
    const int32_t *row_ptr;   /* [n_rows + 1] adjacency */
    const int32_t *col;       /* [nnz] */
    const double *weight;     /* nullable [n_rows]: pre-scale weights (NULL: no pre-scale) */
    double mean_weight;
    double eps;
    double conv_eps;
    int32_t max_iter;
    int32_t *iters_out;       /* device [1] */
    const double *conv_eps_rows; /* nullable [n_rows]: per-agent convergence eps (an agent's own
                                    ConsensusAgent(convergence_eps=...)); overrides conv_eps */
} dl_perron_args;

size_t dl_perron_workspace_bytes(int32_t dtype, int32_t n_rows, int64_t n_params);
int dl_perron_round(const dl_perron_args *args, void *workspace, size_t ws_bytes,
                    dl_stream_t stream);

/* ---------------------------------------------------------------- asyncio message schedule
 * The reference's asyncio round is NOT synchronous Jacobi after the first round: each agent
 * answers REQUEST_VALUE with whatever iterate it holds when the request is served, drops
 * other-round messages (consensus_asyncio.py:276-278) and sees DONE only between exchanges
 * (:241-252, :260-265), so an agent may mix a neighbour's iterate t+1 or t-2 into its own step
 * t, and agents stop at different iteration counts.  The host façade
 * (utils/consensus_asyncio.py) replays that message protocol on asyncio exactly and sends every
 * arithmetic step here.  Iterates live in a caller-owned device arena of fp64 slots
 * ([n_slots][ld]); a message carries a slot index, as the reference's carries its numpy array.
 *
 * dl_async_load: y0 = v * weight / mean_weight (:231) into `slot`.  `src` is HOST memory holding
 *   n_params doubles (the caller converts fp32/int values exactly).  mode 0: numpy computes in
 *   fp64 (fp64 values, or a strong fp64/int64 weight); mode 1: in fp32 (fp32 values with Python
 *   scalar weights, NEP 50) -- weight and mean_weight already rounded to fp32 by the caller.
 *   Stream-ordered; the pageable host copy is consumed before return.
 * dl_async_update: one agent step (:295, :297)
 *     y' = y * keep + eps * S,  S = np.sum([v_0 .. v_{d-1}], axis=0) in arrival order,
 *     converged = all_j all_p ((y' - v_j) <= conv_eps)
 *   keep = 1 - eps*deg (np.float64, computed by the caller), each product and sum rounded
 *   separately.  S follows numpy's reduction exactly: a left fold from +0.0 when n_params > 1;
 *   for n_params == 1 numpy's pairwise sum (8 accumulators once d >= 8); in fp32 when every v_j
 *   is an fp32 pre-scaled value (sum_f32 = 1), else in fp64.  `flags` is a device int32[2]
 *   (zeroed once by the caller): the launch ORs violations into flags[parity] and zeroes
 *   flags[parity ^ 1] for the next launch.  converged_host (nullable): when set, the call copies
 *   the verdict there and SYNCHRONISES the stream (the protocol needs it before the agent's next
 *   message, :301-310).
 * dl_async_read: copies n_params doubles of `slot` to host memory and synchronises the stream. */
#define DL_ASYNC_MAX_NBRS 64
typedef struct dl_async_load_args {
    double *arena;            /* [n_slots][ld] */
    int64_t ld;
    int64_t n_params;
    int32_t slot;
    int32_t mode;             /* 0 = fp64, 1 = fp32 */
    const double *src;        /* host [n_params] */
    double weight;
    double mean_weight;
} dl_async_load_args;
int dl_async_load(const dl_async_load_args *args, dl_stream_t stream);

typedef struct dl_async_update_args {
    double *arena;            /* [n_slots][ld] */
    int64_t ld;
    int64_t n_params;
    int32_t self_slot;        /* the agent's current iterate y */
    int32_t out_slot;         /* receives y' (must differ from every input slot) */
    int32_t n_nbrs;           /* <= DL_ASYNC_MAX_NBRS, in arrival order */
    int32_t nbr_slots[DL_ASYNC_MAX_NBRS];
    int32_t sum_f32;
    double keep;
    double eps;
    double conv_eps;
    int32_t *flags;           /* device int32[2] */
    int32_t parity;
} dl_async_update_args;
int dl_async_update(const dl_async_update_args *args, int32_t *converged_host,
                    dl_stream_t stream);
int dl_async_read(const double *arena, int64_t ld, int32_t slot, int64_t n_params,
                  double *host_out, dl_stream_t stream);

/* ---------------------------------------------------------------- batched per-agent GEMMs
 * BASELINE config c3: every agent trains its own ANNModel (networks/ann_model.py:4-45) on its own
 * batch; the reference runs torch autograd per agent.  Here one launch covers all agents:
 *   C[b] = epi( op(A[b]) . op(B[b]) )      b < batch,  op(A) is M x K,  op(B) is K x N
 * ta: A stored [K][M] (row stride lda) instead of [M][K];  tb: B stored [N][K] instead of [K][N].
 * epi: DL_EPI_BIAS[_RELU|_TANH|_ELU] add bias[b][n] then activate (forward);
 *      DL_EPI_D{RELU,TANH,ELU} multiply by the activation derivative read from the layer's
 *      OUTPUT H[b] (ldh) (backward);  rowsum (nullable) receives sum_k op(A)[b][m][k] (the
 *      bias gradient when op(A) = dZ^T).
 *      DL_EPI_BIAS_XENT (M <= 64 rows = the batch, N <= 64 classes): add bias -> logits z, then
 *      the torch.nn.CrossEntropyLoss head in the same launch: C[b] receives
 *      dZ = (softmax(z) - onehot(labels[b])) / M and loss[b] (nullable) the mean loss; labels
 *      must lie in [0, N).  Deterministic (fixed-order sums).
 * Batch strides: an input stride may be 0 (one operand shared by every batch); with batch > 1
 * the output strides must keep the batches apart, sC >= (M-1) ldc + N and s_rowsum >= M
 * (dl_xent_grad: sD >= rows classes), otherwise DL_ERR_INVALID.
 * fp32 MFMA (16x16x4), exact fp32 products. */
enum dl_epilogue {
    DL_EPI_NONE = 0, DL_EPI_BIAS = 1, DL_EPI_BIAS_RELU = 2, DL_EPI_BIAS_TANH = 3,
    DL_EPI_BIAS_ELU = 4, DL_EPI_DRELU = 5, DL_EPI_DTANH = 6, DL_EPI_DELU = 7,
    DL_EPI_BIAS_XENT = 8
};
typedef struct dl_bgemm_args {
    int32_t batch, M, N, K;
    const float *A; int64_t lda, sA; int32_t ta;  /* sA: batch stride (elements) */
    const float *B; int64_t ldb, sB; int32_t tb;
    float *C; int64_t ldc, sC;
    int32_t epi;
    const float *bias; int64_t s_bias;
    const float *H; int64_t ldh, sH;
    float *rowsum; int64_t s_rowsum;
    const int32_t *labels; int64_t s_labels;   /* DL_EPI_BIAS_XENT: [batch][M] class ids */
    float *loss;                               /* DL_EPI_BIAS_XENT: nullable [batch] */
} dl_bgemm_args;
int dl_bgemm(const dl_bgemm_args *args, dl_stream_t stream);

/* Cross-entropy head (torch.nn.CrossEntropyLoss, mean): dZ[b] = (softmax(Z[b]) - onehot(y[b]))
 * / rows and loss[b] (nullable) = mean_r (logsumexp(Z[b][r]) - Z[b][r][y]).  Z, dZ: [batch]
 * [rows][classes] with batch strides; classes <= 64. */
int dl_xent_grad(const float *Z, int64_t sZ, const int32_t *y, int64_t sY, float *dZ, int64_t sD,
                 float *loss, int32_t batch, int32_t rows, int32_t classes, dl_stream_t stream);

/* Whole-model per-agent gradients of ANNModel (networks/ann_model.py:4-45) in ONE launch: every
 * agent's forward (Linear-ReLU-Linear-Tanh-Linear-ELU-Linear), torch.nn.CrossEntropyLoss (mean)
 * and backward, one workgroup per agent with its activations resident in LDS.  Replaces the
 * 11-launch dl_bgemm sequence for the shapes it supports (batch == 64, input_dim % 4 == 0,
 * even hidden_dim <= 152, output_dim <= 16); other shapes return DL_ERR_UNSUPPORTED and the caller
 * uses dl_bgemm.
 *   X [n_agents, ldx]: parameter rows in the Mixer flatten order (mixer.py:68-69: fc1.weight,
 *     fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias, fc4.weight, fc4.bias);
 *   data [n_agents][batch][input_dim] (agent stride s_data), labels [n_agents][batch] int32 in
 *     [0, output_dim);  G [n_agents, ldg]: receives d loss_a / d params_a (same order; columns
 *     beyond the parameter count untouched);  loss nullable [n_agents]: mean cross-entropy.
 *   tile_cols T > 0: X and G are instead in the column-tiled layout of dl_mix_args
 *     ([ceil(P/T)][n_agents][T], T a power of two >= 4; ldx, ldg ignored), the resident layout
 *     the fused round streams fastest.
 *   out_mode 1 (ABI 7): G receives the local SGD step T = X - lr G instead of the gradient, each
 *     element rounded fl(x - fl(lr g)) as dl_mix_round's fused step computes it, so a round of T
 *     (dl_mix_round with G = NULL) gives bit-for-bit the X' of the fused round of X and G while
 *     streaming one matrix instead of two; row-major needs ldg == ldx.  0: the gradient.
 *   workspace (ABI 10) nullable, else dl_mlp_workspace_bytes(n_agents) 16-byte aligned bytes:
 *     the gradients run as two launches instead of one -- everything up to dZ1, then dW1 with
 *     x's column tiles spread over two workgroups per agent; the same bits as the one-launch
 *     path (measured slower at c3's shapes: an experiment's reproducible form).  The workspace
 *     holds each agent's dZ1 between the launches.  out_mode 1 ignores it (one launch).
 * X, data and G 16-byte aligned, ldx, ldg and s_data multiples of 4, G disjoint from X. */
typedef struct dl_mlp_args {
    int32_t n_agents, batch, input_dim, hidden_dim, output_dim;
    const float *X; int64_t ldx;
    const float *data; int64_t s_data;
    const int32_t *labels; int64_t s_labels;
    float *G; int64_t ldg;
    float *loss;
    int32_t tile_cols;   /* 0 = row-major X, G;  T > 0 = column-tiled (see above) */
    int32_t out_mode;    /* 0 = gradient, 1 = local step X - lr G (ABI 7) */
    float lr;            /* out_mode 1: the step size */
    float *workspace;    /* (ABI 10) nullable: the two-launch path (above) */
} dl_mlp_args;
size_t dl_mlp_workspace_bytes(int32_t n_agents);   /* (ABI 10) */
int dl_mlp_grad(const dl_mlp_args *args, dl_stream_t stream);

/* Per-agent evaluation of ANNModel on a test set, forward only, in one launch (plus a tiny
 * reduce): every agent's mean cross-entropy, its number of correctly classified rows and,
 * optionally, its logits -- the per-node `accuracy ..., loss ...` that the reference's MasterNode
 * prints every stat_step from one shared test_loader (Man_Colab.ipynb cells 21-23), i.e.
 * ANNModel.forward (networks/ann_model.py:27-45) + CrossEntropyLoss + argmax for all agents.
 * The parameters stay in the engine's resident layout (X as dl_mlp_args: row-major, or
 * column-tiled with tile_cols > 0); activations stay in LDS.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   Shapes: input_dim % 4 == 0, even hidden_dim <= 152, output_dim <= 16, rows >= 1 (dl_mlp_grad's
 *     gate without its batch clause); anything else returns DL_ERR_UNSUPPORTED.
 *   data [rows][input_dim] per agent at stride s_data, labels [rows] int32 at stride s_labels;
 *     a stride of 0 shares one test set among all agents (the reference's case).  Labels outside
 *     [0, output_dim) give undefined loss / correct values, never an out-of-bounds access.
 *   Blocks and the reduce rule.  An agent's rows are cut into blocks of 64; one workgroup per
 *     (agent, row split) walks blocks split, split + row_splits, ...  Block b leaves in the
 *     workspace part[a][b] = the sum over its rows of term_r / 64 (term_r = logsumexp(z_r) -
 *     z_r[label_r], summed in dl_mlp_grad's order: a full block's part is, bit for bit, the loss
 *     dl_mlp_grad returns for those 64 rows) and hit[a][b] = the rows whose logit argmax is the
 *     label (first maximum on ties, as torch.argmax; a row with a NaN logit counts as wrong).  A
 *     second launch then sums in block order, no float atomics:
 *         loss[a]    = (float)((sum_b (double)part[a][b]) * 64 / rows)
 *         correct[a] = sum_b hit[a][b]
 *     so the results do not depend on row_splits or the grid.  Rows past the end of a short last
 *     block are masked; nothing is read past data or labels, and their logits are not stored.
 *   logits (nullable) [n_agents][rows][ldz]: columns [output_dim, ldz) are never written.
 *   X and data 16-byte aligned, ldx and s_data multiples of 4; logits, loss, correct and the
 *     workspace must not overlap X or data.  workspace: dl_mlp_eval_workspace_bytes(n_agents,
 *     rows) bytes, 16-byte aligned, else DL_ERR_WORKSPACE.
 *   Every refusal is decided before any device call.  Stream-ordered, no allocation, no host
 *     synchronisation: capturable in a hipGraph.
 * dl_mlp_eval_plan_query: DL_OK and the grid the call would run (blocks = ceil(rows / 64);
 * row_splits chosen so that n_agents * row_splits workgroups cover the compute units, at most
 * blocks; a row_splits hint > 0 instead, clamped to [1, blocks]), or the refusal, without
 * touching the device. */
typedef struct dl_mlp_eval_args {
    int32_t n_agents, rows, input_dim, hidden_dim, output_dim;
    const float *X; int64_t ldx; int32_t tile_cols;     /* as dl_mlp_args */
    const float *data; int64_t s_data;        /* [rows][input_dim]; agent stride, 0 = shared */
    const int32_t *labels; int64_t s_labels;  /* [rows]; 0 = shared; nullable iff loss and correct are NULL */
    float *loss;        /* nullable [n_agents]: mean cross-entropy over the rows */
    int32_t *correct;   /* nullable [n_agents] */
    float *logits; int64_t ldz, s_logits;     /* nullable [n_agents][rows][ldz >= output_dim] */
    int32_t row_splits; /* 0 = choose; a performance hint: any value gives the same bits */
} dl_mlp_eval_args;
typedef struct dl_mlp_eval_plan { int32_t blocks, row_splits, grid, lds_bytes; } dl_mlp_eval_plan;
size_t dl_mlp_eval_workspace_bytes(int32_t n_agents, int32_t rows);
int dl_mlp_eval_plan_query(const dl_mlp_eval_args *args, dl_mlp_eval_plan *plan);
int dl_mlp_eval(const dl_mlp_eval_args *args, void *workspace, size_t ws_bytes,
                dl_stream_t stream);

/* Every agent's next mini-batch gathered by index from a dataset resident in HBM: what each
 * node's DataLoader over its random_split shard hands the training loop (Man_Colab.ipynb cells
 * 16, 19-21), for all agents in one launch, with the step inside the epoch kept on the device so
 * that a replayed hipGraph walks the epoch with no host work.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   With s = (cursor ? cursor[0] : step) mod steps (non-negative, whatever the sign of the
 *     value):  data[a][b][0:dim] = samples[index[a][s * batch + b]][0:dim]  and, with labels,
 *     labels[a][b] = targets[that id],  for a < n_agents, b < batch.  index holds ONE epoch's
 *     sample ids per agent in visiting order; s_index 0 shares one list among all agents.
 *   A sample id outside [0, n_samples) is clamped into range: the values are then those of row 0
 *     or n_samples - 1, and nothing is read out of bounds (dl_mlp_eval's convention for labels).
 *   Elements [batch * dim, s_data) of each agent's data block (the padding between one agent's
 *     batch and the next) are never written, nor anything of an agent's labels past batch.
 *   dim % 4 == 0, at most 2^28; ld_samples >= dim and s_data >= batch * dim, both multiples of 4; samples and
 *     data 16-byte aligned; s_index 0 or >= steps * batch; s_labels >= batch;
 *     n_agents, batch, steps, n_samples >= 1 and n_agents * batch < 2^31.  advance is 0 or 1;
 *     advance without cursor, or labels without targets, is refused.  The outputs (data, labels,
 *     cursor) must not overlap samples, targets, index or each other.  All of these return
 *     DL_ERR_INVALID, decided before any device call.
 *   The dataset may be larger than 4 GiB: row bases are 64-bit.
 *   advance = 1 runs a second, one-thread launch after the gather on the same stream that writes
 *     cursor[0] = (s + 1) mod steps: every workgroup of the gather reads the same cursor, there
 *     is no ticket counter and no atomic, and the result is deterministic.
 *   Stream-ordered, no allocation, no host synchronisation: capturable in a hipGraph. */
typedef struct dl_batch_gather_args {
    const float *samples; int64_t ld_samples;  /* [n_samples][ld_samples >= dim] fp32 dataset */
    const int32_t *targets;                    /* nullable [n_samples] class ids */
    int32_t n_samples, dim;
    const int32_t *index; int64_t s_index;     /* [n_agents][steps*batch] sample ids of ONE epoch,
                                                  in visiting order; agent stride, 0 = shared */
    int32_t n_agents, batch, steps;
    int32_t *cursor;                           /* nullable device int32[1]: step inside the epoch */
    int32_t step;                              /* used when cursor == NULL */
    int32_t advance;                           /* 1 (needs cursor): cursor <- (s + 1) % steps after the gather */
    float *data; int64_t s_data;               /* out [n_agents][batch][dim], s_data >= batch*dim */
    int32_t *labels; int64_t s_labels;         /* out nullable [n_agents][batch]; needs targets */
} dl_batch_gather_args;
int dl_batch_gather(const dl_batch_gather_args *args, dl_stream_t stream);

/* Every agent's next mini-batch of a planar uint8 image dataset, gathered by sample id, cropped
 * from its padded image at the caller's per-sample offset, flipped, and mapped byte by byte
 * through a per-channel table to fp32 NCHW: transform_train of Man_Colab.ipynb cell 16
 * (RandomCrop(H, padding=pad), RandomHorizontalFlip, ToTensor, Normalize) -- and, without aug,
 * transform_test -- for all agents in one launch, the epoch cursor on the device as
 * dl_batch_gather keeps it.  There is no random number generator in the kernel: the draws are
 * data (aug), one word per (agent, position in the epoch), beside index.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   With s = (cursor ? cursor[0] : step) mod steps (non-negative, whatever the sign of the
 *     value), for a < n_agents, b < batch:  id = index[a * s_index + s * batch + b] clamped into
 *     [0, n_samples) (the values are then those of sample 0 or n_samples - 1, and nothing is read
 *     out of bounds), and with labels  labels[a][b] = targets[id].  index holds ONE epoch's sample
 *     ids per agent in visiting order; s_index 0 shares one list among all agents.
 *   The aug word of destination image (a, b) is aug[a * s_aug + s * batch + b] (s_aug 0 shares
 *     one list): bits 0-7 top, bits 8-15 left, bit 16 flip; higher bits are ignored; top and left
 *     are clamped to [0, 2 * pad].  aug == NULL: top = left = pad and no flip -- the test
 *     transform, and with pad = 0 a plain convert.
 *   data[a][b][c][y][x] = lut[c][ P(c, y + top - pad, (flip ? width - 1 - x : x) + left - pad) ]
 *     for c < channels, y < height, x < width, where P(c, i, j) is byte
 *     samples[id * ld_samples + (c * height + i) * width + j] when 0 <= i < height and
 *     0 <= j < width, and `fill` elsewhere.  This is torchvision's order: pad the bytes with
 *     `fill`, crop at (top, left), flip the crop, then convert; a border pixel is lut[c][fill],
 *     not 0.  The kernel copies table entries: the result is exact.
 *   Nothing is read outside [samples, samples + (n_samples - 1) * ld_samples + C*H*W) whatever
 *     the ids and offsets.  Elements [batch * C*H*W, s_data) of each agent's data block are never
 *     written, nor anything of an agent's labels past batch.
 *   Refused with DL_ERR_INVALID, each with its own message, before any device call: null
 *     samples, index, data or lut; n_agents, batch, steps, n_samples, height or width < 1;
 *     channels outside [1, 16]; width % 4 != 0; C*H*W > 2^28; pad outside [0, 127]; fill outside
 *     [0, 255]; samples not 4-byte aligned; ld_samples % 4 != 0 or < C*H*W; data or lut not
 *     16-byte aligned; s_data % 4 != 0 or < batch * C*H*W; s_index, or s_aug with aug, neither 0
 *     nor >= steps * batch; with labels, s_labels < batch; labels without targets; advance
 *     without cursor; advance not 0 or 1; n_agents * batch or steps * batch >= 2^31; any output
 *     (data, labels, cursor) sharing a byte with an input (samples, targets, index, aug, lut) or
 *     with another output -- exact extents: operands that touch do not overlap.
 *   The dataset may be larger than 4 GiB: row bases are 64-bit.
 *   advance = 1 runs a second, one-thread launch after the first on the same stream that writes
 *     cursor[0] = (s + 1) mod steps, as dl_batch_gather does.
 *   Stream-ordered, no allocation, no host synchronisation: capturable in a hipGraph. */
typedef struct dl_image_batch_args {
    const uint8_t *samples; int64_t ld_samples; /* [n_samples][ld_samples >= C*H*W] bytes, planar
                                                   [C][H][W] per sample; ld_samples in bytes */
    const int32_t *targets;                     /* nullable [n_samples] */
    int32_t n_samples, channels, height, width;
    const float *lut;                           /* [channels][256] fp32: out = lut[c][byte] */
    const int32_t *index; int64_t s_index;      /* as dl_batch_gather */
    const int32_t *aug;   int64_t s_aug;        /* nullable, same shape/positions as index; s_aug 0 = shared */
    int32_t pad, fill;                          /* `fill`-byte border of `pad` pixels on every side */
    int32_t n_agents, batch, steps;
    int32_t *cursor; int32_t step; int32_t advance;   /* as dl_batch_gather */
    float *data; int64_t s_data;                /* out [n_agents][batch][C][H][W], s_data >= batch*C*H*W */
    int32_t *labels; int64_t s_labels;          /* out nullable; needs targets */
} dl_image_batch_args;
int dl_image_batch(const dl_image_batch_args *args, dl_stream_t stream);

/* Per-agent gradients of LeNet, the model Man_Colab.ipynb cell 19 trains (model_name = 'lenet'),
 * for all agents in one call: forward, torch.nn.CrossEntropyLoss (mean over the batch) and
 * backward, each agent on its own batch with its own row of parameters.
 *     conv1 = Conv2d(3, 6, 5)   conv2 = Conv2d(6, 16, 5)
 *     fc1 = Linear(400, 120)    fc2 = Linear(120, 84)    fc3 = Linear(84, num_classes)
 *     x[B,3,32,32] -> relu(conv1) -> max_pool2d(2) -> relu(conv2) -> max_pool2d(2)
 *                  -> view(B, 400) (index c*25 + y*5 + x) -> relu(fc1) -> relu(fc2) -> fc3
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   Parameter rows are in the Mixer flatten order (mixer.py:68-69), element offsets
 *     conv1.weight [6,3,5,5] 0, conv1.bias 450, conv2.weight [16,6,5,5] 456, conv2.bias 2856,
 *     fc1.weight [120,400] 2872, fc1.bias 50872, fc2.weight [84,120] 50992, fc2.bias 61072,
 *     fc3.weight [nc,84] 61156, fc3.bias 61156 + 84 nc;  P = dl_lenet_param_count(nc) =
 *     61156 + 85 nc.  G has the same order.
 *   Max-pool backward sends a window's gradient to its first maximum in row-major window order
 *     (torch's rule); ReLU's derivative at 0 is 0, so a window whose maximum is <= 0 passes none.
 *   G == NULL: forward only (evaluation); it writes logits and / or loss, one of which must then
 *     be given.  With G, loss and logits stay optional.
 *   Launches.  One call queues a fixed sequence on the stream: the convolution forward (both
 *     stages, ReLU and pooling fused, fp32 FMA), the three Linear layers as dl_bgemm's GEMMs
 *     (bias + ReLU epilogues; with logits, fc3 once more with the plain bias epilogue into
 *     logits), the cross-entropy head (fused into fc3's GEMM at batch <= 64, else fc3 +
 *     dl_xent_grad's kernel), and with G the five backward GEMMs of the Linear layers (weight
 *     gradients straight into G, bias gradients as row sums), the GEMM dZ1 W1 that gives the
 *     gradient entering the second pooling, the convolution backward and its reduce.
 *   Summation order (no float atomics; results do not depend on the grid, and agent a's outputs
 *     are the same bits whether it runs alone or among n_agents):
 *     - a convolution output starts from its bias and adds input channels, kernel rows and kernel
 *       columns in that order, one fma each;
 *     - the GEMMs are k-ordered fma chains (dl_bgemm); the loss is dl_bgemm's / dl_xent_grad's;
 *     - the gradient entering the first pooling adds conv2's output channels in order and, per
 *       channel, its pooled windows in row-major order;
 *     - a convolution weight gradient adds, per image, the pooled windows in row-major order (one
 *       fma each; only a window's winner carries a gradient), images in order inside a group of
 *       4 consecutive images of the batch, and then the ceil(batch / 4) group sums in group
 *       order; a convolution bias gradient likewise.
 *   Gates, each refused with its own message before any device call: DL_ERR_INVALID for null
 *     args, X or data; no output (G, loss and logits all NULL); labels NULL with G or loss;
 *     n_agents or batch < 1, n_agents > 65535, num_classes < 1; X, data or G not 16-byte
 *     aligned; ldx, ldg or s_data not a multiple of 4; ldx or ldg < P; s_data neither 0 (one batch
 *     shared by all agents) nor >= batch * 3072; s_labels neither 0 nor >= batch; with logits,
 *     ldz < num_classes or (n_agents > 1) s_logits < (batch - 1) ldz + num_classes; any output
 *     (G, loss, logits, workspace) sharing a byte with an input (X, data, labels) or another
 *     output -- exact extents: operands that touch do not overlap.  DL_ERR_UNSUPPORTED for
 *     num_classes > 64 (the cross-entropy head's limit).  DL_ERR_WORKSPACE for a workspace that
 *     is NULL, not 16-byte aligned or smaller than dl_lenet_workspace_bytes.
 *   Columns [P, ldg) of G and [num_classes, ldz) of logits are never written.  Labels outside
 *     [0, num_classes) give undefined loss and gradient values, never an out-of-bounds access.
 *   X and data must be finite.  The backward multiplies a zero gradient (a window with no
 *     winner, a gather slot out of reach) by a value it loads anyway -- a pixel, a pooled
 *     activation, a conv2 weight, possibly at another position -- which is exact for finite
 *     values; an Inf or NaN there would reach gradients that torch leaves finite.
 *   Row-major operands only.  Stream-ordered, no allocation, no host synchronisation: capturable
 *     in a hipGraph. */
typedef struct dl_lenet_args {
    int32_t n_agents, batch, num_classes;
    const float *X; int64_t ldx;              /* [n_agents][ldx >= P] row-major parameter rows */
    const float *data; int64_t s_data;        /* [batch][3][32][32] per agent; agent stride, 0 = shared */
    const int32_t *labels; int64_t s_labels;  /* [batch]; 0 = shared; nullable iff G and loss are NULL */
    float *G; int64_t ldg;                    /* nullable: d loss_a / d params_a, columns [P, ldg) never written */
    float *loss;                              /* nullable [n_agents] */
    float *logits; int64_t ldz, s_logits;     /* nullable [n_agents][batch][ldz >= num_classes] */
} dl_lenet_args;
int32_t dl_lenet_param_count(int32_t num_classes);   /* 0 when num_classes < 1 */
size_t dl_lenet_workspace_bytes(int32_t n_agents, int32_t batch, int32_t num_classes);
int dl_lenet_grad(const dl_lenet_args *args, void *workspace, size_t ws_bytes, dl_stream_t stream);
/* The same call with a HIP event recorded on the stream before each of its launches and one
 * after the last (a measurement aid: the time between consecutive events is one launch's).
 * events: host array of n_events hipEvent_t created by the caller; *n_launches (nullable)
 * receives the launches queued.  Fewer events than launches + 1: DL_ERR_INVALID, nothing runs. */
int dl_lenet_grad_events(const dl_lenet_args *args, void *workspace, size_t ws_bytes,
                         dl_stream_t stream, void *const *events, int32_t n_events,
                         int32_t *n_launches);

/* Per-agent evaluation of LeNet on a test set, forward only, in one launch plus a tiny reduce:
 * every agent's mean cross-entropy, its number of correctly classified rows and, optionally, its
 * logits -- the per-node `accuracy ..., loss ...` that the reference's MasterNode prints every
 * stat_step from one shared test_loader (Man_Colab.ipynb cells 21-23) with model_name = 'lenet'.
 * dl_mlp_eval's counterpart for dl_lenet_grad's model: X, data, labels and logits as in
 * dl_lenet_args (row-major parameter rows in the Mixer flatten order).  Activations never go to
 * HBM: they stay in LDS.
 * Additive: callers detect it by the symbol; DLAMD_ABI_VERSION is unchanged.
 *   Limits, each refused with its own message before any device call: DL_ERR_INVALID for null
 *     args, X or data; no output (loss, correct and logits all NULL); labels NULL with loss or
 *     correct; n_agents < 1 or > 65535; rows < 1; num_classes < 1; X or data not 16-byte aligned;
 *     ldx not a multiple of 4 or < P = dl_lenet_param_count(num_classes); s_data neither 0 (one
 *     test set shared by all agents, the reference's case) nor a multiple of 4 >= rows * 3072;
 *     s_labels neither 0 nor >= rows; with logits, ldz < num_classes or (n_agents > 1) s_logits <
 *     (rows - 1) ldz + num_classes; row_splits < 0, or a hint so large that n_agents * row_splits
 *     reaches 2^31; any output (loss, correct, logits, workspace) sharing a byte with an input (X,
 *     data, labels) or another output -- exact extents: operands that touch do not overlap.
 *     DL_ERR_UNSUPPORTED for num_classes > 64 (the cross-entropy head's limit).
 *     DL_ERR_WORKSPACE for a workspace that is NULL, not 16-byte aligned or smaller than
 *     dl_lenet_eval_workspace_bytes.  rows * 3072 * 4 may pass 4 GiB: row and agent bases are
 *     64-bit.
 *   Blocks.  An agent's rows are cut into blocks of 64; one workgroup per (agent, row split)
 *     walks blocks split, split + row_splits, ...
 *   Logits are, bit for bit, what the forward-only dl_lenet_grad writes for the same inputs: a
 *     convolution output starts from its bias and adds input channels, kernel rows and kernel
 *     columns in that order, one fma each; each Linear output is a k-ordered fp32 fma chain from
 *     0 over the whole K (v_mfma_f32_16x16x4_f32, as dl_bgemm), then + bias, then ReLU.
 *   Block sums.  Block b leaves in the workspace part[a][b] = the sum over its valid rows of
 *     term_r / 64, term_r = logf(sum_c expf(z_r[c] - max)) + max - z_r[label_r] computed as
 *     dl_bgemm's cross-entropy head does (the same butterflies over 64 lanes), summed in that
 *     head's order: wave w of 4 adds rows w, w + 4, ... in increasing order, then (l0 + l1) +
 *     (l2 + l3).  A full block's part is therefore, bit for bit, the loss dl_lenet_grad returns
 *     for those 64 rows as a batch.
 *   Hits.  hit[a][b] = the block's rows whose logit argmax is the label (first maximum on ties,
 *     as torch.argmax; a row with a NaN logit counts as wrong).
 *   Reduce.  A second, tiny launch sums in block order, no float atomics:
 *         loss[a]    = (float)((sum_b (double)part[a][b]) * 64 / rows)
 *         correct[a] = sum_b hit[a][b]
 *     so the results do not depend on row_splits, the grid or n_agents.
 *   Containment.  Rows past the end of a short last block are masked: nothing is read past data
 *     or labels and their logits are not stored.  Labels outside [0, num_classes) give undefined
 *     loss / correct values, never an out-of-bounds access.  Columns [num_classes, ldz) of logits
 *     are never written and columns [P, ldx) of X never read.
 *   Workspace: dl_lenet_eval_workspace_bytes(n_agents, rows) bytes, 16-byte aligned; it holds
 *     only part and hit ([n_agents][ceil(rows / 64)] floats and as many int32, each rounded up to
 *     256 bytes).
 *   Stream-ordered, no allocation, no host synchronisation: capturable in a hipGraph, where a
 *     call with loss or correct is a linear graph of two kernels (logits alone: one).
 * dl_lenet_eval_plan_query: DL_OK and the grid the call would run (blocks = ceil(rows / 64);
 * row_splits chosen so that n_agents * row_splits workgroups cover the compute units at the
 * kernel's two workgroups per unit, at most blocks; a row_splits hint > 0 instead, clamped to
 * [1, blocks]; lds_bytes = what the kernel declares), or the refusal, without touching the
 * device (the workspace is not part of the query). */
typedef struct dl_lenet_eval_args {
    int32_t n_agents, rows, num_classes;
    const float *X; int64_t ldx;              /* as dl_lenet_args: row-major parameter rows */
    const float *data; int64_t s_data;        /* [rows][3][32][32]; agent stride, 0 = shared */
    const int32_t *labels; int64_t s_labels;  /* [rows]; 0 = shared; nullable iff loss and correct are NULL */
    float *loss;        /* nullable [n_agents]: mean cross-entropy over the rows */
    int32_t *correct;   /* nullable [n_agents] */
    float *logits; int64_t ldz, s_logits;     /* nullable [n_agents][rows][ldz >= num_classes] */
    int32_t row_splits; /* 0 = choose; a hint: any value gives the same bits */
} dl_lenet_eval_args;
typedef struct dl_lenet_eval_plan { int32_t blocks, row_splits, grid, lds_bytes; } dl_lenet_eval_plan;
size_t dl_lenet_eval_workspace_bytes(int32_t n_agents, int32_t rows);
int dl_lenet_eval_plan_query(const dl_lenet_eval_args *args, dl_lenet_eval_plan *plan);
int dl_lenet_eval(const dl_lenet_eval_args *args, void *workspace, size_t ws_bytes,
                  dl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLAMD_H */
