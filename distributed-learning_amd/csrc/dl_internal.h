// Internal launcher interface between the C ABI (capi.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "launch.h"   // the kernels' parameters; plan.h: the tile geometry shared with the planner

namespace dl {

// max(a, b) that keeps a NaN, as numpy's max and Python's max over np.linalg.norm values do
// (fmaxf drops it: a NaN deviation then reads as the 0 the maximum started from).  For two
// numbers it is fmaxf's value.  A NaN result's sign is not defined; the atomicMax reductions
// that follow order the bits as unsigned, where a NaN of either sign is above +inf.
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// Raise kernel k's dynamic-LDS limit to the whole CU (kLdsBytes), once per (kernel, device):
// launches then make no attribute call, so they are capturable in a hipGraph and carry no
// per-launch driver work.
hipError_t allow_full_lds(const void *k);
// Launch kernel k on `grid` workgroups of kTileThreads with `lds` bytes of dynamic LDS.
template <class... P, class... A>
hipError_t launch_lds(void (*k)(P...), int grid, int lds, hipStream_t s, const A &...args) {
    hipError_t e = allow_full_lds(reinterpret_cast<const void *>(k));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kTileThreads), lds, s, args...);
    return hipGetLastError();
}

hipError_t launch_mix_tile(const TileArgs &a, int chunks, bool sgd, bool dev, bool mix, int grid,
                           int lds_bytes, bool fast, hipStream_t s);
// columns: Knobs::gather_order_columns
hipError_t launch_mix_gather(const TileArgs &a, bool sgd, bool columns, hipStream_t s);
// The register-CSR tile kernels (plan.h reg_csr_supported / reg_tail_supported).  head 0: the
// regular one (path 4); head > 0: head + LDS tail (path 5), the tail as {weight, row} pairs of
// 8 B (tail_fmt 2, heads < 5) or weights + u16 rows (1: 6 B)
hipError_t launch_mix_tile_reg(const TileArgs &a, int chunks, int head, int tail_fmt, bool sgd,
                               bool dev, int grid, int lds, hipStream_t s);
// The fused momentum-SGD round's tile kernel (mix_sgd.hip) for one launch of a path-1 round
// shaped by shape_sgd_round: TileArgs as for launch_mix_tile (g required, no halo rows, no row
// set), plus the momentum buffers and the optimizer's parameters (launch.h SgdTileArgs).
hipError_t launch_mix_sgd_tile(const TileArgs &a, const SgdTileArgs &q, int chunks, bool dev,
                               int grid, int lds_bytes, bool fast, hipStream_t s);
// The Chebyshev round's tile kernel (mix_cheb.hip) for one launch of a path-1 round shaped by
// shape_cheb_round: TileArgs as for launch_mix_tile (no g, no halo rows, no row set), plus z and
// the coefficients (launch.h ChebTileArgs).
hipError_t launch_mix_cheb_tile(const TileArgs &a, const ChebTileArgs &q, int chunks, bool dev,
                                int grid, int lds_bytes, bool fast, hipStream_t s);
// The gradient-tracking round's tile kernel (mix_track.hip) for one launch of a path-1 round
// shaped by shape_track_round: TileArgs as for launch_mix_tile (g required, no halo rows, no row
// set), plus the tracker, its output and last step's gradient (launch.h TrackTileArgs).
hipError_t launch_mix_track_tile(const TileArgs &a, const TrackTileArgs &q, int chunks, bool dev,
                                 int grid, int lds_bytes, bool fast, hipStream_t s);
// The Adam round's tile kernel (mix_adam.hip) for one launch of a path-1 round shaped by
// shape_adam_round: TileArgs as for launch_mix_tile (g required, no halo rows, no row set), plus
// the two moments and the optimizer's parameters (launch.h AdamTileArgs).
hipError_t launch_mix_adam_tile(const TileArgs &a, const AdamTileArgs &q, int chunks, bool dev,
                                int grid, int lds_bytes, bool fast, hipStream_t s);
// out = fl(fl(a * s) + fl(b * z)) over n_rows x n_params (aux_kernels.hip); vec: float4 accesses
hipError_t launch_axpby(const float *src, int64_t lds_, const float *z, int64_t ldz, float a,
                        float b, float *out, int64_t ldo, int n_rows, int64_t n_params, bool vec,
                        hipStream_t s);
// K rounds of mixing on LDS-resident tiles (mix_multi.hip); FAST tiles only, no halo rows
hipError_t launch_mix_multi(const TileArgs &a, int chunks, int rounds, bool sgd, bool dev,
                            int grid, int lds, hipStream_t s);
// K rounds on LDS-resident column chunks with the per-round max deviation trace
// (mix_trace.hip): mix_trace_kernel + trace_reduce into trace_out[rounds]; at most
// trace_max_rounds() rounds (plan.h).  planes: Knobs::trace_planes
hipError_t launch_mix_trace(const TileArgs &a, int chunks, bool planes, int rounds, int grid,
                            int lds, float *trace_out, hipStream_t s);
// mix_trace_irr_kernel (one image, register head + LDS tail of 8-byte pairs, one 4-column
// chunk per step): irregular graphs of more than 2048 agents and W that are not doubly
// stochastic (general_mean: every round's column mean from its outputs).  KV agents per thread,
// irr_trace_rounds(KV) rounds per pass (plan.h).
// narrow: 2-column steps (8-byte image entries) and a 6-byte LDS tail, for larger CSRs
hipError_t launch_mix_trace_irr(const TileArgs &a, int head, bool general_mean, bool narrow,
                                int rounds, int grid, int lds, float *trace_out, hipStream_t s);
// max_zeroed: an earlier launch on the stream already zeroed dev_max (TileArgs::dev_max_zero)
hipError_t launch_dev_reduce(const float *partial, int nparts, int n_rows, float *dev_sq,
                             float *dev_max, hipStream_t s, bool max_zeroed = false);
hipError_t launch_column_sum(const float *x, int64_t ldx, int n_rows, int64_t n_params,
                             float *colsum, float scale, hipStream_t s);
hipError_t launch_dev_rows(const float *x, int64_t ldx, int n_rows, int64_t n_params,
                           const float *mean, float *partial, int nparts, hipStream_t s);
int dev_rows_parts(int64_t n_params);
hipError_t launch_stream_copy(const float *src, float *dst, int64_t n_floats, int variant,
                              hipStream_t s);
hipError_t launch_tile_convert(const float *src, float *dst, int64_t ld, int n_rows, int64_t n_params,
                               int tile_cols, bool to_tiled, hipStream_t s);
hipError_t launch_max_column_std(const float *x, int64_t ldx, int n_rows, int64_t n_params,
                                 float *out, hipStream_t s);
hipError_t launch_step_rows(const float *x, int64_t ldx, const float *g, int64_t ldg, float lr,
                            const int32_t *rows, int n_sel, int64_t n_params, float *out,
                            int64_t ldo, hipStream_t s);
// a halo pack's peers: peer b's rows are rows[row0[b], row0[b+1]), its tiled block goes to out[b]
constexpr int kMaxPackPeers = 16;
struct PackPeers {
    int32_t n;
    int32_t row0[kMaxPackPeers + 1];
    float4 *out[kMaxPackPeers];
};
hipError_t launch_step_rows_tiled(const float *x, int x_rows, const float *g, int g_rows,
                                  float lr, const int32_t *rows, const PackPeers &pp,
                                  int64_t n_tiles, int tile_cols, hipStream_t s);
hipError_t launch_sgd_step(const float *x, int64_t ldx, const float *g, int64_t ldg, float *buf,
                           int64_t ldb, float *out, int64_t ldo, int n_rows, int64_t n_params,
                           float lr, float mu, float damp, float wd, int first, int nesterov,
                           bool vec, hipStream_t s);
// adam_elem over n_rows x n_params, m and v in place (aux_kernels.hip); vec: float4 accesses
hipError_t launch_adam_step(const float *x, int64_t ldx, const float *g, int64_t ldg, float *m,
                            int64_t ldm, float *v, int64_t ldv, float *out, int64_t ldo,
                            int n_rows, int64_t n_params, const AdamParams &p, bool vec,
                            hipStream_t s);
// one step of the device-resident Adam step count (include/dlamd.h DL_ADAM_*)
hipError_t launch_adam_tick(double *state, hipStream_t s);

struct PerronArgs {
    void *y;
    int64_t ldy;
    void *ybuf;       // workspace ping-pong buffer [n_rows, n_params] (multi-tile only)
    int32_t n_rows;
    int64_t n_params;
    const int32_t *rowptr;
    const int32_t *col;
    const double *weight;
    double mean_weight;
    double eps;
    double conv_eps;
    int32_t max_iter;
    int32_t *iters_out;
    int32_t *notconv;  // workspace flag (multi-tile)
    const double *conv_rows;  // nullable per-row conv eps
};
int perron_tile_cols(int dtype, int n_rows, int64_t n_params);
hipError_t launch_perron_single(const PerronArgs &a, int dtype, int tile_cols, hipStream_t s);
hipError_t launch_perron_step(const PerronArgs &a, int dtype, int tile_cols, const void *yin,
                              void *yout, bool prescale, hipStream_t s);

// Mixer.mix(times, eps) loop in one workgroup (mix_until.hip)
struct UntilArgs {
    const float *x;
    int64_t ldx;
    float *y;
    int64_t ldy;
    int64_t n_params;
    int32_t chunks;   // float4 chunks per LDS row: ceil(n_params / 4)
    int32_t n_rows;
    int32_t nnz;
    const int32_t *rowptr;
    const int32_t *col;
    const float *w;
    int32_t times;
    int32_t use_eps;
    float eps;
    int32_t max_rounds;
    int32_t *status;
    float *dev_trace;
};
int64_t until_lds_bytes(int n_rows, int64_t n_params, int nnz);
hipError_t launch_mix_until(const UntilArgs &a, hipStream_t s);

// c1 consensus GD, all agents and iterations in one workgroup (consensus_gd.hip)
struct GdArgs {
    const double *X;
    const double *y;
    const int32_t *shard_ptr;
    int32_t n_agents;
    int32_t n_features;
    const int32_t *rowptr;
    const int32_t *col;
    double eps;
    double conv_eps;
    double mean_weight;
    double tau;
    const double *steps;
    int32_t iterations;
    int32_t max_iter;
    double *w;
    int32_t *iters_out;
    int32_t x_in_lds;
    int64_t x_off;
};
int64_t gd_lds_bytes(int n_agents, int n_features, int rows, bool x_in_lds, int64_t *x_off);
hipError_t launch_consensus_gd(const GdArgs &a, int lds_bytes, hipStream_t s);

hipError_t launch_bgemm(const BgemmArgs &p, hipStream_t s);
hipError_t launch_xent_grad(const float *Z, int64_t sZ, const int32_t *y, int64_t sY, float *dZ,
                            int64_t sD, float *loss, int batch, int rows, int classes,
                            hipStream_t s);

hipError_t launch_mlp_fused(const float *X, int64_t ldx, const float *data, int64_t s_data,
                            const int32_t *labels, int64_t s_lab, float *G, int64_t ldg,
                            float *loss, int n_agents, int din, int dh, int dout, int tile_cols,
                            bool step, float lr, float *ws, hipStream_t s);
// ws: the split gradient path's workspace (launch.h mlp_workspace_floats), nullable

// dl_mlp_eval's kernel parameter (mlp_fused.hip mlp_eval_kernel), after launch.h shape_mlp_eval
struct MlpEvalArgs {
    const float *X;
    int64_t ldx;
    const float *data;
    int64_t s_data;
    const int32_t *labels;   // nullable with loss == correct == NULL (logits only)
    int64_t s_lab;
    float *part;             // [n_agents][blocks] per-block loss parts (workspace)
    int32_t *hit;            // [n_agents][blocks] per-block correct counts (workspace)
    float *logits;           // nullable
    int64_t ldz, s_logits;
    int32_t rows, blocks, row_splits;
    int32_t din, dh, dout;
    int32_t tsh;             // column-tiled X: log2 of the tile width (0 = row-major)
    int64_t tstride;         // column-tiled: n_agents * T floats per tile
};
// the evaluation launch on n_agents * row_splits workgroups and, with loss or correct, the
// block-order reduce after it
hipError_t launch_mlp_eval(const MlpEvalArgs &p, int n_agents, float *loss, int32_t *correct,
                           hipStream_t s);
// that reduce (also dl_lenet_eval's): loss[a] = (float)((sum_b (double)part[a][b]) * 64 / rows),
// correct[a] = sum_b hit[a][b], both in block order; loss or correct may be NULL
hipError_t launch_eval_reduce(const float *part, const int32_t *hit, int n_agents, int blocks,
                              int rows, float *loss, int32_t *correct, hipStream_t s);

// dl_batch_gather's launches (batch_gather.hip) as launch.h shape_batch_gather shaped them: the
// gather and, with `advance` (the cursor, writable), the one-thread launch that steps it
hipError_t launch_batch_gather(const BatchGatherPlan &p, int32_t *advance, hipStream_t s);

// dl_image_batch's launches (image_batch.hip) as launch.h shape_image_batch shaped them: the
// batch and, with `advance` (the cursor, writable), the one-thread launch that steps it
hipError_t launch_image_batch(const ImageBatchPlan &p, int32_t *advance, hipStream_t s);

// dl_lenet_grad's convolution kernels (lenet.hip) as launch.h shape_lenet shaped them.
hipError_t launch_lenet_conv_fwd(const LenetConvArgs &p, int grid, hipStream_t s);
hipError_t launch_lenet_conv_bwd(const LenetConvArgs &p, int grid, hipStream_t s);
// G[a][j] = sum of agent a's group partials in group order, j < 2872
hipError_t launch_lenet_conv_reduce(const LenetConvArgs &p, int n_agents, hipStream_t s);

// dl_lenet_eval's kernel parameter (lenet_eval.hip), after launch.h shape_lenet_eval
struct LenetEvalArgs {
    const float *X;          // parameter rows
    int64_t ldx;
    const float *data;       // [rows][3][32][32] per agent
    int64_t s_data;
    const int32_t *labels;   // nullable with loss == correct == NULL (logits only)
    int64_t s_lab;
    float *part;             // [n_agents][blocks] per-block loss parts (workspace)
    int32_t *hit;            // [n_agents][blocks] per-block correct counts (workspace)
    float *logits;           // nullable
    int64_t ldz, s_logits;
    int32_t n_agents, rows, blocks, row_splits, nc;
};
// the evaluation launch on n_agents * row_splits workgroups with lds_bytes of LDS and, with loss
// or correct, the block-order reduce after it
hipError_t launch_lenet_eval(const LenetEvalArgs &p, int lds_bytes, float *loss, int32_t *correct,
                             hipStream_t s);

// sets dl_last_error()'s message (capi.hip) and returns code: for host-only entry points
// defined outside capi.hip
int fail_msg(int code, const char *msg);

}  // namespace dl
