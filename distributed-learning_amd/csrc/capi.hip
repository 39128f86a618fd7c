// C ABI of libdlamd.so (include/dlamd.h): the thread-local error, the device's compute units and
// the environment knobs, read once per call.  What an entry point checks and launches is decided
// by the host-only units -- the planner (plan.h) and the launch shaping (launch.h); here their
// description of a call is turned into launch_* calls and the step after them.  Shaped there:
// the rounds (dl_mix_round, dl_mix_rounds, dl_mix_rounds_trace, dl_sgd_round, dl_cheb_round, dl_track_round, dl_adam_round), the one-pass
// deviation, dl_mlp_grad, dl_mlp_eval, dl_bgemm, dl_batch_gather, dl_image_batch, dl_lenet_grad
// and dl_lenet_eval.  The others (dl_mix_until, dl_consensus_gd, dl_perron_round, the two-pass
// deviation, the conversions, the step-rows functions, ...) check their own arguments here:
// their LDS-size functions live in kernel files.  No exceptions cross this boundary; every entry
// point returns a dl_status and leaves a thread-local message for dl_last_error().
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/dlamd.h"
#include "dl_internal.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_fail(hipError_t e, const char *where) {
    return fail(DL_ERR_HIP, "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
}

// Compute units of the current device (cached per device ordinal).
int device_cus() {
    static std::mutex mu;
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    std::lock_guard<std::mutex> lock(mu);
    if (cache[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n <= 0)
            n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

using dl::align_up;
using dl::aligned16;
using dl::overlaps;
constexpr size_t kAlign = dl::kWsAlign;

using dl::Plan;

// A host-only function's status; a failure's text (err) goes to dl_last_error().
int status(int rc, const char *err) { return rc ? fail(rc, "%s", err) : DL_OK; }

// The planners of plan.h for the current device; a failure's text goes to dl_last_error().
template <class P>
int plan_with(int (*planner)(const dl_mix_args &, int, const dl::Knobs &, P *, char *),
              const dl_mix_args *a, const dl::Knobs &k, P *pl) {
    char err[dl::kErrLen];
    return status(planner(*a, device_cus(), k, pl, err), err);
}
int plan_mix(const dl_mix_args *a, Plan *pl) {
    return plan_with(dl::plan_mix, a, dl::read_knobs(), pl);
}
int plan_rounds(const dl_mix_args *a, Plan *pl) {
    return plan_with(dl::plan_rounds, a, dl::read_knobs(), pl);
}
int check_mix_args(const dl_mix_args *a) {
    char err[dl::kErrLen];
    return status(dl::check_mix_args(a, err), err);
}

// Deviation of x (n_rows x n_params) via the two-pass path: mean (given or column mean), then
// per-row partial sums, then the fixed-order reduce.
int deviation_two_pass(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params,
                       const float *mean_in, float *dev_sq, float *dev_max, float *mean_out,
                       char *ws, size_t ws_bytes, hipStream_t s) {
    const int parts = dl::dev_rows_parts(n_params);
    const size_t part_b = align_up((size_t)parts * n_rows * 4);
    const size_t mean_b = align_up((size_t)n_params * 4);
    if (ws_bytes < part_b + mean_b) return fail(DL_ERR_WORKSPACE, "deviation: workspace too small");
    float *partial = reinterpret_cast<float *>(ws);
    const float *mean = mean_in;
    if (!mean) {
        float *m = mean_out ? mean_out : reinterpret_cast<float *>(ws + part_b);
        hipError_t e = dl::launch_column_sum(x, ldx, n_rows, n_params, m, (float)n_rows, s);
        if (e != hipSuccess) return hip_fail(e, "column_sum");
        mean = m;
    } else if (mean_out && mean_out != mean_in) {
        hipError_t e = hipMemcpyAsync(mean_out, mean_in, (size_t)n_params * 4,
                                      hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "mean copy");
    }
    hipError_t e = dl::launch_dev_rows(x, ldx, n_rows, n_params, mean, partial, parts, s);
    if (e != hipSuccess) return hip_fail(e, "dev_rows");
    e = dl::launch_dev_reduce(partial, parts, n_rows, dev_sq, dev_max, s);
    if (e != hipSuccess) return hip_fail(e, "dev_reduce");
    return DL_OK;
}

int zero_deviation(int32_t n_rows, float *dev_sq, float *dev_max, hipStream_t s) {
    if (dev_sq) {
        hipError_t e = hipMemsetAsync(dev_sq, 0, (size_t)n_rows * 4, s);
        if (e != hipSuccess) return hip_fail(e, "memset dev_sq");
    }
    if (dev_max) {
        hipError_t e = hipMemsetAsync(dev_max, 0, 4, s);
        if (e != hipSuccess) return hip_fail(e, "memset dev_max");
    }
    return DL_OK;
}

// Issues the launches a shaping function of launch.h described and the zeroing or reduce after
// them (kAfterPartialRows and kAfterTwoPass are dl_mix_round's own).  tile: what a tile launch
// is called in a HIP failure's text.
int run(const dl::Launches &L, float *dev_sq, float *dev_max, float *trace, const char *tile,
        hipStream_t s) {
    for (int i = 0; i < L.n; ++i) {
        const dl::Launch &l = L.l[i];
        hipError_t e = hipErrorInvalidValue;
        const char *who = "";
        switch (l.kind) {
            case dl::kLaunchTile:
                e = dl::launch_mix_tile(l.t, l.chunks, l.sgd, l.dev, l.mix, l.grid, l.lds, l.fast,
                                        s);
                break;
            case dl::kLaunchSgdTile:
                e = dl::launch_mix_sgd_tile(l.t, l.q, l.chunks, l.dev, l.grid, l.lds, l.fast, s);
                break;
            case dl::kLaunchChebTile:
                e = dl::launch_mix_cheb_tile(l.t, l.c, l.chunks, l.dev, l.grid, l.lds, l.fast, s);
                break;
            case dl::kLaunchTrackTile:
                e = dl::launch_mix_track_tile(l.t, l.k, l.chunks, l.dev, l.grid, l.lds, l.fast, s);
                break;
            case dl::kLaunchAdamTile:
                e = dl::launch_mix_adam_tile(l.t, l.a, l.chunks, l.dev, l.grid, l.lds, l.fast, s);
                break;
            case dl::kLaunchTileReg:
                e = dl::launch_mix_tile_reg(l.t, l.chunks, l.head, l.tail_fmt, l.sgd, l.dev, l.grid,
                                            l.lds, s);
                break;
            case dl::kLaunchGather:
                e = dl::launch_mix_gather(l.t, l.sgd, l.columns, s);
                who = "mix_gather_kernel launch";
                break;
            case dl::kLaunchMulti:
                e = dl::launch_mix_multi(l.t, l.chunks, l.rounds, l.sgd, l.dev, l.grid, l.lds, s);
                who = "mix_multi_kernel launch";
                break;
            case dl::kLaunchTrace:
                e = dl::launch_mix_trace(l.t, l.chunks, l.planes, l.rounds, l.grid, l.lds, trace,
                                         s);
                who = "mix_trace_kernel launch";
                break;
            case dl::kLaunchTraceIrr:
                e = dl::launch_mix_trace_irr(l.t, l.head, l.gm, l.narrow, l.rounds, l.grid, l.lds,
                                             trace, s);
                who = "mix_trace_kernel launch";
                break;
        }
        if (e == hipSuccess) continue;
        if (*who) return hip_fail(e, who);
        return fail(DL_ERR_HIP, "%s%s launch: %s (%d)", tile, l.fast ? "" : " (tail)",
                    hipGetErrorString(e), (int)e);
    }
    if (L.after == dl::kAfterZero) return zero_deviation(L.l[0].t.n_rows, dev_sq, dev_max, s);
    if (L.after == dl::kAfterReduce) {
        hipError_t e = dl::launch_dev_reduce(L.partial, L.parts, L.rows, dev_sq, dev_max, s,
                                             L.max_zeroed);
        if (e != hipSuccess) return hip_fail(e, "dev_reduce launch");
    }
    return DL_OK;
}

// The one-pass deviation (launch.h shape_deviation); DL_ERR_UNSUPPORTED without launching when
// the agents do not fit one tile.
int deviation_one_pass(const float *x, int64_t ldx, int32_t tile_cols, int32_t n_rows,
                       int64_t n_params, float *dev_sq, float *dev_max, float *mean_out,
                       char *ws, size_t ws_bytes, hipStream_t s) {
    dl::Launches L;
    char err[dl::kErrLen] = "";
    const int rc = dl::shape_deviation(x, ldx, tile_cols, n_rows, n_params, mean_out, device_cus(),
                                       ws, ws_bytes, &L, err);
    if (rc) return *err ? status(rc, err) : rc;
    return run(L, dev_sq, dev_max, nullptr, "dev tile", s);
}

// The fused rounds' entry points (launch.h shape_sgd_round, shape_cheb_round, shape_track_round,
// shape_adam_round):
// the plan query, and the round itself.  kernel: `run`'s name for a tile launch.
template <class Args>
using ShapeFused = int (*)(const Args *, int, const dl::Knobs &, void *, size_t, dl_mix_plan *,
                           dl::Launches *, char *);
template <class Args>
int fused_round_plan(ShapeFused<Args> shape, const Args *args, dl_mix_plan *plan) {
    g_err.clear();
    char err[dl::kErrLen];
    return status(shape(args, device_cus(), dl::read_knobs(), nullptr, 0, plan, nullptr, err),
                  err);
}
template <class Args>
int fused_round(ShapeFused<Args> shape, const char *kernel, const Args *args, void *workspace,
                size_t ws_bytes, dl_stream_t stream) {
    g_err.clear();
    dl::Launches L;
    char err[dl::kErrLen];
    const int rc = shape(args, device_cus(), dl::read_knobs(), workspace, ws_bytes, nullptr, &L,
                         err);
    if (rc) return status(rc, err);
    return run(L, args->mix.dev_sq, args->mix.dev_max, nullptr, kernel,
               static_cast<hipStream_t>(stream));
}

}  // namespace

namespace dl {
int fail_msg(int code, const char *msg) {
    g_err = msg;
    return code;
}
}  // namespace dl

extern "C" {

int dl_abi_version(void) { return DLAMD_ABI_VERSION; }

int dl_mix_trace_plan(const dl_mix_args *args, int32_t *max_rounds) {
    g_err.clear();
    if (!max_rounds) return fail(DL_ERR_INVALID, "dl_mix_trace_plan: max_rounds is NULL");
    int rc = check_mix_args(args);
    if (rc) return rc;
    dl::TracePlan tp;
    rc = plan_with(dl::plan_trace, args, dl::read_knobs(), &tp);
    if (rc) return rc;
    *max_rounds = tp.max_rounds;
    return DL_OK;
}

size_t dl_mix_trace_workspace_bytes(int32_t n_rows, int32_t rounds) {
    if (n_rows <= 0 || rounds <= 0) return 0;
    return align_up((size_t)device_cus() * (size_t)rounds * (size_t)n_rows * 4) + kAlign;
}

int dl_mix_rounds_trace(const dl_mix_args *args, int32_t rounds, float *trace, void *workspace,
                        size_t ws_bytes, dl_stream_t stream) {
    g_err.clear();
    int rc = check_mix_args(args);
    if (rc) return rc;
    if (!trace) return fail(DL_ERR_INVALID, "dl_mix_rounds_trace: trace is NULL");
    dl::Launches L;
    char err[dl::kErrLen];
    rc = dl::shape_trace(*args, rounds, device_cus(), dl::read_knobs(), workspace, ws_bytes, &L,
                         err);
    if (rc) return status(rc, err);
    return run(L, nullptr, nullptr, trace, "", static_cast<hipStream_t>(stream));
}

int dl_mix_rounds_plan(const dl_mix_args *args, dl_mix_plan *plan) {
    g_err.clear();
    if (!plan) return fail(DL_ERR_INVALID, "dl_mix_rounds_plan: plan is NULL");
    int rc = check_mix_args(args);
    if (rc) return rc;
    Plan pl;
    rc = plan_rounds(args, &pl);
    if (rc) return rc;
    *plan = pl.pub;
    return DL_OK;
}

int dl_mix_rounds(const dl_mix_args *args, int32_t rounds, void *workspace, size_t ws_bytes,
                  dl_stream_t stream) {
    g_err.clear();
    int rc = check_mix_args(args);
    if (rc) return rc;
    dl::Launches L;
    char err[dl::kErrLen];
    rc = dl::shape_rounds(*args, rounds, device_cus(), dl::read_knobs(), workspace, ws_bytes, &L,
                          err);
    if (rc) return status(rc, err);
    return run(L, args->dev_sq, args->dev_max, nullptr, "", static_cast<hipStream_t>(stream));
}

int dl_mix_until_fits(int32_t n_rows, int64_t n_params, int32_t nnz) {
    if (n_rows <= 0 || n_params <= 0 || nnz < 0) return 0;
    return dl::until_lds_bytes(n_rows, n_params, nnz) <= dl::kLdsBytes ? 1 : 0;
}

int dl_mix_until(const dl_mix_until_args *a, dl_stream_t stream) {
    g_err.clear();
    if (!a) return fail(DL_ERR_INVALID, "dl_mix_until: args is NULL");
    const dl_csr &W = a->W;
    if (W.n_rows <= 0 || a->n_params <= 0 || W.nnz < 0)
        return fail(DL_ERR_INVALID, "dl_mix_until: n_rows, n_params must be > 0, nnz >= 0");
    if (!a->x || !a->y || !a->status || !W.row_ptr || (W.nnz > 0 && (!W.col || !W.w)))
        return fail(DL_ERR_INVALID, "dl_mix_until: null x/y/status/row_ptr/col/w");
    if (a->ldx < a->n_params || a->ldy < a->n_params)
        return fail(DL_ERR_INVALID, "dl_mix_until: ldx/ldy smaller than n_params");
    if (a->times < 0 || a->max_rounds < 1)
        return fail(DL_ERR_INVALID, "dl_mix_until: times must be >= 0 and max_rounds >= 1");
    if (W.uniform_row_nnz < 0 ||
        (W.uniform_row_nnz > 0 && (int64_t)W.uniform_row_nnz * W.n_rows != W.nnz))
        return fail(DL_ERR_INVALID, "dl_mix_until: uniform_row_nnz * n_rows != nnz");
    const size_t xb = ((size_t)(W.n_rows - 1) * a->ldx + a->n_params) * 4;
    const size_t yb = ((size_t)(W.n_rows - 1) * a->ldy + a->n_params) * 4;
    if (!(a->x == a->y && a->ldx == a->ldy) && overlaps(a->x, xb, a->y, yb))
        return fail(DL_ERR_INVALID, "dl_mix_until: y overlaps x (in place needs y == x, ldy == ldx)");
    if (!dl_mix_until_fits(W.n_rows, a->n_params, W.nnz))
        return fail(DL_ERR_UNSUPPORTED, "dl_mix_until: %d agents x %lld parameters (%lld bytes of "
                                        "LDS) do not fit one workgroup", W.n_rows,
                    (long long)a->n_params,
                    (long long)dl::until_lds_bytes(W.n_rows, a->n_params, W.nnz));
    dl::UntilArgs u{};
    u.x = a->x;
    u.ldx = a->ldx;
    u.y = a->y;
    u.ldy = a->ldy;
    u.n_params = a->n_params;
    u.chunks = (int32_t)((a->n_params + 3) / 4);
    u.n_rows = W.n_rows;
    u.nnz = W.nnz;
    u.rowptr = W.row_ptr;
    u.col = W.col;
    u.w = W.w;
    u.times = a->times;
    u.use_eps = a->use_eps ? 1 : 0;
    u.eps = a->eps;
    u.max_rounds = a->max_rounds;
    u.status = a->status;
    u.dev_trace = a->use_eps ? a->dev_trace : nullptr;
    hipError_t e = dl::launch_mix_until(u, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "mix_until_kernel launch");
}

int dl_consensus_gd(const dl_consensus_gd_args *a, int32_t total_rows, dl_stream_t stream) {
    g_err.clear();
    if (!a) return fail(DL_ERR_INVALID, "dl_consensus_gd: args is NULL");
    if (!a->X || !a->y || !a->shard_ptr || !a->row_ptr || !a->steps || !a->w)
        return fail(DL_ERR_INVALID, "dl_consensus_gd: null X/y/shard_ptr/row_ptr/steps/w");
    if (a->n_agents <= 0 || a->n_features <= 0 || a->n_features > 16 || total_rows <= 0 ||
        a->iterations < 0 || a->max_iter < 1)
        return fail(DL_ERR_INVALID, "dl_consensus_gd: need n_agents > 0, 0 < n_features <= 16, "
                                    "rows > 0, iterations >= 0, max_iter >= 1");
    if (!(a->mean_weight > 0.0))
        return fail(DL_ERR_INVALID, "dl_consensus_gd: mean_weight must be > 0");
    int64_t x_off = 0;
    bool in_lds = dl::gd_lds_bytes(a->n_agents, a->n_features, total_rows, true, &x_off) <=
                  dl::kLdsBytes;
    const int64_t lds = dl::gd_lds_bytes(a->n_agents, a->n_features, total_rows, in_lds, &x_off);
    if (lds > dl::kLdsBytes)
        return fail(DL_ERR_UNSUPPORTED, "dl_consensus_gd: %d agents x %d features do not fit LDS",
                    a->n_agents, a->n_features);
    if (a->iterations == 0) return DL_OK;
    dl::GdArgs g{};
    g.X = a->X;
    g.y = a->y;
    g.shard_ptr = a->shard_ptr;
    g.n_agents = a->n_agents;
    g.n_features = a->n_features;
    g.rowptr = a->row_ptr;
    g.col = a->col;
    g.eps = a->eps;
    g.conv_eps = a->conv_eps;
    g.mean_weight = a->mean_weight;
    g.tau = a->tau;
    g.steps = a->steps;
    g.iterations = a->iterations;
    g.max_iter = a->max_iter;
    g.w = a->w;
    g.iters_out = a->iters_out;
    g.x_in_lds = in_lds ? 1 : 0;
    g.x_off = x_off;
    hipError_t e = dl::launch_consensus_gd(g, (int)lds, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "consensus_gd_kernel launch");
}

const char *dl_last_error(void) { return g_err.c_str(); }

size_t dl_mix_workspace_bytes(int32_t n_rows, int32_t n_halo, int64_t n_params) {
    (void)n_halo;
    if (n_rows < 0 || n_params < 0) return 0;
    const size_t parts = (size_t)dl::max_parts(device_cus(), dl::read_knobs());
    return align_up(parts * (size_t)n_rows * 4) + align_up((size_t)n_params * 4) + kAlign;
}

int dl_mix_plan_query(const dl_mix_args *args, dl_mix_plan *plan) {
    g_err.clear();
    int rc = check_mix_args(args);
    if (rc) return rc;
    if (!plan) return fail(DL_ERR_INVALID, "dl_mix_plan_query: plan is NULL");
    Plan pl;
    rc = plan_mix(args, &pl);
    if (rc) return rc;
    *plan = pl.pub;
    return DL_OK;
}

int dl_mix_rounds_plan_shape(int32_t n_rows, int64_t n_params, int32_t nnz,
                             int32_t uniform_row_nnz, int32_t shared_row_weights,
                             int32_t doubly_stochastic, int32_t deviation, int32_t tile_cols,
                             dl_mix_plan *plan) {
    g_err.clear();
    if (!plan || n_rows <= 0 || n_params <= 0 || nnz < 0 || tile_cols < 0)
        return fail(DL_ERR_INVALID, "dl_mix_rounds_plan_shape: bad arguments");
    dl_mix_args a{};
    a.W.n_rows = n_rows;
    a.W.nnz = nnz;
    a.W.uniform_row_nnz = uniform_row_nnz;
    a.W.shared_row_weights = uniform_row_nnz > 0 ? shared_row_weights : 0;
    a.W.doubly_stochastic = doubly_stochastic;
    a.n_params = n_params;
    a.tile_cols = tile_cols;
    float dummy;
    if (deviation) a.dev_max = &dummy;
    Plan pl;
    const int rc = plan_rounds(&a, &pl);
    if (rc) return rc;
    *plan = pl.pub;
    return DL_OK;
}

namespace {
int plan_from_csr(const dl_csr &W, int32_t n_halo, int64_t n_params, int32_t deviation,
                  int32_t tile_cols, dl_mix_plan *plan, const char *who) {
    if (!plan || W.n_rows <= 0 || n_halo < 0 || n_params <= 0 || W.nnz < 0 || tile_cols < -1 ||
        W.min_row_nnz < 0)
        return fail(DL_ERR_INVALID, "%s: bad arguments", who);
    dl_mix_args a{};
    a.W = W;
    a.W.shared_row_weights = W.uniform_row_nnz > 0 ? W.shared_row_weights : 0;
    a.n_halo = n_halo;
    a.n_params = n_params;
    float dummy;
    if (deviation) a.dev_max = &dummy;
    const dl::Knobs k = dl::read_knobs();
    // -1: pick the column-tiled width (a tile of every source row in LDS)
    a.tile_cols = tile_cols == -1 ? dl::choose_tile_cols(a.W, n_halo, n_params, deviation != 0, k)
                                  : tile_cols;
    Plan pl;
    int rc = plan_with(dl::plan_mix, &a, k, &pl);
    if (rc) return rc;
    *plan = pl.pub;
    return DL_OK;
}
}  // namespace

int dl_mix_plan_shape(int32_t n_rows, int32_t n_halo, int64_t n_params, int32_t nnz,
                      int32_t uniform_row_nnz, int32_t shared_row_weights, int32_t deviation,
                      int32_t tile_cols, dl_mix_plan *plan) {
    g_err.clear();
    dl_csr W{};
    W.n_rows = n_rows;
    W.nnz = nnz;
    W.uniform_row_nnz = uniform_row_nnz;
    W.shared_row_weights = shared_row_weights;
    W.min_row_nnz = uniform_row_nnz > 0 ? uniform_row_nnz : 0;
    return plan_from_csr(W, n_halo, n_params, deviation, tile_cols, plan, "dl_mix_plan_shape");
}

int dl_mix_plan_csr(const dl_csr *W, int32_t n_halo, int64_t n_params, int32_t deviation,
                    int32_t tile_cols, dl_mix_plan *plan) {
    g_err.clear();
    if (!W) return fail(DL_ERR_INVALID, "dl_mix_plan_csr: W is NULL");
    return plan_from_csr(*W, n_halo, n_params, deviation, tile_cols, plan, "dl_mix_plan_csr");
}

int dl_mix_round(const dl_mix_args *args, void *workspace, size_t ws_bytes, dl_stream_t stream) {
    g_err.clear();
    int rc = check_mix_args(args);
    if (rc) return rc;
    if (args->partial_rows_out) *args->partial_rows_out = 0;
    dl::Launches L;
    char err[dl::kErrLen];
    rc = dl::shape_round(*args, device_cus(), dl::read_knobs(), workspace, ws_bytes, &L, err);
    if (rc) return status(rc, err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = run(L, args->dev_sq, args->dev_max, nullptr, "mix_tile_kernel", s);
    if (rc) return rc;
    if (L.after == dl::kAfterPartialRows) *args->partial_rows_out = L.parts;
    if (L.after == dl::kAfterTwoPass)
        return deviation_two_pass(args->y, args->ldy, args->W.n_rows, args->n_params, nullptr,
                                  args->dev_sq, args->dev_max, args->mean,
                                  static_cast<char *>(workspace), ws_bytes, s);
    return DL_OK;
}

size_t dl_deviation_workspace_bytes(int32_t n_rows, int64_t n_params) {
    return dl_mix_workspace_bytes(n_rows, 0, n_params);
}

int dl_deviation(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params,
                 const float *mean_in, float *dev_sq, float *dev_max, float *mean_out,
                 void *workspace, size_t ws_bytes, dl_stream_t stream) {
    g_err.clear();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x || n_rows <= 0 || n_params <= 0 || ldx < n_params)
        return fail(DL_ERR_INVALID, "dl_deviation: bad x/n_rows/n_params/ldx");
    char *ws = static_cast<char *>(workspace);
    if (!dl::ws_holds(ws, ws_bytes, 0))
        return fail(DL_ERR_WORKSPACE, "dl_deviation: needs a 16-byte aligned workspace");
    if (n_rows <= 1) {
        if (mean_out) {
            hipError_t e = mean_in ? hipMemcpyAsync(mean_out, mean_in, (size_t)n_params * 4,
                                                    hipMemcpyDeviceToDevice, s)
                                   : hipMemcpy2DAsync(mean_out, (size_t)n_params * 4, x,
                                                      (size_t)ldx * 4, (size_t)n_params * 4, 1,
                                                      hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "dl_deviation mean copy");
        }
        return zero_deviation(n_rows, dev_sq, dev_max, s);
    }
    if (!mean_in) {
        int rc = deviation_one_pass(x, ldx, 0, n_rows, n_params, dev_sq, dev_max, mean_out, ws,
                                    ws_bytes, s);
        if (rc != DL_ERR_UNSUPPORTED) return rc;
    }
    return deviation_two_pass(x, ldx, n_rows, n_params, mean_in, dev_sq, dev_max, mean_out, ws,
                              ws_bytes, s);
}

int dl_deviation_tiled(const float *x, int32_t n_rows, int64_t n_params, int32_t tile_cols,
                       float *dev_sq, float *dev_max, float *mean_out, void *workspace,
                       size_t ws_bytes, dl_stream_t stream) {
    g_err.clear();
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!x || n_rows <= 0 || n_params <= 0 || tile_cols < 4 || tile_cols > 4 * dl::kMaxChunks ||
        (tile_cols & (tile_cols - 1)))
        return fail(DL_ERR_INVALID, "dl_deviation_tiled: bad x/n_rows/n_params/tile_cols");
    char *ws = static_cast<char *>(workspace);
    if (!dl::ws_holds(ws, ws_bytes, 0))
        return fail(DL_ERR_WORKSPACE, "dl_deviation_tiled: needs a 16-byte aligned workspace");
    if (n_rows <= 1) {
        if (mean_out) {
            hipError_t e = dl::launch_tile_convert(x, mean_out, n_params, 1, n_params, tile_cols,
                                                   false, s);
            if (e != hipSuccess) return hip_fail(e, "dl_deviation_tiled mean copy");
        }
        return zero_deviation(n_rows, dev_sq, dev_max, s);
    }
    int rc = deviation_one_pass(x, 0, tile_cols, n_rows, n_params, dev_sq, dev_max, mean_out, ws,
                                ws_bytes, s);
    if (rc == DL_ERR_UNSUPPORTED)
        return fail(DL_ERR_UNSUPPORTED, "dl_deviation_tiled: %d rows exceed one tile", n_rows);
    return rc;
}

int dl_to_tiled(const float *src, int64_t ld, int32_t n_rows, int64_t n_params, int32_t tile_cols,
                float *dst, dl_stream_t stream) {
    g_err.clear();
    if (!src || !dst || n_rows <= 0 || n_params <= 0 || ld < n_params || tile_cols <= 0)
        return fail(DL_ERR_INVALID, "dl_to_tiled: bad arguments");
    hipError_t e = dl::launch_tile_convert(src, dst, ld, n_rows, n_params, tile_cols, true,
                                           static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "tile_convert launch");
}

int dl_from_tiled(const float *src, int32_t n_rows, int64_t n_params, int32_t tile_cols, float *dst,
                  int64_t ld, dl_stream_t stream) {
    g_err.clear();
    if (!src || !dst || n_rows <= 0 || n_params <= 0 || ld < n_params || tile_cols <= 0)
        return fail(DL_ERR_INVALID, "dl_from_tiled: bad arguments");
    hipError_t e = dl::launch_tile_convert(src, dst, ld, n_rows, n_params, tile_cols, false,
                                           static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "tile_convert launch");
}

int dl_column_sum(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params, float *colsum,
                  dl_stream_t stream) {
    g_err.clear();
    if (!x || !colsum || n_rows <= 0 || n_params <= 0 || ldx < n_params)
        return fail(DL_ERR_INVALID, "dl_column_sum: bad arguments");
    hipError_t e = dl::launch_column_sum(x, ldx, n_rows, n_params, colsum, 0.f,
                                         static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "column_sum launch");
}

int dl_row_sums(const float *parts, int32_t n_parts, int32_t n_rows, float *sums, float *max_sqrt,
                int32_t max_zeroed, dl_stream_t stream) {
    g_err.clear();
    if (!parts || n_parts <= 0 || n_rows <= 0 || (!sums && !max_sqrt))
        return fail(DL_ERR_INVALID, "dl_row_sums: bad arguments");
    hipError_t e = dl::launch_dev_reduce(parts, n_parts, n_rows, sums, max_sqrt,
                                         static_cast<hipStream_t>(stream), max_zeroed != 0);
    return e == hipSuccess ? DL_OK : hip_fail(e, "dev_reduce launch");
}

int dl_max_column_std(const float *x, int64_t ldx, int32_t n_rows, int64_t n_params, float *out,
                      dl_stream_t stream) {
    g_err.clear();
    if (!x || !out || n_rows <= 0 || n_params <= 0 || ldx < n_params)
        return fail(DL_ERR_INVALID, "dl_max_column_std: bad arguments");
    hipError_t e = dl::launch_max_column_std(x, ldx, n_rows, n_params, out,
                                             static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "max_column_std launch");
}

int dl_step_rows(const float *x, int64_t ldx, const float *g, int64_t ldg, float lr,
                 const int32_t *rows, int32_t n_sel, int64_t n_params, float *out, int64_t ldo,
                 dl_stream_t stream) {
    g_err.clear();
    if (n_sel == 0) return DL_OK;
    if (!x || !rows || !out || n_sel < 0 || n_sel > 65535 || n_params <= 0 || ldx < n_params ||
        ldo < n_params || (g && ldg < n_params))
        return fail(DL_ERR_INVALID, "dl_step_rows: bad arguments");
    hipError_t e = dl::launch_step_rows(x, ldx, g, ldg, lr, rows, n_sel, n_params, out, ldo,
                                        static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "step_rows launch");
}

namespace {
int step_rows_tiled_peers(const float *x, int32_t x_rows, const float *g, int32_t g_rows, float lr,
                          const int32_t *rows, int32_t n_peers, const int32_t *row0,
                          float *const *outs, int64_t n_params, int32_t tile_cols,
                          dl_stream_t stream, const char *who) {
    if (!x || !rows || !row0 || !outs || n_peers < 1 || n_peers > dl::kMaxPackPeers ||
        n_params <= 0 || x_rows <= 0 || (g && g_rows <= 0) || tile_cols < 4 ||
        tile_cols > 4 * dl::kMaxChunks || (tile_cols & (tile_cols - 1)))
        return fail(DL_ERR_INVALID, "%s: bad arguments", who);
    if (!aligned16(x) || (g && !aligned16(g)))
        return fail(DL_ERR_INVALID, "%s: operands must be 16-byte aligned", who);
    const int64_t n_tiles = (n_params + tile_cols - 1) / tile_cols;
    dl::PackPeers pp{};
    pp.n = n_peers;
    if (row0[0] != 0) return fail(DL_ERR_INVALID, "%s: row0[0] must be 0", who);
    for (int b = 0; b < n_peers; ++b) {
        const int32_t nb = row0[b + 1] - row0[b];
        if (nb < 0 || row0[b + 1] > 65535)
            return fail(DL_ERR_INVALID, "%s: row0 must be non-decreasing, <= 65535", who);
        if (nb > 0 && (!outs[b] || !aligned16(outs[b])))
            return fail(DL_ERR_INVALID, "%s: out[%d] must be a 16-byte aligned pointer", who, b);
        const size_t ob = (size_t)n_tiles * nb * tile_cols * 4;
        if (nb > 0 && (overlaps(outs[b], ob, x, (size_t)n_tiles * x_rows * tile_cols * 4) ||
                       (g && overlaps(outs[b], ob, g, (size_t)n_tiles * g_rows * tile_cols * 4))))
            return fail(DL_ERR_INVALID, "%s: out[%d] overlaps x or g", who, b);
        pp.row0[b] = row0[b];
        pp.out[b] = reinterpret_cast<float4 *>(outs[b]);
    }
    pp.row0[n_peers] = row0[n_peers];
    if (row0[n_peers] == 0) return DL_OK;
    hipError_t e = dl::launch_step_rows_tiled(x, x_rows, g, g_rows, lr, rows, pp, n_tiles,
                                              tile_cols, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "step_rows_tiled launch");
}
}  // namespace

int dl_step_rows_tiled(const float *x, int32_t x_rows, const float *g, int32_t g_rows, float lr,
                       const int32_t *rows, int32_t n_sel, int64_t n_params, int32_t tile_cols,
                       float *out, dl_stream_t stream) {
    g_err.clear();
    if (n_sel == 0) return DL_OK;
    if (n_sel < 0 || n_sel > 65535 || !out)
        return fail(DL_ERR_INVALID, "dl_step_rows_tiled: bad arguments");
    const int32_t row0[2] = {0, n_sel};
    float *outs[1] = {out};
    return step_rows_tiled_peers(x, x_rows, g, g_rows, lr, rows, 1, row0, outs, n_params,
                                 tile_cols, stream, "dl_step_rows_tiled");
}

int dl_step_rows_tiled_peers(const float *x, int32_t x_rows, const float *g, int32_t g_rows,
                             float lr, const int32_t *rows, int32_t n_peers, const int32_t *row0,
                             float *const *outs, int64_t n_params, int32_t tile_cols,
                             dl_stream_t stream) {
    g_err.clear();
    return step_rows_tiled_peers(x, x_rows, g, g_rows, lr, rows, n_peers, row0, outs, n_params,
                                 tile_cols, stream, "dl_step_rows_tiled_peers");
}

int dl_sgd_step(const dl_sgd_args *a, dl_stream_t stream) {
    g_err.clear();
    if (!a) return fail(DL_ERR_INVALID, "dl_sgd_step: null args");
    if (a->n_rows == 0 || a->n_params == 0) return DL_OK;
    if (!a->x || !a->g || !a->out || a->n_rows < 0 || a->n_rows > 65535 || a->n_params < 0 ||
        a->ldx < a->n_params || a->ldg < a->n_params || a->ldo < a->n_params)
        return fail(DL_ERR_INVALID, "dl_sgd_step: bad arguments (n_rows %d, n_params %lld)",
                    a->n_rows, (long long)a->n_params);
    if (a->momentum != 0.f && (!a->buf || a->ldb < a->n_params))
        return fail(DL_ERR_INVALID, "dl_sgd_step: momentum needs a buffer [n_rows, ldb >= n_params]");
    if (a->nesterov && (a->momentum <= 0.f || a->dampening != 0.f))
        return fail(DL_ERR_INVALID, "dl_sgd_step: Nesterov momentum requires a momentum and zero "
                                    "dampening");
    const size_t rb = (size_t)a->n_params * sizeof(float);
    if (a->out != a->x && overlaps(a->out, ((size_t)a->n_rows - 1) * a->ldo * 4 + rb, a->x,
                                   ((size_t)a->n_rows - 1) * a->ldx * 4 + rb))
        return fail(DL_ERR_INVALID, "dl_sgd_step: out must be x itself or not overlap it");
    float *buf = a->momentum != 0.f ? a->buf : nullptr;
    const bool vec = aligned16(a->x) && aligned16(a->g) && aligned16(a->out) &&
                     (!buf || aligned16(buf)) && (a->n_params & 3) == 0 && (a->ldx & 3) == 0 &&
                     (a->ldg & 3) == 0 && (a->ldo & 3) == 0 && (!buf || (a->ldb & 3) == 0);
    hipError_t e = dl::launch_sgd_step(a->x, a->ldx, a->g, a->ldg, buf, a->ldb, a->out, a->ldo,
                                       a->n_rows, a->n_params, a->lr, a->momentum, a->dampening,
                                       a->weight_decay, a->first ? 1 : 0, a->nesterov ? 1 : 0,
                                       vec, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "sgd_step launch");
}

int dl_sgd_round_plan(const dl_sgd_round_args *args, dl_mix_plan *plan) {
    return fused_round_plan(dl::shape_sgd_round, args, plan);
}

int dl_sgd_round(const dl_sgd_round_args *args, void *workspace, size_t ws_bytes,
                 dl_stream_t stream) {
    return fused_round(dl::shape_sgd_round, "mix_sgd_tile_kernel", args, workspace, ws_bytes,
                       stream);
}

int dl_cheb_round_plan(const dl_cheb_round_args *args, dl_mix_plan *plan) {
    return fused_round_plan(dl::shape_cheb_round, args, plan);
}

int dl_cheb_round(const dl_cheb_round_args *args, void *workspace, size_t ws_bytes,
                  dl_stream_t stream) {
    return fused_round(dl::shape_cheb_round, "mix_cheb_tile_kernel", args, workspace, ws_bytes,
                       stream);
}

int dl_track_round_plan(const dl_track_round_args *args, dl_mix_plan *plan) {
    return fused_round_plan(dl::shape_track_round, args, plan);
}

int dl_track_round(const dl_track_round_args *args, void *workspace, size_t ws_bytes,
                   dl_stream_t stream) {
    return fused_round(dl::shape_track_round, "mix_track_tile_kernel", args, workspace, ws_bytes,
                       stream);
}

int dl_adam_step(const dl_adam_args *a, dl_stream_t stream) {
    g_err.clear();
    if (!a) return fail(DL_ERR_INVALID, "dl_adam_step: null args");
    if (a->n_rows == 0 || a->n_params == 0) return DL_OK;
    if (!a->x || !a->g || !a->m || !a->v || !a->out || a->n_rows < 0 || a->n_rows > 65535 ||
        a->n_params < 0 || a->ldx < a->n_params || a->ldg < a->n_params ||
        a->ldm < a->n_params || a->ldv < a->n_params || a->ldo < a->n_params)
        return fail(DL_ERR_INVALID, "dl_adam_step: bad arguments (n_rows %d, n_params %lld)",
                    a->n_rows, (long long)a->n_params);
    char err[dl::kErrLen];
    const int rc = dl::check_adam_params("dl_adam_step", a->beta1, a->beta2, a->eps, a->step_size,
                                         a->bias2_sqrt, a->coef, err);
    if (rc) return status(rc, err);
    const size_t rb = (size_t)a->n_params * sizeof(float);
    auto span = [&](int64_t ld) { return ((size_t)a->n_rows - 1) * ld * 4 + rb; };
    if (a->out != a->x && overlaps(a->out, span(a->ldo), a->x, span(a->ldx)))
        return fail(DL_ERR_INVALID, "dl_adam_step: out must be x itself or not overlap it");
    // m and v are read and written in place: neither shares a byte with anything else
    const struct { const void *p; int64_t ld; const char *name; } mv[] = {{a->m, a->ldm, "m"},
                                                                          {a->v, a->ldv, "v"}},
        other[] = {{a->x, a->ldx, "x"}, {a->g, a->ldg, "g"}, {a->out, a->ldo, "out"}};
    for (const auto &o : mv)
        for (const auto &i : other)
            if (overlaps(o.p, span(o.ld), i.p, span(i.ld)))
                return fail(DL_ERR_INVALID, "dl_adam_step: %s overlaps %s", o.name, i.name);
    if (overlaps(a->m, span(a->ldm), a->v, span(a->ldv)))
        return fail(DL_ERR_INVALID, "dl_adam_step: m overlaps v");
    const bool vec = aligned16(a->x) && aligned16(a->g) && aligned16(a->out) && aligned16(a->m) &&
                     aligned16(a->v) && (a->n_params & 3) == 0 && (a->ldx & 3) == 0 &&
                     (a->ldg & 3) == 0 && (a->ldo & 3) == 0 && (a->ldm & 3) == 0 &&
                     (a->ldv & 3) == 0;
    const dl::AdamParams p = dl::adam_params(a->beta1, a->beta2, a->eps, a->lr, a->weight_decay,
                                             a->decoupled, a->step_size, a->bias2_sqrt, a->coef);
    hipError_t e = dl::launch_adam_step(a->x, a->ldx, a->g, a->ldg, a->m, a->ldm, a->v, a->ldv,
                                        a->out, a->ldo, a->n_rows, a->n_params, p, vec,
                                        static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "adam_step launch");
}

int dl_adam_tick(double *state, dl_stream_t stream) {
    g_err.clear();
    if (!state || (reinterpret_cast<uintptr_t>(state) & 7u))
        return fail(DL_ERR_INVALID, "dl_adam_tick: state must be an 8-byte aligned device "
                                    "double[DL_ADAM_STATE_LEN]");
    hipError_t e = dl::launch_adam_tick(state, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "adam_tick launch");
}

int dl_adam_round_plan(const dl_adam_round_args *args, dl_mix_plan *plan) {
    return fused_round_plan(dl::shape_adam_round, args, plan);
}

int dl_adam_round(const dl_adam_round_args *args, void *workspace, size_t ws_bytes,
                  dl_stream_t stream) {
    return fused_round(dl::shape_adam_round, "mix_adam_tile_kernel", args, workspace, ws_bytes,
                       stream);
}

int dl_axpby(const float *s, int64_t lds_, const float *z, int64_t ldz, float a, float b,
             float *out, int64_t ldo, int32_t n_rows, int64_t n_params, dl_stream_t stream) {
    g_err.clear();
    if (n_rows == 0 || n_params == 0) return DL_OK;
    if (!s || !z || !out || n_rows < 0 || n_rows > 65535 || n_params < 0 || lds_ < n_params ||
        ldz < n_params || ldo < n_params)
        return fail(DL_ERR_INVALID, "dl_axpby: bad arguments (n_rows %d, n_params %lld)", n_rows,
                    (long long)n_params);
    const size_t rb = (size_t)n_params * sizeof(float);
    auto extent = [&](int64_t ld) { return ((size_t)n_rows - 1) * ld * 4 + rb; };
    if (!(out == s && ldo == lds_) && overlaps(out, extent(ldo), s, extent(lds_)))
        return fail(DL_ERR_INVALID, "dl_axpby: out must be s itself or not overlap it");
    if (!(out == z && ldo == ldz) && overlaps(out, extent(ldo), z, extent(ldz)))
        return fail(DL_ERR_INVALID, "dl_axpby: out must be z itself or not overlap it");
    const bool vec = aligned16(s) && aligned16(z) && aligned16(out) && (lds_ & 3) == 0 &&
                     (ldz & 3) == 0 && (ldo & 3) == 0;
    hipError_t e = dl::launch_axpby(s, lds_, z, ldz, a, b, out, ldo, n_rows, n_params, vec,
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "axpby launch");
}

size_t dl_mlp_workspace_bytes(int32_t n_agents) {
    return n_agents > 0 ? dl::mlp_workspace_floats(n_agents) * sizeof(float) : 0;
}

int dl_mlp_grad(const dl_mlp_args *a, dl_stream_t stream) {
    g_err.clear();
    char err[dl::kErrLen];
    const int rc = dl::shape_mlp_grad(a, err);
    if (rc) return status(rc, err);
    if (a->n_agents == 0) return DL_OK;
    hipError_t e = dl::launch_mlp_fused(a->X, a->ldx, a->data, a->s_data, a->labels, a->s_labels,
                                        a->G, a->ldg, a->loss, a->n_agents, a->input_dim,
                                        a->hidden_dim, a->output_dim, a->tile_cols,
                                        a->out_mode == 1, a->lr, a->workspace,
                                        static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "mlp_fused launch");
}

size_t dl_mlp_eval_workspace_bytes(int32_t n_agents, int32_t rows) {
    return dl::eval_workspace_bytes(n_agents, rows);
}

int dl_mlp_eval_plan_query(const dl_mlp_eval_args *a, dl_mlp_eval_plan *plan) {
    g_err.clear();
    char err[dl::kErrLen];
    int rc = dl::shape_mlp_eval(a, device_cus(), nullptr, 0, false, plan, err);
    if (rc) return status(rc, err);
    if (!plan) return fail(DL_ERR_INVALID, "dl_mlp_eval_plan_query: plan is NULL");
    return DL_OK;
}

int dl_mlp_eval(const dl_mlp_eval_args *a, void *workspace, size_t ws_bytes, dl_stream_t stream) {
    g_err.clear();
    char err[dl::kErrLen];
    dl_mlp_eval_plan pl;
    int rc = dl::shape_mlp_eval(a, device_cus(), workspace, ws_bytes, true, &pl, err);
    if (rc) return status(rc, err);
    int tsh = 0;
    while (a->tile_cols > 0 && (1 << tsh) < a->tile_cols) ++tsh;
    float *part = static_cast<float *>(workspace);
    int32_t *hit = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) +
                                               dl::eval_part_bytes(a->n_agents, a->rows));
    const dl::MlpEvalArgs p{a->X, a->ldx, a->data, a->s_data, a->labels, a->s_labels, part, hit,
                            a->logits, a->ldz, a->s_logits, a->rows, pl.blocks, pl.row_splits,
                            a->input_dim, a->hidden_dim, a->output_dim, tsh,
                            (int64_t)a->n_agents * a->tile_cols};
    hipError_t e = dl::launch_mlp_eval(p, a->n_agents, a->loss, a->correct,
                                       static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "mlp_eval launch");
}

int dl_batch_gather(const dl_batch_gather_args *a, dl_stream_t stream) {
    g_err.clear();
    char err[dl::kErrLen];
    dl::BatchGatherPlan pl;
    int rc = dl::shape_batch_gather(a, device_cus(), &pl, err);
    if (rc) return status(rc, err);
    hipError_t e = dl::launch_batch_gather(pl, a->advance ? a->cursor : nullptr,
                                           static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "batch_gather launch");
}

int dl_image_batch(const dl_image_batch_args *a, dl_stream_t stream) {
    g_err.clear();
    char err[dl::kErrLen];
    dl::ImageBatchPlan pl;
    int rc = dl::shape_image_batch(a, device_cus(), &pl, err);
    if (rc) return status(rc, err);
    hipError_t e = dl::launch_image_batch(pl, a->advance ? a->cursor : nullptr,
                                          static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "image_batch launch");
}

int32_t dl_lenet_param_count(int32_t num_classes) { return dl::lenet_param_count(num_classes); }

size_t dl_lenet_workspace_bytes(int32_t n_agents, int32_t batch, int32_t num_classes) {
    return dl::lenet_workspace(n_agents, batch, num_classes).total;
}

namespace {
hipError_t lenet_launch(const dl::LenetPlan &pl, const dl::LenetStep &st, hipStream_t s) {
    const dl::XentArgs &h = st.head;
    switch (st.kind) {
        case dl::kLenetConvFwd: return dl::launch_lenet_conv_fwd(pl.conv, pl.fwd_grid, s);
        case dl::kLenetGemm: return dl::launch_bgemm(st.gemm, s);
        case dl::kLenetHead:
            return dl::launch_xent_grad(h.Z, h.sZ, h.y, h.sY, h.dZ, h.sD, h.loss, h.batch, h.rows,
                                        h.classes, s);
        case dl::kLenetConvBwd: return dl::launch_lenet_conv_bwd(pl.conv, pl.bwd_grid, s);
        case dl::kLenetConvReduce: return dl::launch_lenet_conv_reduce(pl.conv, pl.n_agents, s);
    }
    return hipErrorInvalidValue;
}

// dl_lenet_grad's launches as shape_lenet lists them; with events, one recorded before each and
// one after the last.  After a failure nothing more is launched or recorded.
int lenet_run(const dl_lenet_args *a, void *workspace, size_t ws_bytes, hipStream_t s,
              void *const *events, int32_t n_events, int32_t *n_launches) {
    g_err.clear();
    char err[dl::kErrLen];
    dl::LenetPlan pl;
    int rc = dl::shape_lenet(a, device_cus(), workspace, ws_bytes, &pl, err);
    if (rc) return status(rc, err);
    if (n_launches) *n_launches = pl.n_launches;
    if (events && n_events < pl.n_launches + 1)
        return fail(DL_ERR_INVALID, "dl_lenet_grad_events: needs %d events (got %d)",
                    pl.n_launches + 1, n_events);
    hipError_t e = hipSuccess;
    for (int i = 0; e == hipSuccess && i <= pl.n_launches; ++i) {
        if (events) e = hipEventRecord(static_cast<hipEvent_t>(events[i]), s);
        if (e == hipSuccess && i < pl.n_launches) e = lenet_launch(pl, pl.step[i], s);
    }
    return e == hipSuccess ? DL_OK : hip_fail(e, "lenet launch");
}
}  // namespace

int dl_lenet_grad(const dl_lenet_args *a, void *workspace, size_t ws_bytes, dl_stream_t stream) {
    return lenet_run(a, workspace, ws_bytes, static_cast<hipStream_t>(stream), nullptr, 0,
                     nullptr);
}

int dl_lenet_grad_events(const dl_lenet_args *a, void *workspace, size_t ws_bytes,
                         dl_stream_t stream, void *const *events, int32_t n_events,
                         int32_t *n_launches) {
    if (!events) return fail(DL_ERR_INVALID, "dl_lenet_grad_events: events is NULL");
    return lenet_run(a, workspace, ws_bytes, static_cast<hipStream_t>(stream), events, n_events,
                     n_launches);
}

size_t dl_lenet_eval_workspace_bytes(int32_t n_agents, int32_t rows) {
    return dl::lenet_eval_workspace(n_agents, rows).total;
}

int dl_lenet_eval_plan_query(const dl_lenet_eval_args *a, dl_lenet_eval_plan *plan) {
    g_err.clear();
    char err[dl::kErrLen];
    int rc = dl::shape_lenet_eval(a, device_cus(), nullptr, 0, false, plan, err);
    if (rc) return status(rc, err);
    if (!plan) return fail(DL_ERR_INVALID, "dl_lenet_eval_plan_query: plan is NULL");
    return DL_OK;
}

int dl_lenet_eval(const dl_lenet_eval_args *a, void *workspace, size_t ws_bytes,
                  dl_stream_t stream) {
    g_err.clear();
    char err[dl::kErrLen];
    dl_lenet_eval_plan pl;
    int rc = dl::shape_lenet_eval(a, device_cus(), workspace, ws_bytes, true, &pl, err);
    if (rc) return status(rc, err);
    const dl::LenetEvalWs w = dl::lenet_eval_workspace(a->n_agents, a->rows);
    char *ws = static_cast<char *>(workspace);
    const dl::LenetEvalArgs p{a->X, a->ldx, a->data, a->s_data, a->labels, a->s_labels,
                              reinterpret_cast<float *>(ws + w.part),
                              reinterpret_cast<int32_t *>(ws + w.hit), a->logits, a->ldz,
                              a->s_logits, a->n_agents, a->rows, pl.blocks, pl.row_splits,
                              a->num_classes};
    hipError_t e = dl::launch_lenet_eval(p, pl.lds_bytes, a->loss, a->correct,
                                         static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "lenet_eval launch");
}

int dl_stream_copy(const float *src, float *dst, int64_t n_floats, int32_t variant,
                   dl_stream_t stream) {
    g_err.clear();
    if (!src || !dst || n_floats < 0 || (n_floats & 3) || !aligned16(src) || !aligned16(dst) ||
        variant < 0 || variant > 6 || (variant == 6 && n_floats % 16384))
        return fail(DL_ERR_INVALID, "dl_stream_copy: needs 16-byte aligned buffers, n %% 4 == 0, "
                                    "variant 0..6 (6: n %% 16384 == 0)");
    hipError_t e = dl::launch_stream_copy(src, dst, n_floats, variant,
                                          static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "stream_copy launch");
}

int dl_bgemm(const dl_bgemm_args *a, dl_stream_t stream) {
    g_err.clear();
    char err[dl::kErrLen];
    const int rc = dl::check_bgemm(a, err);
    if (rc) return status(rc, err);
    hipError_t e = dl::launch_bgemm(dl::bgemm_args(*a), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "bgemm launch");
}

int dl_xent_grad(const float *Z, int64_t sZ, const int32_t *y, int64_t sY, float *dZ, int64_t sD,
                 float *loss, int32_t batch, int32_t rows, int32_t classes, dl_stream_t stream) {
    g_err.clear();
    if (!Z || !y || !dZ || batch <= 0 || batch > 65535 || rows <= 0 || classes <= 0 ||
        classes > 64)
        return fail(DL_ERR_INVALID, "dl_xent_grad: bad arguments");
    if (batch > 1 && sD < (int64_t)rows * classes)
        return fail(DL_ERR_INVALID, "dl_xent_grad: output batch stride sD smaller than one batch "
                                    "(rows * classes)");
    hipError_t e = dl::launch_xent_grad(Z, sZ, y, sY, dZ, sD, loss, batch, rows, classes,
                                        static_cast<hipStream_t>(stream));
    return e == hipSuccess ? DL_OK : hip_fail(e, "xent_grad launch");
}

size_t dl_perron_workspace_bytes(int32_t dtype, int32_t n_rows, int64_t n_params) {
    const size_t sz = dtype == 1 ? 8 : 4;
    return align_up((size_t)n_rows * (size_t)n_params * sz) + kAlign;
}

int dl_perron_round(const dl_perron_args *a, void *workspace, size_t ws_bytes,
                    dl_stream_t stream) {
    g_err.clear();
    if (!a) return fail(DL_ERR_INVALID, "dl_perron_round: args is NULL");
    if (a->dtype != 0 && a->dtype != 1) return fail(DL_ERR_INVALID, "dl_perron_round: dtype");
    if (!a->y || !a->row_ptr || !a->iters_out || a->n_rows <= 0 || a->n_params <= 0 ||
        a->ldy < a->n_params || a->max_iter < 1)
        return fail(DL_ERR_INVALID, "dl_perron_round: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tp = dl::perron_tile_cols(a->dtype, a->n_rows, a->n_params);
    if (tp <= 0)
        return fail(DL_ERR_UNSUPPORTED, "dl_perron_round: %d rows do not fit one LDS column",
                    a->n_rows);
    dl::PerronArgs p{};
    p.y = a->y;
    p.ldy = a->ldy;
    p.n_rows = a->n_rows;
    p.n_params = a->n_params;
    p.rowptr = a->row_ptr;
    p.col = a->col;
    p.weight = a->weight;
    p.mean_weight = a->mean_weight;
    p.eps = a->eps;
    p.conv_eps = a->conv_eps;
    p.max_iter = a->max_iter;
    p.iters_out = a->iters_out;
    p.conv_rows = a->conv_eps_rows;
    if (tp == a->n_params) {
        hipError_t e = dl::launch_perron_single(p, a->dtype, tp, s);
        return e == hipSuccess ? DL_OK : hip_fail(e, "perron_single launch");
    }
    // multi-tile: one launch per iteration, host checks the not-converged flag (synchronises)
    const size_t sz = a->dtype == 1 ? 8 : 4;
    const size_t buf_b = align_up((size_t)a->n_rows * a->n_params * sz);
    if (!workspace || ws_bytes < buf_b + kAlign)
        return fail(DL_ERR_WORKSPACE, "dl_perron_round: workspace too small");
    char *ws = static_cast<char *>(workspace);
    p.ybuf = ws;
    p.notconv = reinterpret_cast<int32_t *>(ws + buf_b);
    void *bufs[2] = {a->y, p.ybuf};
    int it = 0, cur = 0;
    int32_t host_flag = 1;
    while (it < a->max_iter) {
        ++it;
        hipError_t e = hipMemsetAsync(p.notconv, 0, 4, s);
        if (e != hipSuccess) return hip_fail(e, "perron flag memset");
        e = dl::launch_perron_step(p, a->dtype, tp, bufs[cur], bufs[cur ^ 1], it == 1, s);
        if (e != hipSuccess) return hip_fail(e, "perron_step launch");
        cur ^= 1;
        e = hipMemcpyAsync(&host_flag, p.notconv, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "perron flag readback");
        if (host_flag == 0) break;
    }
    if (cur == 1) {
        hipError_t e = hipMemcpy2DAsync(a->y, (size_t)a->ldy * sz, p.ybuf, (size_t)a->n_params * sz,
                                        (size_t)a->n_params * sz, a->n_rows,
                                        hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "perron copy-back");
    }
    hipError_t e = hipMemcpyAsync(a->iters_out, &it, 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? DL_OK : hip_fail(e, "perron iters write");
}

}  // extern "C"
