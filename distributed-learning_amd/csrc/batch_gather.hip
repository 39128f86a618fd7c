// dl_batch_gather: every agent's next mini-batch gathered by sample id from a dataset resident in
// HBM (include/dlamd.h).  A copy: data[a][b][:] = samples[index[a][s * batch + b]][:], labels
// likewise, s the step inside the epoch read from a device cursor (or given by the host).
//
// Whole rows, float4 per lane, kGatherRowsInFlight rows in flight per wave, rows grid-strided over
// a grid shaped from the compute units (launch.h shape_batch_gather).  Two kernels:
//   wide   (dim >= 256 floats): one wave per destination row.  The sample id is made
//          wave-uniform, so the row base is scalar and a lane only adds its chunk offset.
//   packed (dim < 256): 2^lane_sh >= dim / 4 lanes share a row and a wave-instruction covers
//          64 >> lane_sh rows, so short rows leave few lanes idle; ids and bases are per lane.
// Plain loads and stores: the gradient kernel reads the batch straight afterwards and a batch
// fits the Infinity Cache.  The cursor is read by every workgroup as one uniform load and
// written only by the one-thread launch that follows on the stream.
#include "dl_internal.h"

namespace dl {
namespace {

constexpr int R = kGatherRowsInFlight;

// the step inside the epoch: wave-uniform, in [0, steps)
__device__ inline int epoch_step(const BatchGatherArgs &a) {
    if (!a.cursor) return a.step;   // normalised on the host
    int s = a.cursor[0] % a.steps;
    return s < 0 ? s + a.steps : s;
}

// the sample id of destination row r < rows, clamped into [0, n_samples); its agent and slot
__device__ inline int sample_id(const BatchGatherArgs &a, int64_t idx0, int r, int *ag, int *b) {
    *ag = r / a.batch;
    *b = r - *ag * a.batch;
    int id = a.index[(int64_t)*ag * a.s_index + idx0 + *b];
    id = id < 0 ? 0 : id;
    return id >= a.n_samples ? a.n_samples - 1 : id;
}

__device__ __forceinline__ float4 ld16(const char *p, uint32_t off) {
    return *reinterpret_cast<const float4 *>(p + off);
}
__device__ __forceinline__ void st16(char *p, uint32_t off, const float4 &v) {
    *reinterpret_cast<float4 *>(p + off) = v;
}

// The rows of a pass are named one by one (no arrays: the compiler moved a float4[R] to LDS).
static_assert(R == 4, "the kernels below spell out four rows in flight");

// row J of a wide pass, looked up by lane J: scalar source and destination row bases
struct WideRow {
    const char *src;
    char *dst;
};
template <int J>
__device__ __forceinline__ WideRow wide_row(const BatchGatherArgs &a, int id, int ag, int b) {
    const int64_t idj = __builtin_amdgcn_readlane(id, J);
    const int64_t agj = __builtin_amdgcn_readlane(ag, J);
    const int64_t bj = __builtin_amdgcn_readlane(b, J);
    return {reinterpret_cast<const char *>(a.samples + idj * a.ld_samples),
            reinterpret_cast<char *>(a.data + agj * a.s_data + bj * a.dim4 * 4)};
}

__global__ __launch_bounds__(kGatherThreads) void batch_gather_wide_kernel(
    const BatchGatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t stride = (int64_t)gridDim.x * (kGatherThreads / 64) * R;
    const int64_t idx0 = (int64_t)epoch_step(a) * a.batch;
    const uint32_t row_bytes = (uint32_t)a.dim4 * 16u;   // dim <= 2^28 (shape_batch_gather)
    for (int64_t r0 = ((int64_t)blockIdx.x * (kGatherThreads / 64) + wave) * R; r0 < a.rows;
         r0 += stride) {
        // lane j < R looks up row r0 + j (the other lanes repeat them); a short last pass
        // repeats the last row, which this wave then copies again with the same values
        const int64_t rl = r0 + (lane & (R - 1));
        int ag, b;
        const int id = sample_id(a, idx0, (int)(rl < a.rows ? rl : a.rows - 1), &ag, &b);
        const WideRow w0 = wide_row<0>(a, id, ag, b), w1 = wide_row<1>(a, id, ag, b),
                      w2 = wide_row<2>(a, id, ag, b), w3 = wide_row<3>(a, id, ag, b);
        for (uint32_t off = (uint32_t)lane * 16u; off < row_bytes; off += 64u * 16u) {
            const float4 v0 = ld16(w0.src, off), v1 = ld16(w1.src, off), v2 = ld16(w2.src, off),
                         v3 = ld16(w3.src, off);
            st16(w0.dst, off, v0);
            st16(w1.dst, off, v1);
            st16(w2.dst, off, v2);
            st16(w3.dst, off, v3);
        }
        if (a.labels && lane < R && rl < a.rows)
            a.labels[(int64_t)ag * a.s_labels + b] = a.targets[id];
    }
}

// one lane's share of row r of a packed pass: chunk c of the row, clamped so that the load is
// always in range; `on` says whether the lane stores it
struct PackedRow {
    const float4 *src;
    float4 *dst;
    int32_t *lab;   // this row's label slot
    int id;
    bool row_on, on;
};
__device__ __forceinline__ PackedRow packed_row(const BatchGatherArgs &a, int64_t idx0,
                                                int64_t r, int c) {
    PackedRow p;
    p.row_on = r < a.rows;
    p.on = p.row_on && c < a.dim4;
    int ag, b;
    p.id = sample_id(a, idx0, (int)(p.row_on ? r : a.rows - 1), &ag, &b);
    const int cc = c < a.dim4 ? c : a.dim4 - 1;
    p.src = reinterpret_cast<const float4 *>(a.samples + (int64_t)p.id * a.ld_samples) + cc;
    p.dst = reinterpret_cast<float4 *>(a.data + (int64_t)ag * a.s_data +
                                       (int64_t)b * a.dim4 * 4) + cc;
    p.lab = a.labels + ((int64_t)ag * a.s_labels + b);
    return p;
}

__global__ __launch_bounds__(kGatherThreads) void batch_gather_packed_kernel(
    const BatchGatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rp = 64 >> a.lane_sh;             // rows per wave-instruction
    const int sub = lane >> a.lane_sh;          // this lane's row among them
    const int c = lane & ((1 << a.lane_sh) - 1);   // and its float4 chunk
    const int64_t pass = (int64_t)R * rp;
    const int64_t stride = (int64_t)gridDim.x * (kGatherThreads / 64) * pass;
    const int64_t idx0 = (int64_t)epoch_step(a) * a.batch;
    for (int64_t r0 = ((int64_t)blockIdx.x * (kGatherThreads / 64) + wave) * pass; r0 < a.rows;
         r0 += stride) {
        const PackedRow p0 = packed_row(a, idx0, r0 + sub, c),
                        p1 = packed_row(a, idx0, r0 + rp + sub, c),
                        p2 = packed_row(a, idx0, r0 + 2 * rp + sub, c),
                        p3 = packed_row(a, idx0, r0 + 3 * rp + sub, c);
        const float4 v0 = *p0.src, v1 = *p1.src, v2 = *p2.src, v3 = *p3.src;
        if (p0.on) *p0.dst = v0;
        if (p1.on) *p1.dst = v1;
        if (p2.on) *p2.dst = v2;
        if (p3.on) *p3.dst = v3;
        if (a.labels && c == 0) {
            if (p0.row_on) *p0.lab = a.targets[p0.id];
            if (p1.row_on) *p1.lab = a.targets[p1.id];
            if (p2.row_on) *p2.lab = a.targets[p2.id];
            if (p3.row_on) *p3.lab = a.targets[p3.id];
        }
    }
}

__global__ void batch_gather_advance_kernel(int32_t *cursor, int32_t steps) {
    int s = cursor[0] % steps;
    if (s < 0) s += steps;
    cursor[0] = (s + 1) % steps;
}

}  // namespace

hipError_t launch_batch_gather(const BatchGatherPlan &p, int32_t *advance, hipStream_t s) {
    if (p.wide)
        hipLaunchKernelGGL(batch_gather_wide_kernel, dim3(p.grid), dim3(kGatherThreads), 0, s,
                           p.k);
    else
        hipLaunchKernelGGL(batch_gather_packed_kernel, dim3(p.grid), dim3(kGatherThreads), 0, s,
                           p.k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !advance) return e;
    hipLaunchKernelGGL(batch_gather_advance_kernel, dim3(1), dim3(1), 0, s, advance, p.k.steps);
    return hipGetLastError();
}

}  // namespace dl
