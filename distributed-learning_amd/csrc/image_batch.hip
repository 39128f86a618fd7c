// dl_image_batch: every agent's next mini-batch of a planar uint8 image dataset resident in HBM
// (include/dlamd.h): gathered by sample id, cropped out of the image padded with `fill` at the
// caller's (top, left), flipped, and mapped byte by byte through a per-channel table of 256
// floats to fp32 NCHW.  No arithmetic on the values and no random numbers: the kernel copies
// table entries, and the draws are data (the aug table beside index).
//
// A wave owns whole destination images, grid-strided over a grid shaped from the compute units
// (launch.h shape_image_batch), so the sample id, the crop offset and the flip are wave-uniform
// and the image bases scalar.  2^lane_sh >= width / 4 lanes share an output row; a lane produces
// four output pixels of a row as one float4 store.  Their four source bytes are consecutive in
// the source row (reversed under a flip) and come from the two aligned dwords that cover them,
// funnel-shifted; a dword lies wholly inside or wholly outside the row (width % 4 == 0), an
// outside one is `fill` and its load is clamped into the row, so nothing outside the image is
// touched.  kImageRowsInFlight rows of a channel are loaded before the first is stored.  The
// table (at most 16 KiB) is staged in LDS once per workgroup.  Plain stores: the consumer reads
// the batch next.  The cursor is read by every workgroup as one uniform load and written only by
// the one-thread launch that follows on the stream.
#include "dl_internal.h"

namespace dl {
namespace {

constexpr int R = kImageRowsInFlight;
static_assert(R == 4, "the kernel below spells out four rows in flight");

// the step inside the epoch: wave-uniform, in [0, steps)
__device__ inline int epoch_step(const ImageBatchArgs &a) {
    if (!a.cursor) return a.step;   // normalised on the host
    int s = a.cursor[0] % a.steps;
    return s < 0 ? s + a.steps : s;
}

// Where a lane's four source bytes lie in any source row of its image: the byte offsets of the
// two covering dwords clamped into the row, whether each lies inside it, and the funnel shift.
struct Cols {
    uint32_t a_off, b_off, sh;
    bool a_in, b_in;
};
__device__ __forceinline__ Cols source_cols(int lo, int W) {
    const int base = lo & ~3;   // floor to a dword, negatives too
    Cols k;
    k.sh = (uint32_t)(lo & 3) * 8u;
    k.a_in = base >= 0 && base <= W - 4;
    k.b_in = base + 4 >= 0 && base + 4 <= W - 4;
    k.a_off = (uint32_t)min(max(base, 0), W - 4);
    k.b_off = (uint32_t)min(max(base + 4, 0), W - 4);
    return k;
}

// the covering dwords of output row y (source row y + dy of the plane), `fill` where outside
struct Row {
    uint32_t a, b;
};
__device__ __forceinline__ Row load_row(const uint8_t *plane, int y, int dy, int H, int W,
                                        const Cols &k, uint32_t fill4) {
    const int sy = y + dy;
    const bool in = sy >= 0 && sy < H;
    const uint8_t *row = plane + (uint32_t)min(max(sy, 0), H - 1) * (uint32_t)W;
    const uint32_t va = *reinterpret_cast<const uint32_t *>(row + k.a_off);
    const uint32_t vb = *reinterpret_cast<const uint32_t *>(row + k.b_off);
    return {in && k.a_in ? va : fill4, in && k.b_in ? vb : fill4};
}

__device__ __forceinline__ void store_row(float *plane, int y, int H, int W, int x, const Row &r,
                                          const Cols &k, bool flip, const float *lut) {
    uint32_t v = __builtin_amdgcn_alignbit(r.b, r.a, k.sh);   // bytes lo .. lo + 3
    if (flip) v = __builtin_bswap32(v);
    const float4 o = make_float4(lut[v & 255u], lut[(v >> 8) & 255u], lut[(v >> 16) & 255u],
                                 lut[v >> 24]);
    if (y < H) *reinterpret_cast<float4 *>(plane + (uint32_t)y * (uint32_t)W + (uint32_t)x) = o;
}

__global__ __launch_bounds__(kImageThreads) void image_batch_kernel(const ImageBatchArgs a) {
    extern __shared__ float s_lut[];   // [channels][256]
    const int C = a.channels, H = a.height, W = a.width, w4 = W >> 2;
    for (int i = threadIdx.x; i < C * 64; i += kImageThreads)
        reinterpret_cast<float4 *>(s_lut)[i] = reinterpret_cast<const float4 *>(a.lut)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rp = 64 >> a.lane_sh;                  // output rows per wave-instruction
    const int sub = lane >> a.lane_sh;               // this lane's row among them
    const int xl = lane & ((1 << a.lane_sh) - 1);    // and its first float4 of the row
    const int64_t idx0 = (int64_t)epoch_step(a) * a.batch;
    const uint32_t hw = (uint32_t)H * (uint32_t)W;   // C * hw <= 2^28 (shape_image_batch)
    const int64_t stride = (int64_t)gridDim.x * (kImageThreads / 64);
    for (int64_t im = (int64_t)blockIdx.x * (kImageThreads / 64) + wave; im < a.images;
         im += stride) {
        const int ag = (int)(im / a.batch), b = (int)(im - (int64_t)ag * a.batch);
        int id = a.index[(int64_t)ag * a.s_index + idx0 + b];
        id = id < 0 ? 0 : id;
        id = __builtin_amdgcn_readfirstlane(id >= a.n_samples ? a.n_samples - 1 : id);
        int top = a.pad, left = a.pad;
        bool flip = false;
        if (a.aug) {
            const int word =
                __builtin_amdgcn_readfirstlane(a.aug[(int64_t)ag * a.s_aug + idx0 + b]);
            top = min(word & 255, 2 * a.pad);
            left = min((word >> 8) & 255, 2 * a.pad);
            flip = (word >> 16) & 1;
        }
        const int dy = top - a.pad, dx = left - a.pad;
        const uint8_t *img = a.samples + (int64_t)id * a.ld_samples;
        float *dst = a.data + (int64_t)ag * a.s_data + (int64_t)b * C * hw;
        if (a.labels && lane == 0) a.labels[(int64_t)ag * a.s_labels + b] = a.targets[id];
        for (int x4 = xl; x4 < w4; x4 += 64) {   // one trip unless a row is wider than 256 pixels
            const int x = 4 * x4;
            const Cols k = source_cols((flip ? W - 4 - x : x) + dx, W);
            for (int c = 0; c < C; ++c) {
                const uint8_t *plane = img + (uint32_t)c * hw;
                float *oplane = dst + (uint32_t)c * hw;
                const float *lut = s_lut + c * 256;
                for (int yb = 0; yb < H; yb += R * rp) {
                    const int y0 = yb + sub, y1 = y0 + rp, y2 = y1 + rp, y3 = y2 + rp;
                    const Row r0 = load_row(plane, y0, dy, H, W, k, a.fill4),
                              r1 = load_row(plane, y1, dy, H, W, k, a.fill4),
                              r2 = load_row(plane, y2, dy, H, W, k, a.fill4),
                              r3 = load_row(plane, y3, dy, H, W, k, a.fill4);
                    store_row(oplane, y0, H, W, x, r0, k, flip, lut);
                    store_row(oplane, y1, H, W, x, r1, k, flip, lut);
                    store_row(oplane, y2, H, W, x, r2, k, flip, lut);
                    store_row(oplane, y3, H, W, x, r3, k, flip, lut);
                }
            }
        }
    }
}

__global__ void image_batch_advance_kernel(int32_t *cursor, int32_t steps) {
    int s = cursor[0] % steps;
    if (s < 0) s += steps;
    cursor[0] = (s + 1) % steps;
}

}  // namespace

hipError_t launch_image_batch(const ImageBatchPlan &p, int32_t *advance, hipStream_t s) {
    hipLaunchKernelGGL(image_batch_kernel, dim3(p.grid), dim3(kImageThreads), p.lds_bytes, s,
                       p.k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !advance) return e;
    hipLaunchKernelGGL(image_batch_advance_kernel, dim3(1), dim3(1), 0, s, advance, p.k.steps);
    return hipGetLastError();
}

}  // namespace dl
