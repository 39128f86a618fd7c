// dl_lenet_grad's convolution stages (include/dlamd.h): LeNet's conv1 -> ReLU -> 2x2 max-pool ->
// conv2 -> ReLU -> 2x2 max-pool forward, and its backward, for every agent's own batch and own
// parameters, in plain fp32 FMA.  The three Linear layers between them are dl_bgemm's GEMMs
// (capi.hip queues the sequence).  Grids come from launch.h shape_lenet: workgroup w of an agent
// walks that agent's passes (forward: kLenetFwdImages images) or groups (backward: kLenetGroup
// images) w, w + wpa, ...; nothing a thread computes depends on wpa.
//
// Forward.  A workgroup keeps the agent's 2872 convolution parameters in LDS, stages the pass's
// images with 16-byte loads and computes each pooled output from the four convolution outputs
// of its window: an input patch of 6 x 6 per input channel in registers, one weight read per
// four FMAs.  Lanes that differ only in the output channel read the same patch (an LDS
// broadcast) and weights a channel stride apart (75 and 150 floats: distinct banks).  pool1
// stays in LDS for conv2; with `train` pool1, pool2 and one byte per pooled output -- the
// window's first maximum in row-major order, or 4 when none is positive, which is all the
// backward needs of ReLU and pooling -- go to the workspace through LDS with coalesced stores.
//
// Backward.  Only a window's winner carries a gradient, so the gradient of a convolution
// output plane is one value and one position per pooled window.  Per image: the weight gradient
// of conv2 is 25 FMAs per element against pool1 at the winners' positions, the gradient entering
// pool1 gathers, per conv2 channel, the at most nine windows whose winner can reach an element
// (the full correlation with conv2.weight, three quarters of it zeros, skipped), and conv1's
// weight gradient is 196 FMAs per element against the image.  A thread owns fixed rows of five
// kernel columns of the 2872 gradients and keeps them in registers over a group of kLenetGroup
// images; group sums go to the workspace and lenet_conv_reduce_kernel adds them in group order.
#include "dl_internal.h"
#include "lenet_ops.h"   // pool_relu, conv_window: shared with lenet_eval.hip

namespace dl {
namespace {

constexpr int FI = kLenetFwdImages;
constexpr int NT = kLenetThreads;
constexpr int kNone = kPoolNone;   // winner code: no positive value in the window

__global__ __launch_bounds__(NT) void lenet_conv_fwd_kernel(const LenetConvArgs a) {
    __shared__ __attribute__((aligned(16))) float s_w[kLenetConvParams];
    __shared__ __attribute__((aligned(16))) float s_img[FI * kLenetImage];
    __shared__ __attribute__((aligned(16))) float s_p1[FI * kLenetPool1];
    __shared__ __attribute__((aligned(16))) float s_p2[FI * kLenetPool2];
    __shared__ __attribute__((aligned(16))) uint8_t s_c1[FI * kLenetPool1];
    __shared__ __attribute__((aligned(16))) uint8_t s_c2[FI * kLenetPool2];
    const int tid = threadIdx.x;
    const int ag = blockIdx.x / a.fwd_wpa, w = blockIdx.x - ag * a.fwd_wpa;
    {
        const float4 *x = reinterpret_cast<const float4 *>(a.X + (int64_t)ag * a.ldx);
        for (int i = tid; i < kLenetConvParams / 4; i += NT)
            reinterpret_cast<float4 *>(s_w)[i] = x[i];
    }
    for (int pass = w; pass < a.passes; pass += a.fwd_wpa) {
        const int b0 = pass * FI;
        const int nimg = min(FI, a.batch - b0);
        const int64_t im0 = (int64_t)ag * a.batch + b0;   // first image's row in the workspace
        __syncthreads();   // the previous pass's readers are done
        {
            const float4 *src = reinterpret_cast<const float4 *>(
                a.data + (int64_t)ag * a.s_data + (int64_t)b0 * kLenetImage);
            for (int i = tid; i < nimg * (kLenetImage / 4); i += NT)
                reinterpret_cast<float4 *>(s_img)[i] = src[i];
        }
        __syncthreads();
        // conv1 + ReLU + pool: item = (image, window, channel), the channel fastest
        for (int it = tid; it < nimg * kLenetPool1; it += NT) {
            const int im = it / kLenetPool1, r = it - im * kLenetPool1;
            const int p = r / 6, c = r - p * 6;
            const int py = p / 14, px = p - py * 14;
            int code;
            const float v = conv_window<3>(s_img + im * kLenetImage + 2 * py * 32 + 2 * px, 1024,
                                           32, s_w + kLenetConv1W + c * 75,
                                           s_w[kLenetConv1B + c], code);
            s_p1[im * kLenetPool1 + c * 196 + p] = v;
            s_c1[im * kLenetPool1 + c * 196 + p] = (uint8_t)code;
        }
        __syncthreads();
        if (a.train) {
            float4 *dp = reinterpret_cast<float4 *>(a.pool1 + im0 * kLenetPool1);
            uint32_t *dc = reinterpret_cast<uint32_t *>(a.code1 + im0 * kLenetPool1);
            for (int i = tid; i < nimg * (kLenetPool1 / 4); i += NT) {
                dp[i] = reinterpret_cast<const float4 *>(s_p1)[i];
                dc[i] = reinterpret_cast<const uint32_t *>(s_c1)[i];
            }
        }
        // conv2 + ReLU + pool on pool1 in LDS
        for (int it = tid; it < nimg * kLenetPool2; it += NT) {
            const int im = it / kLenetPool2, r = it - im * kLenetPool2;
            const int p = r / 16, c = r - p * 16;
            const int py = p / 5, px = p - py * 5;
            int code;
            const float v = conv_window<6>(s_p1 + im * kLenetPool1 + 2 * py * 14 + 2 * px, 196,
                                           14, s_w + kLenetConv2W + c * 150,
                                           s_w[kLenetConv2B + c], code);
            s_p2[im * kLenetPool2 + c * 25 + p] = v;
            s_c2[im * kLenetPool2 + c * 25 + p] = (uint8_t)code;
        }
        __syncthreads();
        {
            float4 *dp = reinterpret_cast<float4 *>(a.pool2 + im0 * kLenetPool2);
            uint32_t *dc = reinterpret_cast<uint32_t *>(a.code2 + im0 * kLenetPool2);
            for (int i = tid; i < nimg * (kLenetPool2 / 4); i += NT) {
                dp[i] = reinterpret_cast<const float4 *>(s_p2)[i];
                if (a.train) dc[i] = reinterpret_cast<const uint32_t *>(s_c2)[i];
            }
        }
    }
}

// A thread's rows of five kernel columns.  conv2.weight has 480 rows (co, ci, ky): thread t owns
// rows t and, below 224, t + 256; conv1.weight has 90: threads below 90 own one.  Threads
// 96..111 own conv2.bias, 112..117 conv1.bias.
constexpr int kRows2 = 16 * 6 * 5, kRows1 = 6 * 3 * 5;
constexpr int kBias2Thread = 96, kBias1Thread = 112;

// The image in LDS for conv1's weight gradient: rows of kImgRow floats and planes of kImgPlane,
// both padded so that the 15 rows (ci, ky) a channel's threads read at once, ci * kImgPlane +
// ky * kImgRow apart, fall on 15 distinct banks (25 ci + 5 ky mod 32).
constexpr int kImgRow = 37, kImgPlane = 32 * kImgRow + 25;
static_assert(kImgRow % 32 == 5 && kImgPlane % 32 == 25, "bank spread of the (ci, ky) rows");

__global__ __launch_bounds__(NT) void lenet_conv_bwd_kernel(const LenetConvArgs a) {
    __shared__ float s_img[3 * kImgPlane];
    __shared__ __attribute__((aligned(16))) float s_p1[kLenetPool1];
    __shared__ __attribute__((aligned(16))) float s_w2[2400];
    // per conv2 window: d loss / d (its winner's output) and the winner's (row << 8 | column) in
    // the 10 x 10 plane, read together; 0 and (0, 0) where no output was positive
    __shared__ float2 s_dw2[kLenetPool2];
    __shared__ float s_d1[kLenetPool1];        // likewise for conv1's 28 x 28 planes
    __shared__ uint16_t s_win1[kLenetPool1];   // row * kImgRow + column
    const int tid = threadIdx.x;
    const int ag = blockIdx.x / a.bwd_wpa, w = blockIdx.x - ag * a.bwd_wpa;
    {
        const float4 *x =
            reinterpret_cast<const float4 *>(a.X + (int64_t)ag * a.ldx + kLenetConv2W);
        for (int i = tid; i < 600; i += NT) reinterpret_cast<float4 *>(s_w2)[i] = x[i];
    }
    // row (co, ci, ky) of conv2.weight -> co * 25 into s_dw2 and ci * 196 + ky * 14 into s_p1;
    // of conv1.weight -> co * 196 into s_d1 / s_win1 and ci * kImgPlane + ky * kImgRow into s_img
    const int ra = tid, rb = tid + NT;
    const bool has_b = rb < kRows2, has_1 = tid < kRows1;
    const int ra_d = (ra / 30) * 25, ra_p = ((ra % 30) / 5) * 196 + (ra % 5) * 14;
    const int rb_d = has_b ? (rb / 30) * 25 : 0;
    const int rb_p = has_b ? ((rb % 30) / 5) * 196 + (rb % 5) * 14 : 0;
    const int r1_d = has_1 ? (tid / 15) * 196 : 0;
    const int r1_p = has_1 ? ((tid % 15) / 5) * kImgPlane + (tid % 5) * kImgRow : 0;
    const bool has_b2 = tid >= kBias2Thread && tid < kBias2Thread + 16;
    const bool has_b1 = tid >= kBias1Thread && tid < kBias1Thread + 6;

    for (int g = w; g < a.groups; g += a.bwd_wpa) {
        float acc_a[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, acc_b[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        float acc_1[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        float acc_bias = 0.f;
        const int b0 = g * kLenetGroup;
        const int nimg = min(kLenetGroup, a.batch - b0);
        for (int j = 0; j < nimg; ++j) {
            const int64_t im = (int64_t)ag * a.batch + b0 + j;
            __syncthreads();   // the previous image's readers are done
            {
                const float4 *src = reinterpret_cast<const float4 *>(
                    a.data + (int64_t)ag * a.s_data + (int64_t)(b0 + j) * kLenetImage);
                for (int i = tid; i < kLenetImage / 4; i += NT) {
                    const float4 v = src[i];
                    float *q = s_img + (i >> 8) * kImgPlane + ((i >> 3) & 31) * kImgRow + (i & 7) * 4;
                    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
                }
                const float4 *p1 = reinterpret_cast<const float4 *>(a.pool1 + im * kLenetPool1);
                for (int i = tid; i < kLenetPool1 / 4; i += NT)
                    reinterpret_cast<float4 *>(s_p1)[i] = p1[i];
                const float *da = a.da + im * kLenetPool2;
                const uint8_t *c2 = a.code2 + im * kLenetPool2;
                for (int i = tid; i < kLenetPool2; i += NT) {
                    const int code = c2[i], p = i % 25;
                    const int py = p / 5, px = p - py * 5;
                    const bool on = code < kNone;
                    s_dw2[i] = make_float2(
                        on ? da[i] : 0.f,
                        __int_as_float(on ? ((2 * py + (code >> 1)) << 8) | (2 * px + (code & 1)) : 0));
                }
                const uint8_t *c1 = a.code1 + im * kLenetPool1;
                for (int i = tid; i < kLenetPool1; i += NT) {
                    const int code = c1[i], p = i % 196;
                    const int py = p / 14, px = p - py * 14;
                    s_win1[i] = code < kNone ? (uint16_t)((2 * py + (code >> 1)) * kImgRow +
                                                          2 * px + (code & 1))
                                             : (uint16_t)0xffff;
                }
            }
            __syncthreads();
            // conv2.weight rows and conv2.bias
#pragma unroll 5
            for (int p = 0; p < 25; ++p) {
                const float2 dw = s_dw2[ra_d + p];
                const int wn = __float_as_int(dw.y);
                const float *q = s_p1 + ra_p + (wn >> 8) * 14 + (wn & 255);
#pragma unroll
                for (int k = 0; k < 5; ++k) acc_a[k] = fmaf(dw.x, q[k], acc_a[k]);
            }
            if (has_b) {
#pragma unroll 5
                for (int p = 0; p < 25; ++p) {
                    const float2 dw = s_dw2[rb_d + p];
                    const int wn = __float_as_int(dw.y);
                    const float *q = s_p1 + rb_p + (wn >> 8) * 14 + (wn & 255);
#pragma unroll
                    for (int k = 0; k < 5; ++k) acc_b[k] = fmaf(dw.x, q[k], acc_b[k]);
                }
            }
            if (has_b2)
                for (int p = 0; p < 25; ++p) acc_bias += s_dw2[(tid - kBias2Thread) * 25 + p].x;
            // The gradient entering pool1, where a window has a winner: element (ci, y, x) gathers
            // the windows of every conv2 channel whose winner (Y, X) has y - 4 <= Y <= y and
            // x - 4 <= X <= x.  They lie among at most 3 x 3 windows, the same for every channel;
            // all nine slots are read (a slot outside the range, or whose winner is out of reach,
            // adds 0 x a weight), so that a channel's loads do not wait for one another.
            for (int i = tid; i < kLenetPool1; i += NT) {
                if (s_win1[i] == 0xffff) {
                    s_win1[i] = 0;
                    s_d1[i] = 0.f;
                    continue;
                }
                const int ci = i / 196, p = i - ci * 196;
                const int y = p / 14, x = p - y * 14;
                const int py0 = max(0, (y - 4) >> 1), py1 = min(4, y >> 1);
                const int px0 = max(0, (x - 4) >> 1), px1 = min(4, x >> 1);
                int slot[9];
                bool live[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    const int py = py0 + c / 3, px = px0 + c % 3;
                    live[c] = py <= py1 && px <= px1;
                    slot[c] = live[c] ? py * 5 + px : 0;
                }
                float acc = 0.f;
#pragma unroll 2
                for (int co = 0; co < 16; ++co) {
                    const float *wq = s_w2 + (co * 6 + ci) * 25;
#pragma unroll
                    for (int c = 0; c < 9; ++c) {
                        const float2 dw = s_dw2[co * 25 + slot[c]];
                        const int wn = __float_as_int(dw.y);
                        const int ky = y - (wn >> 8), kx = x - (wn & 255);
                        const bool hit = live[c] && (unsigned)ky < 5u && (unsigned)kx < 5u;
                        acc = fmaf(hit ? dw.x : 0.f, wq[hit ? ky * 5 + kx : 0], acc);
                    }
                }
                s_d1[i] = acc;
            }
            __syncthreads();
            // conv1.weight rows and conv1.bias
            if (has_1) {
#pragma unroll 4
                for (int p = 0; p < 196; ++p) {
                    const float d = s_d1[r1_d + p];
                    const float *q = s_img + r1_p + s_win1[r1_d + p];
#pragma unroll
                    for (int k = 0; k < 5; ++k) acc_1[k] = fmaf(d, q[k], acc_1[k]);
                }
            }
            if (has_b1)
                for (int p = 0; p < 196; ++p) acc_bias += s_d1[(tid - kBias1Thread) * 196 + p];
        }
        float *part = a.part + ((int64_t)ag * a.groups + g) * kLenetConvParams;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            part[kLenetConv2W + ra * 5 + k] = acc_a[k];
            if (has_b) part[kLenetConv2W + rb * 5 + k] = acc_b[k];
            if (has_1) part[kLenetConv1W + tid * 5 + k] = acc_1[k];
        }
        if (has_b2) part[kLenetConv2B + tid - kBias2Thread] = acc_bias;
        if (has_b1) part[kLenetConv1B + tid - kBias1Thread] = acc_bias;
    }
}

__global__ __launch_bounds__(NT) void lenet_conv_reduce_kernel(const LenetConvArgs a) {
    const int j = blockIdx.x * NT + threadIdx.x, ag = blockIdx.y;
    if (j >= kLenetConvParams) return;
    const float *part = a.part + (int64_t)ag * a.groups * kLenetConvParams + j;
    float s = part[0];
    for (int g = 1; g < a.groups; ++g) s += part[(int64_t)g * kLenetConvParams];
    a.G[(int64_t)ag * a.ldg + j] = s;
}

}  // namespace

hipError_t launch_lenet_conv_fwd(const LenetConvArgs &p, int grid, hipStream_t s) {
    hipLaunchKernelGGL(lenet_conv_fwd_kernel, dim3(grid), dim3(NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_lenet_conv_bwd(const LenetConvArgs &p, int grid, hipStream_t s) {
    hipLaunchKernelGGL(lenet_conv_bwd_kernel, dim3(grid), dim3(NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_lenet_conv_reduce(const LenetConvArgs &p, int n_agents, hipStream_t s) {
    hipLaunchKernelGGL(lenet_conv_reduce_kernel, dim3((kLenetConvParams + NT - 1) / NT, n_agents),
                       dim3(NT), 0, s, p);
    return hipGetLastError();
}

}  // namespace dl
