// Device code that fixes the bits of LeNet's forward and of the cross-entropy head, shared by the
// kernels that must agree bit for bit: lenet.hip (dl_lenet_grad's convolutions), bgemm.hip (the
// in-GEMM and stand-alone heads) and lenet_eval.hip (dl_lenet_eval).
#pragma once
#include <hip/hip_runtime.h>

namespace dl {

constexpr int kPoolNone = 4;   // winner code: no positive value in the window

// winner of a 2 x 2 window in row-major order (first maximum, as torch's max_pool2d) after
// ReLU: the value kept and its code
__device__ __forceinline__ float pool_relu(float a00, float a01, float a10, float a11, int &code) {
    float m = a00;
    code = 0;
    if (a01 > m) { m = a01; code = 1; }
    if (a10 > m) { m = a10; code = 2; }
    if (a11 > m) { m = a11; code = 3; }
    if (!(m > 0.f)) { m = 0.f; code = kPoolNone; }
    return m;
}

// The four convolution outputs (5 x 5 kernel) of one pooling window over CI input planes of
// `plane` floats and `row` floats per row; ip: the window's top-left input, 8-byte aligned;
// wp: the output channel's [CI][25] weights.  Sum order: bias, then ci, ky, kx.
template <int CI>
__device__ __forceinline__ float conv_window(const float *ip, int plane, int row, const float *wp,
                                             float bias, int &code) {
    float a00 = bias, a01 = bias, a10 = bias, a11 = bias;
#pragma unroll 1
    for (int ci = 0; ci < CI; ++ci) {
        float pt[6][6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float2 v = *reinterpret_cast<const float2 *>(ip + ci * plane + r * row + 2 * c);
                pt[r][2 * c] = v.x;
                pt[r][2 * c + 1] = v.y;
            }
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const float w = wp[ci * 25 + ky * 5 + kx];
                a00 = fmaf(w, pt[ky][kx], a00);
                a01 = fmaf(w, pt[ky][kx + 1], a01);
                a10 = fmaf(w, pt[ky + 1][kx], a10);
                a11 = fmaf(w, pt[ky + 1][kx + 1], a11);
            }
    }
    return pool_relu(a00, a01, a10, a11, code);
}

// softmax of one logits row held one class per lane (classes <= 64), butterflies over the 64
// lanes: the row maximum (returned), this lane's exp(v - max) (0 past the classes) and their sum
__device__ __forceinline__ float xent_softmax(float v, int lane, int classes, float &e, float &sum) {
    float mx = lane < classes ? v : -INFINITY;
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    e = lane < classes ? expf(v - mx) : 0.f;
    sum = e;
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    return mx;
}

// softmax cross-entropy of such a row: writes dZ = (softmax - onehot) / rows and returns the
// row's loss / rows (meaningful on all lanes).  torch.nn.CrossEntropyLoss, mean reduction.
__device__ __forceinline__ float xent_row(float v, int lane, int classes, int label, int rows,
                                          float *dz_row) {
    float e, sum;
    const float mx = xent_softmax(v, lane, classes, e, sum);
    if (lane < classes) dz_row[lane] = (e / sum - (lane == label ? 1.f : 0.f)) / (float)rows;
    const float zl = __shfl(v, label);
    return (logf(sum) + mx - zl) / (float)rows;
}

// the same loss / rows without dZ, and the row maximum for the caller's argmax
__device__ __forceinline__ float xent_term(float v, int lane, int classes, int label, int rows,
                                           float &mx) {
    float e, sum;
    mx = xent_softmax(v, lane, classes, e, sum);
    const float zl = __shfl(v, label);
    return (logf(sum) + mx - zl) / (float)rows;
}

}  // namespace dl
