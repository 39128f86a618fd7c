// dl_lenet_eval (include/dlamd.h): every agent's LeNet on a test set, forward only, in one launch
// plus a tiny reduce.  One workgroup per (agent, row split) keeps the agent's 2872 convolution
// parameters in LDS and walks the agent's 64-row blocks b = split, split + row_splits, ...  A
// block is processed in sub-blocks of 16 rows, the M of v_mfma_f32_16x16x4_f32:
//   - passes of kLenetFwdImages images run lenet.hip's two convolution stages (the same
//     conv_window, so the same bits) and leave their pool2 rows in an LDS tile [16][400]; the
//     next pass's images are loaded into registers while this pass computes;
//   - fc1, fc2 and fc3 run on the fp32 MFMA, a k-ordered fma chain from 0 over the whole K like
//     dl_bgemm's, then + bias and ReLU: weight slices of 32 k are staged from the agent's row of X
//     (in L2 after the first sub-block), n-major, the next two slices in registers while this
//     one feeds the MFMAs; h1, h2 and the 16 x nc logits stay in LDS, over the convolution staging;
//   - the head: wave w takes the sub-block's rows w, w + 4, w + 8, w + 12 -- rows w, w + 4, ... of
//     the block, in increasing order over the four sub-blocks, which is the order of dl_bgemm's
//     in-GEMM head -- with xent_term (bgemm.hip's xent_row without dZ) and the argmax.
// Every LDS operand of an MFMA is row-major with a row stride = 2 mod 4, so the 32 lanes that
// ds_read_b32 serves at once (16 rows x 2 consecutive k) fall on 32 distinct banks.
// Rows past the end of a short last block are neither loaded nor stored; what the tile holds in
// their place only reaches their own (masked) outputs, since a GEMM row depends on its own row
// of A alone.  dl_mlp_eval's reduce (launch_eval_reduce) sums the blocks' parts in block order.
#include "dl_internal.h"
#include "lenet_ops.h"

namespace dl {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FI = kLenetFwdImages, NT = kLenetThreads;
constexpr int MB = kEvalBlockRows;
constexpr int SUB = 16;              // rows of a sub-block
constexpr int BK = 32, BN = 128;     // a staged weight slice: BN output units x BK k
constexpr int LDP = kLenetPool2 + 2, LDH1 = kLenetFc1 + 2, LDH2 = kLenetFc2 + 2, LDB = BK + 2;
constexpr int LDZ = kLenetMaxClasses + 1;
static_assert(LDP % 4 == 2 && LDH1 % 4 == 2 && LDH2 % 4 == 2 && LDB % 4 == 2,
              "16 rows x 2 k on 32 distinct banks");
static_assert(kLenetFc1 <= BN && kLenetPool2 % 4 == 0 && kLenetFc1 % 4 == 0 && kLenetFc2 % 4 == 0,
              "one slice covers a layer's outputs; K in whole MFMAs and float4s");
static_assert(MB % SUB == 0 && SUB % 4 == 0 && SUB % FI == 0 && NT == 256, "rows of a wave");
static_assert(BK == 32, "fc_layer deals a slice row as 8 float4s (e >> 3, e & 7)");
// LDS map, in floats: the convolution parameters, the pool2 tile, then the convolution staging
// (images, pool1) and the Linear layers' (weight slice, h1, h2, logits) over each other
constexpr int O_W = 0;
constexpr int O_P2 = O_W + kLenetConvParams;
constexpr int O_U = O_P2 + SUB * LDP;
constexpr int O_IMG = O_U, O_P1 = O_IMG + FI * kLenetImage, CONV_END = O_P1 + FI * kLenetPool1;
constexpr int O_B = O_U, O_H1 = O_B + BN * LDB, O_H2 = O_H1 + SUB * LDH1;
constexpr int O_Z = O_H2 + SUB * LDH2, FC_END = O_Z + SUB * LDZ;
constexpr int O_RED = CONV_END > FC_END ? CONV_END : FC_END;   // [4] loss parts, [4] hit counts
constexpr int LDS_FLOATS = O_RED + 8;
static_assert(O_P2 % 4 == 0 && O_U % 4 == 0 && O_P1 % 2 == 0, "float4 staging, float2 patches");
static_assert(LDS_FLOATS * 4 == kLenetEvalLdsBytes, "launch.h states this file's LDS footprint");
static_assert(kLenetEvalWgPerCu * kLenetEvalLdsBytes <= 160 * 1024, "workgroups per compute unit");

// out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) for the 16 rows m of a sub-block: A and out in
// LDS, W [N][K] and bias in the agent's row of X.  Wave w owns the 16-wide column tiles w and
// w + 4.  Ends with the slice's readers done; the caller syncs before `out` is read.
template <bool RELU>
__device__ __forceinline__ void fc_layer(const float *A, int lda, const float *W,
                                         const float *bias, int N, int K, float *Bs, float *out,
                                         int ldo, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int ntiles = (N + 15) >> 4;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    constexpr int NB = BN * BK / 4 / NT;   // float4s of a slice per thread
    float4 ra[NB], rb[NB];
    auto load = [&](float4 (&r)[NB], int k0) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + i * NT;
            const int n = e >> 3, k = k0 + 4 * (e & 7);
            r[i] = (n < N && k < K) ? *reinterpret_cast<const float4 *>(W + n * K + k)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // one slice: its registers to LDS, the slice after the next into them (two slices are in
    // flight: these GEMMs wait on L2 latency, not on the MFMAs), then the MFMAs
    auto slice = [&](float4 (&r)[NB], int k0) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + i * NT;
            float2 *q = reinterpret_cast<float2 *>(Bs + (e >> 3) * LDB + 4 * (e & 7));
            q[0] = make_float2(r[i].x, r[i].y);
            q[1] = make_float2(r[i].z, r[i].w);
        }
        __syncthreads();
        if (k0 + 2 * BK < K) load(r, k0 + 2 * BK);
        const int ks = min(BK, K - k0);
        for (int kk = 0; kk < ks; kk += 4) {
            const int k = kk + (lane >> 4);
            const float af = A[(lane & 15) * lda + k0 + k];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int t = wave + 4 * j;
                if (t < ntiles)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        af, Bs[(t * 16 + (lane & 15)) * LDB + k], acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    };
    load(ra, 0);
    if (BK < K) load(rb, BK);
    for (int k0 = 0; k0 < K; k0 += 2 * BK) {
        slice(ra, k0);
        if (k0 + BK < K) slice(rb, k0 + BK);
    }
    // C/D map: col = lane & 15, row = 4 * (lane >> 4) + r
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = (wave + 4 * j) * 16 + (lane & 15);
        if (n >= N) continue;
        const float b = bias[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[j][r] + b;
            if (RELU) v = v > 0.f ? v : 0.f;
            out[(4 * (lane >> 4) + r) * ldo + n] = v;
        }
    }
}

// HEAD = false: logits only (no labels are read).
template <bool HEAD>
__global__ __launch_bounds__(NT) void lenet_eval_kernel(const LenetEvalArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_w = lds + O_W, *s_p2 = lds + O_P2, *s_img = lds + O_IMG, *s_p1 = lds + O_P1;
    float *Bs = lds + O_B, *H1 = lds + O_H1, *H2 = lds + O_H2, *Zs = lds + O_Z;
    float *lpart = lds + O_RED;
    int *hpart = reinterpret_cast<int *>(lpart) + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // consecutive workgroups are consecutive agents: with the grid dealt round-robin to the
    // XCDs, an agent's splits -- which read the same Linear weights -- share an L2
    const int ag = blockIdx.x % p.n_agents, split = blockIdx.x / p.n_agents;
    const int nc = p.nc;
    const float *X = p.X + (int64_t)ag * p.ldx;
    {
        const float4 *x = reinterpret_cast<const float4 *>(X);
        for (int i = tid; i < kLenetConvParams / 4; i += NT)
            reinterpret_cast<float4 *>(s_w)[i] = x[i];
    }
    // a pass's images travel in registers while the pass before it (and, at a sub-block's end,
    // the Linear layers) computes: `row` is the agent's row of the first, `n` how many.  LDS
    // admits two workgroups a compute unit, so a thread may use 256 registers: these are free.
    constexpr int PRE = FI * (kLenetImage / 4) / NT;
    static_assert(PRE * NT == FI * (kLenetImage / 4), "a pass's float4s split over the threads");
    float4 pre[PRE];
    auto fetch = [&](int row, int n) {
        const float4 *src = reinterpret_cast<const float4 *>(
            p.data + (int64_t)ag * p.s_data + (int64_t)row * kLenetImage);
#pragma unroll
        for (int i = 0; i < PRE; ++i)
            pre[i] = tid + i * NT < n * (kLenetImage / 4) ? src[tid + i * NT]
                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    if (split < p.blocks) fetch(split * MB, min(FI, p.rows - split * MB));
    for (int b = split; b < p.blocks; b += p.row_splits) {
        const int r0 = b * MB;                    // < rows: no overflow
        const int nv = min(MB, p.rows - r0);      // the block's rows
        float lsum = 0.f;
        int hsum = 0;
        for (int s0 = 0; s0 < nv; s0 += SUB) {
            const int nvs = min(SUB, nv - s0);    // the sub-block's rows
            for (int i0 = 0; i0 < nvs; i0 += FI) {
                const int nimg = min(FI, nvs - i0);
                __syncthreads();   // the previous pass's, or the previous head's, readers are done
#pragma unroll
                for (int i = 0; i < PRE; ++i)
                    if (tid + i * NT < nimg * (kLenetImage / 4))
                        reinterpret_cast<float4 *>(s_img)[tid + i * NT] = pre[i];
                {   // the next pass: of this block (passes are consecutive rows), else of the next
                    const int off = s0 + i0 + FI, bn = b + p.row_splits;
                    if (off < nv)
                        fetch(r0 + off, min(FI, nv - off));
                    else if (bn < p.blocks)
                        fetch(bn * MB, min(FI, p.rows - bn * MB));
                }
                __syncthreads();
                // conv1 + ReLU + pool: item = (image, window, channel), the channel fastest
                for (int it = tid; it < nimg * kLenetPool1; it += NT) {
                    const int im = it / kLenetPool1, r = it - im * kLenetPool1;
                    const int q = r / 6, c = r - q * 6;
                    const int py = q / 14, px = q - py * 14;
                    int code;
                    s_p1[im * kLenetPool1 + c * 196 + q] = conv_window<3>(
                        s_img + im * kLenetImage + 2 * py * 32 + 2 * px, 1024, 32,
                        s_w + kLenetConv1W + c * 75, s_w[kLenetConv1B + c], code);
                }
                __syncthreads();
                // conv2 + ReLU + pool on pool1 in LDS, into the images' rows of the tile
                for (int it = tid; it < nimg * kLenetPool2; it += NT) {
                    const int im = it / kLenetPool2, r = it - im * kLenetPool2;
                    const int q = r / 16, c = r - q * 16;
                    const int py = q / 5, px = q - py * 5;
                    int code;
                    s_p2[(i0 + im) * LDP + c * 25 + q] = conv_window<6>(
                        s_p1 + im * kLenetPool1 + 2 * py * 14 + 2 * px, 196, 14,
                        s_w + kLenetConv2W + c * 150, s_w[kLenetConv2B + c], code);
                }
            }
            __syncthreads();   // the tile is complete; the staging area is free
            fc_layer<true>(s_p2, LDP, X + kLenetFc1W, X + kLenetFc1B, kLenetFc1, kLenetPool2, Bs,
                           H1, LDH1, tid);
            __syncthreads();
            fc_layer<true>(H1, LDH1, X + kLenetFc2W, X + kLenetFc2B, kLenetFc2, kLenetFc1, Bs, H2,
                           LDH2, tid);
            __syncthreads();
            fc_layer<false>(H2, LDH2, X + kLenetFc3W, X + kLenetFc3W + kLenetFc2 * nc, nc,
                            kLenetFc2, Bs, Zs, LDZ, tid);
            __syncthreads();
            if (p.logits) {
                float *zo = p.logits + (int64_t)ag * p.s_logits + (int64_t)(r0 + s0) * p.ldz;
                for (int i = tid; i < nvs * nc; i += NT) {
                    const int m = i / nc, c = i - m * nc;
                    zo[(int64_t)m * p.ldz + c] = Zs[m * LDZ + c];
                }
            }
            if constexpr (HEAD) {
#pragma unroll
                for (int i = 0; i < SUB / 4; ++i) {
                    const int m = wave + 4 * i;
                    if (m >= nvs) break;
                    const int label = p.labels[(int64_t)ag * p.s_lab + r0 + s0 + m];
                    const float v = lane < nc ? Zs[m * LDZ + lane] : 0.f;
                    float mx;
                    lsum += xent_term(v, lane, nc, label, MB, mx);
                    // the first class whose logit is the row maximum; a NaN logit: wrong
                    const unsigned long long at = __ballot(lane < nc && v == mx);
                    const bool nan = __any(lane < nc && v != v);
                    hsum += (!nan && at != 0ull && __ffsll(at) - 1 == label) ? 1 : 0;
                }
            }
        }
        if constexpr (HEAD) {
            if (lane == 0) {
                lpart[wave] = lsum;
                hpart[wave] = hsum;
            }
            __syncthreads();
            if (tid == 0) {
                const int64_t o = (int64_t)ag * p.blocks + b;
                p.part[o] = (lpart[0] + lpart[1]) + (lpart[2] + lpart[3]);
                p.hit[o] = (hpart[0] + hpart[1]) + (hpart[2] + hpart[3]);
            }
            // the next block's first pass syncs before anything writes lpart again
        }
    }
}

}  // namespace

hipError_t launch_lenet_eval(const LenetEvalArgs &p, int lds_bytes, float *loss, int32_t *correct,
                             hipStream_t s) {
    const bool head = loss || correct;
    auto go = [&](auto kern) {
        hipError_t e = allow_full_lds(reinterpret_cast<const void *>(kern));
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)(p.n_agents * p.row_splits)), dim3(NT), lds_bytes,
                           s, p);
        return hipGetLastError();
    };
    hipError_t e = head ? go(lenet_eval_kernel<true>) : go(lenet_eval_kernel<false>);
    if (e != hipSuccess || !head) return e;
    return launch_eval_reduce(p.part, p.hit, p.n_agents, p.blocks, p.rows, loss, correct, s);
}

}  // namespace dl
