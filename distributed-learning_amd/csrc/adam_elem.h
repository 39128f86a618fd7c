// torch.optim.Adam / AdamW step (single-tensor form, torch/optim/adam.py, adamw.py) on one
// element.  Every operation is one separately rounded fp32 operation (plain C++ under
// -ffp-contract=off, no fma), so a numpy fp32 restatement, operation by operation, gives the same
// bits (tests/adam_oracle.py):
//   g  = fl(fl(wd x) + g)                     grad = grad.add(param, alpha=weight_decay)   (Adam, L2)
//   x  = fl(x decay)                          param.mul_(1 - lr * weight_decay)            (AdamW)
//   m' = fl(m + fl(omb1 fl(g - m)))           exp_avg.lerp_(grad, 1 - beta1)
//   v' = fl(fl(b2 v) + fl(fl(omb2 g) g))      exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//   den = fl(fl(fl(sqrt(v')) / bs) + eps)     denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//   s  = fl(x - fl(ss fl(m' / den)))          param.addcdiv_(exp_avg, denom, value=-step_size)
// with ss = lr / (1 - beta1^t) and bs = sqrt(1 - beta2^t) (AdamParams, launch.h).  There is no
// first-step flag: m = v = 0 is the first step.  The square root and the two divides are the
// correctly rounded ones, which is the compiler's default for gfx950; no flag here relaxes it.
// Shared by dl_adam_step (aux_kernels.hip) and the fused Adam round (mix_adam.hip), so the two
// cannot round differently.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"   // AdamParams

namespace dl {

// ss, bs: the coefficients the caller took from p (by value, or once per workgroup from p.coef)
__device__ __forceinline__ float adam_elem(float x, float g, float &m, float &v,
                                           const AdamParams &p, float ss, float bs) {
    if (p.wd != 0.f) {
        if (p.decoupled)
            x = x * p.decay;
        else
            g = p.wd * x + g;
    }
    m = m + p.omb1 * (g - m);
    v = p.b2 * v + (p.omb2 * g) * g;
    const float den = __builtin_sqrtf(v) / bs + p.eps;
    return x - ss * (m / den);
}

__device__ __forceinline__ float adam_step_size(const AdamParams &p) {
    return p.coef ? p.coef[0] : p.ss;
}
__device__ __forceinline__ float adam_bias2_sqrt(const AdamParams &p) {
    return p.coef ? p.coef[1] : p.bs;
}

}  // namespace dl
