// torch.optim.SGD.step (single-tensor form, torch/optim/sgd.py) on one element, in the rounding
// of torch's fused add-with-alpha (one fma per `add(.., alpha=..)`):
//   d = fma(wd, x, g)                                   grad.add(param, alpha=weight_decay)
//   buf = first ? d : fma(1 - dampening, d, mu * buf)   buf.mul_(momentum).add_(grad, alpha=1-damp)
//   d = nesterov ? fma(mu, buf, d) : buf                grad.add(buf, alpha=momentum)
//   out = fma(-lr, d, x)                                param.add_(grad, alpha=-lr)
// Shared by dl_sgd_step (aux_kernels.hip) and the fused momentum round (mix_sgd.hip), so the two
// cannot round differently.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"   // SgdParams

namespace dl {

__device__ __forceinline__ float sgd_elem(float x, float g, float &b, const SgdParams &p) {
    float d = p.wd != 0.f ? __builtin_fmaf(p.wd, x, g) : g;
    if (p.mu != 0.f) {
        b = p.first ? d : __builtin_fmaf(1.f - p.damp, d, p.mu * b);
        d = p.nesterov ? __builtin_fmaf(p.mu, b, d) : b;
    }
    return __builtin_fmaf(-p.lr, d, x);
}

}  // namespace dl
