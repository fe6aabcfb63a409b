// The Adam update of one element, shared by adam_kernel (csrc/train.hip) and optimizer_kernel (csrc/optim.hip): one definition, so that
// vidc_optimizer_step with every option at its default leaves the bits vidc_adam_step leaves.
#pragma once
#include <hip/hip_runtime.h>

namespace vidc {

// One element; every product / sum / quotient rounds once (contraction off: HIP's __fmul_rn / __fadd_rn are plain operators that hipcc
// may still fuse), so an element's bits do not depend on whether the four-wide body or the scalar tail of the launch handled it (the flat
// layout -- and with it an element's position -- differs between the grouped and the per-pyramid form of the step, and
// tests/test_training.py compares their stepped parameters bit for bit).
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float b1, float b2, float c1, float c2, float eps, float step_size,
                                         float bc2_sqrt) {
#pragma clang fp contract(off)
    m = m * b1 + g * c1;
    v = v * b2 + (g * g) * c2;
    const float denom = __fsqrt_rn(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

}  // namespace vidc
