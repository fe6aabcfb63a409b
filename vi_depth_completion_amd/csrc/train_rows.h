// Row-quad helpers of the training kernels (csrc/train.hip).  A "row quad" is four consecutive channels c..c+3 (c % 4 == 0) of one NHWC row:
// one thread owns it, reads it with one 16-byte load into a float[4], works on the four lanes and writes it with one 16-byte store (fp32) or
// one 8-byte store (bf16).  Row strides are multiples of 4 and the tensors 16-byte aligned wherever these are used (host-checked).
#pragma once
#include "common.h"

namespace vidc {

// Thread -> quad of a flat launch over [rows][C / V] groups of V channels (blocks(rows * (C / V)) workgroups of TT): row r, first channel c;
// false for the threads past the end.  V = 4: a row quad; V = 8: two of them side by side (cast_bf16_kernel).
template <int V = 4>
__device__ inline bool row_quad(long long rows, int C, long long& r, int& c) {
    const int cv = C / V;
    const long long i = (long long)blockIdx.x * TT + threadIdx.x;
    if (i >= rows * cv) return false;
    r = i / cv;
    c = (int)(i - r * cv) * V;
    return true;
}

__device__ inline void load4(const float* __restrict__ p, float* v) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
__device__ inline void store4(float* __restrict__ p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
// (bf16 values as they sit in memory: the bf16 operand copies are moved, never re-rounded)
__device__ inline void load4(const unsigned short* __restrict__ p, unsigned short* v) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    v[0] = (unsigned short)q.x; v[1] = (unsigned short)(q.x >> 16); v[2] = (unsigned short)q.y; v[3] = (unsigned short)(q.y >> 16);
}

// Four values as bf16 in 8 bytes, the first in the low half of .x: fp32 values are rounded to nearest even (bf16_rne: the one rounding of
// every bf16 operand copy the training step writes), bf16 values are packed as they are.
__device__ inline uint2 pack4_bf16(const float* v) {
    return make_uint2((unsigned)bf16_rne(v[0]) | ((unsigned)bf16_rne(v[1]) << 16), (unsigned)bf16_rne(v[2]) | ((unsigned)bf16_rne(v[3]) << 16));
}
__device__ inline uint2 pack4_bf16(const unsigned short* v) {
    return make_uint2((unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16));
}
// ... written by one 8-byte store (dst 8-byte aligned), and eight by one 16-byte store (dst 16-byte aligned)
template <typename T>
__device__ inline void store4_bf16(unsigned short* __restrict__ dst, const T* v) { *reinterpret_cast<uint2*>(dst) = pack4_bf16(v); }
__device__ inline void store8_bf16(unsigned short* __restrict__ dst, const float* v) {
    const uint2 a = pack4_bf16(v), b = pack4_bf16(v + 4);
    *reinterpret_cast<uint4*>(dst) = make_uint4(a.x, a.y, b.x, b.y);
}

// The backward of a ReLU on a quad: the gradient passes where the ReLU's OUTPUT y is positive (NaN and both zeros close the gate)
__device__ inline void relu_mask4(float* g, const float* y) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (!(y[k] > 0.f)) g[k] = 0.f;
}

}  // namespace vidc
