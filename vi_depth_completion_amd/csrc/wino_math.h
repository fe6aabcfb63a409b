// The arithmetic every Winograd F(m x m, 3x3) kernel of the library shares (csrc/winograd.hip: the three-launch path; csrc/wfused.hip: both forms of
// the one-launch kernel): the column formulas of the transforms and the value the conv's epilogue makes of a folded sum.  One definition, so that a
// layer's bits are the same whichever kernel folds it: the ORDER of the operations below is part of the result.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vidc.h"

// No mul + add contraction (see csrc/winograd.hip): every product and sum rounds once, in every instantiation and translation unit.  The including
// file says so itself before it includes this header; the line here keeps the header right on its own.
#pragma clang fp contract(off)

namespace vidc {

// B^T d for one column (input transform) and A^T m for one column (output transform); the standard matrices of Lavin & Gray
// ("Fast Algorithms for Convolutional Neural Networks", 2015) with interpolation points 0, +-1 (m = 2) and 0, +-1, +-2 (m = 4).
template <int M_> struct Wino;
template <> struct Wino<2> {
    static constexpr int A = 4;
    template <typename V> __device__ static __forceinline__ void bt(const V (&d)[4], V (&t)[4]) {
        t[0] = d[0] - d[2];
        t[1] = d[1] + d[2];
        t[2] = d[2] - d[1];
        t[3] = d[1] - d[3];
    }
    template <typename V> __device__ static __forceinline__ void at(const V (&m)[4], V (&o)[2]) {
        o[0] = (m[0] + m[1]) + m[2];
        o[1] = (m[1] - m[2]) - m[3];
    }
};
template <> struct Wino<4> {
    static constexpr int A = 6;
    template <typename V> __device__ static __forceinline__ void bt(const V (&d)[6], V (&t)[6]) {
        const V p = d[4] - 4.f * d[2], q = d[3] - 4.f * d[1];
        const V r = d[4] - d[2], s = 2.f * (d[3] - d[1]);
        t[0] = (4.f * d[0] - 5.f * d[2]) + d[4];
        t[1] = p + q;
        t[2] = p - q;
        t[3] = r + s;
        t[4] = r - s;
        t[5] = (4.f * d[1] - 5.f * d[3]) + d[5];
    }
    template <typename V> __device__ static __forceinline__ void at(const V (&m)[6], V (&o)[4]) {
        const V s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
        o[0] = (m[0] + s12) + s34;
        o[1] = d12 + 2.f * d34;
        o[2] = s12 + 4.f * s34;
        o[3] = (d12 + 8.f * d34) + m[5];
    }
};

// The epilogue of conv_mfma.hip on one folded value: acc * s1 + b1 -> relu -> [* s2 + b2 -> relu]; ReLU off = max with -inf.
struct WinoEpilogue {
    float lo1, lo2;
    bool aff2;
    __device__ __forceinline__ explicit WinoEpilogue(int flags)
        : lo1((flags & VIDC_RELU1) ? 0.f : -INFINITY), lo2((flags & VIDC_RELU2) ? 0.f : -INFINITY), aff2(flags & VIDC_AFFINE2) {}
    __device__ static __forceinline__ float stage(float v, float s, float b, float lo) { return fmaxf(v * s + b, lo); }
    __device__ __forceinline__ float operator()(float acc, float s1, float b1, float s2, float b2) const {
        float o = stage(acc, s1, b1, lo1);
        if (aff2) o = stage(o, s2, b2, lo2);
        return o;
    }
    // (wino_out_kernel runs stage 1 over the N channels of its thread, then stage 2 over them under ONE test of aff2: as N calls of operator() hipcc
    // turns the N branches into selects)
};

}  // namespace vidc
