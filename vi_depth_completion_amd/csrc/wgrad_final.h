// The last stage of every conv weight gradient (csrc/train.hip: wgrad_final_kernel), shared by the fp32 entries there and the bf16 entry of
// csrc/wgrad_bf16.hip: partial[chunk][tap][Cout][Cin] fp32 -> dw[Cout][Cin][tap], the chunks summed in fp64 in chunk order and rounded once.
#pragma once
#include "common.h"

namespace vidc {

// Enqueues the kernel on `st`; the caller checks the launch (VIDC_CHECK_LAUNCH).
void launch_wgrad_final(const float* partial, int chunks, int taps, int Cout, int Cin, float* dw_oihw, hipStream_t st);

}  // namespace vidc
