"""CPU emulation of the plain-bf16 operand format (include/vidc.h, VIDC_PREC_BF16): round to nearest even on the fp32 bit pattern
(what vidc_cast_bf16, pack kind 4 and the conv's VIDC_BF16_OUT epilogue write), and the packed-weight layout restated from the header:
[Cout][Cin/64][KH][KW][64 x bf16] -- 64 channels per 128-byte K unit, channel unit major, tap minor."""
import torch


def bits(x):
    """float32 tensor -> the bf16 bit patterns (int32 in [0, 65535]) of its values rounded to nearest even: (u + 0x7FFF + bit 16 of u) >> 16."""
    u = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def rounded(x):
    """The values those bit patterns stand for, as float32 (exact: a bf16 is the upper half of an fp32)."""
    return (bits(x) << 16).view(torch.float32).reshape(x.shape)


def tensor_bits(t):
    """A torch.bfloat16 tensor (any device) -> its bit patterns like bits()."""
    return t.contiguous().view(torch.int16).cpu().to(torch.int32) & 0xFFFF


def packed_weight_order(w_oihw):
    """OIHW -> [Cout][K] in the bf16 conv's K order: [Cin/64][KH][KW][64] (float32, not rounded)."""
    co, ci, kh, kw = w_oihw.shape
    return w_oihw.reshape(co, ci // 64, 64, kh, kw).permute(0, 1, 3, 4, 2).reshape(co, -1).contiguous()


def pack_weight(w_oihw):
    """vidc_pack_conv_weight_bf16 emulated: the bit patterns [Cout][K]."""
    return bits(packed_weight_order(w_oihw.float()))
