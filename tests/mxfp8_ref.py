"""CPU emulation of the MXFP8 format (include/vidc.h): OCP e4m3fn elements, one E8M0 scale byte per 32 consecutive values.
E = max(-127, floor(log2 amax) - 8); element = x * 2^-E rounded to nearest even, saturated to +-448; value = element * 2^E."""
import torch


def _pow2(e):
    """2^e as float32 for integer tensors e in [-126, 127] (built from the exponent field: exact)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quant_blocks(x):
    """x: float32 [..., 32 * nb] -> (e4m3 bytes uint8 [..., 32 * nb], scale bytes uint8 [..., nb])."""
    x = x.float().contiguous()
    xb = x.reshape(*x.shape[:-1], -1, 32)
    amax = xb.abs().amax(-1)
    E = torch.clamp(((amax.view(torch.int32) >> 23) & 0xFF) - 127 - 8, min=-127)
    y = (xb * _pow2(-E)[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)     # (torch's cast gives NaN above 448: clamp first)
    return y.view(torch.uint8).reshape(x.shape), (E + 127).to(torch.uint8)


def dequant_blocks(codes, scales):
    """Inverse of quant_blocks: float64 values element * 2^E."""
    v = codes.contiguous().view(torch.float8_e4m3fn).to(torch.float64)
    vb = v.reshape(*v.shape[:-1], -1, 32)
    return (vb * torch.exp2(scales.to(torch.float64) - 127)[..., None]).reshape(v.shape)


def quant_image(x_rows, groups=1):
    """fp32 rows [rows, G * C] -> the vidc_quant_mxfp8 image (uint8, G plane pairs of [rows][C] data + [rows][C / 32] scales)."""
    rows, ld = x_rows.shape
    C = ld // groups
    out = []
    for g in range(groups):
        codes, scales = quant_blocks(x_rows[:, g * C:(g + 1) * C])
        out += [codes.reshape(-1), scales.reshape(-1)]
    return torch.cat(out)


def dequant_image(img, rows, C, groups=1):
    """vidc_quant_mxfp8 image -> float64 [rows, G * C]."""
    per = rows * C // 32 * 33
    parts = []
    for g in range(groups):
        p = img[g * per:(g + 1) * per]
        parts.append(dequant_blocks(p[:rows * C].reshape(rows, C), p[rows * C:].reshape(rows, C // 32)))
    return torch.cat(parts, 1)


def packed_weight_order(w_oihw):
    """OIHW -> [Cout][K] in the MXFP8 conv's K order: [Cin/128][KH][KW][128] (float32, not quantised)."""
    co, ci, kh, kw = w_oihw.shape
    return w_oihw.reshape(co, ci // 128, 128, kh, kw).permute(0, 1, 3, 4, 2).reshape(co, -1).contiguous()


def pack_weight(w_oihw):
    """vidc_pack_conv_weight_mxfp8 emulated: uint8 [Cout * K] data then [Cout * K / 32] scales."""
    codes, scales = quant_blocks(packed_weight_order(w_oihw.float()))
    return torch.cat([codes.reshape(-1), scales.reshape(-1)])


def dequant_weight(w_oihw):
    """The weights the MXFP8 conv multiplies with, as float64 OIHW."""
    co, ci, kh, kw = w_oihw.shape
    codes, scales = quant_blocks(packed_weight_order(w_oihw.float()))
    v = dequant_blocks(codes, scales)
    return v.reshape(co, ci // 128, kh, kw, 128).permute(0, 1, 4, 2, 3).reshape(co, ci, kh, kw)
