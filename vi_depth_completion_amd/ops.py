"""Functional (tensor in -> tensor out) wrappers over single libvidc.so entry points.

The networks do not go through these (they run as whole `engine.Program`s); they exist so that every C entry
point can be exercised and parity-tested on its own, and for the plane block host code.  All tensors must be
CUDA/HIP tensors; nothing here computes on the CPU.
"""
import ctypes as C

import torch

from . import _lib as L


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("vidc ops take GPU tensors only (no CPU fallback)")


def pack_conv_weight(w_oihw):
    _dev(w_oihw)
    w = w_oihw.contiguous().float()
    co, ci, kh, kw = w.shape
    out = torch.empty((co, kh * kw * ci), dtype=torch.float32, device=w.device)
    L.check(L.lib().vidc_pack_conv_weight(L.ptr(w), L.ptr(out), co, ci, kh, kw, L.current_stream()), "pack_conv_weight")
    return out


def pack_conv_weight_bf16x3(w_oihw):
    """OIHW fp32 -> split-bf16 packed weights; returned as a float32-typed (Cout, K) tensor (same bytes: each 32-wide
    K unit is [32 x bf16 hi | 32 x bf16 lo])."""
    _dev(w_oihw)
    w = w_oihw.contiguous().float()
    co, ci, kh, kw = w.shape
    out = torch.empty((co, kh * kw * ci), dtype=torch.float32, device=w.device)
    L.check(L.lib().vidc_pack_conv_weight_bf16x3(L.ptr(w), L.ptr(out), co, ci, kh, kw, L.current_stream()), "pack_conv_weight_bf16x3")
    return out


def split_bf16x3(x_nhwc):
    """fp32 NHWC -> split-bf16 image of the same shape/bytes (float32-typed storage)."""
    _dev(x_nhwc)
    x = x_nhwc.contiguous().float()
    Cc = x.shape[-1]
    out = torch.empty_like(x)
    L.check(L.lib().vidc_split_bf16x3(L.ptr(x), L.ptr(out), x.numel() // Cc, Cc, Cc, L.current_stream()), "split_bf16x3")
    return out


def pack_conv_weight_bf16(w_oihw):
    """OIHW fp32 -> plain-bf16 packed weights for VIDC_PREC_BF16: bfloat16 (Cout, K), K order [Cin/64][KH][KW][64]; Cin % 64 == 0."""
    _dev(w_oihw)
    w = w_oihw.contiguous().float()
    co, ci, kh, kw = w.shape
    out = torch.empty((co, kh * kw * ci), dtype=torch.bfloat16, device=w.device)
    L.check(L.lib().vidc_pack_conv_weight_bf16(L.ptr(w), L.ptr(out), co, ci, kh, kw, L.current_stream()), "pack_conv_weight_bf16")
    return out


def cast_bf16(x_nhwc):
    """fp32 NHWC -> the plain-bf16 image of the same shape (round to nearest even): the operand of a VIDC_PREC_BF16 conv; channels % 8 == 0."""
    _dev(x_nhwc)
    x = x_nhwc.contiguous().float()
    Cc = x.shape[-1]
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    L.check(L.lib().vidc_cast_bf16(L.ptr(x), L.ptr(out), x.numel() // Cc, Cc, Cc, L.current_stream()), "cast_bf16")
    return out


def pack_conv_weight_mxfp8(w_oihw):
    """OIHW fp32 -> MXFP8 packed weights (include/vidc.h): uint8 (Cout * K * 33 / 32,), the e4m3 rows then their scale bytes."""
    _dev(w_oihw)
    w = w_oihw.contiguous().float()
    co, ci, kh, kw = w.shape
    out = torch.empty(co * kh * kw * ci // 32 * 33, dtype=torch.uint8, device=w.device)
    L.check(L.lib().vidc_pack_conv_weight_mxfp8(L.ptr(w), L.ptr(out), co, ci, kh, kw, L.current_stream()), "pack_conv_weight_mxfp8")
    return out


def quant_mxfp8(x_nhwc, groups=1):
    """fp32 NHWC (..., G*C) -> MXFP8 image (include/vidc.h): uint8 (G * rows * C * 33 / 32,), per group the e4m3 rows then their scales."""
    _dev(x_nhwc)
    x = x_nhwc.contiguous().float()
    ld = x.shape[-1]
    rows = x.numel() // ld
    out = torch.empty(rows * ld // 32 * 33, dtype=torch.uint8, device=x.device)
    L.check(L.lib().vidc_quant_mxfp8(L.ptr(x), L.ptr(out), rows, ld // groups, ld, groups, L.current_stream()), "quant_mxfp8")
    return out


def conv2d_bn_act(x, w_packed, scale1, shift1, kh, kw, stride=1, pad=0, relu1=False, scale2=None, shift2=None, relu2=False,
                  residual=None, relu3=False, accumulate_into=None, tile=0, splitk=1, groups=1, precision=0, split_out=None,
                  no_f32_out=False, workspace=None, dilation=1, mx_out=None, bf16_out=None):
    """x: NHWC (B,H,W,G*Cin) contiguous; w_packed: (G,Cout,kh*kw*Cin) or (Cout,K); returns NHWC (B,Ho,Wo,G*Cout).
    precision=1 (bf16x3): x is split here; w_packed must come from pack_conv_weight_bf16x3.
    precision=2 (plain bf16): x is cast here; w_packed: the pack_conv_weight_bf16 images of the G groups, concatenated (Cin % 64 == 0).
    bf16_out: bfloat16 tensor of y's shape receiving the bf16 image of the result (VIDC_BF16_OUT, precision 2 only).
    precision=3 (MXFP8): x is quantised here; w_packed: the pack_conv_weight_mxfp8 images of the G groups, concatenated.
    mx_out: uint8 tensor of G * B*Ho*Wo * Cout * 33 / 32 bytes receiving the MXFP8 image of the result (VIDC_MXFP8_OUT).
    workspace: optional persistent split-K scratch (float32, zero-initialised once by the caller; include/vidc.h)."""
    _dev(x, w_packed, scale1, shift1)
    x = x.contiguous()
    B, H, W, ld = x.shape
    G = groups
    cin = ld // G
    if precision == L.PREC_BF16X3:
        x = split_bf16x3(x)
    elif precision == L.PREC_BF16:
        x = cast_bf16(x)
    elif precision == L.PREC_MXFP8:
        x = quant_mxfp8(x, G)
    if precision == L.PREC_BF16:
        wp = w_packed.contiguous()
        cout = wp.numel() // (G * kh * kw * cin)
        assert wp.dtype == torch.bfloat16 and wp.numel() == G * cout * kh * kw * cin
    elif precision == L.PREC_MXFP8:
        wp = w_packed.contiguous()
        cout = wp.numel() // G // (kh * kw * cin // 32 * 33)
        assert wp.numel() == G * cout * kh * kw * cin // 32 * 33
    else:
        wp = w_packed.contiguous().view(G, -1, kh * kw * cin)
        cout = wp.shape[1]
    Ho, Wo = (H + 2 * pad - dilation * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dilation * (kw - 1) - 1) // stride + 1
    y = accumulate_into if accumulate_into is not None else torch.empty((B, Ho, Wo, G * cout), dtype=torch.float32, device=x.device)
    s1, b1 = scale1.contiguous().float(), shift1.contiguous().float()
    s2, b2 = (scale2.contiguous().float(), shift2.contiguous().float()) if scale2 is not None else (None, None)
    residual = residual.contiguous() if residual is not None else None
    if mx_out is not None:
        assert mx_out.dtype == torch.uint8 and mx_out.numel() >= G * B * Ho * Wo * cout // 32 * 33
    if bf16_out is not None:
        assert bf16_out.dtype == torch.bfloat16 and bf16_out.is_contiguous() and bf16_out.numel() >= B * Ho * Wo * G * cout
    d = L.conv_desc(B, H, W, cin, cout, kh, kw, stride, pad, dilation, G, Ho, Wo, precision=precision, x=L.ptr(x), w=L.ptr(wp), y=L.ptr(y),
                    scale1=L.ptr(s1), shift1=L.ptr(b1), shared_affine=s1.numel() < G * cout, scale2=L.ptr(s2), shift2=L.ptr(b2),
                    relu1=relu1, relu2=relu2, residual=L.ptr(residual), ldr=residual.shape[-1] if residual is not None else None, relu3=relu3,
                    accumulate=accumulate_into is not None, split_out=L.ptr(split_out), mx_out=L.ptr(mx_out), no_f32_out=no_f32_out,
                    bf16_out=L.ptr(bf16_out))
    _launch(d, x.device, tile, splitk, workspace, "conv2d_bn_act")
    return y


def _launch(d, device, tile, splitk, workspace, what):
    """Tiles `d` -- (tile, splitk), or for tile 0 the planner's tile, with `splitk` kept where it is > 1 -- and launches it, with the
    caller's split-K workspace or a fresh zeroed one where it needs one."""
    L.plan(d, (tile, splitk) if tile else None)
    if not tile and splitk > 1:
        d.splitk = splitk
    ws = None
    nbytes = L.lib().vidc_conv2d_workspace_bytes(C.byref(d))
    if nbytes and workspace is not None:
        if workspace.numel() * 4 < nbytes:
            raise RuntimeError("split-K workspace too small: %d < %d bytes" % (workspace.numel() * 4, nbytes))
        d.workspace = L.ptr(workspace)
    elif nbytes:
        ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)     # zeroed: ticket counters at its head
        d.workspace = L.ptr(ws)
    L.check(L.lib().vidc_conv2d_bn_act(C.byref(d), L.current_stream()), what)


def stem_conv3x3s2(x_nchw, w_oihw, relu=True, split_out=None):
    """split_out: optional float32-typed tensor of y's shape receiving the split-bf16 image of the result (Cout % 32 == 0)."""
    _dev(x_nchw, w_oihw)
    x, w = x_nchw.contiguous().float(), w_oihw.contiguous().float()
    B, cin, H, W = x.shape
    co = w.shape[0]
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((B, Ho, Wo, co), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_stem_conv3x3s2(L.ptr(x), L.ptr(w), L.ptr(y), B, cin, H, W, co, co, int(relu), L.ptr(split_out), 0,
                                        L.current_stream()), "stem")
    return y


def stem_conv3x3s2_warped(x_nchw, warp_params, w_oihw, cx, cy, align_corners=False, relu=True):
    """The stem conv on the gravity-aligned forward warp of x, gathered on the fly (the warped image is never stored)."""
    _dev(x_nchw, warp_params, w_oihw)
    x, w = x_nchw.contiguous().float(), w_oihw.contiguous().float()
    B, cin, H, W = x.shape
    assert cin == 3
    co = w.shape[0]
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((B, Ho, Wo, co), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_stem_conv3x3s2_warped(L.ptr(x), L.ptr(warp_params), L.ptr(w), L.ptr(y), B, H, W, co, co, int(relu), None, 0, float(cx), float(cy),
                                               int(align_corners), L.current_stream()), "stem (warped input)")
    return y


def maxpool3x3s2(x, split_out=None):
    _dev(x)
    x = x.contiguous()
    B, H, W, Cc = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_maxpool3x3s2(L.ptr(x), L.ptr(y), B, H, W, Cc, Cc, Cc, L.ptr(split_out), L.current_stream()), "maxpool")
    return y


def upsample_bilinear_ac(x, size, relu=False, accumulate_into=None, split_out=None, store_f32=True, sum_groups=1):
    """sum_groups = G > 1: x holds G groups of C/G channels; their upsampled (ReLU'd) values are added into accumulate_into (C/G ch)."""
    _dev(x)
    x = x.contiguous()
    B, h, w, Cc = x.shape
    if sum_groups > 1:
        assert accumulate_into is not None and Cc % sum_groups == 0
        y = accumulate_into
        co = Cc // sum_groups
        flags = (L.UP_RELU if relu else 0) | L.UP_ACCUM | (sum_groups << 8)
        L.check(L.lib().vidc_upsample_bilinear_ac(L.ptr(x), L.ptr(y), B, h, w, co, Cc, size[0], size[1], co, flags, L.ptr(split_out),
                                                  L.current_stream()), "upsample")
        return y
    y = accumulate_into if accumulate_into is not None else torch.empty((B, size[0], size[1], Cc), dtype=torch.float32, device=x.device)
    flags = (L.UP_RELU if relu else 0) | (L.UP_ACCUM if accumulate_into is not None else 0) | (0 if store_f32 else L.UP_NO_F32_OUT)
    L.check(L.lib().vidc_upsample_bilinear_ac(L.ptr(x), L.ptr(y), B, h, w, Cc, Cc, size[0], size[1], Cc, flags, L.ptr(split_out),
                                              L.current_stream()), "upsample")
    return y


def head_conv1x1_upsample(x, w, bias, pad, size, relu):
    """x NHWC (B,h,w,Cin); w (Cout,Cin[,1,1]); returns (y NCHW (B,Cout,H,W), lowres NCHW (B,Cout,h+2p,w+2p))."""
    _dev(x, w, bias)
    x = x.contiguous()
    B, h, wd, cin = x.shape
    w2 = w.reshape(w.shape[0], -1).contiguous().float()
    co = w2.shape[0]
    low = torch.empty((B, co, h + 2 * pad, wd + 2 * pad), dtype=torch.float32, device=x.device)
    y = torch.empty((B, co, size[0], size[1]), dtype=torch.float32, device=x.device)
    b = bias.contiguous().float()
    L.check(L.lib().vidc_head_conv1x1_upsample(L.ptr(x), L.ptr(w2), L.ptr(b), L.ptr(low), L.ptr(y), B, h, wd, cin, cin, co, pad,
                                               size[0], size[1], int(relu), L.current_stream()), "head")
    return y, low


# ---- Winograd F(m x m, 3x3) (csrc/winograd.hip) ------------------------------------------------------------------------------
def winograd_weight_transform(w_oihw, m):
    """OIHW (Cout,Cin,3,3) -> U (a*a, Cout, Cin), a = m + 2."""
    _dev(w_oihw)
    w = w_oihw.contiguous().float()
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    a2 = (m + 2) * (m + 2)
    u = torch.empty((a2, co, ci), dtype=torch.float32, device=w.device)
    L.check(L.lib().vidc_winograd_weight_transform(L.ptr(w), L.ptr(u), co, ci, m, L.current_stream()), "winograd_weight_transform")
    return u


def winograd_input_transform(x, cin, m, split=False):
    """x NHWC (B,H,W,G*cin) -> V (tiles, G*a*a*cin) [tile][gg][pos][cin]; split=True: the split-bf16 image (float32-typed storage)."""
    _dev(x)
    x = x.contiguous()
    B, H, W, Cc = x.shape
    th, tw = -(-H // m), -(-W // m)
    a2 = (m + 2) * (m + 2)
    v = torch.empty((B * th * tw, a2 * Cc), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_winograd_input_transform(L.ptr(x), L.ptr(v), B, H, W, Cc, Cc, cin, m, int(split), 0, L.current_stream()),
            "winograd_input_transform")
    return v


def winograd_output_transform(mm, B, Ho, Wo, cout, m, scale1, shift1, relu1=False, scale2=None, shift2=None, relu2=False, split_out=None,
                              no_f32_out=False):
    """mm (tiles, G*a*a*cout) -> y NHWC (B,Ho,Wo,G*cout) = epilogue(A^T M A)."""
    _dev(mm, scale1, shift1)
    mm = mm.contiguous()
    a2 = (m + 2) * (m + 2)
    Cc = mm.shape[1] // a2
    y = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=mm.device)
    s1, b1 = scale1.contiguous().float().view(-1), shift1.contiguous().float().view(-1)
    flags = (L.RELU1 if relu1 else 0)
    s2 = b2 = None
    if scale2 is not None:
        s2, b2 = scale2.contiguous().float().view(-1), shift2.contiguous().float().view(-1)
        flags |= L.AFFINE2 | (L.RELU2 if relu2 else 0)
    if split_out is not None:
        flags |= L.SPLIT_OUT | (L.NO_F32_OUT if no_f32_out else 0)
    L.check(L.lib().vidc_winograd_output_transform(L.ptr(mm), L.ptr(y), L.ptr(split_out), L.ptr(s1), L.ptr(b1), L.ptr(s2), L.ptr(b2), B, Ho, Wo,
                                                   Cc, cout, Cc, m, flags, 0, L.current_stream()), "winograd_output_transform")
    return y


def conv3x3_winograd(x, w_oihw_groups, scale1, shift1, m, relu1=False, scale2=None, shift2=None, relu2=False, precision=0, tile=0, splitk=1,
                     split_out=None, no_f32_out=False):
    """nn.Conv2d(cin, cout, 3, 1, 1) [+ per-channel affines / ReLUs] of G groups as Winograd F(m x m, 3x3): input transform, ONE
    grouped 1x1 GEMM launch (a*a*G groups, identity epilogue) on the MFMA kernel, output transform with the epilogue.
    x NHWC (B,H,W,G*cin); w_oihw_groups: list of G (cout,cin,3,3) tensors; scale / shift: (G, cout)."""
    if precision not in (L.PREC_FP32, L.PREC_BF16X3):
        raise RuntimeError("conv3x3_winograd: precision %d has no Winograd form (fp32 = 0 and bf16x3 = 1 only; plain bf16 and MXFP8 run the direct "
                           "conv: the transforms amplify their rounding)" % precision)
    G = len(w_oihw_groups)
    B, H, W, Cc = x.shape
    cin = Cc // G
    cout = w_oihw_groups[0].shape[0]
    a2 = (m + 2) * (m + 2)
    u = torch.cat([winograd_weight_transform(w, m) for w in w_oihw_groups], 0)              # (G*a2, cout, cin): group gg*a2 + pos
    if precision == L.PREC_BF16X3:
        img = torch.empty_like(u)
        L.check(L.lib().vidc_pack_conv_weight_bf16x3(L.ptr(u), L.ptr(img), G * a2 * cout, cin, 1, 1, L.current_stream()), "pack")
        u = img
    v = winograd_input_transform(x, cin, m, split=precision == L.PREC_BF16X3)
    tiles = v.shape[0]
    mm = torch.empty((tiles, a2 * G * cout), dtype=torch.float32, device=x.device)
    one, zero = torch.ones(cout, dtype=torch.float32, device=x.device), torch.zeros(cout, dtype=torch.float32, device=x.device)
    d = L.gemm_desc(tiles, cin, cout, groups=a2 * G, precision=precision, x=L.ptr(v), w=L.ptr(u), y=L.ptr(mm), scale1=L.ptr(one), shift1=L.ptr(zero))
    _launch(d, x.device, tile, splitk, None, "conv2d_bn_act (winograd GEMMs)")
    return winograd_output_transform(mm, B, H, W, cout, m, scale1, shift1, relu1, scale2, shift2, relu2, split_out, no_f32_out)


def winograd_weight_pack_fused(u):
    """U (36, Cout, Cin) of winograd_weight_transform(w, 4) -> the fragment order the fused kernel streams (same shape / bytes, another order)."""
    _dev(u)
    u = u.contiguous().float()
    a2, co, ci = u.shape
    assert a2 == 36
    out = torch.empty_like(u)
    L.check(L.lib().vidc_winograd_weight_pack_fused(L.ptr(u), L.ptr(out), co, ci, L.current_stream()), "winograd_weight_pack_fused")
    return out


def conv3x3_winograd_fused(x, w_oihw_groups, scale1, shift1, relu1=False, scale2=None, shift2=None, relu2=False, u=None):
    """The same layer as conv3x3_winograd(m = 4) in ONE launch (csrc/wfused.hip, tile VIDC_TILE_WINO4_FUSED): input transform, the 36 products
    and the output transform + epilogue per block of 16 tiles x 32 output channels; no V / M tensors.  fp32 only.
    x NHWC (B,H,W,G*cin); w_oihw_groups: list of G (cout,cin,3,3) tensors (or `u`: their transformed AND packed weights, (G*36,cout,cin) floats); scale / shift: (G, cout)."""
    _dev(x, scale1, shift1)
    x = x.contiguous()
    G = len(w_oihw_groups) if u is None else u.shape[0] // 36
    B, H, W, Cc = x.shape
    cin = Cc // G
    if u is None:
        u = torch.cat([winograd_weight_pack_fused(winograd_weight_transform(w, 4)) for w in w_oihw_groups], 0)      # (G*36, cout, cin) floats, fragment order
    cout = u.shape[1]
    y = torch.empty((B, H, W, G * cout), dtype=torch.float32, device=x.device)
    s1, b1 = scale1.contiguous().float().view(-1), shift1.contiguous().float().view(-1)
    s2, b2 = (scale2.contiguous().float().view(-1), shift2.contiguous().float().view(-1)) if scale2 is not None else (None, None)
    d = L.conv_desc(B, H, W, cin, cout, 3, 3, 1, 1, groups=G, x=L.ptr(x), w=L.ptr(u), y=L.ptr(y), scale1=L.ptr(s1), shift1=L.ptr(b1),
                    shared_affine=s1.numel() < G * cout, scale2=L.ptr(s2), shift2=L.ptr(b2), relu1=relu1, relu2=relu2, wino_fused=True)
    L.check(L.lib().vidc_conv2d_bn_act(C.byref(d), L.current_stream()), "conv2d_bn_act (fused Winograd)")
    return y


def clock_stamps(n, device=None):
    """Buffer for n stamps of `clock_stamp`."""
    return torch.zeros((n, L.CLOCK_STAMP_WGS, 4), dtype=torch.int64, device=device if device is not None else "cuda")


def clock_stamp(stamps, i):
    """Enqueues stamp i on the current stream (include/vidc.h vidc_clock_stamp): per XCD the shader-clock cycle counter and the 100 MHz wall
    clock.  `shader_clock_ghz(stamps, a, b)` turns two stamps into the average shader clock between them."""
    if not stamps.is_cuda or stamps.dtype != torch.int64 or tuple(stamps.shape[1:]) != (L.CLOCK_STAMP_WGS, 4) or not stamps.is_contiguous():
        raise RuntimeError("clock_stamp: a buffer made by ops.clock_stamps is required")
    L.check(L.lib().vidc_clock_stamp(stamps.data_ptr() + 8 * 4 * L.CLOCK_STAMP_WGS * int(i), L.current_stream()), "clock_stamp")


def shader_clock_ghz(stamps, a, b):
    """Median over the XCDs present in both stamps of (cycle difference) / (100 MHz tick difference) x 0.1; None if they share no XCD."""
    h = stamps.cpu()
    sa = {int(r[0]): (int(r[1]), int(r[2])) for r in h[a] if int(r[3]) == 1}
    sb = {int(r[0]): (int(r[1]), int(r[2])) for r in h[b] if int(r[3]) == 1}
    ghz = sorted((sb[x][0] - sa[x][0]) / (sb[x][1] - sa[x][1]) * 0.1 for x in sa if x in sb and sb[x][1] > sa[x][1] and sb[x][0] > sa[x][0])
    return ghz[len(ghz) // 2] if ghz else None


# ---- backward of the per-op surface (torch_ops.py registers these as the autograd formulas of torch.ops.vidc.*) ------------------------
def _scratch(nbytes, device):
    return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)


def _warp_call(entry, tensors, params, tail, channels=True):
    """One warp entry of libvidc.so on NCHW float images: entry(tensors..., params, out, B, [C,] H, W, *tail, stream).  channels=False: the entry
    takes no C (the 3-channel inverse warp).  Returns out, shaped like the images."""
    _dev(*tensors, params)
    tensors = [t.contiguous().float() for t in tensors]
    B, Cc, H, W = tensors[0].shape
    out = torch.empty_like(tensors[0])
    dims = (B, Cc, H, W) if channels else (B, H, W)
    L.check(getattr(L.lib(), entry)(*[L.ptr(t) for t in tensors], L.ptr(params), L.ptr(out), *dims, *tail, L.current_stream()), entry[len("vidc_"):])
    return out


def warp2dof_fwd_backward(dy, params, cx, cy, align_corners):
    """dx of vidc_warp2dof_fwd: dy (B,C,H,W), params the (B,32) record of vidc_warp2dof_params."""
    return _warp_call("vidc_warp2dof_fwd_backward", [dy], params, (float(cx), float(cy), int(align_corners)))


def warp2dof_inv_rot_norm_backward(x, dz, params, cx, cy, align_corners, normalize):
    """dx of vidc_warp2dof_inv_rot_norm: x the forward's input (B,3,H,W), dz the gradient of its output."""
    return _warp_call("vidc_warp2dof_inv_rot_norm_backward", [x, dz], params, (float(cx), float(cy), int(align_corners), int(normalize)), channels=False)


WARP_MODES = {"bilinear": 0, "nearest": 1, "bicubic": 2}      # VIDC_WARP_BILINEAR / _NEAREST / _BICUBIC: F.grid_sample's `mode` strings


def warp2dof_fwd_mode(x, params, cx, cy, align_corners, mode, rotate=False):
    """vidc_warp2dof_fwd_mode: the forward warp of x (B,C,H,W) in interpolation mode 0 / 1 / 2 (WARP_MODES); rotate (C == 3): z = Cg_R_C y per
    pixel.  params: the (B,32) record of vidc_warp2dof_params."""
    return _warp_call("vidc_warp2dof_fwd_mode", [x], params, (float(cx), float(cy), int(align_corners), int(mode), int(rotate)))


def warp2dof_fwd_mode_backward(dy, params, cx, cy, align_corners, mode, rotate=False):
    """dx of vidc_warp2dof_fwd_mode: dy (B,C,H,W), the gradient of its output."""
    return _warp_call("vidc_warp2dof_fwd_mode_backward", [dy], params, (float(cx), float(cy), int(align_corners), int(mode), int(rotate)))


def warp2dof_grids(params, H, W, cx, cy):
    """vidc_warp2dof_grids: (C_R_Cg (B,3,3), grid (B,H,W,2), inverse grid (B,H,W,2)) of the (B,32) records -- image_sampler_forward_inverse."""
    _dev(params)
    B = params.shape[0]
    grid = torch.empty((B, H, W, 2), dtype=torch.float32, device=params.device)
    inv_grid = torch.empty_like(grid)
    rot = torch.empty((B, 3, 3), dtype=torch.float32, device=params.device)
    L.check(L.lib().vidc_warp2dof_grids(L.ptr(params), L.ptr(grid), L.ptr(inv_grid), L.ptr(rot), B, int(H), int(W), float(cx), float(cy),
                                        L.current_stream()), "warp2dof_grids")
    return rot, grid, inv_grid


def affine_act_backward(dy, y, scale, shift, relu, c_raw=None, all_from_raw=False):
    """The conv epilogue y = relu?(c * scale + shift) transposed: (dc, dscale, dshift) from NHWC dy, y (vidc_affine_act_backward).  c_raw: the raw
    conv output, read for the channels whose scale is 0 or whose |shift| > 4 |scale| (torch_ops.affine_reads_raw) -- or, with all_from_raw, for
    every channel (ldc < 0 in the C call)."""
    _dev(dy, y, scale, shift, c_raw)
    dy, y = dy.contiguous().float(), y.contiguous()
    Cc = y.shape[-1]
    M = y.numel() // Cc
    s, b = scale.contiguous().float(), shift.contiguous().float()
    c_raw = c_raw.contiguous() if c_raw is not None else None
    dc = torch.empty_like(y)
    dscale, dshift = torch.empty_like(s), torch.empty_like(b)
    sc = _scratch(L.lib().vidc_train_scratch_bytes(M, Cc), y.device)
    L.check(L.lib().vidc_affine_act_backward(L.ptr(dy), L.ptr(y), L.ptr(c_raw), L.ptr(s), L.ptr(b), L.ptr(dc), L.ptr(dscale), L.ptr(dshift), M, Cc,
                                             Cc, Cc, -Cc if (all_from_raw and c_raw is not None) else Cc, Cc, int(relu), L.ptr(sc), L.current_stream()),
            "affine_act_backward")
    return dc, dscale, dshift


def pack_conv_weight_dgrad(w_oihw, precision=0):
    """OIHW -> the weights of the data-gradient conv (kernel flipped, channels transposed) in the format of `precision` (0 fp32, 1 bf16x3,
    2 plain bf16: a torch.bfloat16 tensor, pack kind 5 through vidc_pack_conv_weights_one -- the batched packer's kernel body with the descriptor
    as a kernel argument: one launch, no descriptor upload)."""
    _dev(w_oihw)
    w = w_oihw.contiguous().float()
    co, ci, kh, kw = w.shape
    if precision == L.PREC_BF16:
        out = torch.empty((ci, kh * kw * co), dtype=torch.bfloat16, device=w.device)
    else:
        out = torch.empty((ci, kh * kw * co), dtype=torch.float32, device=w.device)
    if precision == L.PREC_FP32:
        L.check(L.lib().vidc_pack_conv_weight_dgrad(L.ptr(w), L.ptr(out), co, ci, kh, kw, L.current_stream()), "pack_conv_weight_dgrad")
        return out
    if precision not in (L.PREC_BF16X3, L.PREC_BF16):
        raise RuntimeError("pack_conv_weight_dgrad: precision %d has no data-gradient form" % precision)
    kind = 3 if precision == L.PREC_BF16X3 else 5
    nb = L.lib().vidc_pack_item_blocks(co, ci, kh, kw, kind)
    if nb <= 0:
        if kind == 5:
            raise RuntimeError("conv weight %dx%dx%dx%d cannot be packed for the bf16 data gradient (Cout a multiple of 64, kernels up to 3x3)" % (co, ci, kh, kw))
        raise RuntimeError("conv weight %dx%dx%dx%d cannot be packed for the bf16x3 data gradient (Cout a multiple of 32, kernels up to 3x3)" % (co, ci, kh, kw))
    if kind == 5:
        L.check(L.lib().vidc_pack_conv_weights_one(L.ptr(w), L.ptr(out), co, ci, kh, kw, kind, L.current_stream()), "pack_conv_weights_one")
        return out
    item = (L.PackItem * 1)()
    item[0].w, item[0].packed, item[0].Cout, item[0].Cin, item[0].KH, item[0].KW, item[0].kind, item[0].block_begin = L.ptr(w), L.ptr(out), co, ci, kh, kw, kind, 0
    dev = torch.frombuffer(bytearray(bytes(item)), dtype=torch.uint8).to(w.device)
    L.check(L.lib().vidc_pack_conv_weights_batched(L.ptr(dev), 1, nb, L.current_stream()), "pack_conv_weights_batched")
    return out


def conv_backward_data_precision(w_shape, precision):
    """The arithmetic conv_backward_data runs at `precision` for a conv of weight shape (Cout, Cin, KH, KW) -- the one statement of the rule.
    Precision 2 (plain bf16) needs the conv kernel's bf16 operand geometry: Cout, the K side of the data-gradient conv, in whole 64-channel
    units that pack kind 5 can write (kernels up to 3x3), and Cin, its output side, a multiple of 32.  Any other conv takes its data gradient in
    exact fp32 (0), as at precision 0.  Precisions 0 and 1 are returned as they are."""
    co, ci, kh, kw = w_shape
    if precision != L.PREC_BF16:
        return precision
    return L.PREC_BF16 if ci % 32 == 0 and L.lib().vidc_pack_item_blocks(co, ci, kh, kw, 5) > 0 else L.PREC_FP32


def conv_backward_weight_precision(w_shape, precision, aligned=True):
    """The arithmetic conv_backward_weight runs at `precision` (0 or 2): 2, vidc_conv_wgrad_bf16, where Cin and Cout are multiples of 4 and
    both tensors start on a 16-byte boundary (`aligned`: its 16-byte loads; torch's own allocations do, a view at an odd storage offset may
    not); otherwise the fp32 kernel (0)."""
    co, ci, _kh, _kw = w_shape
    if precision not in (L.PREC_FP32, L.PREC_BF16):
        raise RuntimeError("conv_backward_weight: precision must be 0 (fp32) or 2 (bf16), got %r" % (precision,))
    return L.PREC_BF16 if precision == L.PREC_BF16 and ci % 4 == 0 and co % 4 == 0 and aligned else L.PREC_FP32


def conv_backward_data(dc, w_oihw, H, W, stride, pad, precision=0, dilation=1):
    """dx NHWC (B,H,W,Cin) of a conv from the gradient dc of its raw output: vidc_zero_stuff (stride > 1) + the conv kernel on the
    data-gradient weights, in the arithmetic of `precision` (the sequence DepthCompletionTrainer.conv records).  dilation > 1 (stride 1 only):
    the same conv kernel with the same dilation and pad' = dilation * (k - 1) - pad.  precision=2: the conv kernel at VIDC_PREC_BF16 on pack
    kind 5 weights, dc cast by conv2d_bn_act -- where conv_backward_data_precision allows it, else the fp32 data gradient of precision 0."""
    _dev(dc, w_oihw)
    dc = dc.contiguous()
    co, ci, kh, kw = w_oihw.shape
    precision = conv_backward_data_precision((co, ci, kh, kw), precision)
    B, Ho, Wo, _c = dc.shape
    if dilation != 1:
        if dilation < 1 or stride != 1 or kh != kw or dilation * (kh - 1) - pad < 0:
            raise RuntimeError("conv data gradient: unsupported geometry %dx%d stride %d pad %d dilation %d (a dilated conv must have stride 1, a square "
                               "kernel and pad <= dilation * (k-1))" % (kh, kw, stride, pad, dilation))
        if (Ho, Wo) != (H + 2 * pad - dilation * (kh - 1), W + 2 * pad - dilation * (kw - 1)):
            raise RuntimeError("conv data gradient: dc is %dx%d, a %dx%d conv of dilation %d and pad %d over %dx%d gives %dx%d"
                               % (Ho, Wo, kh, kw, dilation, pad, H, W, H + 2 * pad - dilation * (kh - 1), W + 2 * pad - dilation * (kw - 1)))
        one, zero = torch.ones(ci, dtype=torch.float32, device=dc.device), torch.zeros(ci, dtype=torch.float32, device=dc.device)
        return conv2d_bn_act(dc, pack_conv_weight_dgrad(w_oihw, precision), one, zero, kh, kw, stride=1, pad=dilation * (kh - 1) - pad, precision=precision,
                             dilation=dilation)
    if kh != kw or kh - 1 - pad < 0 or (stride > 1 and 2 * pad > kh - 1):
        raise RuntimeError("conv data gradient: unsupported geometry %dx%d stride %d pad %d (square kernels, pad <= k-1, and pad <= (k-1)/2 when strided)"
                           % (kh, kw, stride, pad))
    wd = pack_conv_weight_dgrad(w_oihw, precision)
    g = dc
    if stride > 1:
        g = torch.empty((B, H, W, co), dtype=torch.float32, device=dc.device)
        L.check(L.lib().vidc_zero_stuff(L.ptr(dc), L.ptr(g), B, Ho, Wo, co, co, stride, H, W, L.current_stream()), "zero_stuff")
    one, zero = torch.ones(ci, dtype=torch.float32, device=dc.device), torch.zeros(ci, dtype=torch.float32, device=dc.device)
    dx = conv2d_bn_act(g, wd, one, zero, kh, kw, stride=1, pad=kh - 1 - pad, precision=precision)
    if dx.shape[1] != H or dx.shape[2] != W:        # a strided conv whose padding is below "same": the rows / columns past the input are not its gradient
        dx = dx[:, :H, :W].contiguous()
    return dx


def conv_backward_weight(dc, x, w_shape, stride, pad, dilation=1, precision=0):
    """dw OIHW (fp32) from the gradient dc of the raw conv output and the conv's NHWC input (vidc_conv_wgrad; vidc_conv_wgrad_dilated when
    dilation != 1).  precision=2: vidc_conv_wgrad_bf16 (both operands rounded to bf16, fp32 accumulation) where
    conv_backward_weight_precision allows it, else the fp32 kernel."""
    _dev(dc, x)
    dc, x = dc.contiguous(), x.contiguous()
    co, ci, kh, kw = w_shape
    B, H, W, _c = x.shape
    _b, Ho, Wo, _co = dc.shape
    dw = torch.empty((co, ci, kh, kw), dtype=torch.float32, device=x.device)
    if conv_backward_weight_precision(w_shape, precision, aligned=dc.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0) == L.PREC_BF16:
        sc = _scratch(L.lib().vidc_conv_wgrad_bf16_scratch_bytes(B, Ho, Wo, co, ci, kh, kw), x.device)
        L.check(L.lib().vidc_conv_wgrad_bf16(L.ptr(dc), L.ptr(x), L.ptr(dw), B, H, W, ci, ci, Ho, Wo, co, co, kh, kw, stride, pad, dilation, L.ptr(sc),
                                             L.current_stream()), "conv_wgrad_bf16")
        return dw
    if dilation != 1:
        sc = _scratch(L.lib().vidc_conv_wgrad_dilated_scratch_bytes(B, Ho, Wo, co, ci, kh, kw), x.device)
        L.check(L.lib().vidc_conv_wgrad_dilated(L.ptr(dc), L.ptr(x), L.ptr(dw), B, H, W, ci, ci, Ho, Wo, co, co, kh, kw, stride, pad, dilation, L.ptr(sc),
                                                L.current_stream()), "conv_wgrad_dilated")
        return dw
    sc = _scratch(L.lib().vidc_conv_wgrad_scratch_bytes(B, Ho, Wo, co, ci, kh, kw), x.device)
    L.check(L.lib().vidc_conv_wgrad(L.ptr(dc), L.ptr(x), L.ptr(dw), B, H, W, ci, ci, Ho, Wo, co, co, kh, kw, stride, pad, L.ptr(sc), L.current_stream()),
            "conv_wgrad")
    return dw


def relu_backward(dy, y):
    """dy * (y > 0) for tensors of any shape (the kernel works on rows of four)."""
    _dev(dy, y)
    dy, y = dy.contiguous().float(), y.contiguous()
    n = dy.numel()
    if n % 4:
        pad = 4 - n % 4
        dy, y = torch.nn.functional.pad(dy.reshape(-1), (0, pad)), torch.nn.functional.pad(y.reshape(-1), (0, pad))
    out = torch.empty_like(dy)
    L.check(L.lib().vidc_relu_backward(L.ptr(dy), L.ptr(y), L.ptr(out), dy.numel() // 4, 4, 4, 4, 4, 0, L.current_stream()), "relu_backward")
    return out.reshape(-1)[:n].reshape(y.shape) if n % 4 else out


def stem_conv3x3s2_backward_data(dy, y, w_oihw, H, W, relu=True):
    """dx NCHW of stem_conv3x3s2; y: the forward output (read for the ReLU mask when relu)."""
    _dev(dy, y, w_oihw)
    dy, w = dy.contiguous().float(), w_oihw.contiguous().float()
    B, _ho, _wo, co = dy.shape
    cin = w.shape[1]
    y = y.contiguous() if relu else None
    dx = torch.empty((B, cin, H, W), dtype=torch.float32, device=dy.device)
    L.check(L.lib().vidc_stem_conv3x3s2_backward_data(L.ptr(dy), L.ptr(y), L.ptr(w), L.ptr(dx), B, cin, H, W, co, co, co, L.current_stream()),
            "stem_conv3x3s2_backward_data")
    return dx


def stem_conv3x3s2_backward_weight(dy, y, x_nchw, w_shape, relu=True):
    _dev(dy, y, x_nchw)
    x = x_nchw.contiguous().float()
    B, cin, H, W = x.shape
    co = w_shape[0]
    g = relu_backward(dy, y) if relu else dy.contiguous().float()
    dw = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    sc = _scratch(L.lib().vidc_stem_wgrad_scratch_bytes(B, cin, H, W, co), x.device)
    L.check(L.lib().vidc_stem_wgrad(L.ptr(g), L.ptr(x), L.ptr(dw), B, cin, H, W, co, co, L.ptr(sc), L.current_stream()), "stem_wgrad")
    return dw


def maxpool3x3s2_backward(dy, x):
    _dev(dy, x)
    dy, x = dy.contiguous().float(), x.contiguous()
    B, H, W, Cc = x.shape
    dx = torch.empty_like(x)
    L.check(L.lib().vidc_maxpool3x3s2_backward(L.ptr(x), L.ptr(dy), L.ptr(dx), B, H, W, Cc, Cc, Cc, Cc, L.current_stream()), "maxpool3x3s2_backward")
    return dx


def upsample_bilinear_ac_backward(dy, size_in, y=None):
    """dx NHWC (B,h,w,C) of upsample_bilinear_ac; y: the forward output when its ReLU was applied."""
    _dev(dy, y)
    dy = dy.contiguous().float()
    B, H, W, Cc = dy.shape
    if y is not None:
        dy = relu_backward(dy, y)
    dx = torch.empty((B, size_in[0], size_in[1], Cc), dtype=torch.float32, device=dy.device)
    L.check(L.lib().vidc_upsample_bilinear_ac_backward(L.ptr(dy), L.ptr(dx), B, size_in[0], size_in[1], Cc, Cc, Cc, H, W, L.current_stream()),
            "upsample_bilinear_ac_backward")
    return dx


def avgpool2d(x, kernel, stride, padding):
    """nn.AvgPool2d(kernel, stride, padding) with count_include_pad=True on NHWC (B,H,W,C), C % 4 == 0 (vidc_avgpool2d); kernel, stride and
    padding are (h, w) pairs."""
    _dev(x)
    x = x.contiguous().float()
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
    B, H, W, Cc = x.shape
    if min(kh, kw, sh, sw) < 1 or min(ph, pw) < 0 or H + 2 * ph < kh or W + 2 * pw < kw:
        raise RuntimeError("avgpool2d: bad geometry: kernel %s stride %s padding %s on a %dx%d map" % (kernel, stride, padding, H, W))
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    y = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_avgpool2d(L.ptr(x), L.ptr(y), B, H, W, Cc, Cc, kh, kw, sh, sw, ph, pw, Cc, L.current_stream()), "avgpool2d")
    return y


def avgpool2d_backward(dy, size_in, kernel, stride, padding):
    """dx NHWC (B,H,W,C) of avgpool2d from the gradient dy of its output; size_in = (H, W) (vidc_avgpool2d_backward)."""
    _dev(dy)
    dy = dy.contiguous().float()
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
    B, Ho, Wo, Cc = dy.shape
    H, W = size_in
    if min(kh, kw, sh, sw) < 1 or min(ph, pw) < 0 or H + 2 * ph < kh or W + 2 * pw < kw or (Ho, Wo) != ((H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1):
        raise RuntimeError("avgpool2d_backward: dy is %dx%d, which is not the pool of a %dx%d map with kernel %s stride %s padding %s"
                           % (Ho, Wo, H, W, kernel, stride, padding))
    dx = torch.empty((B, H, W, Cc), dtype=torch.float32, device=dy.device)
    L.check(L.lib().vidc_avgpool2d_backward(L.ptr(dy), L.ptr(dx), B, H, W, Cc, Cc, kh, kw, sh, sw, ph, pw, Cc, L.current_stream()), "avgpool2d_backward")
    return dx


def head_conv1x1_upsample_backward(dy, x, w, pad, y=None):
    """(dx NHWC, dw, dbias (Cout,)) of head_conv1x1_upsample for up to four output channels and pad 0 or 1: vidc_relu_backward (y: the forward
    output when relu), the upsample backward on the B * Cout one-channel planes, vidc_head_backward_multi."""
    _dev(dy, x, w, y)
    x = x.contiguous()
    B, h, wd, cin = x.shape
    w2 = w.reshape(w.shape[0], -1).contiguous().float()
    co = w2.shape[0]
    if not 1 <= co <= 4 or pad not in (0, 1):
        raise RuntimeError("head_conv1x1_upsample backward: 1 to 4 output channels and pad 0 or 1 only (got Cout %d, pad %d)" % (co, pad))
    dy = dy.contiguous().float()
    H, W = dy.shape[2], dy.shape[3]
    ph, pw = h + 2 * pad, wd + 2 * pad
    g = relu_backward(dy, y) if y is not None else dy
    g_low = torch.empty((B * co, ph, pw), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_upsample_bilinear_ac_backward(L.ptr(g), L.ptr(g_low), B * co, ph, pw, 1, 1, 1, H, W, L.current_stream()), "upsample_bilinear_ac_backward")
    dx = torch.empty_like(x)
    dw = torch.empty(w.shape, dtype=torch.float32, device=x.device)
    db = torch.empty((co,), dtype=torch.float32, device=x.device)
    sc = _scratch(L.lib().vidc_head_backward_multi_scratch_bytes(B, h, wd, cin, co, pad), x.device)
    L.check(L.lib().vidc_head_backward_multi(L.ptr(g_low), L.ptr(x), L.ptr(w2), L.ptr(dx), L.ptr(dw), L.ptr(db), B, h, wd, cin, cin, cin, co, pad, L.ptr(sc),
                                             L.current_stream()), "head_backward")
    return dx, dw, db


# ---- train-mode BatchNorm, Dropout2d, F.normalize's adjoint, the normal loss (torch.ops.vidc's TRAIN_OPS) ---------------------------------
def _rows(t):
    """(tensor, M, C, ld) of NHWC rows for the row kernels: `t` itself when it is a dense tensor or a channel slice of one (unit channel stride,
    rows `ld` floats apart, 16-byte aligned), else a dense copy."""
    Cc = t.shape[-1]
    M = t.numel() // Cc
    ok = t.dtype == torch.float32 and t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and t.dim() >= 2
    if ok and t.is_contiguous():
        return t, M, Cc, Cc
    if ok:
        ld = t.stride(-2)
        ok = ld >= Cc and ld % 4 == 0 and all(t.shape[i] == 1 or t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 2))
    if not ok:
        t = t.contiguous().float()
        ld = Cc
    return t, M, Cc, ld


def batch_norm_train(x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None):
    """(y, save_mean, save_rstd): y = relu?(BatchNorm2d_train(x) + residual) on NHWC rows (x, residual: dense or channel slices); running_mean /
    running_var are updated in place as nn.BatchNorm2d does (vidc_bn_train_forward_add)."""
    _dev(x, gamma, beta, running_mean, running_var, residual)
    x, M, Cc, ldx = _rows(x)
    if not (gamma.numel() == beta.numel() == running_mean.numel() == running_var.numel() == Cc):
        raise RuntimeError("batch_norm_train: %d channels, parameters of %d / %d / %d / %d" % (Cc, gamma.numel(), beta.numel(), running_mean.numel(), running_var.numel()))
    if not (running_mean.is_contiguous() and running_var.is_contiguous() and running_mean.dtype == running_var.dtype == torch.float32):
        raise RuntimeError("batch_norm_train: the running statistics are updated in place: dense float32 tensors")
    r, ldr = None, 0
    if residual is not None:
        if residual.shape != x.shape:
            raise RuntimeError("batch_norm_train: residual %s for x %s" % (tuple(residual.shape), tuple(x.shape)))
        r, _m, _c, ldr = _rows(residual)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    mean, rstd = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    sc = _scratch(L.lib().vidc_train_scratch_bytes(M, Cc), x.device)
    L.check(L.lib().vidc_bn_train_forward_add(L.ptr(x), L.ptr(y), M, Cc, ldx, Cc, L.ptr(gamma.contiguous().float()), L.ptr(beta.contiguous().float()),
                                              L.ptr(running_mean), L.ptr(running_var), eps, momentum, int(relu), L.ptr(mean), L.ptr(rstd), None, L.ptr(r), ldr,
                                              L.ptr(sc), L.current_stream()), "bn_train_forward")
    return y, mean, rstd


def batch_norm_train_backward(dy, x, y, gamma, save_mean, save_rstd, has_residual):
    """(dx, dgamma, dbeta, dresidual) of batch_norm_train.  y: the forward output when a ReLU followed, else None.  With a residual the ReLU sits
    behind the sum: vidc_relu_backward masks dy first, the masked gradient is dresidual and what the BatchNorm part starts from; without one the
    mask is applied inside vidc_bn_train_backward and dresidual comes back empty."""
    _dev(dy, x, y, gamma, save_mean, save_rstd)
    x, M, Cc, ldx = _rows(x)
    dy, _m, _c, lddy = _rows(dy)
    lib, st = L.lib(), L.current_stream()
    y_relu, ldy = None, 0
    dres = dy.new_empty(0)
    if y is not None:
        y_relu, _m, _c, ldy = _rows(y)
    if has_residual:
        dres = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        L.check(lib.vidc_relu_backward(L.ptr(dy), L.ptr(y_relu), L.ptr(dres), M, Cc, lddy, ldy, Cc, 0, st), "relu_backward")      # (y None: a copy)
        dy, lddy, y_relu, ldy = dres, Cc, None, 0
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dgamma, dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    sc = _scratch(lib.vidc_train_scratch_bytes(M, Cc), x.device)
    L.check(lib.vidc_bn_train_backward(L.ptr(dy), L.ptr(x), L.ptr(y_relu), L.ptr(dx), M, Cc, lddy, ldx, ldy, Cc, L.ptr(gamma.contiguous().float()),
                                       L.ptr(save_mean), L.ptr(save_rstd), L.ptr(dgamma), L.ptr(dbeta), None, L.ptr(sc), st), "bn_train_backward")
    return dx, dgamma, dbeta, dres


def _bn_eval_stats(what, Cc, gamma, beta, running_mean, running_var):
    """The four per-channel vectors of a frozen BatchNorm as dense float32 (the running statistics are only read: a copy is harmless)."""
    vs = [v for v in (gamma, beta, running_mean, running_var) if v is not None]
    if any(v.numel() != Cc for v in vs):
        raise RuntimeError("%s: %d channels, per-channel vectors of %s" % (what, Cc, " / ".join(str(v.numel()) for v in vs)))
    return [None if v is None else v.contiguous().float() for v in (gamma, beta, running_mean, running_var)]


def batch_norm_eval(x, gamma, beta, running_mean, running_var, eps, relu, residual=None):
    """y = relu?(BatchNorm2d_eval(x) + residual) on NHWC rows (x, residual: dense or channel slices): nn.BatchNorm2d in eval() mode, the running
    statistics read and left alone (vidc_bn_eval_forward_add, one launch)."""
    _dev(x, gamma, beta, running_mean, running_var, residual)
    x, M, Cc, ldx = _rows(x)
    gamma, beta, running_mean, running_var = _bn_eval_stats("batch_norm_eval", Cc, gamma, beta, running_mean, running_var)
    r, ldr = None, 0
    if residual is not None:
        if residual.shape != x.shape:
            raise RuntimeError("batch_norm_eval: residual %s for x %s" % (tuple(residual.shape), tuple(x.shape)))
        r, _m, _c, ldr = _rows(residual)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_bn_eval_forward_add(L.ptr(x), L.ptr(y), M, Cc, ldx, Cc, L.ptr(gamma), L.ptr(beta), L.ptr(running_mean), L.ptr(running_var), eps,
                                             int(relu), L.ptr(r), ldr, L.current_stream()), "bn_eval_forward")
    return y


def batch_norm_eval_backward(dy, x, y, gamma, running_mean, running_var, eps, has_residual, need_dx, need_affine):
    """(dx, dgamma, dbeta, dresidual) of batch_norm_eval; what nobody needs comes back empty and is not computed.  y: the forward output when a ReLU
    followed, else None; x: the forward input, read for dgamma only (None unless need_affine).  With a residual AND a ReLU the ReLU sits behind the
    sum: vidc_relu_backward masks dy first, the masked gradient is dresidual and what the BatchNorm part starts from.  Without a ReLU the masked
    gradient is dy itself and dresidual comes back empty (the caller hands dy on).  vidc_bn_eval_backward: need_affine -> the pass over the chunks
    that also writes dx, and the reduction; else one elementwise launch, no scratch."""
    _dev(dy, x, y, gamma, running_mean, running_var)
    dy, M, Cc, lddy = _rows(dy)
    gamma, _b, running_mean, running_var = _bn_eval_stats("batch_norm_eval_backward", Cc, gamma, None, running_mean, running_var)
    lib, st = L.lib(), L.current_stream()
    empty = lambda: dy.new_empty(0)              # noqa: E731  (one per output: the outputs of a custom operator must not alias each other)
    y_relu, ldy = None, 0
    if y is not None:
        y_relu, _m, _c, ldy = _rows(y)
    dres = empty()
    if has_residual and y_relu is not None:
        dres = torch.empty(dy.shape, dtype=torch.float32, device=dy.device)
        L.check(lib.vidc_relu_backward(L.ptr(dy), L.ptr(y_relu), L.ptr(dres), M, Cc, lddy, ldy, Cc, 0, st), "relu_backward")
        dy, lddy, y_relu, ldy = dres, Cc, None, 0
    if not (need_dx or need_affine):
        return empty(), empty(), empty(), dres
    xr, ldx, sc = None, 0, None
    dgamma, dbeta = empty(), empty()
    if need_affine:
        if x is None or x.shape != dy.shape:
            raise RuntimeError("batch_norm_eval_backward: dgamma needs the forward input x, shaped like dy")
        xr, _m, _c, ldx = _rows(x)
        dgamma, dbeta = torch.empty(Cc, dtype=torch.float32, device=dy.device), torch.empty(Cc, dtype=torch.float32, device=dy.device)
        sc = _scratch(lib.vidc_train_scratch_bytes(M, Cc), dy.device)
    dx = torch.empty(dy.shape, dtype=torch.float32, device=dy.device) if need_dx else empty()
    L.check(lib.vidc_bn_eval_backward(L.ptr(dy), L.ptr(xr), L.ptr(y_relu), L.ptr(dx) if need_dx else None, M, Cc, lddy, ldx, ldy, Cc, L.ptr(gamma),
                                      L.ptr(running_mean), L.ptr(running_var), eps, L.ptr(dgamma) if need_affine else None,
                                      L.ptr(dbeta) if need_affine else None, L.ptr(sc), st), "bn_eval_backward")
    return dx, dgamma, dbeta, dres


def dropout2d_mask(B, Cc, p, seed, offset, device):
    """keep (B, C): 0 or 1 / (1 - p) per (image, channel), Philox4x32-10 at (seed, offset) (vidc_dropout2d_mask)."""
    if not 0.0 <= p < 1.0:
        raise RuntimeError("dropout2d: p must be in [0, 1), got %r" % (p,))
    if seed < 0 or offset < 0:
        raise RuntimeError("dropout2d: seed and offset are unsigned 64-bit values")
    keep = torch.empty((B, Cc), dtype=torch.float32, device=device)
    L.check(L.lib().vidc_dropout2d_mask(L.ptr(keep), B, Cc, p, seed, offset, L.current_stream()), "dropout2d_mask")
    return keep


def scale_image_channels(x, keep):
    """y[b,h,w,c] = x[b,h,w,c] * keep[b][c] on NHWC (x: dense or a channel slice); vidc_scale_image_channels."""
    _dev(x, keep)
    B, Cc = x.shape[0], x.shape[-1]
    if tuple(keep.shape) != (B, Cc):
        raise RuntimeError("scale_image_channels: keep %s for x %s" % (tuple(keep.shape), tuple(x.shape)))
    x, M, _c, ldx = _rows(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_scale_image_channels(L.ptr(x), L.ptr(keep.contiguous().float()), L.ptr(y), B, M // B, Cc, ldx, Cc, L.current_stream()),
            "scale_image_channels")
    return y


def normalize_nchw(x):
    """F.normalize(x, dim=1) on NCHW (vidc_normalize_nchw)."""
    _dev(x)
    x = x.contiguous().float()
    B, Cc = x.shape[0], x.shape[1]
    y = torch.empty_like(x)
    L.check(L.lib().vidc_normalize_nchw(L.ptr(x), L.ptr(y), B, Cc, x.numel() // (B * Cc), L.current_stream()), "normalize_nchw")
    return y


def normalize_nchw_backward(x, dy):
    """dx of normalize_nchw (vidc_normalize_nchw_backward)."""
    _dev(x, dy)
    x, dy = x.contiguous().float(), dy.contiguous().float()
    B, Cc = x.shape[0], x.shape[1]
    dx = torch.empty_like(x)
    L.check(L.lib().vidc_normalize_nchw_backward(L.ptr(x), L.ptr(dy), L.ptr(dx), B, Cc, x.numel() // (B * Cc), L.current_stream()), "normalize_nchw_backward")
    return dx


def normal_l1_loss(pred, normal_gt, mask, normalize_prediction):
    """(sums float64 (3,) = loss, count, angle; dpred NCHW) of the masked L1 normal loss: one vidc_normal_l1_loss call."""
    _dev(pred, normal_gt, mask)
    pred, gt, m = pred.contiguous().float(), normal_gt.contiguous().float(), mask.contiguous().float()
    B, Cc, H, W = pred.shape
    if Cc != 3 or gt.shape != pred.shape or m.numel() != B * H * W:
        raise RuntimeError("normal_l1_loss: pred / normal_gt (B,3,H,W) and mask (B,[1,]H,W); got %s, %s, %s" % (tuple(pred.shape), tuple(gt.shape), tuple(mask.shape)))
    sums = torch.empty(3, dtype=torch.float64, device=pred.device)
    dpred = torch.empty_like(pred)
    sc = _scratch(L.lib().vidc_normal_l1_loss_scratch_bytes(B, H, W), pred.device)
    L.check(L.lib().vidc_normal_l1_loss(L.ptr(pred), L.ptr(gt), L.ptr(m), B, H, W, int(normalize_prediction), L.ptr(sums), L.ptr(sums[1:]), L.ptr(sums[2:]),
                                        L.ptr(dpred), L.ptr(sc), L.current_stream()), "normal_l1_loss")
    return sums, dpred


def scale_by_scalar(x, s):
    """x * s for a one-element device tensor s, as vidc_scale_image_channels over rows of four (the loss's upstream gradient times dpred)."""
    _dev(x, s)
    flat = x.contiguous().float().reshape(-1)
    n = flat.numel()
    if n % 4:
        flat = torch.nn.functional.pad(flat, (0, 4 - n % 4))
    k = s.reshape(1).float().expand(4).contiguous()
    y = torch.empty_like(flat)
    L.check(L.lib().vidc_scale_image_channels(L.ptr(flat), L.ptr(k), L.ptr(y), 1, flat.numel() // 4, 4, 4, 4, L.current_stream()), "scale_by_scalar")
    return y[:n].reshape(x.shape)


# ---- training ModifiedFPN / SurfaceNormalPrediction under autograd (torch.ops.vidc's NET_TRAIN_OPS) ------------------------------------------
def depth_l1_loss(pred, depth_gt):
    """(sums float64 (7,) = loss, count, ratios[5]; dpred shaped like pred) of the depth half of `_network_loss`: one vidc_depth_l1_loss call.  pred and
    depth_gt (B,1,H,W) or (B,H,W)."""
    _dev(pred, depth_gt)
    pred, gt = pred.contiguous().float(), depth_gt.contiguous().float()
    if pred.dim() < 2 or gt.numel() != pred.numel() or tuple(gt.shape[-2:]) != tuple(pred.shape[-2:]):
        raise RuntimeError("depth_l1_loss: pred and depth_gt (B,1,H,W) or (B,H,W) of one size; got %s, %s" % (tuple(pred.shape), tuple(depth_gt.shape)))
    H, W = pred.shape[-2:]
    B = pred.numel() // (H * W)
    sums = torch.empty(7, dtype=torch.float64, device=pred.device)
    dpred = torch.empty_like(pred)
    sc = _scratch(L.lib().vidc_depth_l1_loss_scratch_bytes(B, H, W), pred.device)
    L.check(L.lib().vidc_depth_l1_loss(L.ptr(pred), L.ptr(gt), B, H, W, L.ptr(sums), L.ptr(sums[1:]), L.ptr(sums[2:]), L.ptr(dpred), L.ptr(sc),
                                       L.current_stream()), "depth_l1_loss")
    return sums, dpred


def feature_mask_scale(x, image):
    """x NHWC (B,h,w,C) (dense or a channel slice) times the use_mask mask of surface_normal.py:151-162: (r + g + b > 1e-2) of image NCHW (B,3,H,W),
    nearest-resized to (h, w) (vidc_mask_scale; the mask is never stored)."""
    _dev(x, image)
    img = image.contiguous().float()
    if x.dim() != 4 or img.dim() != 4 or img.shape[1] != 3 or img.shape[0] != x.shape[0]:
        raise RuntimeError("feature_mask_scale: x NHWC (B,h,w,C) and image NCHW (B,3,H,W); got %s, %s" % (tuple(x.shape), tuple(image.shape)))
    B, h, w, Cc = x.shape
    x, _m, _c, ldx = _rows(x)
    y = torch.empty((B, h, w, Cc), dtype=torch.float32, device=x.device)
    L.check(L.lib().vidc_mask_scale(L.ptr(x), L.ptr(img), L.ptr(y), B, h, w, Cc, ldx, Cc, img.shape[2], img.shape[3], L.current_stream()), "mask_scale")
    return y


def add_rows(a, b, relu=False):
    """relu?(a + b) on NHWC rows (a, b: dense or channel slices); vidc_add_rows."""
    _dev(a, b)
    if a.shape != b.shape:
        raise RuntimeError("add_rows: a %s and b %s" % (tuple(a.shape), tuple(b.shape)))
    a, M, Cc, lda = _rows(a)
    b, _m, _c, ldb = _rows(b)
    y = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    L.check(L.lib().vidc_add_rows(L.ptr(a), L.ptr(b), L.ptr(y), M, Cc, lda, ldb, Cc, int(relu), L.current_stream()), "add_rows")
    return y


def relu_backward_rows(dy, y):
    """dy * (y > 0) on NHWC rows (dy, y: dense or channel slices) -> dense; vidc_relu_backward."""
    _dev(dy, y)
    dy, M, Cc, lddy = _rows(dy)
    y, _m, _c, ldy = _rows(y)
    out = torch.empty(dy.shape, dtype=torch.float32, device=dy.device)
    L.check(L.lib().vidc_relu_backward(L.ptr(dy), L.ptr(y), L.ptr(out), M, Cc, lddy, ldy, Cc, 0, L.current_stream()), "relu_backward")
    return out
