"""Thin torch-tensor wrappers over the kernel-level C entry points (used by tests, the eval harness and bench)."""
import ctypes as C

import torch

from . import lib as L


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


PREC = {None: 0, "f32": 1, "f16x3": 2, "bf16": 3}


def split16(w, scale=1.0):
    """fp16-split image of (an f32 cuda tensor * scale), numel % 4 == 0: what `gemm(..., prec="f16x3", w_split=scale)`
    consumes; scale is a power of two."""
    lib = L.load()
    w = w.contiguous()
    out = torch.empty_like(w)
    L.check(lib.actmi_op_split16(_p(w), _p(out), w.numel(), float(scale), L.current_stream_ptr()), None, "op_split16")
    return out


def permute_conv_k(w_rows, taps, cin):
    """[rows, ld] convolution weight rows, the first taps*cin columns re-ordered (tap, c) -> (c / 32, tap, c % 32): the K order
    the engine's split images use (actmi_gemm_desc.k_tap_inner)."""
    lib = L.load()
    w_rows = w_rows.contiguous()
    out = torch.empty_like(w_rows)
    rows, ld = w_rows.numel() // w_rows.shape[-1], w_rows.shape[-1]
    L.check(lib.actmi_op_permute_conv_k(_p(w_rows), _p(out), rows, int(taps), int(cin), int(ld), L.current_stream_ptr()), None,
            "op_permute_conv_k")
    return out


def pow2_scale(x):
    """[scale, scratch]: scale = the power of two that brings max|x| into [2^13, 2^14) (device-side, no host sync);
    pass the tensor as gemm(..., a_scale_dev=) / b_scale_dev= for operands far from the fp16 range."""
    lib = L.load()
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.zeros(2, dtype=torch.float32, device=x.device)
    L.check(lib.actmi_op_pow2_scale(_p(x), x.stride(0), x.shape[0], x.shape[1], _p(out), L.current_stream_ptr()), None,
            "op_pow2_scale")
    return out


def auto_splitk(M, N, K):
    """Split factor for a product whose grid is too small to fill 256 CUs while every workgroup walks a long contraction (the
    engine's rule for its own small-batch launches, engine.hip:ctx_gemm): aim at 1536 64x64-tile equivalents, keep >= 12 K
    tiles of 32 per split, at most 8 splits; 0 = do not split."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    nk = (K + 31) // 32
    if tiles >= 768 or nk < 24:
        return 0
    s = min(8, (1536 + tiles - 1) // tiles, nk // 12)
    while s >= 2 and (s - 1) * ((nk + s - 1) // s) >= nk:
        s -= 1
    return s if s >= 2 else 0


def gemm(A, W, bias=None, scale=None, res=None, res_mod=0, relu=False, a_add=None, add_mod=0, add_ncols=0, rowmap=None,
         out=None, out_rows=None, drop_p=0.0, drop_seed=0, prec=None, w_split=False, a_scale=0.0, b_scale=0.0,
         a_scale_dev=None, b_scale_dev=None, splitk=0, tile_hint=0):
    """out[rowmap(m)] = act((A' @ W.T) * scale + bias + res[m % res_mod]); A [M,K], W [N,K] row-major f32 cuda.
    tile_hint: actmi_gemm_desc.tile_hint (0 = chosen per launch shape, 1 = 128x128, 2 = 128x64, 3 = 64x64).
    splitk > 1: the contraction is split into that many plain slices which a combine pass sums in a fixed order before
    the epilogue (what the engine does for small grids); no rowmap / res_mod / dropout in that form."""
    lib = L.load()
    M, K = A.shape
    N = W.shape[0]
    if splitk == "auto":
        splitk = auto_splitk(M, N, K) if (rowmap is None and not res_mod and not drop_p and N % 4 == 0 and a_scale_dev is None
                                          and b_scale_dev is None) else 0
    if splitk and splitk > 1:
        assert rowmap is None and not res_mod and not drop_p
        part = torch.empty((splitk, M, N), dtype=torch.float32, device=A.device)
        d = L.GemmDesc()
        d.A, d.lda, d.mode = A.data_ptr(), A.stride(0), 0
        if a_add is not None:
            d.A_add, d.ld_add, d.add_mod, d.add_ncols = a_add.data_ptr(), a_add.stride(0), add_mod, add_ncols
        d.Bw, d.ldb = W.data_ptr(), W.stride(0)
        d.C, d.ldc = part.data_ptr(), N
        d.M, d.N, d.K, d.groups = M, N, K, 1
        d.splitk, d.split_stride = int(splitk), M * N
        d.prec, d.b_split, d.b_scale = PREC[prec], 1 if w_split else 0, float(w_split) if w_split else float(b_scale)
        d.a_scale = float(a_scale)
        d.tile_hint = int(tile_hint)
        L.check(lib.actmi_op_gemm(C.byref(d), L.current_stream_ptr()), None, "op_gemm")
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=A.device)
        L.check(lib.actmi_op_splitk_combine(part.data_ptr(), int(splitk), M * N, N, M, N, _p(scale), _p(bias), _p(res),
                                            res.stride(0) if res is not None else 0,
                                            2 if relu == "gelu" else (1 if relu else 0), out.data_ptr(), out.stride(0),
                                            L.current_stream_ptr()), None, "op_splitk_combine")
        return out
    if out is None:
        out = torch.zeros((out_rows or M, N), dtype=torch.float32, device=A.device)
    d = L.GemmDesc()
    d.A, d.lda, d.mode = A.data_ptr(), A.stride(0), 0
    if a_add is not None:
        d.A_add, d.ld_add, d.add_mod, d.add_ncols = a_add.data_ptr(), a_add.stride(0), add_mod, add_ncols
    d.Bw, d.ldb = W.data_ptr(), W.stride(0)
    d.scale = scale.data_ptr() if scale is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        d.res, d.ldres, d.res_mod = res.data_ptr(), res.stride(0), res_mod
    d.relu = 2 if relu == "gelu" else (1 if relu else 0)
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.rowmap = rowmap.data_ptr() if rowmap is not None else None
    d.M, d.N, d.K, d.groups = M, N, K, 1
    d.drop_p, d.drop_seed = float(drop_p), int(drop_seed)
    d.prec, d.b_split, d.b_scale = PREC[prec], 1 if w_split else 0, float(w_split) if w_split else float(b_scale)
    d.a_scale = float(a_scale)
    d.a_scale_dev = a_scale_dev.data_ptr() if a_scale_dev is not None else None
    d.b_scale_dev = b_scale_dev.data_ptr() if b_scale_dev is not None else None
    d.tile_hint = int(tile_hint)
    L.check(lib.actmi_op_gemm(C.byref(d), L.current_stream_ptr()), None, "op_gemm")
    return out


def conv2d_with_second_source(y1, x, wf_split, w_scale, bias, stride_x=2, relu=True, splitk=0, k_tap_inner=False, tile_hint=0):
    """A ResNet block's conv2 with the block's 1x1 / stride-2 downsample branch in the same contraction (gemm.hip second
    source): y1 [G,B,H,W,C] is convolved 3x3 / s1 / p1, x [G,B,Hx,Wx,Cx] joins at stride_x as extra columns of the contraction.
    wf_split: split16 image (built with w_scale) of [G][Cout][9*C + Cx]; bias [G,Cout].  f16x3 only.  tile_hint as in gemm.
    Returns [G,B,H,W,Cout]."""
    lib = L.load()
    G, B, H, W, Cc = y1.shape
    _, _, Hx, Wx, Cx = x.shape
    Cout = wf_split.shape[1]
    Kf = 9 * Cc + Cx
    assert wf_split.numel() == G * Cout * Kf
    M = B * H * W

    def desc(C_ptr, ldc, gC):
        d = L.GemmDesc()
        d.A, d.mode = y1.data_ptr(), 1
        d.H, d.W, d.Cin, d.KH, d.KW, d.stride, d.pad, d.Ho, d.Wo = H, W, Cc, 3, 3, 1, 1, H, W
        d.img_stride = H * W * Cc
        d.Ax, d.kx_begin, d.Hx, d.Wx, d.Cx, d.stride_x, d.gAx = x.data_ptr(), 9 * Cc, Hx, Wx, Cx, stride_x, B * Hx * Wx * Cx
        d.Bw, d.ldb = wf_split.data_ptr(), Kf
        d.C, d.ldc = C_ptr, ldc
        d.M, d.N, d.K, d.groups = M, Cout, Kf, G
        d.gA, d.gB, d.gSB, d.gC = B * H * W * Cc, Cout * Kf, Cout, gC
        d.prec, d.b_split, d.b_scale = PREC["f16x3"], 1, float(w_scale)
        d.k_tap_inner = 1 if k_tap_inner else 0
        d.tile_hint = int(tile_hint)
        return d
    out = torch.empty((G, B, H, W, Cout), dtype=torch.float32, device=y1.device)
    if splitk and splitk > 1:
        part = torch.empty((G, splitk, M, Cout), dtype=torch.float32, device=y1.device)
        d = desc(part.data_ptr(), Cout, splitk * M * Cout)
        d.splitk, d.split_stride = int(splitk), M * Cout
        L.check(lib.actmi_op_gemm(C.byref(d), L.current_stream_ptr()), None, "op_gemm(conv + second source, split)")
        for g in range(G):
            L.check(lib.actmi_op_splitk_combine(part[g].data_ptr(), int(splitk), M * Cout, Cout, M, Cout, None, _p(bias[g]), None, 0,
                                                1 if relu else 0, out[g].data_ptr(), Cout, L.current_stream_ptr()), None, "combine")
        return out
    d = desc(out.data_ptr(), Cout, M * Cout)
    d.bias = bias.data_ptr()
    d.relu = 1 if relu else 0
    L.check(lib.actmi_op_gemm(C.byref(d), L.current_stream_ptr()), None, "op_gemm(conv + second source)")
    return out


def conv2d_nhwc(x, w_ohwi, scale=None, bias=None, res=None, relu=False, stride=1, pad=1, prec=None, w_split=False, b_scale=0.0,
                k_tap_inner=False, tile_hint=0):
    """x [G,B,H,W,Cin] camera-major NHWC; w_ohwi [G,Cout,KH,KW,Cin]; scale/bias [G,Cout]; returns [G,B,Ho,Wo,Cout].
    k_tap_inner: the rows of w_ohwi were re-ordered by permute_conv_k (channel blocks outer, taps inner); tile_hint as in gemm."""
    lib = L.load()
    G, B, H, W, Cin = x.shape
    _, Cout, KH, KW, _ = w_ohwi.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    out = torch.empty((G, B, Ho, Wo, Cout), dtype=torch.float32, device=x.device)     # every element is written (no split-K here)
    d = L.GemmDesc()
    d.A, d.mode = x.data_ptr(), 1
    d.H, d.W, d.Cin, d.KH, d.KW, d.stride, d.pad, d.Ho, d.Wo = H, W, Cin, KH, KW, stride, pad, Ho, Wo
    d.img_stride = H * W * Cin
    d.Bw, d.ldb = w_ohwi.data_ptr(), KH * KW * Cin
    d.scale = scale.data_ptr() if scale is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        d.res, d.ldres = res.data_ptr(), Cout
    d.relu = 1 if relu else 0
    d.C, d.ldc = out.data_ptr(), Cout
    d.M, d.N, d.K, d.groups = B * Ho * Wo, Cout, KH * KW * Cin, G
    d.gA, d.gB, d.gSB = B * H * W * Cin, Cout * KH * KW * Cin, Cout
    d.gC = d.gRes = B * Ho * Wo * Cout
    # f16x3: w_split = scale of a pre-split weight image; b_scale = power-of-two scale applied to plain fp32 weights on the fly
    d.prec, d.b_split, d.b_scale = PREC[prec], 1 if w_split else 0, float(w_split) if w_split else float(b_scale)
    d.k_tap_inner = 1 if k_tap_inner else 0
    d.tile_hint = int(tile_hint)
    L.check(lib.actmi_op_gemm(C.byref(d), L.current_stream_ptr()), None, "op_gemm(conv)")
    return out


def sample_onehot(logits, temperature=1.0, seed=0, want_probs=False):
    """one categorical draw per row of logits [n, V] -> one-hot [n, V] (device-side inverse CDF, counter-based generator)."""
    lib = L.load()
    logits = logits.contiguous()
    n, V = logits.shape
    code = torch.empty_like(logits)
    probs = torch.empty_like(logits) if want_probs else None
    L.check(lib.actmi_op_sample_onehot(_p(logits), n, V, float(temperature), C.c_uint64(int(seed)), _p(probs), _p(code),
                                       L.current_stream_ptr()), None, "op_sample_onehot")
    return (code, probs) if want_probs else code


def conv1_prepare(w_oihw, lut_mode=1):
    """prepared stem weights (actmi_op_conv1_prepare): w_oihw [C, Cout, 3, 7, 7]; lut_mode 0 = the ACT path's ImageNet
    normalisation of the u8 pixels, 1 = v / 255 only.  Returns the workspace tensor to hand to conv1_prepared."""
    lib = L.load()
    w_oihw = w_oihw.contiguous()
    Cc, Cout = w_oihw.shape[0], w_oihw.shape[1]
    ws = torch.zeros(int(lib.actmi_op_conv1_workspace_floats(Cc, Cout)), dtype=torch.float32, device=w_oihw.device)
    L.check(lib.actmi_op_conv1_prepare(_p(w_oihw), _p(ws), Cc, Cout, int(lut_mode), L.current_stream_ptr()), None, "op_conv1_prepare")
    return ws


def conv1_prepared(image, ws, Cout, relu=False, scale=None, bias=None, vpool=False, cam0=0, ncam=0, out=None, prec=None):
    """the 7x7 / s2 stem on prepared weights (actmi_op_conv1_prepared_ex): image u8 [B, C, H, W, 3] or f32 [B, C, 3, H, W] (the
    f32 form is ImageNet-normalised in the loader) -> [C, B, Ho, Wo, Cout], or [C, B, Ho/2, Wo, Cout] under vpool (max over conv
    rows 2a-1, 2a, 2a+1); launch only.  cam0 / ncam: compute that camera range only, into the whole-tensor `out` given."""
    lib = L.load()
    image = image.contiguous()
    if image.dtype == torch.uint8:
        B, Cc, H, W, _ = image.shape
        fmt = L.IMG_U8_NHWC
    elif image.dtype == torch.float32:
        B, Cc, _, H, W = image.shape
        fmt = L.IMG_F32_NCHW
    else:
        raise TypeError(f"conv1_prepared: image dtype {image.dtype} not supported (uint8 or float32)")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    shape = (Cc, B, Ho // 2 if vpool else Ho, Wo, Cout)
    if out is None:
        if ncam:
            raise ValueError("conv1_prepared: a camera range writes into a caller-supplied whole-tensor out")
        out = torch.empty(shape, dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"conv1_prepared: out must be a contiguous float32 tensor of shape {shape}")
    L.check(lib.actmi_op_conv1_prepared_ex(_p(image), fmt, _p(ws), _p(scale), _p(bias), _p(out), B, Cc, H, W, Cout, 1 if relu else 0,
                                           1 if vpool else 0, int(cam0), int(ncam), PREC[prec], L.current_stream_ptr()),
            None, "op_conv1_prepared")
    return out


def conv1_seam_floats(B, Cc, H, W, Cout):
    """floats of the seam workspace conv1_pooled needs for frames of H x W (0 when the conv map is at most 64 columns wide)"""
    return int(L.load().actmi_op_conv1_seam_floats(int(B), int(Cc), int(H), int(W), int(Cout)))


def conv1_pooled(image, ws, Cout, relu=True, scale=None, bias=None, cam0=0, ncam=0, out=None, seam="auto", prec=None):
    """the 7x7 / s2 stem with the whole 3x3 / s2 / p1 max pool fused (actmi_op_conv1_pooled): image as conv1_prepared ->
    [C, B, Ho/2, (Wo-1)//2+1, Cout], bit-equal to hpool(conv1_prepared(..., vpool=True)); launch only.  seam: the float32
    workspace of at least conv1_seam_floats(...) elements that a conv map wider than 64 columns needs ("auto": allocated
    here; None: none is passed).  cam0 / ncam: compute that camera range only, into the whole-tensor `out` (and `seam`) given."""
    lib = L.load()
    image = image.contiguous()
    if image.dtype == torch.uint8:
        B, Cc, H, W, _ = image.shape
        fmt = L.IMG_U8_NHWC
    elif image.dtype == torch.float32:
        B, Cc, _, H, W = image.shape
        fmt = L.IMG_F32_NCHW
    else:
        raise TypeError(f"conv1_pooled: image dtype {image.dtype} not supported (uint8 or float32)")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    shape = (Cc, B, Ho // 2, (Wo - 1) // 2 + 1, Cout)
    if out is None:
        if ncam:
            raise ValueError("conv1_pooled: a camera range writes into a caller-supplied whole-tensor out")
        out = torch.empty(shape, dtype=torch.float32, device=image.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"conv1_pooled: out must be a contiguous float32 tensor of shape {shape}")
    if isinstance(seam, str):
        n = conv1_seam_floats(B, Cc, H, W, Cout)
        seam = torch.empty(n, dtype=torch.float32, device=image.device) if n else None
    elif seam is not None and (seam.dtype != torch.float32 or not seam.is_contiguous()):
        raise ValueError("conv1_pooled: seam must be a contiguous float32 tensor")
    L.check(lib.actmi_op_conv1_pooled(_p(image), fmt, _p(ws), _p(scale), _p(bias), _p(out), _p(seam), seam.numel() if seam is not None else 0,
                                      B, Cc, H, W, Cout, 1 if relu else 0, int(cam0), int(ncam), PREC[prec], L.current_stream_ptr()),
            None, "op_conv1_pooled")
    return out


def hpool(x):
    """horizontal half of the 3x3 / s2 / p1 max pool: x [..., W, C] NHWC rows -> [..., Wo, C], max over columns 2pw-1 .. 2pw+1."""
    lib = L.load()
    x = x.contiguous()
    W, Cc = x.shape[-2], x.shape[-1]
    nrows = x.numel() // (W * Cc) if W * Cc else 0
    y = torch.empty(tuple(x.shape[:-2]) + ((W - 1) // 2 + 1, Cc), dtype=torch.float32, device=x.device)
    L.check(lib.actmi_op_hpool(_p(x), _p(y), nrows, W, Cc, L.current_stream_ptr()), None, "op_hpool")
    return y


def conv3x3_c64(x, w_ohwi, scale=None, bias=None, res=None, relu=False, w_scale=256.0, w16=None):
    """direct 3x3/s1/p1 conv, 64 -> 64 channels, f16x3: x [G,B,H,W,64]; w_ohwi [G,64,3,3,64]; returns [G,B,H,W,64].
    w16: the split image of w_ohwi built with w_scale (split16) when the caller keeps one; else it is built per call."""
    lib = L.load()
    G, B, H, W, Cin = x.shape
    assert Cin == 64 and tuple(w_ohwi.shape[1:]) == (64, 3, 3, 64)
    out = torch.empty_like(x)
    if w16 is None:
        w16 = split16(w_ohwi, w_scale)
    scale = scale if scale is not None else torch.ones(G, 64, device=x.device)
    bias = bias if bias is not None else torch.zeros(G, 64, device=x.device)
    L.check(lib.actmi_op_conv3x3_c64(_p(x.contiguous()), _p(w16), float(w_scale), _p(scale.contiguous()), _p(bias.contiguous()),
                                     _p(res), _p(out), G, B, H, W, 1 if relu else 0, L.current_stream_ptr()), None,
            "op_conv3x3_c64")
    return out


def conv3x3_c64_dgrad(dy, wd_ohwi, dy_scale=None, res=None, mask=None, post_scale=None, amax_out=None, w_scale=256.0):
    """the direct 3x3 kernel as layer1's data gradient: dy [G,B,H,W,64]; wd_ohwi [G,64 cin,3,3,64 cout] = the flipped, transposed
    forward weights; dx = where(mask > 0, conv(dy) (+ res), 0) * post_scale[G,64].  dy_scale: pow2_scale tensor of dy;
    amax_out: one int32 word raised to the bits of max |dx|."""
    lib = L.load()
    G, B, H, W, Cc = dy.shape
    assert Cc == 64 and tuple(wd_ohwi.shape[1:]) == (64, 3, 3, 64)
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    for t in (res, mask):
        assert t is None or (t.shape == dy.shape and t.is_contiguous())
    assert post_scale is None or (tuple(post_scale.shape) == (G, 64) and post_scale.is_contiguous())
    w16 = split16(wd_ohwi, w_scale)
    L.check(lib.actmi_op_conv3x3_c64_dgrad(_p(dy), _p(w16), float(w_scale), _p(dy_scale), _p(res),
                                           _p(mask), _p(post_scale), _p(amax_out), _p(dx), G, B, H, W, L.current_stream_ptr()),
            None, "op_conv3x3_c64_dgrad")
    return dx


def _wgrad_buffers(G, slice_floats, default_partials, dw_shape, device, max_partials, out, accumulate, ws):
    """workspace and result of the two direct weight-gradient ops: ws sized for max_partials partials per group (default: the
    launcher's own cap, one unit per workgroup), or the caller's; dw a fresh tensor, or the caller's `out` (dense, fp32; any float
    alignment)"""
    if ws is None:
        k = default_partials if max_partials is None else int(max_partials)
        ws = torch.empty(G * k * slice_floats, device=device, dtype=torch.float32)
    else:
        assert max_partials is None, "max_partials sizes the op's own workspace; a caller's ws has its size"
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.device == device
    if out is None:
        assert not accumulate, "accumulate adds into out"
        out = torch.empty(dw_shape, device=device, dtype=torch.float32)
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(dw_shape) and out.is_contiguous() and out.device == device
    return ws, out


def wgrad3x3_c64(dy, x, dy_scale=None, max_partials=None, out=None, accumulate=False, ws=None):
    """dW [G][64][3][3][64] (O, kh, kw, I) of the 64 -> 64 channel 3x3 / s1 / p1 convolution from dy, x [G][B][H][W][64].
    max_partials: size the workspace for this many partials per group (fewer than the default = several (image, strip) units
    per workgroup); ws: a caller's workspace instead (the first G * nwg slices of 64 * 576 floats are written); out: a caller's
    dw; accumulate: out += dW (the training step's form)."""
    G, B, H, W, Cc = x.shape
    assert Cc == 64 and dy.shape == x.shape
    nwg = max(1, min(256 // G, B * ((W + 31) // 32)))
    ws, dw = _wgrad_buffers(G, 64 * 576, nwg, (G, 64, 3, 3, 64), x.device, max_partials, out, accumulate, ws)
    lib = L.load()
    L.check(lib.actmi_op_wgrad3x3_c64_ex(_p(dy.contiguous()), _p(x.contiguous()), _p(dw), _p(ws), ws.numel(),
                                         _p(dy_scale) if dy_scale is not None else None, G, B, H, W, 1 if accumulate else 0,
                                         L.current_stream_ptr()),
            None, "op_wgrad3x3_c64")
    return dw


def wgrad7x7s2(dy, x4, dy_scale=None, max_partials=None, out=None, accumulate=False, ws=None):
    """dW [G][64][7][7][4] (O, kh, kw, I) of the stem convolution (7x7 / s2 / p3) from dy [G][B][Ho][Wo][64], x4 [G][B][H][W][4].
    max_partials / ws / out / accumulate as in wgrad3x3_c64 (slices of 64 * 196 floats)."""
    G, B, H, W, Cc = x4.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert Cc == 4 and tuple(dy.shape) == (G, B, Ho, Wo, 64)
    nwg = max(1, min(512 // G, B * ((Wo + 31) // 32)))
    ws, dw = _wgrad_buffers(G, 64 * 196, nwg, (G, 64, 7, 7, 4), x4.device, max_partials, out, accumulate, ws)
    lib = L.load()
    L.check(lib.actmi_op_wgrad7x7s2_ex(_p(dy.contiguous()), _p(x4.contiguous()), _p(dw), _p(ws), ws.numel(),
                                       _p(dy_scale) if dy_scale is not None else None, G, B, H, W, 1 if accumulate else 0,
                                       L.current_stream_ptr()),
            None, "op_wgrad7x7s2")
    return dw


def attention(q, k, v, nheads, kpm=None, q_shared=False, want_lse=False, split=True, drop_p=0.0, drop_seed=0, prec=None,
              causal=False):
    """q [B,Nq,D] (or [Nq,D] when q_shared), k/v [B,Nk,D] (views with row stride allowed); returns [B,Nq,D]."""
    lib = L.load()
    B, Nk, D = k.shape
    Nq = q.shape[-2]
    hd = D // nheads
    out = torch.zeros((B, Nq, D), dtype=torch.float32, device=k.device)
    lse = torch.zeros((B, nheads, Nq), dtype=torch.float32, device=k.device) if want_lse else None
    d = L.AttnDesc()
    d.Q, d.q_bs, d.q_rs = q.data_ptr(), (0 if q_shared else q.stride(0)), q.stride(-2)
    d.K, d.k_bs, d.k_rs = k.data_ptr(), k.stride(0), k.stride(1)
    d.V, d.v_bs, d.v_rs = v.data_ptr(), v.stride(0), v.stride(1)
    d.O, d.o_bs, d.o_rs = out.data_ptr(), out.stride(0), out.stride(1)
    if kpm is not None:
        d.kpm, d.kpm_bs = kpm.data_ptr(), kpm.stride(0)
    d.lse = lse.data_ptr() if lse is not None else None
    if split:                                   # workspace for the split-KV path (used when the grid is small)
        ws = torch.empty(8 * B * Nq * (D + 2 * nheads), dtype=torch.float32, device=k.device)
        d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
    d.B, d.H, d.Nq, d.Nk, d.HD = B, nheads, Nq, Nk, hd
    d.scale = 1.0 / (hd ** 0.5)
    d.drop_p, d.drop_seed = float(drop_p), int(drop_seed)
    d.prec = PREC[prec]
    d.causal = 1 if causal else 0
    L.check(lib.actmi_op_attention(C.byref(d), L.current_stream_ptr()), None, "op_attention")
    return (out, lse) if want_lse else out


def attention_weights(q, k, nheads, kpm=None, q_shared=False, prec=None, causal=False, out=None):
    """Head-averaged softmax weights of ``attention`` on the same views (actmi_op_attn_weights): q [B,Nq,D] (or [Nq,D] when
    q_shared), k [B,Nk,D] (row-strided views allowed) -> [B,Nq,Nk] float32, what nn.MultiheadAttention(need_weights=True)
    returns beside its output.  out: a float32 tensor or view of that shape with last-dim stride 1 to write into."""
    lib = L.load()
    B, Nk, D = k.shape
    Nq = q.shape[-2]
    hd = D // nheads
    if out is None:
        out = torch.empty((B, Nq, Nk), dtype=torch.float32, device=k.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, Nq, Nk) or out.stride(2) != 1 or out.device != k.device:
        raise ValueError(f"out must be a float32 [{B}, {Nq}, {Nk}] tensor on {k.device} with last-dim stride 1")
    d = L.AttnDesc()
    d.Q, d.q_bs, d.q_rs = q.data_ptr(), (0 if q_shared else q.stride(0)), q.stride(-2)
    d.K, d.k_bs, d.k_rs = k.data_ptr(), k.stride(0), k.stride(1)
    if kpm is not None:
        d.kpm, d.kpm_bs = kpm.data_ptr(), kpm.stride(0)
    d.B, d.H, d.Nq, d.Nk, d.HD = B, nheads, Nq, Nk, hd
    d.scale = 1.0 / (hd ** 0.5)
    d.prec = PREC[prec]
    d.causal = 1 if causal else 0
    L.check(lib.actmi_op_attn_weights(C.byref(d), out.data_ptr(), out.stride(0), out.stride(1), L.current_stream_ptr()), None,
            "op_attn_weights")
    return out


def heat_ramp():
    """The fixed 256-entry colour table of the attention overlays, u8 [256, 3]: black - blue - magenta - orange - yellow -
    white, piecewise linear between six anchors, built in numpy (no plotting library)."""
    import numpy as np
    anchors = np.array([[0, 0, 0], [20, 20, 160], [180, 30, 150], [250, 120, 30], [255, 230, 60], [255, 255, 255]], np.float64)
    x = np.arange(256, dtype=np.float64) / 255.0 * (len(anchors) - 1)
    i0 = np.minimum(x.astype(np.int64), len(anchors) - 2)
    w = (x - i0)[:, None]
    return np.floor(anchors[i0] * (1 - w) + anchors[i0 + 1] * w + 0.5).astype(np.uint8)


def heat_overlay(frames, heat, lut, alpha=0.5):
    """actmi_op_heat_overlay_u8: frames u8 [B,K,H,W,3] and heat f32 [B,K,fh,fw] (>= 0, finite) on one device, lut u8 [256,3]
    (tensor or array), -> the blended frames, a new u8 tensor.  The arithmetic is defined in include/actmi.h."""
    import numpy as np
    lib = L.load()
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 [B, K, H, W, 3] tensor")
    B, K, H, W, _ = frames.shape
    if heat.dtype != torch.float32 or heat.dim() != 4 or tuple(heat.shape[:2]) != (B, K) or not heat.is_contiguous() \
            or heat.device != frames.device:
        raise ValueError(f"heat must be a contiguous float32 [{B}, {K}, fh, fw] tensor on {frames.device}")
    lut_t = torch.as_tensor(np.ascontiguousarray(lut) if isinstance(lut, np.ndarray) else lut)
    if lut_t.dtype != torch.uint8 or tuple(lut_t.shape) != (256, 3):
        raise ValueError("lut must be uint8 [256, 3]")
    lut_t = lut_t.to(frames.device).contiguous()
    out = torch.empty_like(frames)
    ws = torch.empty(B, dtype=torch.float32, device=frames.device)
    L.check(lib.actmi_op_heat_overlay_u8(frames.data_ptr(), heat.data_ptr(), lut_t.data_ptr(), float(alpha), out.data_ptr(),
                                         ws.data_ptr(), B, K, H, W, heat.shape[2], heat.shape[3], L.current_stream_ptr()),
            None, "op_heat_overlay_u8")
    return out


def heat_overlay_ref(frames, heat, lut, alpha=0.5):
    """heat_overlay on the host, numpy float32 with one rounding per operation in the order include/actmi.h gives: the same
    bytes as the device.  frames u8 [B,K,H,W,3], heat f32 [B,K,fh,fw], lut u8 [256,3] (arrays)."""
    import numpy as np
    f32 = np.float32
    frames, heat, lut = np.asarray(frames), np.asarray(heat, dtype=f32), np.asarray(lut)
    B, K, H, W, _ = frames.shape
    fh, fw = heat.shape[2:]
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("alpha must lie in [0, 1]")
    alpha = f32(alpha)

    def taps(n_out, n_in):
        scale = f32(n_in) / f32(n_out)
        c = np.maximum((np.arange(n_out, dtype=f32) + f32(0.5)) * scale - f32(0.5), f32(0))
        i0 = np.minimum(np.floor(c).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), (c - i0.astype(f32)).astype(f32)

    y0, y1, wy = taps(H, fh)
    x0, x1, wx = taps(W, fw)
    m = np.maximum(heat.reshape(B, -1).max(1), f32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(m[:, None, None, None] > 0, heat / m[:, None, None, None], f32(0)).astype(f32)
    wx_, wy_ = wx[None, None, None, :], wy[None, None, :, None]
    t0 = g[:, :, y0][:, :, :, x0] * (f32(1) - wx_) + g[:, :, y0][:, :, :, x1] * wx_
    t1 = g[:, :, y1][:, :, :, x0] * (f32(1) - wx_) + g[:, :, y1][:, :, :, x1] * wx_
    gp = (t0 * (f32(1) - wy_) + t1 * wy_).astype(f32)                                   # [B, K, H, W]
    idx = np.clip(np.floor(gp * f32(255) + f32(0.5)), 0, 255).astype(np.int64)
    a = (alpha * gp)[..., None]
    v = np.floor(frames.astype(f32) * (f32(1) - a) + lut[idx].astype(f32) * a + f32(0.5))
    return np.clip(v, 0, 255).astype(np.uint8)


def attention_bwd(q, k, v, o, lse, dout, nheads, kpm=None, drop_p=0.0, drop_seed=0, do_scale=None, want_amax=False, out=None,
                  amax_out=None):
    """dq, dk, dv of ``attention`` (f16x3, no materialised scores): q [B,Nq,D], k / v [B,Nk,D] (row-strided views allowed),
    o / dout [B,Nq,D] contiguous (the forward's output and its gradient), lse [B,H,Nq] from ``attention(..., want_lse=True)``.
    out: a (dq, dk, dv) triple of float32 tensors or views of shapes [B,Nq,D], [B,Nk,D], [B,Nk,D] with last-dim stride 1 that
    the kernels write through their own batch and row strides (the packed gradient buffer of the training step); without it
    dense tensors are allocated.  amax_out: one int32 word that the three gradients raise to the bits of their largest
    magnitude (a running maximum: the caller seeds it); it is returned as the fourth value, as with want_amax."""
    lib = L.load()
    B, Nk, D = k.shape
    Nq = q.shape[1]
    if out is None:
        dq = torch.empty((B, Nq, D), dtype=torch.float32, device=k.device)
        dk = torch.empty((B, Nk, D), dtype=torch.float32, device=k.device)
        dv = torch.empty((B, Nk, D), dtype=torch.float32, device=k.device)
    else:
        dq, dk, dv = out
        for name, t, n in (("dq", dq, Nq), ("dk", dk, Nk), ("dv", dv, Nk)):
            if tuple(t.shape) != (B, n, D) or t.dtype != torch.float32 or t.device != k.device or t.stride(2) != 1:
                raise ValueError(f"attention_bwd: out {name} must be float32 [{B},{n},{D}] on {k.device} with last-dim stride 1, "
                                 f"got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    ws = torch.empty(B * nheads * Nq, dtype=torch.float32, device=k.device)
    if amax_out is not None:
        if amax_out.dtype != torch.int32 or amax_out.numel() != 1 or amax_out.device != k.device:
            raise ValueError("attention_bwd: amax_out must be one int32 word on the operands' device")
        amax = amax_out
    else:
        amax = torch.zeros(1, dtype=torch.int32, device=k.device) if want_amax else None
    d = L.AttnBwdDesc()
    d.q, d.q_bs, d.q_rs = q.data_ptr(), q.stride(0), q.stride(1)
    d.k, d.k_bs, d.k_rs = k.data_ptr(), k.stride(0), k.stride(1)
    d.v, d.v_bs, d.v_rs = v.data_ptr(), v.stride(0), v.stride(1)
    d.o, d.d_o, d.lse = o.data_ptr(), dout.data_ptr(), lse.data_ptr()
    d.dq, d.dq_bs, d.dq_rs = dq.data_ptr(), dq.stride(0), dq.stride(1)
    d.dk, d.dk_bs, d.dk_rs = dk.data_ptr(), dk.stride(0), dk.stride(1)
    d.dv, d.dv_bs, d.dv_rs = dv.data_ptr(), dv.stride(0), dv.stride(1)
    if kpm is not None:
        d.kpm, d.kpm_bs = kpm.data_ptr(), kpm.stride(0)
    d.B, d.H, d.Nq, d.Nk, d.HD = B, nheads, Nq, Nk, D // nheads
    d.drop_p, d.drop_seed = float(drop_p), int(drop_seed)
    d.delta_ws = ws.data_ptr()
    d.do_scale = do_scale.data_ptr() if do_scale is not None else None
    d.amax_out = amax.data_ptr() if amax is not None else None
    L.check(lib.actmi_op_attention_bwd(C.byref(d), L.current_stream_ptr()), None, "op_attention_bwd")
    return (dq, dk, dv, amax) if amax is not None else (dq, dk, dv)


def layernorm(x, w, b, res=None, res_mod=0, w2=None, b2=None, eps=1e-5):
    lib = L.load()
    M, D = x.shape
    y = torch.empty_like(x)
    L.check(lib.actmi_op_layernorm(_p(x), _p(res), res_mod, _p(w), _p(b), _p(w2), _p(b2), _p(y), M, D, eps,
                                   L.current_stream_ptr()), None, "op_layernorm")
    return y


def layernorm_ex(x, w, b, M, D, nsplit=1, split_stride=0, bias=None, res=None, res_mod=0, w2=None, b2=None, eps=1e-5, add2=None,
                 add2_mod=0, head_w=None, head_b=None, head_n=0, flag=None, flag_bit=0, want_y2=None, want_head=None):
    """actmi_op_layernorm_ex: LayerNorm with the fused forms of the engine.  x holds nsplit slices [M, D], slice s at element
    offset s * split_stride, summed by the row loader (+ bias [D], + res[m % res_mod]).  add2 [rows, D]: also y2 = y +
    add2[m % add2_mod]; head_w [head_n, D] (+ head_b): also head = y @ head_w.T + head_b, `flag` (one int32 word) gaining
    flag_bit when a head output is not finite.  want_y2 / want_head force the outputs on without their operands (the launcher's
    rejections).  Returns y, or (y, y2, head) with None for an absent output."""
    lib = L.load()
    y = torch.empty((M, D), dtype=torch.float32, device=x.device)
    y2 = torch.empty((M, D), dtype=torch.float32, device=x.device) if (add2 is not None if want_y2 is None else want_y2) else None
    with_head = head_w is not None if want_head is None else want_head
    if head_w is not None and not head_n:
        head_n = head_w.shape[0]
    head = torch.empty((M, max(int(head_n), 1)), dtype=torch.float32, device=x.device) if with_head else None
    L.check(lib.actmi_op_layernorm_ex(_p(x), int(nsplit), int(split_stride), _p(bias), _p(res), int(res_mod), _p(w), _p(b), _p(w2),
                                      _p(b2), _p(y), _p(y2), _p(add2), int(add2_mod), _p(head), _p(head_w), _p(head_b), int(head_n),
                                      _p(flag), int(flag_bit), int(M), int(D), eps, L.current_stream_ptr()), None, "op_layernorm_ex")
    return y if (y2 is None and head is None) else (y, y2, head)


def maxpool3x3s2(x):
    """x [n,H,W,C] NHWC -> [n,Ho,Wo,C]."""
    lib = L.load()
    n, H, W, Cc = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((n, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    L.check(lib.actmi_op_maxpool3x3s2(_p(x), _p(y), n, H, W, Cc, L.current_stream_ptr()), None, "op_maxpool")
    return y


def conv1(image, w_oihw, scale, bias, prec=None):
    """image u8 [B,C,H,W,3] or f32 [B,C,3,H,W]; w [C,Cout,3,7,7]; scale/bias [C,Cout] -> [C,B,Ho,Wo,Cout]."""
    lib = L.load()
    image = image.contiguous()
    if image.dtype == torch.uint8:
        B, Cn, H, W, _ = image.shape
        fmt = L.IMG_U8_NHWC
    else:
        B, Cn, _, H, W = image.shape
        fmt = L.IMG_F32_NCHW
    Cout = w_oihw.shape[1]
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    out = torch.zeros((Cn, B, Ho, Wo, Cout), dtype=torch.float32, device=image.device)
    ws = torch.empty(Cn * Cout * 148 + 768, dtype=torch.float32, device=image.device)
    L.check(lib.actmi_op_conv1(_p(image), fmt, _p(w_oihw), _p(scale), _p(bias), _p(out), _p(ws), B, Cn, H, W, Cout,
                               PREC[prec], L.current_stream_ptr()), None, "op_conv1")
    return out


def depth_minmax(depth_u16, out=None):
    """per-sample extremes of a raw depth batch: depth uint16 [B, ...] (contiguous; everything behind the batch axis is one
    sample) -> float32 [B, 2] = (min, max), exact; no host synchronisation."""
    lib = L.load()
    if depth_u16.dtype != torch.uint16:
        raise TypeError(f"depth_minmax: dtype {depth_u16.dtype} not supported (uint16)")
    depth_u16 = depth_u16.contiguous()
    B = depth_u16.shape[0]
    n = depth_u16.numel() // B if B else 0
    if out is None:
        out = torch.empty((B, 2), dtype=torch.float32, device=depth_u16.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B, 2)
    L.check(lib.actmi_op_depth_minmax_u16(_p(depth_u16), _p(out), B, n, L.current_stream_ptr()), None, "op_depth_minmax_u16")
    return out


def conv1_depth(depth, w_oihw, scale, bias, out=None, out_cam0=0, lohi=None):
    """depth stem: depth f32 [B, Cd, 1, H, W] un-normalised; w [Cd, Cout, 1, 7, 7]; scale / bias [Cd, Cout].  Returns the
    camera-major map [Cd, B, Ho, Wo, Cout], or writes cameras out_cam0 .. out_cam0 + Cd - 1 of a given `out` [Ct, B, Ho, Wo, Cout].
    A raw uint16 `depth` needs lohi = depth_minmax(depth) ([B, 2]): the loader normalises every sample with its extremes first."""
    lib = L.load()
    if depth.dtype == torch.uint16:
        if lohi is None:
            raise ValueError("conv1_depth: a uint16 depth batch needs lohi=depth_minmax(depth)")
    elif depth.dtype != torch.float32:
        raise TypeError(f"conv1_depth: depth dtype {depth.dtype} not supported (float32 or uint16)")
    elif lohi is not None:
        raise ValueError("conv1_depth: lohi goes with a uint16 depth batch")
    depth, w_oihw, scale, bias = depth.contiguous(), w_oihw.contiguous(), scale.contiguous(), bias.contiguous()
    B, Cd, one, H, W = depth.shape
    Cout = w_oihw.shape[1]
    assert one == 1 and tuple(w_oihw.shape) == (Cd, Cout, 1, 7, 7) and tuple(scale.shape) == (Cd, Cout) == tuple(bias.shape)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    if out is None:
        out = torch.empty((Cd, B, Ho, Wo, Cout), dtype=torch.float32, device=depth.device)
    assert out.is_contiguous() and tuple(out.shape[1:]) == (B, Ho, Wo, Cout) and 0 <= out_cam0 and out_cam0 + Cd <= out.shape[0]
    if lohi is not None:
        lohi = lohi.contiguous()
        assert lohi.dtype == torch.float32 and tuple(lohi.shape) == (B, 2)
        L.check(lib.actmi_op_conv1_depth_u16(_p(depth), _p(lohi), _p(w_oihw), _p(scale), _p(bias), _p(out), B, Cd, H, W, Cout,
                                             int(out_cam0), L.current_stream_ptr()), None, "op_conv1_depth_u16")
        return out
    L.check(lib.actmi_op_conv1_depth(_p(depth), _p(w_oihw), _p(scale), _p(bias), _p(out), B, Cd, H, W, Cout, int(out_cam0),
                                     L.current_stream_ptr()), None, "op_conv1_depth")
    return out


# ---- DiffusionPolicy path (reference policy.py:20-241): the non-GEMM ops, channel-last ---------------------------------
ACT = {None: 0, "none": 0, "relu": 1, "mish": 2}


_GN_WS = {}


def groupnorm(x, weight, bias, groups, eps=1e-5, act=None, res=None, res_after=False, film=None, out=None):
    """x [n, P, C] (any leading spatial shape flattened into P is fine: pass [n, ..., C]); torch.nn.GroupNorm statistics.
    out = act(GN(x) + res) (res_after=False) or act(GN(x)) * film_scale + film_bias + res (res_after=True).
    `out`: optional contiguous tensor of x's shape to write into."""
    lib = L.load()
    x = x.contiguous()
    n, Cc = x.shape[0], x.shape[-1]
    P = x.numel() // (n * Cc)
    if out is None:
        out = torch.empty_like(x)
    assert out.is_contiguous() and out.shape == x.shape
    fs, fb = (film[0].contiguous(), film[1].contiguous()) if film is not None else (None, None)
    rm = 0 if res is None else (2 if res_after else 1)
    # chunk statistics of the large-map path (3 floats per sample, group, chunk): one workspace per (device, stream) -- two
    # streams normalising concurrently must not share it
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    ws = _GN_WS.get(key)
    if ws is None:
        ws = _GN_WS[key] = torch.empty(1 << 20, dtype=torch.float32, device=x.device)
    L.check(lib.actmi_op_groupnorm(_p(x), _p(res.contiguous() if res is not None else None), _p(fs), _p(fb), _p(weight), _p(bias),
                                   _p(out), n, P, Cc, int(groups), float(eps), ACT[act], rm, _p(ws), ws.numel(),
                                   L.current_stream_ptr()), None, "op_groupnorm")
    return out


def spatial_softmax(logits, H, W, temperature=1.0):
    """logits [n, H*W, K] -> [n, K, 2] expected (x, y) keypoints (robomimic SpatialSoftmax)."""
    lib = L.load()
    logits = logits.contiguous()
    n, P, K = logits.shape
    assert P == H * W
    out = torch.empty((n, K, 2), dtype=torch.float32, device=logits.device)
    L.check(lib.actmi_op_spatial_softmax(_p(logits), _p(out), n, H, W, K, float(temperature), L.current_stream_ptr()), None,
            "op_spatial_softmax")
    return out


def unfold1d(x, k, stride=1, pad=0, transposed=False):
    """x [B, T, C] -> [B, To, k*C]: the rows a Conv1d (or, transposed, a ConvTranspose1d) contracts with its weights."""
    lib = L.load()
    x = x.contiguous()
    B, T, Cc = x.shape
    To = (T - 1) * stride - 2 * pad + k if transposed else (T + 2 * pad - k) // stride + 1
    out = torch.empty((B, To, k * Cc), dtype=torch.float32, device=x.device)
    L.check(lib.actmi_op_unfold1d(_p(x), _p(out), B, T, Cc, k, stride, pad, To, 1 if transposed else 0, L.current_stream_ptr()),
            None, "op_unfold1d")
    return out


def ddim_step(x, eps, alpha_t, alpha_prev, clip=True):
    """in place: diffusers DDIMScheduler.step with eta = 0, epsilon prediction."""
    lib = L.load()
    assert x.is_contiguous() and eps.is_contiguous() and x.numel() == eps.numel()
    L.check(lib.actmi_op_ddim_step(_p(x), _p(eps), x.numel(), float(alpha_t ** -0.5), float((1.0 - alpha_t) ** 0.5),
                                   float(alpha_prev ** 0.5), float(max(0.0, 1.0 - alpha_prev) ** 0.5), 1 if clip else 0,
                                   L.current_stream_ptr()), None, "op_ddim_step")
    return x


def mish(x):
    lib = L.load()
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(lib.actmi_op_mish(_p(x), _p(y), x.numel(), L.current_stream_ptr()), None, "op_mish")
    return y


def u8_to_nhwc4(image_u8):
    """u8 [B, Cam, H, W, 3] -> f32 [Cam, B, H, W, 4] in [0, 1] (channel 3 = 0): the GEMM convolution wants Cin % 4 == 0."""
    lib = L.load()
    image_u8 = image_u8.contiguous()
    B, Cam, H, W, _ = image_u8.shape
    out = torch.empty((Cam, B, H, W, 4), dtype=torch.float32, device=image_u8.device)
    L.check(lib.actmi_op_u8_to_nhwc4(_p(image_u8), _p(out), B, Cam, H, W, L.current_stream_ptr()), None, "op_u8_to_nhwc4")
    return out


# ---- pieces of the latent-prior training step (csrc/prior.hip; reference train_latent_model.py:323-343) -----------------
def gemm_t(A, Bm, ta=False, tb=False, bias=None, res=None, out=None, prec="f32"):
    """C = A' @ B'^T (+ bias + res) with the transposed operand forms of the backward: ta: A is stored [K][M]; tb: B is stored
    [K][N] (else [N][K], the nn.Linear layout).  Linear backward: dX = gemm_t(dY, W, tb=True); dW = gemm_t(dY, X, ta=True, tb=True)."""
    lib = L.load()
    if ta:
        K, M = A.shape
    else:
        M, K = A.shape
    N = Bm.shape[1] if tb else Bm.shape[0]
    assert (Bm.shape[0] if tb else Bm.shape[1]) == K, (A.shape, Bm.shape, ta, tb)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    d = L.GemmDesc()
    d.A, d.lda, d.mode, d.ta = A.data_ptr(), A.stride(0), 0, 1 if ta else 0
    d.Bw, d.ldb, d.tb = Bm.data_ptr(), Bm.stride(0), 1 if tb else 0
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        d.res, d.ldres = res.data_ptr(), res.stride(0)
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.M, d.N, d.K, d.groups = M, N, K, 1
    d.prec = PREC[prec]
    L.check(lib.actmi_op_gemm(C.byref(d), L.current_stream_ptr()), None, "op_gemm")
    return out


def gelu(x):
    y = torch.empty_like(x)
    L.check(L.load().actmi_op_gelu(_p(x), _p(y), x.numel(), L.current_stream_ptr()), None, "op_gelu")
    return y


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    L.check(L.load().actmi_op_gelu_bwd(_p(x), _p(dy), _p(dx), x.numel(), L.current_stream_ptr()), None, "op_gelu_bwd")
    return dx


def dropout(x, p, seed):
    """y = x * keep(seed, i) / (1 - p); the backward is the same call on the gradient"""
    y = torch.empty_like(x)
    L.check(L.load().actmi_op_dropout(_p(x), _p(y), x.numel(), float(p), int(seed), L.current_stream_ptr()), None, "op_dropout")
    return y


def small_attention(qkv, nheads, causal=True, drop_p=0.0, seed=0):
    """qkv [n,T,3D] (q | k | v) -> [n,T,D]; T <= 64, D / nheads <= 64"""
    n, T, D3 = qkv.shape
    D = D3 // 3
    out = torch.empty((n, T, D), dtype=torch.float32, device=qkv.device)
    L.check(L.load().actmi_op_small_attention(_p(qkv), _p(out), n, T, nheads, D // nheads, 1 if causal else 0, float(drop_p), int(seed),
                                              L.current_stream_ptr()), None, "op_small_attention")
    return out


def small_attention_bwd(qkv, dout, nheads, causal=True, drop_p=0.0, seed=0):
    n, T, D3 = qkv.shape
    D = D3 // 3
    dqkv = torch.empty_like(qkv)
    L.check(L.load().actmi_op_small_attention_bwd(_p(qkv), _p(dout), _p(dqkv), n, T, nheads, D // nheads, 1 if causal else 0,
                                                  float(drop_p), int(seed), L.current_stream_ptr()), None, "op_small_attention_bwd")
    return dqkv


def soft_ce_dim1(logits, target, want_grad=True):
    """F.cross_entropy(logits [B,T,V], target [B,T,V] probabilities): classes along dim 1.  -> (loss [1], dlogits or None)"""
    B, T, V = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = torch.empty(B * V, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    L.check(L.load().actmi_op_soft_ce_dim1(_p(logits), _p(target), B, T, V, _p(loss), _p(dl), _p(ws), L.current_stream_ptr()), None,
            "op_soft_ce_dim1")
    return loss, dl


def argmax_l1(logits, target):
    """mean |one_hot(argmax(logits, -1)) - target|"""
    V = logits.shape[-1]
    rows = logits.numel() // V
    out = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = torch.empty(rows, dtype=torch.float32, device=logits.device)
    L.check(L.load().actmi_op_argmax_l1(_p(logits), _p(target), rows, V, _p(out), _p(ws), L.current_stream_ptr()), None, "op_argmax_l1")
    return out


def layernorm_bwd(x, w, dy, dw, db, ws, dx_add=None, eps=1e-5):
    """-> dx; dw += , db += (views of the gradient arena)"""
    M, D = x.shape
    dx = torch.empty_like(x)
    L.check(L.load().actmi_op_layernorm_bwd(_p(x), _p(w), _p(dy), _p(dx_add), _p(dx), _p(dw), _p(db), M, D, eps, _p(ws), ws.numel(),
                                            L.current_stream_ptr()), None, "op_layernorm_bwd")
    return dx


def colsum(src, out, ws=None):
    """out[n] += sum_m src[m][n]; src may be a column view of a wider matrix (row stride = its stride(0))"""
    M, N = src.shape
    L.check(L.load().actmi_op_colsum(_p(src), src.stride(0), _p(out), M, N, _p(ws), ws.numel() if ws is not None else 0,
                                     L.current_stream_ptr()), None, "op_colsum")


def pcd_embed(xyz, rgb, w0, b0):
    """PointNet layer 0: gelu(cat(xyz, rgb) @ w0.T + b0) in fp32 FMAs; xyz, rgb [..., 3] -> [rows, H]"""
    xyz, rgb = xyz.contiguous().view(-1, 3), rgb.contiguous().view(-1, 3)
    rows, H = xyz.shape[0], w0.shape[0]
    out = torch.empty((rows, H), dtype=torch.float32, device=xyz.device)
    L.check(L.load().actmi_op_pcd_embed(_p(xyz), _p(rgb), _p(w0.contiguous()), _p(b0.contiguous()), _p(out), rows, H,
                                        L.current_stream_ptr()), None, "op_pcd_embed")
    return out


def colmax(x, O=None, split=True, counts=None):
    """x [B, P, ld] -> (max over the points [B, O], int32 index of the winner [B, O]) for the columns < O (default ld); the
    lowest index wins a tie, a NaN propagates.  split=False: one block column per sample (no workspace).  counts (int32 [B] on
    x's device): sample b's points are its rows [0, clamp(counts[b], 1, P)); the rows behind them are never read."""
    B, P, ld = x.shape
    O = ld if O is None else O
    out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, O), dtype=torch.int32, device=x.device)
    ws = torch.empty(2 * B * 64 * O, dtype=torch.float32, device=x.device) if split else None
    if counts is not None:
        if counts.dtype != torch.int32 or tuple(counts.shape) != (B,) or counts.device != x.device or not counts.is_contiguous():
            raise ValueError(f"colmax: counts must be a contiguous int32 [{B}] tensor on {x.device}")
        L.check(L.load().actmi_op_colmax_n(_p(x), B, P, O, ld, _p(counts), _p(out), _p(arg), _p(ws), ws.numel() if split else 0,
                                           L.current_stream_ptr()), None, "op_colmax_n")
        return out, arg
    L.check(L.load().actmi_op_colmax(_p(x), B, P, O, ld, _p(out), _p(arg), _p(ws), ws.numel() if split else 0,
                                     L.current_stream_ptr()), None, "op_colmax")
    return out, arg


def sum_batch(src, dst, accumulate=False):
    """src [B,R,D] -> dst[R,D] (+)= sum_b src[b]"""
    B, Rr, D = src.shape
    L.check(L.load().actmi_op_sum_batch(_p(src), src.stride(0), src.stride(1), _p(dst), B, Rr, D, 1 if accumulate else 0,
                                        L.current_stream_ptr()), None, "op_sum_batch")


def adamw(p, g, m, v, lr, weight_decay, step, betas=(0.9, 0.999), eps=1e-8):
    L.check(L.load().actmi_op_adamw(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(weight_decay), float(betas[0]),
                                    float(betas[1]), float(eps), int(step), L.current_stream_ptr()), None, "op_adamw")


# ---- the non-GEMM kernels of the ACT training step (csrc/bwd.hip, csrc/pool.hip), one wrapper per launcher ---------------
def _st():
    return L.current_stream_ptr()


def maxpool3x3s2_idx(x):
    """x [n,H,W,C] NHWC -> (out [n,Ho,Wo,C], codes uint8 [n,Ho,Wo,C]): code r*3+s = the window position of the maximum."""
    n, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((n, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    codes = torch.empty((n, Ho, Wo, Cc), dtype=torch.uint8, device=x.device)
    L.check(L.load().actmi_op_maxpool3x3s2_idx(_p(x), _p(y), _p(codes), n, H, W, Cc, _st()), None, "op_maxpool3x3s2_idx")
    return y, codes


def maxpool3x3s2_bwd(codes, dy, H, W, relu_x=None, bn_scale=None, imgs_per_group=1, amax_out=None):
    """dx [n,H,W,C] from the codes and dy [n,Ho,Wo,C]; relu_x [n,H,W,C] + bn_scale [groups,C]: the fused ReLU + FrozenBN form,
    amax_out (one int32 word) raised to the bits of max |dx|."""
    n, _, _, Cc = dy.shape
    dx = torch.empty((n, H, W, Cc), dtype=torch.float32, device=dy.device)
    L.check(L.load().actmi_op_maxpool3x3s2_bwd(_p(codes), _p(dy), _p(dx), n, H, W, Cc, _p(relu_x), _p(bn_scale), int(imgs_per_group),
                                               _p(amax_out), _st()), None, "op_maxpool3x3s2_bwd")
    return dx


def relu_bn_bwd(x, C_, add=None, mask=None, scale=None, want_plain=True, want_scaled=True, amax_out=None):
    """x [G, per_group] (NHWC maps of C_ channels, flattened): v = where(mask > 0, x + add, 0); -> (y_plain = v or None,
    y_scaled = v * scale[g][c] or None)"""
    G, per_group = x.shape
    yp = torch.empty_like(x) if want_plain else None
    ys = torch.empty_like(x) if want_scaled else None
    L.check(L.load().actmi_op_relu_bn_bwd(_p(x), _p(add), _p(mask), _p(scale), _p(yp), _p(ys), G, per_group, int(C_), _p(amax_out),
                                          _st()), None, "op_relu_bn_bwd")
    return yp, ys


def act_losses(a_hat, actions, is_pad, latent_info=None, kl_weight=0.0, L_=0, buf=None):
    """-> tensor [l1, kl, loss] (a view of the 516-float buffer the kernels reduce in); is_pad uint8 [B,Q]"""
    B, Q, A = a_hat.shape
    if buf is None:
        buf = torch.empty(3 + 1 + 512, dtype=torch.float32, device=a_hat.device)
    L.check(L.load().actmi_op_act_losses(_p(a_hat), _p(actions), _p(is_pad), _p(latent_info), _p(buf), buf.numel(), B, Q, A, int(L_),
                                         float(kl_weight), _st()), None, "op_act_losses")
    return buf[:3]


def l1_bwd(a_hat, actions, is_pad, gscale=1.0):
    B, Q, A = a_hat.shape
    d = torch.empty_like(a_hat)
    L.check(L.load().actmi_op_l1_bwd(_p(a_hat), _p(actions), _p(is_pad), _p(d), B, Q, A, float(gscale), _st()), None, "op_l1_bwd")
    return d


def reparam(latent_info, eps, want_stats=False):
    """latent_info [B, 2L] (mu | logvar), eps [B, L] -> z (and copies of mu, logvar)"""
    B, L2 = latent_info.shape
    z = torch.empty_like(eps)
    mu, lv = (torch.empty_like(eps), torch.empty_like(eps)) if want_stats else (None, None)
    L.check(L.load().actmi_op_reparam(_p(latent_info), _p(eps), _p(z), _p(mu), _p(lv), B, L2 // 2, _st()), None, "op_reparam")
    return (z, mu, lv) if want_stats else z


def reparam_kl_bwd(latent_info, eps, dz, klw_scaled):
    B, L2 = latent_info.shape
    d = torch.empty_like(latent_info)
    L.check(L.load().actmi_op_reparam_kl_bwd(_p(latent_info), _p(eps), _p(dz), _p(d), B, L2 // 2, float(klw_scaled), _st()), None,
            "op_reparam_kl_bwd")
    return d


def vq_bwd(probs, g):
    """probs, g [B, VC, VD] -> dlogits"""
    B, VC, VD = probs.shape
    d = torch.empty_like(probs)
    L.check(L.load().actmi_op_vq_bwd(_p(probs), _p(g), _p(d), B, VC, VD, _st()), None, "op_vq_bwd")
    return d


def dropout_bwd(dy, p, seed):
    dz = torch.empty_like(dy)
    L.check(L.load().actmi_op_dropout_bwd(_p(dy), _p(dz), dy.numel(), float(p), int(seed), _st()), None, "op_dropout_bwd")
    return dz


def attn_delta(dO, O, nheads):
    """dO, O [B, Nq, H*HD] -> delta [B, H, Nq]"""
    B, Nq, D = dO.shape
    delta = torch.empty((B, nheads, Nq), dtype=torch.float32, device=dO.device)
    L.check(L.load().actmi_op_attn_delta(_p(dO), _p(O), _p(delta), B, nheads, Nq, D // nheads, _st()), None, "op_attn_delta")
    return delta


def attn_drop(P, Pd, Nk, p, seed):
    """P, Pd [..., Nq, ldp] (G = the product of the leading dimensions): Pd = P * keep / (1 - p), columns >= Nk zero"""
    Nq, ldp = P.shape[-2:]
    L.check(L.load().actmi_op_attn_drop(_p(P), _p(Pd), int(seed), float(p), P.numel() // (Nq * ldp), Nq, int(Nk), ldp, _st()), None,
            "op_attn_drop")


def attn_ds_drop(P, dP, delta, scale, Nk, p, seed):
    """in place: dP = P * (dP * keep / (1 - p) - delta) * scale, columns >= Nk zero"""
    Nq, ldp = P.shape[-2:]
    L.check(L.load().actmi_op_attn_ds_drop(_p(P), _p(dP), _p(delta), float(scale), int(seed), float(p), P.numel() // (Nq * ldp), Nq,
                                           int(Nk), ldp, _st()), None, "op_attn_ds_drop")


def zero_cols(x, c0):
    """x [..., ld]: the columns c0 .. ld-1 of every row = 0"""
    ld = x.shape[-1]
    L.check(L.load().actmi_op_zero_cols(_p(x), x.numel() // ld, ld, int(c0), _st()), None, "op_zero_cols")


def adamw_groups(p, g, m, v, group, lr, lr_backbone, weight_decay, step, betas=(0.9, 0.999), eps=1e-8, flags=None, skip_mask=0):
    """the engine's AdamW: group uint8 per 64-float slot (0 untouched, 1 lr, 2 lr_backbone); flags (one int32 word) & skip_mask
    non-zero skips the update on the device"""
    L.check(L.load().actmi_op_adamw_groups(_p(p), _p(g), _p(m), _p(v), _p(group), p.numel(), float(lr), float(lr_backbone),
                                           float(weight_decay), float(betas[0]), float(betas[1]), float(eps), int(step), _p(flags),
                                           int(skip_mask), _st()), None, "op_adamw_groups")


def layernorm_bwd_ex(x, w, dy, dw, db, ws=None, dx_add=None, eps=1e-5, dx_amax=None):
    """layernorm_bwd with the dx_amax word (one int32) and an optional workspace"""
    M, D = x.shape
    dx = torch.empty_like(x)
    L.check(L.load().actmi_op_layernorm_bwd_ex(_p(x), _p(w), _p(dy), _p(dx_add), _p(dx), _p(dw), _p(db), M, D, eps, _p(ws),
                                               ws.numel() if ws is not None else 0, _p(dx_amax), _st()), None, "op_layernorm_bwd_ex")
    return dx


# ---- RGB-D frames -> the point cloud of a use_pcd policy (csrc/rgbd_cloud.hip; contract at actmi_rgbd_desc in actmi.h) ----------
def rgbd_select_key(seed, b, k, pixel, H, W):
    """The selection key of actmi_op_rgbd_cloud in numpy: a seeded bijection of [0, 2^m), m = max(1, ceil(log2(H * W))), of which
    camera k of sample b keeps the quota[k] survivors with the smallest values.  pixel: integers (any shape) -> uint32."""
    import numpy as np
    m = max(1, int(H * W - 1).bit_length())
    M64 = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    s0 = mix((int(seed) + 0x9E3779B97F4A7C15 * (int(b) * 8 + int(k) + 1)) & M64)
    s1 = mix((s0 + 0x9E3779B97F4A7C15) & M64)
    s2 = mix((s1 + 0x9E3779B97F4A7C15) & M64)
    c0, adds = s0 & 0xFFFFFFFF, (s0 >> 32, s1 & 0xFFFFFFFF, s1 >> 32, s2 & 0xFFFFFFFF)
    mask, h = np.uint64((1 << m) - 1), np.uint64((m + 1) // 2)
    x = (np.asarray(pixel).astype(np.uint64) ^ np.uint64(c0)) & mask
    for g, a in zip((0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F), adds):
        x = (x * np.uint64(g)) & mask                  # (x < 2^20, g < 2^32: no 64-bit overflow)
        x ^= x >> h
        x = (x + np.uint64(a)) & mask
    return x.astype(np.uint32)


def rgbd_fps_select(xyz_f32, key, quota, pool):
    """Which survivors of one camera actmi_op_rgbd_cloud_fps keeps, in numpy: the definition at actmi_rgbd_fps_desc in actmi.h,
    stated once more -- the oracle of the device op, not a fallback for it.

    xyz_f32 [M, 3]: the survivors' coordinates in pixel order (the fp32 values of the device); key [M]: their selection keys
    (rgbd_select_key).  -> (kept, sequence): the kept indices into the M survivors in ascending order, and the same indices in
    the order they were picked.  M <= quota: every survivor, picked in pixel order.  Otherwise the pool is every survivor
    (M <= pool) or the `pool` smallest keys, in pixel order; the start is the pool's smallest key; then `quota - 1` times: the
    picked point's distance becomes -1 for good, every other dist = min(dist, ((dx * dx) + (dy * dy)) + (dz * dz)) in float32,
    and the next pick is the largest dist, the lowest index among equals."""
    import numpy as np
    p = np.ascontiguousarray(xyz_f32, dtype=np.float32).reshape(-1, 3)
    key = np.asarray(key).reshape(-1)
    M, quota, pool = len(p), int(quota), int(pool)
    if key.shape != (M,) or quota < 1 or pool < quota:
        raise ValueError(f"rgbd_fps_select: {M} points, {key.shape} keys, quota {quota}, pool {pool}: needs a key per point and "
                         f"1 <= quota <= pool")
    if M <= quota:
        every = np.arange(M, dtype=np.int64)
        return every, every.copy()
    members = np.arange(M, dtype=np.int64) if M <= pool else np.sort(np.argsort(key, kind="stable")[:pool])
    px, py, pz = (np.ascontiguousarray(p[members, i]) for i in range(3))
    dist = np.full(len(members), np.inf, dtype=np.float32)
    seq = np.empty(quota, dtype=np.int64)
    s = int(np.argmin(key[members]))
    minus_one = np.float32(-1.0)
    with np.errstate(over="ignore"):
        for it in range(quota):
            seq[it] = s
            dist[s] = minus_one
            if it + 1 == quota:
                break
            dx, dy, dz = px - px[s], py - py[s], pz - pz[s]
            np.minimum(dist, ((dx * dx) + (dy * dy)) + (dz * dz), out=dist)      # float32 throughout; a picked point stays at -1
            s = int(np.argmax(dist))                                            # the first maximum: the lowest index among equals
    picked = members[seq]
    return np.sort(picked), picked


class RGBDFusion:
    """Builds the cloud of a use_pcd policy from raw depth frames on the device (actmi_op_rgbd_cloud), in place of the reference's
    host-side fusion node (aloha_scripts/jie_aloha_scripts/pcd_fusion.py:186-243, 278-279).  Owns the device parameter block, the
    seed word, the workspace and the output buffers.

    engine_or_device: an ACTEngine (its num_cams, image size, max_points and device are checked against) or a device.
    K fusion cameras of H x W pixels; cam_index[k]: the colour frame registered to depth camera k; intrinsics [K, 4] = (fx, fy,
    cx, cy); depth_scale: metres per depth unit (a number or [K]); extrinsics [K, 3, 4] or [K, 4, 4]: camera optical frame ->
    base; box = (xmin, xmax, ymin, ymax, zmin, zmax), ends included; quota [K] >= 1: points kept per camera at most, P =
    sum(quota) rows per sample; max_batch sizes the buffers (default: the engine's).

    sampling: which survivors a camera keeps when it has more than its quota.  "key" (default): the quota smallest values of the
    seeded key (actmi_op_rgbd_cloud; the reference's np.random.choice branch).  "fps": farthest-point sampling
    (actmi_op_rgbd_cloud_fps; what the reference's node runs under --use_fps), over the fps_pool smallest keys of the camera,
    started at the smallest; fps_pool defaults to min(ACTMI_RGBD_FPS_MAX_POOL, 4 * max(quota)); ``order`` [max_batch, P] int32
    then holds the iteration at which every row was picked (-1 behind n[b]).  rgbd_fps_select is the same selection in numpy.

    fuse(image_u8, depth_u16, B) -> {"xyz", "rgb": [B, P, 3] f32, "n": [B] int32}: views of the fusion's own buffers, valid until
    the next fuse.  Everything is validated on the host, before any device call (ValueError)."""

    def __init__(self, engine_or_device, K, H, W, cam_index, intrinsics, depth_scale, extrinsics, box, quota, max_batch=None,
                 num_cams=None, seed=0, sampling="key", fps_pool=None):
        import numpy as np
        if sampling not in ("key", "fps"):
            raise ValueError(f"RGBDFusion: sampling must be 'key' or 'fps', got {sampling!r}")
        if sampling == "key" and fps_pool is not None:
            raise ValueError("RGBDFusion: fps_pool given with sampling='key' (the pool belongs to sampling='fps')")
        self.sampling = sampling
        eng = engine_or_device if hasattr(engine_or_device, "max_points") else None
        self.device = torch.device(eng.device if eng is not None else engine_or_device)
        if self.device.type != "cuda":
            raise ValueError(f"RGBDFusion: device must be a cuda device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        K, H, W = int(K), int(H), int(W)
        if not 1 <= K <= L.RGBD_MAX_CAMS:
            raise ValueError(f"RGBDFusion: K = {K} fusion cameras: needs 1 <= K <= {L.RGBD_MAX_CAMS}")
        if H < 1 or W < 1 or not 2 <= H * W <= 1 << 20:
            raise ValueError(f"RGBDFusion: frames of {H} x {W}: needs 2 <= H * W <= 2^20")
        if eng is not None:
            num_cams = eng.cfg.num_cams
            if (H, W) != (eng.cfg.image_h, eng.cfg.image_w):
                raise ValueError(f"RGBDFusion: depth frames of {H} x {W}, the engine's colour frames {eng.cfg.image_h} x "
                                 f"{eng.cfg.image_w}: the depth is registered to the colour frame and has its size")
            if max_batch is None:
                max_batch = eng.max_batch
        self.K, self.H, self.W = K, H, W
        self.num_cams = None if num_cams is None else int(num_cams)
        self.max_batch = int(max_batch if max_batch is not None else 8)
        if self.max_batch < 1:
            raise ValueError(f"RGBDFusion: max_batch {max_batch} < 1")
        ci = np.asarray(cam_index)
        if ci.shape != (K,) or ci.dtype.kind not in "iu":
            raise ValueError(f"RGBDFusion: cam_index must hold {K} integers, got {ci.dtype} {ci.shape}")
        if ci.min() < 0 or (self.num_cams is not None and ci.max() >= self.num_cams):
            raise ValueError(f"RGBDFusion: cam_index {ci.tolist()} outside 0..{'C-1' if self.num_cams is None else self.num_cams - 1}")
        q = np.asarray(quota)
        if q.shape != (K,) or q.dtype.kind not in "iu" or q.min() < 1:
            raise ValueError(f"RGBDFusion: quota must hold {K} integers >= 1, got {q.dtype} {q.shape} {q.tolist() if q.size <= 8 else ''}")
        self.P = int(q.sum())
        self.fps_pool = None
        if sampling == "fps":
            if fps_pool is None:
                fps_pool = min(L.RGBD_FPS_MAX_POOL, 4 * int(q.max()))
            if isinstance(fps_pool, bool) or not isinstance(fps_pool, (int, np.integer)):
                raise ValueError(f"RGBDFusion: fps_pool must be an integer, got {fps_pool!r}")
            if not int(q.max()) <= fps_pool <= L.RGBD_FPS_MAX_POOL:
                raise ValueError(f"RGBDFusion: fps_pool = {fps_pool}: needs max(quota) = {int(q.max())} <= fps_pool <= "
                                 f"{L.RGBD_FPS_MAX_POOL} (ACTMI_RGBD_FPS_MAX_POOL)")
            self.fps_pool = int(fps_pool)
        if eng is not None and self.P > eng.max_points:
            raise ValueError(f"RGBDFusion: sum(quota) = {self.P} points per sample > the engine's max_points {eng.max_points}")
        intr = np.asarray(intrinsics, dtype=np.float64)
        if intr.shape != (K, 4) or not np.isfinite(intr).all() or (intr[:, :2] == 0).any():
            raise ValueError(f"RGBDFusion: intrinsics must be finite [{K}, 4] = (fx, fy, cx, cy) with fx, fy != 0, got {intr.shape}")
        ds = np.broadcast_to(np.asarray(depth_scale, dtype=np.float64), (K,)) if np.ndim(depth_scale) <= 1 and \
            np.size(depth_scale) in (1, K) else None
        if ds is None or not np.isfinite(ds).all() or (ds <= 0).any():
            raise ValueError(f"RGBDFusion: depth_scale must be a positive number or [{K}] of them")
        bx = np.asarray(box, dtype=np.float64)
        if bx.shape != (6,) or not np.isfinite(bx).all() or (bx[0::2] > bx[1::2]).any():
            raise ValueError("RGBDFusion: box must be 6 finite numbers (xmin, xmax, ymin, ymax, zmin, zmax) with min <= max")
        self.cam_index, self.quota = [int(v) for v in ci], [int(v) for v in q]
        self._host = L.RgbdCalib()
        for k in range(K):
            c = self._host.cam[k]
            c.cam_index, c.quota = self.cam_index[k], self.quota[k]
            c.fx, c.fy, c.cx, c.cy = (float(v) for v in intr[k])
            c.depth_scale = float(ds[k])
        for i in range(6):
            self._host.box[i] = float(bx[i])
        self._fill_extrinsics(extrinsics)
        self._seed_host = int(seed) & ((1 << 64) - 1)
        self._calib = None                             # device buffers: made on the first use of a GPU (the checks above need none)
        if torch.cuda.is_available():
            self._alloc()

    def _fill_extrinsics(self, extrinsics):
        import numpy as np
        T = np.asarray(extrinsics, dtype=np.float64)
        if T.shape not in ((self.K, 3, 4), (self.K, 4, 4)) or not np.isfinite(T).all():
            raise ValueError(f"RGBDFusion: extrinsics must be finite [{self.K}, 3, 4] or [{self.K}, 4, 4], got {T.shape}")
        for k in range(self.K):
            for i, v in enumerate(T[k, :3].reshape(12)):
                self._host.cam[k].T[i] = float(v)

    def _alloc(self):
        dev, MB, P, K = self.device, self.max_batch, self.P, self.K
        if self.sampling == "fps":
            nbytes = int(L.load().actmi_op_rgbd_cloud_fps_workspace_bytes(MB, K, self.H, self.W, self.fps_pool))
        else:
            nbytes = int(L.load().actmi_op_rgbd_cloud_workspace_bytes(MB, K, self.H, self.W))
        if nbytes < 0:
            raise ValueError(f"RGBDFusion: shape B = {MB}, K = {K}, {self.H} x {self.W} not supported by actmi_op_rgbd_cloud")
        self._ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        self._calib = torch.zeros(C.sizeof(L.RgbdCalib), dtype=torch.uint8, device=dev)
        self._seed = torch.zeros(1, dtype=torch.int64, device=dev)
        self.xyz = torch.zeros((MB, P, 3), dtype=torch.float32, device=dev)
        self.rgb = torch.zeros((MB, P, 3), dtype=torch.float32, device=dev)
        self.n = torch.zeros((MB,), dtype=torch.int32, device=dev)
        self.src_idx = torch.full((MB, P), -1, dtype=torch.int32, device=dev)
        self.survivors = torch.zeros((MB, K), dtype=torch.int32, device=dev)
        self.order = torch.full((MB, P), -1, dtype=torch.int32, device=dev) if self.sampling == "fps" else None
        self._push_calib()
        self.set_seed(self._seed_host)

    def _push_calib(self):
        if self._calib is not None:                    # a copy on the current stream: launches enqueued behind it, captured ones too, see it
            host = torch.frombuffer(bytearray(bytes(self._host)), dtype=torch.uint8)
            with torch.cuda.device(self.device):
                self._calib.copy_(host)

    def set_extrinsics(self, extrinsics):
        """new camera -> base transforms [K, 3, 4] or [K, 4, 4], copied into the device block on the current stream"""
        self._fill_extrinsics(extrinsics)
        self._push_calib()

    def set_seed(self, seed):
        """the 64-bit seed of the subset drawn where a camera has more survivors than its quota; a copy on the current stream"""
        self._seed_host = int(seed) & ((1 << 64) - 1)
        if self._calib is not None:
            v = self._seed_host - (1 << 64) if self._seed_host >= 1 << 63 else self._seed_host
            with torch.cuda.device(self.device):
                self._seed.copy_(torch.tensor([v], dtype=torch.int64))

    def check_inputs(self, image_u8, depth_u16, B):
        """the host-side checks of fuse(); returns depth as [B, K, H, W]"""
        K, H, W = self.K, self.H, self.W
        B = int(B)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"RGBDFusion: B = {B}: needs 1 <= B <= max_batch {self.max_batch}")
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8:
            raise ValueError(f"RGBDFusion: the image batch must be a uint8 [B, C, H, W, 3] tensor (the colours are its bytes), got "
                             f"{getattr(image_u8, 'dtype', type(image_u8))}")
        if image_u8.dim() != 5 or image_u8.shape[0] != B or tuple(image_u8.shape[2:]) != (H, W, 3):
            raise ValueError(f"RGBDFusion: image shape {tuple(image_u8.shape)} != {(B, 'C', H, W, 3)}")
        Cn = image_u8.shape[1]
        if (self.num_cams is not None and Cn != self.num_cams) or max(self.cam_index) >= Cn:
            raise ValueError(f"RGBDFusion: image holds {Cn} cameras; cam_index {self.cam_index}, num_cams {self.num_cams}")
        if not isinstance(depth_u16, torch.Tensor) or depth_u16.dtype != torch.uint16:
            raise ValueError(f"RGBDFusion: depth must be a uint16 tensor, got {getattr(depth_u16, 'dtype', type(depth_u16))}")
        if tuple(depth_u16.shape) == (B, K, 1, H, W):
            depth_u16 = depth_u16.view(B, K, H, W) if depth_u16.is_contiguous() else depth_u16.reshape(B, K, H, W)
        if tuple(depth_u16.shape) != (B, K, H, W):
            raise ValueError(f"RGBDFusion: depth shape {tuple(depth_u16.shape)} != {(B, K, H, W)} (or {(B, K, 1, H, W)})")
        if not (image_u8.is_contiguous() and depth_u16.is_contiguous()):
            raise ValueError("RGBDFusion: image and depth must be contiguous")
        for name, t in (("image", image_u8), ("depth", depth_u16)):
            if not t.is_cuda or t.device != self.device:
                raise ValueError(f"RGBDFusion: {name} lives on {t.device}, the fusion on {self.device}")
        return depth_u16

    def outputs(self, B):
        """the views fuse() returns, without a launch"""
        if self._calib is None:
            self._alloc()
        return {"xyz": self.xyz[:B], "rgb": self.rgb[:B], "n": self.n[:B]}

    def fuse(self, image_u8, depth_u16, B=None):
        B = int(depth_u16.shape[0] if B is None else B)
        depth_u16 = self.check_inputs(image_u8, depth_u16, B)
        if self._calib is None:
            self._alloc()
        d = L.RgbdDesc()
        d.depth, d.image, d.calib, d.seed = depth_u16.data_ptr(), image_u8.data_ptr(), self._calib.data_ptr(), self._seed.data_ptr()
        d.xyz, d.rgb, d.n = self.xyz.data_ptr(), self.rgb.data_ptr(), self.n.data_ptr()
        d.src_idx, d.survivors = self.src_idx.data_ptr(), self.survivors.data_ptr()
        d.ws, d.ws_bytes = self._ws.data_ptr(), self._ws.numel() * 8
        d.B, d.K, d.C, d.H, d.W, d.P = B, self.K, image_u8.shape[1], self.H, self.W, self.P
        for k in range(self.K):
            d.quota[k], d.cam_index[k] = self.quota[k], self.cam_index[k]
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            if self.sampling == "fps":
                f = L.RgbdFpsDesc()
                f.base, f.pool, f.order = d, self.fps_pool, self.order.data_ptr()
                L.check(L.load().actmi_op_rgbd_cloud_fps(C.byref(f), st), None, "op_rgbd_cloud_fps")
            else:
                L.check(L.load().actmi_op_rgbd_cloud(C.byref(d), st), None, "op_rgbd_cloud")
        return self.outputs(B)


# ---- training-time image augmentation (csrc/augment.hip; contract at actmi_augment_desc in actmi.h) ------------------------------
AUGMENT_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))      # 0 brightness, 1 contrast, 2 saturation


def augment_record_dtype():
    """actmi_augment_record as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("top", "<i4"), ("left", "<i4"), ("order", "<i4"), ("cos", "<f4"), ("sin", "<f4"), ("fb", "<f4"), ("fc", "<f4"),
                     ("fs", "<f4")])


def augment_records(B, top=0, left=0, angle=0.0, order=0, fb=1.0, fc=1.0, fs=1.0):
    """[B] records from numbers or [B] arrays; angle in degrees, counter-clockwise (torchvision's sign): cos and sin are taken in
    double on the host and rounded to float32.  The defaults are the identity when the crop is the whole frame."""
    import numpy as np
    r = np.zeros(int(B), dtype=augment_record_dtype())
    a = np.deg2rad(np.broadcast_to(np.asarray(angle, dtype=np.float64), (int(B),)))
    r["top"], r["left"], r["order"] = top, left, order
    r["cos"], r["sin"] = np.cos(a), np.sin(a)
    r["fb"], r["fc"], r["fs"] = fb, fc, fs
    return r


def _augment_geometry(H, W, ch, cw, rec):
    """the gather of one record in numpy float32: (inside [H, W] bool, y0, y1, x0, x1 int, wy, wx float32, top, left) -- and sx, sy
    for the tests that want to know how close a pixel sits to a rounding boundary"""
    import numpy as np
    f = np.float32
    cs, sn = f(rec["cos"]), f(rec["sin"])
    top = min(max(int(rec["top"]), 0), H - ch)
    left = min(max(int(rec["left"]), 0), W - cw)
    hw, hh = f(W) * f(0.5), f(H) * f(0.5)
    x = ((np.arange(W, dtype=f) + f(0.5)) - hw)[None, :]
    y = ((np.arange(H, dtype=f) + f(0.5)) - hh)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        sx = ((x * cs) - (y * sn)) + (hw - f(0.5))
        sy = ((x * sn) + (y * cs)) + (hh - f(0.5))
        fj, fi = np.rint(sx), np.rint(sy)
        inside = (fj >= 0) & (fj < W) & (fi >= 0) & (fi < H)
    rj = np.where(inside, fj, 0).astype(np.int64)
    ri = np.where(inside, fi, 0).astype(np.int64)

    def taps(r, n_in, n_out):
        c = np.maximum((r.astype(f) + f(0.5)) * (f(n_in) / f(n_out)) - f(0.5), f(0))
        i0 = np.minimum(np.floor(c).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), c - i0.astype(f)
    y0, y1, wy = taps(ri, ch, H)
    x0, x1, wx = taps(rj, cw, W)
    return inside, y0, y1, x0, x1, wy, wx, top, left, sx, sy


def _augment_warp(planes, H, W, ch, cw, rec):
    """planes [..., H, W] (any integer dtype) -> the warped planes as float32 whole numbers (before the cast)"""
    import numpy as np
    f = np.float32
    inside, y0, y1, x0, x1, wy, wx, top, left, _, _ = _augment_geometry(H, W, ch, cw, rec)
    v = planes.astype(f)
    v00, v01 = v[..., top + y0, left + x0], v[..., top + y0, left + x1]
    v10, v11 = v[..., top + y1, left + x0], v[..., top + y1, left + x1]
    t0 = (v00 * (f(1) - wx)) + (v01 * wx)
    t1 = (v10 * (f(1) - wx)) + (v11 * wx)
    out = np.rint((t0 * (f(1) - wy)) + (t1 * wy))
    return np.where(inside, out, f(0))


def _augment_jitter(x, rec):
    """x [K, H, W, 3] float32 whole numbers 0..255 -> the same after the record's three ops"""
    import numpy as np
    f = np.float32

    def gray(a):
        return np.trunc(((f(0.2989) * a[..., 0]) + (f(0.587) * a[..., 1])) + (f(0.114) * a[..., 2]))[..., None]

    def blend(a, b, r):
        r = f(r)
        return np.trunc(np.clip((r * a) + ((f(1) - r) * b), f(0), f(255)))
    for op in AUGMENT_ORDERS[min(max(int(rec["order"]), 0), 5)]:
        if op == 0:
            x = blend(x, f(0), rec["fb"])
        elif op == 1:
            g = gray(x)
            total = g.astype(np.int64).sum(axis=(1, 2, 3), keepdims=True)                   # per camera image, exact
            mean = (total.astype(np.float64) / float(g.shape[1] * g.shape[2])).astype(f)
            x = blend(x, mean, rec["fc"])
        else:
            x = blend(x, gray(x), rec["fs"])
    return x


def image_augment_ref(image_u8, records, ch, cw):
    """actmi_op_augment_u8 in numpy: the definition at actmi_augment_desc in actmi.h stated once more -- the oracle of the device
    op, not a fallback for it.  image_u8 [B, K, H, W, 3] uint8 (numpy or a CPU tensor), records [B] (augment_record_dtype) ->
    numpy uint8 of the same shape."""
    import numpy as np
    img = np.asarray(image_u8)
    B, K, H, W, _ = img.shape
    ch, cw = int(ch), int(cw)
    if img.dtype != np.uint8 or img.shape[4] != 3 or len(records) != B or not (1 <= ch <= H and 1 <= cw <= W):
        raise ValueError(f"image_augment_ref: frames {img.dtype} {img.shape}, {len(records)} records, crop {ch} x {cw}")
    out = np.empty_like(img)
    for b in range(B):
        planes = np.moveaxis(img[b], -1, 1)                                                  # [K, 3, H, W]
        warped = np.moveaxis(_augment_warp(planes, H, W, ch, cw, records[b]), 1, -1)         # [K, H, W, 3]
        out[b] = _augment_jitter(warped, records[b]).astype(np.uint8)
    return out


def depth_warp_ref(depth_u16, records, ch, cw):
    """actmi_op_warp_u16 in numpy: the geometric steps of image_augment_ref on uint16 [B, Kd, H, W] (or [B, Kd, 1, H, W]) frames"""
    import numpy as np
    d = np.asarray(depth_u16)
    H, W = d.shape[-2:]
    ch, cw = int(ch), int(cw)
    if d.dtype != np.uint16 or d.ndim not in (4, 5) or len(records) != d.shape[0] or not (1 <= ch <= H and 1 <= cw <= W):
        raise ValueError(f"depth_warp_ref: frames {d.dtype} {d.shape}, {len(records)} records, crop {ch} x {cw}")
    out = np.empty_like(d)
    for b in range(d.shape[0]):
        out[b] = np.clip(_augment_warp(d[b], H, W, ch, cw, records[b]), 0, 65535).astype(np.uint16)
    return out


class _RecordRing:
    """The device block of an augmenter's records, one per sample, and the ring of pinned host blocks it is fed through: an upload
    is stream-ordered, and the pinned block a copy reads from is not rewritten before that copy has run (an event each)."""
    RING = 4

    def __init__(self, device, nbytes):
        self.device = device
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self._host = [torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        self._events = [None] * self.RING
        self._slot = 0

    def upload(self, rec):
        """rec: a contiguous numpy record array -> the front of the device block, on the current stream"""
        n = rec.nbytes
        i = self._slot
        self._slot = (i + 1) % self.RING
        if self._events[i] is not None:
            self._events[i].synchronize()
        self._host[i].numpy()[:n] = rec.view("u1")
        with torch.cuda.device(self.device):
            self.dev[:n].copy_(self._host[i][:n], non_blocking=True)
            self._events[i] = torch.cuda.Event()
            self._events[i].record(torch.cuda.current_stream(self.device))


class ImageAugment:
    """The reference dataset's training augmentation (utils.py:141-156: RandomCrop at `ratio`, Resize back with antialias,
    RandomRotation within `degrees`, ColorJitter) as one device op over the u8 batch of a training step (actmi_op_augment_u8), and
    the three geometric steps over the raw uint16 depth frames of a use_depth batch with the SAME draws (actmi_op_warp_u16).  Owns
    the output buffers, the workspace, and the records (a _RecordRing).

    engine_or_device: an ACTEngine (its device) or a device.  K cameras (Kd depth cameras, 0: none) of H x W pixels.  One draw per
    SAMPLE: top, left uniform integers over the crop's positions, angle U[-degrees, degrees], factors U[1 - x, 1 + x] (not below
    0), order uniform over the 6 -- from a numpy.random.Generator seeded with `seed`.  The distributions are torchvision's;
    draw-for-draw parity with torchvision's generator is not claimed.

    draw(B) fills and uploads records; run(image_u8, depth_u16, B) launches with the records on the device; apply = draw + run.
    The returned tensors are views of the augmenter's own buffers, valid until the next run."""

    def __init__(self, engine_or_device, K, H, W, max_batch, ratio=0.95, degrees=5.0, brightness=0.3, contrast=0.4, saturation=0.5,
                 seed=0, Kd=0):
        import numpy as np
        eng = engine_or_device if hasattr(engine_or_device, "cfg") else None
        self.device = torch.device(eng.device if eng is not None else engine_or_device)
        if self.device.type != "cuda":
            raise ValueError(f"ImageAugment: device must be a cuda device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.K, self.Kd, self.H, self.W, self.max_batch = int(K), int(Kd), int(H), int(W), int(max_batch)
        if self.K < 1 or self.Kd < 0 or self.H < 1 or self.W < 1 or self.max_batch < 1:
            raise ValueError(f"ImageAugment: K = {K}, Kd = {Kd}, {H} x {W}, max_batch = {max_batch}")
        if not 0.0 < ratio <= 1.0 or degrees < 0 or min(brightness, contrast, saturation) < 0:
            raise ValueError(f"ImageAugment: ratio {ratio} outside (0, 1], or a negative range")
        self.ch, self.cw = max(1, int(self.H * ratio)), max(1, int(self.W * ratio))           # utils.py:147
        self.degrees = float(degrees)
        self.ranges = tuple((max(0.0, 1.0 - float(x)), 1.0 + float(x)) for x in (brightness, contrast, saturation))
        self._np = np
        self.set_seed(seed)
        self._ring = None                                  # device and pinned buffers: made on the first use of a GPU
        self._last = np.zeros(0, dtype=augment_record_dtype())
        if torch.cuda.is_available():
            self._alloc()

    def _alloc(self):
        dev, MB = self.device, self.max_batch
        nbytes = max(int(L.load().actmi_op_augment_workspace_bytes(MB, k, self.H, self.W)) for k in (self.K, max(self.Kd, 1)))
        if nbytes < 0:
            raise ValueError(f"ImageAugment: shape B = {MB}, K = {self.K}, {self.H} x {self.W} not supported by actmi_op_augment_u8")
        self._ws = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        self._ring = _RecordRing(dev, MB * 32)
        self.out = torch.zeros((MB, self.K, self.H, self.W, 3), dtype=torch.uint8, device=dev)
        self.depth_out = torch.zeros((MB, self.Kd, 1, self.H, self.W), dtype=torch.uint16, device=dev) if self.Kd else None

    def set_seed(self, seed):
        """restart the generator of the draws"""
        self._rng = self._np.random.default_rng(int(seed))

    def draw_records(self, B):
        """[B] fresh records on the host (nothing is uploaded)"""
        rng, B = self._rng, int(B)
        top = rng.integers(0, self.H - self.ch + 1, size=B)
        left = rng.integers(0, self.W - self.cw + 1, size=B)
        angle = rng.uniform(-self.degrees, self.degrees, size=B)
        fb, fc, fs = (rng.uniform(lo, hi, size=B) for lo, hi in self.ranges)
        order = rng.integers(0, 6, size=B)
        return augment_records(B, top, left, angle, order, fb, fc, fs)

    def set_records(self, records):
        """upload [B] records (augment_record_dtype) on the current stream: launches enqueued behind it, captured ones too, see
        them.  The pinned block a copy reads from is not rewritten before that copy has run (a ring of blocks, an event each)."""
        rec = self._np.ascontiguousarray(records, dtype=augment_record_dtype())
        B = len(rec)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"ImageAugment: {B} records: needs 1 <= B <= max_batch {self.max_batch}")
        self._last = rec.copy()
        if self._ring is None:
            self._alloc()
        self._ring.upload(rec)

    def records(self):
        """the records of the last draw / set_records, on the host"""
        return self._last.copy()

    def draw(self, B):
        self.set_records(self.draw_records(B))

    def _check(self, name, t, dtype, shape):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise NotImplementedError(f"ImageAugment: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))} (the "
                                      f"augmentation runs on the raw frames)")
        if tuple(t.shape) != shape:
            raise ValueError(f"ImageAugment: {name} shape {tuple(t.shape)} != {shape}")
        if not t.is_cuda or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"ImageAugment: {name} must be contiguous on {self.device} (it is on {t.device})")

    def run(self, image_u8, depth_u16=None, B=None):
        """launch with the records on the device -> the augmented image batch, or (image, depth) when depth frames are given"""
        B = int(image_u8.shape[0] if B is None else B)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"ImageAugment: B = {B}: needs 1 <= B <= max_batch {self.max_batch}")
        self._check("image", image_u8, torch.uint8, (B, self.K, self.H, self.W, 3))
        if depth_u16 is not None:
            if not self.Kd:
                raise ValueError("ImageAugment: depth frames given to an augmenter built with Kd = 0")
            if isinstance(depth_u16, torch.Tensor) and tuple(depth_u16.shape) == (B, self.Kd, self.H, self.W):
                depth_u16 = depth_u16.unsqueeze(2)
            self._check("depth", depth_u16, torch.uint16, (B, self.Kd, 1, self.H, self.W))
        if self._ring is None:
            self._alloc()
        d = L.AugmentDesc()
        d.records, d.ws, d.ws_bytes = self._ring.dev.data_ptr(), self._ws.data_ptr(), self._ws.numel() * 4
        d.B, d.H, d.W, d.ch, d.cw = B, self.H, self.W, self.ch, self.cw
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            d.in_, d.out, d.K = image_u8.data_ptr(), self.out.data_ptr(), self.K
            L.check(L.load().actmi_op_augment_u8(C.byref(d), st), None, "op_augment_u8")
            if depth_u16 is None:
                return self.out[:B]
            d.in_, d.out, d.K = depth_u16.data_ptr(), self.depth_out.data_ptr(), self.Kd
            L.check(L.load().actmi_op_warp_u16(C.byref(d), st), None, "op_warp_u16")
        return self.out[:B], self.depth_out[:B]

    def apply(self, image_u8, depth_u16=None, B=None):
        """one fresh draw per sample, then run"""
        self.draw(int(image_u8.shape[0] if B is None else B))
        return self.run(image_u8, depth_u16, B)


# ---- training-time point-cloud augmentation (csrc/cloud_augment.hip; contract at actmi_cloud_augment_desc in actmi.h) ------------
def cloud_augment_record_dtype():
    """actmi_cloud_augment_record as a numpy structured dtype (56 bytes)"""
    import numpy as np
    return np.dtype([(k, "<f4") for k in ("cos", "sin", "scale", "tx", "ty", "tz", "jitter", "drop", "fb", "fc", "fs")] +
                    [("order", "<i4"), ("seed_lo", "<u4"), ("seed_hi", "<u4")])


def cloud_augment_records(B, angle=0.0, scale=1.0, shift=(0, 0, 0), jitter=0.0, drop=0.0, order=0, fb=1.0, fc=1.0, fs=1.0, seed=0):
    """[B] records from numbers or [B] arrays (shift: 3 numbers or [B, 3]; seed: 64-bit integers); angle in degrees about +z,
    counter-clockwise seen from above: cos and sin are taken in double on the host and rounded to float32.  The defaults are the
    identity."""
    import numpy as np
    B = int(B)
    r = np.zeros(B, dtype=cloud_augment_record_dtype())
    a = np.deg2rad(np.broadcast_to(np.asarray(angle, dtype=np.float64), (B,)))
    r["cos"], r["sin"] = np.cos(a), np.sin(a)
    r["scale"], r["jitter"], r["drop"], r["order"] = scale, jitter, drop, order
    t = np.broadcast_to(np.asarray(shift, dtype=np.float64), (B, 3))
    r["tx"], r["ty"], r["tz"] = t[:, 0], t[:, 1], t[:, 2]
    r["fb"], r["fc"], r["fs"] = fb, fc, fs
    s = np.broadcast_to(np.asarray(seed, dtype=np.uint64), (B,))
    r["seed_lo"], r["seed_hi"] = s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)
    return r


def _mix32(x):
    """actmi_mix32 of csrc/dropout.h on a uint32 array (products wrap)"""
    import numpy as np
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def u01_ref(seed, idx):
    """actmi_u01 of csrc/dropout.h in numpy: seed a 64-bit integer, idx an array of 64-bit element indices -> float32 in [0, 1),
    24 bits each"""
    import numpy as np
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    h = _mix32(lo ^ np.uint32(seed & 0xFFFFFFFF))
    h = _mix32(h ^ hi ^ np.uint32(seed >> 32) ^ np.uint32(0x9E3779B9))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _cloud_counts(n, B, P):
    import numpy as np
    if n is None:
        return np.full(B, P, np.int64)
    n = np.asarray(n).astype(np.int64).reshape(-1)
    if len(n) != B:
        raise ValueError(f"cloud_augment_ref: {len(n)} counts for {B} samples")
    return np.clip(n, 1, P)


def cloud_augment_ref(xyz, rgb, n, records, pivot):
    """actmi_op_cloud_augment in numpy: the definition at actmi_cloud_augment_desc in actmi.h stated once more -- the oracle of the
    device op, not a fallback for it.  xyz, rgb [B, P, 3] float32 (numpy or CPU tensors), n [B] integers or None (P everywhere),
    records [B] (cloud_augment_record_dtype), pivot 3 numbers -> (xyz, rgb [B, P, 3] float32, counts [B] int32), numpy."""
    import numpy as np
    f = np.float32
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    if xyz.dtype != f or rgb.dtype != f or xyz.ndim != 3 or xyz.shape[2] != 3 or rgb.shape != xyz.shape or len(records) != len(xyz):
        raise ValueError(f"cloud_augment_ref: xyz {xyz.dtype} {xyz.shape}, rgb {rgb.dtype} {rgb.shape}, {len(records)} records")
    B, P, _ = xyz.shape
    counts = _cloud_counts(n, B, P)
    pv = np.asarray(pivot, dtype=f).reshape(3)
    out_xyz, out_rgb, out_n = np.zeros_like(xyz), np.zeros_like(rgb), np.zeros(B, np.int32)

    def gray(c):
        return ((f(0.2989) * c[:, 0]) + (f(0.587) * c[:, 1])) + (f(0.114) * c[:, 2])

    def blend(a, b, r):
        return np.fmin(np.fmax((r * a) + ((f(1) - r) * b), f(0)), f(255))       # fmax / fmin: the operand that is a number

    with np.errstate(all="ignore"):
        for b in range(B):
            rec, m = records[b], int(counts[b])
            seed = int(rec["seed_lo"]) | int(rec["seed_hi"]) << 32
            u = u01_ref(seed, np.arange(4 * m, dtype=np.uint64)).reshape(m, 4)
            d = xyz[b, :m] - pv
            cs, sn = f(rec["cos"]), f(rec["sin"])
            r = np.stack([(d[:, 0] * cs) - (d[:, 1] * sn), (d[:, 0] * sn) + (d[:, 1] * cs), d[:, 2]], axis=1)
            t = np.array([rec["tx"], rec["ty"], rec["tz"]], dtype=f)
            j = ((u[:, :3] + u[:, :3]) - f(1)) * f(rec["jitter"])
            q = (((r * f(rec["scale"])) + pv) + t) + j
            c = rgb[b, :m]
            for op in AUGMENT_ORDERS[min(max(int(rec["order"]), 0), 5)]:
                if op == 0:
                    c = blend(c, f(0), f(rec["fb"]))
                elif op == 1:
                    total = int(np.trunc(np.fmin(np.fmax(gray(c), f(0)), f(255))).astype(np.int64).sum())       # exact
                    c = blend(c, f(np.float64(total) / np.float64(m)), f(rec["fc"]))
                else:
                    c = blend(c, gray(c)[:, None], f(rec["fs"]))
            keep = u[:, 3] >= f(rec["drop"])
            if not keep.any():
                keep[0] = True
            k = int(keep.sum())
            out_xyz[b, :k], out_rgb[b, :k], out_n[b] = q[keep], c[keep], k
    return out_xyz, out_rgb, out_n


def _cloud_check(name, t, B, P, device=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"cloud_augment: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 3 or t.shape[2] != 3 or (B is not None and tuple(t.shape) != (B, P, 3)):
        raise ValueError(f"cloud_augment: {name} shape {tuple(t.shape)} != {(B if B is not None else 'B', P if B is not None else 'P', 3)}")
    if not t.is_cuda or not t.is_contiguous() or (device is not None and t.device != device):
        raise ValueError(f"cloud_augment: {name} must be contiguous on {device or 'a cuda device'} (it is on {t.device})")


def _cloud_counts_check(n, B, device):
    if n is None:
        return
    if not isinstance(n, torch.Tensor) or n.dtype != torch.int32:
        raise TypeError(f"cloud_augment: n must be an int32 tensor, got {getattr(n, 'dtype', type(n))}")
    if tuple(n.shape) != (B,) or not n.is_contiguous() or n.device != device:
        raise ValueError(f"cloud_augment: n shape {tuple(n.shape)} on {n.device} != {(B,)} (contiguous) on {device}")


def _cloud_launch(xyz, rgb, n, rec_ptr, pivot, out_xyz, out_rgb, out_n, B, P):
    d = L.CloudAugmentDesc()
    d.xyz, d.rgb, d.counts, d.records = xyz.data_ptr(), rgb.data_ptr(), (n.data_ptr() if n is not None else None), rec_ptr
    d.out_xyz, d.out_rgb, d.out_counts = out_xyz.data_ptr(), out_rgb.data_ptr(), out_n.data_ptr()
    d.pivot[0], d.pivot[1], d.pivot[2] = (float(v) for v in pivot)
    d.B, d.P = B, P
    with torch.cuda.device(xyz.device):
        st = C.c_void_p(torch.cuda.current_stream(xyz.device).cuda_stream)
        L.check(L.load().actmi_op_cloud_augment(C.byref(d), st), None, "op_cloud_augment")


def cloud_augment(xyz, rgb, n, records, pivot, out=None):
    """actmi_op_cloud_augment, the raw op: xyz, rgb [B, P, 3] float32 on the device, n int32 [B] on the device or None, records
    [B] -- a numpy array of cloud_augment_record_dtype (uploaded here, which waits for the copy) or a uint8 device tensor of B * 56
    bytes -- and the pivot's 3 numbers -> (xyz, rgb, counts) in `out` (three tensors of those shapes) or in fresh ones."""
    import numpy as np
    _cloud_check("xyz", xyz, None, None)
    B, P, _ = xyz.shape
    _cloud_check("rgb", rgb, B, P, xyz.device)
    _cloud_counts_check(n, B, xyz.device)
    if not isinstance(records, torch.Tensor):
        rec = np.ascontiguousarray(records, dtype=cloud_augment_record_dtype())
        records = torch.from_numpy(rec.view(np.uint8).copy()).to(xyz.device)
    if records.dtype != torch.uint8 or records.numel() != B * 56 or records.device != xyz.device or not records.is_contiguous():
        raise ValueError(f"cloud_augment: records must be {B} x 56 bytes (uint8, contiguous) on {xyz.device}")
    if out is None:
        out = (torch.empty_like(xyz), torch.empty_like(rgb), torch.empty(B, dtype=torch.int32, device=xyz.device))
    out_xyz, out_rgb, out_n = out
    _cloud_check("out xyz", out_xyz, B, P, xyz.device)
    _cloud_check("out rgb", out_rgb, B, P, xyz.device)
    _cloud_counts_check(out_n, B, xyz.device)
    _cloud_launch(xyz, rgb, n, records.data_ptr(), pivot, out_xyz, out_rgb, out_n, B, P)
    return out_xyz, out_rgb, out_n


class CloudAugment:
    """Training augmentation for the stored clouds of a use_pcd batch, as one device op (actmi_op_cloud_augment): a yaw about +z
    of the cloud's frame, an isotropic scale about `pivot`, a shift, a per-point uniform jitter, random point dropout, and
    ImageAugment's colour jitter on the points' colours (0..255 floats).  Owns the output buffers and the records (a _RecordRing),
    as ImageAugment does.

    engine_or_device: an ACTEngine (its device) or a device.  Clouds of up to `max_points` points, batches of up to `max_batch`.
    One draw per SAMPLE from a numpy.random.Generator seeded with `seed`: angle U[-degrees, degrees], scale U[1 - scale, 1 + scale],
    each shift component U[-shift, shift] (the cloud's units: metres for the recorder's clouds), the three colour factors
    U[1 - x, 1 + x] (not below 0) and the order uniform over the 6 as ImageAugment draws them, and 64 seed bits for the per-point
    draws; `jitter` (the half width of the per-coordinate uniform jitter) and `drop` (the probability that a point is dropped) go
    into every record as they are.

    The defaults are choices, not measurements: the image augmentation's 5 degrees and colour ranges, 5 % of scale, a centimetre
    of shift, 2 mm of jitter -- about a depth camera's noise at arm's length -- and a tenth of the points dropped.  No training run
    has tuned them; the reference has no cloud augmentation to take them from.

    draw(B) fills and uploads records; run(xyz, rgb, n) launches with the records on the device; apply = draw + run.  The
    returned tensors are views of the augmenter's own buffers, valid until the next run."""
    REC = 56

    def __init__(self, engine_or_device, max_points, max_batch, pivot=(0, 0, 0), degrees=5.0, scale=0.05, shift=0.01, jitter=0.002,
                 drop=0.1, brightness=0.3, contrast=0.4, saturation=0.5, seed=0):
        import numpy as np
        eng = engine_or_device if hasattr(engine_or_device, "cfg") else None
        self.device = torch.device(eng.device if eng is not None else engine_or_device)
        if self.device.type != "cuda":
            raise ValueError(f"CloudAugment: device must be a cuda device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.max_points, self.max_batch = int(max_points), int(max_batch)
        if self.max_points < 1 or not 1 <= self.max_batch <= 65535:
            raise ValueError(f"CloudAugment: max_points = {max_points}, max_batch = {max_batch}")
        self.pivot = tuple(float(v) for v in pivot)
        if len(self.pivot) != 3 or not all(np.isfinite(self.pivot)):
            raise ValueError(f"CloudAugment: pivot {pivot} is not 3 finite numbers")
        if min(degrees, scale, shift, jitter, brightness, contrast, saturation) < 0 or scale >= 1 or not 0.0 <= drop < 1.0:
            raise ValueError("CloudAugment: a negative range, scale >= 1, or drop outside [0, 1)")
        self.degrees, self.scale, self.shift, self.jitter, self.drop = (float(v) for v in (degrees, scale, shift, jitter, drop))
        self.ranges = tuple((max(0.0, 1.0 - float(x)), 1.0 + float(x)) for x in (brightness, contrast, saturation))
        self._np = np
        self.set_seed(seed)
        self._ring = None                                  # device and pinned buffers: made on the first use of a GPU
        self._last = np.zeros(0, dtype=cloud_augment_record_dtype())
        if torch.cuda.is_available():
            self._alloc()

    def _alloc(self):
        dev, MB = self.device, self.max_batch
        self._ring = _RecordRing(dev, MB * self.REC)
        self.out_xyz = torch.zeros(MB * self.max_points * 3, dtype=torch.float32, device=dev)
        self.out_rgb = torch.zeros(MB * self.max_points * 3, dtype=torch.float32, device=dev)
        self.out_n = torch.zeros(MB, dtype=torch.int32, device=dev)

    def set_seed(self, seed):
        """restart the generator of the draws"""
        self._rng = self._np.random.default_rng(int(seed))

    def draw_records(self, B):
        """[B] fresh records on the host (nothing is uploaded)"""
        rng, B = self._rng, int(B)
        angle = rng.uniform(-self.degrees, self.degrees, size=B)
        scale = rng.uniform(1.0 - self.scale, 1.0 + self.scale, size=B)
        shift = rng.uniform(-self.shift, self.shift, size=(B, 3))
        fb, fc, fs = (rng.uniform(lo, hi, size=B) for lo, hi in self.ranges)
        order = rng.integers(0, 6, size=B)
        seed = rng.integers(0, 1 << 64, size=B, dtype=self._np.uint64)
        return cloud_augment_records(B, angle, scale, shift, self.jitter, self.drop, order, fb, fc, fs, seed)

    def set_records(self, records):
        """upload [B] records (cloud_augment_record_dtype) on the current stream: launches enqueued behind it, captured ones too,
        see them.  The pinned block a copy reads from is not rewritten before that copy has run (a ring of blocks, an event each)."""
        rec = self._np.ascontiguousarray(records, dtype=cloud_augment_record_dtype())
        B = len(rec)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"CloudAugment: {B} records: needs 1 <= B <= max_batch {self.max_batch}")
        self._last = rec.copy()
        if self._ring is None:
            self._alloc()
        self._ring.upload(rec)

    def records(self):
        """the records of the last draw / set_records, on the host"""
        return self._last.copy()

    def draw(self, B):
        self.set_records(self.draw_records(B))

    def run(self, xyz, rgb, n=None):
        """launch with the records on the device -> (xyz, rgb [B, P, 3], n int32 [B]): the kept points in front, zeros behind"""
        _cloud_check("xyz", xyz, None, None, self.device)
        B, P, _ = xyz.shape
        if not 1 <= B <= self.max_batch or P > self.max_points:
            raise ValueError(f"CloudAugment: clouds {tuple(xyz.shape)}: needs B <= max_batch {self.max_batch}, 1 <= P <= max_points "
                             f"{self.max_points}")
        _cloud_check("rgb", rgb, B, P, self.device)
        _cloud_counts_check(n, B, self.device)
        if self._ring is None:
            self._alloc()
        out = self.out_xyz[:B * P * 3].view(B, P, 3), self.out_rgb[:B * P * 3].view(B, P, 3), self.out_n[:B]
        _cloud_launch(xyz, rgb, n, self._ring.dev.data_ptr(), self.pivot, *out, B, P)
        return out

    def apply(self, xyz, rgb, n=None):
        """one fresh draw per sample, then run -> (xyz, rgb, n) for the policy's pointcloud"""
        self.draw(int(xyz.shape[0]))
        return self.run(xyz, rgb, n)


class TemporalEnsemble:
    """Batched temporal ensembling state for E episodes (reference imitate_episodes.py:338-339, 402-411).
    Ring buffer [E,Q,Q,A] instead of the reference's [T,T+Q,A] per episode: only the last Q chunks can
    contribute to step t."""

    def __init__(self, num_episodes, num_queries, action_dim=16, k=0.01, device="cuda:0"):
        self.E, self.Q, self.A, self.k = num_episodes, num_queries, action_dim, float(k)
        self.ring = torch.zeros((self.E, self.Q, self.Q, self.A), dtype=torch.float32, device=device)
        self.t = torch.zeros((self.E,), dtype=torch.int32, device=device)
        self.out = torch.zeros((self.E, self.A), dtype=torch.float64, device=device)
        self.populated = torch.zeros((self.E, self.Q), dtype=torch.uint8, device=device)

    def reset(self):
        self.ring.zero_()
        self.t.zero_()

    def step(self, all_actions):
        """all_actions [E,Q,A] f32 cuda -> raw_action [E,A] f64 (same dtype as the reference's raw_action)."""
        lib = L.load()
        a = all_actions.contiguous()
        dev = self.ring.device
        if a.device != dev:
            raise ValueError(f"all_actions lives on {a.device} but this ensemble is bound to {dev}")
        with torch.cuda.device(dev):          # the kernel launches on the ring's device whatever the caller left current
            L.check(lib.actmi_ensemble_step(_p(self.ring), _p(self.t), _p(a), self.k, _p(self.out), _p(self.populated),
                                            self.E, self.Q, self.A, L.current_stream_ptr()), None, "ensemble_step")
        return self.out


# ---- open-loop replay of recorded episodes (csrc/replay_eval.hip) --------------------------------------------------------------
def _device_table(name, t, dtype, dims):
    """the operand ``name`` of a replay op: a cuda tensor of ``dtype`` with the dimensions ``dims`` ("E, T, Q, A") -> contiguous"""
    if t.dim() != dims.count(",") + 1 or t.dtype != dtype or not t.is_cuda:
        raise ValueError(f"{name} must be a {str(dtype)[6:]} cuda tensor [{dims}], got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _stats_f64(op, mean, std, A, dev, optional=False):
    """mean / std of the A action components -> float64 [A] tensors on ``dev``; ``optional``: both may be None, together"""
    if optional and (mean is None or std is None):
        if (mean is None) != (std is None):
            raise ValueError(f"{op}: mean and std come together")
        return None, None
    mean, std = (torch.as_tensor(v).to(device=dev, dtype=torch.float64).reshape(-1).contiguous() for v in (mean, std))
    if mean.numel() != A or std.numel() != A:
        raise ValueError(f"{op}: mean / std hold {mean.numel()} / {std.numel()} values for action_dim {A}")
    return mean, std


def _lengths_i32(lengths, E, T, device):
    if lengths is None:
        return None
    ln = torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()
    if tuple(ln.shape) != (E,):
        raise ValueError(f"lengths has shape {tuple(ln.shape)}, expected ({E},)")
    return ln


def episode_ensemble(chunks, lengths=None, k=0.01, want_populated=False):
    """The temporal ensemble of every step of every episode in one launch (actmi_op_ensemble_episode).  chunks [E, T, Q, A] f32
    cuda: row (e, r) is the chunk predicted from frame r; lengths [E] (valid steps per episode; None: all T) -> raw [E, T, A]
    f64, and with ``want_populated`` the u8 mask [E, T, Q] of the rows that counted (row j of step t is r = t-(Q-1)+j).  Step t
    of episode e is bit for bit what the t-th ``TemporalEnsemble.step`` gives on the same chunks; rows t >= lengths[e] are
    zeros."""
    chunks = _device_table("chunks", chunks, torch.float32, "E, T, Q, A")
    E, T, Q, A = (int(v) for v in chunks.shape)
    dev = chunks.device
    ln = _lengths_i32(lengths, E, T, dev)
    out = torch.empty((E, T, A), dtype=torch.float64, device=dev)
    pop = torch.empty((E, T, Q), dtype=torch.uint8, device=dev) if want_populated else None
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_ensemble_episode(_p(chunks), _p(ln), float(k), _p(out), _p(pop), E, T, Q, A,
                                                   L.current_stream_ptr()), None, "op_ensemble_episode")
    return (out, pop) if want_populated else out


def episode_ensemble_ref(chunks, lengths=None, k=0.01, want_populated=False):
    """numpy statement of ``episode_ensemble`` (reference imitate_episodes.py:402-411 for every step at once); needs no library.
    chunks: ndarray or CPU tensor [E, T, Q, A] -> raw [E, T, A] float64 (and the bool mask [E, T, Q])."""
    import numpy as np
    c = np.asarray(chunks, dtype=np.float32)
    E, T, Q, A = c.shape
    ln = np.full(E, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    out = np.zeros((E, T, A), dtype=np.float64)
    pop = np.zeros((E, T, Q), dtype=bool)
    for e in range(E):
        for t in range(int(ln[e])):
            j = np.arange(max(0, Q - 1 - t), Q)             # the candidate rows that exist: r = t-(Q-1)+j >= 0
            r = t - (Q - 1) + j
            rows = c[e, r, t - r]                           # [n, A], oldest first
            ok = np.all(rows != 0, axis=1)
            pop[e, t, j] = ok
            rows = rows[ok]
            if len(rows):
                w = np.exp(-float(k) * np.arange(len(rows)))
                out[e, t] = (rows.astype(np.float64) * (w / w.sum())[:, None]).sum(axis=0)
    return (out, pop) if want_populated else out


def action_error(raw, target, lengths, mean, std, want_pred=True):
    """Un-normalise and compare with the recording on the device (actmi_op_action_error).  raw [E, T, A] f64 cuda, target
    [E, T, A] f32 (file units, already aligned), lengths [E] or None, mean / std [A] -> (pred [E, T, A] f64 = raw * std + mean
    or None, stats [E, 3, A] f64 = sum |d|, sum d^2, max |d| over t < lengths[e], d = pred - target)."""
    raw = _device_table("raw", raw, torch.float64, "E, T, A")
    E, T, A = (int(v) for v in raw.shape)
    dev = raw.device
    target = torch.as_tensor(target).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(target.shape) != (E, T, A):
        raise ValueError(f"target has shape {tuple(target.shape)}, expected {(E, T, A)}")
    mean, std = _stats_f64("action_error", mean, std, A, dev)
    ln = _lengths_i32(lengths, E, T, dev)
    pred = torch.empty((E, T, A), dtype=torch.float64, device=dev) if want_pred else None
    stats = torch.empty((E, 3, A), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_action_error(_p(raw), _p(target), _p(ln), _p(mean), _p(std), _p(pred), _p(stats), E, T, A,
                                               L.current_stream_ptr()), None, "op_action_error")
    return pred, stats


def action_error_ref(raw, target, lengths, mean, std, want_pred=True):
    """numpy statement of ``action_error`` (float64); needs no library.  -> (pred, stats) as ndarrays."""
    import numpy as np
    raw = np.asarray(raw, dtype=np.float64)
    E, T, A = raw.shape
    pred = raw * np.asarray(std, dtype=np.float64).reshape(1, 1, A) + np.asarray(mean, dtype=np.float64).reshape(1, 1, A)
    d = np.abs(pred - np.asarray(target, dtype=np.float32).astype(np.float64))
    ln = np.full(E, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    stats = np.zeros((E, 3, A), dtype=np.float64)
    for e in range(E):
        de = d[e, :int(ln[e])]
        if len(de):
            stats[e] = np.stack([de.sum(axis=0), (de * de).sum(axis=0), de.max(axis=0)])
    return (pred if want_pred else None), stats


def chunk_error(chunks, actions, lengths, shift, mean, std, stride=1):
    """The error along the predicted chunk on the device (actmi_op_chunk_error).  chunks [E, S, Q, A] f32 cuda (normalised
    a_hat): row s is the chunk predicted from frame r = s * stride; actions [E, T, A] f32 (file units, NOT aligned); lengths [E]
    or None (= T); shift [E] of 0 / 1 or None (= 0; 1: a real-robot episode under align="train"); mean / std [A].  Slot j of row
    s is compared with actions[e, max(0, r - shift[e]) + j] while r and that index are below the length: the entries the dataset
    trains the slot on.  -> (stats [E, Q, 3, A] f64 = sum |d|, sum d^2, max |d|, count [E, Q] int32 pairs per slot)."""
    chunks = _device_table("chunks", chunks, torch.float32, "E, S, Q, A")
    E, S, Q, A = (int(v) for v in chunks.shape)
    dev = chunks.device
    actions = torch.as_tensor(actions).to(device=dev, dtype=torch.float32).contiguous()
    if actions.dim() != 3 or int(actions.shape[0]) != E or int(actions.shape[2]) != A:
        raise ValueError(f"actions has shape {tuple(actions.shape)}, expected ({E}, T, {A})")
    T, stride = int(actions.shape[1]), int(stride)
    if E > 65535 or Q > 65535 or Q < 1 or A < 1 or T < 1 or stride < 1:
        raise ValueError(f"chunk_error: E {E} and Q {Q} must be at most 65535, Q, A {A}, T {T} and stride {stride} at least 1")
    mean, std = _stats_f64("chunk_error", mean, std, A, dev)
    ln = _lengths_i32(lengths, E, T, dev)
    sh = _lengths_i32(shift, E, T, dev)
    if not (E and S):                            # nothing is launched: the zeros are the answer
        return torch.zeros((E, Q, 3, A), dtype=torch.float64, device=dev), torch.zeros((E, Q), dtype=torch.int32, device=dev)
    stats = torch.empty((E, Q, 3, A), dtype=torch.float64, device=dev)      # the kernel writes every entry, the empty slots' zeros too
    count = torch.empty((E, Q), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_chunk_error(_p(chunks), _p(actions), _p(ln), _p(sh), _p(mean), _p(std), stride, _p(stats),
                                              _p(count), E, S, T, Q, A, L.current_stream_ptr()), None, "op_chunk_error")
    return stats, count


def chunk_error_ref(chunks, actions, lengths, shift, mean, std, stride=1):
    """numpy statement of ``chunk_error`` (float64); needs no library.  -> (stats [E, Q, 3, A], count [E, Q] int32) as ndarrays."""
    import numpy as np
    c = np.asarray(chunks, dtype=np.float32).astype(np.float64)
    a = np.asarray(actions, dtype=np.float32).astype(np.float64)
    E, S, Q, A = c.shape
    T, stride = a.shape[1], int(stride)
    if a.shape[0] != E or a.shape[2] != A or T < 1 or stride < 1:
        raise ValueError(f"chunk_error_ref: chunks {c.shape}, actions {a.shape}, stride {stride}")
    ln = np.full(E, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)
    sh = np.zeros(E, dtype=np.int64) if shift is None else (np.asarray(shift, dtype=np.int64) > 0).astype(np.int64)
    sd, mu = np.asarray(std, dtype=np.float64).reshape(1, A), np.asarray(mean, dtype=np.float64).reshape(1, A)
    stats = np.zeros((E, Q, 3, A), dtype=np.float64)
    count = np.zeros((E, Q), dtype=np.int32)
    r = np.arange(S, dtype=np.int64) * stride
    for e in range(E):
        base = np.maximum(0, r - sh[e])
        for j in range(Q):
            ok = (r < ln[e]) & (base + j < ln[e])
            if ok.any():
                d = np.abs(c[e, ok, j] * sd + mu - a[e, base[ok] + j])
                stats[e, j] = np.stack([d.sum(axis=0), (d * d).sum(axis=0), d.max(axis=0)])
                count[e, j] = int(ok.sum())
    return stats, count


# ---- replay schedule sweep: G execution schedules read off one chunk table (csrc/replay_eval.hip; contract at actmi_schedule) -----
SCHEDULE_ENSEMBLE, SCHEDULE_LATEST = 0, 1
SCHEDULE_MODES = ("ensemble", "latest")


def schedule_dtype():
    """actmi_schedule as a numpy structured dtype (24 bytes)"""
    import numpy as np
    return np.dtype([("every", np.int32), ("horizon", np.int32), ("mode", np.int32), ("reserved", np.int32), ("k", np.float64)])


def check_schedules(schedules, Q):
    """The refusals of a schedule grid for chunks of Q slots, before anything is launched -> the grid as a contiguous
    ``schedule_dtype()`` array.  ValueError: an empty grid, every < 1, horizon outside [1, Q], horizon < every (such a schedule
    leaves steps without an action), an unknown mode, a non-finite k, |k| * Q > 700 (exp leaves the float64 range)."""
    import numpy as np
    S = np.ascontiguousarray(np.asarray(schedules, dtype=schedule_dtype()).reshape(-1))
    Q = int(Q)
    if len(S) == 0:
        raise ValueError("schedules: the grid is empty")
    for g, s in enumerate(S):
        f, h, mode, k = int(s["every"]), int(s["horizon"]), int(s["mode"]), float(s["k"])
        if f < 1:
            raise ValueError(f"schedule {g}: every {f} must be at least 1")
        if not 1 <= h <= Q:
            raise ValueError(f"schedule {g}: horizon {h} must be in 1..{Q} (the slots of a chunk)")
        if h < f:
            raise ValueError(f"schedule {g}: horizon {h} < every {f} leaves steps without an action")
        if mode not in (SCHEDULE_ENSEMBLE, SCHEDULE_LATEST):
            raise ValueError(f"schedule {g}: mode {mode} is neither ensemble (0) nor latest (1)")
        if not np.isfinite(k) or abs(k) * Q > 700.0:
            raise ValueError(f"schedule {g}: k {k} must be finite with |k| * Q <= 700 (exp(-k * i) stays in the float64 range)")
    return S


def make_schedules(Q, every=(1,), horizon=None, k=(0.01,), latest=True):
    """The product grid every x horizon x k of ensemble schedules for chunks of Q slots, in that nesting order and without
    repeats, then (``latest``) one latest-chunk schedule per (every, horizon) pair.  Pairs with horizon < every are left out of
    the product (they leave steps without an action); every value is checked on its own (``check_schedules``), and a grid in
    which no pair remains is refused.  horizon None: Q.  -> a ``schedule_dtype()`` array [G]."""
    import numpy as np
    Q = int(Q)
    every = [int(f) for f in np.atleast_1d(every)]
    horizon = [Q] if horizon is None else [int(h) for h in np.atleast_1d(horizon)]
    ks = [float(v) for v in np.atleast_1d(k)]
    if not (every and horizon and ks):
        raise ValueError("make_schedules: every, horizon and k each need a value")
    for h in horizon:                                     # (a horizon below 1 would drop out of the pairs unnoticed)
        if not 1 <= h <= Q:
            raise ValueError(f"make_schedules: horizon {h} must be in 1..{Q} (the slots of a chunk)")
    pairs = list(dict.fromkeys((f, h) for f in every for h in horizon if h >= f))
    if not pairs:
        raise ValueError(f"make_schedules: every {every} x horizon {horizon} holds no pair with horizon >= every")
    grid = list(dict.fromkeys((f, h, SCHEDULE_ENSEMBLE, 0, kk) for f, h in pairs for kk in ks))
    if latest:
        grid += [(f, h, SCHEDULE_LATEST, 0, 0.0) for f, h in pairs]
    return check_schedules(grid, Q)


def schedules_as_dicts(schedules):
    """-> [{"every", "horizon", "mode": "ensemble" | "latest", "k"}] (what the replay's result and its JSON hold)"""
    return [{"every": int(s["every"]), "horizon": int(s["horizon"]), "mode": SCHEDULE_MODES[int(s["mode"])], "k": float(s["k"])}
            for s in schedules]


def device_schedules(schedules, Q, device):
    """``check_schedules`` and one copy to the device -> uint8 cuda tensor [G, 24], what ``ensemble_sweep`` takes without
    checking or copying again (a replay uploads its grid once for all episodes)"""
    S = check_schedules(schedules, Q)
    return torch.from_numpy(S.view("u1").reshape(len(S), schedule_dtype().itemsize).copy()).to(device)


def ensemble_sweep(chunks, schedules, length=None, want_empty=False):
    """G execution schedules read off one episode's chunk table in one launch (actmi_op_ensemble_sweep).  chunks [T, Q, A] f32
    cuda: row r is the chunk predicted from frame r; schedules: a ``schedule_dtype()`` array (checked and copied here) or the
    tensor of ``device_schedules``; length: the valid steps (None: all T) -> raw [G, T, A] f64, and with ``want_empty`` the
    int32 [G] count of the steps t < length of an ensemble schedule that found no populated live row (they are zeros).  An
    ensemble schedule (every, horizon, k) gives the bits of ``episode_ensemble`` with that k on the table whose dead entries
    (r % every != 0 or slot >= horizon) are zeroed; rows t >= length are zeros."""
    chunks = _device_table("chunks", chunks, torch.float32, "T, Q, A")
    T, Q, A = (int(v) for v in chunks.shape)
    dev = chunks.device
    if A < 1 or A > 64 or Q < 1 or Q > 7680:
        raise ValueError(f"ensemble_sweep: action_dim {A} must be in 1..64 and num_queries {Q} in 1..7680 (as episode_ensemble)")
    if not torch.is_tensor(schedules):
        schedules = device_schedules(schedules, Q, dev)
    if (schedules.dtype != torch.uint8 or schedules.dim() != 2 or int(schedules.shape[1]) != schedule_dtype().itemsize
            or schedules.device != dev or not schedules.is_contiguous()):
        raise ValueError("ensemble_sweep: schedules must be a schedule_dtype() array or the tensor of device_schedules on the chunks' device")
    G = int(schedules.shape[0])
    if G < 1 or G > 65535:
        raise ValueError(f"ensemble_sweep: {G} schedules, one launch holds 1..65535")
    n = T if length is None else int(length)
    raw = torch.empty((G, T, A), dtype=torch.float64, device=dev)
    empty = torch.empty((G,), dtype=torch.int32, device=dev) if want_empty else None
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_ensemble_sweep(_p(chunks), n, _p(schedules), _p(raw), _p(empty), G, T, Q, A,
                                                 L.current_stream_ptr()), None, "op_ensemble_sweep")
    return (raw, empty) if want_empty else raw


def ensemble_sweep_ref(chunks, schedules, length=None, want_empty=False):
    """numpy statement of ``ensemble_sweep``; needs no library.  chunks: ndarray or CPU tensor [T, Q, A]; schedules as
    ``check_schedules`` takes them -> raw [G, T, A] float64 (and empty [G] int32).  The live rows of a step are selected
    directly: r in (t - horizon, t], r % every == 0, oldest first."""
    import numpy as np
    c = np.asarray(chunks, dtype=np.float32)
    T, Q, A = c.shape
    S = check_schedules(schedules, Q)
    n = T if length is None else int(np.clip(int(length), 0, T))
    raw = np.zeros((len(S), T, A), dtype=np.float64)
    empty = np.zeros(len(S), dtype=np.int32)
    for g, s in enumerate(S):
        f, h, k = int(s["every"]), int(s["horizon"]), float(s["k"])
        for t in range(n):
            if int(s["mode"]) == SCHEDULE_LATEST:
                r = (t // f) * f
                raw[g, t] = c[r, t - r].astype(np.float64)
                continue
            lo = max(0, t - h + 1)
            r = np.arange(-(-lo // f) * f, t + 1, f)              # the live frames: multiples of f in [lo, t], oldest first
            rows = c[r, t - r]                                     # [n, A]
            rows = rows[np.all(rows != 0, axis=1)]
            if len(rows):
                w = np.exp(-k * np.arange(len(rows)))
                raw[g, t] = (rows.astype(np.float64) * (w / w.sum())[:, None]).sum(axis=0)
            else:
                empty[g] += 1
    return (raw, empty) if want_empty else raw


def sweep_error(raw, target, length, mean, std, want_pred=True):
    """Un-normalise G trajectories and compare each with the ONE recording on the device (actmi_op_sweep_error).  raw [G, T, A]
    f64 cuda, target [T, A] f32 (file units, already aligned; read by every g, never expanded), length or None (= T), mean / std
    [A] -> (pred [G, T, A] f64 = raw * std + mean or None, stats [G, 4, A] f64: rows 0-2 = sum |d|, sum d^2, max |d| over
    t < length, the bits of ``action_error`` on raw[g]; row 3 = sum over 1 <= t < length of |pred[t] - pred[t-1]|, the
    roughness of the executed trajectory)."""
    raw = _device_table("raw", raw, torch.float64, "G, T, A")
    G, T, A = (int(v) for v in raw.shape)
    dev = raw.device
    if G < 1 or G > 65535 or A < 1:
        raise ValueError(f"sweep_error: {G} schedules (one launch holds 1..65535), action_dim {A}")
    target = torch.as_tensor(target).to(device=dev, dtype=torch.float32).contiguous()
    if tuple(target.shape) != (T, A):
        raise ValueError(f"target has shape {tuple(target.shape)}, expected {(T, A)}")
    mean, std = _stats_f64("sweep_error", mean, std, A, dev)
    n = T if length is None else int(length)
    pred = torch.empty((G, T, A), dtype=torch.float64, device=dev) if want_pred else None
    stats = torch.empty((G, 4, A), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_sweep_error(_p(raw), _p(target), n, _p(mean), _p(std), _p(stats), _p(pred), G, T, A,
                                              L.current_stream_ptr()), None, "op_sweep_error")
    return pred, stats


def sweep_error_ref(raw, target, length, mean, std, want_pred=True):
    """numpy statement of ``sweep_error`` (float64); needs no library.  -> (pred, stats [G, 4, A]) as ndarrays."""
    import numpy as np
    raw = np.asarray(raw, dtype=np.float64)
    G, T, A = raw.shape
    pred = raw * np.asarray(std, dtype=np.float64).reshape(1, 1, A) + np.asarray(mean, dtype=np.float64).reshape(1, 1, A)
    d = np.abs(pred - np.asarray(target, dtype=np.float32).astype(np.float64).reshape(1, T, A))
    n = T if length is None else int(np.clip(int(length), 0, T))
    stats = np.zeros((G, 4, A), dtype=np.float64)
    for g in range(G):
        dg = d[g, :n]
        if len(dg):
            stats[g, :3] = np.stack([dg.sum(axis=0), (dg * dg).sum(axis=0), dg.max(axis=0)])
            stats[g, 3] = np.abs(np.diff(pred[g, :n], axis=0)).sum(axis=0)
    return (pred if want_pred else None), stats


# ---- device-resident episode store (csrc/episode_store.hip; contracts at actmi_op_gather_frames / actmi_op_gather_chunks) ------
def episode_rec_dtype():
    """actmi_episode_rec as a numpy structured dtype (16 bytes)"""
    import numpy as np
    return np.dtype([("row0", np.int64), ("T", np.int32), ("is_sim", np.int32)])


def _store_arena(op, arena, src_off=None):
    """the arena a store op gathers from -- a contiguous 1-D uint8 cuda tensor -- and, when given, the byte offsets into it"""
    if arena.dtype != torch.uint8 or arena.dim() != 1 or not arena.is_cuda or not arena.is_contiguous():
        raise ValueError(f"{op}: arena must be a contiguous 1-D uint8 cuda tensor, got {arena.dtype} {tuple(arena.shape)}")
    if src_off is not None and (src_off.dtype != torch.int64 or src_off.dim() != 1 or src_off.device != arena.device
                                or not src_off.is_contiguous()):
        raise ValueError(f"{op}: src_off must be a contiguous 1-D int64 tensor on the arena's device")


def gather_frames(arena, src_off, item_bytes, out=None, aligned=0):
    """actmi_op_gather_frames: arena 1-D uint8 cuda, src_off [n] int64 cuda (byte offsets into the arena) -> out [n, item_bytes]
    uint8 (or the caller's contiguous cuda tensor of n * item_bytes bytes, any dtype and shape).  aligned: 0 general, 1 the
    caller vouches that every offset is a multiple of 16 (item_bytes, arena and out must be), 2 the same with non-temporal loads."""
    _store_arena("gather_frames", arena, src_off)
    n, item_bytes = int(src_off.numel()), int(item_bytes)
    if out is None:
        out = torch.empty((n, item_bytes), dtype=torch.uint8, device=arena.device)
    elif out.device != arena.device or not out.is_contiguous() or out.numel() * out.element_size() != n * item_bytes:
        raise ValueError(f"gather_frames: out must be contiguous on {arena.device} and hold {n} x {item_bytes} bytes")
    with torch.cuda.device(arena.device):
        L.check(L.load().actmi_op_gather_frames(_p(arena), int(arena.numel()), _p(src_off), _p(out), n, item_bytes, int(aligned),
                                                L.current_stream_ptr()), None, "op_gather_frames")
    return out


def gather_frames_ref(arena, src_off, item_bytes):
    """numpy statement of ``gather_frames``; needs no library.  arena: 1-D uint8 ndarray (or CPU tensor), src_off [n] -> [n, item_bytes]
    uint8; an item whose range leaves the arena is zeros."""
    import numpy as np
    a = np.asarray(arena).reshape(-1).view(np.uint8)
    off = np.asarray(src_off, dtype=np.int64).reshape(-1)
    n = int(item_bytes)
    out = np.zeros((len(off), n), dtype=np.uint8)
    for i, o in enumerate(off):
        if 0 <= o and o + n <= a.size:
            out[i] = a[o:o + n]
    return out


def gather_frames_mirror(arena, src_off, flip, H, W, px_bytes, out=None, aligned=0):
    """actmi_op_gather_frames_mirror: ``gather_frames`` for items that are frames of H rows of W pixels of px_bytes bytes (3: u8
    BGR, 2: raw uint16 depth), item i mirrored along W where flip[i] != 0 and copied where it is 0.  arena 1-D uint8 cuda, src_off
    [n] int64 and flip [n] uint8 on its device -> out [n, H, W, px_bytes] uint8 (or the caller's contiguous cuda tensor of that
    many bytes, any dtype and shape).  aligned: as for ``gather_frames``; 1 and 2 also state that W is a multiple of 16 (px 3) or
    8 (px 2)."""
    _store_arena("gather_frames_mirror", arena, src_off)
    n, H, W, px = int(src_off.numel()), int(H), int(W), int(px_bytes)
    if flip.dtype != torch.uint8 or flip.dim() != 1 or flip.device != arena.device or not flip.is_contiguous() or flip.numel() != n:
        raise ValueError(f"gather_frames_mirror: flip must be a contiguous 1-D uint8 tensor of {n} flags on the arena's device")
    if out is None:
        out = torch.empty((n, H, W, px), dtype=torch.uint8, device=arena.device)
    elif out.device != arena.device or not out.is_contiguous() or out.numel() * out.element_size() != n * H * W * px:
        raise ValueError(f"gather_frames_mirror: out must be contiguous on {arena.device} and hold {n} x {H} x {W} x {px} bytes")
    d = L.GatherMirrorDesc()
    d.arena, d.arena_bytes, d.src_off, d.flip, d.out = arena.data_ptr(), int(arena.numel()), src_off.data_ptr(), flip.data_ptr(), out.data_ptr()
    d.n_items, d.H, d.W, d.px_bytes, d.aligned = n, H, W, px, int(aligned)
    with torch.cuda.device(arena.device):
        L.check(L.load().actmi_op_gather_frames_mirror(C.byref(d), L.current_stream_ptr()), None, "op_gather_frames_mirror")
    return out


def gather_frames_mirror_ref(arena, src_off, flip, H, W, px_bytes):
    """numpy statement of ``gather_frames_mirror``; needs no library.  -> [n, H, W, px_bytes] uint8: item i is the frame at
    arena[src_off[i]:], its pixels in reverse order along W where flip[i] != 0; an item whose range leaves the arena is zeros."""
    import numpy as np
    H, W, px = int(H), int(W), int(px_bytes)
    out = gather_frames_ref(arena, src_off, H * W * px).reshape(-1, H, W, px)
    fl = np.asarray(flip).reshape(-1) != 0
    if len(fl) != len(out):
        raise ValueError(f"gather_frames_mirror_ref: {len(fl)} flags for {len(out)} items")
    out[fl] = out[fl][:, :, ::-1]
    return out


def cloud_item_dtype():
    """actmi_cloud_item as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("xyz_off", np.int64), ("rgb_off", np.int64), ("rows", np.int32), ("n", np.int32), ("flags", np.int32),
                     ("pad", np.int32)])


def gather_clouds(arena, items, P, rgb_fmt, mirror=None, out=None, aligned=0):
    """actmi_op_gather_clouds: arena 1-D uint8 cuda; items: a contiguous cuda tensor (uint8 or int64) on its device holding [B]
    records (cloud_item_dtype) -> (xyz [B, P, 3] f32, rgb [B, P, 3] f32, n [B] int32), or the caller's ``out`` triple.  rgb_fmt: 0
    the arena holds uint8 colours, 1 f32.  mirror: (axis, c2) for the items whose flags carry bit 0 (c2 is taken as float32), None
    when no item does.  aligned: 0 general; 1 the outputs are 16-byte aligned and P % 4 == 0 (checked); 2 the same with
    non-temporal loads."""
    _store_arena("gather_clouds", arena)
    nb = items.numel() * items.element_size()
    if items.dtype not in (torch.uint8, torch.int64) or items.device != arena.device or not items.is_contiguous() or nb % 32:
        raise ValueError("gather_clouds: items must be a contiguous uint8 or int64 tensor of whole 32-byte records on the arena's device")
    B, P = nb // 32, int(P)
    dev = arena.device
    if out is None:
        out = (torch.empty((B, P, 3), dtype=torch.float32, device=dev), torch.empty((B, P, 3), dtype=torch.float32, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev))
    xyz, rgb, n = out
    for name, t, dt, numel in (("xyz", xyz, torch.float32, B * P * 3), ("rgb", rgb, torch.float32, B * P * 3), ("n", n, torch.int32, B)):
        if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() != numel:
            raise ValueError(f"gather_clouds: out {name} must be a contiguous {dt} tensor of {numel} values on {dev}")
    axis, c2 = (0, 0.0) if mirror is None else (int(mirror[0]), float(mirror[1]))
    d = L.GatherCloudsDesc()
    d.arena, d.arena_bytes, d.items = arena.data_ptr(), int(arena.numel()), items.data_ptr()
    d.out_xyz, d.out_rgb, d.out_n = xyz.data_ptr(), rgb.data_ptr(), n.data_ptr()
    d.B, d.P, d.rgb_fmt, d.mirror_axis, d.mirror_c2, d.aligned = B, P, int(rgb_fmt), axis, c2, int(aligned)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_gather_clouds(C.byref(d), L.current_stream_ptr()), None, "op_gather_clouds")
    return xyz, rgb, n


def gather_clouds_ref(arena, items, P, rgb_fmt, mirror=None):
    """numpy statement of ``gather_clouds``; needs no library.  arena: 1-D uint8 ndarray, items: [B] records (cloud_item_dtype)
    -> (xyz [B, P, 3] f32, rgb [B, P, 3] f32, n [B] int32).  With r = clamp(rows, 0, P): rows [0, r) are the stored ones (uint8
    colours converted), the rest zero; flags & 1: xyz[..., axis] = float32(c2) - xyz[..., axis] over the copied rows; an item either
    of whose source ranges leaves the arena is zeros with n = 0."""
    import numpy as np
    a = np.asarray(arena).reshape(-1).view(np.uint8)
    it = np.asarray(items).reshape(-1)
    P, f32c = int(P), bool(rgb_fmt)
    xyz, rgb = np.zeros((len(it), P, 3), dtype=np.float32), np.zeros((len(it), P, 3), dtype=np.float32)
    n = np.zeros(len(it), dtype=np.int32)
    for b, rec in enumerate(it):
        xo, co, r = int(rec["xyz_off"]), int(rec["rgb_off"]), min(max(int(rec["rows"]), 0), P)
        xb, cb = r * 12, r * (12 if f32c else 3)
        if xo < 0 or co < 0 or xo + xb > a.size or co + cb > a.size:
            continue
        n[b] = rec["n"]
        x = np.frombuffer(a[xo:xo + xb].tobytes(), dtype=np.float32).reshape(r, 3).copy()
        if int(rec["flags"]) & 1:
            if mirror is None:
                raise ValueError("gather_clouds_ref: an item is flagged and no mirror rule is given")
            x[:, int(mirror[0])] = np.float32(mirror[1]) - x[:, int(mirror[0])]
        xyz[b, :r] = x
        c = a[co:co + cb]
        rgb[b, :r] = (np.frombuffer(c.tobytes(), dtype=np.float32) if f32c else c.astype(np.float32)).reshape(r, 3)
    return xyz, rgb, n


def gather_chunks(actions, qpos, episodes, samples, action_mean, action_std, qpos_mean, qpos_std, Q):
    """actmi_op_gather_chunks.  actions [R, A] / qpos [R, S] f32 cuda (all episodes' rows back to back), episodes: uint8 cuda
    tensor holding [E] records (episode_rec_dtype), samples [B, 2] int32 cuda (episode, t), the four stat vectors f32 cuda ->
    (qpos [B, S] f32, action [B, Q, A] f32, is_pad [B, Q] bool)."""
    dev = actions.device
    for name, t, dt in (("actions", actions, torch.float32), ("qpos", qpos, torch.float32), ("episodes", episodes, torch.uint8),
                        ("samples", samples, torch.int32), ("action_mean", action_mean, torch.float32),
                        ("action_std", action_std, torch.float32), ("qpos_mean", qpos_mean, torch.float32),
                        ("qpos_std", qpos_std, torch.float32)):
        if t.dtype != dt or not t.is_cuda or t.device != dev or not t.is_contiguous():
            raise ValueError(f"gather_chunks: {name} must be a contiguous {dt} tensor on {dev}, got {t.dtype} on {t.device}")
    if actions.dim() != 2 or qpos.dim() != 2 or qpos.shape[0] != actions.shape[0]:
        raise ValueError(f"gather_chunks: actions {tuple(actions.shape)} and qpos {tuple(qpos.shape)} must be [R, A] and [R, S]")
    R, A, S = int(actions.shape[0]), int(actions.shape[1]), int(qpos.shape[1])
    if samples.dim() != 2 or samples.shape[1] != 2 or episodes.numel() % 16 or episodes.numel() == 0:
        raise ValueError("gather_chunks: samples must be [B, 2] and episodes a whole number of 16-byte records")
    if action_mean.numel() != A or action_std.numel() != A or qpos_mean.numel() != S or qpos_std.numel() != S:
        raise ValueError(f"gather_chunks: the stat vectors must hold {A} (action) and {S} (qpos) values")
    B, Q = int(samples.shape[0]), int(Q)
    qpos_out = torch.empty((B, S), dtype=torch.float32, device=dev)
    action_out = torch.empty((B, Q, A), dtype=torch.float32, device=dev)
    is_pad = torch.empty((B, Q), dtype=torch.bool, device=dev)
    d = L.GatherChunksDesc()
    d.actions, d.qpos, d.episodes, d.samples = actions.data_ptr(), qpos.data_ptr(), episodes.data_ptr(), samples.data_ptr()
    d.action_mean, d.action_std, d.qpos_mean, d.qpos_std = (t.data_ptr() for t in (action_mean, action_std, qpos_mean, qpos_std))
    d.qpos_out, d.action_out, d.is_pad = qpos_out.data_ptr(), action_out.data_ptr(), is_pad.data_ptr()
    d.n_rows, d.n_episodes, d.B, d.A, d.S, d.Q = R, episodes.numel() // 16, B, A, S, Q
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_gather_chunks(C.byref(d), L.current_stream_ptr()), None, "op_gather_chunks")
    return qpos_out, action_out, is_pad


def gather_chunks_ref(actions, qpos, episodes, samples, action_mean, action_std, qpos_mean, qpos_std, Q):
    """numpy statement of ``gather_chunks`` (EpisodicDataset.__getitem__ without the frames, for B samples); needs no library.
    episodes: [E] records (episode_rec_dtype) or rows (row0, T, is_sim); samples [B, 2] -> (qpos [B, S] f32, action [B, Q, A] f32,
    is_pad [B, Q] bool).  float32 subtract, then float32 divide: numpy's are the IEEE operations torch's are."""
    import numpy as np
    a, q = np.asarray(actions, dtype=np.float32), np.asarray(qpos, dtype=np.float32)
    ep = np.asarray(episodes)
    if ep.dtype.names:
        ep = np.stack([ep["row0"].astype(np.int64), ep["T"].astype(np.int64), ep["is_sim"].astype(np.int64)], axis=1)
    smp = np.asarray(samples, dtype=np.int64).reshape(-1, 2)
    am, asd, qm, qsd = (np.asarray(v, dtype=np.float32).reshape(-1) for v in (action_mean, action_std, qpos_mean, qpos_std))
    B, Q, A = len(smp), int(Q), a.shape[1]
    qpos_out = np.empty((B, q.shape[1]), dtype=np.float32)
    action_out = np.empty((B, Q, A), dtype=np.float32)
    is_pad = np.zeros((B, Q), dtype=bool)
    for b, (e, t) in enumerate(smp):
        row0, T, is_sim = (int(v) for v in ep[e])
        s = t if is_sim else max(0, t - 1)
        n = min(T - s, Q)
        rows = np.zeros((Q, A), dtype=np.float32)
        rows[:n] = a[row0 + s:row0 + s + n]
        qpos_out[b] = (q[row0 + t] - qm) / qsd
        action_out[b] = (rows - am) / asd
        is_pad[b, n:] = True
    return qpos_out, action_out, is_pad


# ---- nearest-neighbour action retrieval (csrc/knn.hip; contracts at actmi_op_knn_topk / _predict / _ksweep) ------------------
KNN_MAX_K = 512


def check_knn_args(K, state_weight, support_rows=None):
    """The refusals every kNN entry shares, raised before anything is launched: K in [1, 512] and at most the support rows (when
    given), state_weight finite and not negative.  -> (K, state_weight)"""
    import math
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= KNN_MAX_K:
        raise ValueError(f"kNN: K must be an integer in [1, {KNN_MAX_K}], got {K!r}")
    K = int(K)
    if support_rows is not None and K > int(support_rows):
        raise ValueError(f"kNN: K = {K} exceeds the {int(support_rows)} support rows")
    w = float(state_weight)
    if not math.isfinite(w) or w < 0:
        raise ValueError(f"kNN: state_weight must be finite and not negative, got {state_weight!r}")
    return K, w


def _knn_sqnorm_ref(a, b):
    """[Nq, Ns] fp32 squared distances in the ABI's summation order: partial sum j takes the dimensions d = j (mod 4) ascending,
    one subtract, one multiply and one add per term, and the four combine as (p0 + p1) + (p2 + p3)."""
    import numpy as np
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    p = np.zeros((4, a.shape[0], b.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for d in range(a.shape[1]):
            diff = a[:, None, d] - b[None, :, d]
            p[d & 3] = p[d & 3] + diff * diff
        return (p[0] + p[1]) + (p[2] + p[3])


def knn_topk_ref(qv, qs, sv, ss, K, state_weight=1.0, sep=None, exclude=None):
    """numpy statement of ``knn_topk``: fp32 distances in the stated order, the K eligible rows of smallest (distance bits, index).
    -> (idx [Nq, K] int32, dist [Nq, K] f32, n [Nq] int32); needs no library."""
    import numpy as np
    qv, sv = np.asarray(qv, dtype=np.float32), np.asarray(sv, dtype=np.float32)
    Nq, Ns = qv.shape[0], sv.shape[0]
    K = int(K)
    with np.errstate(all="ignore"):
        dv = np.sqrt(_knn_sqnorm_ref(qv, sv))
        if qs is not None and np.asarray(qs).shape[1] > 0:
            dsn = np.sqrt(_knn_sqnorm_ref(qs, ss))
        else:
            dsn = np.zeros((Nq, Ns), dtype=np.float32)
        d = (dv + np.float32(state_weight) * dsn).astype(np.float32)
    ok = np.isfinite(d)
    if exclude is not None:
        ex = np.asarray(exclude, dtype=np.int64).reshape(Nq, 1)
        ok &= ~((ex >= 0) & (np.asarray(sep, dtype=np.int64).reshape(1, Ns) == ex))
    idx = np.full((Nq, K), -1, dtype=np.int32)
    dist = np.full((Nq, K), np.inf, dtype=np.float32)
    n = np.zeros(Nq, dtype=np.int32)
    for q in range(Nq):
        rows = np.nonzero(ok[q])[0]
        key = (d[q, rows].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
        order = rows[np.argsort(key, kind="stable")][:K]
        n[q] = len(order)
        idx[q, :len(order)] = order
        dist[q, :len(order)] = d[q, order]
    return idx, dist, n


def knn_predict_ref(idx, dist, n, k, actions, off, left, Q, mean=None, std=None):
    """numpy statement of ``knn_predict`` (float64, neighbour order; needs no library) -> (chunk [Nq, Q, A] f32, empty)."""
    import numpy as np
    idx, n = np.asarray(idx, dtype=np.int64), np.asarray(n, dtype=np.int64)
    dist = np.asarray(dist, dtype=np.float32).astype(np.float64)
    actions = np.asarray(actions, dtype=np.float32).astype(np.float64)
    off, left = np.asarray(off, dtype=np.int64), np.asarray(left, dtype=np.int64)
    Nq, A, Q = idx.shape[0], actions.shape[1], int(Q)
    out = np.zeros((Nq, Q, A), dtype=np.float32)
    empty = 0
    j = np.arange(Q)
    for q in range(Nq):
        m = int(min(int(k), n[q]))
        if m <= 0:
            empty += 1
            continue
        e = np.exp(-(dist[q, :m] - dist[q, 0]))
        num, den = np.zeros((Q, A)), 0.0
        for i in range(m):
            s = idx[q, i]
            rows = off[s] + np.minimum(j, max(int(left[s]), 1) - 1)
            num = num + e[i] * actions[rows]
            den = den + e[i]
        v = num / den
        if mean is not None:
            v = (v - np.asarray(mean, dtype=np.float64).reshape(1, A)) / np.asarray(std, dtype=np.float64).reshape(1, A)
        out[q] = v.astype(np.float32)
    return out, empty


def knn_ksweep_ref(idx, dist, n, actions, off, target, mean=None, std=None, want_partial=False):
    """numpy statement of ``knn_ksweep``: sse [K] float64, sse[k - 1] = the squared error of slot 0 of ``knn_predict_ref`` at k
    against target [Nq, A], the queries added in order.  ``want_partial``: also the per-query terms [Nq, K]."""
    import numpy as np
    idx = np.asarray(idx)
    Nq, K = idx.shape
    target = np.asarray(target, dtype=np.float32).astype(np.float64)
    left = np.ones(len(np.asarray(off)), dtype=np.int64)
    partial = np.zeros((Nq, K), dtype=np.float64)
    for k in range(1, K + 1):
        pred, _ = knn_predict_ref(idx, dist, n, k, actions, off, left, 1, mean, std)
        d = pred[:, 0].astype(np.float64) - target
        dd = d * d
        s = np.zeros(Nq)
        for a in range(dd.shape[1]):
            s = s + dd[:, a]
        partial[:, k - 1] = s
    sse = np.zeros(K)
    for q in range(Nq):
        sse = sse + partial[q]
    return (sse, partial) if want_partial else sse


def pooled_features_ref(layer4, B, C, fh, fw):
    """numpy statement of the bound trunk embedding (actmi_bind_features_out): layer4 camera-major [C, B, fh, fw, F] (any shape of
    that many values) -> [B, C * F] f32: an fp32 sum over the fh * fw positions in row-major order, one add at a time, then one
    fp32 divide by float(fh * fw)."""
    import numpy as np
    m = np.asarray(layer4, dtype=np.float32).reshape(C, B, fh * fw, -1)
    s = np.zeros((C, B, m.shape[3]), dtype=np.float32)
    for p in range(fh * fw):
        s = s + m[:, :, p]
    s = s / np.float32(fh * fw)
    return np.ascontiguousarray(s.transpose(1, 0, 2).reshape(B, -1))


def _knn_f32(name, t, dev, cols=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or (dev is not None and t.device != dev):
        raise ValueError(f"knn: {name} must be a 2-D float32 cuda tensor on one device")
    if cols is not None and t.shape[1] != cols:
        raise ValueError(f"knn: {name} has {t.shape[1]} columns, expected {cols}")
    return t.contiguous()


def knn_topk(qv, qs, sv, ss, K, state_weight=1.0, sep=None, exclude=None, ws=None):
    """actmi_op_knn_topk.  qv [Nq, Dv], qs [Nq, S] or None, sv [Ns, Dv], ss [Ns, S] or None (f32 cuda), sep [Ns] / exclude [Nq]
    int32 cuda or None -> (idx [Nq, K] int32, dist [Nq, K] f32, n [Nq] int32).  ``ws``: a uint8 cuda tensor of at least
    ``knn_workspace_bytes(Nq, Ns)`` bytes to reuse between calls."""
    K, w = check_knn_args(K, state_weight)
    qv = _knn_f32("qv", qv, None)
    dev = qv.device
    sv = _knn_f32("sv", sv, dev, qv.shape[1])
    Nq, Ns, Dv = int(qv.shape[0]), int(sv.shape[0]), int(qv.shape[1])
    if Nq < 1 or Ns < 1 or Dv < 1:
        raise ValueError(f"knn_topk: Nq = {Nq}, Ns = {Ns}, Dv = {Dv} must each be at least 1")
    S = 0
    if qs is not None and qs.shape[1] > 0:
        qs = _knn_f32("qs", qs, dev)
        S = int(qs.shape[1])
        ss = _knn_f32("ss", ss, dev, S)
        if qs.shape[0] != Nq or ss.shape[0] != Ns:
            raise ValueError("knn_topk: the state rows do not match the feature rows")
    else:
        qs = ss = None
    if exclude is not None:
        if sep is None:
            raise ValueError("knn_topk: exclude needs the support rows' episode ids (sep)")
        for name, t, rows in (("sep", sep, Ns), ("exclude", exclude, Nq)):
            if t.dtype != torch.int32 or t.device != dev or t.numel() != rows or not t.is_contiguous():
                raise ValueError(f"knn_topk: {name} must be a contiguous int32 tensor of {rows} values on {dev}")
    else:
        sep = None
    lib = L.load()
    need = int(lib.actmi_op_knn_workspace_bytes(Nq, Ns))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif ws.dtype != torch.uint8 or ws.device != dev or ws.numel() < need:
        raise ValueError(f"knn_topk: the workspace must be a uint8 tensor of at least {need} bytes on {dev}")
    idx = torch.empty((Nq, K), dtype=torch.int32, device=dev)
    dist = torch.empty((Nq, K), dtype=torch.float32, device=dev)
    n = torch.empty(Nq, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.actmi_op_knn_topk(_p(qv), _p(qs), _p(sv), _p(ss), _p(sep), _p(exclude), w, K, Nq, Ns, Dv, S, _p(idx), _p(dist),
                                      _p(n), _p(ws), ws.numel(), L.current_stream_ptr()), None, "op_knn_topk")
    return idx, dist, n


def knn_workspace_bytes(Nq, Ns):
    return int(L.load().actmi_op_knn_workspace_bytes(int(Nq), int(Ns)))


def _knn_neighbours(idx, dist, n):
    dev = idx.device
    if idx.dtype != torch.int32 or dist.dtype != torch.float32 or n.dtype != torch.int32 or idx.dim() != 2 or dist.shape != idx.shape \
            or n.numel() != idx.shape[0] or not idx.is_cuda or dist.device != dev or n.device != dev:
        raise ValueError("knn: idx [Nq, K] int32, dist [Nq, K] float32 and n [Nq] int32 must be cuda tensors of one device")
    return idx.contiguous(), dist.contiguous(), n.contiguous()


def _knn_rows(actions, off, left, dev):
    if actions.dtype != torch.float32 or actions.dim() != 2 or actions.device != dev or not actions.is_contiguous():
        raise ValueError("knn: actions must be a contiguous float32 [R, A] tensor on the neighbours' device")
    if off.dtype != torch.int64 or off.device != dev or off.dim() != 1 or not off.is_contiguous():
        raise ValueError("knn: off must be a contiguous int64 [Ns] tensor on the neighbours' device")
    if left is not None and (left.dtype != torch.int32 or left.device != dev or left.shape != off.shape or not left.is_contiguous()):
        raise ValueError("knn: left must be a contiguous int32 [Ns] tensor on the neighbours' device")


def knn_predict(idx, dist, n, k, actions, off, left, Q, mean=None, std=None, empty=None):
    """actmi_op_knn_predict.  idx / dist / n from ``knn_topk``; actions [R, A] f32, off [Ns] int64, left [Ns] int32 (cuda); mean / std
    [A] or None -> (chunk [Nq, Q, A] f32, empty: an int32 cuda word counting the queries without a neighbour; pass one in to
    keep counting)."""
    idx, dist, n = _knn_neighbours(idx, dist, n)
    dev = idx.device
    Nq, K = (int(v) for v in idx.shape)
    if not 1 <= int(k) <= K <= KNN_MAX_K:
        raise ValueError(f"knn_predict: need 1 <= k <= K <= {KNN_MAX_K}, got k = {k}, K = {K}")
    if left is None:
        raise ValueError("knn_predict: left (the rows that remain in each support row's episode, int32 [Ns]) is required")
    _knn_rows(actions, off, left, dev)
    R, A, Q = int(actions.shape[0]), int(actions.shape[1]), int(Q)
    if Nq < 1 or R < 1 or Q < 1 or off.numel() < 1:
        raise ValueError("knn_predict: empty operand")
    mean, std = _stats_f64("knn", mean, std, A, dev, optional=True)
    if empty is None:
        empty = torch.zeros(1, dtype=torch.int32, device=dev)
    chunk = torch.empty((Nq, Q, A), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_knn_predict(_p(idx), _p(dist), _p(n), K, int(k), _p(actions), R, _p(off), _p(left), off.numel(), Q, A,
                                              _p(mean), _p(std), _p(chunk), _p(empty), Nq, L.current_stream_ptr()), None,
                "op_knn_predict")
    return chunk, empty


def knn_ksweep(idx, dist, n, actions, off, target, mean=None, std=None, want_partial=False):
    """actmi_op_knn_ksweep.  target [Nq, A] f32 cuda (in the units of the prediction: z-scored when mean / std are given) ->
    sse [K] float64 cuda (and the per-query terms [Nq, K] with ``want_partial``)."""
    idx, dist, n = _knn_neighbours(idx, dist, n)
    dev = idx.device
    Nq, K = (int(v) for v in idx.shape)
    _knn_rows(actions, off, None, dev)
    R, A = int(actions.shape[0]), int(actions.shape[1])
    if target.dtype != torch.float32 or target.device != dev or tuple(target.shape) != (Nq, A):
        raise ValueError(f"knn_ksweep: target must be a float32 [{Nq}, {A}] tensor on {dev}")
    target = target.contiguous()
    mean, std = _stats_f64("knn", mean, std, A, dev, optional=True)
    partial = torch.empty((Nq, K), dtype=torch.float64, device=dev)
    sse = torch.empty(K, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_knn_ksweep(_p(idx), _p(dist), _p(n), K, _p(actions), R, _p(off), off.numel(), A, _p(mean), _p(std),
                                             _p(target), _p(partial), _p(sse), Nq, L.current_stream_ptr()), None, "op_knn_ksweep")
    return (sse, partial) if want_partial else sse


# ---- baseline JPEG decode (csrc/jpeg_decode.hip, csrc/jpeg_core.h; the definition is at actmi_op_jpeg_decode in actmi.h) ---------
JPEG_MODES = {"gray": 0, "444": 1, "422": 2, "420": 3}
JPEG_FORMS = {"bgr": 0, "rgb": 1, "u16": 2}
JPEG_STATUS = {0: "ok", 1: "overrun", 2: "invalid code", 3: "coefficient index out of range", 4: "restart marker missing or out of sequence",
               5: "destination outside the buffer", 6: "table set outside the array", 7: "mark malformed or missed by its interval"}
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


class JpegUnsupported(ValueError):
    """what ``jpeg_parse`` refuses: not a JPEG, or a JPEG outside what actmi_op_jpeg_decode accepts"""


def jpeg_tables_dtype():
    """actmi_jpeg_tables as a numpy structured dtype (1960 bytes)"""
    import numpy as np
    huff = np.dtype([("maxcode", np.int32, 17), ("valoff", np.int32, 17), ("vals", np.uint8, 256)])
    return np.dtype([("q", np.uint16, (3, 64)), ("huff", huff, 4), ("dc_sel", np.uint8, 3), ("ac_sel", np.uint8, 3), ("reserved", np.uint8, 2)])


def jpeg_frame_dtype():
    """actmi_jpeg_frame as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("seg_off", np.int64), ("dst_off", np.int64), ("seg_len", np.int32), ("restart_interval", np.int32),
                     ("table_set", np.int32), ("reserved", np.int32)])


def jpeg_mark_dtype():
    """actmi_jpeg_mark as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("byte_off", np.int64), ("bit", np.int32), ("pred", np.int32, 3), ("togo", np.int32), ("rst", np.int32)])


def jpeg_out_shape(H, W, form):
    return (int(H), int(W)) if form == "u16" else (int(H), int(W), 3)


def jpeg_parse(buf):
    """The host parser of one JPEG file (1-D uint8 array or bytes; bytes after EOI are ignored) -> dict with ``H``, ``W``, ``mode``
    ("gray", "444", "422", "420"), ``restart_interval``, ``tables`` (one ``jpeg_tables_dtype`` record: quantisation tables in natural
    order per component, up to four Huffman tables and which of them each component uses), ``seg_off`` / ``seg_len`` (the entropy
    segment: from the byte after the SOS header up to the marker that ends it, or the end of `buf` when there is none).  Raises
    ``JpegUnsupported`` for everything actmi_op_jpeg_decode does not accept (see actmi.h)."""
    import numpy as np
    a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    n = a.size
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        raise JpegUnsupported("not a JPEG (no SOI marker)")
    qt, ht = {}, {}
    frame = adobe_transform = None
    ri = 0
    pos = 2
    while True:
        if pos + 4 > n:
            raise JpegUnsupported("the header ends before a scan begins")
        if a[pos] != 0xFF:
            raise JpegUnsupported(f"no marker at byte {pos}")
        m = int(a[pos + 1])
        if m == 0xFF:                                             # fill byte
            pos += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if m == 0xD9:
            raise JpegUnsupported("EOI before any scan")
        ln = (int(a[pos + 2]) << 8) | int(a[pos + 3])
        if ln < 2 or pos + 2 + ln > n:
            raise JpegUnsupported("a header segment is cut short")
        seg = a[pos + 4:pos + 2 + ln]
        if m == 0xC0:
            if frame is not None:
                raise JpegUnsupported("more than one frame header")
            if seg.size < 6 or seg[0] != 8:
                raise JpegUnsupported("samples are not 8-bit")
            H, W, nc = (int(seg[1]) << 8) | int(seg[2]), (int(seg[3]) << 8) | int(seg[4]), int(seg[5])
            if nc not in (1, 3):
                raise JpegUnsupported(f"{nc} components (1 or 3 are decoded)")
            if seg.size < 6 + 3 * nc or H < 1 or W < 1:
                raise JpegUnsupported("bad frame header")
            frame = (H, W, [(int(seg[6 + 3 * i]), int(seg[7 + 3 * i]) >> 4, int(seg[7 + 3 * i]) & 15, int(seg[8 + 3 * i])) for i in range(nc)])
        elif 0xC0 < m <= 0xCF and m not in (0xC4, 0xC8):
            if m == 0xCC:
                raise JpegUnsupported("arithmetic coding conditioning (DAC)")
            raise JpegUnsupported(f"SOF{m - 0xC0} (only baseline SOF0 is decoded)")
        elif m == 0xC4:
            p = 0
            while p < seg.size:
                if p + 17 > seg.size:
                    raise JpegUnsupported("a Huffman table is cut short")
                tc, th = int(seg[p]) >> 4, int(seg[p]) & 15
                counts = seg[p + 1:p + 17].astype(np.int64)
                tot = int(counts.sum())
                if tc > 1 or th > 3 or tot > 256 or p + 17 + tot > seg.size:
                    raise JpegUnsupported("bad Huffman table (class above 1, index above 3 or more than 256 codes)")
                vals = seg[p + 17:p + 17 + tot]
                if tc == 0 and tot and int(vals.max()) > 15:
                    raise JpegUnsupported("a DC Huffman table holds a category above 15")
                ht[(tc, th)] = (counts, vals.copy())
                p += 17 + tot
        elif m == 0xDB:
            p = 0
            while p < seg.size:
                pq, tq = int(seg[p]) >> 4, int(seg[p]) & 15
                if pq != 0:
                    raise JpegUnsupported("16-bit quantisation table")
                if tq > 3 or p + 65 > seg.size:
                    raise JpegUnsupported("bad quantisation table")
                qt[tq] = seg[p + 1:p + 65].copy()
                p += 65
        elif m == 0xDD:
            if seg.size < 2:
                raise JpegUnsupported("bad DRI segment")
            ri = (int(seg[0]) << 8) | int(seg[1])
        elif m == 0xEE:
            if seg.size >= 12 and bytes(seg[:5]) == b"Adobe":
                adobe_transform = int(seg[11])
        elif m == 0xDA:
            break
        pos += 2 + ln
    if frame is None:
        raise JpegUnsupported("a scan before the frame header")
    H, W, comps = frame
    if adobe_transform == 0 and len(comps) == 3:
        raise JpegUnsupported("Adobe APP14 with transform 0 (the components are not YCbCr)")
    ns = int(seg[0]) if seg.size else 0
    if ns != len(comps) or seg.size < 1 + 2 * ns + 3:
        raise JpegUnsupported("the scan does not hold every component (more than one scan)")
    if int(seg[1 + 2 * ns]) != 0 or int(seg[2 + 2 * ns]) != 63 or int(seg[3 + 2 * ns]) != 0:
        raise JpegUnsupported("spectral selection or successive approximation in a baseline scan")
    if len(comps) == 1:
        mode = "gray"
    else:
        samp = tuple((h, v) for _cid, h, v, _tq in comps)
        mode = {((1, 1), (1, 1), (1, 1)): "444", ((2, 1), (1, 1), (1, 1)): "422", ((2, 2), (1, 1), (1, 1)): "420"}.get(samp)
        if mode is None:
            raise JpegUnsupported(f"sampling factors {samp}")
    tb = np.zeros((), dtype=jpeg_tables_dtype())
    slots = {}
    zz = np.asarray(_JPEG_ZIGZAG)
    for i, (cid, _h, _v, tq) in enumerate(comps):
        if int(seg[1 + 2 * i]) != cid:
            raise JpegUnsupported("the scan's components are not in the frame's order")
        td, ta = int(seg[2 + 2 * i]) >> 4, int(seg[2 + 2 * i]) & 15
        if tq > 3 or td > 3 or ta > 3:
            raise JpegUnsupported("a table index above 3")
        if tq not in qt or (0, td) not in ht or (1, ta) not in ht:
            raise JpegUnsupported("a table the scan names is missing")
        q = np.zeros(64, dtype=np.uint16)
        q[zz] = qt[tq]
        tb["q"][i] = q
        for key, sel in (((0, td), "dc_sel"), ((1, ta), "ac_sel")):
            if key not in slots:
                if len(slots) == 4:
                    raise JpegUnsupported("more than four Huffman tables in one scan")
                slots[key] = len(slots)
                counts, vals = ht[key]
                h = tb["huff"][slots[key]]
                h["maxcode"][:] = -1
                code = k = 0
                for l in range(1, 17):
                    c = int(counts[l - 1])
                    if c:
                        h["valoff"][l] = k - code
                        code += c
                        k += c
                        h["maxcode"][l] = code - 1
                        if code > (1 << l):
                            raise JpegUnsupported("a Huffman table with more codes than its lengths allow")
                    code <<= 1
                h["vals"][:len(vals)] = vals
            tb[sel][i] = slots[key]
    seg_off = pos + 2 + ln
    tail = a[seg_off:]
    # the segment ends at the first 0xFF that is followed by neither 0x00 nor RSTn
    ff = np.flatnonzero(tail[:-1] == 0xFF) if tail.size > 1 else np.zeros(0, dtype=np.int64)
    nxt = tail[ff + 1] if ff.size else ff
    stop = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7))] if ff.size else ff
    if stop.size:
        seg_len = int(stop[0])
        if int(tail[seg_len + 1]) not in (0xD9, 0xFF):
            raise JpegUnsupported(f"marker 0x{int(tail[seg_len + 1]):02x} after the scan (more than one scan, or DNL)")
    else:
        seg_len = int(tail.size)
    return {"H": H, "W": W, "mode": mode, "restart_interval": ri, "tables": tb, "seg_off": int(seg_off), "seg_len": seg_len}


class _JpegRefBits:
    """the bit reader of ``jpeg_decode_ref``: the data bytes from `pos` up to the end of the data (a marker, 0xFF as the last byte,
    the end of the segment), then zero bits; ``over`` once one of those is consumed"""

    def __init__(self, data, end):
        self.d, self.end = data, end
        self.over = False
        self.load(0)

    def load(self, pos):
        import numpy as np
        d, end, out, after = self.d, self.end, bytearray(), []
        i = pos
        while i < end:
            c = d[i]
            if c != 0xFF:
                out.append(c)
                i += 1
            elif i + 1 < end and d[i + 1] == 0:
                out.append(0xFF)
                i += 2
            else:
                break
            after.append(i)
        self.start, self.after = pos, after
        self.bits = np.unpackbits(np.frombuffer(bytes(out), dtype=np.uint8)).tolist() + [0] * 32
        self.nbits, self.cur = 8 * len(out), 0

    def get(self, k):
        v = 0
        for b in self.bits[self.cur:self.cur + k]:
            v = (v << 1) | b
        self.cur += k
        if self.cur > self.nbits:
            self.over = True
            self.bits += [0] * 32
        return v

    def byte_pos(self):
        nb = (min(self.cur, self.nbits) + 7) // 8
        return self.after[nb - 1] if nb else self.start

    def mark_pos(self):
        """the position convention of actmi_jpeg_mark -> (byte_off, bit): data byte cur // 8 of this load begins where the one
        before it ends (``after``), or at ``start``; with every data bit consumed that is the offset of what follows"""
        cur = min(self.cur, self.nbits)
        k = cur // 8
        return (self.after[k - 1] if k else self.start), cur % 8


def jpeg_decode_ref(buf, form="bgr", with_status=False, info=None, _at_mcu=None):
    """numpy statement of ``jpeg_decode`` for one file (the definition in actmi.h, step by step; needs no library): -> the frame, u8
    [H, W, 3] (``form`` "bgr" or "rgb") or uint16 [H, W] ("u16").  ``with_status``: -> (frame, status) with the status the op gives
    (a frame whose status is not 0 holds unspecified pixels); without it a damaged stream raises ``ValueError``.  ``info``: what
    ``jpeg_parse`` said of `buf` before its entropy segment was changed (its ``seg_off`` / ``seg_len`` name bytes of `buf`)."""
    import numpy as np
    if form not in JPEG_FORMS:
        raise ValueError(f"jpeg_decode_ref: form must be one of {sorted(JPEG_FORMS)}")
    if info is None:
        info = jpeg_parse(buf)
    a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    H, W, mode, tb = info["H"], info["W"], info["mode"], info["tables"]
    nc = 1 if mode == "gray" else 3
    hmax, vmax = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[mode]
    hs, vs = [hmax, 1, 1][:nc], [vmax, 1, 1][:nc]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coef = [np.zeros((my * vs[c], mx * hs[c], 64), dtype=np.int64) for c in range(nc)]
    seg = bytes(a[info["seg_off"]:info["seg_off"] + info["seg_len"]])
    rd = _JpegRefBits(seg, len(seg))
    huff = []
    for t in range(4):
        h = tb["huff"][t]
        huff.append(([int(x) for x in h["maxcode"]], [int(x) for x in h["valoff"]], [int(x) for x in h["vals"]]))

    def sym(t):
        maxcode, valoff, vals = huff[t]
        code = 0
        for l in range(1, 17):
            code = (code << 1) | rd.get(1)
            if code <= maxcode[l]:
                return vals[(code + valoff[l]) & 255]
        return None

    def extend(t):
        if t == 0:
            return 0
        v = rd.get(t)
        return v - (1 << t) + 1 if v < (1 << (t - 1)) else v

    status, pred, ri, togo, rst = 0, [0] * nc, info["restart_interval"], info["restart_interval"], 0
    for m in range(mx * my):
        if status:
            break
        if _at_mcu is not None:                                     # jpeg_marks_ref: the state before any restart handling
            _at_mcu(m, rd, pred, togo, rst)
        if ri > 0 and togo == 0:
            p = rd.byte_pos()
            if rd.nbits - rd.cur >= 8 or p + 1 >= len(seg) or seg[p] != 0xFF or seg[p + 1] != 0xD0 + rst:
                status = 4
                break
            rd.load(p + 2)
            rst, pred, togo = (rst + 1) & 7, [0] * nc, ri
        if ri > 0:
            togo -= 1
        myi, mxi = divmod(m, mx)
        for c in range(nc):
            for bv in range(vs[c]):
                for bh in range(hs[c]):
                    if status:
                        break
                    blk = coef[c][myi * vs[c] + bv, mxi * hs[c] + bh]
                    t = sym(int(tb["dc_sel"][c]) & 3)
                    if t is None or t > 15:
                        status = 2
                        break
                    pred[c] = (pred[c] + extend(t) + 2 ** 31) % 2 ** 32 - 2 ** 31
                    blk[0] = (pred[c] + 2 ** 15) % 2 ** 16 - 2 ** 15
                    k = 1
                    while k < 64:
                        rs = sym(int(tb["ac_sel"][c]) & 3)
                        if rs is None:
                            status = 2
                            break
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                status = 3
                                break
                            blk[_JPEG_ZIGZAG[k]] = extend(s)
                            k += 1
                        elif r != 15:
                            break
                        else:
                            k += 16
                    if not status and rd.over:
                        status = 1
    if _at_mcu is not None and not status:
        _at_mcu(mx * my, rd, pred, togo, rst)
    if status and not with_status:
        raise ValueError(f"jpeg_decode_ref: damaged entropy segment ({JPEG_STATUS[status]})")

    def idct_1d(c, n):
        z1 = (c[2] + c[6]) * 4433
        t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
        t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2 = z1 * -7373, z2 * -20995
        z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        r = 1 << (n - 1)
        return [(x + r) >> n for x in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)]

    planes = []
    for c in range(nc):
        x = coef[c] * tb["q"][c].astype(np.int64)                 # [by, bx, 64]
        x = x.reshape(x.shape[0], x.shape[1], 8, 8)
        p1 = np.stack(idct_1d([x[:, :, k, :] for k in range(8)], 11), axis=2)                      # down the columns
        p2 = np.stack(idct_1d([p1[:, :, :, k].astype(np.int32).astype(np.int64) for k in range(8)], 18), axis=3)   # along the rows
        s = np.clip(p2 + 128, 0, 255)
        planes.append(s.transpose(0, 2, 1, 3).reshape(s.shape[0] * 8, s.shape[1] * 8))
    Y = planes[0][:H, :W]
    if nc == 1:
        R = G = B = Y
    else:
        dw, dh = -(-W // hmax), -(-H // vmax)
        up = []
        for p in planes[1:]:
            p = p[:dh, :dw]
            if hmax == 1:
                o = p
            elif dw <= 2:
                o = np.repeat(np.repeat(p, vmax, axis=0), 2, axis=1)
            else:
                if vmax == 2:
                    o = np.empty((2 * dh, 2 * dw), dtype=np.int64)
                    above, below = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
                    for v, far, b0, b1 in ((0, above, 8, 7), (1, below, 8, 7)):
                        s = 3 * p + far
                        left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
                        o[v::2, 0::2] = (3 * s + left + b0) >> 4
                        o[v::2, 1::2] = (3 * s + right + b1) >> 4
                else:
                    o = np.empty((dh, 2 * dw), dtype=np.int64)
                    left, right = np.concatenate([p[:, :1], p[:, :-1]], axis=1), np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
                    o[:, 0::2] = (3 * p + left + 1) >> 2
                    o[:, 1::2] = (3 * p + right + 2) >> 2
                    o[:, 0], o[:, -1] = p[:, 0], p[:, -1]
            up.append(o[:H, :W])
        cb, cr = up[0] - 128, up[1] - 128
        R = np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255)
        B = np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)
        G = np.clip(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0, 255)
    if form == "u16":
        out = B.astype(np.uint16)
    else:
        out = np.stack([B, G, R] if form == "bgr" else [R, G, B], axis=-1).astype(np.uint8)
    out = np.ascontiguousarray(out)
    return (out, status) if with_status else out


def jpeg_marks_ref(buf, rows_per_mark=1, info=None):
    """numpy statement of ``jpeg_index`` for one file (the definition is at actmi_jpeg_mark in actmi.h): the walk of
    ``jpeg_decode_ref`` -> (marks, status): ``jpeg_mark_dtype`` records [M + 1], M = ceil(my / rows_per_mark), mark j the scan's state
    at the entry of the first MCU of row j * rows_per_mark, before any restart handling of it, mark M the state after the last MCU.
    The marks of a file whose status is not 0 are unspecified (here: zero from the failing row on)."""
    import numpy as np
    R = int(rows_per_mark)
    if R < 1:
        raise ValueError("jpeg_marks_ref: rows_per_mark must be at least 1")
    if info is None:
        info = jpeg_parse(buf)
    hmax, vmax = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[info["mode"]]
    mx, my = -(-info["W"] // (8 * hmax)), -(-info["H"] // (8 * vmax))
    M = -(-my // R)
    marks = np.zeros(M + 1, dtype=jpeg_mark_dtype())

    def at_mcu(m, rd, pred, togo, rst):
        row, col = divmod(m, mx)
        if col or (row % R and row != my):
            return
        k = M if row == my else row // R
        marks[k]["byte_off"], marks[k]["bit"] = rd.mark_pos()
        marks[k]["pred"][:len(pred)] = pred
        marks[k]["togo"], marks[k]["rst"] = togo, rst
    _, status = jpeg_decode_ref(buf, with_status=True, info=info, _at_mcu=at_mcu)
    return marks, status


def _jpeg_bytes(buf):
    import numpy as np
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(buf, dtype=np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)


def _jpeg_plan(bufs, infos, form, offsets, table_index):
    """what one decode call takes, from the files: -> (H, W, mode, stream [bytes] u8, frames [n] records, frame_bytes).  The entropy
    segments are laid back to back; frame i goes to offsets[i] (default: i * frame_bytes)."""
    import numpy as np
    if form not in JPEG_FORMS:
        raise ValueError(f"jpeg_decode: form must be one of {sorted(JPEG_FORMS)}")
    bufs = [_jpeg_bytes(b) for b in bufs]
    if infos is None:
        infos = [jpeg_parse(b) for b in bufs]
    if not bufs or len(infos) != len(bufs):
        raise ValueError("jpeg_decode: no frames, or not one parse per frame")
    H, W, mode = infos[0]["H"], infos[0]["W"], infos[0]["mode"]
    if any((i["H"], i["W"], i["mode"]) != (H, W, mode) for i in infos):
        raise ValueError("jpeg_decode: one call decodes frames of one size and one sampling mode")
    fb = H * W * (2 if form == "u16" else 3)
    frames = np.zeros(len(bufs), dtype=jpeg_frame_dtype())
    lens = np.asarray([i["seg_len"] for i in infos], dtype=np.int64)
    frames["seg_len"] = lens
    frames["seg_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    frames["dst_off"] = np.arange(len(bufs), dtype=np.int64) * fb if offsets is None else np.asarray(offsets, dtype=np.int64)
    frames["restart_interval"] = [i["restart_interval"] for i in infos]
    frames["table_set"] = [table_index(i["tables"]) for i in infos]
    stream = np.concatenate([b[i["seg_off"]:i["seg_off"] + i["seg_len"]] for b, i in zip(bufs, infos)] + [np.zeros(1, dtype=np.uint8)])
    return H, W, mode, stream, frames, fb


class _JpegTableSets:
    """table sets deduplicated by content (cv2 writes the same standard tables into every frame of a recording)"""

    def __init__(self):
        self.sets, self._index = [], {}

    def index(self, tables):
        key = tables.tobytes()
        i = self._index.get(key)
        if i is None:
            i = self._index[key] = len(self.sets)
            self.sets.append(key)
        return i

    def array(self):
        import numpy as np
        return np.frombuffer(b"".join(self.sets), dtype=np.uint8).copy()


def _aligned_u8(nbytes, align=16):
    import numpy as np
    raw = np.empty(nbytes + align, dtype=np.uint8)
    o = (-raw.ctypes.data) % align
    return raw[o:o + nbytes]


def jpeg_decode_host(bufs, out=None, offsets=None, form="bgr", infos=None, ws=None):
    """actmi_jpeg_decode_host, the CPU twin of ``jpeg_decode`` (the same core, no device): `bufs` JPEG files of one size and
    sampling mode -> (out, status): out u8 [n, H, W, 3] / uint16 [n, H, W], or the caller's contiguous 1-D uint8 array in which frame
    i starts at byte offsets[i]; status int32 [n].  ``infos``: a parse per file that replaces ``jpeg_parse`` (tests change a
    segment after it was parsed).  ``ws``: a 16-byte aligned uint8 array of at least ``jpeg_workspace_bytes`` bytes."""
    import numpy as np
    sets = _JpegTableSets()
    H, W, mode, stream, frames, fb = _jpeg_plan(bufs, infos, form, offsets, sets.index)
    n = len(frames)
    if out is None:
        if offsets is not None:
            raise ValueError("jpeg_decode_host: offsets name places in the caller's out")
        out = np.empty((n,) + jpeg_out_shape(H, W, form), dtype=np.uint16 if form == "u16" else np.uint8)
    elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
        raise ValueError("jpeg_decode_host: out must be a contiguous 1-D uint8 array")
    lib = L.load()
    need = int(lib.actmi_op_jpeg_workspace_bytes(n, H, W, JPEG_MODES[mode]))
    if ws is None:
        ws = _aligned_u8(need)
    tables = _aligned_u8(len(sets.sets) * jpeg_tables_dtype().itemsize)
    tables[:] = sets.array()
    status = np.full(n, -1, dtype=np.int32)
    d = L.JpegDesc()
    d.stream, d.stream_bytes, d.frames, d.tables = stream.ctypes.data, stream.size - 1, frames.ctypes.data, tables.ctypes.data
    d.dst, d.dst_bytes, d.ws, d.ws_bytes, d.status = out.ctypes.data, out.nbytes, ws.ctypes.data, ws.nbytes, status.ctypes.data
    d.n, d.n_tables, d.H, d.W, d.mode, d.form = n, len(sets.sets), H, W, JPEG_MODES[mode], JPEG_FORMS[form]
    L.check(lib.actmi_jpeg_decode_host(C.byref(d)), None, "jpeg_decode_host")
    return out, status


def jpeg_workspace_bytes(n, H, W, mode):
    return int(L.load().actmi_op_jpeg_workspace_bytes(int(n), int(H), int(W), JPEG_MODES[mode]))


def jpeg_mark_count(H, mode, rows_per_mark=1):
    """M: a frame of H lines has M + 1 marks"""
    if int(rows_per_mark) < 1:
        raise ValueError("jpeg marks: rows_per_mark must be at least 1")
    my = -(-int(H) // (16 if mode == "420" else 8))
    return -(-my // int(rows_per_mark))


def _host_desc(stream, frames, tables, n_tables, status, H, W, mode, form="bgr", out=None, ws=None):
    d = L.JpegDesc()
    d.stream, d.stream_bytes, d.frames, d.tables, d.status = stream.ctypes.data, stream.size - 1, frames.ctypes.data, tables.ctypes.data, status.ctypes.data
    if out is not None:
        d.dst, d.dst_bytes, d.ws, d.ws_bytes = out.ctypes.data, out.nbytes, ws.ctypes.data, ws.nbytes
    d.n, d.n_tables, d.H, d.W, d.mode, d.form = len(frames), n_tables, H, W, JPEG_MODES[mode], JPEG_FORMS[form]
    return d


def jpeg_index_host(bufs, rows_per_mark=1, infos=None):
    """actmi_jpeg_index_host, the CPU twin of ``jpeg_index``: `bufs` JPEG files of one size and sampling mode -> (marks, status):
    ``jpeg_mark_dtype`` records [n, M + 1] (``jpeg_marks_ref`` of every file whose status is 0), status int32 [n]"""
    import numpy as np
    sets = _JpegTableSets()
    H, W, mode, stream, frames, _fb = _jpeg_plan(bufs, infos, "bgr", None, sets.index)
    n, M = len(frames), jpeg_mark_count(H, mode, rows_per_mark)
    tables = _aligned_u8(len(sets.sets) * jpeg_tables_dtype().itemsize)
    tables[:] = sets.array()
    status = np.full(n, -1, dtype=np.int32)
    marks = np.zeros((n, M + 1), dtype=jpeg_mark_dtype())
    first = np.arange(n, dtype=np.int64) * (M + 1)
    d = _host_desc(stream, frames, tables, len(sets.sets), status, H, W, mode)
    m = L.JpegMarks()
    m.marks, m.n_marks, m.first, m.rows_per_mark = marks.ctypes.data, marks.size, first.ctypes.data, int(rows_per_mark)
    L.check(L.load().actmi_jpeg_index_host(C.byref(d), C.byref(m)), None, "jpeg_index_host")
    return marks, status


def jpeg_decode_marked_host(bufs, marks, first=None, rows_per_mark=1, out=None, offsets=None, form="bgr", infos=None, ws=None, sticky=None):
    """actmi_jpeg_decode_marked_host, the CPU twin of ``jpeg_decode_marked``: as ``jpeg_decode_host``, every frame entered at its
    marks.  `marks`: ``jpeg_mark_dtype`` records, [n, M + 1] or any flat array with first[i] the index of frame i's mark 0.
    ``sticky``: an int32 array of one word that receives the largest status.  -> (out, status)"""
    import numpy as np
    sets = _JpegTableSets()
    H, W, mode, stream, frames, fb = _jpeg_plan(bufs, infos, form, offsets, sets.index)
    n = len(frames)
    marks = np.ascontiguousarray(marks, dtype=jpeg_mark_dtype())
    if first is None:
        if marks.ndim != 2 or marks.shape[0] != n:
            raise ValueError("jpeg_decode_marked_host: marks must be [n, M + 1] when first is not given")
        first = np.arange(n, dtype=np.int64) * marks.shape[1]
    first = np.ascontiguousarray(first, dtype=np.int64)
    if first.shape != (n,):
        raise ValueError("jpeg_decode_marked_host: first must hold one index per frame")
    if out is None:
        if offsets is not None:
            raise ValueError("jpeg_decode_marked_host: offsets name places in the caller's out")
        out = np.empty((n,) + jpeg_out_shape(H, W, form), dtype=np.uint16 if form == "u16" else np.uint8)
    elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
        raise ValueError("jpeg_decode_marked_host: out must be a contiguous 1-D uint8 array")
    if sticky is not None and (not isinstance(sticky, np.ndarray) or sticky.dtype != np.int32 or sticky.size != 1):
        raise ValueError("jpeg_decode_marked_host: sticky must be an int32 array of one word")
    if ws is None:
        ws = _aligned_u8(jpeg_workspace_bytes(n, H, W, mode))
    tables = _aligned_u8(len(sets.sets) * jpeg_tables_dtype().itemsize)
    tables[:] = sets.array()
    status = np.full(n, -1, dtype=np.int32)
    d = _host_desc(stream, frames, tables, len(sets.sets), status, H, W, mode, form, out, ws)
    m = L.JpegMarks()
    m.marks, m.n_marks, m.first, m.rows_per_mark = marks.ctypes.data if marks.size else None, marks.size, first.ctypes.data, int(rows_per_mark)
    m.sticky = sticky.ctypes.data if sticky is not None else None
    L.check(L.load().actmi_jpeg_decode_marked_host(C.byref(d), C.byref(m)), None, "jpeg_decode_marked_host")
    return out, status


class JpegDecoder:
    """The device state of ``jpeg_decode`` for frames of one size: the workspace (``max_frames`` slots of the largest sampling mode
    met so far), the table sets met so far, deduplicated by content and uploaded when a new one appears, and one parse cache (the
    frames of a recording share their header bytes).  ``decode`` launches actmi_op_jpeg_decode for up to ``max_frames`` frames at a
    time on the current stream and returns the statuses as a device tensor: nothing is read back here."""

    def __init__(self, device, H, W, max_frames=64):
        self.device, self.H, self.W, self.max_frames = torch.device(device), int(H), int(W), int(max_frames)
        if self.max_frames < 1 or self.max_frames > 65535:
            raise ValueError("JpegDecoder: max_frames must be in 1..65535")
        self._sets, self._uploaded, self._tables = _JpegTableSets(), 0, None
        self._ws, self._hdr = None, None

    def parse(self, buf):
        """``jpeg_parse`` of one file; a file that begins with the bytes of the last one's header reuses its parse"""
        import numpy as np
        a = _jpeg_bytes(buf)
        if self._hdr is not None:
            head, info = self._hdr
            k = len(head)
            if a.size > k + 1 and a[:k].tobytes() == head:
                tail = a[k:]
                ff = np.flatnonzero(tail[:-1] == 0xFF)
                nxt = tail[ff + 1]
                stop = ff[(nxt != 0) & ((nxt < 0xD0) | (nxt > 0xD7))]
                if stop.size and int(tail[stop[0] + 1]) == 0xD9:
                    return dict(info, seg_len=int(stop[0]))
        info = jpeg_parse(a)
        self._hdr = (a[:info["seg_off"]].tobytes(), info)
        return info

    def table_index(self, tables):
        return self._sets.index(tables)

    def workspace_bytes(self, mode):
        return jpeg_workspace_bytes(self.max_frames, self.H, self.W, mode)

    def decode(self, stream, frames, mode, form, dst):
        """stream: 1-D uint8 tensor on the device holding the entropy segments; frames: ``jpeg_frame_dtype`` records (numpy); dst: a
        contiguous tensor on the device (any dtype: offsets and the bound are bytes) -> status int32 [n] on the device"""
        n = len(frames)
        if n == 0:
            return torch.zeros(0, dtype=torch.int32, device=self.device)
        if stream.dtype != torch.uint8 or stream.dim() != 1 or stream.device != self.device or not stream.is_contiguous():
            raise ValueError(f"JpegDecoder: stream must be a contiguous 1-D uint8 tensor on {self.device}")
        if dst.device != self.device or not dst.is_contiguous():
            raise ValueError(f"JpegDecoder: dst must be contiguous on {self.device}")
        lib = L.load()
        if len(self._sets.sets) != self._uploaded:
            self._tables = torch.from_numpy(self._sets.array()).to(self.device)
            self._uploaded = len(self._sets.sets)
        if self._tables is None:
            raise ValueError("JpegDecoder: no table set (table_index gives the frames' indices)")
        need = self.workspace_bytes(mode)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        import numpy as np
        rec = torch.from_numpy(np.ascontiguousarray(frames).view(np.uint8).reshape(-1).copy()).to(self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        d = L.JpegDesc()
        d.stream, d.stream_bytes, d.tables, d.n_tables = stream.data_ptr(), int(stream.numel()), self._tables.data_ptr(), self._uploaded
        d.dst, d.dst_bytes, d.ws, d.ws_bytes = dst.data_ptr(), int(dst.numel() * dst.element_size()), self._ws.data_ptr(), int(self._ws.numel())
        d.H, d.W, d.mode, d.form = self.H, self.W, JPEG_MODES[mode], JPEG_FORMS[form]
        with torch.cuda.device(self.device):
            for i0 in range(0, n, self.max_frames):
                m = min(self.max_frames, n - i0)
                d.frames, d.status, d.n = rec.data_ptr() + 32 * i0, status.data_ptr() + 4 * i0, m
                L.check(lib.actmi_op_jpeg_decode(C.byref(d), L.current_stream_ptr()), None, "op_jpeg_decode")
        return status

    def _marked_args(self, what, stream, frames, marks, first):
        """the checks and uploads the two mark ops share -> (records on the device, n, first on the device)"""
        import numpy as np
        if stream.dtype != torch.uint8 or stream.dim() != 1 or stream.device != self.device or not stream.is_contiguous():
            raise ValueError(f"JpegDecoder.{what}: stream must be a contiguous 1-D uint8 tensor on {self.device}")
        if torch.is_tensor(frames):
            if frames.dtype != torch.uint8 or frames.device != self.device or not frames.is_contiguous() or frames.numel() % 32:
                raise ValueError(f"JpegDecoder.{what}: frames on the device are contiguous uint8 records of 32 bytes")
            rec = frames
        else:
            rec = torch.from_numpy(np.ascontiguousarray(frames, dtype=jpeg_frame_dtype()).view(np.uint8).reshape(-1).copy()).to(self.device)
        n = rec.numel() // 32
        if marks.dtype != torch.uint8 or marks.device != self.device or not marks.is_contiguous() or marks.numel() % 32 or marks.data_ptr() % 8:
            raise ValueError(f"JpegDecoder.{what}: marks must be a contiguous, 8-byte aligned uint8 tensor of 32-byte records on {self.device}")
        if first is None:
            raise ValueError(f"JpegDecoder.{what}: marks come with first, the index of every frame's mark 0")
        if not torch.is_tensor(first):
            first = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int64)).to(self.device)
        if first.dtype != torch.int64 or first.device != self.device or not first.is_contiguous() or first.numel() != n:
            raise ValueError(f"JpegDecoder.{what}: first must hold one int64 index per frame on {self.device}")
        if len(self._sets.sets) != self._uploaded:
            self._tables = torch.from_numpy(self._sets.array()).to(self.device)
            self._uploaded = len(self._sets.sets)
        if self._tables is None:
            raise ValueError("JpegDecoder: no table set (table_index gives the frames' indices)")
        return rec, n, first

    def index(self, stream, frames, mode, marks=None, first=None, rows_per_mark=1):
        """actmi_op_jpeg_index: the entropy walk alone.  stream, frames as ``decode`` (frames may also be records on the device).
        ``marks``: a uint8 tensor of 32-byte ``jpeg_mark_dtype`` records on the device with first[i] the index of frame i's mark 0;
        without it one of [n, M + 1, 32] is made.  -> (marks, status int32 [n] on the device)"""
        M = jpeg_mark_count(self.H, mode, rows_per_mark)
        if marks is None:
            n = frames.numel() // 32 if torch.is_tensor(frames) else len(frames)
            marks = torch.zeros((n, M + 1, 32), dtype=torch.uint8, device=self.device)
            first = torch.arange(n, dtype=torch.int64, device=self.device) * (M + 1)
        rec, n, first = self._marked_args("index", stream, frames, marks, first)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return marks, status
        d, m = L.JpegDesc(), L.JpegMarks()
        d.stream, d.stream_bytes, d.tables, d.n_tables = stream.data_ptr(), int(stream.numel()), self._tables.data_ptr(), self._uploaded
        d.H, d.W, d.mode = self.H, self.W, JPEG_MODES[mode]
        m.marks, m.n_marks, m.rows_per_mark = marks.data_ptr(), marks.numel() // 32, int(rows_per_mark)
        lib = L.load()
        with torch.cuda.device(self.device):
            for i0 in range(0, n, self.max_frames):
                d.frames, d.status, d.n = rec.data_ptr() + 32 * i0, status.data_ptr() + 4 * i0, min(self.max_frames, n - i0)
                m.first = first.data_ptr() + 8 * i0
                L.check(lib.actmi_op_jpeg_index(C.byref(d), C.byref(m), L.current_stream_ptr()), None, "op_jpeg_index")
        return marks, status

    def decode_marked(self, stream, frames, marks, first, mode, form, dst, sticky=None, rows_per_mark=1):
        """actmi_op_jpeg_decode_marked: ``decode`` with every frame entered at its marks (what ``index`` wrote, with the same
        ``rows_per_mark``).  ``sticky``: an int32 tensor of one word on the device that receives the largest status of the launches.
        -> status int32 [n] on the device"""
        rec, n, first = self._marked_args("decode_marked", stream, frames, marks, first)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return status
        if dst.device != self.device or not dst.is_contiguous():
            raise ValueError(f"JpegDecoder: dst must be contiguous on {self.device}")
        if sticky is not None and (sticky.dtype != torch.int32 or sticky.numel() != 1 or sticky.device != self.device):
            raise ValueError(f"JpegDecoder.decode_marked: sticky must be an int32 tensor of one word on {self.device}")
        need = self.workspace_bytes(mode)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        d, m = L.JpegDesc(), L.JpegMarks()
        d.stream, d.stream_bytes, d.tables, d.n_tables = stream.data_ptr(), int(stream.numel()), self._tables.data_ptr(), self._uploaded
        d.dst, d.dst_bytes, d.ws, d.ws_bytes = dst.data_ptr(), int(dst.numel() * dst.element_size()), self._ws.data_ptr(), int(self._ws.numel())
        d.H, d.W, d.mode, d.form = self.H, self.W, JPEG_MODES[mode], JPEG_FORMS[form]
        m.marks, m.n_marks, m.rows_per_mark = marks.data_ptr(), marks.numel() // 32, int(rows_per_mark)
        m.sticky = sticky.data_ptr() if sticky is not None else None
        lib = L.load()
        with torch.cuda.device(self.device):
            for i0 in range(0, n, self.max_frames):
                d.frames, d.status, d.n = rec.data_ptr() + 32 * i0, status.data_ptr() + 4 * i0, min(self.max_frames, n - i0)
                m.first = first.data_ptr() + 8 * i0
                L.check(lib.actmi_op_jpeg_decode_marked(C.byref(d), C.byref(m), L.current_stream_ptr()), None, "op_jpeg_decode_marked")
        return status


def jpeg_decode(bufs, out=None, offsets=None, form="bgr", infos=None, device=None, decoder=None):
    """actmi_op_jpeg_decode: `bufs` JPEG files (1-D uint8 arrays or bytes) of one size and sampling mode, decoded on the device ->
    (out, status): out u8 [n, H, W, 3] in B, G, R (``form`` "bgr") or R, G, B ("rgb") order, or uint16 [n, H, W] ("u16": channel 0 of
    the B, G, R pixel) -- or the caller's contiguous cuda tensor, in which frame i starts at byte offsets[i]; status int32 [n] on the
    device, 0 or the cause (``JPEG_STATUS``): the pixels of such a frame are unspecified, those of every other frame are
    ``jpeg_decode_ref``'s bit for bit.  A file ``jpeg_parse`` refuses raises ``JpegUnsupported``: nothing is launched."""
    import numpy as np
    if out is not None:
        device = out.device
    elif device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    sets = decoder._sets if decoder is not None else _JpegTableSets()
    H, W, mode, stream, frames, fb = _jpeg_plan(bufs, infos, form, offsets, sets.index)
    n = len(frames)
    if decoder is None:
        decoder = JpegDecoder(device, H, W, max_frames=min(n, 256))
        decoder._sets = sets
    elif (decoder.H, decoder.W) != (H, W) or decoder.device != device:
        raise ValueError(f"jpeg_decode: the decoder is for {decoder.H} x {decoder.W} frames on {decoder.device}")
    if out is None:
        if offsets is not None:
            raise ValueError("jpeg_decode: offsets name places in the caller's out")
        out = torch.empty((n,) + jpeg_out_shape(H, W, form), dtype=torch.uint16 if form == "u16" else torch.uint8, device=device)
    elif not out.is_cuda or not out.is_contiguous():
        raise ValueError("jpeg_decode: out must be a contiguous cuda tensor")
    pinned = torch.empty(stream.size, dtype=torch.uint8, pin_memory=True)     # one byte more than the segments: never empty
    pinned.numpy()[:] = stream
    dev_stream = pinned.to(device, non_blocking=True)
    status = decoder.decode(dev_stream, frames, mode, form, out)
    torch.cuda.current_stream(device).synchronize()                # the pinned staging is this call's alone
    return out, status


def _jpeg_device_call(what, bufs, infos, form, offsets, device, decoder):
    """what ``jpeg_index`` and ``jpeg_decode_marked`` share: the plan, the decoder and the segments on the device"""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    sets = decoder._sets if decoder is not None else _JpegTableSets()
    H, W, mode, stream, frames, _fb = _jpeg_plan(bufs, infos, form, offsets, sets.index)
    if decoder is None:
        decoder = JpegDecoder(device, H, W, max_frames=min(len(frames), 256))
        decoder._sets = sets
    elif (decoder.H, decoder.W) != (H, W) or decoder.device != device:
        raise ValueError(f"{what}: the decoder is for {decoder.H} x {decoder.W} frames on {decoder.device}")
    return decoder, mode, torch.from_numpy(stream).to(device), frames


def jpeg_index(bufs, infos=None, device=None, decoder=None, rows_per_mark=1):
    """actmi_op_jpeg_index: `bufs` JPEG files of one size and sampling mode, their entropy segments walked once on the device ->
    (marks, status): marks uint8 [n, M + 1, 32] on the device (``jpeg_mark_dtype`` records: ``jpeg_marks_ref`` of every file whose
    status is 0), status int32 [n] on the device"""
    decoder, mode, stream, frames = _jpeg_device_call("jpeg_index", bufs, infos, "bgr", None, device, decoder)
    return decoder.index(stream, frames, mode, rows_per_mark=rows_per_mark)


def jpeg_decode_marked(bufs, marks, first=None, rows_per_mark=1, out=None, offsets=None, form="bgr", infos=None, device=None, decoder=None,
                       sticky=None):
    """actmi_op_jpeg_decode_marked: ``jpeg_decode`` with every frame entered at its marks (uint8 [n, M + 1, 32] on the device, or any
    block of records with first[i] the index of frame i's mark 0) -> (out, status)"""
    if out is not None:
        device = out.device
    decoder, mode, stream, frames = _jpeg_device_call("jpeg_decode_marked", bufs, infos, form, offsets, device, decoder)
    n = len(frames)
    if first is None:
        if marks.dim() != 3 or marks.shape[0] != n:
            raise ValueError("jpeg_decode_marked: marks must be [n, M + 1, 32] when first is not given")
        first = torch.arange(n, dtype=torch.int64, device=decoder.device) * marks.shape[1]
    if out is None:
        if offsets is not None:
            raise ValueError("jpeg_decode_marked: offsets name places in the caller's out")
        out = torch.empty((n,) + jpeg_out_shape(decoder.H, decoder.W, form), dtype=torch.uint16 if form == "u16" else torch.uint8,
                          device=decoder.device)
    elif not out.is_cuda or not out.is_contiguous():
        raise ValueError("jpeg_decode_marked: out must be a contiguous cuda tensor")
    status = decoder.decode_marked(stream, frames, marks, first, mode, form, out, sticky=sticky, rows_per_mark=rows_per_mark)
    return out, status


# ---- baseline JPEG encode (csrc/jpeg_encode.hip, csrc/jpeg_enc_core.h; the definition is at actmi_op_jpeg_encode in actmi.h) -----
JPEG_ST_DEST = 5
_JPEG_STD_Q = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
# the standard Huffman tables of Annex K in the order of the file's DHT segments: (class << 4 | index, counts per length, symbols)
_JPEG_STD_DHT = (
    (0x00, "00010501010101010100000000000000", "000102030405060708090a0b"),
    (0x10, "0002010303020403050504040000017d",
     "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
     "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
     "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    (0x01, "00030101010101010101010000000000", "000102030405060708090a0b"),
    (0x11, "00020102040403040705040400010277",
     "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
     "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
     "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def _jpeg_enc_args(mode, form=None, quality=None):
    """the Python layer's refusals: the encoder takes 4:2:0 and 4:4:4, B, G, R or R, G, B pixels, a quality in 1..100"""
    if mode not in ("420", "444"):
        raise ValueError(f"jpeg_encode: mode must be '420' or '444' (4:2:2 and gray are not encoded), got {mode!r}")
    if form is not None and form not in ("bgr", "rgb"):
        raise ValueError(f"jpeg_encode: form must be 'bgr' or 'rgb', got {form!r}")
    if quality is not None and not (int(quality) == quality and 1 <= int(quality) <= 100):
        raise ValueError(f"jpeg_encode: quality must be an integer in 1..100, got {quality!r}")


def jpeg_quant_tables(quality):
    """the luma and chroma quantisation tables of a quality, uint16 [2, 64] in natural order: Annex K scaled as
    ``jpeg_set_quality(quality, force_baseline)`` scales it"""
    import numpy as np
    _jpeg_enc_args("420", quality=quality)
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(_JPEG_STD_Q, dtype=np.int64) * s + 50) // 100, 1, 255).astype(np.uint16)


def jpeg_file_header(H, W, quality=50, mode="420"):
    """everything ``Image.save(..., "JPEG", quality=quality, subsampling=...)`` writes ahead of the entropy segment of an H x W frame:
    SOI, JFIF APP0, two DQT segments, SOF0, four DHT segments, SOS"""
    import numpy as np
    _jpeg_enc_args(mode, quality=quality)
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("jpeg_file_header: H and W must be in 1..65535")
    q = jpeg_quant_tables(quality)
    zz = np.asarray(_JPEG_ZIGZAG)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + q[t][zz].astype(np.uint8).tobytes()
    out += b"\xff\xc0\x00\x11\x08" + bytes([H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22 if mode == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, counts, vals in _JPEG_STD_DHT:
        body = bytes([tc_th]) + bytes.fromhex(counts) + bytes.fromhex(vals)
        out += b"\xff\xc4" + bytes([(len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def jpeg_assemble(header, segment):
    """the file: ``jpeg_file_header``'s bytes, the entropy segment (bytes or a uint8 array), EOI"""
    import numpy as np
    seg = segment if isinstance(segment, (bytes, bytearray)) else np.ascontiguousarray(segment, dtype=np.uint8).tobytes()
    return bytes(header) + bytes(seg) + b"\xff\xd9"


def _jpeg_std_codes():
    """symbol -> (code, size) of the four standard tables, in ``_JPEG_STD_DHT``'s order"""
    tables = []
    for _id, counts, vals in _JPEG_STD_DHT:
        counts, vals = bytes.fromhex(counts), bytes.fromhex(vals)
        code, k, t = 0, 0, {}
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                t[vals[k]] = (code, l)
                code += 1
                k += 1
            code <<= 1
        tables.append(t)
    return tables


def _jpeg_fdct_ref(d, pass1):
    """one pass of jfdctint's islow along the last axis of int64 [..., 8]"""
    import numpy as np
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if pass1 else 15
    r = 1 << (n - 1)
    o = np.empty_like(d)
    if pass1:
        o[..., 0], o[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[..., 0], o[..., 4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o[..., 2], o[..., 6] = (z1 + t13 * 6270 + r) >> n, (z1 - t12 * 15137 + r) >> n
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7], o[..., 5], o[..., 3], o[..., 1] = (t4 + z1 + z3 + r) >> n, (t5 + z2 + z4 + r) >> n, (t6 + z2 + z3 + r) >> n, (t7 + z1 + z4 + r) >> n
    return o


def _jpeg_edge(p, rows, cols):
    """`p` extended to rows x cols by repeating its last row and column"""
    import numpy as np
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def jpeg_encode_segment_ref(frame, quality=50, mode="420", form="bgr", symbols=None, row_states=None):
    """The numpy statement of actmi_op_jpeg_encode (the text is at its declaration in actmi.h): `frame` uint8 [H, W, 3] -> the
    entropy segment as bytes.  ``symbols``: a list that receives (table, symbol) of every Huffman symbol emitted, table 0..3 in the
    order of the file's DHT segments (DC luma, AC luma, DC chroma, AC chroma).  ``row_states``: a list that receives, before every
    MCU row and once after the last, (the data bits put so far, the three DC predictors); a last entry holds the unstuffed bytes."""
    import numpy as np
    _jpeg_enc_args(mode, form, quality)
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(f"jpeg_encode: a frame is uint8 [H, W, 3], got {f.dtype} {f.shape}")
    H, W = f.shape[:2]
    f = f.astype(np.int64)
    R, G, B = (f[..., 0], f[..., 1], f[..., 2]) if form == "rgb" else (f[..., 2], f[..., 1], f[..., 0])
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16
    hs = 2 if mode == "420" else 1
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * hs))
    planes = [_jpeg_edge(Y, 8 * hs * mh, 8 * hs * mw)]
    for p in (Cb, Cr):
        if mode == "420":
            p = _jpeg_edge(p, 2 * -(-H // 2), 16 * mw)
            bias = np.tile(np.asarray([1, 2], dtype=np.int64), 4 * mw)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        planes.append(_jpeg_edge(p, 8 * mh, 8 * mw))
    q = jpeg_quant_tables(quality).astype(np.int64)
    zz = np.asarray(_JPEG_ZIGZAG)
    coef = []                                                     # per component [block rows, block cols, 64] in zigzag order
    for c, p in enumerate(planes):
        b = (p - 128).reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        b = _jpeg_fdct_ref(b, True)                               # along the rows
        b = _jpeg_fdct_ref(b.swapaxes(-1, -2), False).swapaxes(-1, -2)   # down the columns
        d = 8 * q[1 if c else 0].reshape(8, 8)
        b = np.sign(b) * ((np.abs(b) + (d >> 1)) // d)
        coef.append(b.reshape(b.shape[0], b.shape[1], 64)[..., zz])
    tables = _jpeg_std_codes()
    rbw, rbh = -(-W // 8), -(-H // 8)
    bits, pred, last_dc, nbits = [], [0, 0, 0], 0, [0]

    def put(code, size):
        if size:
            bits.append(format(code, f"0{size}b"))
            nbits[0] += size

    def sym(t, s):
        if symbols is not None:
            symbols.append((t, s))
        put(*tables[t][s])

    def value(v, s):
        put(v + (1 << s) - 1 if v < 0 else v, s)

    for my in range(mh):
        if row_states is not None:
            row_states.append((nbits[0], tuple(pred)))
        for mx in range(mw):
            for c in range(3):
                dc_t, ac_t = (0, 1) if c == 0 else (2, 3)
                h = hs if c == 0 else 1
                for bv in range(h):
                    for bh in range(h):
                        by, bx = my * h + bv, mx * h + bh
                        blk = coef[c][by, bx]
                        if c == 0 and (bx >= rbw or by >= rbh):   # a dummy block: the DC of the block emitted before it in Y
                            blk = np.zeros(64, dtype=np.int64)
                            blk[0] = last_dc
                        if c == 0:
                            last_dc = int(blk[0])
                        diff = int(blk[0]) - pred[c]
                        pred[c] = int(blk[0])
                        s = abs(diff).bit_length()
                        sym(dc_t, s)
                        value(diff, s)
                        run = 0
                        for k in range(1, 64):
                            v = int(blk[k])
                            if v == 0:
                                run += 1
                                continue
                            while run >= 16:
                                sym(ac_t, 0xF0)
                                run -= 16
                            s = abs(v).bit_length()
                            sym(ac_t, (run << 4) | s)
                            value(v, s)
                            run = 0
                        if run:
                            sym(ac_t, 0x00)
    s = "".join(bits)
    s += "1" * (-len(s) % 8)
    unstuffed = int(s, 2).to_bytes(len(s) // 8, "big")
    if row_states is not None:
        row_states += [(nbits[0], tuple(pred)), unstuffed]
    return unstuffed.replace(b"\xff", b"\xff\x00")


def jpeg_encode_marks_ref(frame, quality=50, mode="420", form="bgr", rows_per_mark=1):
    """numpy statement of the marks actmi_op_jpeg_encode_marked writes for one frame (the rule is at its declaration in actmi.h),
    from the encoder's symbol walk and not from a decode of what it wrote: ``jpeg_mark_dtype`` records [M + 1], M = ceil(my /
    rows_per_mark).  Mark j, the state before MCU row j * rows_per_mark (mark M: after the last MCU), with b the data bits put before
    it and u = b >> 3: bit = b & 7, byte_off = u + the 0xFF bytes among the unstuffed bytes [0, u), pred the DC predictors the walk
    holds there, togo = rst = 0."""
    import numpy as np
    R = int(rows_per_mark)
    if R < 1:
        raise ValueError("jpeg_encode_marks_ref: rows_per_mark must be at least 1")
    states = []
    jpeg_encode_segment_ref(frame, quality, mode, form, row_states=states)
    unstuffed, states = np.frombuffer(states[-1], dtype=np.uint8), states[:-1]
    my = len(states) - 1
    M = -(-my // R)
    marks = np.zeros(M + 1, dtype=jpeg_mark_dtype())
    ff_before = np.concatenate([[0], np.cumsum(unstuffed == 0xFF)])   # [u]: 0xFF bytes among [0, u)
    for j in range(M + 1):
        b, pred = states[min(j * R, my)]
        u = b >> 3
        marks[j]["byte_off"], marks[j]["bit"], marks[j]["pred"] = u + int(ff_before[u]), b & 7, pred
    return marks


def jpeg_encode_ref(frame, quality=50, mode="420", form="bgr"):
    """``jpeg_encode_segment_ref`` inside its file: the bytes ``Image.fromarray(rgb).save(buf, "JPEG", quality=quality,
    subsampling=2 or 0)`` writes.  Pure numpy."""
    seg = jpeg_encode_segment_ref(frame, quality, mode, form)
    return jpeg_assemble(jpeg_file_header(frame.shape[0], frame.shape[1], quality, mode), seg)


def jpeg_enc_frame_dtype():
    """actmi_jpeg_enc_frame as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("src_off", np.int64), ("dst_off", np.int64), ("dst_cap", np.int32), ("reserved", np.int32, 3)])


def jpeg_encode_bound(H, W, mode="420"):
    """actmi_jpeg_encode_bound: bytes no entropy segment of an H x W frame can exceed"""
    _jpeg_enc_args(mode)
    return int(L.load().actmi_jpeg_encode_bound(int(H), int(W), JPEG_MODES[mode]))


def jpeg_encode_workspace_bytes(n, H, W, mode="420"):
    _jpeg_enc_args(mode)
    return int(L.load().actmi_op_jpeg_encode_workspace_bytes(int(n), int(H), int(W), JPEG_MODES[mode]))


def jpeg_enc_records(n, H, W, cap, src_off=None, dst_off=None):
    """the records of n frames laid back to back in `src`, every segment in a window of `cap` bytes (or at the offsets given)"""
    import numpy as np
    rec = np.zeros(int(n), dtype=jpeg_enc_frame_dtype())
    rec["src_off"] = np.arange(n, dtype=np.int64) * (int(H) * int(W) * 3) if src_off is None else np.asarray(src_off, dtype=np.int64)
    rec["dst_off"] = np.arange(n, dtype=np.int64) * int(cap) if dst_off is None else np.asarray(dst_off, dtype=np.int64)
    rec["dst_cap"] = cap
    return rec


def _jpeg_enc_desc(H, W, quality, mode, form, q=None):
    import numpy as np
    _jpeg_enc_args(mode, form, quality)
    d = L.JpegEncDesc()
    q = jpeg_quant_tables(quality) if q is None else np.ascontiguousarray(q, dtype=np.uint16).reshape(2, 64)
    C.memmove(d.q, q.ctypes.data, 256)
    d.H, d.W, d.mode, d.form = int(H), int(W), JPEG_MODES[mode], JPEG_FORMS[form]
    return d


def _jpeg_enc_marks(what, marks, first, rows_per_mark, n):
    """the three mark arguments of an encode come together or not at all -> whether they came"""
    given = [a is not None for a in (marks, first, rows_per_mark)]
    if any(given) and not all(given):
        raise ValueError(f"{what}: marks, first and rows_per_mark come together")
    if given[0] and int(rows_per_mark) < 1:
        raise ValueError(f"{what}: rows_per_mark must be at least 1")
    return given[0]


def jpeg_encode_host_raw(src, records, dst, H, W, quality=50, mode="420", form="bgr", ws=None, q=None, marks=None, first=None,
                         rows_per_mark=None):
    """actmi_jpeg_encode_host, the CPU twin of ``JpegEncoder.encode`` (the same core, no device), on the caller's buffers: `src` and
    `dst` contiguous 1-D uint8 arrays, `records` ``jpeg_enc_frame_dtype`` -> (seg_len, status), int32 [n] each.  ``ws``: a 16-byte
    aligned uint8 array of at least ``jpeg_encode_workspace_bytes`` bytes; ``q``: quantisation tables in place of the quality's.
    ``marks`` (a contiguous 1-D ``jpeg_mark_dtype`` array, written in place), ``first`` (int64 [n]: the index of every frame's mark
    0) and ``rows_per_mark``: actmi_jpeg_encode_marked_host instead, which also writes every frame's marks."""
    import numpy as np
    for name, a in (("src", src), ("dst", dst)):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
            raise ValueError(f"jpeg_encode_host: {name} must be a contiguous 1-D uint8 array")
    rec = np.ascontiguousarray(records, dtype=jpeg_enc_frame_dtype())
    n = len(rec)
    d = _jpeg_enc_desc(H, W, quality, mode, form, q)
    lib = L.load()
    if ws is None:
        ws = _aligned_u8(max(16, int(lib.actmi_op_jpeg_encode_workspace_bytes(n, d.H, d.W, d.mode))))
    seg_len, status = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    d.src, d.src_bytes, d.frames, d.dst, d.dst_bytes = src.ctypes.data, src.size, rec.ctypes.data, dst.ctypes.data, dst.size
    d.ws, d.ws_bytes, d.seg_len, d.status, d.n = ws.ctypes.data, ws.size, seg_len.ctypes.data, status.ctypes.data, n
    if _jpeg_enc_marks("jpeg_encode_host", marks, first, rows_per_mark, n):
        if not isinstance(marks, np.ndarray) or marks.dtype != jpeg_mark_dtype() or marks.ndim != 1 or not marks.flags.c_contiguous:
            raise ValueError("jpeg_encode_host: marks must be a contiguous 1-D array of jpeg_mark_dtype records")
        first = np.ascontiguousarray(first, dtype=np.int64)
        if first.shape != (n,):
            raise ValueError("jpeg_encode_host: first must hold one index per frame")
        m = L.JpegMarks()
        m.marks, m.n_marks, m.first, m.rows_per_mark = marks.ctypes.data if marks.size else None, marks.size, first.ctypes.data, int(rows_per_mark)
        L.check(lib.actmi_jpeg_encode_marked_host(C.byref(d), C.byref(m)), None, "jpeg_encode_marked_host")
        return seg_len, status
    L.check(lib.actmi_jpeg_encode_host(C.byref(d)), None, "jpeg_encode_host")
    return seg_len, status


def _jpeg_enc_frames(frames):
    import numpy as np
    f = np.ascontiguousarray(frames)
    if f.ndim == 3:
        f = f[None]
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3 or 0 in f.shape:
        raise ValueError(f"jpeg_encode: frames are uint8 [n, H, W, 3] (or one [H, W, 3]), got {f.dtype} {f.shape}")
    return f


def jpeg_encode_host(frames, quality=50, mode="420", form="bgr"):
    """`frames` uint8 [n, H, W, 3] (numpy) encoded by the CPU twin -> one ``bytes`` per frame, each the whole file
    (``jpeg_encode_ref``'s bytes)"""
    import numpy as np
    f = _jpeg_enc_frames(frames)
    n, H, W = f.shape[:3]
    cap = jpeg_encode_bound(H, W, mode)
    dst = np.empty(n * cap, dtype=np.uint8)
    seg_len, status = jpeg_encode_host_raw(f.reshape(-1), jpeg_enc_records(n, H, W, cap), dst, H, W, quality, mode, form)
    if status.any():
        raise RuntimeError(f"jpeg_encode_host: status {status.tolist()} with windows of the bound's size")
    head = jpeg_file_header(H, W, quality, mode)
    return [jpeg_assemble(head, dst[i * cap:i * cap + int(seg_len[i])]) for i in range(n)]


def _pil_jpeg_file(frame, quality, mode, form):
    """one frame through PIL: by the definition of the encode, the bytes the op's segment gives inside its header"""
    import io
    import numpy as np
    from PIL import Image
    rgb = np.ascontiguousarray(frame if form == "rgb" else frame[..., ::-1])
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=int(quality), subsampling=2 if mode == "420" else 0)
    return buf.getvalue()


class JpegHostEncoder:
    """``JpegEncoder``'s ``files`` on the CPU twin (no device): what ``compress_episode`` takes as ``encoder=`` in tests"""

    def __init__(self, H, W, max_frames=64, quality=50, mode="420"):
        _jpeg_enc_args(mode, quality=quality)
        self.device, self.H, self.W, self.max_frames, self.quality, self.mode = None, int(H), int(W), int(max_frames), int(quality), mode
        self.stats = {"frames": 0, "fallback": 0}

    def files(self, src, form="bgr"):
        f = _jpeg_enc_frames(src.numpy() if torch.is_tensor(src) else src)
        if f.shape[1:3] != (self.H, self.W):
            raise ValueError(f"JpegHostEncoder: frames {f.shape[1:3]}, the encoder is for {self.H} x {self.W}")
        self.stats["frames"] += len(f)
        return jpeg_encode_host(f, self.quality, self.mode, form)


class JpegEncoder:
    """The device state of ``jpeg_encode`` for frames of one size, quality and sampling mode: the workspace of ``max_frames`` slots,
    the records of the default layout (frames back to back in `src`, every segment in a window of ``cap`` bytes of `dst`; the
    default leaves half a raw frame and 4 KiB, ``cap=encoder.bound`` what no frame exceeds) and the file header.  ``encode``
    launches actmi_op_jpeg_encode for up to ``max_frames`` frames at a time on the current stream and reads nothing back;
    ``files`` reads lengths and statuses back once and returns one file per frame.  ``stats``: frames encoded by ``files``, and how
    many of them were re-encoded on the host because their status was not 0."""

    def __init__(self, device, H, W, max_frames=64, quality=50, mode="420", cap=None):
        _jpeg_enc_args(mode, quality=quality)
        self.device, self.H, self.W, self.max_frames = torch.device(device), int(H), int(W), int(max_frames)
        self.quality, self.mode = int(quality), mode
        if self.max_frames < 1 or self.max_frames > 65535:
            raise ValueError("JpegEncoder: max_frames must be in 1..65535")
        self.bound = jpeg_encode_bound(self.H, self.W, mode)
        if self.bound < 0:
            raise ValueError("JpegEncoder: H and W must be in 1..65535")
        self.frame_bytes = self.H * self.W * 3
        self.default_cap = min(self.bound, self.frame_bytes // 2 + 4096 if cap is None else int(cap))
        self.header = jpeg_file_header(self.H, self.W, quality, mode)
        self._q = jpeg_quant_tables(quality)
        self._ws = torch.empty(max(16, jpeg_encode_workspace_bytes(self.max_frames, self.H, self.W, mode)), dtype=torch.uint8, device=self.device)
        self._rec_cap, self._rec = None, None
        self.stats = {"frames": 0, "fallback": 0}

    def _records(self, n, cap):
        """the default layout's records on the device, kept for the largest n asked for with this cap"""
        if self._rec_cap != cap or self._rec.numel() < 32 * n:
            import numpy as np
            rec = jpeg_enc_records(max(n, self.max_frames), self.H, self.W, cap)
            self._rec, self._rec_cap = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(self.device), cap
        return self._rec

    def encode(self, src, dst=None, cap=None, form="bgr", records=None, marks=None, first=None, rows_per_mark=None):
        """src: contiguous uint8 tensor on the device, n frames [H, W, 3] back to back (``records`` None) -> (dst, seg_len, status):
        dst uint8 [n * cap] on the device (``cap`` defaults to ``default_cap``; a frame that needs more has status DEST), seg_len
        and status int32 [n] on the device.  ``records``: ``jpeg_enc_frame_dtype`` records (numpy) that place every frame in `src`
        and its window in the caller's `dst` instead.  ``marks`` (a contiguous, 8-byte aligned uint8 tensor of 32-byte
        ``jpeg_mark_dtype`` records on the device; it may be a view of `dst`'s buffer), ``first`` (int64 [n], numpy or on the device:
        the index of every frame's mark 0) and ``rows_per_mark``: actmi_op_jpeg_encode_marked instead, which also writes every
        frame's marks (status MARK for a frame whose marks would leave the tensor)."""
        import numpy as np
        _jpeg_enc_args(self.mode, form)
        if not torch.is_tensor(src) or src.dtype != torch.uint8 or src.device != self.device or not src.is_contiguous():
            raise ValueError(f"JpegEncoder: src must be a contiguous uint8 tensor on {self.device}")
        if records is None:
            if src.numel() % self.frame_bytes:
                raise ValueError(f"JpegEncoder: src holds {src.numel()} bytes, not whole frames of {self.H} x {self.W} x 3")
            n = src.numel() // self.frame_bytes
            cap = self.default_cap if cap is None else int(cap)
            if cap < 0 or cap > 0x7FFFFFFF:
                raise ValueError("JpegEncoder: cap must be in 0..2^31-1")
            if dst is None:
                dst = torch.empty(max(1, n * cap), dtype=torch.uint8, device=self.device)
            rec = self._records(n, cap)
        else:
            if dst is None:
                raise ValueError("JpegEncoder: records name windows in the caller's dst")
            rec = np.ascontiguousarray(records, dtype=jpeg_enc_frame_dtype())
            n = len(rec)
            rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(self.device)
        if dst.dtype != torch.uint8 or dst.device != self.device or not dst.is_contiguous():
            raise ValueError(f"JpegEncoder: dst must be a contiguous uint8 tensor on {self.device}")
        seg_len = torch.empty(n, dtype=torch.int32, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return dst, seg_len, status
        d = _jpeg_enc_desc(self.H, self.W, self.quality, self.mode, form, self._q)
        d.src, d.src_bytes, d.dst, d.dst_bytes = src.data_ptr(), int(src.numel()), dst.data_ptr(), int(dst.numel())
        d.ws, d.ws_bytes = self._ws.data_ptr(), int(self._ws.numel())
        lib = L.load()
        m = None
        if _jpeg_enc_marks("JpegEncoder", marks, first, rows_per_mark, n):
            if not torch.is_tensor(marks) or marks.dtype != torch.uint8 or marks.device != self.device or not marks.is_contiguous() or \
                    marks.numel() % 32 or marks.data_ptr() % 8:
                raise ValueError(f"JpegEncoder: marks must be a contiguous, 8-byte aligned uint8 tensor of 32-byte records on {self.device}")
            if not torch.is_tensor(first):
                first = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int64)).to(self.device)
            if first.dtype != torch.int64 or first.device != self.device or not first.is_contiguous() or first.numel() != n:
                raise ValueError(f"JpegEncoder: first must hold one int64 index per frame on {self.device}")
            m = L.JpegMarks()
            m.marks, m.n_marks, m.rows_per_mark = marks.data_ptr(), marks.numel() // 32, int(rows_per_mark)
        with torch.cuda.device(self.device):
            for i0 in range(0, n, self.max_frames):
                d.frames, d.seg_len, d.status = rec.data_ptr() + 32 * i0, seg_len.data_ptr() + 4 * i0, status.data_ptr() + 4 * i0
                d.n = min(self.max_frames, n - i0)
                if m is None:
                    L.check(lib.actmi_op_jpeg_encode(C.byref(d), L.current_stream_ptr()), None, "op_jpeg_encode")
                else:
                    m.first = first.data_ptr() + 8 * i0
                    L.check(lib.actmi_op_jpeg_encode_marked(C.byref(d), C.byref(m), L.current_stream_ptr()), None, "op_jpeg_encode_marked")
        return dst, seg_len, status

    def files(self, src, form="bgr"):
        """`src` as ``encode`` (or uint8 [n, H, W, 3]) -> one ``bytes`` per frame, the whole file.  The lengths and statuses are read
        back once, then the segments in one copy.  A frame with a nonzero status (its segment is longer than ``default_cap``) is
        re-encoded on the host with PIL, which by definition gives the same bytes, and counted in ``stats``."""
        dst, seg_len, status = self.encode(src, form=form)
        n, cap = seg_len.numel(), self.default_cap
        meta = torch.stack([seg_len, status]).cpu().numpy()
        lens, st = meta[0], meta[1]
        ok = [i for i in range(n) if st[i] == 0]
        segs = torch.cat([dst[i * cap:i * cap + int(lens[i])] for i in ok]).cpu().numpy() if ok else None
        out, pos, frames = [None] * n, 0, None
        for i in range(n):
            if st[i] == 0:
                out[i] = jpeg_assemble(self.header, segs[pos:pos + int(lens[i])])
                pos += int(lens[i])
            else:
                if frames is None:
                    frames = src.reshape(n, self.H, self.W, 3)
                out[i] = _pil_jpeg_file(frames[i].cpu().numpy(), self.quality, self.mode, form)
                self.stats["fallback"] += 1
        self.stats["frames"] += n
        return out


def jpeg_encode(frames, quality=50, mode="420", form="bgr", device=None, encoder=None):
    """actmi_op_jpeg_encode: `frames` uint8 [n, H, W, 3] (numpy, or a tensor on any device) encoded on the device -> one ``bytes`` per
    frame: the file PIL writes for it at this quality and subsampling (``jpeg_encode_ref``'s bytes)."""
    _jpeg_enc_args(mode, form, quality)
    if torch.is_tensor(frames):
        t = frames if frames.dim() == 4 else frames[None]
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or 0 in t.shape:
            raise ValueError(f"jpeg_encode: frames are uint8 [n, H, W, 3], got {t.dtype} {tuple(t.shape)}")
    else:
        t = torch.from_numpy(_jpeg_enc_frames(frames))
    n, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    if encoder is None:
        if device is None:
            device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        encoder = JpegEncoder(device, H, W, max_frames=min(n, 64), quality=quality, mode=mode)
    elif (encoder.H, encoder.W, encoder.quality, encoder.mode) != (H, W, int(quality), mode):
        raise ValueError(f"jpeg_encode: the encoder is for {encoder.H} x {encoder.W} frames at quality {encoder.quality}, mode {encoder.mode}")
    if encoder.device is None:                                    # the host twin
        return encoder.files(t, form)
    return encoder.files(t.to(encoder.device).contiguous(), form)


# ---- packed depth: lossless uint16 frames (actmi_op_depth_pack / actmi_op_depth_unpack; the format is defined in actmi.h) ------------
DEPTH_PACK_STATUS = {0: "ok", 1: "row table out of order, unaligned or outside the stream", 2: "invalid group header or mask byte",
                     3: "row length differs from what its headers imply", 4: "destination extent leaves the buffer"}
DEPTH_FLIP = 1


def depth_pack_bound(H, W):
    """actmi_depth_pack_bound in numpy's terms: bytes no stream of an H x W frame exceeds"""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("depth_pack: H and W must be in 1..65535")
    return 4 * (H + 1) + H * (2 * ((W + 7) // 8) + 2 * W + 3)


def _depth_frame(frame):
    import numpy as np
    f = np.asarray(frame)
    if f.dtype != np.uint16 or f.ndim != 2 or 0 in f.shape:
        raise ValueError(f"depth_pack: a frame is uint16 [H, W], got {f.dtype} {f.shape}")
    return f


def depth_pack_row_ref(row):
    """one row of ``depth_pack_ref``: headers, mask bytes, payloads, zero bytes up to a multiple of 4"""
    import numpy as np
    x = np.asarray(row, dtype=np.int64)
    W = len(x)
    valid = x != 0
    xv = x[valid]
    d = (xv - np.concatenate([[0], xv[:-1]])) & 0xFFFF             # the chain over the row's valid pixels, prev starts at 0
    d = np.where(d >= 0x8000, d - 0x10000, d)                      # int16
    zv = ((d << 1) ^ (d >> 15)) & 0xFFFF
    z = np.zeros(W, dtype=np.int64)
    z[valid] = zv
    heads, masks, pays = bytearray(), bytearray(), bytearray()
    for g0 in range(0, W, 8):
        v, zz = valid[g0:g0 + 8], z[g0:g0 + 8]
        zs = [int(t) for t in zz[v]]
        w = max(zs).bit_length() if zs else 0
        flagged = not v.all()
        heads.append(w | (0x80 if flagged else 0))
        if flagged:
            masks.append(sum(1 << i for i in range(len(v)) if v[i]))
        acc = 0
        for j, t in enumerate(zs):
            acc |= t << (j * w)
        pays += acc.to_bytes((len(zs) * w + 7) // 8, "little")
    out = bytes(heads) + bytes(masks) + bytes(pays)
    return out + b"\0" * (-len(out) % 4)


def depth_pack_ref(frame):
    """The packed-depth stream of one uint16 [H, W] frame, stated in numpy: the definition actmi_op_depth_pack and
    actmi_depth_pack_host are compared with byte for byte."""
    import numpy as np
    f = _depth_frame(frame)
    H = f.shape[0]
    rows = [depth_pack_row_ref(f[r]) for r in range(H)]
    off = np.cumsum([4 * (H + 1)] + [len(r) for r in rows]).astype("<u4")
    return off.tobytes() + b"".join(rows)


def depth_unpack_ref(buf, H, W, flip=False):
    """``depth_pack_ref`` undone, with actmi_op_depth_unpack's checks -> (frame uint16 [H, W], status).  A row that fails a check is
    zeros; the status is the smallest nonzero one of the rows' (``DEPTH_PACK_STATUS``).  ``flip``: every row mirrored."""
    import numpy as np
    H, W = int(H), int(W)
    s = bytes(buf)
    L_, ng, table = len(s), (W + 7) // 8, 4 * (H + 1)
    out = np.zeros((H, W), dtype=np.uint16)
    if L_ < table + 4 or L_ > 0x7FFFFFFF:
        return out, 1
    off = np.frombuffer(s, dtype="<u4", count=H + 1).astype(np.int64)
    if off[H] != L_:
        return out, 1
    codes = set()
    for r in range(H):
        a, b = int(off[r]), int(off[r + 1])
        if a % 4 or b % 4 or a < table or not a < b or b > L_:
            codes.add(1)
            continue
        at = lambda i: s[min(max(i, 0), L_ - 1)]                  # the kernels' clamped read  # noqa: E731
        heads = [at(a + g) for g in range(ng)]
        ns = [min(8, W - 8 * g) for g in range(ng)]
        bad = any((h & 0x60) or (h & 0x1F) > 16 for h in heads)
        masks, mpos = [], a + ng
        for g, h in enumerate(heads):
            if h & 0x80:
                masks.append(at(mpos))
                bad = bad or masks[-1] >> ns[g] != 0
                mpos += 1
            else:
                masks.append((1 << ns[g]) - 1)
        if bad:
            codes.add(2)
            continue
        pbs = [(bin(m).count("1") * (h & 0x1F) + 7) // 8 for m, h in zip(masks, heads)]
        if (ng + (mpos - a - ng) + sum(pbs) + 3) // 4 * 4 != b - a:
            codes.add(3)
            continue
        prev, ppos = 0, mpos
        for g, (h, m, pb) in enumerate(zip(heads, masks, pbs)):
            w = h & 0x1F
            acc = int.from_bytes(s[ppos:ppos + pb], "little")
            ppos += pb
            j = 0
            for i in range(ns[g]):
                if m >> i & 1:
                    z = (acc >> (j * w)) & ((1 << w) - 1)
                    prev = (prev + ((z >> 1) ^ -(z & 1))) & 0xFFFF
                    out[r, 8 * g + i] = prev
                    j += 1
    return (out[:, ::-1].copy() if flip else out), min(codes, default=0)


def depth_pack_frame_dtype():
    """actmi_depth_pack_frame as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("src_off", np.int64), ("dst_off", np.int64), ("dst_cap", np.int32), ("reserved", np.int32, 3)])


def depth_unpack_frame_dtype():
    """actmi_depth_unpack_frame as a numpy structured dtype (32 bytes)"""
    import numpy as np
    return np.dtype([("seg_off", np.int64), ("dst_off", np.int64), ("seg_len", np.int32), ("flags", np.int32), ("reserved", np.int32, 2)])


def depth_pack_workspace_bytes(n, H):
    return int(L.load().actmi_op_depth_pack_workspace_bytes(int(n), int(H)))


def depth_pack_records(n, H, W, cap, src_off=None, dst_off=None):
    """the records of n frames laid back to back in `src`, every stream in a window of `cap` bytes (or at the offsets given)"""
    import numpy as np
    rec = np.zeros(int(n), dtype=depth_pack_frame_dtype())
    rec["src_off"] = np.arange(n, dtype=np.int64) * (2 * int(H) * int(W)) if src_off is None else np.asarray(src_off, dtype=np.int64)
    rec["dst_off"] = np.arange(n, dtype=np.int64) * int(cap) if dst_off is None else np.asarray(dst_off, dtype=np.int64)
    rec["dst_cap"] = cap
    return rec


def depth_unpack_records(seg_off, seg_len, H, W, dst_off=None, flags=0):
    """the records of the frames whose streams lie at `seg_off` / `seg_len`, decoded back to back into `dst` (or at the offsets given)"""
    import numpy as np
    n = len(seg_off)
    rec = np.zeros(n, dtype=depth_unpack_frame_dtype())
    rec["seg_off"], rec["seg_len"], rec["flags"] = seg_off, seg_len, flags
    rec["dst_off"] = np.arange(n, dtype=np.int64) * (2 * int(H) * int(W)) if dst_off is None else np.asarray(dst_off, dtype=np.int64)
    return rec


def _depth_host_array(what, name, a):
    import numpy as np
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError(f"{what}: {name} must be a contiguous 1-D uint8 array")
    return a


def depth_pack_host_raw(src, records, dst, H, W):
    """actmi_depth_pack_host, the CPU twin of ``DepthPacker.pack`` (the same core, no device) on the caller's buffers: `src` (2-byte
    aligned) and `dst` contiguous 1-D uint8 arrays, `records` ``depth_pack_frame_dtype`` -> (seg_len, status), int32 [n] each"""
    import numpy as np
    _depth_host_array("depth_pack_host", "src", src), _depth_host_array("depth_pack_host", "dst", dst)
    rec = np.ascontiguousarray(records, dtype=depth_pack_frame_dtype())
    n = len(rec)
    seg_len, status = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    d = L.DepthPackDesc()
    one = np.zeros(1, dtype=np.uint8)                             # an empty array still has to name memory
    d.src, d.src_bytes, d.frames = (src if src.size else one).ctypes.data, src.size, rec.ctypes.data
    d.dst, d.dst_bytes = (dst if dst.size else one).ctypes.data, dst.size
    d.seg_len, d.status, d.n, d.H, d.W = seg_len.ctypes.data, status.ctypes.data, n, int(H), int(W)
    L.check(L.load().actmi_depth_pack_host(C.byref(d)), None, "depth_pack_host")
    return seg_len, status


def depth_unpack_host_raw(stream, records, dst, H, W, sticky=None):
    """actmi_depth_unpack_host on the caller's buffers: `stream` and `dst` (2-byte aligned) contiguous 1-D uint8 arrays, `records`
    ``depth_unpack_frame_dtype`` -> status int32 [n].  ``sticky``: an int32 [1] array that receives the largest status."""
    import numpy as np
    _depth_host_array("depth_unpack_host", "stream", stream), _depth_host_array("depth_unpack_host", "dst", dst)
    rec = np.ascontiguousarray(records, dtype=depth_unpack_frame_dtype())
    n = len(rec)
    status = np.full(n, -1, dtype=np.int32)
    d = L.DepthUnpackDesc()
    one = np.zeros(2, dtype=np.uint8)
    d.stream, d.stream_bytes, d.frames = (stream if stream.size else one).ctypes.data, stream.size, rec.ctypes.data
    d.dst, d.dst_bytes = (dst if dst.size else one).ctypes.data, dst.size
    d.status, d.sticky, d.n, d.H, d.W = status.ctypes.data, None if sticky is None else sticky.ctypes.data, n, int(H), int(W)
    L.check(L.load().actmi_depth_unpack_host(C.byref(d)), None, "depth_unpack_host")
    return status


def _depth_frames(frames):
    import numpy as np
    f = np.ascontiguousarray(frames)
    if f.ndim == 2:
        f = f[None]
    if f.dtype != np.uint16 or f.ndim != 3 or 0 in f.shape:
        raise ValueError(f"depth_pack: frames are uint16 [n, H, W] (or one [H, W]), got {f.dtype} {f.shape}")
    return f


def depth_pack_host(frames):
    """`frames` uint16 [n, H, W] (numpy) packed by the CPU twin -> one ``bytes`` per frame (``depth_pack_ref``'s bytes)"""
    import numpy as np
    f = _depth_frames(frames)
    n, H, W = f.shape
    cap = depth_pack_bound(H, W)
    dst = np.empty(n * cap, dtype=np.uint8)
    seg_len, status = depth_pack_host_raw(f.reshape(-1).view(np.uint8), depth_pack_records(n, H, W, cap), dst, H, W)
    if status.any():
        raise RuntimeError(f"depth_pack_host: status {status.tolist()} with windows of the bound's size")
    return [dst[i * cap:i * cap + int(seg_len[i])].tobytes() for i in range(n)]


def depth_unpack_host(bufs, H, W, flip=False):
    """streams (one ``bytes`` per frame) decoded by the CPU twin -> (frames uint16 [n, H, W], status int32 [n])"""
    import numpy as np
    lens = np.array([len(b) for b in bufs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(bufs) else lens
    stream = np.frombuffer(b"".join(bytes(b) for b in bufs), dtype=np.uint8).copy()
    out = np.full((len(bufs), int(H), int(W)), 0xABCD, dtype=np.uint16)
    status = depth_unpack_host_raw(stream, depth_unpack_records(offs, lens, H, W, flags=DEPTH_FLIP if flip else 0),
                                   out.reshape(-1).view(np.uint8), H, W)
    return out, status


def _depth_dev_tensor(what, name, t, device):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.device != device or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous uint8 tensor on {device}")
    return t


def _records_to(rec, dtype, device):
    import numpy as np
    rec = np.ascontiguousarray(rec, dtype=dtype)
    return len(rec), torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(device)


class DepthPacker:
    """The device state of ``depth_pack`` for frames of one size: the workspace of ``max_frames`` slots and the length and status
    buffers of the last launch, as ``JpegEncoder`` holds them.  ``pack`` launches actmi_op_depth_pack for up to ``max_frames``
    frames at a time on the current stream and reads nothing back; ``sizes`` is the launch with empty windows, read back."""

    def __init__(self, device, H, W, max_frames=64):
        self.device, self.H, self.W, self.max_frames = torch.device(device), int(H), int(W), int(max_frames)
        if self.max_frames < 1 or self.max_frames > 65535:
            raise ValueError("DepthPacker: max_frames must be in 1..65535")
        self.bound = int(L.load().actmi_depth_pack_bound(self.H, self.W))
        if self.bound < 0:
            raise ValueError("DepthPacker: H and W must be in 1..65535 and the bound must fit int32")
        self.frame_bytes = 2 * self.H * self.W
        self._ws = torch.empty(max(4, depth_pack_workspace_bytes(self.max_frames, self.H)), dtype=torch.uint8, device=self.device)
        self._one = torch.zeros(16, dtype=torch.uint8, device=self.device)   # what an empty dst names

    def pack(self, src, records, dst):
        """src: contiguous uint8 tensor on the device that holds the uint16 pixels; records: ``depth_pack_frame_dtype`` (numpy) that
        place every frame in `src` and its window in `dst` -> (seg_len, status), int32 [n] on the device"""
        _depth_dev_tensor("DepthPacker", "src", src, self.device), _depth_dev_tensor("DepthPacker", "dst", dst, self.device)
        n, rec = _records_to(records, depth_pack_frame_dtype(), self.device)
        seg_len = torch.empty(n, dtype=torch.int32, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        if n == 0:
            return seg_len, status
        d = L.DepthPackDesc()
        d.src, d.src_bytes = (src if src.numel() else self._one).data_ptr(), int(src.numel())
        d.dst, d.dst_bytes = (dst if dst.numel() else self._one).data_ptr(), int(dst.numel())
        d.ws, d.ws_bytes, d.H, d.W = self._ws.data_ptr(), int(self._ws.numel()), self.H, self.W
        lib = L.load()
        with torch.cuda.device(self.device):
            for i0 in range(0, n, self.max_frames):
                d.frames, d.seg_len, d.status = rec.data_ptr() + 32 * i0, seg_len.data_ptr() + 4 * i0, status.data_ptr() + 4 * i0
                d.n = min(self.max_frames, n - i0)
                L.check(lib.actmi_op_depth_pack(C.byref(d), L.current_stream_ptr()), None, "op_depth_pack")
        return seg_len, status

    def sizes(self, src, n=None, src_off=None):
        """the true stream lengths of the frames in `src` (back to back, or at ``src_off``), by a launch with empty windows -> int64
        numpy [n]; a frame whose pixels leave `src` raises"""
        import numpy as np
        if src_off is None:
            n = src.numel() // self.frame_bytes if n is None else int(n)
        else:
            n = len(src_off)
        rec = depth_pack_records(n, self.H, self.W, 0, src_off=src_off, dst_off=np.zeros(n, dtype=np.int64))
        seg_len, _ = self.pack(src, rec, self._one[:0])
        lens = seg_len.cpu().numpy().astype(np.int64)
        if n and lens.min() <= 0:
            raise RuntimeError("DepthPacker: a frame's pixels leave src")
        return lens


def depth_pack(frames, device=None, packer=None):
    """actmi_op_depth_pack: `frames` uint16 [n, H, W] (numpy, or a tensor on any device) packed on the device -> one ``bytes`` per
    frame (``depth_pack_ref``'s bytes): one launch with empty windows for the lengths, one with exact windows."""
    import numpy as np
    t = frames if torch.is_tensor(frames) else torch.from_numpy(_depth_frames(frames))
    t = t if t.dim() == 3 else t[None]
    if t.dtype != torch.uint16 or t.dim() != 3 or 0 in t.shape:
        raise ValueError(f"depth_pack: frames are uint16 [n, H, W], got {t.dtype} {tuple(t.shape)}")
    n, H, W = (int(v) for v in t.shape)
    if packer is None:
        if device is None:
            device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        packer = DepthPacker(device, H, W, max_frames=min(n, 256))
    elif (packer.H, packer.W) != (H, W):
        raise ValueError(f"depth_pack: the packer is for {packer.H} x {packer.W} frames")
    src = t.to(packer.device).contiguous().view(torch.uint8).reshape(-1)
    lens = packer.sizes(src, n)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    dst = torch.empty(int(lens.sum()), dtype=torch.uint8, device=packer.device)
    rec = depth_pack_records(n, H, W, 0, dst_off=offs)
    rec["dst_cap"] = lens
    _, status = packer.pack(src, rec, dst)
    if bool(status.any()):
        raise RuntimeError(f"depth_pack: status {status.tolist()} with exact windows")
    out = dst.cpu().numpy()
    return [out[o:o + ln].tobytes() for o, ln in zip(offs, lens)]


def depth_unpack_raw(stream, records, dst, H, W, sticky=None, status=None):
    """actmi_op_depth_unpack on the caller's tensors: `stream` and `dst` contiguous uint8 tensors on one device, `records`
    ``depth_unpack_frame_dtype`` (numpy), or a uint8 tensor of them already on the device -> status int32 [n] on the device.
    ``sticky``: an int32 [1] tensor on the device that receives the largest status of the launch."""
    dev = stream.device
    _depth_dev_tensor("depth_unpack", "stream", stream, dev), _depth_dev_tensor("depth_unpack", "dst", dst, dev)
    if torch.is_tensor(records):
        _depth_dev_tensor("depth_unpack", "records", records, dev)
        n, rec = records.numel() // 32, records
    else:
        n, rec = _records_to(records, depth_unpack_frame_dtype(), dev)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return status
    if n > 65535:
        raise ValueError("depth_unpack: at most 65535 frames a launch")
    d = L.DepthUnpackDesc()
    d.stream, d.stream_bytes, d.frames = stream.data_ptr(), int(stream.numel()), rec.data_ptr()
    d.dst, d.dst_bytes, d.status = dst.data_ptr(), int(dst.numel()), status.data_ptr()
    d.sticky, d.n, d.H, d.W = None if sticky is None else sticky.data_ptr(), n, int(H), int(W)
    with torch.cuda.device(dev):
        L.check(L.load().actmi_op_depth_unpack(C.byref(d), L.current_stream_ptr()), None, "op_depth_unpack")
    return status


def depth_unpack(bufs, H, W, flip=False, device=None):
    """actmi_op_depth_unpack: streams (one ``bytes`` per frame) decoded on the device -> (frames uint16 [n, H, W] tensor on the
    device, status int32 [n] numpy)"""
    import numpy as np
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lens = np.array([len(b) for b in bufs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(bufs) else lens
    stream = torch.from_numpy(np.frombuffer(b"".join(bytes(b) for b in bufs) or b"\0", dtype=np.uint8).copy()).to(device)
    out = torch.empty((len(bufs), int(H), int(W)), dtype=torch.uint16, device=device)
    status = depth_unpack_raw(stream, depth_unpack_records(offs, lens, H, W, flags=DEPTH_FLIP if flip else 0),
                              out.view(torch.uint8).reshape(-1), H, W)
    return out, status.cpu().numpy()
