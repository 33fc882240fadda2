"""Kernel-level parity of the launch forms of the convolution stem (conv1.hip) and of the pooling kernels (pool.hip) that no
other kernel test reaches, against torch float64 on the CPU.

a. u8 frames whose byte count is no multiple of 4 (the loader's tail word; the last pixel of every image is 255 so that a
   dropped byte shows), one of them starting one byte into its allocation;
b. Cout % 4 != 0: the scalar store epilogue of both stem kernels;
c. one-pixel, 63 / 64 / 65 / 129-pixel output rows, frames shorter than the filter, an odd Ho under the f16x3 row pair;
d. the prepared stem (conv1_prepare + conv1_prepared): bit-equal to ops.conv1 f16x3 on the same operands, and its lut_mode 1 /
   no-ReLU / no scale and bias form against float64;
e. the fused vertical pool (vpool) with an empty last row segment, a one-pair segment behind a halo step, a partial second
   strip, Cout below one quad block, an odd-byte frame and f32 input: bit-equal to the max over conv rows (2a-1, 2a, 2a+1) of
   the plain output, and hpool(vpool) bit-equal to maxpool3x3s2(plain) and to F.max_pool2d; the launcher's rejections;
f. a camera range (cam0, ncam), plain and vpool, into a sentinel-filled whole tensor;
g. hpool on rows full of ties and negative values, bit-equal to F.max_pool2d (1, 3) / (1, 2) / (0, 1), a case that makes the
   grid-stride loop take a second pass, C % 4 != 0 rejected, zero rows a no-op;
i. u8_to_nhwc4, bit-equal to (v / 255 in float64) rounded to fp32, fourth channel exactly 0.
(h, the max-pool shapes, extends test_maxpool_bit_exact in test_gpu_kernels.py and POOL_CASES in test_gpu_train_kernels.py.)

Bound: the project's stem bound, max |got - float64| <= 2e-6 of the result's largest magnitude (K = 147 fp32 / split-fp16
products accumulated in fp32; test_conv1_u8_and_f32, test_conv1_depth_matches_float64_convolution).  The reference takes the
loader's fp32 normalised pixels as its input, as those tests do.  "Bitwise" is torch.equal.  Every case prints its worst
error with the bound.

Worst errors measured on an MI355X (bound 2e-6): a. 6.8e-7 (fp32 kernel, 30 x 43), 3.0e-7 f16x3; b. 4.0e-7; c. 4.0e-7;
d. 3.5e-7 prepared, 3.7e-7 without normalisation / ReLU; e. / f. plain outputs 3.9e-7, everything else bit-equal.  With the
tail word rounded down to a multiple of 4 (the loader before conv1_loader.h's tail-word rule) all ten cases of (a) fail in both kernels: u8
against float64 9.5e-2 (7 x 9), 1.4e-1 (30 x 43), 2.3e-1 (13 x 17), 7.2e-2 (35 x 150), every time in the bottom-right corner,
with the f32 input form unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402

BOUND = 2e-6
PRECS = ["f32", "f16x3"]
MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
SENTINEL = 0x7FC12345                                              # a NaN payload: any write shows


def dev():
    return torch.device("cuda:0")


def _err(got, exp):
    """max |got - exp| relative to the largest magnitude of the WHOLE expected tensor `exp[0]` (so that a part of the output
    is judged on the scale of the output): exp = (whole, part) or a tensor"""
    whole, part = exp if isinstance(exp, tuple) else (exp, exp)
    return float((got.detach().cpu().double() - part).abs().max() / (whole.abs().max() + 1e-30))


@functools.lru_cache(maxsize=None)
def _case(B, Cn, H, W, Cout, seed, last_255=False):
    """operands of one stem case and its float64 results: ImageNet-normalised with FrozenBN + ReLU (`exp`), and x / 255 with
    neither scale, bias nor ReLU (`exp_raw`); both [C][B][Ho][Wo][Cout]"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, Cn, H, W, 3), dtype=torch.uint8, generator=g)
    if last_255:
        img[:, :, -1, -1, :] = 255
    w = torch.randn(Cn, Cout, 3, 7, 7, generator=g) / 147 ** 0.5
    scale, bias = torch.rand(Cn, Cout, generator=g) + 0.5, torch.randn(Cn, Cout, generator=g) * 0.1
    x = torch.from_numpy(np.moveaxis(img.numpy(), -1, -3) / 255.0).float()           # get_image contract: f32 [B][C][3][H][W]
    xn = ((x - MEAN) / STD).double()                                                   # the loader's fp32 normalised pixels
    conv = lambda inp, c: F.conv2d(inp[:, c], w[c].double(), None, 2, 3)               # noqa: E731
    exp = torch.stack([torch.relu(conv(xn, c) * scale[c].double().view(1, -1, 1, 1) + bias[c].double().view(1, -1, 1, 1))
                       for c in range(Cn)]).permute(0, 1, 3, 4, 2).contiguous()
    exp_raw = torch.stack([conv(x.double(), c) for c in range(Cn)]).permute(0, 1, 3, 4, 2).contiguous()
    return dict(img=img, x=x, w=w, scale=scale, bias=bias, exp=exp, exp_raw=exp_raw)


def _check_plain(tag, B, Cn, H, W, Cout, prec, seed, last_255=False, image_dev=None):
    """ops.conv1 on u8 and on f32 input against float64, the two bit-equal, the bottom-right 4 x 4 corner on its own"""
    c = _case(B, Cn, H, W, Cout, seed, last_255)
    d = dev()
    w, scale, bias = c["w"].to(d), c["scale"].to(d), c["bias"].to(d)
    got_u8 = ops.conv1(c["img"].to(d) if image_dev is None else image_dev, w, scale, bias, prec=prec).cpu()
    got_f32 = ops.conv1(c["x"].to(d), w, scale, bias, prec=prec).cpu()
    exp = c["exp"]
    assert got_u8.shape == exp.shape
    corner = (Ellipsis, slice(-4, None), slice(-4, None), slice(None))
    e_u8, e_f32 = _err(got_u8, exp), _err(got_f32, exp)
    e_corner = _err(got_u8[corner], (exp, exp[corner]))
    print(f"{tag} {B}x{Cn}x{H}x{W} Cout {Cout} {prec}: u8 {e_u8:.2e}, f32 {e_f32:.2e}, u8 bottom-right corner {e_corner:.2e} "
          f"(bound {BOUND:.0e}); u8 == f32 bitwise: {torch.equal(got_u8, got_f32)}")
    assert e_corner <= BOUND, f"bottom-right 4x4 output corner of the u8 form: {e_corner:.3e}"
    assert e_u8 <= BOUND, e_u8
    assert e_f32 <= BOUND, e_f32
    assert torch.equal(got_u8, got_f32)          # LUT path == arithmetic path, bit for bit


# ---- a. u8 frames of 4m + 1, 2, 3 bytes ------------------------------------------------------------------------------------
ODD_FRAMES = [(2, 2, 7, 9, 8), (3, 1, 30, 43, 8), (2, 3, 13, 17, 64), (1, 1, 35, 150, 8)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,Cn,H,W,Cout", ODD_FRAMES)
def test_u8_frames_whose_byte_count_is_no_multiple_of_4(B, Cn, H, W, Cout, prec):
    assert (H * W * 3) % 4 != 0
    _check_plain("a.", B, Cn, H, W, Cout, prec, seed=1000 * H + W, last_255=True)


@pytest.mark.parametrize("prec", PRECS)
def test_u8_batch_that_starts_one_byte_into_its_allocation(prec):
    """host feeds may hand the engine any pointer: the loader's words are aligned relative to the image, not to memory"""
    B, Cn, H, W, Cout = 2, 2, 7, 9, 8
    c = _case(B, Cn, H, W, Cout, 1000 * H + W, True)
    n = c["img"].numel()
    big = torch.full((n + 9,), 77, dtype=torch.uint8, device=dev())
    big[1:1 + n] = c["img"].to(dev()).view(-1)
    view = big[1:1 + n].view(B, Cn, H, W, 3)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    _check_plain("a. (offset 1)", B, Cn, H, W, Cout, prec, seed=1000 * H + W, last_255=True, image_dev=view)


def test_u8_frame_below_four_bytes_is_rejected_and_f32_1x1_runs():
    """the smallest u8 frame the loader can fetch without leaving the image is 4 bytes: 1 x 1 (3 bytes) is refused with a
    message by both entries; the f32 form has no such limit"""
    d = dev()
    c = _case(2, 1, 1, 1, 8, 11)
    w, scale, bias = c["w"].to(d), c["scale"].to(d), c["bias"].to(d)
    for prec in PRECS:
        with pytest.raises(RuntimeError, match=r"code -2.*at least 4 bytes"):
            ops.conv1(c["img"].to(d), w, scale, bias, prec=prec)
        e = _err(ops.conv1(c["x"].to(d), w, scale, bias, prec=prec), c["exp"])
        print(f"a. 1x1 f32 frame {prec}: {e:.2e} (bound {BOUND:.0e})")
        assert e <= BOUND
    ws = ops.conv1_prepare(w, lut_mode=0)
    with pytest.raises(RuntimeError, match=r"code -2.*at least 4 bytes"):
        ops.conv1_prepared(c["img"].to(d), ws, 8, relu=True)
    # 1 x 2 = 6 bytes is the smallest frame above the limit
    _check_plain("a. (6 bytes)", 2, 1, 1, 2, 8, "f16x3", seed=12, last_255=True)
    _check_plain("a. (6 bytes)", 2, 1, 1, 2, 8, "f32", seed=12, last_255=True)


# ---- b. scalar epilogue, c. row and column edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cout", [3, 6, 33, 62])
def test_cout_not_a_multiple_of_4(Cout, prec):
    _check_plain("b.", 2, 2, 14, 22, Cout, prec, seed=500 + Cout)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H,W", [(6, 2), (6, 126), (6, 128), (6, 130), (6, 258), (1, 40), (2, 40), (3, 40), (10, 40)])
def test_row_and_column_edges(H, W, prec):
    _check_plain("c.", 2, 2, H, W, 8, prec, seed=2000 * H + W)


# ---- d. prepared stem ----------------------------------------------------------------------------------------------------------
PREPARED = [(2, 2, 30, 43, 64), (1, 1, 64, 96, 8)]


@pytest.mark.parametrize("B,Cn,H,W,Cout", PREPARED)
def test_prepared_stem_is_bit_equal_to_conv1_f16x3(B, Cn, H, W, Cout):
    """the weight image built once by conv1_wimg_kernel and the split made in the kernel's prologue are the same entries"""
    c = _case(B, Cn, H, W, Cout, 3000 + H, True)
    d = dev()
    img, w, scale, bias = c["img"].to(d), c["w"].to(d), c["scale"].to(d), c["bias"].to(d)
    ws = ops.conv1_prepare(w, lut_mode=0)
    got = ops.conv1_prepared(img, ws, Cout, relu=True, scale=scale, bias=bias)
    ref = ops.conv1(img, w, scale, bias, prec="f16x3")
    e = _err(got, c["exp"])
    print(f"d. prepared {B}x{Cn}x{H}x{W} Cout {Cout}: {e:.2e} (bound {BOUND:.0e}); == conv1 f16x3 bitwise: {torch.equal(got, ref)}")
    assert e <= BOUND
    assert torch.equal(got, ref)
    got_f32in = ops.conv1_prepared(c["x"].to(d), ws, Cout, relu=True, scale=scale, bias=bias)
    assert torch.equal(got_f32in, ref)           # the f32 input form of the entry


@pytest.mark.parametrize("B,Cn,H,W,Cout", PREPARED)
def test_prepared_stem_without_normalisation_relu_scale_or_bias(B, Cn, H, W, Cout):
    """what the diffusion policy runs: lut_mode 1 (x / 255), relu_floor -inf, the workspace's unit scale and zero bias"""
    c = _case(B, Cn, H, W, Cout, 3000 + H, True)
    exp = c["exp_raw"]
    share = float((exp < 0).double().mean())
    assert share >= 0.25, share                  # the missing ReLU is exercised
    d = dev()
    ws = ops.conv1_prepare(c["w"].to(d), lut_mode=1)
    got = ops.conv1_prepared(c["img"].to(d), ws, Cout, relu=False, scale=None, bias=None)
    e = _err(got, exp)
    print(f"d. prepared raw {B}x{Cn}x{H}x{W} Cout {Cout}: {e:.2e} (bound {BOUND:.0e}), {share:.2f} of the outputs negative")
    assert e <= BOUND
    assert float((got < 0).double().mean()) >= 0.25


# ---- e. fused vertical pool ----------------------------------------------------------------------------------------------------
VPOOL = [(1, 1, 164, 40, 8, "u8"),       # 41 row pairs in 10 segments of 5: the last segment empty, the one before a single pair + halo
         (1, 2, 36, 150, 64, "u8"),      # 9 row pairs in 2 segments, a second strip of 11 columns
         (3, 2, 20, 40, 4, "u8"),        # one segment, Cout below one quad block
         (1, 1, 35, 43, 8, "u8"),        # 4515 bytes per frame, Ho = 18
         (1, 2, 36, 150, 64, "f32")]


def _prepared_pair(B, Cn, H, W, Cout, src, seed):
    c = _case(B, Cn, H, W, Cout, seed, True)
    d = dev()
    image = (c["img"] if src == "u8" else c["x"]).to(d)
    ws = ops.conv1_prepare(c["w"].to(d), lut_mode=0)
    args = dict(relu=True, scale=c["scale"].to(d), bias=c["bias"].to(d))
    return c, image, ws, args


@pytest.mark.parametrize("B,Cn,H,W,Cout,src", VPOOL)
def test_fused_vertical_pool(B, Cn, H, W, Cout, src):
    c, image, ws, args = _prepared_pair(B, Cn, H, W, Cout, src, 4000 + H)
    plain = ops.conv1_prepared(image, ws, Cout, **args)
    e = _err(plain, c["exp"])
    vp = ops.conv1_prepared(image, ws, Cout, vpool=True, **args)
    Ho, Wo = plain.shape[2], plain.shape[3]
    assert Ho % 2 == 0 and vp.shape == (Cn, B, Ho // 2, Wo, Cout)
    p_nchw = plain.cpu().view(Cn * B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    exp_v = F.max_pool2d(p_nchw, (3, 1), (2, 1), (1, 0)).permute(0, 2, 3, 1)              # rows 2a-1, 2a, 2a+1; outside rows skipped
    exp_p = F.max_pool2d(p_nchw, 3, 2, 1).permute(0, 2, 3, 1)
    got_v = vp.cpu().view(Cn * B, Ho // 2, Wo, Cout)
    got_hp = ops.hpool(vp.view(Cn * B, Ho // 2, Wo, Cout)).cpu()
    got_mp = ops.maxpool3x3s2(plain.view(Cn * B, Ho, Wo, Cout)).cpu()
    ok = (torch.equal(got_v, exp_v), torch.equal(got_hp, got_mp), torch.equal(got_hp, exp_p), torch.equal(got_mp, exp_p))
    print(f"e. vpool {B}x{Cn}x{H}x{W} Cout {Cout} {src}: plain {e:.2e} (bound {BOUND:.0e}); bitwise vpool == row max: {ok[0]}, "
          f"hpool(vpool) == maxpool(plain): {ok[1]}, == F.max_pool2d: {ok[2]} / {ok[3]}; "
          f"vpool rows that differ: {sorted(set(torch.nonzero((got_v != exp_v).any(3).any(2))[:, 1].tolist()))[:12]}")
    assert e <= BOUND
    assert ok[0], "vpool output != max over conv rows (2a-1, 2a, 2a+1) of the plain output"
    assert ok[1], "hpool(vpool output) != maxpool3x3s2(plain output)"
    assert ok[2] and ok[3], "pool outputs != F.max_pool2d(plain, 3, 2, 1)"


def test_fused_vertical_pool_rejections():
    d = dev()
    for (H, Cout, kw, msg) in [(70, 8, {}, "even output height"),                    # Ho = 35
                               (36, 6, {}, "Cout % 4 == 0"),
                               (36, 8, dict(prec="f32"), "vpool needs prec f16x3")]:
        c, image, ws, args = _prepared_pair(1, 1, H, 40, Cout, "u8", 4100 + H)
        with pytest.raises(RuntimeError, match=r"code -2") as e:
            ops.conv1_prepared(image, ws, Cout, vpool=True, **args, **kw)
        assert msg in str(e.value), str(e.value)
    c, image, ws, args = _prepared_pair(1, 1, 36, 40, 8, "u8", 4136)
    with pytest.raises(RuntimeError, match=r"code -2.*without ReLU"):
        ops.conv1_prepared(image, ws, 8, vpool=True, relu=False)
    with pytest.raises(RuntimeError, match=r"code -2.*without ReLU"):
        ops.conv1_prepared(image, ws, 8, relu=False, prec="f32")
    # the plain fp32 form of the entry does run, and is the fp32 kernel of ops.conv1
    got = ops.conv1_prepared(image, ws, 8, prec="f32", **args)
    assert torch.equal(got, ops.conv1(image, c["w"].to(d), args["scale"], args["bias"], prec="f32"))
    torch.cuda.synchronize()


# ---- f. camera range -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vpool", [False, True])
def test_camera_range_writes_its_cameras_only(vpool):
    B, Cn, H, W, Cout = 2, 3, 20, 40, 8
    c, image, ws, args = _prepared_pair(B, Cn, H, W, Cout, "u8", 5000)
    whole = ops.conv1_prepared(image, ws, Cout, vpool=vpool, **args)
    if not vpool:
        e = _err(whole, c["exp"])
        print(f"f. whole launch {B}x{Cn}x{H}x{W}: {e:.2e} (bound {BOUND:.0e})")
        assert e <= BOUND
    wbits = whole.view(torch.int32).cpu()
    for cam0, ncam in [(1, 2), (0, 1)]:
        buf = torch.full(tuple(whole.shape), SENTINEL, dtype=torch.int32, device=dev()).view(torch.float32)
        ops.conv1_prepared(image, ws, Cout, vpool=vpool, cam0=cam0, ncam=ncam, out=buf, **args)
        bits = buf.view(torch.int32).cpu()
        inside = torch.equal(bits[cam0:cam0 + ncam], wbits[cam0:cam0 + ncam])
        outside = bool((bits[:cam0] == SENTINEL).all()) and bool((bits[cam0 + ncam:] == SENTINEL).all())
        print(f"f. cameras {cam0}..{cam0 + ncam - 1} of {Cn}{' vpool' if vpool else ''}: range == whole launch bitwise: {inside}, "
              f"other cameras untouched: {outside}")
        assert inside and outside
    buf = torch.zeros_like(whole)
    for cam0, ncam in [(2, 2), (-1, 1), (1, 0)]:
        with pytest.raises(RuntimeError, match=r"code -2.*camera range"):
            ops.conv1_prepared(image, ws, Cout, vpool=vpool, cam0=cam0, ncam=ncam, out=buf, **args)


# ---- g. hpool ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(nrows, W, Cc):
    g = torch.Generator().manual_seed(100000 + 1000 * nrows + 10 * W + Cc)
    x = torch.round(torch.randn(nrows, W, Cc, generator=g))                       # a few levels, both signs: ties everywhere
    exp = F.max_pool2d(x.permute(0, 2, 1).unsqueeze(2), (1, 3), (1, 2), (0, 1)).squeeze(2).permute(0, 2, 1).contiguous()
    return x, exp


def test_hpool_inputs_are_full_of_ties_and_negative_values():
    x, exp = _rows(7, 33, 64)
    win = F.pad(x.permute(0, 2, 1), (1, 1), value=float("-inf")).unfold(2, 3, 2)             # [n][C][Wo][3]
    tied = (win == exp.permute(0, 2, 1).unsqueeze(-1)).sum(-1) >= 2
    print(f"g. hpool inputs: {float(tied.float().mean()):.2f} of the windows tied, {float((exp < 0).float().mean()):.3f} of the maxima negative")
    assert float(tied.float().mean()) >= 0.25 and bool((exp < 0).any()) and bool(tied[:, :, 0].any())


@pytest.mark.parametrize("nrows", [1, 7])
@pytest.mark.parametrize("Cc", [4, 8, 64])
@pytest.mark.parametrize("W", [1, 2, 31, 32, 33])
def test_hpool_bit_exact(W, Cc, nrows):
    x, exp = _rows(nrows, W, Cc)
    got = ops.hpool(x.to(dev()))
    assert got.shape == exp.shape and torch.equal(got.cpu(), exp)


def test_hpool_grid_stride_second_pass():
    """the grid is capped at 4096 blocks of 256 threads: more than 1 048 576 float4 outputs make every thread loop"""
    nrows, W, Cc = 2100, 64, 64
    assert nrows * ((W - 1) // 2 + 1) * (Cc // 4) > 4096 * 256
    x, exp = _rows(nrows, W, Cc)
    got = ops.hpool(x.to(dev())).cpu()
    bad = int((got != exp).sum())
    print(f"g. hpool {nrows}x{W}x{Cc}: {bad} of {exp.numel()} outputs differ")
    assert torch.equal(got, exp)


def test_hpool_rejects_bad_channel_count_and_ignores_zero_rows():
    with pytest.raises(RuntimeError, match=r"code -2.*multiple of 4"):
        ops.hpool(torch.zeros(3, 9, 6, device=dev()))
    lib = L.load()
    assert lib.actmi_op_hpool(C.c_void_p(0), C.c_void_p(0), 0, 9, 8, L.current_stream_ptr()) == 0
    y = ops.hpool(torch.zeros(0, 9, 8, device=dev()))
    assert tuple(y.shape) == (0, 5, 8)
    torch.cuda.synchronize()


# ---- i. u8_to_nhwc4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cam,H,W", [(1, 1, 1, 1), (2, 3, 7, 9), (3, 2, 30, 43)])
def test_u8_to_nhwc4_bit_exact(B, Cam, H, W):
    g = torch.Generator().manual_seed(7000 + H)
    img = torch.randint(0, 256, (B, Cam, H, W, 3), dtype=torch.uint8, generator=g)
    img[0, 0, 0, 0, 0], img[-1, -1, -1, -1, -1] = 255, 1
    got = ops.u8_to_nhwc4(img.to(dev())).cpu()
    assert got.shape == (Cam, B, H, W, 4)
    exp = (img.double() / 255).float().permute(1, 0, 2, 3, 4)
    assert torch.equal(got[..., :3], exp)
    assert torch.equal(got[..., 3].view(torch.int32), torch.zeros(Cam, B, H, W, dtype=torch.int32))      # +0.0 exactly
