"""The stem's full-pool form (conv1.hip vpool 2 + the seam pass of pool.hip; ops.conv1_pooled): conv1 writes the finished
3x3 / s2 / p1 max pool.  Every comparison is torch.equal against two references computed in the same case:

    ops.hpool(ops.conv1_prepared(..., vpool=True))      the two-launch form it replaces in inference
    F.max_pool2d(plain, 3, 2, 1)                        of the plain form's output

The output, and the seam workspace, are pre-filled with a NaN sentinel in every case, so an element the kernels do not write
(or a seam column that the seam pass leaves as the right strip's partial max) shows.

a. widths: Wo = 18 (one short strip), 64 (one strip: no seam pass), 65 / 66 (the right strip owns one / two columns), 127, 128,
   129 (around two full strips), 130 (three strips);
b. heights and row segments at B = 1, C = 1: Ho = 2, Ho = 4, and the segment geometry of test_gpu_stem_forms section e (41 row
   pairs in 10 segments of 5: the last segment empty, the one before a single pair behind a halo step), also with three strips;
c. u8 and f32 images, Cout 8 and 64, C = 2 with B = 2;
d. a camera range into sentinel-filled out and seam: the range equals the whole launch bitwise, everything else (the other
   cameras' seam rows included) keeps the sentinel;
e. ties and zeros: a bias that puts most ReLU outputs at exactly 0, and an image with constant regions across a seam; the
   share of tied 3x3 windows is printed and must be above zero;
f. rejections: the four of the vpool 1 form, and a missing or too small seam workspace when Wo > 64;
g. engine level (tiny config, 2 cameras, image_w = 160: Wo = 80, two strips, B = 2): maxpool and a_hat of the default engine
   bit-equal to those of an engine created under ACTMI_CONV1_VPOOL=0; the captured graph returns the eager step's a_hat.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402

SENTINEL = 0x7FC12345                                              # a NaN payload: any write shows


def dev():
    return torch.device("cuda:0")


def _width(Wo, even):
    W = 2 * Wo if even else 2 * Wo - 1
    assert (W - 1) // 2 + 1 == Wo
    return W


@functools.lru_cache(maxsize=None)
def _case(B, Cn, H, W, Cout, src, seed, kind="random"):
    """operands of one case on the device and the two references on the host (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, Cn, H, W, 3), dtype=torch.uint8, generator=g)
    w = torch.randn(Cn, Cout, 3, 7, 7, generator=g) / 147 ** 0.5
    scale, bias = torch.rand(Cn, Cout, generator=g) + 0.5, torch.randn(Cn, Cout, generator=g) * 0.1
    if kind == "zeros":
        bias = bias - 1.5                                          # most pre-activations negative: ReLU outputs exactly 0
    if kind == "constant":
        img[:, :, :, W // 4: (3 * W) // 4, :] = 128                # a constant band over every seam of the frame's middle
        img[:, :, : H // 2, : W // 8, :] = 7
    d = dev()
    image = img.to(d) if src == "u8" else (img.permute(0, 1, 4, 2, 3).float() / 255).contiguous().to(d)
    ws = ops.conv1_prepare(w.to(d), lut_mode=0)
    args = dict(relu=True, scale=scale.to(d), bias=bias.to(d))
    plain = ops.conv1_prepared(image, ws, Cout, **args)
    Ho, Wo = plain.shape[2], plain.shape[3]
    vp = ops.conv1_prepared(image, ws, Cout, vpool=True, **args)
    ref_hp = ops.hpool(vp.view(Cn * B, Ho // 2, Wo, Cout)).cpu().view(Cn, B, Ho // 2, -1, Cout)
    p_nchw = plain.cpu().view(Cn * B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    ref_mp = F.max_pool2d(p_nchw, 3, 2, 1).permute(0, 2, 3, 1).contiguous().view(Cn, B, Ho // 2, -1, Cout)
    return dict(image=image, ws=ws, args=args, plain=p_nchw, ref_hp=ref_hp, ref_mp=ref_mp, Ho=Ho, Wo=Wo)


def _sentinel(shape_or_n):
    return torch.full(shape_or_n if isinstance(shape_or_n, tuple) else (shape_or_n,), SENTINEL, dtype=torch.int32,
                      device=dev()).view(torch.float32)


def _run(c, Cout, **kw):
    """conv1_pooled into sentinel-filled out and seam -> (out on the host as int32 bits, seam bits)"""
    B, Cn = c["ref_hp"].shape[1], c["ref_hp"].shape[0]
    out = _sentinel(tuple(c["ref_hp"].shape))
    img = c["image"]
    H, W = (img.shape[2], img.shape[3]) if img.dtype == torch.uint8 else (img.shape[3], img.shape[4])
    n = ops.conv1_seam_floats(B, Cn, H, W, Cout)
    assert (n > 0) == (c["Wo"] > 64)
    seam = _sentinel(n) if n else None
    ops.conv1_pooled(img, c["ws"], Cout, out=out, seam=seam, **c["args"], **kw)
    torch.cuda.synchronize()
    return out.view(torch.int32).cpu(), (seam.view(torch.int32).cpu() if n else None)


def _check(tag, B, Cn, H, W, Cout, src, seed, kind="random"):
    c = _case(B, Cn, H, W, Cout, src, seed, kind)
    bits, _ = _run(c, Cout)
    got = bits.view(torch.float32)
    assert tuple(got.shape) == (Cn, B, c["Ho"] // 2, (c["Wo"] - 1) // 2 + 1, Cout)
    unwritten = int((bits == SENTINEL).sum())
    ok_hp, ok_mp = torch.equal(got, c["ref_hp"]), torch.equal(got, c["ref_mp"])
    cols = sorted(set(torch.nonzero((got != c["ref_hp"]).any(4).any(2).any(1).any(0))[:, 0].tolist()))[:12]
    print(f"{tag} {B}x{Cn}x{H}x{W} (Ho {c['Ho']}, Wo {c['Wo']}) Cout {Cout} {src}: unwritten {unwritten} of {bits.numel()}; "
          f"== hpool(vpool): {ok_hp}, == F.max_pool2d(plain): {ok_mp}; pooled columns that differ: {cols}")
    assert unwritten == 0, "elements of the pooled map that no kernel wrote"
    assert ok_hp, "conv1_pooled != hpool(vpool 1 output)"
    assert ok_mp, "conv1_pooled != F.max_pool2d(plain output, 3, 2, 1)"
    return c, got


# ---- a. seams and widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Wo,even", [(18, False), (64, True), (65, False), (66, True), (127, False), (128, True), (129, False),
                                     (130, True)])
def test_widths_and_seams(Wo, even):
    _check("a.", 2, 2, 12, _width(Wo, even), 64, "u8", 100 + Wo)


# ---- b. heights and row segments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 40),          # Ho = 2: a single row pair
                                 (8, 40),          # Ho = 4
                                 (164, 40),        # 41 row pairs in 10 segments of 5: last empty, the one before one pair + halo
                                 (36, 128),        # 9 row pairs in 2 segments, exactly one strip
                                 (164, 260)])      # the same segments over three strips (Wo = 130)
def test_heights_and_row_segments(H, W):
    _check("b.", 1, 1, H, W, 8, "u8", 200 + H + W)


# ---- c. formats and channels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("Cout", [8, 64])
@pytest.mark.parametrize("W", [43, 129, 260])      # Wo = 22, 65, 130
def test_formats_and_channels(W, Cout, src):
    _check("c.", 2, 2, 20, W, Cout, src, 300 + W + Cout)


# ---- d. camera range ---------------------------------------------------------------------------------------------------------------
def test_camera_range_writes_its_cameras_only():
    B, Cn, H, W, Cout = 2, 3, 20, 160, 8                              # Wo = 80: two strips, one seam column per row
    c = _case(B, Cn, H, W, Cout, "u8", 400)
    whole, whole_seam = _run(c, Cout)
    assert torch.equal(whole.view(torch.float32), c["ref_hp"]) and not bool((whole_seam == SENTINEL).any())
    for cam0, ncam in [(1, 2), (0, 1), (1, 1)]:
        bits, seam = _run(c, Cout, cam0=cam0, ncam=ncam)
        seam, wseam = seam.view(Cn, -1), whole_seam.view(Cn, -1)
        inside = torch.equal(bits[cam0:cam0 + ncam], whole[cam0:cam0 + ncam]) and torch.equal(seam[cam0:cam0 + ncam], wseam[cam0:cam0 + ncam])
        outside = all(bool((x == SENTINEL).all()) for x in (bits[:cam0], bits[cam0 + ncam:], seam[:cam0], seam[cam0 + ncam:]))
        print(f"d. cameras {cam0}..{cam0 + ncam - 1} of {Cn}: range == whole launch bitwise: {inside}, other cameras' out and seam untouched: {outside}")
        assert inside and outside
    for cam0, ncam in [(2, 2), (-1, 1), (1, 0)]:
        with pytest.raises(RuntimeError, match=r"code -2.*camera range"):
            _run(c, Cout, cam0=cam0, ncam=ncam)


# ---- e. ties and zeros -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zeros", "constant"])
def test_ties_and_zeros(kind):
    c, got = _check(f"e. {kind}", 1, 2, 20, 260, 8, "u8", 500, kind)
    win = F.pad(c["plain"], (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2)       # [n][C][Hp][Wp][3][3]
    mx = win.amax((-1, -2), keepdim=True)
    tied = ((win == mx).sum((-1, -2)) >= 2).float()
    zero = float((c["plain"] == 0).float().mean())
    seam_tied = float(tied[:, :, :, 32::32].mean())
    print(f"e. {kind}: {float(tied.mean()):.3f} of the 3x3 windows tied ({seam_tied:.3f} of those on seam columns), "
          f"{zero:.3f} of the ReLU outputs exactly 0")
    assert float(tied.mean()) > 0 and seam_tied > 0
    if kind == "zeros":
        assert zero > 0.5


# ---- f. rejections -----------------------------------------------------------------------------------------------------------------
def test_rejections():
    d = dev()

    def operands(H, W, Cout):
        g = torch.Generator().manual_seed(600 + H + Cout)
        image = torch.randint(0, 256, (1, 1, H, W, 3), dtype=torch.uint8, generator=g).to(d)
        ws = ops.conv1_prepare((torch.randn(1, Cout, 3, 7, 7, generator=g) / 12).to(d), lut_mode=0)
        return image, ws

    for (H, Cout, kw, msg) in [(70, 8, {}, "even output height"),                    # Ho = 35
                               (36, 6, {}, "Cout % 4 == 0"),
                               (36, 8, dict(prec="f32"), "vpool needs prec f16x3"),
                               (36, 8, dict(relu=False), "without ReLU")]:
        image, ws = operands(H, 40, Cout)
        with pytest.raises(RuntimeError, match=r"code -2") as e:
            ops.conv1_pooled(image, ws, Cout, **kw)
        assert msg in str(e.value), str(e.value)
    image, ws = operands(36, 130, 8)                                                 # Wo = 65
    need = ops.conv1_seam_floats(1, 1, 36, 130, 8)
    assert need == 1 * 1 * 9 * 1 * 8
    for seam in (None, torch.zeros(need - 1, device=d)):
        with pytest.raises(RuntimeError, match=r"code -2.*seam workspace"):
            ops.conv1_pooled(image, ws, 8, seam=seam)
    ops.conv1_pooled(image, ws, 8, seam=torch.zeros(need, device=d))                 # the exact size runs
    image, ws = operands(36, 128, 8)                                                 # Wo = 64: no workspace needed
    assert ops.conv1_seam_floats(1, 1, 36, 128, 8) == 0
    ops.conv1_pooled(image, ws, 8, seam=None)
    torch.cuda.synchronize()


# ---- g. engine level ---------------------------------------------------------------------------------------------------------------
def test_engine_stem_is_bit_identical_and_graph_equals_eager(monkeypatch):
    from actmi import weights as W
    from actmi.config import tiny_config
    from actmi.engine import ACTEngine
    B = 2
    cfg = tiny_config(camera_names=["a", "b"], image_w=160)
    sd_np = W.generate_state_dict(cfg, seed=6)
    inp = W.generate_inputs(cfg, B, seed=9)
    q, im = torch.from_numpy(inp["qpos"]).cuda(), torch.from_numpy(inp["image_u8"]).cuda()

    def engine():
        eng = ACTEngine(cfg, max_batch=B, gemm_prec="f16x3")
        eng.load_state_dict(sd_np)
        eng.finalize()
        return eng

    eng = engine()
    a = eng.forward_infer(q, im).clone()
    pool = eng.debug_tensor("maxpool").clone()
    with pytest.raises(RuntimeError):
        eng.debug_tensor("conv1")                                    # this path writes no conv1 map: the entry must not name one
    replay = eng.capture_infer(B)
    a_graph = replay(q, im).clone()
    torch.cuda.synchronize()
    monkeypatch.setenv("ACTMI_CONV1_VPOOL", "0")
    ref = engine()
    a_ref = ref.forward_infer(q, im).clone()
    pool_ref = ref.debug_tensor("maxpool").clone()
    assert ref.debug_tensor("conv1").numel() == cfg.num_cams * B * (cfg.image_h // 2) * (cfg.image_w // 2) * cfg.base_width
    assert pool.numel() == cfg.num_cams * B * (cfg.image_h // 4) * 40 * cfg.base_width
    ok = (torch.equal(pool, pool_ref), torch.equal(a, a_ref), torch.equal(a_graph, a))
    print(f"g. engine 2 cameras {cfg.image_h}x{cfg.image_w} B {B}: maxpool == two-kernel form: {ok[0]}, a_hat: {ok[1]}, graph == eager: {ok[2]}")
    assert torch.isfinite(a).all() and all(ok)
