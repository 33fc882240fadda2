"""The device-side training augmentation on the GPU: actmi_op_augment_u8 and actmi_op_warp_u16 against their numpy definitions
(actmi.ops.image_augment_ref / depth_warp_ref), the ImageAugment class, graph capture, the error returns and forward_pass.

Every equality here is bitwise.  That bar is derived, not measured: the definition fixes the order of every fp32 product and sum
and forbids contraction; numpy on the CPU and the gfx950 VALU both round each of them correctly; the two divisions (the resize
scale, on the host; the mean, in double) are correctly rounded on both sides; the grey sum is an integer.

Shapes: (37, 53) -- odd, 1961 pixels, so images after the first start off a word boundary and the last workgroup of an image is
partly empty; (48, 64) -- whole workgroups, every image word-aligned; SEVERAL = (70, 101) -- 7070 pixels, seven workgroups of 1024
pixels per image, so that the grey sum of contrast crosses workgroups (the other two shapes take two and three)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402

DEV = "cuda:0"
SEVERAL = (70, 101)
SHAPES = [(37, 53), (48, 64), SEVERAL]


def _crop(H, W):
    return int(H * 0.95), int(W * 0.95)


def _frames(kind, B, K, H, W, seed):
    if kind == "zeros":
        return np.zeros((B, K, H, W, 3), np.uint8)
    if kind == "ones":
        return np.full((B, K, H, W, 3), 255, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, (B, K, H, W, 3), dtype=np.uint8)


def _records(B, H, W, code, flip):
    """B records of jitter order `code`: offsets at 0 and at their maxima, angles 0 / +5 / -5 and the factors at both ends of their
    ranges, rotated through the samples (and through `flip`) so that every launch mixes them"""
    ch, cw = _crop(H, W)
    i = np.arange(B) + flip
    return ops.augment_records(B, top=np.where(i % 2 == 0, 0, H - ch), left=np.where((i // 2) % 2 == 0, W - cw, 0),
                               angle=np.choose(i % 3, [0.0, 5.0, -5.0]), order=code,
                               fb=np.where(i % 2 == 0, 0.7, 1.3), fc=np.where((i + code) % 2 == 0, 1.4, 0.6),
                               fs=np.where((i // 2 + code) % 2 == 0, 0.5, 1.5))


def _desc(inp, out, rec, ws, B, K, H, W, ch, cw, ws_bytes=None):
    d = L.AugmentDesc()
    d.in_, d.out, d.records, d.ws = inp, out, rec, ws
    d.ws_bytes = ws_bytes if ws_bytes is not None else int(L.load().actmi_op_augment_workspace_bytes(B, K, H, W))
    d.B, d.K, d.H, d.W, d.ch, d.cw = B, K, H, W, ch, cw
    return d


def _rec_dev(rec):
    return torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)


# ---- 1. bitwise equality with the numpy definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B,K", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_augment_is_bitwise_the_numpy_definition(B, K, H, W):
    ch, cw = _crop(H, W)
    aug = ops.ImageAugment(DEV, K, H, W, max_batch=3)
    assert (aug.ch, aug.cw) == (ch, cw)
    saturated = False
    for code in range(6):
        for n, kind in enumerate(("random", "zeros", "ones")):
            img = _frames(kind, B, K, H, W, seed=code)
            rec = _records(B, H, W, code, flip=n + code)
            aug.set_records(rec)
            got = aug.run(torch.from_numpy(img).to(DEV)).cpu().numpy()
            exp = ops.image_augment_ref(img, rec, ch, cw)
            assert np.array_equal(got, exp), (code, kind, int(np.abs(got.astype(int) - exp).max()), float((got != exp).mean()))
            assert kind != "random" or not np.array_equal(exp, img)    # the records really change the frames
            saturated = saturated or (kind == "ones" and exp.max() == 255 and float(rec["fb"][0]) > 1)
    assert saturated                                                   # an all-255 frame met gains above 1 and stayed at 255


def test_identity_records_two_runs_and_the_draw():
    H, W, B, K = 37, 53, 3, 3
    img = torch.from_numpy(_frames("random", B, K, H, W, 1)).to(DEV)
    depth = torch.from_numpy(np.random.default_rng(2).integers(0, 65536, (B, K, 1, H, W)).astype(np.uint16)).to(DEV)
    whole = ops.ImageAugment(DEV, K, H, W, max_batch=B, ratio=1.0, Kd=K)
    for code in range(6):
        whole.set_records(ops.augment_records(B, order=code))
        o, d = whole.run(img, depth)
        assert torch.equal(o, img) and torch.equal(d.view(torch.int16), depth.view(torch.int16)), code
    aug = ops.ImageAugment(DEV, K, H, W, max_batch=B, seed=3, Kd=K)
    a, da = (t.clone() for t in aug.apply(img, depth))
    rec = aug.records()
    assert len(rec) == B and not torch.equal(a, img)
    b, db = (t.clone() for t in aug.run(img, depth))                   # the same records once more: bitwise repeatable
    assert torch.equal(a, b) and torch.equal(da.view(torch.int16), db.view(torch.int16))
    ch, cw = _crop(H, W)
    assert np.array_equal(a.cpu().numpy(), ops.image_augment_ref(img.cpu().numpy(), rec, ch, cw))
    assert np.array_equal(da.cpu().numpy(), ops.depth_warp_ref(depth.cpu().numpy(), rec, ch, cw))
    c = aug.apply(img).clone()                                         # a fresh draw
    assert not torch.equal(c, a) and not np.array_equal(aug.records(), rec)
    aug.set_seed(3)
    assert torch.equal(aug.apply(img), a)
    with pytest.raises(NotImplementedError):
        aug.run(img.float())
    with pytest.raises(ValueError):
        aug.run(img[:, :2].contiguous())


# ---- 2. nothing is written outside `out` ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 64])
def test_sentinels_around_out_survive_at_odd_width(lead):
    """3-byte pixels at odd W: rows and images end off a word boundary.  `out` sits `lead` bytes into a buffer of 0xA5 sentinels
    (lead 1: not even image 0 is word-aligned) and is followed by 64 more."""
    lib = L.load()
    B, K, H, W = 2, 3, 37, 53
    ch, cw = _crop(H, W)
    n = B * K * H * W * 3
    img = _frames("random", B, K, H, W, 5)
    rec = _records(B, H, W, 3, 0)
    t_in, t_rec = torch.from_numpy(img).to(DEV), _rec_dev(rec)
    ws = torch.zeros(int(lib.actmi_op_augment_workspace_bytes(B, K, H, W)) // 4, dtype=torch.int32, device=DEV)
    buf = torch.full((lead + n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    d = _desc(t_in.data_ptr(), buf.data_ptr() + lead, t_rec.data_ptr(), ws.data_ptr(), B, K, H, W, ch, cw)
    L.check(lib.actmi_op_augment_u8(C.byref(d), L.current_stream_ptr()), None, "op_augment_u8")
    got = buf.cpu().numpy()
    assert (got[:lead] == 0xA5).all() and (got[lead + n:] == 0xA5).all()
    assert np.array_equal(got[lead:lead + n].reshape(img.shape), ops.image_augment_ref(img, rec, ch, cw))
    # the u16 warp: `lead` elements in, so that 8-byte stores are possible for no image (lead 1) or for some
    dep = np.random.default_rng(6).integers(0, 65536, (B, K, H, W)).astype(np.uint16)
    t_dep = torch.from_numpy(dep).to(DEV)
    m = B * K * H * W
    buf16 = torch.full((lead + m + 32,), 0x5A5A, dtype=torch.int16, device=DEV)
    d = _desc(t_dep.data_ptr(), buf16.data_ptr() + 2 * lead, t_rec.data_ptr(), ws.data_ptr(), B, K, H, W, ch, cw)
    L.check(lib.actmi_op_warp_u16(C.byref(d), L.current_stream_ptr()), None, "op_warp_u16")
    got = buf16.cpu().numpy()
    assert (got[:lead] == 0x5A5A).all() and (got[lead + m:] == 0x5A5A).all()
    assert np.array_equal(got[lead:lead + m].view(np.uint16).reshape(dep.shape), ops.depth_warp_ref(dep, rec, ch, cw))


# ---- 3. the u16 warp ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("B,Kd", [(1, 1), (3, 3)])
def test_warp_u16_is_bitwise_the_numpy_definition(B, Kd, H, W):
    ch, cw = _crop(H, W)
    aug = ops.ImageAugment(DEV, 1, H, W, max_batch=3, Kd=Kd)
    img = torch.zeros((B, 1, H, W, 3), dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(H)
    for n in range(3):
        dep = rng.integers(0, 65536, (B, Kd, 1, H, W)).astype(np.uint16)
        dep[:, :, :, ::5, ::7] = 65535                                 # the top of the range must survive (a signed or 15-bit path would not)
        if n == 2:
            dep[:] = 65535
        rec = _records(B, H, W, n, flip=n)
        aug.set_records(rec)
        got = aug.run(img, torch.from_numpy(dep).to(DEV))[1].cpu().numpy()
        exp = ops.depth_warp_ref(dep, rec, ch, cw)
        assert got.shape == dep.shape and np.array_equal(got, exp), n
        assert exp.max() > 60000 and (n != 2 or exp.max() == 65535)
        for b in range(B):                                             # rotated-out corners are 0, whatever the frame holds
            if rec["sin"][b] != 0:
                assert got[b, :, 0, 0, 0].max() == 0 and got[b, :, 0, -1, -1].max() == 0
                assert n != 2 or got[b, :, 0, H // 2, W // 2].min() == 65535


# ---- 4. what the kernel finds in a record is held to its range ----------------------------------------------------------------------------
def test_out_of_range_record_fields_are_clamped():
    B, K, H, W = 4, 2, 37, 53
    ch, cw = _crop(H, W)
    img = _frames("random", B, K, H, W, 7)
    dep = np.random.default_rng(8).integers(0, 65536, (B, K, 1, H, W)).astype(np.uint16)
    aug = ops.ImageAugment(DEV, K, H, W, max_batch=B, Kd=K)
    wild = ops.augment_records(B, top=[-1, H, 1 << 30, -(1 << 30)], left=[W, -5, -(1 << 31), (1 << 31) - 1], order=[-1, 6, 1 << 20, -(1 << 31)],
                               angle=2.5, fb=1.2, fc=0.8, fs=1.4)
    held = ops.augment_records(B, top=[0, H - ch, H - ch, 0], left=[W - cw, 0, 0, W - cw], order=[0, 5, 5, 0], angle=2.5, fb=1.2, fc=0.8, fs=1.4)
    aug.set_records(wild)
    a, da = (t.cpu().numpy() for t in aug.run(torch.from_numpy(img).to(DEV), torch.from_numpy(dep).to(DEV)))
    assert np.array_equal(a, ops.image_augment_ref(img, held, ch, cw)) and np.array_equal(a, ops.image_augment_ref(img, wild, ch, cw))
    assert np.array_equal(da, ops.depth_warp_ref(dep, held, ch, cw))


# ---- 5. the error returns ---------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_with_a_message_and_launch_nothing():
    lib = L.load()
    B, K, H, W = 2, 2, 37, 53
    ch, cw = _crop(H, W)
    n = B * K * H * W
    t_in = torch.from_numpy(_frames("random", B, K, H, W, 9)).to(DEV)
    t_rec = _rec_dev(_records(B, H, W, 0, 0))
    nws = int(lib.actmi_op_augment_workspace_bytes(B, K, H, W))
    assert nws == B * K * 2 * 4
    ws = torch.zeros(nws // 4 + 1, dtype=torch.int32, device=DEV)
    out = torch.full((n * 3 + 16,), 7, dtype=torch.uint8, device=DEV)
    i, o, r, w = t_in.data_ptr(), out.data_ptr(), t_rec.data_ptr(), ws.data_ptr()
    bad = {
        "null in": _desc(0, o, r, w, B, K, H, W, ch, cw), "null out": _desc(i, 0, r, w, B, K, H, W, ch, cw),
        "null records": _desc(i, o, 0, w, B, K, H, W, ch, cw), "null ws": _desc(i, o, r, 0, B, K, H, W, ch, cw),
        "out is in": _desc(o, o, r, w, B, K, H, W, ch, cw), "out overlaps the end of in": _desc(o + 8, o, r, w, B, K, H, W, ch, cw),
        "ch 0": _desc(i, o, r, w, B, K, H, W, 0, cw), "ch > H": _desc(i, o, r, w, B, K, H, W, H + 1, cw),
        "cw 0": _desc(i, o, r, w, B, K, H, W, ch, 0), "cw > W": _desc(i, o, r, w, B, K, H, W, ch, W + 1),
        "misaligned ws": _desc(i, o, r, w + 2, B, K, H, W, ch, cw), "short ws": _desc(i, o, r, w, B, K, H, W, ch, cw, ws_bytes=nws - 4),
        "B 0": _desc(i, o, r, w, 0, K, H, W, ch, cw),
    }
    for fn in (lib.actmi_op_augment_u8, lib.actmi_op_warp_u16):
        for name, d in bad.items():
            rc = fn(C.byref(d), L.current_stream_ptr())
            msg = lib.actmi_op_last_error()
            assert rc != 0 and msg, name
        assert fn(None, L.current_stream_ptr()) != 0 and b"null descriptor" in lib.actmi_op_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((ws == 0).all())            # nothing ran
    assert lib.actmi_op_augment_workspace_bytes(1, 70000, H, W) < 0
    good = _desc(i, o, r, w, B, K, H, W, ch, cw)                        # and the same buffers are fine when asked properly
    L.check(lib.actmi_op_augment_u8(C.byref(good), L.current_stream_ptr()), None, "op_augment_u8")
    assert not lib.actmi_op_last_error()
    torch.cuda.synchronize()
    assert bool((out[n * 3:] == 7).all()) and not bool((out[:n * 3] == 7).all())


# ---- 6. a captured launch reads the records of every replay ----------------------------------------------------------------------------------
def test_captured_graph_replays_with_new_records():
    B, K, H, W = 2, 2, 48, 64
    ch, cw = _crop(H, W)
    img = _frames("random", B, K, H, W, 10)
    dep = np.random.default_rng(11).integers(0, 65536, (B, K, 1, H, W)).astype(np.uint16)
    t_img, t_dep = torch.from_numpy(img).to(DEV), torch.from_numpy(dep).to(DEV)
    aug = ops.ImageAugment(DEV, K, H, W, max_batch=B, Kd=K)
    r1, r2 = _records(B, H, W, 1, 0), _records(B, H, W, 4, 1)
    aug.set_records(r1)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug.run(t_img, t_dep)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        o, d = aug.run(t_img, t_dep)
    for rec in (r1, r2, r1):
        aug.set_records(rec)
        aug.out.zero_()
        graph.replay()
        assert np.array_equal(o.cpu().numpy(), ops.image_augment_ref(img, rec, ch, cw))
        assert np.array_equal(d.cpu().numpy(), ops.depth_warp_ref(dep, rec, ch, cw))


# ---- 7. forward_pass at tiny_config ------------------------------------------------------------------------------------------------------------
def _policy(**over):
    from policy import ACTPolicy
    kw = {"kl_weight": 10, "lr": 1e-5, "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2,
          "nheads": 4, "camera_names": ["a", "b"], "image_h": 64, "image_w": 96, "base_width": 8}      # tiny_config's sizes
    kw.update(over)
    pol = ACTPolicy(kw, max_batch=2)
    pol.train()
    pol.train_dropout = 0.0                                            # (the compared calls must draw the same masks: none)
    return pol


@pytest.mark.parametrize("use_depth", [False, True])
def test_forward_pass_augments_on_the_device_like_the_numpy_definition(use_depth):
    import imitate_episodes as ie
    from actmi.config import tiny_config
    cfg = tiny_config()
    B, K, H, W = 2, len(cfg.camera_names), cfg.image_h, cfg.image_w
    over = {"use_depth": True, "depth_camera_names": ["a", "b"]} if use_depth else {}
    p1, p2 = _policy(**over), _policy(**over)
    assert (p1.model.cfg.image_h, p1.model.cfg.image_w, p1.model.cfg.hidden_dim) == (H, W, cfg.hidden_dim)
    rng = np.random.default_rng(12)
    img = torch.from_numpy(rng.integers(0, 256, (B, K, H, W, 3), dtype=np.uint8))
    qpos, act = torch.randn(B, 14, generator=torch.Generator().manual_seed(1)), torch.randn(B, 8, 16, generator=torch.Generator().manual_seed(2))
    pad = torch.zeros(B, 8, dtype=torch.bool)
    pad[:, 6:] = True
    depth = torch.from_numpy(rng.integers(300, 60000, (B, K, 1, H, W)).astype(np.uint16))
    batch = (img, qpos, act, pad) + ((depth,) if use_depth else ())
    eps = torch.randn(B, p1.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(3)).cuda()
    aug = ie.make_augment({"augment_images": True}, p1, seed=4)
    assert (aug.K, aug.Kd, aug.H, aug.W, aug.max_batch) == (K, K if use_depth else 0, H, W, 2)
    p1.next_eps = eps
    got = ie.forward_pass(batch, p1, augment=aug)
    rec = aug.records()
    img_ref = torch.from_numpy(ops.image_augment_ref(img.numpy(), rec, aug.ch, aug.cw))
    assert not torch.equal(img_ref, img)
    ref_batch = (img_ref, qpos, act, pad) + ((torch.from_numpy(ops.depth_warp_ref(depth.numpy(), rec, aug.ch, aug.cw)),) if use_depth else ())
    p2.next_eps = eps
    exp = ie.forward_pass(ref_batch, p2)
    p2.next_eps = eps
    plain = ie.forward_pass(batch, p2)                                 # without `augment`: the batch as it is
    p1.next_eps = eps
    plain1 = ie.forward_pass(batch, p1, augment=None)
    for k in ("l1", "kl", "loss"):
        print(f"use_depth={use_depth} {k}: augmented {float(got[k]):.6f}, plain {float(plain[k]):.6f}")
        assert np.isfinite(float(got[k])) and float(got[k]) == float(exp[k]), k
        assert float(plain1[k]) == float(plain[k]), k
    assert float(got["loss"]) != float(plain["loss"])
    if use_depth:
        with pytest.raises(NotImplementedError, match="uint16"):
            ie.forward_pass((img, qpos, act, pad, depth.float() / 65535.0), p1, augment=aug)
    with pytest.raises(NotImplementedError, match="u8"):
        ie.forward_pass((img.permute(0, 1, 4, 2, 3).float() / 255.0,) + batch[1:], p1, augment=aug)
