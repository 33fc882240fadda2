"""Depth-camera input of the ACT policy (use_depth): the 1-channel stem kernel on its own against a float64 convolution, the
golden fixtures made by the reference's own modules (tests/golden/tiny_depth.npz and depth_w64.npz, tools/gen_golden_depth.py)
for inference and one training step, token cross-talk, graph replay, branch counts and the error returns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import load_fixture, regenerate, sample_like  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402
from actmi import weights as W  # noqa: E402
from actmi.config import tiny_config  # noqa: E402
from actmi.engine import ACTEngine  # noqa: E402

ATOL = 1e-4
_FIX = {}


def _fixture(name):
    """(z, cfg, state_dict, inputs) of a golden fixture, regenerated and hash-checked once per session"""
    if name not in _FIX:
        z, cfg = load_fixture(name)
        sd_np, inp = regenerate(z, cfg)
        _FIX[name] = (z, cfg, sd_np, inp)
    return _FIX[name]


def _engine(cfg, sd_np, max_batch, prec=None, training=False, env=None):
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = ACTEngine(cfg, max_batch=max_batch, gemm_prec=prec, training=training)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.load_state_dict(sd_np)
    eng.finalize()
    return eng


def _dev_inputs(inp, d):
    return (torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d), torch.from_numpy(inp["depth"]).to(d))


def _src(eng, qpos, img, depth):
    """the token matrix the encoder sees, [B, N, D]"""
    eng.debug_stop_after("src")
    eng.forward_infer(qpos, img, depth_img=depth)
    src = eng.debug_tensor("src").view(qpos.shape[0], eng.cfg.num_tokens, eng.cfg.hidden_dim).cpu()
    eng.debug_stop_after("")
    return src


# ---- 1. the stem alone ------------------------------------------------------------------------------------------------------
def _stem_case(B, Cd, H, W, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    depth = torch.rand(B, Cd, 1, H, W, generator=g)
    depth.view(-1)[::17] = 0.0                                    # holes of a depth sensor
    w = torch.randn(Cd, Cout, 1, 7, 7, generator=g) * (2.0 / 49) ** 0.5
    scale = (0.5 + torch.rand(Cd, Cout, generator=g)) * (torch.randint(0, 2, (Cd, Cout), generator=g) * 2 - 1).float()
    bias = 0.3 * torch.randn(Cd, Cout, generator=g)
    return depth, w, scale, bias


def _stem_ref(depth, w, scale, bias):
    """float64 convolution of the fp32-normalised image, scale, bias, ReLU -> (ref, S), both [Cd, B, Ho, Wo, Cout];
    S = |scale| * conv(|x_norm|, |w|) + |bias|"""
    xn = ((depth - 0.5) / 0.5).double()                           # (d - 0.5) / 0.5 in fp32, then exact
    refs, Ss = [], []
    for c in range(depth.shape[1]):
        y = F.conv2d(xn[:, c], w[c].double(), stride=2, padding=3)                          # [B, Cout, Ho, Wo]
        ya = F.conv2d(xn[:, c].abs(), w[c].double().abs(), stride=2, padding=3)
        sc, bi = scale[c].double().view(1, -1, 1, 1), bias[c].double().view(1, -1, 1, 1)
        refs.append(torch.relu(y * sc + bi).permute(0, 2, 3, 1))
        Ss.append((ya * sc.abs() + bi.abs()).permute(0, 2, 3, 1))
    return torch.stack(refs), torch.stack(Ss)


def _check_stem(B, Cd, H, W, Cout):
    depth, w, scale, bias = _stem_case(B, Cd, H, W, Cout, seed=H * 131 + W * 7 + Cout + B)
    ref, S = _stem_ref(depth, w, scale, bias)
    got = ops.conv1_depth(depth.cuda(), w.cuda(), scale.cuda(), bias.cuda())
    assert tuple(got.shape) == tuple(ref.shape) == (Cd, B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout)
    err = (got.cpu().double() - ref).abs()
    bound = 53 * 2.0 ** -24 * S                                   # 49 products + 4: any summation order + the two epilogue operations
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"conv1_depth B{B} Cd{Cd} {H}x{W} Cout{Cout}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}, "
          f"relu zeros {float((ref == 0).double().mean()):.2f}")
    assert bool((err <= bound).all())
    assert 0.05 < float((ref == 0).double().mean()) < 0.95         # both sides of the ReLU are exercised
    return depth, w, scale, bias, got


@pytest.mark.parametrize("B,Cd", [(1, 1), (3, 2)])
@pytest.mark.parametrize("Cout", [8, 64])
@pytest.mark.parametrize("H,W", [(64, 96), (30, 50), (7, 9)])
def test_conv1_depth_matches_float64_convolution(H, W, Cout, B, Cd):
    _check_stem(B, Cd, H, W, Cout)


def test_conv1_depth_full_frame():
    _check_stem(1, 1, 480, 640, 64)


def test_conv1_depth_camera_offset_and_repeatable():
    B, Cd, H, W, Cout = 2, 2, 30, 50, 8
    depth, w, scale, bias, alone = _check_stem(B, Cd, H, W, Cout)
    Ho, Wo = alone.shape[2], alone.shape[3]
    sentinel = 0x7FC12345                                          # a NaN payload: any write shows
    buf = torch.full((5, B, Ho, Wo, Cout), sentinel, dtype=torch.int32, device="cuda").view(torch.float32)
    ops.conv1_depth(depth.cuda(), w.cuda(), scale.cuda(), bias.cuda(), out=buf, out_cam0=2)
    bits = buf.view(torch.int32).cpu()
    assert bool((bits[:2] == sentinel).all()) and bool((bits[4:] == sentinel).all())       # the other cameras' bytes
    assert torch.equal(bits[2:4], alone.view(torch.int32).cpu())                            # two runs, bit for bit
    again = ops.conv1_depth(depth.cuda(), w.cuda(), scale.cuda(), bias.cuda())
    assert torch.equal(again.view(torch.int32), alone.view(torch.int32))


# ---- 2. golden inference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["tiny_depth", "depth_w64"])
def test_depth_forward_matches_reference_golden(name, prec):
    z, cfg, sd_np, inp = _fixture(name)
    B = int(z["batch"])
    assert cfg.use_depth and inp["depth"].shape == (B, cfg.num_depth_cams, 1, cfg.image_h, cfg.image_w)
    eng = _engine(cfg, sd_np, B, prec)
    qpos, img, depth = _dev_inputs(inp, eng.device)
    a = eng.forward_infer(qpos, img, depth_img=depth).cpu().numpy()
    err = np.abs(a - z["infer.a_hat"]).max()
    print(f"{name} [{prec}]: max|a_hat - ref| = {err:.3e}")
    assert err <= ATOL
    got = _src(eng, qpos, img, depth).permute(1, 0, 2).contiguous().numpy()               # [N, B, D] as in the reference
    exp = z["stage.src"]
    tol = 1e-4 * max(1.0, float(np.abs(exp).max()))
    e_all = np.abs(got - exp).max()
    fh, fw = cfg.feat_hw
    d0 = 2 + cfg.num_cams * fh * fw                                                         # first depth token
    assert got.shape == exp.shape == (d0 + cfg.num_depth_cams * fh * fw, B, cfg.hidden_dim)
    e_d = np.abs(got[d0:] - exp[d0:]).max()
    print(f"{name} [{prec}]: src max err {e_all:.3e}, depth rows {e_d:.3e} (tol {tol:.3e}, |depth rows| max {np.abs(exp[d0:]).max():.3f})")
    assert e_all <= tol and e_d <= tol and np.abs(exp[d0:]).max() > 0.05
    assert eng.read_flags() == 0


# ---- 3. no cross-talk ---------------------------------------------------------------------------------------------------------
def test_depth_tokens_do_not_leak_into_rgb_tokens_or_other_cameras():
    z, cfg, sd_np, inp = _fixture("tiny_depth")
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B)
    qpos, img, depth = _dev_inputs(inp, eng.device)
    fh, fw = cfg.feat_hw
    C, Cd = cfg.num_cams, cfg.num_depth_cams
    d0 = 2 + C * fh * fw
    s0 = _src(eng, qpos, img, depth)
    other = torch.from_numpy(W.generate_inputs(cfg, B, seed=99)["depth"]).to(eng.device)
    s1 = _src(eng, qpos, img, other)
    assert torch.equal(s0[:, :d0].view(torch.int32), s1[:, :d0].view(torch.int32))         # latent, proprio, RGB rows: the same bits
    assert not torch.equal(s0[:, d0:], s1[:, d0:])
    # one camera's frame changed: only that camera's rows (h, cam, w) of the depth block change
    mixed = depth.clone()
    mixed[:, 1] = other[:, 1]
    s2 = _src(eng, qpos, img, mixed)
    blk0, blk2 = s0[:, d0:].view(B, fh, Cd, fw, -1), s2[:, d0:].view(B, fh, Cd, fw, -1)
    assert torch.equal(blk0[:, :, 0].view(torch.int32), blk2[:, :, 0].view(torch.int32))
    assert float((blk0[:, :, 1] - blk2[:, :, 1]).abs().max()) > 1e-3
    assert torch.equal(s0[:, :d0].view(torch.int32), s2[:, :d0].view(torch.int32))


# ---- 4. golden training step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("tiny_depth", "f16x3"), ("tiny_depth", "f32"), ("depth_w64", "f16x3")])
def test_depth_training_step_matches_reference_gradients_and_adamw(name, prec):
    z, cfg, sd_np, inp = _fixture(name)
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B, prec, training=True)
    d = eng.device
    qpos, img, depth = _dev_inputs(inp, d)
    actions, is_pad, eps = torch.from_numpy(inp["actions"]).to(d), torch.from_numpy(inp["is_pad"]).to(d), torch.from_numpy(z["train.eps"]).to(d)

    def step():
        out = eng.forward_train(qpos, img, actions, is_pad, eps=eps, depth_img=depth)
        eng.zero_grad()
        eng.backward(1.0)
        return out, eng.grad_arena().clone()
    out, arena = step()
    for k in ("l1", "kl", "loss"):
        got, exp = float(out[k]), float(z["train." + k][0])
        print(f"{name} [{prec}] {k}: hip {got:.6f} ref {exp:.6f}")
        assert abs(got - exp) <= 1e-4 * max(1.0, abs(exp)), k
    for k in ("a_hat", "mu", "logvar"):
        assert np.abs(out[k].cpu().numpy() - z["train." + k]).max() <= 1e-4, k
    none = set(str(n) for n in z["grad_none"])
    assert none == {"is_pad_head.weight", "is_pad_head.bias", "depth_pos_embed.weight"}
    worst_n, worst_s, sampled = (0.0, ""), (0.0, ""), set()
    for n, ref_l2 in zip([str(n) for n in z["grad_names"]], z["grad_l2"]):
        g = eng.grad(n).cpu()
        if n in none or ref_l2 == 0.0:
            assert float(g.abs().max()) == 0.0, n
            continue
        if ref_l2 < 1e-6:                                  # mathematically zero in the reference (fp noise there)
            assert float(g.double().norm()) < 1e-6, n
            continue
        e = abs(float(g.double().norm()) - ref_l2) / ref_l2
        worst_n = max(worst_n, (e, n))
        assert e <= 2e-3, (n, e)
        if "grad." + n in z.files:
            exp = z["grad." + n].reshape(-1).astype(np.float64)
            gs = sample_like(g.numpy(), z).astype(np.float64)
            e = float(np.abs(gs - exp).max() / max(np.abs(exp).max(), 1e-6))     # against the reference's max |grad| (of the sample)
            worst_s = max(worst_s, (e, n))
            sampled.add(n)
            assert e <= 2e-3, (n, e)
    print(f"{name} [{prec}]: worst gradient-norm error {worst_n[0]:.2e} at {worst_n[1]}; worst sampled error / max|grad| "
          f"{worst_s[0]:.2e} at {worst_s[1]}")
    keys = ["depth_backbones.0.0.body.conv1.weight", f"depth_backbones.{cfg.num_depth_cams - 1}.0.body.layer4.1.conv2.weight",
            "depth_backbones.0.0.body.layer2.0.downsample.0.weight", "input_proj_depth.weight", "input_proj_depth.bias", "input_proj.weight"]
    assert set(keys) <= sampled
    assert float(eng.grad("depth_backbones.0.0.body.conv1.weight").abs().max()) > 0
    _, arena2 = step()
    assert torch.equal(arena2.view(torch.int32), arena.view(torch.int32))                   # two identical steps, bitwise
    # one AdamW step with two distinct rates: depth_backbones.* moves with lr_backbone, input_proj_depth.* with lr, and the
    # parameters without a gradient stay where they are
    lr, lr_bb, wd = 1e-5, 3e-5, 1e-4
    before = {k: torch.from_numpy(sd_np[k]).clone() for k in keys + sorted(none)}
    grads = {k: eng.grad(k).cpu() for k in keys}
    eng.adamw_step(lr, lr_bb, wd, step=1)
    after = eng.state_dict()
    for k in sorted(none):
        assert torch.equal(after[k].view(torch.int32), before[k].view(torch.int32)), k
    for k in keys:
        assert W.is_backbone_param(k) == k.startswith("depth_backbones.")
        rate = lr_bb if W.is_backbone_param(k) else lr
        p = before[k].clone().requires_grad_(True)
        opt = torch.optim.AdamW([p], lr=rate, weight_decay=wd)
        p.grad = grads[k].clone()
        opt.step()
        err = float((after[k] - p.detach()).abs().max())
        assert err <= 1e-7 + 1e-6 * float(p.detach().abs().max()), (k, err)
        moved = float((after[k] - before[k]).abs().max())
        assert 0.5 * rate <= moved <= 1.5 * rate, (k, moved)
    assert torch.isfinite(eng.forward_infer(qpos, img, depth_img=depth)).all()              # inference sees the updated weights


# ---- 5. plumbing ----------------------------------------------------------------------------------------------------------------
def test_depth_graph_replay_branches_and_small_batch():
    z, cfg, sd_np, _ = _fixture("tiny_depth")
    MB = 3
    single = _engine(cfg, sd_np, MB, env={"ACTMI_CAM_PIPE": "0"})
    two = _engine(cfg, sd_np, MB, env={"ACTMI_CAM_PIPE": "1"})
    four = _engine(cfg, sd_np, MB, env={"ACTMI_CAM_PIPE": "1", "ACTMI_BRANCHES": "4"})
    d = single.device
    for B in (1, 2, MB):                                                                    # B below max_batch too
        qpos, img, depth = _dev_inputs(W.generate_inputs(cfg, B, seed=50 + B), d)
        ref = single.forward_infer(qpos, img, depth_img=depth).clone()
        assert tuple(ref.shape) == (B, cfg.num_queries, cfg.action_dim) and torch.isfinite(ref).all()
        for tag, eng in (("two", two), ("four", four)):
            got = eng.forward_infer(qpos, img, depth_img=depth)
            assert torch.equal(got, ref), f"B={B} {tag}: max diff {float((got - ref).abs().max()):.3e}"
    replay = two.capture_infer(MB)
    outs = []
    for t in range(2):                                                                      # the second replay: new depth data
        qpos, img, depth = _dev_inputs(W.generate_inputs(cfg, MB, seed=70 + t), d)
        a_g = replay(qpos, img, depth_img=depth).clone()
        a_e = two.forward_infer(qpos, img, depth_img=depth).clone()
        assert torch.equal(a_g, a_e)
        outs.append(a_g)
    assert not torch.equal(outs[0], outs[1])
    with pytest.raises(ValueError):
        replay(qpos, img)
    assert single.read_flags() == 0 and two.read_flags() == 0 and four.read_flags() == 0
    from actmi.engine import InferPipeline
    with pytest.raises(NotImplementedError):
        InferPipeline(two, MB)


@pytest.mark.parametrize("ncam", [2, 3])
def test_depth_src_is_bitwise_equal_with_and_without_camera_branches(ncam):
    """The trunk's camera ranges against the RGB / depth camera groups: with the branches off ONE range [0, Ct) crosses the
    group boundary and issues one projection per group; with ACTMI_BRANCHES=3 the ranges are [0,1) [1,2) [2,4) for 2 + 2
    cameras (every range inside one group) and [0,2) [2,4) [4,6) for 3 + 3 (the middle range straddles the boundary at 3).
    f32 products, so the split-K policy cannot differ between the modes: the token matrix must be the same bits."""
    names = ["a", "b", "c"][:ncam]
    cfg = tiny_config(camera_names=names, use_depth=True, depth_camera_names=list(names))
    sd_np = _fixture("tiny_depth")[2] if ncam == 2 else W.generate_state_dict(cfg, seed=0)
    B = 3
    qpos, img, depth = _dev_inputs(W.generate_inputs(cfg, B, seed=31), torch.device("cuda", 0))

    def src_of(env):
        eng = _engine(cfg, sd_np, B, "f32", env=env)
        # (a debug stop turns the branches off: run the trunk as forward phase 1, then stop phase 2 at the tokens it left)
        eng.set_forward_phase(1)
        eng.forward_infer(qpos, img, depth_img=depth)
        eng.set_forward_phase(2)
        src = _src(eng, qpos, img, depth)
        assert eng.read_flags() == 0
        return src
    off = src_of({"ACTMI_CAM_PIPE": "0"})
    on = src_of({"ACTMI_CAM_PIPE": "1", "ACTMI_BRANCHES": "3"})
    assert torch.isfinite(off).all() and float(off[:, 2 + ncam * cfg.feat_hw[0] * cfg.feat_hw[1]:].abs().max()) > 0.05
    assert torch.equal(on.view(torch.int32), off.view(torch.int32)), f"{int((on != off).sum())} elements differ"


def _raw_config(max_batch=1):
    return L.ActmiConfig(struct_size=C.sizeof(L.ActmiConfig), num_cams=2, image_h=64, image_w=96, base_width=8, hidden_dim=64, nheads=4,
                         dim_feedforward=128, enc_layers=2, dec_layers=2, num_queries=8, state_dim=14, action_dim=16, latent_dim=32,
                         has_cvae_encoder=1, max_batch=max_batch, enable_training=0, kl_weight=10.0)


def test_depth_errors_are_codes_and_exceptions():
    lib = L.load()
    z, cfg, sd_np, inp = _fixture("tiny_depth")
    eng = _engine(cfg, sd_np, 2)
    d = eng.device
    qpos, img, depth = _dev_inputs(inp, d)
    out = torch.full((2, cfg.num_queries, cfg.action_dim), 7.0, device=d)

    def raw_forward(B):
        return lib.actmi_forward_infer(eng.h, C.c_void_p(qpos.data_ptr()), C.c_void_p(img.data_ptr()), L.IMG_U8_NHWC, B,
                                       C.c_void_p(out.data_ptr()), eng._sp())
    # nothing bound: ACTMI_E_STATE, and nothing was launched (the output buffer is untouched)
    assert raw_forward(2) == -4 and b"actmi_set_depth" in lib.actmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    eng.forward_infer(qpos, img, depth_img=depth)                                            # a binding is consumed by one forward
    assert raw_forward(2) == -4
    assert lib.actmi_set_depth(eng.h, C.c_void_p(depth.data_ptr()), 1) == 0                  # bound for another batch
    assert raw_forward(2) == -4 and b"1 samples" in lib.actmi_last_error(eng.h)
    assert lib.actmi_set_depth(eng.h, C.c_void_p(depth.data_ptr()), 3) == -1                 # beyond max_batch
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img)                                                         # no depth
    with pytest.raises(ValueError, match=r"5-D \[B, Cd, 1, H, W\]"):
        eng.forward_infer(qpos, img, depth_img=depth[:, :, 0])                               # the 4-D batch
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, depth_img=depth[:, :1].contiguous())                    # wrong shape
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, depth_img=depth[:, :, :, :, :-1].contiguous())
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, depth_img=depth.transpose(3, 4).contiguous().transpose(3, 4))     # not contiguous
    with pytest.raises(TypeError):
        eng.forward_infer(qpos, img, depth_img=depth.double())
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, depth_img=depth.cpu())
    # a plain handle has no depth to bind
    plain_cfg = tiny_config()
    plain = _engine(plain_cfg, W.generate_state_dict(plain_cfg, seed=5), 2)
    assert lib.actmi_set_depth(plain.h, C.c_void_p(depth.data_ptr()), 2) == -4
    with pytest.raises(ValueError):
        plain.forward_infer(qpos, img, depth_img=depth)
    # the guarded struct and the create rules
    c, h = _raw_config(), C.c_void_p()
    assert C.sizeof(L.ActmiDepthConfig) == 8
    dc = L.ActmiDepthConfig(struct_size=12, num_depth_cams=2)
    assert lib.actmi_create_ex2(C.byref(c), None, C.byref(dc), C.byref(h)) == -1 and not h.value
    assert b"actmi_depth_config.struct_size is 12" in lib.actmi_last_error(None)
    dc = L.ActmiDepthConfig(struct_size=8, num_depth_cams=1)
    assert lib.actmi_create_ex2(C.byref(c), None, C.byref(dc), C.byref(h)) == -1 and not h.value
    assert b"num_depth_cams" in lib.actmi_last_error(None)
    dc = L.ActmiDepthConfig(struct_size=8, num_depth_cams=2)
    pc = L.ActmiPcdConfig(struct_size=16, max_points=8, hidden_dim=64, output_dim=64)
    assert lib.actmi_create_ex2(C.byref(c), C.byref(pc), C.byref(dc), C.byref(h)) == -1 and not h.value
    assert b"point-cloud" in lib.actmi_last_error(None)
    # depth == NULL is actmi_create_ex
    assert lib.actmi_create_ex2(C.byref(c), None, None, C.byref(h)) == 0
    n_plain = lib.actmi_num_params(h)
    lib.actmi_destroy(h)
    h = C.c_void_p()
    assert lib.actmi_create(C.byref(c), C.byref(h)) == 0 and lib.actmi_num_params(h) == n_plain
    lib.actmi_destroy(h)
    assert lib.actmi_version() == 110
    # a checkpoint trained without depth does not load into an engine with it: the missing keys are named
    with pytest.raises(RuntimeError, match="input_proj_depth.weight"):
        eng.load_state_dict(W.generate_state_dict(plain_cfg, seed=5))


def test_depth_policy_surface():
    from policy import ACTPolicy
    z, cfg, sd_np, inp = _fixture("tiny_depth")
    args = {"use_depth": True, "depth_camera_names": ["a", "b"], "kl_weight": 10, "lr": 1e-5, "num_queries": 8, "hidden_dim": 64,
            "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4, "camera_names": ["a", "b"], "image_h": 64,
            "image_w": 96, "base_width": 8, "training": False}
    pol = ACTPolicy(args, max_batch=2)
    qpos, img, depth = _dev_inputs(inp, pol.model.device)
    with pytest.raises(ValueError):
        pol(qpos, img)
    a = pol(qpos, img, depth_img=depth)
    assert torch.isfinite(a).all()
    blob = pol.serialize()
    assert "model.input_proj_depth.weight" in blob and "model.depth_backbones.1.0.body.conv1.weight" in blob
    assert "model.depth_pos_embed.weight" in blob and tuple(blob["model.depth_backbones.0.0.body.conv1.weight"].shape) == (8, 1, 7, 7)
    pol2 = ACTPolicy(dict(args), max_batch=2, init_seed=3)
    assert not torch.equal(pol2(qpos, img, depth_img=depth), a)
    pol2.deserialize(blob)
    assert torch.equal(pol2(qpos, img, depth_img=depth), a)
    # depth_img is ignored by a policy without use_depth, as in the reference
    plain = ACTPolicy({k: v for k, v in args.items() if k not in ("use_depth", "depth_camera_names")}, max_batch=2)
    assert torch.equal(plain(qpos, img, depth_img=depth), plain(qpos, img))
    with pytest.raises(NotImplementedError):
        ACTPolicy({"use_depth": True, "kl_weight": 10, "lr": 1e-5})
    with pytest.raises(NotImplementedError):
        ACTPolicy(dict(args, depth_camera_names=["a"]))
