"""Point-cloud input of the ACT policy (use_pcd): the PointNet kernels on their own, the golden fixture made by the reference's
own modules (tests/golden/tiny_pcd.npz, tools/gen_golden_pcd.py) for inference and one training step, the reference widths
(H = O = 512) with a winner-robust gradient check, capacity edges, graph replay and the error returns."""
import ctypes as C

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
MLP = "pcl_backbone.pointnet._mlp."
PCD_KEYS = [MLP + f"{i}.{s}" for i in (0, 3, 6, 9) for s in ("weight", "bias")] + ["input_proj_pointnet.weight",
                                                                                 "input_proj_pointnet.bias"]


def _engine(cfg, sd_np, max_batch, prec=None, training=False, max_points=64):
    eng = ACTEngine(cfg, max_batch=max_batch, gemm_prec=prec, training=training, max_points=max_points)
    eng.load_state_dict(sd_np)
    eng.finalize()
    return eng


def _cloud(inp, dev, perm=None):
    xyz, rgb = torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"])
    if perm is not None:
        xyz, rgb = xyz[:, perm], rgb[:, perm]
    return {"xyz": xyz.contiguous().to(dev), "rgb": rgb.contiguous().to(dev)}


def _pointnet_ref(sd, xyz, rgb, winners=None):
    """float64 restatement of the branch (pointnet.py:29-36, 65-80; detr_vae.py:206-207): -> (token [B, D], last layer
    [B, P, O]); winners [B, O]: gather those points instead of taking the maximum"""
    p = {k: (v if torch.is_tensor(v) else torch.from_numpy(v)).double() for k, v in sd.items() if k in PCD_KEYS}
    x = torch.cat([xyz.double(), rgb.double()], dim=-1)
    for i in (0, 3, 6):
        x = F.gelu(F.linear(x, p[MLP + f"{i}.weight"], p[MLP + f"{i}.bias"]))
    y = F.linear(x, p[MLP + "9.weight"], p[MLP + "9.bias"])
    feat = y.amax(dim=1) if winners is None else torch.gather(y, 1, winners.long().unsqueeze(1)).squeeze(1)
    return F.linear(feat, p["input_proj_pointnet.weight"], p["input_proj_pointnet.bias"]), y


def _token_row2(eng, qpos, img, cloud):
    eng.debug_stop_after("src")
    eng.forward_infer(qpos, img, pointcloud=cloud)
    src = eng.debug_tensor("src").view(qpos.shape[0], eng.cfg.num_tokens, eng.cfg.hidden_dim).cpu()
    eng.debug_stop_after("")
    return src[:, 2]


# ---- 1. layer 0 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb_scale", [1.0, 255.0])
@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("rows", [1, 37, 1025])
def test_pcd_embed_matches_torch_fp32(rows, H, rgb_scale):
    g = torch.Generator().manual_seed(rows * 7 + H)
    xyz = torch.randn(rows, 3, generator=g)
    rgb = torch.rand(rows, 3, generator=g) * rgb_scale
    a = (6.0 / (H + 6)) ** 0.5
    w0 = (torch.rand(H, 6, generator=g) * 2 - 1) * a
    b0 = torch.randn(H, generator=g) * 0.05
    ref = F.gelu(F.linear(torch.cat([xyz, rgb], -1), w0, b0))
    got = ops.pcd_embed(xyz.cuda(), rgb.cuda(), w0.cuda(), b0.cuda()).cpu()
    err, bar = float((got - ref).abs().max()), 1e-6 * max(1.0, float(ref.abs().max()))
    print(f"pcd_embed rows {rows} H {H} rgb x{rgb_scale:g}: max err {err:.3e} (bar {bar:.3e}, max|ref| {float(ref.abs().max()):.3f})")
    assert tuple(got.shape) == (rows, H) and err <= bar


# ---- 2. maximum over the points -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,pad", [(64, 0), (512, 0), (64, 4)])
@pytest.mark.parametrize("P", [1, 37, 257, 2051])
def test_colmax_is_exact_lowest_index_and_repeatable(P, O, pad):
    B, ld = 2, O + pad
    g = torch.Generator().manual_seed(P * 3 + O + pad)
    x = torch.randn(B, P, ld, generator=g)
    if P >= 3:
        # exact duplicates: one row sits at three positions, so wherever it wins a column there is a three-way tie
        r = [int(v) for v in torch.randperm(P, generator=g)[:3]]
        x[:, r[1]] = x[:, r[0]]
        x[:, r[2]] = x[:, r[0]]
        # and make it win a good share of the columns
        x[:, r, ::2] += 6.0
    xc = x[:, :, :O]
    ref_v, _ = xc.max(dim=1)
    ref_i = (xc == ref_v.unsqueeze(1)).int().argmax(dim=1).int()      # the first (lowest) index that attains the maximum
    xd = x.cuda()
    v, i = ops.colmax(xd, O)
    assert torch.equal(v.cpu(), ref_v) and torch.equal(i.cpu(), ref_i)
    if P >= 3:
        assert int((ref_i == min(r)).sum()) >= B * O // 4              # the ties were really there
    v1, i1 = ops.colmax(xd, O, split=False)                            # one split: the same answer
    assert torch.equal(v1.cpu(), ref_v) and torch.equal(i1.cpu(), ref_i)
    # a NaN comes out in its column only, as torch.max propagates it
    xn = x.clone()
    xn[1, P // 2, 5] = float("nan")
    vn, _ = ops.colmax(xn.cuda(), O)
    vn = vn.cpu()
    assert torch.isnan(vn[1, 5]) and int(torch.isnan(vn).sum()) == 1
    keep = torch.ones(B, O, dtype=torch.bool)
    keep[1, 5] = False
    assert torch.equal(vn[keep], ref_v[keep])
    vn2, in2 = ops.colmax(xn.cuda(), O)
    v2, i2 = ops.colmax(xd, O)
    assert torch.equal(v2, v) and torch.equal(i2, i) and torch.equal(vn2.cpu().view(torch.int32), vn.view(torch.int32))


# ---- 3. golden inference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_pcd_forward_matches_reference_golden(prec):
    z, cfg = load_fixture("tiny_pcd")
    sd_np, inp = regenerate(z, cfg)
    B, P = int(z["batch"]), int(z["points"])
    assert float(z["top2_gap"]) >= 1e-4 and inp["pcd_xyz"].shape == (B, P, 3)
    eng = _engine(cfg, sd_np, B, prec)
    d = eng.device
    qpos, img = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d)
    a = eng.forward_infer(qpos, img, pointcloud=_cloud(inp, d)).cpu().numpy()
    err = np.abs(a - z["infer.a_hat"]).max()
    print(f"tiny_pcd [{prec}]: max|a_hat - ref| = {err:.3e}")
    assert err <= ATOL
    # the token matrix the encoder sees ([N, B, D] in the reference): row 2 is the point-cloud token
    eng.debug_stop_after("src")
    eng.forward_infer(qpos, img, pointcloud=_cloud(inp, d))
    got = eng.debug_tensor("src").cpu().view(B, cfg.num_tokens, cfg.hidden_dim).permute(1, 0, 2).contiguous().numpy()
    eng.debug_stop_after("")
    exp = z["stage.src"]
    tol = 1e-4 * max(1.0, float(np.abs(exp).max()))
    assert got.shape == exp.shape and np.abs(got - exp).max() <= tol
    e2 = np.abs(got[2] - exp[2]).max()
    print(f"tiny_pcd [{prec}]: token row 2 max err {e2:.3e} (|row| max {np.abs(exp[2]).max():.3f})")
    assert e2 <= tol and np.abs(exp[2]).max() > 0.05
    # permuting the points changes nothing but the order candidates meet in
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(7))
    ap = eng.forward_infer(qpos, img, pointcloud=_cloud(inp, d, perm)).cpu().numpy()
    assert np.abs(ap - a).max() <= 1e-6


# ---- 4. golden training step -----------------------------------------------------------------------------------------------
def test_pcd_training_step_matches_reference_gradients_and_adamw():
    z, cfg = load_fixture("tiny_pcd")
    sd_np, inp = regenerate(z, cfg)
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B, training=True)
    d = eng.device
    out = eng.forward_train(torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d),
                            torch.from_numpy(inp["actions"]).to(d), torch.from_numpy(inp["is_pad"]).to(d),
                            eps=torch.from_numpy(z["train.eps"]).to(d), pointcloud=_cloud(inp, d))
    for k in ("l1", "kl", "loss"):
        got, exp = float(out[k]), float(z["train." + k][0])
        print(f"tiny_pcd {k}: hip {got:.6f} ref {exp:.6f}")
        assert abs(got - exp) <= 1e-4 * max(1.0, abs(exp)), k
    for k in ("a_hat", "mu", "logvar"):
        assert np.abs(out[k].cpu().numpy() - z["train." + k]).max() <= 1e-4, k
    eng.zero_grad()
    eng.backward(1.0)
    none = set(str(n) for n in z["grad_none"])
    worst, seen = (0.0, ""), set()
    for n, ref_l2 in zip([str(n) for n in z["grad_names"]], z["grad_l2"]):
        g = eng.grad(n).cpu()
        if n in none:
            assert float(g.abs().max()) == 0.0, n
            continue
        if ref_l2 == 0.0:
            assert float(g.abs().max()) == 0.0, n
            continue
        if ref_l2 < 1e-6:                                  # mathematically zero in the reference (fp noise there)
            assert float(g.double().norm()) < 1e-6, n
            continue
        exp = z["grad." + n].reshape(-1).astype(np.float64)
        gs = sample_like(g.numpy(), z).astype(np.float64)
        e = float(np.linalg.norm(gs - exp) / np.linalg.norm(exp))
        worst = max(worst, (e, n))
        seen.add(n)
        assert e <= 2e-3, (n, e)
    print(f"tiny_pcd: worst relative L2 gradient error {worst[0]:.2e} at {worst[1]}")
    assert set(PCD_KEYS) <= seen and "additional_pos_embed.weight" in seen
    # all three rows of additional_pos_embed, each on its own
    ga, ea = eng.grad("additional_pos_embed.weight").cpu().double(), torch.from_numpy(z["grad.additional_pos_embed.weight"]).double()
    ea = ea.view(3, cfg.hidden_dim)
    for r in range(3):
        assert float((ga[r] - ea[r]).norm() / ea[r].norm()) <= 2e-3, r
    # one AdamW step with two distinct rates: pcl_backbone.* moves with lr_backbone, input_proj_pointnet.* with lr
    keys = [MLP + "0.weight", MLP + "3.weight", MLP + "6.bias", MLP + "9.weight", "input_proj_pointnet.weight",
            "input_proj_pointnet.bias", "additional_pos_embed.weight"]
    lr, lr_bb, wd = 1e-5, 3e-5, 1e-4
    before = {k: torch.from_numpy(sd_np[k]).clone() for k in keys}
    grads = {k: eng.grad(k).cpu() for k in keys}
    eng.adamw_step(lr, lr_bb, wd, step=1)
    after = eng.state_dict()
    for k in keys:
        assert W.is_backbone_param(k) == k.startswith("pcl_backbone.")
        p = before[k].clone().requires_grad_(True)
        opt = torch.optim.AdamW([p], lr=lr_bb if W.is_backbone_param(k) else lr, weight_decay=wd)
        p.grad = grads[k].clone()
        opt.step()
        err = float((after[k] - p.detach()).abs().max())
        assert err <= 1e-7 + 1e-6 * float(p.detach().abs().max()), (k, err)
        moved = float((after[k] - before[k]).abs().max())
        assert 0.5 * (lr_bb if W.is_backbone_param(k) else lr) <= moved <= 1.5 * (lr_bb if W.is_backbone_param(k) else lr), (k, moved)
    # the inference path sees the updated weights
    a1 = eng.forward_infer(torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d), pointcloud=_cloud(inp, d))
    assert torch.isfinite(a1).all()


# ---- 5. the reference's widths, winner-robust -------------------------------------------------------------------------------
def test_pcd_real_widths_forward_and_winner_robust_backward():
    """H = O = 512 on the tiny trunk, B = 2, P = 2051.  At this size the two largest values of a column can coincide to the last
    bit, so the winner is not unique: the library's winners are read back, each must attain the column maximum to 1e-5, and the
    torch gradient is taken through a gather at those winners."""
    cfg = tiny_config(use_pcd=True)
    assert cfg.pcd_hidden_dim == 512 and cfg.pcd_output_dim == 512
    B, P = 2, 2051
    sd_np = W.generate_state_dict(cfg, seed=17)
    inp = W.generate_inputs(cfg, B, seed=31, with_actions=True, num_points=P)
    xyz, rgb = torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"])
    eng = _engine(cfg, sd_np, B, training=True, max_points=P)
    d = eng.device
    qpos, img, cloud = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d), _cloud(inp, d)
    tok_ref, y_ref = _pointnet_ref(sd_np, xyz, rgb)
    tok = _token_row2(eng, qpos, img, cloud).double()
    err, bar = float((tok - tok_ref).abs().max()), 1e-4 * max(1.0, float(tok_ref.abs().max()))
    print(f"H=O=512 P={P}: token row 2 max err {err:.3e} (bar {bar:.3e})")
    assert err <= bar

    def step():
        eng.forward_train(qpos, img, torch.from_numpy(inp["actions"]).to(d), torch.from_numpy(inp["is_pad"]).to(d),
                          eps=torch.from_numpy(inp["eps"]).to(d), pointcloud=cloud)
        eng.zero_grad()
        eng.backward(1.0)
        return eng.grad_arena().clone()
    arena = step()
    win = eng.debug_tensor("pcd_argmax").view(torch.int32).view(B, cfg.pcd_output_dim).cpu()
    g_tok = eng.debug_tensor("pcd_dtoken").view(B, cfg.hidden_dim).cpu().double()
    assert int(win.min()) >= 0 and int(win.max()) < P
    won = torch.gather(y_ref, 1, win.long().unsqueeze(1)).squeeze(1)
    gap = float((y_ref.amax(dim=1) - won).max())
    print(f"largest (column maximum - value at the library's winner) = {gap:.3e}; |dL/dtoken| max {float(g_tok.abs().max()):.3e}")
    assert gap <= 1e-5 and float(g_tok.abs().max()) > 0
    params = {k: torch.from_numpy(sd_np[k]).double().requires_grad_(True) for k in PCD_KEYS}
    t, _ = _pointnet_ref(params, xyz, rgb, winners=win)
    t.backward(g_tok)
    for k in PCD_KEYS:
        g, ref = eng.grad(k).cpu().double(), params[k].grad
        e = float((g - ref).norm() / ref.norm())
        print(f"  {k}: relative L2 error {e:.2e}")
        assert e <= 2e-3, (k, e)
    assert torch.equal(step().view(torch.int32), arena.view(torch.int32))      # two identical steps, bitwise


# ---- 6. batch and capacity edges --------------------------------------------------------------------------------------------
def test_pcd_batch_and_capacity_edges_and_graph_replay():
    cfg = tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    sd_np = W.generate_state_dict(cfg, seed=5)
    MB, MP = 3, 64
    eng = _engine(cfg, sd_np, MB, max_points=MP)
    d = eng.device
    for B, P in ((1, 1), (MB, MP), (MB, 1), (1, MP), (2, 37)):       # one handle, clouds of another size every call
        inp = W.generate_inputs(cfg, B, seed=40 + B * 100 + P, num_points=P)
        qpos, img, cloud = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d), _cloud(inp, d)
        ref, _ = _pointnet_ref(sd_np, torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"]))
        tok = _token_row2(eng, qpos, img, cloud).double()
        assert float((tok - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max())), (B, P)
        a = eng.forward_infer(qpos, img, pointcloud=cloud)
        assert tuple(a.shape) == (B, cfg.num_queries, cfg.action_dim) and torch.isfinite(a).all()
    assert eng.read_flags() == 0
    # the captured graph replays the whole step, PointNet included, bit for bit
    replay = eng.capture_infer(MB, num_points=37)
    for t in range(2):
        inp = W.generate_inputs(cfg, MB, seed=70 + t, num_points=37)
        qpos, img, cloud = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d), _cloud(inp, d)
        a_g = replay(qpos, img, pointcloud=cloud).clone()
        a_e = eng.forward_infer(qpos, img, pointcloud=cloud).clone()
        assert torch.equal(a_g, a_e)
    with pytest.raises(ValueError):
        replay(qpos, img)
    from actmi.engine import InferPipeline
    with pytest.raises(NotImplementedError):
        InferPipeline(eng, MB)


# ---- 7. errors, no fault ----------------------------------------------------------------------------------------------------
def test_pcd_errors_are_codes_and_exceptions():
    lib = L.load()
    cfg = tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    sd_np = W.generate_state_dict(cfg, seed=5)
    eng = _engine(cfg, sd_np, 2, max_points=16)
    d = eng.device
    inp = W.generate_inputs(cfg, 2, seed=3, num_points=16)
    qpos, img, cloud = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d), _cloud(inp, d)
    out = torch.full((2, cfg.num_queries, cfg.action_dim), 7.0, device=d)

    def raw_forward(B):
        return lib.actmi_forward_infer(eng.h, C.c_void_p(qpos.data_ptr()), C.c_void_p(img.data_ptr()), L.IMG_U8_NHWC, B,
                                       C.c_void_p(out.data_ptr()), eng._sp())
    # nothing bound: ACTMI_E_STATE, and nothing was launched (the output buffer is untouched)
    assert raw_forward(2) == -4 and b"actmi_set_pointcloud" in lib.actmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    # a binding is consumed by one forward
    eng.forward_infer(qpos, img, pointcloud=cloud)
    assert raw_forward(2) == -4
    # bound for another batch
    assert lib.actmi_set_pointcloud(eng.h, C.c_void_p(cloud["xyz"].data_ptr()), C.c_void_p(cloud["rgb"].data_ptr()), 1, 16) == 0
    assert raw_forward(2) == -4 and b"1 samples" in lib.actmi_last_error(eng.h)
    # more points than the workspace holds
    assert lib.actmi_set_pointcloud(eng.h, C.c_void_p(cloud["xyz"].data_ptr()), C.c_void_p(cloud["rgb"].data_ptr()), 2, 17) == -1
    assert b"max_points" in lib.actmi_last_error(eng.h)
    big = {k: torch.zeros(2, 17, 3, device=d) for k in ("xyz", "rgb")}
    with pytest.raises(ValueError, match="max_points"):
        eng.forward_infer(qpos, img, pointcloud=big)
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img)                                                   # no clouds
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, pointcloud={"xyz": cloud["xyz"], "rgb": cloud["rgb"][:, :5]})
    with pytest.raises(TypeError):
        eng.forward_infer(qpos, img, pointcloud={"xyz": cloud["xyz"].double(), "rgb": cloud["rgb"]})
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, pointcloud={"xyz": cloud["xyz"].cpu(), "rgb": cloud["rgb"]})
    # a plain handle has no clouds to bind
    plain_cfg = tiny_config()
    plain = _engine(plain_cfg, W.generate_state_dict(plain_cfg, seed=5), 2)
    assert lib.actmi_set_pointcloud(plain.h, C.c_void_p(cloud["xyz"].data_ptr()), C.c_void_p(cloud["rgb"].data_ptr()), 2, 16) == -4
    with pytest.raises(ValueError):
        plain.forward_infer(qpos, img, pointcloud=cloud)
    # the guarded struct
    c = L.ActmiConfig(struct_size=C.sizeof(L.ActmiConfig), num_cams=2, image_h=64, image_w=96, base_width=8, hidden_dim=64, nheads=4,
                      dim_feedforward=128, enc_layers=2, dec_layers=2, num_queries=8, state_dim=14, action_dim=16, latent_dim=32,
                      has_cvae_encoder=1, max_batch=1, enable_training=0, kl_weight=10.0)
    pc = L.ActmiPcdConfig(struct_size=12, max_points=8, hidden_dim=64, output_dim=64)
    h = C.c_void_p()
    assert lib.actmi_create_ex(C.byref(c), C.byref(pc), C.byref(h)) == -1 and not h.value
    assert b"actmi_pcd_config.struct_size is 12" in lib.actmi_last_error(None)
    pc = L.ActmiPcdConfig(struct_size=16, max_points=8, hidden_dim=48, output_dim=64)          # not a multiple of 32
    assert lib.actmi_create_ex(C.byref(c), C.byref(pc), C.byref(h)) == -1 and not h.value
    # pcd == NULL is actmi_create
    assert lib.actmi_create_ex(C.byref(c), None, C.byref(h)) == 0 and lib.actmi_num_params(h) == plain_num_params(lib, c)
    lib.actmi_destroy(h)
    # a checkpoint trained without the branch does not load into an engine with it: the missing keys are named
    with pytest.raises(RuntimeError, match="input_proj_pointnet.weight"):
        eng.load_state_dict(W.generate_state_dict(plain_cfg, seed=5))
    # ... and the policy surface
    from policy import ACTPolicy
    pol = ACTPolicy({"use_pcd": True, "pcd_hidden_dim": 64, "pcd_output_dim": 64, "max_points": 16, "kl_weight": 10, "lr": 1e-5,
                     "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4,
                     "camera_names": ["a", "b"], "image_h": 64, "image_w": 96, "base_width": 8, "training": False}, max_batch=2)
    with pytest.raises(ValueError):
        pol(qpos, img)
    assert torch.isfinite(pol(qpos, img, pointcloud=cloud)).all()
    with pytest.raises(NotImplementedError):
        ACTPolicy({"use_depth": True, "kl_weight": 10, "lr": 1e-5})


def plain_num_params(lib, c):
    h = C.c_void_p()
    assert lib.actmi_create(C.byref(c), C.byref(h)) == 0
    n = lib.actmi_num_params(h)
    lib.actmi_destroy(h)
    return n
