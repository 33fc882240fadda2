"""Ragged point clouds (pointcloud["n"], actmi_set_pointcloud_n): the column maximum with per-sample counts on its own, padding
that cannot be seen in any output bit, the ragged golden fixture made by the reference one sample at a time
(tests/golden/tiny_pcd_ragged.npz, tools/gen_golden_pcd_ragged.py), graph replay with a static counts buffer, the host-fed
pipeline, the error returns, and episode files -> loader -> prefetcher -> policy.

Tolerances are those of tests/test_gpu_pointcloud.py: 1e-4 absolute on a_hat, 1e-4 * max(1, |ref|) on tokens and losses, 2e-3
relative L2 on gradients, the generator's MIN_GAP on winner uniqueness."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_fixture, regenerate, sample_like  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402
from actmi import weights as W  # noqa: E402
from actmi.config import tiny_config  # noqa: E402
from actmi.engine import ACTEngine, InferPipeline  # noqa: E402

ATOL = 1e-4
MIN_GAP = 1e-4
MLP = "pcl_backbone.pointnet._mlp."
PCD_KEYS = [MLP + f"{i}.{s}" for i in (0, 3, 6, 9) for s in ("weight", "bias")] + ["input_proj_pointnet.weight",
                                                                                 "input_proj_pointnet.bias"]


def _engine(cfg, sd_np, max_batch, training=False, max_points=64):
    eng = ACTEngine(cfg, max_batch=max_batch, training=training, max_points=max_points)
    eng.load_state_dict(sd_np)
    eng.finalize()
    return eng


def _i32(v, dev):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def _padded(xyz, rgb, counts, P, fill, seed=0):
    """clouds [B, P, 3] whose rows below counts[b] are those of xyz / rgb and whose other rows hold zeros or finite random points"""
    B = xyz.shape[0]
    g = torch.Generator().manual_seed(seed)
    if fill == "zeros":
        ox, oc = torch.zeros(B, P, 3), torch.zeros(B, P, 3)
    else:
        ox, oc = torch.randn(B, P, 3, generator=g) * 3.0, torch.rand(B, P, 3, generator=g) * 255.0
    for b, n in enumerate(counts):
        ox[b, :n], oc[b, :n] = xyz[b, :n], rgb[b, :n]
    return ox.contiguous(), oc.contiguous()


def _cloud(xyz, rgb, dev, n=None):
    c = {"xyz": xyz.to(dev), "rgb": rgb.to(dev)}
    if n is not None:
        c["n"] = _i32(n, dev)
    return c


def _token_row2(eng, qpos, img, cloud):
    eng.debug_stop_after("src")
    eng.forward_infer(qpos, img, pointcloud=cloud)
    src = eng.debug_tensor("src").view(qpos.shape[0], eng.cfg.num_tokens, eng.cfg.hidden_dim).cpu()
    eng.debug_stop_after("")
    return src[:, 2]


def _check_losses(out, z, tag):
    for k in ("l1", "kl", "loss"):
        got, exp = float(out[k]), float(z["train." + k][0])
        print(f"{tag} {k}: hip {got:.6f} ref {exp:.6f}")
        assert abs(got - exp) <= 1e-4 * max(1.0, abs(exp)), k
    for k in ("a_hat", "mu", "logvar"):
        assert np.abs(out[k].cpu().numpy() - z["train." + k]).max() <= 1e-4, k


def _check_grads(eng, z, tag):
    none = set(str(n) for n in z["grad_none"])
    worst, seen = (0.0, ""), set()
    for n, ref_l2 in zip([str(n) for n in z["grad_names"]], z["grad_l2"]):
        g = eng.grad(n).cpu()
        if n in none or ref_l2 == 0.0:
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
    print(f"{tag}: worst relative L2 gradient error {worst[0]:.2e} at {worst[1]}")
    assert set(PCD_KEYS) <= seen and "additional_pos_embed.weight" in seen


@functools.lru_cache(maxsize=None)
def _ragged():
    """the ragged fixture, its regenerated weights and inputs (hashes checked), and one training engine for the tests that share it"""
    z, cfg = load_fixture("tiny_pcd_ragged")
    B, P = int(z["batch"]), int(z["points"])
    sd_np = W.generate_state_dict(cfg, int(z["seed_w"]))
    inp = W.generate_inputs(cfg, B, int(z["seed_in"]), with_actions=True, num_points=P)
    for k in z.files:
        if k.startswith("sha:"):
            a = inp[k[4:]] if k[4:] in inp else sd_np[k[4:]]
            assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(z[k]), f"regenerated {k[4:]} differs"
    counts = [int(v) for v in z["counts"]]
    assert (B, P, counts) == (3, 64, [64, 5, 37]) and float(z["top2_gap"]) >= MIN_GAP
    eng = _engine(cfg, sd_np, B, training=True, max_points=P)
    d = eng.device
    t = {k: torch.from_numpy(inp[k]).to(d) for k in ("qpos", "image_u8", "actions", "is_pad")}
    t["eps"] = torch.from_numpy(z["train.eps"]).to(d)
    return z, cfg, sd_np, inp, counts, eng, t


@functools.lru_cache(maxsize=None)
def _ragged_infer_engine():
    """an inference-only engine with the ragged fixture's weights (graph capture, host-fed pipeline)"""
    z, cfg, sd_np = _ragged()[:3]
    return _engine(cfg, sd_np, int(z["batch"]), max_points=int(z["points"]))


# ---- 1. the maximum over the first n_b points -------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,pad", [(64, 0), (512, 0), (64, 4)])
@pytest.mark.parametrize("P", [1, 37, 257, 2051])
def test_colmax_with_counts_is_exact_and_never_sees_the_padding(P, O, pad):
    B, ld = 3, O + pad
    g = torch.Generator().manual_seed(P * 5 + O + pad)
    clean = torch.randn(B, P, ld, generator=g)
    for counts in [[1, P, P // 2 + 1]] + ([[3, 3, 3]] if P == 2051 else []):          # [3, 3, 3]: whole splits hold no point
        x = clean.clone()
        for b, n in enumerate(counts):
            if n >= 3:                                     # a tie between the first and the last valid row, winning many columns
                x[b, n - 1] = x[b, 0]
                x[b, [0, n - 1], ::2] += 6.0
            x[b, n:] += 20.0                               # padding: larger than any point ...
            if n < P:
                x[b, n + (P - n) // 2, 5] = float("nan")   # ... and one NaN
        ref_v = torch.stack([x[b, :n, :O].max(dim=0).values for b, n in enumerate(counts)])
        ref_i = torch.stack([(x[b, :n, :O] == ref_v[b]).int().argmax(dim=0).int() for b, n in enumerate(counts)])
        assert torch.isfinite(ref_v).all()
        xd, cd = x.cuda(), _i32(counts, "cuda")
        v, i = ops.colmax(xd, O, counts=cd)
        assert torch.equal(v.cpu(), ref_v) and torch.equal(i.cpu(), ref_i), counts
        assert bool((i.cpu() < torch.tensor(counts).view(B, 1)).all()) and int(i.min()) >= 0
        if counts[1] >= 3:
            assert int((ref_i[1] == 0).sum()) >= O // 4                                 # the ties were really there
        v1, i1 = ops.colmax(xd, O, split=False, counts=cd)                              # one split: the same answer
        assert torch.equal(v1.cpu(), ref_v) and torch.equal(i1.cpu(), ref_i)
        v2, i2 = ops.colmax(xd, O, counts=cd)                                           # twice: bit for bit
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(i2, i)
    # counts=None is today's call: all P rows, and so is a count of P (or more: clamped) for every sample
    full_v = clean[:, :, :O].max(dim=1).values
    full_i = (clean[:, :, :O] == full_v.unsqueeze(1)).int().argmax(dim=1).int()
    cdev = clean.cuda()
    v0, i0 = ops.colmax(cdev, O)
    vn, in_ = ops.colmax(cdev, O, counts=None)
    vp, ip = ops.colmax(cdev, O, counts=_i32([P, P + 7, P], "cuda"))
    for vv, ii in ((v0, i0), (vn, in_), (vp, ip)):
        assert torch.equal(vv.cpu(), full_v) and torch.equal(ii.cpu(), full_i)
    # a count below 1 is clamped to one point
    vz, iz = ops.colmax(cdev, O, counts=_i32([0, -5, 1], "cuda"))
    assert torch.equal(vz.cpu(), clean[:, 0, :O]) and int(iz.abs().max()) == 0
    with pytest.raises(ValueError):
        ops.colmax(cdev, O, counts=torch.ones(B, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.colmax(cdev, O, counts=_i32([1] * (B + 1), "cuda"))


# ---- 2. the dense fixture behind padding --------------------------------------------------------------------------------------------
def test_dense_fixture_with_extra_rows_and_full_counts_matches_the_reference():
    z, cfg = load_fixture("tiny_pcd")
    sd_np, inp = regenerate(z, cfg)
    B, P, EXTRA = int(z["batch"]), int(z["points"]), 11
    xyz, rgb = _padded(torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"]), [P] * B, P + EXTRA, "random", seed=3)
    assert float(xyz[:, P:].abs().min()) > 0 and torch.isfinite(xyz).all() and torch.isfinite(rgb).all()
    eng = _engine(cfg, sd_np, B, training=True, max_points=P + EXTRA)
    d = eng.device
    cloud = _cloud(xyz, rgb, d, n=[P] * B)
    qpos, img = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d)
    a = eng.forward_infer(qpos, img, pointcloud=cloud).cpu().numpy()
    err = np.abs(a - z["infer.a_hat"]).max()
    print(f"tiny_pcd + {EXTRA} padding rows, n = P: max|a_hat - ref| = {err:.3e}")
    assert err <= ATOL
    out = eng.forward_train(qpos, img, torch.from_numpy(inp["actions"]).to(d), torch.from_numpy(inp["is_pad"]).to(d),
                            eps=torch.from_numpy(z["train.eps"]).to(d), pointcloud=cloud)
    _check_losses(out, z, "tiny_pcd padded")
    eng.zero_grad()
    eng.backward(1.0)
    _check_grads(eng, z, "tiny_pcd padded")
    win = eng.debug_tensor("pcd_argmax").view(torch.int32)
    assert int(win.min()) >= 0 and int(win.max()) < P


# ---- 3. padding is inert, bit for bit ----------------------------------------------------------------------------------------------------
def test_what_the_padding_rows_hold_changes_no_bit():
    z, cfg, sd_np, inp, counts, eng, t = _ragged()
    d = eng.device
    P = int(z["points"])
    src_xyz, src_rgb = torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"])
    res = []
    for fill in ("zeros", "random"):
        xyz, rgb = _padded(src_xyz, src_rgb, counts, P, fill, seed=11)
        cloud = _cloud(xyz, rgb, d, n=counts)
        a = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=cloud).clone()
        out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"], pointcloud=cloud)
        eng.zero_grad()
        eng.backward(1.0)
        res.append((a, {k: out[k].clone() for k in ("l1", "kl", "loss")}, eng.grad_arena().clone(), xyz))
    assert not torch.equal(res[0][3], res[1][3])                       # the fillings did differ
    assert torch.isfinite(res[0][0]).all() and torch.equal(res[0][0], res[1][0])
    for k in ("l1", "kl", "loss"):
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    assert float(res[0][2].abs().max()) > 0 and torch.equal(res[0][2].view(torch.int32), res[1][2].view(torch.int32))
    # and the counts are what does it: the same random filling read as points gives another answer
    xyz, rgb = _padded(src_xyz, src_rgb, counts, P, "random", seed=11)
    a_all = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=_cloud(xyz, rgb, d))
    assert not torch.equal(a_all, res[0][0])


# ---- 4. the ragged fixture ---------------------------------------------------------------------------------------------------------------
def test_ragged_batch_matches_the_reference_run_one_sample_at_a_time():
    z, cfg, sd_np, inp, counts, eng, t = _ragged()
    d = eng.device
    B, P = int(z["batch"]), int(z["points"])
    src_xyz, src_rgb = torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"])
    xyz, rgb = _padded(src_xyz, src_rgb, counts, P, "zeros")
    cloud = _cloud(xyz, rgb, d, n=counts)
    a = eng.forward_infer(t["qpos"], t["image_u8"], pointcloud=cloud).cpu().numpy()
    err = np.abs(a - z["infer.a_hat"]).max()
    print(f"tiny_pcd_ragged n = {counts}: max|a_hat - ref| = {err:.3e}")
    assert err <= ATOL
    tok = _token_row2(eng, t["qpos"], t["image_u8"], cloud).numpy()
    exp = z["stage.src_row2"]
    tol = 1e-4 * max(1.0, float(np.abs(exp).max()))
    e2 = np.abs(tok - exp).max()
    print(f"tiny_pcd_ragged: token row 2 max err {e2:.3e} (|row| max {np.abs(exp).max():.3f})")
    assert tok.shape == exp.shape and e2 <= tol and np.abs(exp).max() > 0.05
    # every sample's token is that of its truncated cloud alone
    for b, n in enumerate(counts):
        one = _cloud(src_xyz[b:b + 1, :n].contiguous(), src_rgb[b:b + 1, :n].contiguous(), d)
        tb = _token_row2(eng, t["qpos"][b:b + 1], t["image_u8"][b:b + 1], one).numpy()[0]
        assert np.abs(tok[b] - tb).max() <= 1e-4 * max(1.0, float(np.abs(tb).max())), b
    out = eng.forward_train(t["qpos"], t["image_u8"], t["actions"], t["is_pad"], eps=t["eps"], pointcloud=cloud)
    _check_losses(out, z, "tiny_pcd_ragged")
    eng.zero_grad()
    eng.backward(1.0)
    _check_grads(eng, z, "tiny_pcd_ragged")
    win = eng.debug_tensor("pcd_argmax").view(torch.int32).view(B, cfg.pcd_output_dim).cpu()
    assert bool((win < torch.tensor(counts).view(B, 1)).all()) and int(win.min()) >= 0


# ---- 5. a captured graph reads the counts of every replay ----------------------------------------------------------------------------------
def test_captured_forward_sees_new_counts_on_every_replay():
    z, cfg = _ragged()[:2]
    eng = _ragged_infer_engine()
    d = eng.device
    B, P = int(z["batch"]), int(z["points"])
    replay = eng.capture_infer(B, num_points=P)
    sn = replay.static_cloud["n"]
    assert sn.dtype == torch.int32 and tuple(sn.shape) == (B,) and sn.tolist() == [P] * B
    outs = []
    for step, n in enumerate(([64, 5, 37], [9, 64, 1])):
        g = W.generate_inputs(cfg, B, seed=90 + step, num_points=P)
        qpos, img = torch.from_numpy(g["qpos"]).to(d), torch.from_numpy(g["image_u8"]).to(d)
        cloud = _cloud(torch.from_numpy(g["pcd_xyz"]), torch.from_numpy(g["pcd_rgb"]), d, n=n)
        a_g = replay(qpos, img, pointcloud=cloud).clone()
        assert replay.static_cloud["n"].tolist() == n
        a_e = eng.forward_infer(qpos, img, pointcloud=cloud).clone()
        assert torch.equal(a_g, a_e), n
        outs.append(a_g)
    assert not torch.equal(outs[0], outs[1])
    # without "n" the buffer is refilled: every row a point
    dense = {k: cloud[k] for k in ("xyz", "rgb")}
    a_g = replay(qpos, img, pointcloud=dense).clone()
    assert replay.static_cloud["n"].tolist() == [P] * B
    assert torch.equal(a_g, eng.forward_infer(qpos, img, pointcloud=dict(dense, n=_i32([P] * B, d))))
    assert torch.equal(a_g, eng.forward_infer(qpos, img, pointcloud=dense)) and not torch.equal(a_g, outs[1])
    with pytest.raises(TypeError):
        replay(qpos, img, pointcloud=dict(dense, n=torch.ones(B, device=d)))
    with pytest.raises(ValueError):
        replay(qpos, img, pointcloud=dict(dense, n=_i32([1] * (B - 1), d)))


# ---- 6. the host-fed pipeline ----------------------------------------------------------------------------------------------------------------
def test_infer_pipeline_feeds_clouds_and_counts_from_the_host():
    z, cfg = _ragged()[:2]
    eng = _ragged_infer_engine()
    d = eng.device
    B, P = int(z["batch"]), int(z["points"])
    with pytest.raises(NotImplementedError):
        InferPipeline(eng, B)
    pipe = InferPipeline(eng, B, num_points=P, copy_stream_candidates=1)
    ns = ([64, 5, 37], [1, 64, 20], [33, 2, 64])
    host = []
    for step, n in enumerate(ns):
        g = W.generate_inputs(cfg, B, seed=120 + step, num_points=P)
        xyz, rgb = _padded(torch.from_numpy(g["pcd_xyz"]), torch.from_numpy(g["pcd_rgb"]), n, P, "zeros")
        host.append((torch.from_numpy(g["qpos"]).pin_memory(), torch.from_numpy(g["image_u8"]).pin_memory(),
                     {"xyz": xyz.pin_memory(), "rgb": rgb.pin_memory(), "n": torch.tensor(n, dtype=torch.int32).pin_memory()}))
    with pytest.raises(ValueError):
        pipe.feed(host[0][0], host[0][1])                              # no clouds
    for bad in ([0, 5, 37], [64, 65, 1]):
        with pytest.raises(ValueError):
            pipe.feed(host[0][0], host[0][1], cloud_host=dict(host[0][2], n=torch.tensor(bad, dtype=torch.int32)))
    with pytest.raises(ValueError):
        pipe.feed(host[0][0], host[0][1], cloud_host=dict(host[0][2], n=torch.tensor(ns[0], dtype=torch.int64)))
    pipe.feed(host[0][0], host[0][1], cloud_host=host[0][2])
    outs = []
    for step in range(3):
        outs.append(pipe.step(next_inputs=host[step + 1] if step + 1 < 3 else None).clone())
    torch.cuda.synchronize()
    for step in range(3):
        q, i, c = host[step]
        exp = eng.forward_infer(q.to(d), i.to(d), pointcloud={k: v.to(d) for k, v in c.items()})
        assert torch.equal(outs[step], exp), step
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert eng.read_flags() == 0


# ---- 7. errors, no fault ---------------------------------------------------------------------------------------------------------------------
def test_counts_errors_are_codes_and_exceptions():
    lib = L.load()
    cfg = tiny_config(use_pcd=True, pcd_hidden_dim=64, pcd_output_dim=64)
    sd_np = W.generate_state_dict(cfg, seed=5)
    eng = _engine(cfg, sd_np, 2, max_points=16)
    d = eng.device
    inp = W.generate_inputs(cfg, 2, seed=3, num_points=16)
    qpos, img = torch.from_numpy(inp["qpos"]).to(d), torch.from_numpy(inp["image_u8"]).to(d)
    cloud = _cloud(torch.from_numpy(inp["pcd_xyz"]), torch.from_numpy(inp["pcd_rgb"]), d, n=[16, 4])
    out = torch.full((2, cfg.num_queries, cfg.action_dim), 7.0, device=d)
    px, pr, pn = (C.c_void_p(cloud[k].data_ptr()) for k in ("xyz", "rgb", "n"))

    def raw_forward(B):
        return lib.actmi_forward_infer(eng.h, C.c_void_p(qpos.data_ptr()), C.c_void_p(img.data_ptr()), L.IMG_U8_NHWC, B,
                                       C.c_void_p(out.data_ptr()), eng._sp())
    # more points than the workspace holds
    assert lib.actmi_set_pointcloud_n(eng.h, px, pr, pn, 2, 17) == -1 and b"max_points" in lib.actmi_last_error(eng.h)
    assert lib.actmi_set_pointcloud_n(eng.h, px, None, pn, 2, 16) == -1
    # bound for another batch: ACTMI_E_STATE before anything is launched (the output buffer is untouched)
    assert lib.actmi_set_pointcloud_n(eng.h, px, pr, pn, 1, 16) == 0
    assert raw_forward(2) == -4 and b"1 samples" in lib.actmi_last_error(eng.h)
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    # counts == NULL is actmi_set_pointcloud; a binding serves one forward
    assert lib.actmi_set_pointcloud_n(eng.h, px, pr, None, 2, 16) == 0 and raw_forward(2) == 0
    dense = out.clone()
    assert raw_forward(2) == -4
    assert lib.actmi_set_pointcloud_n(eng.h, px, pr, pn, 2, 16) == 0 and raw_forward(2) == 0
    torch.cuda.synchronize()
    assert torch.equal(dense, eng.forward_infer(qpos, img, pointcloud={k: cloud[k] for k in ("xyz", "rgb")}))
    assert torch.equal(out, eng.forward_infer(qpos, img, pointcloud=cloud)) and not torch.equal(out, dense)
    # the Python surface
    with pytest.raises(TypeError):
        eng.forward_infer(qpos, img, pointcloud=dict(cloud, n=cloud["n"].float()))
    with pytest.raises(TypeError):
        eng.forward_infer(qpos, img, pointcloud=dict(cloud, n=cloud["n"].long()))
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, pointcloud=dict(cloud, n=cloud["n"].cpu()))
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, pointcloud=dict(cloud, n=_i32([16, 4, 1], d)))
    with pytest.raises(ValueError):
        eng.forward_infer(qpos, img, pointcloud=dict(cloud, n=_i32([16, 0, 4, 0], d)[::2]))      # not contiguous
    # a plain handle has no clouds to bind
    plain_cfg = tiny_config()
    plain = _engine(plain_cfg, W.generate_state_dict(plain_cfg, seed=5), 2)
    assert lib.actmi_set_pointcloud_n(plain.h, px, pr, pn, 2, 16) == -4
    with pytest.raises(ValueError):
        InferPipeline(plain, 2, num_points=16)
    assert eng.read_flags() == 0


# ---- 8. episode files -> loader -> prefetcher -> policy ----------------------------------------------------------------------------------------
def test_ragged_cloud_episodes_train_end_to_end(tmp_path):
    from actmi.data import DevicePrefetcher, load_data
    from imitate_episodes import forward_pass
    from policy import ACTPolicy
    cams, H, Wd, T, name = ["a", "b"], 64, 96, 6, "fused_pcd"
    rng = np.random.default_rng(0)
    n_max = [13, 7, 16]                                              # every episode pads to its own largest cloud
    for e in range(3):
        ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32),
              "/observations/qvel": np.zeros((T, 14), np.float32), "/action": rng.standard_normal((T, 16)).astype(np.float32),
              "attrs_sim": np.array(True)}
        for c in cams:
            ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8)
        n = rng.integers(1, n_max[e] + 1, T)
        n[0] = n_max[e]
        mask = np.arange(n_max[e])[None, :] < n[:, None]
        ep[f"/observations/pointcloud/{name}/xyz"] = (rng.standard_normal((T, n_max[e], 3)) * mask[..., None]).astype(np.float32)
        ep[f"/observations/pointcloud/{name}/rgb"] = (rng.integers(1, 256, (T, n_max[e], 3)) * mask[..., None]).astype(np.uint8)
        ep[f"/observations/pointcloud/{name}/padding_mask"] = mask
        np.savez(tmp_path / f"episode_{e}.npz", **ep)
    train_dl, _, _, _ = load_data(str(tmp_path), lambda n: True, cams, 3, 3, 8, policy_class="ACT", num_workers=0, train_ratio=0.67,
                                  rng=np.random.default_rng(1), pointcloud_names=[name], use_pcd=True, max_points=16)
    it = DevicePrefetcher(iter(train_dl))
    batch = next(it)
    for _ in range(8):                                               # a batch whose samples really differ in their counts
        if len(set(batch[6].tolist())) > 1:
            break
        batch = next(it)
    assert len(batch) == 7 and len(set(batch[6].tolist())) > 1
    image, qpos, action, is_pad, xyz, rgb, n = batch
    assert n.dtype == torch.int32 and n.is_cuda and tuple(n.shape) == (3,) and xyz.is_cuda and rgb.is_cuda
    assert xyz.dtype == torch.float32 and rgb.dtype == torch.float32 and tuple(xyz.shape) == tuple(rgb.shape) == (3, xyz.shape[1], 3)
    assert image.dtype == torch.uint8 and float(rgb.max()) > 1.0 and 1 <= int(n.min()) and int(n.max()) <= xyz.shape[1] <= 16
    pol = ACTPolicy({"use_pcd": True, "pcd_hidden_dim": 64, "pcd_output_dim": 64, "max_points": 16, "kl_weight": 10, "lr": 1e-5,
                     "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4,
                     "camera_names": cams, "image_h": H, "image_w": Wd, "base_width": 8}, max_batch=3)
    pol.train()
    pol.train_dropout = 0.0                                           # (the two calls below must draw the same masks: none)
    eps = torch.randn(3, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(2)).cuda()
    pol.next_eps = eps
    got = forward_pass(batch, pol)
    pol.next_eps = eps
    exp = pol(qpos, image, action, is_pad, pointcloud={"xyz": xyz, "rgb": rgb, "n": n})
    for k in ("l1", "kl", "loss"):
        print(f"end to end {k}: {float(got[k]):.6f}")
        assert np.isfinite(float(got[k])) and float(got[k]) == float(exp[k]), k
    # the counts reached the maximum: the same batch read as dense clouds (zero rows as points) gives another loss
    pol.next_eps = eps
    dense = pol(qpos, image, action, is_pad, pointcloud={"xyz": xyz, "rgb": rgb})
    assert float(dense["loss"]) != float(exp["loss"])
