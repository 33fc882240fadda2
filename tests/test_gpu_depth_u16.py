"""Raw 16-bit depth frames: the per-sample min / max kernel, the u16 depth stem, and the engine / graph / pipeline / dataset paths
that feed them.

Every equality here is ``torch.equal``.  That bar is derived, not measured: u16 -> fp32 is exact; the loader performs the same
correctly rounded fp32 subtractions and divisions as torch on the CPU (no fast-math in the build); everything downstream of
the normalised patch is the code of the f32 path, which is bitwise repeatable.  The reference side of every case is the
reference dataset's line (utils_arm_gripper_all.py:189) restated on the CPU, per sample over all of its depth cameras:
``f = d.float(); n[b] = (f[b] - f[b].min()) / (f[b].max() - f[b].min() + 1e-6)``, uploaded as float32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_fixture, regenerate  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.engine import ACTEngine, InferPipeline  # noqa: E402

_FIX = {}


def _fixture():
    if not _FIX:
        z, cfg = load_fixture("tiny_depth")
        sd_np, inp = regenerate(z, cfg)
        _FIX["v"] = (cfg, sd_np, inp)
    return _FIX["v"]


def _normalise(d_u16):
    """the reference dataset's normalisation, per sample, in CPU float32"""
    f = d_u16.float()
    n = torch.empty_like(f)
    for b in range(f.shape[0]):
        n[b] = (f[b] - f[b].min()) / (f[b].max() - f[b].min() + 1e-6)
    return n


def _raw_batch(B, Cd, H, W, seed):
    """uint16 [B, Cd, 1, H, W] (CPU): every sample its own range; the extremes planted at the very first and the very last element
    (sample 0: min first / max last, sample 1: the reverse); with B >= 3 the LAST sample is constant and sample 1 spans 0 and 65535
    (values >= 32768 catch a signed read)"""
    rng = np.random.default_rng(seed)
    d = np.empty((B, Cd * H * W), dtype=np.int64)
    for b in range(B):
        lo = 300 + 4000 * b
        hi = 36000 + 5000 * b                                         # above 32767 in every sample
        d[b] = rng.integers(lo + 1, hi, size=d.shape[1])
        d[b, ::13] = lo + 1                                           # holes of a depth sensor: many equal values
        first, last = (lo, hi) if b % 2 == 0 else (hi, lo)
        if b == 1:
            first, last = 65535, 0
        d[b, 0], d[b, -1] = first, last
    if B >= 3:
        d[B - 1] = 41234
    return torch.from_numpy(d.astype(np.uint16)).view(B, Cd, 1, H, W)


# ---- 1. min / max ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cd,H,W", [(1, 1, 7, 9), (3, 1, 30, 43), (3, 2, 64, 96), (2, 4, 33, 65)])
def test_depth_minmax_equals_amin_amax_per_sample(B, Cd, H, W):
    # (3, 1, 30, 43): n = 1290, samples 1 and 2 start on a 4-byte, not a 16-byte, boundary and n is no multiple of 8
    d = _raw_batch(B, Cd, H, W, seed=B * 1000 + H)
    f = d.float().view(B, -1)
    exp = torch.stack([f.amin(1), f.amax(1)], dim=1)
    assert len({tuple(r.tolist()) for r in exp}) == B                 # every sample its own range: a batch-global reduction shows
    if B >= 2:
        assert exp[1].tolist() == [0.0, 65535.0]
    if B >= 3:
        assert exp[B - 1, 0] == exp[B - 1, 1] == 41234.0
    got = ops.depth_minmax(d.cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 2)
    print(f"depth_minmax B{B} Cd{Cd} {H}x{W}: got {got.cpu().tolist()} expected {exp.tolist()}")
    assert torch.equal(got.cpu(), exp)
    # a view that starts 2 bytes into an allocation: the head elements in front of the first 16-byte boundary
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint16), d.numpy().reshape(-1)])).cuda()
    shifted = flat[1:].view(B, -1)
    assert shifted.data_ptr() % 16 == 2 and torch.equal(ops.depth_minmax(shifted).cpu(), exp)


# ---- 2. the u16 stem against the f32 stem -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [8, 64])
@pytest.mark.parametrize("B,Cd,H,W", [(1, 1, 7, 9), (3, 2, 30, 50), (3, 2, 64, 96)])
def test_conv1_depth_u16_is_bitwise_the_f32_stem_on_the_normalised_batch(B, Cd, H, W, Cout):
    d = _raw_batch(B, Cd, H, W, seed=7 * H + Cout + B)
    n = _normalise(d)
    g = torch.Generator().manual_seed(H * 131 + W * 7 + Cout + B)
    w = (torch.randn(Cd, Cout, 1, 7, 7, generator=g) * (2.0 / 49) ** 0.5).cuda()
    scale = ((0.5 + torch.rand(Cd, Cout, generator=g)) * (torch.randint(0, 2, (Cd, Cout), generator=g) * 2 - 1).float()).cuda()
    bias = (0.3 * torch.randn(Cd, Cout, generator=g)).cuda()
    dd = d.cuda()
    got = ops.conv1_depth(dd, w, scale, bias, lohi=ops.depth_minmax(dd))
    exp = ops.conv1_depth(n.cuda(), w, scale, bias)
    assert torch.isfinite(got).all()
    diff = int((got.view(torch.int32) != exp.view(torch.int32)).sum())
    print(f"conv1_depth u16 B{B} Cd{Cd} {H}x{W} Cout{Cout}: {diff} of {got.numel()} elements differ from the f32 stem")
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))
    if B >= 3:
        # the constant sample normalises to 0 everywhere, the stem sees -1: the all-(-1)-input result, not NaN
        minus1 = ops.conv1_depth(torch.zeros(1, Cd, 1, H, W, device="cuda"), w, scale, bias)
        assert torch.equal(got[:, B - 1].view(torch.int32), minus1[:, 0].view(torch.int32))
    with pytest.raises(ValueError):
        ops.conv1_depth(dd, w, scale, bias)                           # u16 without its table


# ---- 3. engine inference ---------------------------------------------------------------------------------------------------------------
def _engine(training=False, max_batch=2):
    cfg, sd_np, _ = _fixture()
    eng = ACTEngine(cfg, max_batch=max_batch, training=training)
    eng.load_state_dict(sd_np)
    eng.finalize()
    return eng


def _frames(cfg, seed):
    """(qpos, image u8, depth u16, depth normalised f32) of a B = 2 step, CPU"""
    _, _, inp = _fixture()
    g = torch.Generator().manual_seed(seed)
    qpos = torch.from_numpy(inp["qpos"])[:2] + 0.01 * seed
    img = torch.randint(0, 256, (2, cfg.num_cams, cfg.image_h, cfg.image_w, 3), generator=g, dtype=torch.uint8)
    d = _raw_batch(2, cfg.num_depth_cams, cfg.image_h, cfg.image_w, seed=seed)
    return qpos, img, d, _normalise(d)


def test_engine_infer_u16_depth_is_bitwise_the_f32_path_eager_graph_and_alternating():
    eng = _engine()
    cfg, dev = eng.cfg, eng.device
    qpos, img, d, n = (t.to(dev) for t in _frames(cfg, 1))
    a_f32 = eng.forward_infer(qpos, img, depth_img=n).clone()
    a_u16 = eng.forward_infer(qpos, img, depth_img=d).clone()
    assert torch.isfinite(a_u16).all() and torch.equal(a_u16, a_f32)
    # one handle, alternating bindings: each reproduces itself
    q2, i2, d2, n2 = (t.to(dev) for t in _frames(cfg, 2))
    b_f32 = eng.forward_infer(q2, i2, depth_img=n2).clone()
    assert not torch.equal(b_f32, a_f32)
    assert torch.equal(eng.forward_infer(qpos, img, depth_img=d), a_f32)
    assert torch.equal(eng.forward_infer(q2, i2, depth_img=n2), b_f32)
    assert torch.equal(eng.forward_infer(q2, i2, depth_img=d2), b_f32)
    # a captured graph with a u16 depth buffer, replayed with two batches: the table is recomputed by every replay
    replay = eng.capture_infer(2, depth_dtype=torch.uint16)
    assert replay.static_depth.dtype == torch.uint16
    assert torch.equal(replay(qpos, img, depth_img=d), a_f32)
    assert torch.equal(replay(q2, i2, depth_img=d2), b_f32)
    with pytest.raises(ValueError):
        replay(q2, i2, depth_img=n2)                                  # f32 into a u16 capture: no silent conversion
    with pytest.raises(TypeError):
        eng.forward_infer(qpos, img, depth_img=d.to(torch.int32))
    assert eng.read_flags() == 0


# ---- 4. engine training ----------------------------------------------------------------------------------------------------------------
def test_engine_training_step_u16_depth_is_bitwise_the_f32_path():
    eng = _engine(training=True)
    cfg, dev = eng.cfg, eng.device
    _, _, inp = _fixture()
    qpos, img, d, n = (t.to(dev) for t in _frames(cfg, 3))
    actions, is_pad = torch.from_numpy(inp["actions"])[:2].to(dev), torch.from_numpy(inp["is_pad"])[:2].to(dev)
    eps = torch.randn(2, cfg.latent_in_dim, generator=torch.Generator().manual_seed(5)).to(dev)

    def step(depth):
        out = eng.forward_train(qpos, img, actions, is_pad, eps=eps, depth_img=depth)
        eng.zero_grad()
        eng.backward(1.0)
        return {k: out[k].clone() for k in ("l1", "kl", "loss", "a_hat", "mu", "logvar")}, {k: eng.grad(k) for k in eng.spec}
    out_f, g_f = step(n)
    out_u, g_u = step(d)
    for k in out_f:
        assert torch.isfinite(out_u[k]).all() and torch.equal(out_u[k], out_f[k]), k
    for k in g_f:
        assert torch.equal(g_u[k].view(torch.int32), g_f[k].view(torch.int32)), k
    assert float(g_u["depth_backbones.0.0.body.conv1.weight"].abs().max()) > 0


# ---- 5. the host-fed pipeline ----------------------------------------------------------------------------------------------------------
def test_infer_pipeline_feeds_u16_depth_from_the_host():
    eng = _engine()
    cfg, dev = eng.cfg, eng.device
    with pytest.raises(NotImplementedError):
        InferPipeline(eng, 2)
    pipe = InferPipeline(eng, 2, depth_dtype=torch.uint16, copy_stream_candidates=1)
    host = [tuple(t.pin_memory() for t in _frames(cfg, 10 + t)[:3]) for t in range(3)]
    with pytest.raises(ValueError):
        pipe.feed(host[0][0], host[0][1])
    pipe.feed(host[0][0], host[0][1], depth_host=host[0][2])
    outs = []
    for t in range(3):
        outs.append(pipe.step(next_inputs=host[t + 1] if t + 1 < 3 else None).clone())
    torch.cuda.synchronize()
    for t in range(3):
        q, i, d = (x.to(dev) for x in host[t])
        assert torch.equal(outs[t], eng.forward_infer(q, i, depth_img=d)), t
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    assert eng.read_flags() == 0


# ---- 6. episode files -> loader -> prefetcher -> policy ----------------------------------------------------------------------------------
def test_u16_depth_episodes_train_end_to_end(tmp_path):
    from actmi.data import DevicePrefetcher, load_data
    from imitate_episodes import forward_pass
    from policy import ACTPolicy
    cams, H, W, T = ["a", "b"], 64, 96, 6
    rng = np.random.default_rng(0)
    for e in range(3):
        ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32),
              "/observations/qvel": np.zeros((T, 14), np.float32), "/action": rng.standard_normal((T, 16)).astype(np.float32),
              "attrs_sim": np.array(True)}
        for c in cams:
            ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
            ep[f"/observations/depth_images/{c}"] = rng.integers(200 + 100 * e, 40000 + 1000 * e, (T, H, W)).astype(np.uint16)
        np.savez(tmp_path / f"episode_{e}.npz", **ep)
    train_dl, _, _, _ = load_data(str(tmp_path), lambda n: True, cams, 2, 2, 8, policy_class="ACT", num_workers=0, train_ratio=0.67,
                                  rng=np.random.default_rng(1), depth_camera_names=cams, use_depth=True)
    batch = next(DevicePrefetcher(iter(train_dl)))
    assert len(batch) == 5 and batch[4].dtype == torch.uint16 and batch[4].is_cuda and tuple(batch[4].shape) == (2, 2, 1, H, W)
    assert batch[0].dtype == torch.uint8
    pol = ACTPolicy({"use_depth": True, "depth_camera_names": cams, "kl_weight": 10, "lr": 1e-5, "num_queries": 8, "hidden_dim": 64,
                     "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4, "camera_names": cams, "image_h": H,
                     "image_w": W, "base_width": 8}, max_batch=2)
    pol.train()
    pol.train_dropout = 0.0                                           # (the two calls below must draw the same masks: none)
    eps = torch.randn(2, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(2)).cuda()
    pol.next_eps = eps
    got = forward_pass(batch, pol)
    image, qpos, action, is_pad, depth = batch
    pol.next_eps = eps
    exp = pol(qpos, image, action, is_pad, depth_img=_normalise(depth.cpu()).cuda())
    for k in ("l1", "kl", "loss"):
        print(f"end to end {k}: {float(got[k]):.6f}")
        assert np.isfinite(float(got[k])) and float(got[k]) == float(exp[k]), k
