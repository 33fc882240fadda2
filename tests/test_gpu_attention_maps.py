"""The decoder's cross-attention map through the engine (actmi_bind_attention_out, ACTEngine.bind_attention,
capture_infer(attention=True), ACTPolicy.attention) on the tiny, tiny_c3, tiny_depth and tiny_pcd fixtures.

The bound map is compared with helpers_attention_maps.decoder_map_ref: float64, from the fixture's reference memory
(stage.memory) or, where the fixture holds only stage.src, from the oracle's encoder on it.  The engine's memory carries the
error of its own trunk-free part (the encoder), so the map is held to the engine's a_hat error class rather than to the op's:
MAP_BOUND below, 4x the largest error measured on these four fixtures under both precisions, never above the
project's 1e-4 bar; the margin is for accumulation-order differences from box to box, not for arithmetic."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import load_fixture, regenerate  # noqa: E402
import helpers_attention_maps as HA  # noqa: E402
from actmi import weights as W  # noqa: E402
from actmi.engine import ACTEngine  # noqa: E402

ATOL = 1e-4
MAP_BOUND = 4 * 3.3e-7          # measured: 3.3e-7 (tiny, f16x3) the largest of the eight; the table is in DESIGN 5i
assert MAP_BOUND <= 1e-4
FIXTURES = ["tiny", "tiny_c3", "tiny_depth", "tiny_pcd"]
SENTINEL = 0x7FC12345
_FIX = {}


def _fixture(name):
    """(z, cfg, state_dict, inputs, float64 map) of a golden fixture, once per session"""
    if name not in _FIX:
        z, cfg = load_fixture(name)
        sd_np, inp = regenerate(z, cfg)
        sd = HA.sd64(sd_np)
        if "stage.memory" in z.files:
            memory = torch.from_numpy(z["stage.memory"]).double()
        else:
            memory = HA.encoder_memory(sd, cfg, torch.from_numpy(z["stage.src"]))
        _FIX[name] = (z, cfg, sd_np, inp, HA.decoder_map_ref(sd_np, cfg, memory))
    return _FIX[name]


def _engine(cfg, sd_np, max_batch, prec=None, env=None):
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = ACTEngine(cfg, max_batch=max_batch, gemm_prec=prec, max_points=64)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    eng.load_state_dict(sd_np)
    eng.finalize()
    return eng


def _inputs(cfg, inp, d, B=None):
    """(qpos, image, keyword inputs) of the first B samples on the device"""
    s = slice(0, B)
    kw = {}
    if cfg.use_depth:
        kw["depth_img"] = torch.from_numpy(inp["depth"][s]).to(d)
    if cfg.use_pcd:
        kw["pointcloud"] = {"xyz": torch.from_numpy(inp["pcd_xyz"][s]).contiguous().to(d),
                            "rgb": torch.from_numpy(inp["pcd_rgb"][s]).contiguous().to(d)}
    return torch.from_numpy(inp["qpos"][s]).to(d), torch.from_numpy(inp["image_u8"][s]).to(d), kw


def _buffer(eng, B, fill=None):
    cfg = eng.cfg
    if fill is None:
        return torch.zeros((B, cfg.num_queries, cfg.num_tokens), dtype=torch.float32, device=eng.device)
    return torch.full((B, cfg.num_queries, cfg.num_tokens), fill, dtype=torch.int32, device=eng.device).view(torch.float32)


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_bound_map_matches_float64_and_leaves_a_hat_alone(name, prec):
    z, cfg, sd_np, inp, exp = _fixture(name)
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B, prec)
    qpos, img, kw = _inputs(cfg, inp, eng.device)
    lay = eng.attention_layout()
    fh, fw = cfg.feat_hw
    assert tuple(lay) == (cfg.num_queries, cfg.num_tokens, 3 if cfg.use_pcd else 2, cfg.num_cams, cfg.num_depth_cams, fh, fw)
    plain = eng.forward_infer(qpos, img, **kw).clone()
    buf = _buffer(eng, B + 1, SENTINEL)                            # one sample more than the forward's batch
    eng.bind_attention(buf)
    bound = eng.forward_infer(qpos, img, **kw).clone()
    assert torch.equal(bound, plain), "a_hat depends on the binding"
    err_a = float(np.abs(bound.cpu().numpy() - z["infer.a_hat"]).max())
    got = buf[:B].cpu()
    err = float((got.double() - exp).abs().max())
    sums = float((got.double().sum(-1) - 1).abs().max())
    print(f"{name} [{prec}]: max|map - float64| = {err:.3e} (bound {MAP_BOUND:.1e}), max|row sum - 1| = {sums:.2e}, "
          f"max|a_hat - ref| = {err_a:.3e}, largest weight {float(exp.max()):.3f}")
    assert err_a <= ATOL
    assert bool(torch.isfinite(got).all()) and err <= MAP_BOUND and sums <= cfg.num_tokens * 2.0 ** -23
    assert bool((buf[B:].view(torch.int32) == SENTINEL).all().cpu()), "rows behind the forward's batch were written"
    # unbound again: the former buffer stays as it is
    eng.bind_attention(None)
    buf.view(torch.int32).fill_(SENTINEL)
    again = eng.forward_infer(qpos, img, **kw)
    assert torch.equal(again, plain) and bool((buf.view(torch.int32) == SENTINEL).all().cpu())
    assert eng.read_flags() == 0


def test_buffer_smaller_than_the_batch_is_refused_before_any_write():
    z, cfg, sd_np, inp, _ = _fixture("tiny_pcd")
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B)
    qpos, img, kw = _inputs(cfg, inp, eng.device)
    buf = _buffer(eng, B - 1, SENTINEL)
    eng.bind_attention(buf)
    with pytest.raises(RuntimeError, match=r"code -4.*attention buffer"):
        eng.forward_infer(qpos, img, **kw)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENTINEL).all().cpu())
    eng.forward_infer(qpos[:B - 1], img[:B - 1], pointcloud={k: v[:B - 1].contiguous() for k, v in kw["pointcloud"].items()})
    assert bool(torch.isfinite(buf).all().cpu())                  # the refused call left the handle usable
    with pytest.raises(ValueError):
        eng.bind_attention(buf[:, :, :-1])
    with pytest.raises(ValueError):
        eng.bind_attention(buf.double())


@pytest.mark.parametrize("name,B", [("tiny", 5), ("tiny_depth", 3)])
def test_branches_write_the_same_bits_as_one_branch(name, B):
    """every batch branch writes the rows of its own samples: two and four branches against ACTMI_CAM_PIPE=0"""
    z, cfg, sd_np, _, _ = _fixture(name)
    inp = W.generate_inputs(cfg, B, seed=100 + B)
    maps = {}
    for tag, env in (("one", {"ACTMI_CAM_PIPE": "0"}), ("two", {"ACTMI_CAM_PIPE": "1"}),
                     ("four", {"ACTMI_CAM_PIPE": "1", "ACTMI_BRANCHES": "4"})):
        eng = _engine(cfg, sd_np, B, env=env)
        qpos, img, kw = _inputs(cfg, inp, eng.device)
        buf = _buffer(eng, B)
        eng.bind_attention(buf)
        a = eng.forward_infer(qpos, img, **kw)
        maps[tag] = (buf.clone(), a.clone())
    for tag in ("two", "four"):
        assert torch.equal(maps[tag][0].view(torch.int32), maps["one"][0].view(torch.int32)), tag
        assert torch.equal(maps[tag][1], maps["one"][1]), tag
    assert not torch.equal(maps["one"][0][0], maps["one"][0][1])   # the samples' maps differ: the rows are not mixed up by luck


@pytest.mark.parametrize("name", ["tiny", "tiny_pcd"])
def test_captured_step_carries_the_binding(name):
    z, cfg, sd_np, inp, _ = _fixture(name)
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B)
    qpos, img, kw = _inputs(cfg, inp, eng.device)
    eager_buf = _buffer(eng, B)
    eng.bind_attention(eager_buf)
    eager_a = eng.forward_infer(qpos, img, **kw).clone()
    replay = eng.capture_infer(B, attention=True, num_points=inp["pcd_xyz"].shape[1] if cfg.use_pcd else None)
    assert eng.attention_out is replay.attention and eng.attention_out is not eager_buf
    a = replay(qpos, img, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, eager_a) and torch.equal(eng.attention_out.view(torch.int32), eager_buf.view(torch.int32))
    # new frames change the map; an unbind after the capture does not reach the graph
    first = eng.attention_out.clone()
    static = eng.attention_out
    eng.bind_attention(None)
    other = W.generate_inputs(cfg, B, seed=77)
    replay(qpos, torch.from_numpy(other["image_u8"]).to(eng.device), **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(static).all()) and not torch.equal(static, first)
    eng.check_flags()


@pytest.mark.parametrize("name", FIXTURES)
def test_policy_attention(name):
    from policy import ACTPolicy
    z, cfg, sd_np, inp, exp = _fixture(name)
    B = int(z["batch"])
    pc = dict(cfg.to_dict(), max_batch=B, training=False, max_points=64, device="cuda:0")
    pol = ACTPolicy(pc)
    pol.deserialize({"model." + k: torch.from_numpy(v) for k, v in sd_np.items()})
    pol.eval()
    qpos, img, kw = _inputs(cfg, inp, pol.model.device)
    plain = pol(qpos, img, **kw).clone()
    a_hat, maps = pol.attention(qpos, img, **kw)
    assert torch.equal(a_hat, plain) and pol.model.attention_out is None
    lay = pol.model.attention_layout()
    Q, ne, K, Kd = lay.Q, lay.n_extra, lay.K, lay.Kd
    assert ne == (3 if cfg.use_pcd else 2)
    tokens = maps["tokens"].cpu().numpy()
    assert float(np.abs(tokens - exp.numpy()).max()) <= MAP_BOUND
    assert maps["rgb"].shape == (B, K, lay.fh, lay.fw) and maps["depth"].shape == (B, Kd, lay.fh, lay.fw)
    assert maps["extra"].shape == (B, ne) and maps["share"].shape == (B, ne + K + Kd)
    assert all(m.is_cuda for m in maps.values())
    # the mean over ONE slot is that slot: there the split is an index map and must be exact
    for q0 in (0, Q - 1):
        _, one = pol.attention(qpos, img, slots=(q0, q0 + 1), **kw)
        rgb, depth, extra, _ = HA.split_brute_force(tokens, ne, K, Kd, lay.fh, lay.fw, q0, q0 + 1)
        assert np.array_equal(one["rgb"].cpu().numpy(), rgb.astype(np.float32))
        assert np.array_equal(one["depth"].cpu().numpy(), depth.astype(np.float32))
        assert np.array_equal(one["extra"].cpu().numpy(), extra.astype(np.float32))
    # over all slots the device's fp32 mean against the float64 mean: Q roundings of numbers below 1
    rgb, depth, extra, share = HA.split_brute_force(tokens, ne, K, Kd, lay.fh, lay.fw, 0, Q)
    tol = (Q + lay.fh * lay.fw) * 2.0 ** -24
    for key, ref in (("rgb", rgb), ("depth", depth), ("extra", extra), ("share", share)):
        assert maps[key].shape == ref.shape and (ref.size == 0 or float(np.abs(maps[key].cpu().numpy() - ref).max()) <= tol), key
    assert float((maps["share"].double().sum(1) - 1).abs().max()) <= cfg.num_tokens * 2.0 ** -23
    _, first = pol.attention(qpos, img, slots=(0, 1), **kw)
    _, last = pol.attention(qpos, img, slots=(Q - 1, Q), **kw)
    assert not torch.equal(first["rgb"], last["rgb"])
    for bad in ((0, Q + 1), (-1, 2), (3, 3)):
        with pytest.raises(ValueError):
            pol.attention(qpos, img, slots=bad, **kw)


def _launch_counts(fn):
    from actmi import lib as L
    torch.cuda.synchronize()
    L.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        rep = L.profile_report()
    finally:
        L.profile_enable(False)
    return {r["name"]: r["count"] for r in rep}


def test_unbound_forward_launches_what_it_always_did():
    """the library's own launch record: bound, the forward has one more launch (the map kernel) and the others unchanged;
    never bound, unbound again -- the same record, with no map kernel in it"""
    z, cfg, sd_np, inp, _ = _fixture("tiny")
    B = int(z["batch"])
    eng = _engine(cfg, sd_np, B)
    qpos, img, kw = _inputs(cfg, inp, eng.device)
    before = _launch_counts(lambda: eng.forward_infer(qpos, img, **kw))
    eng.bind_attention(_buffer(eng, B))
    bound = _launch_counts(lambda: eng.forward_infer(qpos, img, **kw))
    eng.bind_attention(None)
    after = _launch_counts(lambda: eng.forward_infer(qpos, img, **kw))
    mine = [n for n in bound if n.startswith("attn_weights")]
    assert len(mine) == 1 and bound[mine[0]] == 1, bound
    assert before == after and not [n for n in before if n.startswith("attn_weights")]
    assert {n: c for n, c in bound.items() if n != mine[0]} == before
