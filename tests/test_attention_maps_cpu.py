"""The host side of the attention maps, without a GPU: the float64 statement against torch's own multi-head attention, the
decoder-operand restatement against the oracle, the layout split against a brute-force loop, the overlay's numpy statement
against F.interpolate, the new exports, and the flags / refusals of the replay."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers_attention_maps as HA
from helpers import load_fixture, regenerate
from oracle import act_ref as R
from actmi import lib as L
from actmi import ops
from actmi.attention_maps import AttentionLayout, split_attention, source_names, check_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_attn_weights_ref_is_torch_multi_head_attention(masked, shared):
    B, Nq, Nk, H, hd = 3, 7, 19, 4, 8
    D = H * hd
    g = torch.Generator().manual_seed(11 + masked + 2 * shared)
    q_in = torch.randn(Nq, D, generator=g, dtype=torch.float64) if shared else torch.randn(B, Nq, D, generator=g, dtype=torch.float64)
    k_in, v_in = torch.randn(B, Nk, D, generator=g, dtype=torch.float64), torch.randn(B, Nk, D, generator=g, dtype=torch.float64)
    Win, b_in = torch.randn(3 * D, D, generator=g, dtype=torch.float64) / D ** 0.5, torch.randn(3 * D, generator=g, dtype=torch.float64)
    Wo, bo = torch.randn(D, D, generator=g, dtype=torch.float64) / D ** 0.5, torch.randn(D, generator=g, dtype=torch.float64)
    kpm = None
    if masked:
        kpm = torch.zeros(B, Nk, dtype=torch.bool)
        kpm[0, Nk - 5:] = True
        kpm[1, ::3] = True
        kpm[2, 1:] = True                                       # a single live key
    qb = q_in.unsqueeze(0).expand(B, -1, -1) if shared else q_in
    out, w = F.multi_head_attention_forward(qb.transpose(0, 1), k_in.transpose(0, 1), v_in.transpose(0, 1), D, H, Win, b_in, None, None,
                                            False, 0.0, Wo, bo, training=False, key_padding_mask=kpm, need_weights=True,
                                            average_attn_weights=True)
    q = F.linear(q_in, Win[:D], b_in[:D])
    k = F.linear(k_in, Win[D:2 * D], b_in[D:2 * D])
    got = HA.attn_weights_ref(q, k, H, kpm=kpm, q_shared=shared)
    assert got.shape == w.shape == (B, Nq, Nk)
    assert float((got - w).abs().max()) <= 1e-12
    if masked:
        assert bool((got[2, :, 0] == 1).all()) and bool((got[0, :, Nk - 5:] == 0).all())


def test_all_masked_row_is_nan_like_torch():
    q, k = torch.randn(1, 3, 16, dtype=torch.float64), torch.randn(1, 5, 16, dtype=torch.float64)
    w = HA.attn_weights_ref(q, k, 2, kpm=torch.ones(1, 5, dtype=torch.bool))
    assert bool(torch.isnan(w).all())


@pytest.mark.parametrize("name", ["tiny", "tiny_c3"])
def test_decoder_operand_restatement_is_the_oracles_cross_attention(name):
    """per-head weights x V through out_proj against oracle.act_ref.mha of the decoder layer's own inputs, and the constant
    query path against the oracle's self-attention block, in float64"""
    z, cfg = load_fixture(name)
    sd_np, _ = regenerate(z, cfg)
    sd = HA.sd64(sd_np)
    memory = torch.from_numpy(z["stage.memory"]).double()                  # [N, B, D]
    N, B, D = memory.shape
    H, Q = cfg.nheads, cfg.num_queries
    p = "transformer.decoder.layers.0."
    q, k, v, q_in = HA.decoder_cross_operands(sd, cfg, memory)
    # the oracle's route to the same q_in: zeros through self-attention and norm1 (decoder_layer's first two lines)
    query_pos = sd["query_embed.weight"].unsqueeze(1).repeat(1, B, 1)
    tgt = torch.zeros_like(query_pos)
    tgt = R._ln(tgt + R.mha(tgt + query_pos, tgt + query_pos, tgt, sd, p + "self_attn.", H), sd, p + "norm1.")
    assert float((tgt + query_pos - q_in.unsqueeze(1)).abs().max()) <= 1e-10
    pos = HA.token_pos(sd, cfg).expand(-1, B, -1)
    exp = R.mha(tgt + query_pos, memory + pos, memory, sd, p + "multihead_attn.", H)        # [Q, B, D]
    probs = HA.attn_probs_ref(q, k, H, q_shared=True)                                          # [B, H, Q, N]
    o = (probs @ HA._heads(v, H)).transpose(1, 2).reshape(B, Q, D)
    got = F.linear(o, sd[p + "multihead_attn.out_proj.weight"], sd[p + "multihead_attn.out_proj.bias"]).transpose(0, 1)
    assert float((got - exp).abs().max()) <= 1e-10
    # and the oracle's encoder from stage.src lands on stage.memory (the route the depth / cloud fixtures take)
    mem2 = HA.encoder_memory(sd, cfg, torch.from_numpy(z["stage.src"]))
    assert float((mem2 - memory).abs().max()) <= 1e-5 * float(memory.abs().max())
    w = HA.decoder_map_ref(sd_np, cfg, memory)
    assert w.shape == (B, Q, N) and float((w.sum(-1) - 1).abs().max()) <= 1e-12


# ---- the layout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fh,fw", [(2, 3), (3, 2), (1, 1)])
@pytest.mark.parametrize("cloud", [False, True])
@pytest.mark.parametrize("Kd", [0, "K"])
@pytest.mark.parametrize("K", [1, 3])
def test_split_against_a_brute_force_loop(K, Kd, cloud, fh, fw):
    Kd = K if Kd == "K" else 0
    B, Q, ne = 2, 5, 3 if cloud else 2
    lay = AttentionLayout(Q, ne + (K + Kd) * fh * fw, ne, K, Kd, fh, fw).check()
    g = torch.Generator().manual_seed(K * 100 + Kd * 10 + fh)
    tokens = torch.softmax(3 * torch.randn(B, Q, lay.N, generator=g), -1)
    for slots in (None, (0, 1), (Q - 1, Q), (1, 4)):
        q0, q1 = check_slots(lay, slots)
        rgb, depth, extra, share = HA.split_brute_force(tokens.numpy(), ne, K, Kd, fh, fw, q0, q1)
        for maps in (split_attention(tokens, lay, slots), split_attention(tokens.numpy(), lay, slots)):
            got = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in maps.items()}
            assert got["rgb"].shape == (B, K, fh, fw) and got["depth"].shape == (B, Kd, fh, fw)
            assert got["extra"].shape == (B, ne) and got["share"].shape == (B, lay.n_sources)
            tol = (q1 - q0 + fh * fw) * 2.0 ** -24
            for key, ref in (("rgb", rgb), ("depth", depth), ("extra", extra), ("share", share)):
                assert float(np.abs(got[key] - ref).max()) <= tol if ref.size else True, key
            if q1 - q0 == 1:                                   # one slot: an index map, exact
                assert np.array_equal(got["rgb"], rgb.astype(np.float32)) and np.array_equal(got["depth"], depth.astype(np.float32))
            assert float(np.abs(got["share"].astype(np.float64).sum(1) - 1).max()) <= lay.N * 2.0 ** -23
    # the index rule, token by token
    n = ne
    for blk, cams, tok in ((0, K, lay.rgb_token), (1, Kd, lay.depth_token)):
        for y in range(fh):
            for c in range(cams):
                for x in range(fw):
                    assert tok(c, y, x) == n
                    n += 1
    assert n == lay.N
    names = source_names(lay, [f"c{i}" for i in range(K)], [f"c{i}" for i in range(Kd)])
    assert len(names) == lay.n_sources and names[:2] == ["latent", "proprio"] and (names[2] == "cloud") == cloud
    for bad in ((0, Q + 1), (-1, 2), (2, 2), (3, 1)):
        with pytest.raises(ValueError):
            check_slots(lay, bad)
    with pytest.raises(ValueError):
        AttentionLayout(Q, lay.N + 1, ne, K, Kd, fh, fw).check()


def test_layout_from_config_matches_the_token_count():
    for name in ("tiny", "tiny_c3", "tiny_depth", "tiny_pcd"):
        _, cfg = load_fixture(name)
        lay = AttentionLayout.from_config(cfg).check()
        assert lay.N == cfg.num_tokens and lay.n_extra == cfg.num_extra_tokens and lay.Kd == cfg.num_depth_cams


# ---- the overlay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("H,W,fh,fw", [(64, 48, 2, 3), (33, 17, 15, 20), (30, 40, 3, 2)])
def test_heat_overlay_ref_against_torch_interpolate(H, W, fh, fw, alpha):
    B, K = 2, 3
    rng = np.random.default_rng(H + W + fh)
    frames = rng.integers(0, 256, (B, K, H, W, 3), dtype=np.uint8)
    heat = rng.random((B, K, fh, fw), dtype=np.float32) ** 3
    lut = ops.heat_ramp()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and tuple(lut[0]) == (0, 0, 0) and tuple(lut[255]) == (255, 255, 255)
    got = ops.heat_overlay_ref(frames, heat, lut, alpha)
    g = heat.astype(np.float64) / heat.reshape(B, -1).max(1).astype(np.float64)[:, None, None, None]
    gp = F.interpolate(torch.from_numpy(g), size=(H, W), mode="bilinear", align_corners=False).numpy()
    idx = np.floor(gp * 255 + 0.5).astype(np.int64)
    a = (alpha * gp)[..., None]
    exp = np.clip(np.floor(frames * (1 - a) + lut[idx] * a + 0.5), 0, 255)
    assert got.dtype == np.uint8 and int(np.abs(got.astype(np.int64) - exp).max()) <= 1
    assert np.array_equal(ops.heat_overlay_ref(frames, np.zeros_like(heat), lut, alpha), frames)
    if alpha == 0.0:
        assert np.array_equal(got, frames)
    with pytest.raises(ValueError):
        ops.heat_overlay_ref(frames, heat, lut, 1.5)


# ---- the library ------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_and_present():
    lib = L.load()
    declared = L.declared_symbols(os.path.join(ROOT, "include", "actmi.h"))
    for name in ("actmi_op_attn_weights", "actmi_bind_attention_out", "actmi_attention_layout", "actmi_op_heat_overlay_u8"):
        assert name in declared and hasattr(lib, name), name
    assert lib.actmi_bind_attention_out(None, None, 0) != 0 and lib.actmi_attention_layout(None, None) != 0
    assert lib.actmi_op_attn_weights(None, None, 0, 0, None) != 0
    assert lib.actmi_op_heat_overlay_u8(None, None, None, 0.5, None, None, 1, 1, 1, 1, 1, 1, None) != 0
    src = open(os.path.join(ROOT, "act-plus-plus_amd", "csrc", "attn_weights.hip")).read()
    assert not re.search(r"\batomic", src.split("#include", 1)[1]), "the head sum must not be accumulated atomically"


# ---- the replay's flags -----------------------------------------------------------------------------------------------------
def _cli(extra):
    import imitate_episodes as IE
    base = ("--ckpt_dir c --policy_class ACT --task_name sim_transfer_cube_scripted --batch_size 8 --seed 0 --num_steps 1 --lr 1e-5 "
            "--dataset_dir d ")
    args = vars(IE.make_parser().parse_args((base + extra).split()))
    return IE, dict(args, chunk_size=10, kl_weight=10, hidden_dim=64, dim_feedforward=64)


def test_cli_and_build_config_take_the_attention_flags():
    IE, args = _cli("--eval --replay --replay_attention --replay_attention_slots 2 5 --replay_attention_frames")
    cfg = IE.build_config(args)
    assert cfg["replay_attention"] is True and cfg["replay_attention_slots"] == [2, 5] and cfg["replay_attention_frames"] is True
    IE, args = _cli("--eval --replay --replay_attention")
    cfg = IE.build_config(args)
    assert cfg["replay_attention_slots"] is None and cfg["replay_attention_frames"] is False
    IE, args = _cli("--eval --replay")
    assert "replay_attention" not in IE.build_config(args)


@pytest.mark.parametrize("extra,exc", [("--replay_attention", ValueError),                                  # no --replay
                                       ("--eval --replay_attention", ValueError),
                                       ("--eval --replay --replay_attention_slots 0 3", ValueError),         # slots without the flag
                                       ("--eval --replay --replay_attention_frames", ValueError),
                                       ("--eval --replay --replay_attention --replay_attention_slots 0 11", ValueError),
                                       ("--eval --replay --replay_attention --replay_attention_slots 4 4", ValueError),
                                       ("--eval --replay --replay_attention --replay_attention_slots -1 4", ValueError)])
def test_build_config_refusals(extra, exc):
    IE, args = _cli(extra)
    with pytest.raises(exc):
        IE.build_config(args)


def test_build_config_refuses_a_diffusion_policy():
    IE, args = _cli("--eval --replay --replay_attention")
    with pytest.raises(NotImplementedError, match="replay_attention"):
        IE.build_config(dict(args, policy_class="Diffusion"))


def test_replay_bc_refusals_without_a_gpu(tmp_path):
    """a Diffusion policy, a policy without an engine, frames without maps: plain errors before anything is read"""
    import imitate_episodes as IE
    config = {"ckpt_dir": str(tmp_path), "state_dim": 14, "policy_class": "Diffusion", "policy_config": {"num_queries": 4},
              "camera_names": ["top"], "episode_len": 4, "task_name": "sim_transfer_cube_scripted", "temporal_agg": True,
              "dataset_dir": str(tmp_path)}
    with pytest.raises(NotImplementedError):
        IE.replay_bc(config, "policy_last.ckpt", attention=True)
    import inspect
    sig = inspect.signature(IE.replay_bc).parameters
    assert sig["attention"].default is False and sig["attention_slots"].default is None and sig["attention_frames"].default is False
