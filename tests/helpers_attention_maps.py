"""float64 statements behind the attention-map tests (test infrastructure; tests/helpers.py stays as it is).

attn_probs_ref / attn_weights_ref: the softmax of nn.MultiheadAttention per head and averaged over the heads.
decoder_cross_operands: the operands of the ONE cross-attention the inference decoder runs (layer 0 with the constant query
path), restated from the state_dict; test_attention_maps_cpu.py proves it against oracle.act_ref.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import act_ref as R


def _heads(t, H):
    B, n, D = t.shape
    return t.reshape(B, n, H, D // H).transpose(1, 2)                       # [B, H, n, hd]


def attn_probs_ref(q, k, H, kpm=None, q_shared=False, causal=False):
    """softmax_j(q_{b,h,i} . k_{b,h,j} / sqrt(hd) [+ masks]) in float64 -> [B, H, Nq, Nk].  q [B, Nq, D], or [Nq, D] shared by
    the batch; k [B, Nk, D]; kpm [B, Nk], True / non-zero = masked key.  A row with every key masked is NaN, as torch's is."""
    k = k.double()
    B = k.shape[0]
    q = q.double()
    if q_shared:
        q = q.unsqueeze(0).expand(B, -1, -1)
    hd = k.shape[2] // H
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) / hd ** 0.5
    if kpm is not None:
        s = s.masked_fill(kpm.bool().view(B, 1, 1, -1), float("-inf"))
    if causal:
        n = s.shape[-1]
        s = s.masked_fill(torch.triu(torch.ones(s.shape[-2], n, dtype=torch.bool), diagonal=1), float("-inf"))
    return torch.softmax(s, -1)


def attn_weights_ref(q, k, H, kpm=None, q_shared=False, causal=False):
    """the head average of attn_probs_ref -> [B, Nq, Nk] float64: nn.MultiheadAttention(need_weights=True,
    average_attn_weights=True)'s second result"""
    return attn_probs_ref(q, k, H, kpm, q_shared, causal).mean(1)


def sd64(sd_np):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd_np.items()}


def token_pos(sd, cfg):
    """position rows of the N memory tokens [N, 1, D]: additional_pos_embed for the tokens in front, the sine table of one
    camera grid repeated per camera along the width (h, cam, w), and the same rows again for the depth cameras"""
    fh, fw = cfg.feat_hw
    D = cfg.hidden_dim
    sine = R.position_embedding_sine(fh, fw, D // 2).double()                                # [1, D, fh, fw]
    rows = [sd["additional_pos_embed.weight"].double().unsqueeze(1)]
    for n in (cfg.num_cams, cfg.num_depth_cams):
        if n:
            rows.append(torch.cat([sine] * n, dim=3).flatten(2).permute(2, 0, 1))
    return torch.cat(rows, dim=0)


def encoder_memory(sd, cfg, src):
    """the encoder's output for the token matrix src [N, B, D] (float64, oracle.act_ref.encoder_layer)"""
    pos = token_pos(sd, cfg)
    mem = src.double()
    for i in range(cfg.enc_layers):
        mem = R.encoder_layer(mem, pos.expand(-1, mem.shape[1], -1), sd, f"transformer.encoder.layers.{i}.", cfg.nheads)
    return mem


def decoder_cross_operands(sd, cfg, memory):
    """(q [Q, D], k [B, N, D], v [B, N, D], q_in [Q, D]) of decoder layer 0's cross-attention at inference, after the
    multihead_attn input projections.  tgt starts at zero (transformer.py:114), so the layer's self-attention sees value rows
    that are all the bias b_v: whatever its weights, its output is out_proj(b_v) + b_o for every query, and
    q_in = norm1(that row) + query_pos.  k_in = memory + pos, v_in = memory (transformer.py:286-289).  memory [N, B, D] float64."""
    D = cfg.hidden_dim
    p = "transformer.decoder.layers.0."
    bv = sd[p + "self_attn.in_proj_bias"][2 * D:]
    sa = F.linear(bv, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])       # [D]
    t1 = F.layer_norm(sa, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-5)
    q_in = t1.unsqueeze(0) + sd["query_embed.weight"]                                                # [Q, D]
    W, b = sd[p + "multihead_attn.in_proj_weight"], sd[p + "multihead_attn.in_proj_bias"]
    q = F.linear(q_in, W[:D], b[:D])
    k = F.linear(memory + token_pos(sd, cfg), W[D:2 * D], b[D:2 * D]).transpose(0, 1)
    v = F.linear(memory, W[2 * D:], b[2 * D:]).transpose(0, 1)
    return q, k.contiguous(), v.contiguous(), q_in


def decoder_map_ref(sd_np, cfg, memory):
    """the map [B, Q, N] the engine's bound buffer must hold, float64, from the memory [N, B, D]"""
    sd = sd64(sd_np)
    q, k, _, _ = decoder_cross_operands(sd, cfg, memory.double())
    return attn_weights_ref(q, k, cfg.nheads, q_shared=True)


def split_brute_force(tokens, n_extra, K, Kd, fh, fw, q0, q1):
    """the layout split by a plain loop over (y, cam, x): numpy float64 -> (rgb, depth, extra, share)"""
    tokens = np.asarray(tokens, dtype=np.float64)
    B = tokens.shape[0]
    m = tokens[:, q0:q1].sum(1) / (q1 - q0)
    rgb, depth = np.zeros((B, K, fh, fw)), np.zeros((B, Kd, fh, fw))
    n = n_extra
    for dst, cams in ((rgb, K), (depth, Kd)):
        for y in range(fh):
            for c in range(cams):
                for x in range(fw):
                    dst[:, c, y, x] = m[:, n]
                    n += 1
    assert n == tokens.shape[2]
    extra = m[:, :n_extra]
    share = np.concatenate([extra, rgb.sum((2, 3)), depth.sum((2, 3))], 1)
    return rgb, depth, extra, share
