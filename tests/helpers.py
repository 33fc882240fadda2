"""Shared helpers for the parity tests (test infrastructure)."""
import json
import os

import numpy as np
import torch

from actmi.config import ACTConfig
from actmi import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg = ACTConfig(**json.loads(str(z["config_json"]))).validate()
    return z, cfg


def regenerate(z, cfg, with_actions=True):
    """Weights and inputs are regenerated from seeds; the fixture's hashes prove they are the same bytes."""
    import hashlib
    sd = W.generate_state_dict(cfg, int(z["seed_w"]))
    inp = W.generate_inputs(cfg, int(z["batch"]), int(z["seed_in"]), with_actions=with_actions)
    for k in z.files:
        if k.startswith("sha:"):
            name = k[4:]
            a = inp[name] if name in inp else sd[name]
            assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(z[k]), f"regenerated {name} differs"
    return sd, inp


def sample_like(a, z):
    m = int(z["sample_max_elems"])
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return W.fixture_sample(a, m) if m else a.reshape(-1)


def torch_sd(sd_np, prefix="model."):
    return {prefix + k: torch.from_numpy(v) for k, v in sd_np.items()}


def rel_err(got, exp):
    """max |got - exp| over max |exp|, in float64 on the CPU"""
    got, exp = got.detach().cpu().double(), exp.detach().cpu().double()
    return float((got - exp).abs().max() / (exp.abs().max() + 1e-30))


def host_mix32(x):
    """actmi_mix32 of csrc/dropout.h on a uint32 array (wrap-around arithmetic)"""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def host_u01(seed, idx):
    """actmi_u01(seed, idx) for an array of element indices: float32 in [0, 1) with 24 bits"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    h = host_mix32(lo ^ np.uint32(seed & 0xFFFFFFFF))
    h = host_mix32(h ^ hi ^ np.uint32(seed >> 32) ^ np.uint32(0x9E3779B9))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def host_keep(seed, idx, p):
    """Host transcription of actmi_keep(seed, idx, p) (csrc/dropout.h): a bool array, True = the element is kept.

    Pinned against the device through actmi_op_dropout for element indices 0 .. 100002 only: that op takes no index base, so the
    comparison covers the low word of the index alone.  The `hi` word path of actmi_u01 (indices at or above 2^32) is transcribed
    here but NOT proven against the device; every test that uses this mask stays below 2^32."""
    return host_u01(seed, idx) >= np.float32(p)


BIG_SEED = (0x5A17 << 32) | 0x9E3779B1           # above 2^32: the high seed word takes part


# ---- float64 references of the kernels of csrc/diffusion.hip and csrc/prior.hip, shared by the GPU parity files and
#      test_kernel_refs_cpu.py (which proves them against torch's own operators) ------------------------------------------------
ACTS = {None: lambda v: v, "relu": torch.relu, "mish": torch.nn.functional.mish}
GN_EPILOGUES = ["plain", "res", "film", "film+res_after"]


def groupnorm_ref(x, w, b, G, act=None, res=None, film=None, res_after=False, eps=1e-5):
    """channel-last x [n, ..., C]: F.group_norm in float64 on the channel-first permutation, then the epilogue documented in
    csrc/diffusion.hip: act(GN(x) + res), or with res_after act(GN(x)) * film_scale + film_bias + res"""
    n, C = x.shape[0], x.shape[-1]
    xc = x.double().reshape(n, -1, C).permute(0, 2, 1)
    # torch.group_norm is the operator behind F.group_norm, without the latter's refusal of one value per channel (n * P == 1)
    v = torch.group_norm(xc, G, w.double(), b.double(), eps, False).permute(0, 2, 1)
    if res is not None and not res_after:
        v = v + res.double().reshape(n, -1, C)
    v = ACTS[act](v)
    if film is not None:
        v = v * film[0].double()[:, None] + film[1].double()[:, None]
    if res is not None and res_after:
        v = v + res.double().reshape(n, -1, C)
    return v.reshape(x.shape)


def gn_epilogue_args(name, res, film):
    """keyword arguments (for ops.groupnorm and groupnorm_ref alike) of one of GN_EPILOGUES"""
    return {"plain": {}, "res": {"res": res}, "film": {"film": film},
            "film+res_after": {"film": film, "res": res, "res_after": True}}[name]


def gn_ramp(n, P, C, gen):
    """x = randn + 40 p / P: a ramp along the positions, so that the chunk means of the large-map path differ and Chan's
    between-chunk term carries most of the variance"""
    return torch.randn(n, P, C, generator=gen) + 40.0 * torch.arange(P, dtype=torch.float32).view(1, P, 1) / P


def gn_chunks(n, G, per):
    """the chunk count actmi_op_groupnorm picks for `per` values per (sample, group)"""
    return max(1, min(per // 16384, 2048 // (n * G) + 1, 256))


def gn_chunked_variance(x, G, nch, between=True):
    """biased variance per (sample, group) of channel-last x [n, P, C] in float64, combined from `nch` position chunks
    [P ch / nch, P (ch + 1) / nch) as gn_apply_kernel combines them (Chan's update); between=False drops the between-chunk
    term d * d * (cnt * cb / ct) -- the wrong rule the ramp case must catch"""
    n, P, C = x.shape
    xg = x.double().reshape(n, P, G, C // G)
    cnt, mean, m2 = 0.0, torch.zeros(n, G, dtype=torch.float64), torch.zeros(n, G, dtype=torch.float64)
    for ch in range(nch):
        part = xg[:, P * ch // nch:P * (ch + 1) // nch]
        cb = part.shape[1] * part.shape[3]
        if cb == 0:
            continue
        mb = part.mean((1, 3))
        qb = ((part - mb[:, None, :, None]) ** 2).sum((1, 3))
        ct, d = cnt + cb, mb - mean
        mean = mean + d * (cb / ct)
        m2 = m2 + qb + (d * d * (cnt * cb / ct) if between else 0.0)
        cnt = ct
    return m2 / cnt


def mish_inputs():
    """float32 inputs of the Mish check: a dense sweep, the softplus threshold 20 and its neighbours, the ends of expf's range,
    tiny values and both zeros"""
    t20 = np.float32(20.0)
    extra = [t20, np.nextafter(t20, np.float32(np.inf)), np.nextafter(t20, np.float32(-np.inf)), 88.0, 1e4, -60.0, 1e-20, -1e-20,
             0.0, -0.0]
    return torch.cat([torch.linspace(-30, 30, 6001), torch.tensor(np.array(extra, dtype=np.float32))])


def elem_rel_err(got, exp):
    """worst elementwise |got - exp| / |exp| over the elements whose expected value is non-zero, in float64"""
    got, exp = got.detach().cpu().double().reshape(-1), exp.detach().cpu().double().reshape(-1)
    nz = exp != 0
    return float(((got[nz] - exp[nz]).abs() / exp[nz].abs()).max())


def keypoint_grid(H, W):
    """(x, y) coordinates [H*W] each of robomimic's SpatialSoftmax: np.linspace(-1, 1, W) along a row, np.linspace(-1, 1, H) down
    a column (a single-element linspace is [-1])"""
    px, py = np.meshgrid(np.linspace(-1.0, 1.0, W), np.linspace(-1.0, 1.0, H))
    return torch.from_numpy(px.reshape(-1).copy()), torch.from_numpy(py.reshape(-1).copy())


def spatial_softmax_ref(logits, H, W, temperature=1.0):
    """logits [n, H*W, K] -> float64 [n, K, 2]: softmax over the positions of logits / temperature, expectation of the grid"""
    att = torch.softmax(logits.double().permute(0, 2, 1) / temperature, dim=-1)
    px, py = keypoint_grid(H, W)
    return torch.stack([(att * px).sum(-1), (att * py).sum(-1)], -1)


def unfold1d_out_len(T, k, stride, pad, transposed=False):
    return (T - 1) * stride - 2 * pad + k if transposed else (T + 2 * pad - k) // stride + 1


def unfold1d_ref(x, k, stride, pad, transposed=False):
    """the gather csrc/diffusion.hip states for unfold1d, by index arithmetic: x [B, T, C] -> [B, To, k*C] in x's dtype.
    out[b][to][j][c] = x[b][to*stride - pad + j][c] or 0; transposed: out[b][t][j][c] = x[b][(t + pad - j) / stride][c] when
    divisible and in range, else 0"""
    B, T, C = x.shape
    To = unfold1d_out_len(T, k, stride, pad, transposed)
    out = torch.zeros(B, To, k, C, dtype=x.dtype)
    for to in range(To):
        for j in range(k):
            if transposed:
                num = to + pad - j
                ok, ti = num >= 0 and num % stride == 0 and num // stride < T, num // stride
            else:
                ti = to * stride - pad + j
                ok = 0 <= ti < T
            if ok:
                out[:, to, j] = x[:, ti]
    return out.reshape(B, To, k * C)


UNFOLD_FWD = [(5, 1, 2, 16), (3, 2, 1, 16), (1, 1, 0, 8), (3, 1, 1, 7), (5, 1, 2, 1), (3, 2, 1, 2), (7, 3, 0, 20)]   # k, stride, pad, T
UNFOLD_TRANSPOSED = [(4, 2, 1, 8), (4, 2, 1, 1), (3, 1, 1, 7), (5, 3, 2, 6), (2, 2, 0, 5)]


def attention_keep(seed, n, H, T, p):
    """bool [n, H, T, T]: the keep mask of the small attention kernels, element index ((g*T + q)*T + key) with g = b*H + h"""
    cnt = n * H * T * T
    assert cnt < 2 ** 32
    return torch.from_numpy(host_keep(seed, np.arange(cnt, dtype=np.uint64), p)).view(n, H, T, T)


def masked_attention_ref(qkv, H, causal, keep=None, p=0.0):
    """qkv [n, T, 3D] (q | k | v as nn.MultiheadAttention's in_proj leaves it; float64, may require grad) -> [n, T, D]:
    (softmax(q k^T / sqrt(HD)) * keep / (1 - p)) @ v per head, the weight dropout of nn.MultiheadAttention under a given mask"""
    n, T, D3 = qkv.shape
    Dm = D3 // 3
    HD = Dm // H
    q, k, v = (t.reshape(n, T, H, HD).transpose(1, 2) for t in qkv.split(Dm, dim=-1))
    s = (q @ k.transpose(-1, -2)) / HD ** 0.5
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1), float("-inf"))
    w = s.softmax(-1)
    if keep is not None:
        w = w * keep.to(w.dtype) / (1.0 - p)
    return (w @ v).transpose(1, 2).reshape(n, T, Dm)


def fully_dropped_rows(keep, causal):
    """(sample, head, query) index triples whose every live key is dropped"""
    T = keep.shape[-1]
    live = torch.tril(torch.ones(T, T, dtype=torch.bool)) if causal else torch.ones(T, T, dtype=torch.bool)
    return torch.nonzero(~((keep & live).any(-1)))


def argmax_tie_case(rows, V, seed):
    """float32 logits [rows, V] and soft targets for the L1 metric: in every third row the maximum is copied into one or two
    later columns, and in every second of those rows the maximum first moves to the LAST column and is copied into an earlier
    one too, so ties lie on both sides of the column a plain scan meets first.  -> (x, target, rows that hold a tie)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 3
    tg = torch.rand(rows, V, generator=g)
    tied = torch.zeros(rows, dtype=torch.bool)
    if V > 1:
        for r in range(0, rows, 3) if rows >= 12 else range(rows):
            m = float(x[r].max())
            a = int(torch.argmax(x[r]))
            if (r // 3) % 2 == 1 or a == V - 1:            # the maximum to the last column, copies before it
                x[r, a] = m - 1.0
                x[r, V - 1] = m
                cols = torch.randperm(V - 1, generator=g)[:2 if V > 2 else 1]
            else:                                          # copies behind it
                cols = a + 1 + torch.randperm(V - 1 - a, generator=g)[:2 if V - 1 - a > 1 and r % 2 == 0 else 1]
            x[r, cols] = m
            tied[r] = True
    return x, tg, tied


def argmax_l1_ref(x, tg, last=False):
    """mean |one_hot(argmax) - target| in float64 with torch.argmax on the float32 values (the FIRST maximum); last=True takes the
    last maximum instead: the wrong tie rule"""
    V = x.shape[-1]
    idx = V - 1 - torch.argmax(x.flip(-1), dim=-1) if last else torch.argmax(x, dim=-1)
    return float((torch.nn.functional.one_hot(idx, V).double() - tg.double()).abs().mean())


def gemm_desc(**kw):
    """an actmi_gemm_desc from keyword fields; tensors become their device addresses (the caller keeps them alive)"""
    from actmi import lib as L
    d = L.GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def run_gemm(what, **kw):
    """actmi_op_gemm on the current stream; RuntimeError with the library's message when the launch is rejected"""
    import ctypes as C
    from actmi import lib as L
    desc = gemm_desc(**kw)
    L.check(L.load().actmi_op_gemm(C.byref(desc), L.current_stream_ptr()), None, what)


# ---- the fp16 operand split of csrc/split16.h and the operand rounding of attn_f16x3_kernel (csrc/attn.hip), modelled on the
#      CPU; test_kernel_refs_cpu.py proves that the sink cases of test_gpu_attention_envelope.py bite --------------------------
LOG2E = 1.4426950408889634


def split16_model(x):
    """(hi, lo) of split16: hi = rn16(x), lo = rn16(x - hi), both fp16 with subnormals kept (torch's CPU conversion rounds to
    nearest even and keeps them, as v_cvt_f16_f32 does with denormals on)"""
    x = x.float()
    hi = x.half()
    return hi, (x - hi.float()).half()


def prod3_model(ah, al, bh, bl):
    """the three kept products of two split operands, hi hi + hi lo + lo hi (lo lo dropped), contracted over the last axis
    of a and the first of b^T in float64: the exact sum the fp16 MFMAs accumulate, before any fp32 accumulation rounding"""
    ah, al, bh, bl = (t.double() for t in (ah, al, bh, bl))
    return ah @ bh + ah @ bl + al @ bh


def attn_p_bias(drop_p=0.0):
    """launch_attention's exponent bias of the f16x3 probabilities: the largest b <= 15 with 2^b / (1 - drop_p) <= 65000, in
    fp32 as the host computes it; None where no b >= 0 holds (the launch is refused)"""
    ds = np.float32(1.0) / (np.float32(1.0) - np.float32(drop_p)) if drop_p > 0 else np.float32(1.0)
    b = 15
    while b >= 0 and np.float32(np.ldexp(ds, b)) > np.float32(65000.0):
        b -= 1
    return b if b >= 0 else None


def _heads(t, H, hd):
    return t.reshape(t.shape[0], t.shape[1], H, hd).transpose(1, 2)


def attn_ref64(q, k, v, H, hd, dead=None, keep=None, drop_p=0.0, exact_products=True):
    """float64 softmax(q k^T / sqrt(hd) + mask) (* keep / (1 - p)) v and the log-sum-exp of the masked scores.  q [B,Nq,D],
    k / v [B,Nk,D], dead / keep broadcastable to [B,H,Nq,Nk] (dead: True = masked).  exact_products=False is the CONTROL of
    the sink cases: the same operation with q pre-scaled in fp32, every product rounded to fp32 (sums exact) and exp2
    evaluated in fp32, i.e. the operation at fp32 operand precision, which no fp32 kernel can beat -> (out [B,Nq,D], lse [B,H,Nq])"""
    B, Nq = q.shape[0], q.shape[1]
    if exact_products:
        qq, kk, vv = (_heads(t.double(), H, hd) for t in (q, k, v))
        s = qq @ kk.transpose(-1, -2) / hd ** 0.5
        if dead is not None:
            s = s.masked_fill(dead, float("-inf"))
        w = torch.softmax(s, -1)
        if keep is not None:
            w = w * keep.double() / (1.0 - drop_p)
        return (w @ vv).transpose(1, 2).reshape(B, Nq, H * hd), torch.logsumexp(s, -1)
    qs = _heads(q.float(), H, hd) * np.float32(np.float32(1.0 / hd ** 0.5) * np.float32(LOG2E))
    kk, vv = _heads(k.float(), H, hd), _heads(v.float(), H, hd)
    s = (qs.unsqueeze(-2) * kk.unsqueeze(-3)).double().sum(-1).float()      # every product rounded to fp32, summed exactly
    if dead is not None:
        s = s.masked_fill(dead, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    l = p.double().sum(-1, keepdim=True)
    if keep is not None:
        p = p * keep.float() * (np.float32(1.0) / (np.float32(1.0) - np.float32(drop_p)))
    o = (p.unsqueeze(-1) * vv.unsqueeze(-3)).double().sum(-2) / l
    return o.transpose(1, 2).reshape(B, Nq, H * hd), (m.double() / LOG2E + torch.log(l)).squeeze(-1)


ATTN_Q_UP, ATTN_V_UP = 2, 4          # log2 of the fixed up-scales attn_f16x3_kernel gives q * scale * log2 e and v before their split


def attn_f16x3_model(q, k, v, H, hd, p_bias=0, dead=None, keep=None, drop_p=0.0, q_up=0, v_up=0):
    """The operand rounding of attn_f16x3_kernel, in the kernel's order and without its schedule (no key tiles, no online
    rescale: one maximum per row):
      q * (scale * log2 e * 2^q_up) in fp32, split; k split; the three-product score in float64, rounded to fp32 (it
      carries 2^q_up, which the exponent's fused multiply-add takes out exactly);
      the row reference m' = max - p_bias and P = exp2(S - m') in fp32 (P <= 2^p_bias); the fp32 row sum of the un-dropped P;
      P (* 1 / (1 - p) where kept, else 0) split; v * 2^v_up split; the three-product P V in float64; division by the fp32 row
      sum (and 2^v_up).
    p_bias = q_up = v_up = 0 is the kernel before the scales (P <= 1, lo pieces of every p < 2^-2 subnormal); the shipped
    kernel uses attn_p_bias(drop_p), ATTN_Q_UP, ATTN_V_UP.  -> (out [B,Nq,D] float64, lse [B,H,Nq] float64, the natural-log sum with the bias taken out)"""
    B, Nq = q.shape[0], q.shape[1]
    qscale = np.float32(np.float32(1.0 / hd ** 0.5) * np.float32(LOG2E))
    qh, ql = split16_model(_heads(q.float(), H, hd) * np.float32(qscale * np.float32(2.0 ** q_up)))
    kh, kl = split16_model(_heads(k.float(), H, hd).transpose(-1, -2))
    s = prod3_model(qh, ql, kh, kl).float() * np.float32(2.0 ** -q_up)
    if dead is not None:
        s = s.masked_fill(dead, float("-inf"))
    m = s.amax(-1, keepdim=True) - np.float32(p_bias)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp2(s - m)
    l = p.double().sum(-1, keepdim=True).float()
    if keep is not None:
        p = torch.where(keep, p * (np.float32(1.0) / (np.float32(1.0) - np.float32(drop_p))), torch.zeros_like(p))
    assert float(p.max()) < 65504.0, "the biased probabilities leave the fp16 range"
    ph, pl = split16_model(p)
    vh, vl = split16_model(_heads(v.float(), H, hd) * np.float32(2.0 ** v_up))
    o = prod3_model(ph, pl, vh, vl) / (l.double() * 2.0 ** v_up)
    lse = (m.double() + p_bias) / LOG2E + torch.log(l.double() * 2.0 ** -p_bias)
    return o.transpose(1, 2).reshape(B, Nq, H * hd), lse.squeeze(-1)


def attn_f16x3_shipped(q, k, v, H, hd, dead=None, keep=None, drop_p=0.0):
    """attn_f16x3_model with the scales of the kernel as it ships: the exponent bias of the launch and the fixed q / v up-scales"""
    return attn_f16x3_model(q, k, v, H, hd, p_bias=attn_p_bias(drop_p), dead=dead, keep=keep, drop_p=drop_p, q_up=ATTN_Q_UP,
                            v_up=ATTN_V_UP)


def attn_sink_case(B, H, Nq, Nk, hd, margin, seed, v_sink=0.0, sink=0):
    """The attention-sink inputs: q, k, v ~ randn; per head, component 0 of every key is zero and key `sink` is e_0;
    q[..., 0] = margin * sqrt(hd), so the sink's score is `margin` (natural units) and every other score is N(0,1) (its
    component 0 contributes nothing); v[sink] = v_sink (a float, or a tensor broadcastable to [B, H*hd]).  The output is then
    the sum over the NON-sink keys, whose weights are e^-margin and smaller.
    -> (q [B,Nq,D], k [B,Nk,D], v [B,Nk,D], share of the softmax mass off the sink: float64 [B,H,Nq])"""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q, k, v = torch.randn(B, Nq, D, generator=g), torch.randn(B, Nk, D, generator=g), torch.randn(B, Nk, D, generator=g)
    k.view(B, Nk, H, hd)[..., 0] = 0.0
    k[:, sink] = 0.0
    k.view(B, Nk, H, hd)[:, sink, :, 0] = 1.0
    q.view(B, Nq, H, hd)[..., 0] = margin * hd ** 0.5
    v[:, sink] = v_sink
    s = _heads(q.double(), H, hd) @ _heads(k.double(), H, hd).transpose(-1, -2) / hd ** 0.5
    off = 1.0 - torch.softmax(s, -1)[..., sink]
    return q, k, v, off


# ---- the operand rounding of the fused attention backward (csrc/attn_bwd.hip), modelled on the CPU; test_kernel_refs_cpu.py
#      proves it against float64 autograd and shows that a dropped cross product bites; test_gpu_attention_bwd_forms.py takes
#      its tight bound from it ---------------------------------------------------------------------------------------------------
ATTN_BWD_PRODUCTS = ("S_dq", "T_dq", "dQ", "S_dkv", "T_dkv", "dK", "dV")     # the seven three-product contractions
ATTN_BWD_DROPS = [(w, piece) for w in ATTN_BWD_PRODUCTS for piece in ("hl", "lh")]
ATTN_BWD_E_UP = 10                   # log2 of the fixed scale the dK / dV kernel gives the (dropped) softmax weights before their split


def attn_bwd_ref64(q, k, v, dout, H, hd, dead=None, keep=None, drop_p=0.0):
    """float64 autograd through attn_ref64 -> (dq, dk, dv, out, lse [B,H,Nq], delta [B,H,Nq] = sum over the head of dout * out)"""
    qd, kd, vd = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    out, lse = attn_ref64(qd, kd, vd, H, hd, dead=dead, keep=keep, drop_p=drop_p)
    out.backward(dout.double())
    out = out.detach()
    delta = _heads(dout.double() * out, H, hd).sum(-1)
    return qd.grad, kd.grad, vd.grad, out, lse.detach(), delta


def _prod3_drop(ah, al, bh, bl, piece=None):
    """prod3_model of a @ b with one cross product removable: piece "hl" leaves out a_hi b_lo, "lh" leaves out a_lo b_hi"""
    ah, al, bh, bl = (t.double() for t in (ah, al, bh, bl))
    out = ah @ bh
    if piece != "hl":
        out = out + ah @ bl
    if piece != "lh":
        out = out + al @ bh
    return out


def _prod3_acc32(ah, al, bh, bl, first, piece=None):
    """the same three products as the MFMA chain of score_tile accumulates them: the contraction axis in steps of 16, per step
    the cross product named `first` ("hl" or "lh"), the other cross product, then hi hi; each MFMA adds the exact sum of its 16
    products to the fp32 accumulator and rounds once (how the hardware rounds inside one MFMA is not specified; this is the
    model's reading)"""
    ah, al, bh, bl = (t.double() for t in (ah, al, bh, bl))
    acc = torch.zeros(*ah.shape[:-1], bh.shape[-1], dtype=torch.float32)
    for s0 in range(0, ah.shape[-1], 16):
        sl = slice(s0, s0 + 16)
        parts = {"hl": (ah[..., sl], bl[..., sl, :]), "lh": (al[..., sl], bh[..., sl, :])}
        for name in (first, "lh" if first == "hl" else "hl"):
            if name != piece:
                acc = (acc.double() + parts[name][0] @ parts[name][1]).float()
        acc = (acc.double() + ah[..., sl] @ bh[..., sl, :]).float()
    return acc


def attn_delta_fp32_model(dout, o, H, hd):
    """attn_delta_kernel (csrc/bwd.hip) bit for bit for hd <= 64: one fp32 product dout * o per lane, summed by the wave's xor
    butterfly (lane i += lane i ^ 32, ^ 16, .. ^ 1) in fp32 -> float32 [B,H,Nq]"""
    assert hd <= 64
    B, Nq = dout.shape[0], dout.shape[1]
    x = torch.nn.functional.pad((dout.float() * o.float()).reshape(B, Nq, H, hd), (0, 64 - hd))
    w = 32
    while w >= 1:
        x = x[..., :w] + x[..., w:2 * w]
        w //= 2
    return x[..., 0].transpose(1, 2)


def column_scale_model(ds):
    """dS as acc_to_frags sees it behind column_scale: float32 ds [..., n], the last axis walked in steps of 32 from index 0.
    Per step the power of two s = 2^(140 - ex), ex the biased exponent of the step's largest magnitude clamped to [40, 230]
    (largest element in [2^13, 2^14)); ds * s in fp32, split; -> the two pieces in float64 with 1 / s taken out again (exact),
    so that one contraction over the whole axis equals the kernel's sum of per-step products times their inverse scales"""
    n = ds.shape[-1]
    x = torch.nn.functional.pad(ds.float(), (0, (-n) % 32)).reshape(*ds.shape[:-1], -1, 32)
    mx = x.abs().amax(-1, keepdim=True).contiguous()
    ex = ((mx.view(torch.int32) >> 23) & 0xff).clamp(40, 230)
    hi, lo = split16_model(x * torch.ldexp(torch.ones_like(mx), 140 - ex))
    inv = torch.ldexp(torch.ones_like(mx, dtype=torch.float64), ex - 140)
    return tuple((t.double() * inv).reshape(*ds.shape[:-1], -1)[..., :n] for t in (hi, lo))


def attn_bwd_f16x3_model(q, k, v, dout, lse, delta, H, hd, dead=None, keep=None, drop_p=0.0, do_scale=1.0, drop=None,
                         mfma_acc=False):
    """The operand rounding of attn_bwd_dq_kernel and attn_bwd_dkv_kernel, in the kernels' order and without their schedule (no
    tiles, every contraction summed in float64; the per-32-step scale of dS is kept, it is arithmetic and not schedule):
      dQ kernel: q * (scale * log2 e) in fp32, split; k, v split as they are; dout * do_scale (a power of two) in fp32, split;
      S = q k^T and T = dout v^T as three products, rounded to fp32; E = exp2(S - lse * log2 e) in fp32, zero on dead keys;
      dS = E * (T' - delta * do_scale) * scale in fp32 with T' = T / (1 - p) where kept, else 0; dS scaled per (query, 32-key
      step) by column_scale_model, split; dQ = dS k as three products, times 1 / do_scale.
      dK / dV kernel: k * (scale * log2 e) in fp32, split; q split as it is; S, T, E, dS as above from these pieces; the dropped
      weights E' = E / (1 - p) where kept times 2^10, split; dV = E'^T dout; dS scaled per (key, 32-query step), split;
      dK = dS^T q; both times 1 / do_scale (dV also 2^-10).
    q [B,Nq,D], k / v [B,Nk,D], dout [B,Nq,D], lse / delta [B,H,Nq] (rounded to fp32 here, as the kernels read them), dead /
    keep broadcastable to [B,H,Nq,Nk].  drop = (one of ATTN_BWD_PRODUCTS, "hl" | "lh") removes one cross product of that
    contraction, the factors named as written above: "hl" is left-hi right-lo.  mfma_acc=True accumulates S and T as the
    kernels' MFMA chains do (_prod3_acc32: fp32 after every MFMA, the products in each kernel's order) instead of rounding
    the exact sum once: T - delta cancels where few keys are alive, and the accumulation's rounding then shows in dS.
    -> float64 dq [B,Nq,D], dk, dv [B,Nk,D]"""
    f32 = np.float32
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    which, piece = drop if drop is not None else (None, None)
    assert which in ATTN_BWD_PRODUCTS + (None,) and piece in ("hl", "lh", None)

    def pc(name):
        return piece if which == name else None
    scale = f32(1.0) / np.sqrt(f32(hd))
    qscale, scale = float(f32(scale * f32(LOG2E))), float(scale)
    sdo = float(f32(do_scale))
    dsc = float(f32(1.0) / (f32(1.0) - f32(drop_p))) if drop_p > 0 else 1.0
    qq, kk, vv, gg = (_heads(t.float(), H, hd) for t in (q, k, v, dout))
    gh, gl = split16_model(gg * sdo)
    vh, vl = split16_model(vv)
    lse2 = (lse.float() * float(f32(LOG2E))).unsqueeze(-1)
    dlt = (delta.float() * sdo).unsqueeze(-1)

    def weights(S, T):
        E = torch.exp2(S - lse2)
        if dead is not None:
            E = torch.where(dead, torch.zeros_like(E), E)
        dp, Ed = T, E
        if keep is not None:
            dp = torch.where(keep, T * dsc, torch.zeros_like(T))
            Ed = torch.where(keep, E * dsc, torch.zeros_like(E))
        return Ed, E * (dp - dlt) * scale

    def t_(x):
        return x.transpose(-1, -2)

    def score(ah, al, bh, bl, first, name):
        """S or T of one kernel; `first` is the cross product its MFMA chain issues first (the LDS rows' lo piece leads)"""
        if mfma_acc:
            return _prod3_acc32(ah, al, t_(bh), t_(bl), first, pc(name))
        return _prod3_drop(ah, al, t_(bh), t_(bl), pc(name)).float()
    # dQ kernel
    qh, ql = split16_model(qq * qscale)
    kh, kl = split16_model(kk)
    S = score(qh, ql, kh, kl, "hl", "S_dq")                 # the streamed k and v rows come from LDS: k_lo q_hi first
    T = score(gh, gl, vh, vl, "hl", "T_dq")
    dsh, dsl = column_scale_model(weights(S, T)[1])
    dq = _prod3_drop(dsh, dsl, kh, kl, pc("dQ")) / sdo
    # dK / dV kernel
    kh, kl = split16_model(kk * qscale)
    qh, ql = split16_model(qq)
    S = score(qh, ql, kh, kl, "lh", "S_dkv")                # the streamed q and dout rows come from LDS: q_lo k_hi first
    T = score(gh, gl, vh, vl, "lh", "T_dkv")
    Ed, dS = weights(S, T)
    eh, el = split16_model(Ed * float(2.0 ** ATTN_BWD_E_UP))
    dv = _prod3_drop(t_(eh), t_(el), gh, gl, pc("dV")) / (sdo * 2.0 ** ATTN_BWD_E_UP)
    dsh, dsl = column_scale_model(t_(dS).contiguous())
    dk = _prod3_drop(dsh, dsl, qh, ql, pc("dK")) / sdo
    return tuple(t.transpose(1, 2).reshape(B, n, H * hd) for t, n in ((dq, Nq), (dk, Nk), (dv, Nk)))
