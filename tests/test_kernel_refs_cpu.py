"""The hand-written float64 references of tests/helpers.py that test_gpu_diffusion_kernels.py and test_gpu_prior_kernels.py
compare the kernels with, proven here against torch's own operators (no GPU), and the proofs that the hard cases bite: a
wrong rule (chunk variance without the between-chunk term, the last maximum on a tie, log(1 + exp(x)) for log1p(exp(x)),
no max subtraction before expf) misses the bound of its GPU test by a wide margin."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
from helpers import rel_err


# ---- unfold1d ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("k,stride,pad,T", Hh.UNFOLD_FWD)
def test_unfold_reference_contracts_to_conv1d(k, stride, pad, T, C, B):
    g = torch.Generator().manual_seed(3)
    Co = 5
    x = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    w, b = torch.randn(Co, C, k, generator=g, dtype=torch.float64), torch.randn(Co, generator=g, dtype=torch.float64)
    exp = F.conv1d(x.permute(0, 2, 1), w, b, stride=stride, padding=pad).permute(0, 2, 1)
    cols = Hh.unfold1d_ref(x, k, stride, pad)
    got = cols.reshape(-1, k * C) @ w.permute(0, 2, 1).reshape(Co, -1).T + b
    assert cols.shape[1] == exp.shape[1]
    assert float((got.reshape(exp.shape) - exp).abs().max()) < 1e-12


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("k,stride,pad,T", Hh.UNFOLD_TRANSPOSED)
def test_unfold_reference_contracts_to_conv_transpose1d(k, stride, pad, T, C, B):
    g = torch.Generator().manual_seed(4)
    Co = 5
    x = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    w, b = torch.randn(C, Co, k, generator=g, dtype=torch.float64), torch.randn(Co, generator=g, dtype=torch.float64)
    exp = F.conv_transpose1d(x.permute(0, 2, 1), w, b, stride=stride, padding=pad).permute(0, 2, 1)
    cols = Hh.unfold1d_ref(x, k, stride, pad, transposed=True)
    got = cols.reshape(-1, k * C) @ w.permute(1, 2, 0).reshape(Co, -1).T + b
    assert cols.shape[1] == exp.shape[1]
    assert float((got.reshape(exp.shape) - exp).abs().max()) < 1e-12


# ---- spatial softmax ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (7, 1), (3, 4), (9, 13)])
def test_keypoint_grid_and_spatial_softmax_reference(H, W):
    """the grid against torch.linspace (and [-1] for one element); the expectation against logsumexp weights and an einsum"""
    px, py = Hh.keypoint_grid(H, W)
    lx = torch.linspace(-1, 1, W, dtype=torch.float64) if W > 1 else torch.tensor([-1.0], dtype=torch.float64)
    ly = torch.linspace(-1, 1, H, dtype=torch.float64) if H > 1 else torch.tensor([-1.0], dtype=torch.float64)
    assert float((px.view(H, W) - lx.view(1, W)).abs().max()) < 1e-15
    assert float((py.view(H, W) - ly.view(H, 1)).abs().max()) < 1e-15
    g = torch.Generator().manual_seed(H * 16 + W)
    lg = torch.randn(2, H * W, 3, generator=g) * 4
    for temp in (0.5, 1.0, 2.0):
        z = lg.double() / temp
        wgt = torch.exp(z - torch.logsumexp(z, dim=1, keepdim=True)).view(2, H, W, 3)
        exp = torch.stack([torch.einsum("nhwk,w->nk", wgt, lx), torch.einsum("nhwk,h->nk", wgt, ly)], -1)
        assert float((Hh.spatial_softmax_ref(lg, H, W, temp) - exp).abs().max()) < 1e-14


# ---- masked attention --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,H,HD,causal", [(2, 16, 4, 16, True), (1, 33, 2, 24, False), (1, 1, 1, 1, True), (3, 33, 4, 17, True)])
def test_masked_attention_reference_without_dropout_is_sdpa(n, T, H, HD, causal):
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(n, T, 3 * H * HD, generator=g, dtype=torch.float64)
    q, k, v = (t.reshape(n, T, H, HD).transpose(1, 2) for t in qkv.split(H * HD, dim=-1))
    exp = F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(n, T, H * HD)
    keep = Hh.attention_keep(Hh.BIG_SEED, n, H, T, 0.0)
    assert bool(keep.all())                                                     # p = 0 keeps every weight
    assert rel_err(Hh.masked_attention_ref(qkv, H, causal, keep, 0.0), exp) < 1e-14
    assert rel_err(Hh.masked_attention_ref(qkv, H, causal), exp) < 1e-14


def test_dropout_mask_has_a_fully_dropped_row_and_the_asked_rate():
    """the causal p = 0.5 case of the GPU test: some query loses every live key (row 0 has a single one), so the kernel's 0 / 0-free
    handling of such a row is exercised; the mask differs between samples and heads"""
    assert len(Hh.fully_dropped_rows(Hh.attention_keep(Hh.BIG_SEED, 2, 1, 64, 0.5), causal=True)) >= 1
    keep = Hh.attention_keep(Hh.BIG_SEED, 2, 4, 16, 0.5)
    rows = Hh.fully_dropped_rows(keep, causal=True)
    assert len(rows) >= 1
    assert abs(float(keep.float().mean()) - 0.5) < 0.03
    assert not torch.equal(keep[0, 0], keep[1, 3])
    qkv = torch.randn(2, 16, 3 * 64, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    out = Hh.masked_attention_ref(qkv, 4, True, keep, 0.5).view(2, 16, 4, 16)
    for b, h, q in rows.tolist():
        assert float(out[b, q, h].abs().max()) == 0.0


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
def test_groupnorm_reference_epilogues_and_degenerate_group():
    g = torch.Generator().manual_seed(1)
    n, P, C, G = 2, 5, 6, 3
    x, res = torch.randn(n, P, C, generator=g) * 3 + 1, torch.randn(n, P, C, generator=g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    film = (torch.randn(n, C, generator=g), torch.randn(n, C, generator=g))
    # statistics by hand: biased variance over (P x C/G)
    xg = x.double().view(n, P, G, C // G)
    mu, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
    gn = ((xg - mu) / torch.sqrt(var + 1e-5)).view(n, P, C) * w.double() + b.double()
    assert rel_err(Hh.groupnorm_ref(x, w, b, G), gn) < 1e-14
    assert rel_err(Hh.groupnorm_ref(x, w, b, G, act="mish", res=res), F.mish(gn + res.double())) < 1e-14
    exp = F.relu(gn) * film[0].double()[:, None] + film[1].double()[:, None] + res.double()
    assert rel_err(Hh.groupnorm_ref(x, w, b, G, act="relu", res=res, film=film, res_after=True), exp) < 1e-14
    # one value per group: variance 0, the output is the bias
    x1 = torch.randn(1, 1, 8, generator=g)
    w1, b1 = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    assert float((Hh.groupnorm_ref(x1, w1, b1, 8).reshape(-1) - b1.double()).abs().max()) < 1e-12    # torch's own statistics: 1e-13
    # the chunked combination IS the variance (and the chunk counts are the dispatcher's)
    xr = Hh.gn_ramp(1, 12289, 8, g)
    assert Hh.gn_chunks(1, 2, 12289 * 4) == 3 and Hh.gn_chunks(2, 8, 33 * 47 * 16) == 1 and Hh.gn_chunks(1, 1, 1050001 * 4) == 256
    var3 = Hh.gn_chunked_variance(xr, 2, 3)
    assert rel_err(var3, xr.double().view(1, 12289, 2, 4).var((1, 3), unbiased=False)) < 1e-13


@pytest.mark.parametrize("P,C,G", [(12289, 8, 2), (1050001, 4, 1)])
def test_ramp_case_catches_a_dropped_between_chunk_term(P, C, G):
    """x = randn + 40 p / P: normalising with the within-chunk variance alone misses the chunked path's 3e-6 bound by far more
    than 100 x, so the GPU test on this input cannot pass a kernel that drops Chan's between-chunk term"""
    g = torch.Generator().manual_seed(P)
    x = Hh.gn_ramp(1, P, C, g)
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    nch = Hh.gn_chunks(1, G, P * (C // G))
    right = Hh.groupnorm_ref(x, w, b, G)
    var_w = Hh.gn_chunked_variance(x, G, nch, between=False)
    var_t = Hh.gn_chunked_variance(x, G, nch)
    assert float((var_w / var_t).max()) < 0.5                                   # the between-chunk term is the larger part
    xg = x.double().view(1, P, G, C // G)
    wrong = ((xg - xg.mean((1, 3), keepdim=True)) / torch.sqrt(var_w.view(1, 1, G, 1) + 1e-5)).view(1, P, C) * w.double() + b.double()
    err = rel_err(wrong, right)
    print(f"within-chunk variance only, P={P}: error {err:.2e} of the maximum = {err / 3e-6:.0f} x the bound 3e-6")
    assert err > 100 * 3e-6
    # stationary data (the older test's) would not have caught it at that margin
    xs = torch.randn(1, P, C, generator=g) * 2 + 30.0
    vs = Hh.gn_chunked_variance(xs, G, nch, between=False) / Hh.gn_chunked_variance(xs, G, nch)
    assert float((1 - vs).abs().max()) < 1e-3


# ---- Mish --------------------------------------------------------------------------------------------------------------------
def test_mish_bound_passes_torch_float32_and_fails_a_plain_log_softplus():
    x = Hh.mish_inputs()
    exp = F.mish(x.double())
    cpu32 = Hh.elem_rel_err(F.mish(x), exp)
    bound = 4 * cpu32
    print(f"float32 CPU F.mish: worst elementwise relative error {cpu32:.2e}, bound {bound:.2e}")
    assert 1e-8 < cpu32 < 1e-6
    wrong = x * torch.tanh(torch.where(x > 20, x, torch.log(1 + torch.exp(x))))
    assert Hh.elem_rel_err(wrong, exp) > 100 * bound                           # returns 0 below about -17
    assert float((wrong.double() - exp).abs().max()) < 1e-5                     # ... which the absolute check let through
    assert int((exp != 0).sum()) == x.numel() - 2 and bool((exp[-2:] == 0).all())


# ---- soft cross entropy and the L1 metric ----------------------------------------------------------------------------------
def test_offset_logits_need_the_max_subtraction():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(9, 32, 32, generator=g) * 3 + 80
    tg = torch.rand(9, 32, 32, generator=g)
    loss = F.cross_entropy(x.double(), tg.double())
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    naive = torch.log(torch.exp(x).sum(1))                                      # float32 without the subtraction
    assert not bool(torch.isfinite(naive).all())
    # the dim-1 convention: classes along the SEQUENCE axis, mean over B * V pairs
    lse = torch.logsumexp(x.double(), dim=1, keepdim=True)
    byhand = -(tg.double() * (x.double() - lse)).sum(1).mean()
    assert abs(float(byhand) - float(loss)) < 1e-12 * float(loss)


@pytest.mark.parametrize("rows,V", [(256, 32), (257, 33), (1300, 32), (5, 1)])
def test_tie_case_catches_a_last_maximum_rule(rows, V):
    x, tg, tied = Hh.argmax_tie_case(rows, V, seed=rows + V)
    first, last = Hh.argmax_l1_ref(x, tg), Hh.argmax_l1_ref(x, tg, last=True)
    if V == 1:
        assert first == last and not bool(tied.any())
        return
    assert float(tied.float().mean()) >= 0.25
    mx = x.max(-1, keepdim=True).values
    cnt = (x == mx).sum(-1)
    a_first = torch.argmax(x, -1)
    assert bool((cnt[tied] >= 2).all()) and bool((cnt[~tied] == 1).all())
    # ties on both sides: rows whose first maximum is a copy placed before the original, rows whose copies lie behind it
    assert bool((x[tied, V - 1] == mx[tied, 0]).any()) and bool((x[tied, V - 1] != mx[tied, 0]).any())
    assert bool((a_first[tied] < V - 1).all())
    print(f"argmax tie case rows={rows} V={V}: first {first:.6f}, last {last:.6f}, moved by {abs(first - last):.2e} (bound 1e-6)")
    assert abs(first - last) > 100 * 1e-6


# ---- attention at a peaked softmax: the CPU model of attn_f16x3_kernel's operand rounding (helpers.attn_f16x3_model) -----------
def test_split16_model_is_the_exact_two_piece_split():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g) * s for s in (1e-6, 1e-3, 1.0, 300.0, 3e3)])
    hi, lo = Hh.split16_model(x)
    assert hi.dtype == lo.dtype == torch.float16
    err = (hi.double() + lo.double() - x.double()).abs()
    # relative 2^-22 while lo is a normal number, else the 2^-25 rounding error of the subnormal grid: subnormals are KEPT
    assert bool((err <= torch.maximum(x.double().abs() * 2.0 ** -22, torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    tiny = x.abs() < 1e-5
    assert bool((hi[tiny] != 0).any()), "fp16 subnormals must not be flushed"


@pytest.mark.parametrize("p,bias", [(0.0, 15), (0.1, 15), (0.49, 15), (0.5, 14), (0.9, 12), (0.99998, 0), (0.99999, None), (1.0, None)])
def test_attn_p_bias_holds_the_fp16_range(p, bias):
    assert Hh.attn_p_bias(p) == bias
    if bias is not None:
        top = 2.0 ** bias / (1.0 - p)
        assert top <= 65000.0 and (bias == 15 or 2.0 * top > 65000.0)


SINK_CPU = [(hd, Nk, margin) for hd in (16, 32, 64) for Nk in (200,) for margin in (10, 14)] + [(64, 1202, 10), (64, 1202, 14)]


@pytest.mark.parametrize("hd,Nk,margin", SINK_CPU)
def test_sink_case_bites_the_unbiased_split_and_not_the_shipped_one(hd, Nk, margin):
    """The three facts the GPU sink tests rest on, max-relative against float64 with the GPU tests' bound of 3e-6:
    the operation itself at fp32 operand precision (the control) stays under 1e-6, so the bound need not move for these inputs;
    the kernel's operand rounding WITHOUT the exponent bias misses the bound by 10x and more, so the cases are not vacuous;
    with the bias launch_attention picks (and the kernel's fixed q / v up-scales) it holds the bound."""
    B, H, Nq = 1, 2, 40
    q, k, v, off = Hh.attn_sink_case(B, H, Nq, Nk, hd, margin, seed=hd + Nk + margin)
    assert 0.0 < float(off.max()) < 0.2, "the sink must hold nearly all the mass"
    exp, lse = Hh.attn_ref64(q, k, v, H, hd)
    ctl, ctl_lse = Hh.attn_ref64(q, k, v, H, hd, exact_products=False)
    raw, raw_lse = Hh.attn_f16x3_model(q, k, v, H, hd, p_bias=0)
    fix, fix_lse = Hh.attn_f16x3_shipped(q, k, v, H, hd)
    e_ctl, e_raw, e_fix = rel_err(ctl, exp), rel_err(raw, exp), rel_err(fix, exp)
    print(f"sink hd={hd} Nk={Nk} margin={margin} off-sink mass {float(off.max()):.1e}: control {e_ctl:.2e}, split with P <= 1 "
          f"{e_raw:.2e}, with P <= 2^15 {e_fix:.2e} (bound 3.0e-06)")
    assert e_ctl < 1e-6 and rel_err(ctl_lse, lse) < 1e-6
    assert e_raw > 10 * 3e-6
    assert e_fix < 3e-6
    assert rel_err(raw_lse, lse) < 3e-6 and rel_err(fix_lse, lse) < 3e-6        # the row sum is dominated by the sink either way


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_sink_case_with_dropout_keeps_the_split_in_range(p):
    """the largest split value is 2^bias / (1 - p): attn_f16x3_model asserts it finite; the bound holds down to bias 12 (p = 0.9)"""
    B, H, Nq, Nk, hd, margin = 1, 2, 40, 200, 64, 10
    q, k, v, _ = Hh.attn_sink_case(B, H, Nq, Nk, hd, margin, seed=7)
    keep = torch.from_numpy(Hh.host_keep(Hh.BIG_SEED, np.arange(B * H * Nq * Nk, dtype=np.uint64), p)).view(B, H, Nq, Nk)
    exp, _ = Hh.attn_ref64(q, k, v, H, hd, keep=keep, drop_p=p)
    raw, _ = Hh.attn_f16x3_model(q, k, v, H, hd, p_bias=0, keep=keep, drop_p=p)
    fix, _ = Hh.attn_f16x3_shipped(q, k, v, H, hd, keep=keep, drop_p=p)
    print(f"sink with dropout p={p}: P <= 1 {rel_err(raw, exp):.2e}, P <= 2^{Hh.attn_p_bias(p)} {rel_err(fix, exp):.2e}")
    assert rel_err(raw, exp) > 3e-6 and rel_err(fix, exp) < 3e-6


@pytest.mark.parametrize("hd", [16, 32, 64])
def test_small_sink_value_and_traded_q_k_need_the_operand_scales(hd):
    """the two in-range cases of test_gpu_attention_envelope.py that the exponent bias alone does not carry: a sink value vector
    of 1e-3 (its lo pieces subnormal: absolute error 2^-25 on an output of 3e-3) and q / 16 against 16 k (the lo pieces of
    q * scale * log2 e subnormal).  With v split at 2^4 and q at 2^2 the model holds the bound with room."""
    B, H, Nq, Nk, margin = 1, 2, 40, 200, 14
    vs = 1e-3 * torch.randn(B, H * hd, generator=torch.Generator().manual_seed(hd))
    q, k, v, _ = Hh.attn_sink_case(B, H, Nq, Nk, hd, margin, seed=hd, v_sink=vs)
    exp, _ = Hh.attn_ref64(q, k, v, H, hd)
    bias_only = rel_err(Hh.attn_f16x3_model(q, k, v, H, hd, p_bias=15)[0], exp)
    shipped = rel_err(Hh.attn_f16x3_shipped(q, k, v, H, hd)[0], exp)
    print(f"small sink value hd={hd}: bias only {bias_only:.2e}, with the operand scales {shipped:.2e} (bound 3.0e-06)")
    assert bias_only > 3e-6 and shipped < 1.5e-6
    q, k, v, _ = Hh.attn_sink_case(B, H, Nq, Nk, hd, 10, seed=hd)
    q, k = q / 16, k * 16
    exp, _ = Hh.attn_ref64(q, k, v, H, hd)
    bias_only = rel_err(Hh.attn_f16x3_model(q, k, v, H, hd, p_bias=15)[0], exp)
    shipped = rel_err(Hh.attn_f16x3_shipped(q, k, v, H, hd)[0], exp)
    print(f"q / 16, 16 k hd={hd}: bias only {bias_only:.2e}, with the operand scales {shipped:.2e} (bound 3.0e-06)")
    assert shipped < 1.5e-6 and shipped < bias_only


# ---- the fused attention backward: the CPU model of attn_bwd.hip's operand rounding (helpers.attn_bwd_f16x3_model) -------------
BWD_CPU = [(Nq, Nk, hd) for (Nq, Nk) in ((33, 63), (129, 257)) for hd in (16, 64)]


@functools.lru_cache(maxsize=None)
def _bwd_cpu_case(Nq, Nk, hd):
    """randn inputs (B = 1, H = 2) and their float64 gradients, log-sum-exp and delta, computed once"""
    B, H = 1, 2
    g = torch.Generator().manual_seed(100 * hd + Nq + Nk)
    q, k, v, dout = (torch.randn(B, n, H * hd, generator=g) for n in (Nq, Nk, Nk, Nq))
    dq, dk, dv, _, lse, delta = Hh.attn_bwd_ref64(q, k, v, dout, H, hd)
    return q, k, v, dout, lse, delta, (dq, dk, dv)


@pytest.mark.parametrize("Nq,Nk,hd", BWD_CPU)
def test_attention_backward_model_holds_2e6_and_every_dropped_product_bites(Nq, Nk, hd):
    """The two facts the tight bound of test_gpu_attention_bwd_forms.py rests on, max-relative per gradient against float64
    autograd with lse and delta from float64: the full operand rounding of the kernels stays under 2e-6 (measured 2.6e-7 ..
    6.4e-7), and leaving out any one cross product (hi lo or lo hi) of any of the seven contractions raises at least one
    gradient above 1e-4 (measured 1.6e-4 .. 8.0e-4).  The variant the GPU tests use (delta as attn_delta_kernel forms it in
    fp32, S and T accumulated in fp32 along their MFMA chains) holds the same 2e-6 (measured 2.3e-7 .. 7.2e-7)."""
    H = 2
    q, k, v, dout, lse, delta, ref = _bwd_cpu_case(Nq, Nk, hd)
    full = [rel_err(a, b) for a, b in zip(Hh.attn_bwd_f16x3_model(q, k, v, dout, lse, delta, H, hd), ref)]
    print(f"attention bwd model {Nq}x{Nk} hd={hd}: dq {full[0]:.2e} dk {full[1]:.2e} dv {full[2]:.2e} (bound 2.0e-06)")
    assert max(full) < 2e-6
    # the GPU tests' variant: delta as attn_delta_kernel forms it in fp32, S and T accumulated in fp32 along the MFMA chains
    out64 = Hh.attn_ref64(q, k, v, H, hd)[0]
    delta32 = Hh.attn_delta_fp32_model(dout, out64.float(), H, hd)
    assert delta32.dtype == torch.float32 and rel_err(delta32, delta) < 1e-6
    chain = [rel_err(a, b) for a, b in zip(Hh.attn_bwd_f16x3_model(q, k, v, dout, lse, delta32, H, hd, mfma_acc=True), ref)]
    print(f"  with the fp32 delta and the MFMA-chain accumulation: dq {chain[0]:.2e} dk {chain[1]:.2e} dv {chain[2]:.2e}")
    assert max(chain) < 2e-6
    for drop in Hh.ATTN_BWD_DROPS:
        errs = [rel_err(a, b) for a, b in zip(Hh.attn_bwd_f16x3_model(q, k, v, dout, lse, delta, H, hd, drop=drop), ref)]
        print(f"  without {drop[0]} {drop[1]}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} (must pass 1.0e-04)")
        assert max(errs) > 1e-4, drop


def test_attention_backward_model_masked_and_dropped():
    """tail padding and weight dropout at p = 0.5 (the host mask of csrc/dropout.h), a power-of-two dO scale: the same 2e-6"""
    B, H, Nq, Nk, hd, p = 1, 2, 129, 257, 64, 0.5
    g = torch.Generator().manual_seed(5)
    q, k, v, dout = (torch.randn(B, n, H * hd, generator=g) for n in (Nq, Nk, Nk, Nq))
    dead = torch.zeros(B, 1, 1, Nk, dtype=torch.bool)
    dead[..., Nk - 37:] = True
    keep = torch.from_numpy(Hh.host_keep(Hh.BIG_SEED, np.arange(B * H * Nq * Nk, dtype=np.uint64), p)).view(B, H, Nq, Nk)
    dq, dk, dv, _, lse, delta = Hh.attn_bwd_ref64(q, k, v, dout, H, hd, dead=dead, keep=keep, drop_p=p)
    got = Hh.attn_bwd_f16x3_model(q, k, v, dout, lse, delta, H, hd, dead=dead, keep=keep, drop_p=p, do_scale=2.0 ** 12)
    errs = [rel_err(a, b) for a, b in zip(got, (dq, dk, dv))]
    print(f"attention bwd model masked, p={p}: dq {errs[0]:.2e} dk {errs[1]:.2e} dv {errs[2]:.2e} (bound 2.0e-06)")
    assert max(errs) < 2e-6
    assert bool((got[1][:, Nk - 37:] == 0).all()) and bool((got[2][:, Nk - 37:] == 0).all())
