"""Kernel-level parity of csrc/prior.hip at its edges: gelu / gelu_bwd, the flat adamw (grid-stride loop included), sum_batch,
soft_ce_dim1 and argmax_l1 beyond one workgroup (and the strided loop of the ordered sum behind them), logits far from zero,
ties in the argmax, small_attention and its backward at T < 4, T = 1, odd head widths and hundreds of (sample, head) groups,
and under dropout against an exact float64 autograd reference built with the host transcription of the keep mask
(tests/helpers.py; test_kernel_refs_cpu.py proves the references against torch's own operators and proves that the tie and
offset cases bite).  Every test prints its measured error next to its bound.

Bounds are the project's, as tests/test_gpu_prior_training.py states them: gelu 1e-6 and gelu_bwd 2e-6 of the maximum, adamw and
sum_batch 2e-6, cross-entropy loss 1e-5 relative, its gradient 5e-6 of the maximum, the L1 metric 1e-6 absolute, attention forward
2e-6 and backward 3e-6 of each tensor's maximum (dq, dk and dv judged separately) -- with dropout too.

Left uncovered on purpose: dropout element indices at or above 2^32 (the high index word of actmi_u01): every mask here is far
below that, see helpers.host_keep."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import helpers as Hh  # noqa: E402
from helpers import BIG_SEED, rel_err  # noqa: E402
from actmi import ops  # noqa: E402

D = "cuda:0"


# ---- F. gelu, gelu_bwd, adamw, sum_batch -----------------------------------------------------------------------------------
def _gelu_case(x, dy, name):
    xd = x.double().requires_grad_(True)
    y = F.gelu(xd)
    y.backward(dy.double())
    ef = rel_err(ops.gelu(x.to(D)), y)
    eb = rel_err(ops.gelu_bwd(x.to(D), dy.to(D)), xd.grad)
    print(f"F. gelu {name}: forward {ef:.2e} of max (bound 1.0e-06), backward {eb:.2e} of max (bound 2.0e-06)")
    assert ef < 1e-6 and eb < 2e-6


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gelu_lengths(n):
    g = torch.Generator().manual_seed(n)
    x, dy = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    _gelu_case(x, dy, f"n={n}")


def test_gelu_sweep():
    """of the maximum, not elementwise: 1 + erf cancels below -3 in torch's float32 as well"""
    x = torch.linspace(-12, 12, 4801)
    dy = torch.randn(4801, generator=torch.Generator().manual_seed(0))
    _gelu_case(x, dy, "linspace(-12, 12, 4801)")
    assert bool(torch.isfinite(ops.gelu_bwd(x.to(D), dy.to(D))).all())


@pytest.mark.parametrize("n", [1, 257, 600001])
def test_adamw_flat(n):
    """three steps against torch.optim.AdamW in float64; 600 001 is above 2048 blocks x 256 threads, so the grid stride runs"""
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    pt = p0.clone().double().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=3e-3)
    p, m, v = p0.clone().to(D), torch.zeros(n, device=D), torch.zeros(n, device=D)
    with pytest.raises(RuntimeError):
        ops.adamw(p, p, m, v, 3e-3, 0.01, 0)                                    # steps count from 1
    assert torch.equal(p.cpu(), p0) and not bool(m.any()) and not bool(v.any())
    # the moments too (they are checkpointed state).  The C entry takes the betas as float, so the moments' own reference uses the
    # float32 values: 0.999f is 0.99900001287, and 1 - 0.999f differs from 0.001 by 1.3e-5 of itself.  In the parameters that
    # cancels against the bias correction, which the library computes from the same float value.
    b1, b2 = float(torch.tensor(0.9, dtype=torch.float32)), float(torch.tensor(0.999, dtype=torch.float32))
    mt, vt = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (10.0 ** (step - 2))
        pt.grad = gr.double()
        opt.step()
        ops.adamw(p, gr.to(D), m, v, 3e-3, 0.01, step)
        mt, vt = b1 * mt + (1 - b1) * gr.double(), b2 * vt + (1 - b2) * gr.double() ** 2
    ep, em, ev = rel_err(p, pt), rel_err(m, mt), rel_err(v, vt)
    print(f"F. adamw n={n}: parameters {ep:.2e}, m {em:.2e}, v {ev:.2e} of max (bound 2.0e-06)")
    assert ep < 2e-6 and em < 2e-6 and ev < 2e-6


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,R,Dm", [(1, 3, 8), (7, 5, 100)])
def test_sum_batch(B, R, Dm, accumulate):
    g = torch.Generator().manual_seed(B + R)
    src, d0 = torch.randn(B, R, Dm, generator=g), torch.randn(R, Dm, generator=g)
    dst = d0.clone().to(D)
    ops.sum_batch(src.to(D), dst, accumulate=accumulate)
    exp = src.double().sum(0) + (d0.double() if accumulate else 0.0)
    err = rel_err(dst, exp)
    print(f"F. sum_batch B={B} R={R} D={Dm} accumulate={accumulate}: {err:.2e} of max (bound 2.0e-06)")
    assert err < 2e-6


# ---- G. soft_ce_dim1 and argmax_l1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["one-hot", "soft"])
@pytest.mark.parametrize("B,T,V,offset", [(1, 1, 1, 0.0), (9, 32, 32, 0.0), (3, 7, 100, 0.0), (40, 64, 32, 0.0), (9, 32, 32, 80.0)])
def test_soft_ce_dim1(B, T, V, offset, target):
    """F.cross_entropy with the class axis on dim 1 (the reference's call) in float64: 1, 288, 300 and 1280 (b, v) pairs -- more
    than one workgroup, and more than 256 partial losses for the ordered sum; logits around 80, where expf without the max
    subtraction overflows.  There the gradient comes near its bound by construction (4.4e-6 of 5e-6 measured): lse is about 85,
    one float32 ulp of it is 7.6e-6, and expf(x - lse) carries half of that as a relative error"""
    g = torch.Generator().manual_seed(B * 1000 + T + V)
    x32 = torch.randn(B, T, V, generator=g) * 3 + offset
    if target == "one-hot":
        tg32 = F.one_hot(torch.randint(0, V, (B, T), generator=g), V).float()
    else:
        tg32 = torch.rand(B, T, V, generator=g)
    x = x32.double().requires_grad_(True)
    loss = F.cross_entropy(x, tg32.double())
    loss.backward()
    loss = float(loss.detach())
    gl, gd = ops.soft_ce_dim1(x32.to(D), tg32.to(D))
    el = abs(float(gl) - loss) / max(abs(loss), 1e-30)
    eg = rel_err(gd, x.grad)
    print(f"G. soft_ce_dim1 B={B} T={T} V={V} offset={offset} {target}: loss {float(gl):.6f}, {el:.2e} relative (bound 1.0e-05), "
          f"gradient {eg:.2e} of max (bound 5.0e-06)")
    assert bool(torch.isfinite(gl).all()) and el < 1e-5 and eg < 5e-6
    gl2, none = ops.soft_ce_dim1(x32.to(D), tg32.to(D), want_grad=False)
    assert none is None and torch.equal(gl, gl2)


@pytest.mark.parametrize("rows,V", [(5, 1), (256, 32), (257, 33), (1300, 32)])
def test_argmax_l1_with_ties(rows, V):
    """soft targets, so the chosen column changes the value; a third of the rows hold their maximum two or three times, before and
    behind the column it was drawn in.  torch.argmax on the same float32 values takes the first (test_kernel_refs_cpu.py: the
    last would move the metric by > 100 x the bound)"""
    x, tg, tied = Hh.argmax_tie_case(rows, V, seed=rows + V)
    exp = Hh.argmax_l1_ref(x, tg)
    got = float(ops.argmax_l1(x.to(D), tg.to(D)))
    err = abs(got - exp)
    print(f"G. argmax_l1 rows={rows} V={V} ({int(tied.sum())} rows tied): {err:.2e} absolute (bound 1.0e-06)")
    assert err < 1e-6


# ---- H. small_attention and small_attention_bwd ----------------------------------------------------------------------------
def _attention_case(n, T, H, HD, causal, p, seed, data_seed):
    g = torch.Generator().manual_seed(data_seed)
    Dm = H * HD
    qkv32, dout32 = torch.randn(n, T, 3 * Dm, generator=g), torch.randn(n, T, Dm, generator=g)
    keep = Hh.attention_keep(seed, n, H, T, p) if p > 0 else None
    qkv = qkv32.double().requires_grad_(True)
    out = Hh.masked_attention_ref(qkv, H, causal, keep, p)
    out.backward(dout32.double())
    return qkv32, dout32, keep, out.detach(), qkv.grad


def _check_attention(tag, n, T, H, HD, causal, p=0.0, seed=0):
    Dm = H * HD
    qkv32, dout32, keep, out, grad = _attention_case(n, T, H, HD, causal, p, seed, data_seed=T * 100 + HD)
    got = ops.small_attention(qkv32.to(D), H, causal=causal, drop_p=p, seed=seed)
    dqkv = ops.small_attention_bwd(qkv32.to(D), dout32.to(D), H, causal=causal, drop_p=p, seed=seed)
    ef = rel_err(got, out)
    eb = [rel_err(a, b) for a, b in zip(dqkv.split(Dm, dim=-1), grad.split(Dm, dim=-1))]
    print(f"{tag} n={n} T={T} H={H} HD={HD} causal={causal} p={p}: forward {ef:.2e} (bound 2.0e-06), dq {eb[0]:.2e} dk {eb[1]:.2e} "
          f"dv {eb[2]:.2e} of each maximum (bound 3.0e-06)")
    assert ef < 2e-6 and max(eb) < 3e-6
    return qkv32, dout32, keep, got, dqkv


@pytest.mark.parametrize("n,T,H,HD,causal", [(1, 1, 1, 1, True), (2, 3, 2, 8, True), (2, 5, 3, 24, False), (1, 63, 1, 64, True),
                                             (1, 64, 2, 64, False), (3, 33, 4, 17, True), (40, 32, 8, 32, True)])
def test_small_attention_shapes(n, T, H, HD, causal):
    """fewer rows than waves, one row, head widths that are no power of two, the 64 x 64 limit, 320 (sample, head) groups"""
    _check_attention("H.1 small_attention", n, T, H, HD, causal)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n,T,H,HD,causal", [(2, 16, 4, 16, True), (1, 33, 2, 24, False), (2, 64, 1, 64, True)])
def test_small_attention_under_dropout_against_autograd(n, T, H, HD, causal, p):
    """(softmax(s) * keep / (1 - p)) @ v in float64 with the host's keep mask, element index ((g T + q) T + key): forward and all
    three gradients at the no-dropout bounds; bitwise repeatable; a query whose every live key is dropped gives exactly 0"""
    qkv32, dout32, keep, got, dqkv = _check_attention("H.2 small_attention dropout", n, T, H, HD, causal, p, BIG_SEED)
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.05
    assert torch.equal(got, ops.small_attention(qkv32.to(D), H, causal=causal, drop_p=p, seed=BIG_SEED))
    assert torch.equal(dqkv, ops.small_attention_bwd(qkv32.to(D), dout32.to(D), H, causal=causal, drop_p=p, seed=BIG_SEED))
    assert not torch.equal(got, ops.small_attention(qkv32.to(D), H, causal=causal, drop_p=p, seed=BIG_SEED + 1))
    if causal and p == 0.5:
        rows = Hh.fully_dropped_rows(keep, causal=True)
        assert len(rows) >= 1                                                   # this seed has one (test_kernel_refs_cpu.py too)
        gv = got.cpu().view(n, T, H, HD)
        for b, h, q in rows.tolist():
            assert float(gv[b, q, h].abs().max()) == 0.0, (b, h, q)
        print(f"H.2 {len(rows)} fully dropped rows, each exactly 0")


@pytest.mark.parametrize("T,HD,p", [(65, 8, 0.0), (8, 65, 0.0), (8, 8, 1.0), (8, 8, -0.1)])
def test_small_attention_rejections(T, HD, p):
    qkv, dout = torch.zeros(1, T, 3 * HD, device=D), torch.zeros(1, T, HD, device=D)
    with pytest.raises(RuntimeError):
        ops.small_attention(qkv, 1, drop_p=p)
    with pytest.raises(RuntimeError):
        ops.small_attention_bwd(qkv, dout, 1, drop_p=p)
    torch.cuda.synchronize()
