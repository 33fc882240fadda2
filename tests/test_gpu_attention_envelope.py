"""The attention kernels (csrc/attn.hip forward, csrc/attn_bwd.hip fused backward) away from unit-scale randn inputs: a peaked
softmax -- one "sink" key takes nearly all the mass and has a zero (or small) value vector, so the output is the sum over the
keys whose weights are e^-margin and smaller -- and operands whose magnitude is off unit scale.  Every forward test runs under
both precisions with the SAME bound, 3e-6 of the output maximum, against float64 on the same fp32 inputs, and checks the output
and the log-sum-exp; tests/test_kernel_refs_cpu.py shows that the operation itself stays under 1e-6 on these inputs and that
the f16x3 operand rounding WITHOUT the exponent bias of the probabilities misses the bound by 20x .. 2700x (measured on the
card at the parent of the commit that added the bias: 7e-5 .. 1.2e-4 at margin 10, 3.5e-3 .. 7.3e-3 at margin 14, the fp32 kernel
4e-7 .. 1.5e-6 on the same inputs).  Every f16x3 result is bit-identical on a second run.  Every test prints its errors."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as Hh  # noqa: E402
from helpers import rel_err  # noqa: E402
from actmi import ops  # noqa: E402
from test_gpu_kernels import PRECS, attn_split_rule  # noqa: E402  (the dispatcher's split rule: one definition)
import test_gpu_train_kernels as TK  # noqa: E402  (the float64 reference under the host dropout mask: one definition)

BOUND = 3e-6
H = 2
HDS = [16, 32, 64]


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def sink_case(B, Nq, Nk, hd, margin, sink=0, small_v=False):
    """inputs (CPU) of one sink case and their float64 output / log-sum-exp without masks, computed once per session"""
    seed = 1000 * hd + Nk + margin
    v_sink = 0.0
    if small_v:
        v_sink = 1e-3 * torch.randn(B, H * hd, generator=torch.Generator().manual_seed(seed + 1))
    q, k, v, off = Hh.attn_sink_case(B, H, Nq, Nk, hd, margin, seed, v_sink=v_sink, sink=sink)
    exp, lse = Hh.attn_ref64(q, k, v, H, hd)
    return q, k, v, float(off.max()), exp, lse


def run(q, k, v, prec, kpm=None, **kw):
    """ops.attention with the log-sum-exp; the f16x3 result must be bit-identical on a second run"""
    d = dev()
    args = (q.to(d), k.to(d), v.to(d), H)
    kd = kpm.to(torch.uint8).to(d) if kpm is not None else None
    out, lse = ops.attention(*args, kpm=kd, want_lse=True, prec=prec, **kw)
    if prec == "f16x3":
        out2, lse2 = ops.attention(*args, kpm=kd, want_lse=True, prec=prec, **kw)
        assert torch.equal(out, out2) and torch.equal(lse, lse2), "f16x3 attention is not repeatable"
    return out, lse


def check(what, got, lse, exp, lse_exp, bound=BOUND, lse_bound=BOUND):
    e, el = rel_err(got, exp), rel_err(lse, lse_exp)
    print(f"{what}: out {e:.2e} (bound {bound:.1e}), lse {el:.2e} (bound {lse_bound:.1e})")
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(lse).all()), what
    assert e < bound and el < lse_bound, what
    return e


# ---- the sink, one pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("margin", [6, 10, 14])
@pytest.mark.parametrize("Nk", [200, 1202])
@pytest.mark.parametrize("hd", HDS)
def test_sink_one_pass(hd, Nk, margin, prec):
    """sink at key 0, v[sink] = 0, no split: Nk = 200 is three key tiles and a ragged fourth, 1202 the encoder's length"""
    q, k, v, off, exp, lse_exp = sink_case(1, 40, Nk, hd, margin)
    got, lse = run(q, k, v, prec, split=False)
    check(f"sink one pass {prec} hd={hd} Nk={Nk} margin={margin} (off-sink mass {off:.1e})", got, lse, exp, lse_exp)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("hd", HDS)
def test_sink_in_the_last_ragged_tile(hd, margin, prec):
    """sink at key Nk - 1, in the ragged last tile: the running maximum jumps by the whole margin at the very end and alpha
    rescales an O that holds only small weights"""
    Nk = 200
    q, k, v, off, exp, lse_exp = sink_case(2, 130, Nk, hd, margin, sink=Nk - 1)
    got, lse = run(q, k, v, prec, split=False)
    check(f"sink at the last key {prec} hd={hd} margin={margin} (off-sink mass {off:.1e})", got, lse, exp, lse_exp)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("Nk", [200, 1202])
@pytest.mark.parametrize("hd", HDS)
def test_sink_with_a_small_value_vector(hd, Nk, margin, prec):
    """v[sink] = 1e-3 * randn instead of zero: the trained-transformer variant, same bound"""
    q, k, v, off, exp, lse_exp = sink_case(1, 40, Nk, hd, margin, small_v=True)
    got, lse = run(q, k, v, prec, split=False)
    check(f"sink with small v {prec} hd={hd} Nk={Nk} margin={margin}", got, lse, exp, lse_exp)


# ---- the sink under split-KV, a key-padding mask, the causal mask -----------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("hd", HDS)
def test_sink_split_kv(hd, margin, prec):
    """Nk = 530 in 4 splits of 192 keys: the sink sits in split 0, splits 1 and 2 hold only small weights (their partial O and l
    are e^-margin of split 0's and must survive the combine pass), split 3 owns no key.  With the split, without it, with a
    shared query: each within the bound of float64 and of each other."""
    B, Nq, Nk = 2, 40, 530
    tiles, nsplit, chunk = attn_split_rule(B, H, Nq, Nk)
    assert (tiles, nsplit, chunk) == (9, 4, 192) and (nsplit - 1) * chunk >= Nk, "the case must keep a split that owns no key"
    q, k, v, off, exp, lse_exp = sink_case(B, Nq, Nk, hd, margin)
    for shared in (False, True):
        if shared:
            qs = q[0]
            exp_s, lse_s = Hh.attn_ref64(qs.unsqueeze(0).expand(B, -1, -1), k, v, H, hd)
        else:
            qs, exp_s, lse_s = q, exp, lse_exp
        outs = {}
        for split in (True, False):
            outs[split], lse = run(qs, k, v, prec, q_shared=shared, split=split)
            check(f"sink split-KV {prec} hd={hd} margin={margin} shared={shared} split={split}", outs[split], lse, exp_s, lse_s)
        e = rel_err(outs[True], outs[False])
        print(f"sink split-KV {prec} hd={hd} margin={margin} shared={shared}: split against one pass {e:.2e}")
        assert e < BOUND


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("hd", HDS)
def test_sink_key_padding_mask(hd, margin, prec):
    """the sink is visible; keys 70 .. 89 are 4x larger, so their scores are the largest after (often above) the sink's, and the
    masked range 64 .. 95 holds them: a masked key must not move the row reference; the tail is masked too, per batch"""
    B, Nq, Nk = 2, 40, 200
    q, k, v, _, _, _ = sink_case(B, Nq, Nk, hd, margin)
    k = k.clone()
    k[:, 70:90] *= 4.0
    kpm = torch.zeros(B, Nk, dtype=torch.bool)
    kpm[:, 64:96] = True
    kpm[0, Nk - 13:] = True
    kpm[1, Nk - 70:] = True                                        # the whole last tile and part of the third
    dead = kpm.view(B, 1, 1, Nk)
    exp, lse_exp = Hh.attn_ref64(q, k, v, H, hd, dead=dead)
    s = Hh._heads(q.double(), H, hd) @ Hh._heads(k.double(), H, hd).transpose(-1, -2) / hd ** 0.5
    assert float(s[..., 70:90].max()) > float(s.masked_fill(dead, float("-inf"))[..., 1:].max()), "the masked keys score highest"
    for split in (True, False):
        got, lse = run(q, k, v, prec, kpm=kpm, split=split)
        check(f"sink with key padding {prec} hd={hd} margin={margin} split={split}", got, lse, exp, lse_exp)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("N", [130, 200])
@pytest.mark.parametrize("hd", HDS)
def test_sink_causal(hd, N, margin, prec):
    """the classical first-token sink under the causal mask; N = 200 runs in 2 splits.  Query 0 sees the sink alone: its output
    is v[sink], exactly zero"""
    B = 1
    if N == 200:
        assert attn_split_rule(B, H, N, N) == (4, 2, 128)
    q, k, v, _, _, _ = sink_case(B, N, N, hd, margin)
    dead = torch.triu(torch.ones(N, N, dtype=torch.bool), diagonal=1)
    exp, lse_exp = Hh.attn_ref64(q, k, v, H, hd, dead=dead)
    got, lse = run(q, k, v, prec, causal=True)
    check(f"sink causal {prec} hd={hd} N={N} margin={margin}", got, lse, exp, lse_exp)
    assert bool((got[:, 0] == 0).all()), "query 0 attends to the sink alone: exact zeros"


# ---- the sink under weight dropout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("hd", [16, 64])
def test_sink_with_weight_dropout(hd, margin, p, prec):
    """the kept weights are multiplied by 1 / (1 - p) BEFORE the split: the exponent bias of the f16x3 probabilities shrinks
    with p (15, 14, 12) so that the sink's own kept weight, 2^bias / (1 - p), stays a finite fp16 number"""
    B, Nq, Nk = 2, 40, 200
    q, k, v, _, _, lse_exp = sink_case(B, Nq, Nk, hd, margin)
    seed = Hh.BIG_SEED + hd + margin
    exp = TK._attn_drop_ref(q, k, v, H, None, p, seed)
    assert Hh.attn_p_bias(p) == {0.1: 15, 0.5: 14, 0.9: 12}[p]
    outs = {}
    for split in (True, False):
        outs[split], lse = run(q, k, v, prec, split=split, drop_p=p, drop_seed=seed)
        check(f"sink with dropout {prec} hd={hd} margin={margin} p={p} split={split}", outs[split], lse, exp, lse_exp)
    assert rel_err(outs[True], outs[False]) < BOUND


def test_dropout_rate_the_f16x3_split_cannot_hold_is_refused():
    """1 / (1 - p) above 65000 leaves no exponent bias >= 0 under which a kept weight is a finite fp16 number: the launch fails
    cleanly; the largest rate that still fits runs and is finite"""
    q, k, v, _, _, _ = sink_case(1, 40, 200, 16, 10)
    d = dev()
    for bad in (0.99999, 1.0):
        with pytest.raises(RuntimeError, match="drop_p"):
            ops.attention(q.to(d), k.to(d), v.to(d), H, drop_p=bad, drop_seed=1, prec="f16x3")
    assert Hh.attn_p_bias(0.99998) == 0
    got = ops.attention(q.to(d), k.to(d), v.to(d), H, drop_p=0.99998, drop_seed=1, prec="f16x3")
    assert bool(torch.isfinite(got).all())


# ---- operand magnitudes -----------------------------------------------------------------------------------------------------------
def _scaled(hd, margin, vscale, c):
    B, Nq, Nk = 2, 40, 200
    if margin is None:
        g = torch.Generator().manual_seed(77 + hd)
        q, k, v = (torch.randn(B, n, H * hd, generator=g) for n in (Nq, Nk, Nk))
    else:
        q, k, v, _, _, _ = sink_case(B, Nq, Nk, hd, margin)
    return q * c, k / c, v * vscale


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("vscale,c", [(1e-2, 1.0), (1.0, 1.0), (300.0, 1.0), (1.0, 1.0 / 16), (1.0, 16.0)])
@pytest.mark.parametrize("margin", [None, 10])
@pytest.mark.parametrize("hd", HDS)
def test_operand_magnitudes_in_range(hd, margin, vscale, c, prec):
    """the operand window the f16x3 mode claims (test_gemm_f16x3_magnitudes): v from 1e-2 to 300 of unit scale, q and k traded
    against each other by 16 either way (the scores do not change) -- same bound"""
    q, k, v = _scaled(hd, margin, vscale, c)
    exp, lse_exp = Hh.attn_ref64(q, k, v, H, hd)
    got, lse = run(q, k, v, prec, split=False)
    check(f"magnitudes {prec} hd={hd} margin={margin} v*{vscale:g} q*{c:g} k/{c:g}", got, lse, exp, lse_exp)


@pytest.mark.parametrize("vscale,c", [(1e-4, 1.0), (1.0, 1e3)])
@pytest.mark.parametrize("margin", [None, 10])
@pytest.mark.parametrize("hd", HDS)
def test_operand_magnitudes_out_of_range_degrade_to_the_split_floor(hd, margin, vscale, c):
    """v at 1e-4, or k at 1e-3 (against q at 1e3): every piece of the small operand sits on the 2^-24 subnormal grid, so its
    elements carry the absolute error 2^-25 -- the documented limit of the mode.  fp32 stays at 3e-6; f16x3 is held
    to the error the split model (helpers.attn_f16x3_model) has on THIS input, times 4 for the fp32 accumulation order the model
    leaves out (never below the 3e-6 of the in-range cases)"""
    q, k, v = _scaled(hd, margin, vscale, c)
    exp, lse_exp = Hh.attn_ref64(q, k, v, H, hd)
    got32, lse32 = run(q, k, v, "f32", split=False)
    check(f"out of range f32 hd={hd} margin={margin} v*{vscale:g} q*{c:g}", got32, lse32, exp, lse_exp)
    mod, mod_lse = Hh.attn_f16x3_shipped(q, k, v, H, hd)
    floor, floor_lse = rel_err(mod, exp), rel_err(mod_lse, lse_exp)
    got, lse = run(q, k, v, "f16x3", split=False)
    print(f"out of range f16x3 hd={hd} margin={margin} v*{vscale:g} q*{c:g}: model out {floor:.2e} lse {floor_lse:.2e}")
    check(f"out of range f16x3 hd={hd} margin={margin} v*{vscale:g} q*{c:g}", got, lse, exp, lse_exp,
          bound=max(BOUND, 4 * floor), lse_bound=max(BOUND, 4 * floor_lse))


# ---- the same inputs through the fused backward ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_case(hd, N, margin, pad, p):
    """inputs, dout (unit scale), seed, key padding and float64 out / dq / dk / dv (autograd under the host mask)"""
    B = 1
    q, k, v, _, _, _ = sink_case(B, N, N, hd, margin)
    dout = torch.randn(B, N, H * hd, generator=torch.Generator().manual_seed(N + hd))
    kpm = None
    if pad:
        kpm = torch.zeros(B, N, dtype=torch.bool)
        kpm[:, N - 37:] = True
        kpm[0, 5] = True
    seed = Hh.BIG_SEED + N
    if p > 0:
        ref = TK._attn_drop_ref(q, k, v, H, kpm, p, seed, dout)
    else:
        qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
        s = Hh._heads(qd, H, hd) @ Hh._heads(kd, H, hd).transpose(-1, -2) / hd ** 0.5
        if kpm is not None:
            s = s.masked_fill(kpm.view(B, 1, 1, N), float("-inf"))
        out = (torch.softmax(s, -1) @ Hh._heads(vd, H, hd)).transpose(1, 2).reshape(B, N, H * hd)
        out.backward(dout.double())
        ref = (out.detach(), qd.grad, kd.grad, vd.grad)
    return q, k, v, dout, kpm, seed, ref


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("margin", [10, 14])
@pytest.mark.parametrize("N", [130, 300])
@pytest.mark.parametrize("hd", HDS)
def test_sink_fused_backward(hd, N, margin, pad, p):
    """ops.attention_bwd on the sink inputs (the sink at key 0 is visible under the padding mask): dq, dk, dv against float64
    autograd at the existing 2e-5 of each tensor's maximum, with dout at unit scale and at 3e-7 under its device-side scale
    (the reference is linear in dout).  The sink's own rows of dk and dv are the largest by far and would hide every other key,
    so dk and dv restricted to the NON-sink keys are held to 2e-5 of their own maximum as well."""
    q, k, v, dout, kpm, seed, (exp, dq, dk, dv) = _bwd_case(hd, N, margin, pad, p)
    B = q.shape[0]
    d = dev()
    qd, kd, vd = q.to(d), k.to(d), v.to(d)
    kp = kpm.to(torch.uint8).to(d) if kpm is not None else None
    o, lse = ops.attention(qd, kd, vd, H, kpm=kp, want_lse=True, drop_p=p, drop_seed=seed, prec="f16x3")
    assert rel_err(o, exp) < BOUND
    for dscale in (1.0, 3e-7):
        do = (dout * dscale).to(d)
        dsc = ops.pow2_scale(do.view(B * N, H * hd)) if dscale != 1.0 else None
        got = ops.attention_bwd(qd, kd, vd, o, lse, do, H, kpm=kp, drop_p=p, drop_seed=seed, do_scale=dsc)
        again = ops.attention_bwd(qd, kd, vd, o, lse, do, H, kpm=kp, drop_p=p, drop_seed=seed, do_scale=dsc)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        errs = {}
        for name, a, b in zip(("dq", "dk", "dv"), got, (dq, dk, dv)):
            errs[name] = rel_err(a, b * dscale)
        for name, a, b in (("dk off the sink", got[1], dk), ("dv off the sink", got[2], dv)):
            errs[name] = rel_err(a[:, 1:], b[:, 1:] * dscale)
        print(f"sink fused backward hd={hd} N={N} margin={margin} pad={pad} p={p} dout*{dscale:g}: "
              + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()) + " (bound 2.0e-05)")
        assert all(bool(torch.isfinite(t).all()) for t in got)
        for n, e in errs.items():
            assert e < 2e-5, n
