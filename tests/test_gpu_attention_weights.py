"""actmi_op_attn_weights (csrc/attn_weights.hip) against the float64 statement helpers_attention_maps.attn_weights_ref, under
both product precisions.

Bound: 3e-6 absolute, the figure tests/test_gpu_attention_envelope.py holds the forward's output to (relative to an output
maximum of order one; a probability is bounded by 1 like that output), with unit-scale operands.  Every case prints its error.
Exact properties: a masked key is exactly 0, an unmasked row sums to 1 within Nk ulps of fp32, two launches give the same bits,
nothing outside the [Nq][Nk] blocks of w is written.

Head widths: launch_attention accepts 16, 32 and 64 and so does this op (the tiny fixtures are D = 64 over 4 heads: 16);
8 is refused by both, which test_refusals pins.  Key counts straddle the 64-key tile and the 128 keys the kernel stages per
barrier; query counts straddle the 32-row block."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as Hh  # noqa: E402
from helpers_attention_maps import attn_weights_ref  # noqa: E402
from actmi import ops  # noqa: E402

PRECS = ["f32", "f16x3"]
BOUND = 3e-6
HEADS = {16: 4, 32: 3, 64: 2}              # (3 heads: the head average is not a power-of-two division)
NQS = [1, 8, 33, 100]
NKS = [1, 14, 63, 64, 65, 127, 128, 129, 130, 257]
ULP = 2.0 ** -23
SENTINEL = 0x7FC12345                      # a NaN payload: any write shows


def dev():
    return torch.device("cuda:0")


def _rand(B, Nq, Nk, hd, seed, shared=False):
    H = HEADS[hd]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Nq, H * hd, generator=g) if shared else torch.randn(B, Nq, H * hd, generator=g)
    return q, torch.randn(B, Nk, H * hd, generator=g), H


def _check(what, got, exp, kpm=None, causal=False, bound=BOUND):
    """error against float64, exact zeros at masked keys, row sums; rows with every key masked are left to the caller"""
    got = got.cpu()
    B, Nq, Nk = got.shape
    dead = torch.zeros(B, Nq, Nk, dtype=torch.bool)
    if kpm is not None:
        dead |= kpm.bool().view(B, 1, Nk)
    if causal:
        dead |= torch.triu(torch.ones(Nq, Nk, dtype=torch.bool), diagonal=1)
    live_rows = ~dead.all(-1)
    err = float((got.double() - exp)[live_rows].abs().max())
    sums = got.double().sum(-1)[live_rows]
    serr = float((sums - 1).abs().max())
    print(f"{what}: max err {err:.2e} (bound {bound:.1e}), max |row sum - 1| {serr:.2e} (bound {Nk * ULP:.2e})")
    assert bool(torch.isfinite(got[live_rows]).all()), what
    assert err < bound, what
    assert bool((got[dead & live_rows.unsqueeze(-1)] == 0).all()), what + ": a masked key is not exactly 0"
    assert serr <= Nk * ULP, what
    return err


def _run(q, k, H, prec, **kw):
    d = dev()
    kd = {n: (v.to(d) if torch.is_tensor(v) else v) for n, v in kw.items()}
    a = ops.attention_weights(q.to(d), k.to(d), H, prec=prec, **kd)
    b = ops.attention_weights(q.to(d), k.to(d), H, prec=prec, **kd)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches differ"
    return a


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_sizes_across_tile_and_block_edges(hd, shared, prec):
    worst = 0.0
    for Nq in NQS:
        for Nk in NKS:
            q, k, H = _rand(2, Nq, Nk, hd, 1000 * hd + 10 * Nq + Nk, shared)
            got = _run(q, k, H, prec, q_shared=shared)
            worst = max(worst, _check(f"{prec} hd={hd} shared={shared} Nq={Nq} Nk={Nk}", got, attn_weights_ref(q, k, H, q_shared=shared)))
    print(f"{prec} hd={hd} shared={shared}: worst error over the size grid {worst:.2e}")


@pytest.mark.parametrize("prec", PRECS)
def test_full_shape(prec):
    """the decoder's own shape (Q = 100, N = 1202, 8 heads of 64) at batch 2, shared queries"""
    g = torch.Generator().manual_seed(5)
    q, k = torch.randn(100, 512, generator=g), torch.randn(2, 1202, 512, generator=g)
    got = _run(q, k, 8, prec, q_shared=True)
    _check(f"{prec} full shape", got, attn_weights_ref(q, k, 8, q_shared=True))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hd", [16, 64])
def test_packed_kv_view_strided_output_and_sentinels(hd, prec):
    """K as the column view of a packed [B*N][2D] buffer whose V columns hold a sentinel; w through a row stride wider than Nk
    inside a sentinel-filled buffer with guard rows behind it"""
    B, Nq, Nk = 2, 33, 130
    q, k, H = _rand(B, Nq, Nk, hd, 77 + hd, shared=True)
    D = H * hd
    d = dev()
    kv = torch.full((B * Nk, 2 * D), SENTINEL, dtype=torch.int32, device=d).view(torch.float32)
    kv[:, :D] = k.reshape(B * Nk, D).to(d)
    kview = kv.view(B, Nk, 2 * D)[:, :, :D]
    pad = 7
    big = torch.full((B + 1, Nq, Nk + pad), SENTINEL, dtype=torch.int32, device=d).view(torch.float32)
    out = big[:B, :, :Nk]
    ops.attention_weights(q.to(d), kview, H, q_shared=True, prec=prec, out=out)
    bits = big.view(torch.int32).cpu()
    assert bool((bits[:B, :, Nk:] == SENTINEL).all()) and bool((bits[B] == SENTINEL).all()), "bytes outside the map were written"
    assert bool((kv.view(torch.int32)[:, D:] == SENTINEL).all().cpu())
    dense = _run(q, k, H, prec, q_shared=True)
    assert torch.equal(out.contiguous().view(torch.int32), dense.view(torch.int32)), "the strided views change the bits"
    _check(f"{prec} hd={hd} packed K view, strided w", out.contiguous(), attn_weights_ref(q, k, H, q_shared=True))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hd", [16, 64])
def test_key_padding_masks(hd, prec):
    """a masked tail, scattered masked keys, a single live key, and a sample with every key masked: that sample's rows are NaN
    in every entry, the documented convention (actmi_op_attention's output row of such a query is NaN too)"""
    B, Nq, Nk = 4, 33, 130
    q, k, H = _rand(B, Nq, Nk, hd, 300 + hd)
    kpm = torch.zeros(B, Nk, dtype=torch.uint8)
    kpm[0, Nk - 37:] = 1
    kpm[1, torch.randperm(Nk, generator=torch.Generator().manual_seed(3))[:50]] = 1
    kpm[2] = 1
    kpm[2, 70] = 0
    kpm[3] = 1
    got = _run(q, k, H, prec, kpm=kpm)
    _check(f"{prec} hd={hd} key padding", got[:3], attn_weights_ref(q, k, H, kpm=kpm)[:3], kpm=kpm[:3])
    g = got.cpu()
    assert bool((g[2, :, 70] == 1).all()), "a single live key takes weight exactly 1"
    assert bool(torch.isnan(g[3]).all()), "a row with every key masked is NaN throughout"
    fwd = ops.attention(q.to(dev()), k.to(dev()), k.to(dev()), H, kpm=kpm.to(dev()), prec=prec, split=False).cpu()
    assert bool(torch.isnan(fwd[3]).all()), "the forward's convention for such a row changed: the op follows it"


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [33, 130])
def test_causal(N, prec):
    q, k, H = _rand(2, N, N, 32, 900 + N)
    got = _run(q, k, H, prec, causal=True)
    _check(f"{prec} causal N={N}", got, attn_weights_ref(q, k, H, causal=True), causal=True)
    assert bool((got.cpu()[:, 0, 0] == 1).all())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hd", [16, 64])
def test_peaked_row(hd, prec):
    """one logit 60 above the rest: weight exactly 1 at that key, and nothing (below 1e-20) anywhere else; the sink sits in
    the ragged last tile"""
    B, Nq, Nk, H = 2, 33, 130, HEADS[hd]
    q, k, _, _ = Hh.attn_sink_case(B, H, Nq, Nk, hd, 60, 4242 + hd, sink=Nk - 1)
    got = _run(q, k, H, prec)
    _check(f"{prec} hd={hd} peaked", got, attn_weights_ref(q, k, H))
    g = got.cpu()
    assert bool((g[:, :, Nk - 1] == 1).all()) and float(g[:, :, :Nk - 1].max()) < 1e-20


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", [1.0 / 16, 16.0])
@pytest.mark.parametrize("hd", [16, 64])
def test_operands_at_the_edges_of_the_f16x3_window(hd, c, prec):
    """q and k traded against each other by 16 either way, as in test_gpu_attention_envelope.py: the scores do not change"""
    q, k, H = _rand(2, 40, 200, hd, 55 + hd)
    q, k = q * c, k / c
    got = _run(q, k, H, prec)
    _check(f"{prec} hd={hd} q*{c:g} k/{c:g}", got, attn_weights_ref(q, k, H))


def test_refusals():
    """what the op does not take is an error before any launch: the sentinel-filled output stays as it is"""
    d = dev()
    out = torch.full((1, 4, 8), SENTINEL, dtype=torch.int32, device=d).view(torch.float32)
    q, k = torch.randn(1, 4, 32, device=d), torch.randn(1, 8, 32, device=d)
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attention_weights(q, k, 4, out=out)                       # head width 8, as launch_attention refuses it
    with pytest.raises(RuntimeError, match="head_dim"):
        ops.attention(q, k, k, 4)
    with pytest.raises(RuntimeError, match="causal"):
        ops.attention_weights(q, k, 2, causal=True, out=out)          # Nq != Nk
    with pytest.raises(RuntimeError, match="strides"):
        ops.attention_weights(q, torch.randn(1, 8, 34, device=d)[:, :, :32], 2, out=out)
    import ctypes as C
    from actmi import lib as L
    desc = L.AttnDesc()
    desc.Q, desc.q_rs, desc.K, desc.k_rs = q.data_ptr(), 32, k.data_ptr(), 32
    desc.B, desc.H, desc.Nq, desc.Nk, desc.HD, desc.scale, desc.drop_p = 1, 2, 4, 8, 16, 0.25, 0.1
    lib = L.load()
    assert lib.actmi_op_attn_weights(C.byref(desc), out.data_ptr(), 32, 8, None) != 0          # drop_p != 0
    desc.drop_p = 0.0
    assert lib.actmi_op_attn_weights(C.byref(desc), out.data_ptr(), 32, 7, None) != 0          # row stride below Nk
    assert lib.actmi_op_attn_weights(C.byref(desc), None, 32, 8, None) != 0
    for field in ("B", "H", "Nq", "Nk"):                                                       # zero sizes
        keep = getattr(desc, field)
        setattr(desc, field, 0)
        assert lib.actmi_op_attn_weights(C.byref(desc), out.data_ptr(), 32, 8, None) != 0, field
        setattr(desc, field, keep)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all().cpu())
