"""The fused attention backward (csrc/attn_bwd.hip: attn_bwd_dq_kernel, attn_bwd_dkv_kernel) in the forms the training step
gives it and at the edges of its tile walk, through ops.attention_bwd with the caller's outputs (out=, amax_out=):

a. every head width at the boundaries of the walk (one key pair, the 32-row step, the 64-row LDS tile, 128 queries per dQ
   workgroup, 256 keys per dK / dV workgroup, odd counts in the row-pair transposed staging), at grids whose block count is no
   multiple of 8 (the remainder branch of the XCD order);
b. key-padding masks with a dead key 0, a whole dead 64-key tile, a dead 32-key step, two live keys, a mask row stride that is
   not Nk; the dead keys carry 100 * randn so that a leaked mask shows, their dk / dv rows are exactly zero;
c. the training form: Q | K | V column views of one packed buffer with pad columns, dQ | dK | dV column views of a packed
   buffer with pad columns and a spare row pre-filled with a sentinel, per-sample padding, dropout off and on, dO under the
   device-side power-of-two scale, one shared amax word; and the cross form (dense Q, packed K | V, packed dK | dV);
d. the amax word as a running maximum; e. exact invariance under a power-of-two scale of dO; f. a query shared by the
   samples (batch stride 0); g. the refusals, which leave the outputs untouched.

Every case compares dq, dk, dv with float64 autograd per tensor (helpers.rel_err: the largest difference over the largest
reference element), asserts finiteness, a bit-identical second run and the project's hard bound 2e-5, and prints its errors.
Every undropped case also holds the TIGHT bound  err < max(3e-6, 4 * model_err):  model_err is the error against float64 of
helpers.attn_bwd_f16x3_model, the kernels' arithmetic on the CPU with the kernel's own log-sum-exp and forward output (on the
CPU alone it stays under 1e-6 on randn inputs and a dropped cross product of any of the seven contractions gives 1.6e-4 ..
8e-4: tests/test_kernel_refs_cpu.py); 3e-6 is the project's f16x3 attention bound; the factor 4 covers the fp32 accumulation
order inside the kernels' tiles and the hardware exp2, which the model does not have.

Measured on an MI355X, worst per gradient (dq dk dv) over the cases of a group, the model's own error in brackets:
  a. sweep, 24 cases without (Nq, Nk) = (1, 2)   8.8e-7 1.2e-6 8.3e-7   (7.9e-7 1.2e-6 8.4e-7)
  a. sweep, (1, 2) at hd 16 / 32 / 64            2.5e-6 3.7e-6 3.8e-7   (1.9e-6 2.4e-6 4.1e-7)
  b. masks (i) (ii) (iii), 9 cases               8.3e-7 7.0e-7 9.1e-7   (8.9e-7 7.8e-7 7.9e-7);  (iv) bit-identical to (ii)
  c. self-attention form  p = 0                  1.0e-6 8.9e-7 6.0e-7   (7.7e-7 5.7e-7 6.0e-7);  p = 0.1: 7.6e-7 8.8e-7 6.7e-7
  c. cross-attention form p = 0                  6.2e-7 6.6e-7 7.3e-7   (6.2e-7 4.8e-7 4.7e-7);  p = 0.1: 8.2e-7 7.2e-7 6.0e-7
  e. scale, 6 cases                              7.4e-7 8.5e-7 1.1e-6   (7.3e-7 6.4e-7 6.6e-7);  2^-40 and 2^20 exact
  f. shared query                                4.6e-7 4.3e-7 5.9e-7   (4.7e-7 4.9e-7 5.6e-7)
No kernel fault and no leak beside the outputs was found.  One finding, in the model and not in the kernels: (1, 2) at hd 64
gave dk 3.68e-6 while the model as first written (operand rounding only, delta taken from float64) gave 7.7e-7, so the tight
bound stood at 3.09e-6 and was missed.  With two keys T - delta = P_other * (T - T_other) cancels (28-fold in the worst head of
that case), and with six (sample, head) rows the tensor maximum is small, so what the kernels add to T and delta in fp32 shows:
delta is attn_delta_kernel's fp32 butterfly sum of fp32 products, T the fp32 chain of 3 * hd / 16 MFMAs.  The model now forms
delta exactly as that kernel does (helpers.attn_delta_fp32_model: the unmodelled part of dk fell from 3.2e-6 to 1.6e-6) and
accumulates S and T in fp32 per MFMA (mfma_acc=True); its own error on that case is then 2.4e-6 and the case holds the bound,
which did not move.  96 independent (1, 2) rows per head width showed kernel and model errors of the same size (worst
4.0e-7 against 3.9e-7 of a 32-sample tensor maximum).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as Hh  # noqa: E402
from helpers import rel_err  # noqa: E402
from actmi import ops  # noqa: E402
import test_gpu_train_kernels as TK  # noqa: E402  (the float64 reference under the host dropout mask: one definition)

HARD, FLOOR, FACTOR = 2e-5, 3e-6, 4.0
HDS = [16, 32, 64]
SENTINEL = 123.0
SENTINEL_BITS = int(torch.tensor(SENTINEL).view(torch.int32))
NAMES = ("dq", "dk", "dv")


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def operands(B, H, Nq, Nk, hd, seed=0):
    """randn q, k, v, dout on the CPU, once per shape"""
    g = torch.Generator().manual_seed(1000 * hd + 10 * Nq + Nk + seed)
    return tuple(torch.randn(B, n, H * hd, generator=g) for n in (Nq, Nk, Nk, Nq))


def model_of(q, k, v, dout, o, lse, H, hd, dead=None, do_scale=1.0):
    """the CPU model of the kernels' arithmetic on the same inputs, with the kernel's own log-sum-exp and forward output: delta
    as attn_delta_kernel forms it in fp32, S and T accumulated in fp32 along their MFMA chains"""
    delta = Hh.attn_delta_fp32_model(dout, o.cpu(), H, hd)
    return Hh.attn_bwd_f16x3_model(q, k, v, dout, lse.cpu(), delta, H, hd, dead=dead, do_scale=do_scale, mfma_acc=True)


def check(what, got, ref, model=None):
    """finite, the hard bound, and with a model result the tight bound; prints every figure before it asserts"""
    errs = [rel_err(a, b) for a, b in zip(got, ref)]
    merrs = [rel_err(a, b) for a, b in zip(model, ref)] if model is not None else None
    line = ", ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs))
    if merrs is not None:
        line += " (model " + ", ".join(f"{e:.2e}" for e in merrs) + f"; tight bound max({FLOOR:.0e}, {FACTOR:.0f} x model))"
    print(f"{what}: {line} (hard bound {HARD:.0e})")
    for n, t in zip(NAMES, got):
        assert bool(torch.isfinite(t).all()), (what, n)
    for i, n in enumerate(NAMES):
        assert errs[i] < HARD, (what, n, errs[i])
        if merrs is not None:
            assert errs[i] < max(FLOOR, FACTOR * merrs[i]), (what, n, errs[i], merrs[i])
    return errs


def run_twice(*args, **kw):
    """ops.attention_bwd with dense outputs; the second run must give the same bits"""
    got = ops.attention_bwd(*args, **kw)
    again = ops.attention_bwd(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "the fused attention backward is not repeatable"
    return got


def untouched(buf, written):
    """every word of the float32 buffer outside the bool mask `written` still holds the sentinel's bits"""
    return bool((buf.view(torch.int32) == SENTINEL_BITS)[~written].all())


# ---- a. the boundaries of the tile walk, per head width ---------------------------------------------------------------------------
SWEEP = [(1, 2), (1, 65), (65, 2), (31, 33), (32, 64), (33, 63), (127, 255), (128, 256), (129, 257)]


@pytest.mark.parametrize("Nq,Nk", SWEEP)
@pytest.mark.parametrize("hd", HDS)
def test_boundary_sweep(hd, Nq, Nk):
    """B = 2, H = 3: 6 .. 18 workgroups per kernel, never a multiple of 8; no mask.  (Nk = 1 is left out: dq and dk are exactly
    zero there and a relative bound means nothing.)"""
    B, H = 2, 3
    for blocks in (B * H * ((Nq + 127) // 128), B * H * ((Nk + 255) // 256)):
        assert blocks % 8 != 0, "the case must reach the remainder branch of the XCD block order"
    q, k, v, dout = operands(B, H, Nq, Nk, hd)
    d = dev()
    qd, kd, vd, dod = (t.to(d) for t in (q, k, v, dout))
    o, lse = ops.attention(qd, kd, vd, H, want_lse=True, prec="f16x3")
    got = run_twice(qd, kd, vd, o, lse, dod, H)
    ref = Hh.attn_bwd_ref64(q, k, v, dout, H, hd)[:3]
    check(f"a. sweep hd={hd} {Nq}x{Nk}", got, ref, model_of(q, k, v, dout, o, lse, H, hd))


# ---- b. masks -------------------------------------------------------------------------------------------------------------------
MASK_SHAPE = (2, 2, 70, 200)            # B, H, Nq, Nk


def mask_pattern(name):
    B, _, _, Nk = MASK_SHAPE
    kpm = torch.zeros(B, Nk, dtype=torch.bool)
    if name == "key0+tile":             # (i) key 0 and the whole LDS tile [64, 128) dead
        kpm[:, 0] = True
        kpm[:, 64:128] = True
    elif name == "step+tail":           # (ii) the 32-key step [96, 128) dead in sample 0, the tail [150, 200) in sample 1
        kpm[0, 96:128] = True
        kpm[1, 150:] = True
    elif name == "two-live":            # (iii) only keys 5 and 199 alive
        kpm[:] = True
        kpm[:, 5] = False
        kpm[:, 199] = False
    return kpm


@functools.lru_cache(maxsize=None)
def mask_case(hd, name):
    """operands with 100 * randn in the dead keys' k and v rows, the mask, and the float64 gradients, once per case"""
    B, H, Nq, Nk = MASK_SHAPE
    q, k, v, dout = (t.clone() for t in operands(B, H, Nq, Nk, hd, seed=1))
    kpm = mask_pattern(name)
    g = torch.Generator().manual_seed(hd + len(name))
    k[kpm] = 100.0 * torch.randn(int(kpm.sum()), H * hd, generator=g)
    v[kpm] = 100.0 * torch.randn(int(kpm.sum()), H * hd, generator=g)
    ref = Hh.attn_bwd_ref64(q, k, v, dout, H, hd, dead=kpm.view(B, 1, 1, Nk))[:3]
    return q, k, v, dout, kpm, ref


def run_masked(hd, name, kpm_dev=None):
    B, H, Nq, Nk = MASK_SHAPE
    q, k, v, dout, kpm, ref = mask_case(hd, name)
    d = dev()
    qd, kd, vd, dod = (t.to(d) for t in (q, k, v, dout))
    if kpm_dev is None:
        kpm_dev = kpm.to(torch.uint8).to(d)
    o, lse = ops.attention(qd, kd, vd, H, kpm=kpm_dev, want_lse=True, prec="f16x3")
    got = run_twice(qd, kd, vd, o, lse, dod, H, kpm=kpm_dev)
    return got, o, lse


@pytest.mark.parametrize("name", ["key0+tile", "step+tail", "two-live"])
@pytest.mark.parametrize("hd", HDS)
def test_masks(hd, name):
    """dead key 0 with a dead LDS tile (column_scale sees all-zero columns), a dead 32-key step with a dead tail, two live keys"""
    B, H, Nq, Nk = MASK_SHAPE
    q, k, v, dout, kpm, ref = mask_case(hd, name)
    got, o, lse = run_masked(hd, name)
    check(f"b. mask {name} hd={hd}", got, ref, model_of(q, k, v, dout, o, lse, H, hd, dead=kpm.view(B, 1, 1, Nk)))
    for n, t in zip(NAMES[1:], got[1:]):
        assert bool((t.cpu()[kpm] == 0).all()), f"{n} of a dead key is not exactly zero"


@pytest.mark.parametrize("hd", HDS)
def test_mask_row_stride(hd):
    """the mask of (ii) as a column view of a [B, Nk + 24] byte buffer whose other bytes say `dead`: kpm_bs != Nk, same bits"""
    B, H, Nq, Nk = MASK_SHAPE
    q, k, v, dout, kpm, ref = mask_case(hd, "step+tail")
    buf = torch.ones(B, Nk + 24, dtype=torch.uint8, device=dev())
    view = buf[:, 8:8 + Nk]
    view.copy_(kpm.to(torch.uint8))
    assert view.stride(0) == Nk + 24
    dense, _, _ = run_masked(hd, "step+tail")
    got, _, _ = run_masked(hd, "step+tail", kpm_dev=view)
    check(f"b. mask step+tail hd={hd} with row stride {Nk + 24}", got, ref)
    assert all(torch.equal(a, b) for a, b in zip(got, dense))


# ---- c. the training form ---------------------------------------------------------------------------------------------------------
def tail_padding(B, Nk):
    """per-sample tail padding and one inner key, as TK._qkv"""
    kpm = torch.zeros(B, Nk, dtype=torch.bool)
    for b in range(B):
        kpm[b, Nk - 37 - 3 * b:] = True
    kpm[0, 5] = True
    return kpm


def packed_form(what, hd, p, Nq, Nk, q_cols, out_cols):
    """One packed call.  q_cols / out_cols: (buffer width, column of q, of k, of v) for the operand and the gradient buffers
    (q and dq live in buffers of their own when the query is not part of the packed rows: column None)."""
    B, H = 2, 2
    D = H * hd
    d = dev()
    q, k, v, dout = operands(B, H, Nq, Nk, hd, seed=2)
    dout = dout * 2.0 ** -18
    kpm = tail_padding(B, Nk)
    seed = TK.BIG_SEED + Nk + hd
    # operands: column views of one packed buffer (or a dense q beside a packed K | V) whose other columns hold noise
    g = torch.Generator().manual_seed(hd)
    W, cq, ck, cv = q_cols
    pk = torch.randn(B, Nk, W, generator=g)
    pk[..., ck:ck + D], pk[..., cv:cv + D] = k, v
    if cq is not None:
        pk[..., cq:cq + D] = q
    pkd = pk.to(d)
    qd = pkd[..., cq:cq + D] if cq is not None else q.to(d)
    kd, vd = pkd[..., ck:ck + D], pkd[..., cv:cv + D]
    assert kd.stride(1) == W and not kd.is_contiguous()
    dod, kpd = dout.to(d), kpm.to(torch.uint8).to(d)
    dsc = ops.pow2_scale(dod.view(B * Nq, D))
    o, lse = ops.attention(qd, kd, vd, H, kpm=kpd, want_lse=True, drop_p=p, drop_seed=seed, prec="f16x3")

    def packed_call():
        """the gradients as column views of sentinel-filled buffers with pad columns and a spare row"""
        Wo, oq, ok, ov = out_cols
        gk = torch.full((B, Nk + 1, Wo), SENTINEL, device=d)
        gq = gk if oq is not None else torch.full((B, Nq + 1, D + 8), SENTINEL, device=d)
        outs = (gq[:, :Nq, (oq or 0):(oq or 0) + D], gk[:, :Nk, ok:ok + D], gk[:, :Nk, ov:ov + D])
        word = torch.zeros(1, dtype=torch.int32, device=d)
        ret = ops.attention_bwd(qd, kd, vd, o, lse, dod, H, kpm=kpd, drop_p=p, drop_seed=seed, do_scale=dsc, out=outs,
                                amax_out=word)
        assert all(a is b for a, b in zip(ret[:3], outs)) and ret[3] is word
        written = []
        for buf in ((gq, gk) if gq is not gk else (gk,)):
            wr = torch.zeros(buf.shape, dtype=torch.bool, device=d)
            for t, c in zip(outs, (oq or 0, ok, ov)):
                if t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr():
                    wr[:, :t.shape[1], c:c + D] = True
            written.append((buf, wr))
        return outs, word, written
    outs, word, written = packed_call()
    for buf, wr in written:
        assert untouched(buf, wr), f"{what}: a word beside the gradients (pad column or spare row) was written"
    outs2, word2, written2 = packed_call()
    assert all(torch.equal(a[0], b[0]) for a, b in zip(written, written2)) and torch.equal(word, word2)
    dense = ops.attention_bwd(qd, kd, vd, o, lse, dod, H, kpm=kpd, drop_p=p, drop_seed=seed, do_scale=dsc, want_amax=True)
    assert all(torch.equal(a, b) for a, b in zip(outs, dense[:3])), f"{what}: packed and dense outputs differ"
    assert torch.equal(word, dense[3])
    big = max(float(t.abs().max()) for t in outs)
    assert int(word.item()) == int(torch.tensor(big, dtype=torch.float32).view(torch.int32)), "the amax word"
    ref = TK._attn_drop_ref(q, k, v, H, kpm, p, seed, dout)[1:]
    model = None
    if p == 0:
        model = model_of(q, k, v, dout, o, lse, H, hd, dead=kpm.view(B, 1, 1, Nk), do_scale=float(dsc[0].cpu()))
    check(f"{what} hd={hd} {Nq}x{Nk} p={p} (dO scale 2^{int(torch.log2(dsc[0]).item())})", outs, ref, model)
    assert bool((outs[1].cpu()[kpm] == 0).all()) and bool((outs[2].cpu()[kpm] == 0).all())


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("hd", HDS)
def test_training_form_self_attention(hd, p):
    """N = 258, the smallest self-attention length the step sends to the fused path with three dQ workgroups and a two-key second
    dK / dV workgroup: Q | K | V in [B, N, 3D + 8], dQ | dK | dV in a sentinel-filled [B, N + 1, 3D + 8]"""
    D = 2 * hd
    packed_form("c. self", hd, p, 258, 258, (3 * D + 8, 0, D, 2 * D), (3 * D + 8, 0, D, 2 * D))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("hd", HDS)
def test_training_form_cross_attention(hd, p):
    """dense Q [B, 70, D] against K | V packed in [B, 200, 2D]; dK | dV packed in a sentinel-filled [B, 201, 2D + 8], dQ in a
    sentinel-filled [B, 71, D + 8]"""
    D = 2 * hd
    packed_form("c. cross", hd, p, 70, 200, (2 * D, None, 0, D), (2 * D + 8, None, 0, D))


# ---- d. the amax word is a running maximum --------------------------------------------------------------------------------------
def test_amax_word_is_a_running_maximum():
    B, H, Nq, Nk, hd = 1, 2, 33, 63, 16
    d = dev()
    qd, kd, vd, dod = (t.to(d) for t in operands(B, H, Nq, Nk, hd))
    o, lse = ops.attention(qd, kd, vd, H, want_lse=True, prec="f16x3")
    dq, dk, dv, fresh = ops.attention_bwd(qd, kd, vd, o, lse, dod, H, want_amax=True)
    big = max(float(t.abs().max()) for t in (dq, dk, dv))
    true_bits = int(torch.tensor(big, dtype=torch.float32).view(torch.int32))
    assert int(fresh.item()) == true_bits

    def seeded(value):
        word = torch.tensor([value], dtype=torch.float32, device=d).view(torch.int32)
        got = ops.attention_bwd(qd, kd, vd, o, lse, dod, H, amax_out=word)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], (dq, dk, dv)))
        return int(word.item())
    above = 4.0 * big
    assert seeded(above) == int(torch.tensor(above, dtype=torch.float32).view(torch.int32)), "a larger word must survive"
    assert seeded(1e-30) == true_bits, "a smaller word must be raised"
    zero = torch.zeros_like(dod)
    sc = ops.pow2_scale(zero.view(B * Nq, H * hd))
    word = torch.zeros(1, dtype=torch.int32, device=d)
    got = ops.attention_bwd(qd, kd, vd, o, lse, zero, H, do_scale=sc, amax_out=word)
    assert all(bool((t == 0).all()) for t in got[:3]) and int(word.item()) == 0
    print(f"d. amax word: true maximum {big:.4e}, seeds {above:.4e} (kept) and 1e-30 (raised), zero dout leaves 0")


# ---- e. a power-of-two scale of dO scales the gradients exactly ------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nk", [(33, 63), (129, 257)])
@pytest.mark.parametrize("hd", HDS)
def test_power_of_two_scale_of_dout_is_exact(hd, Nq, Nk):
    """dO enters the kernels times the power of two of pow2_scale and the results leave through its inverse; delta is the fp32
    dO . O of the unscaled values, which scales exactly too: dout * 2^k must give every gradient times 2^k, bit for bit"""
    B, H = 1, 2
    q, k, v, dout = operands(B, H, Nq, Nk, hd)
    d = dev()
    qd, kd, vd, dod = (t.to(d) for t in (q, k, v, dout))
    o, lse = ops.attention(qd, kd, vd, H, want_lse=True, prec="f16x3")

    def run(e):
        do = dod * 2.0 ** e
        sc = ops.pow2_scale(do.view(B * Nq, H * hd))
        return run_twice(qd, kd, vd, o, lse, do, H, do_scale=sc), float(sc[0].cpu())
    base, s0 = run(0)
    ref = Hh.attn_bwd_ref64(q, k, v, dout, H, hd)[:3]
    check(f"e. scale hd={hd} {Nq}x{Nk} dO scale {s0:.0f}", base, ref, model_of(q, k, v, dout, o, lse, H, hd, do_scale=s0))
    for e in (-40, 20):
        got, s = run(e)
        assert s == s0 * 2.0 ** -e
        for n, a, b in zip(NAMES, got, base):
            assert torch.equal(a, b * 2.0 ** e), f"{n} under dout * 2^{e} is not the unscaled result times 2^{e}"


# ---- f. a query shared by the samples -------------------------------------------------------------------------------------------
def test_shared_query_batch_stride_zero():
    B, H, Nq, Nk, hd = 2, 2, 33, 63, 32
    q, k, v, dout = operands(B, H, Nq, Nk, hd)
    q = q[:1].expand(B, -1, -1)
    d = dev()
    qd = q[:1].to(d).expand(B, -1, -1)
    assert qd.stride(0) == 0
    kd, vd, dod = (t.to(d) for t in (k, v, dout))
    o, lse = ops.attention(qd, kd, vd, H, want_lse=True, prec="f16x3")
    got = run_twice(qd, kd, vd, o, lse, dod, H)
    ref = Hh.attn_bwd_ref64(q, k, v, dout, H, hd)[:3]               # the per-sample dq: q enters as B separate copies
    check(f"f. shared query hd={hd} {Nq}x{Nk}", got, ref, model_of(q, k, v, dout, o, lse, H, hd))


# ---- g. refusals ----------------------------------------------------------------------------------------------------------------
def _padded(t, pad):
    """t as a view of a buffer whose rows are `pad` floats longer"""
    buf = torch.zeros(*t.shape[:-1], t.shape[-1] + pad, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def _offset(t):
    """t as a view one float into a flat buffer: its base is 4 bytes off 16-byte alignment"""
    flat = torch.zeros(t.numel() + 4, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("what", ["hd=8", "input row stride", "output row stride", "input base", "output base", "output shape"])
def test_refusals_leave_the_outputs_untouched(what):
    B, H, Nq, Nk = 1, 2, 33, 63
    hd = 8 if what == "hd=8" else 16
    D = H * hd
    d = dev()
    g = torch.Generator().manual_seed(3)
    qd, kd, vd, dod = (torch.randn(B, n, D, generator=g).to(d) for n in (Nq, Nk, Nk, Nq))
    o, lse = torch.zeros(B, Nq, D, device=d), torch.zeros(B, H, Nq, device=d)       # never read past the delta pass
    outs = [torch.full((B, n, D), SENTINEL, device=d) for n in (Nq, Nk, Nk)]
    full = list(outs)
    err, match = RuntimeError, "attention backward"
    if what == "input row stride":
        kd = _padded(kd, 2)
    elif what == "output row stride":
        full[1] = torch.full((B, Nk, D + 2), SENTINEL, device=d)
        outs[1] = full[1][..., :D]
    elif what == "input base":
        qd = _offset(qd)
    elif what == "output base":
        full[0] = torch.full((B * Nq * D + 4,), SENTINEL, device=d)
        outs[0] = full[0][1:1 + B * Nq * D].view(B, Nq, D)
    elif what == "output shape":
        outs[2] = full[2] = torch.full((B, Nk + 1, D), SENTINEL, device=d)
        err, match = ValueError, "out dv"
    word = torch.zeros(1, dtype=torch.int32, device=d)
    with pytest.raises(err, match=match) as info:
        ops.attention_bwd(qd, kd, vd, o, lse, dod, H, out=tuple(outs), amax_out=word)
    torch.cuda.synchronize()
    print(f"g. {what}: {info.value}")
    assert all(bool((t.view(torch.int32) == SENTINEL_BITS).all()) for t in full) and int(word.item()) == 0
