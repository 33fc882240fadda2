"""Kernel-level parity of the GEMM launch forms of the INFERENCE forward (gemm.hip through actmi_op_gemm): the broadcast addend
with its column limit, the feature-complete epilogue (row map, res_mod, scale / bias, ReLU), the dropout epilogue element by
element, the 16-byte-store and the scalar plain epilogue, pre-split weights, the sliced split-K with its combine pass, the
second-source convolution and the taps-inner K order -- under every tile shape (tile_hint 1 / 2 / 3) and in every precision,
against plain float64 on the CPU.

Bounds and layout are those of test_gpu_gemm_backward_forms.py: the project's bound(K) = 3e-6 * max(1, sqrt(K / 512)) of the
reference's maximum for f32, f16x3 and bf16 (bf16 against operands rounded to bf16 AFTER the fp32 addend, products in float64,
and more than 1e-4 away from the unrounded product: the mode was active).  The padding of every leading dimension holds PAD,
output elements a launch does not own hold SENTINEL before and after.  Every test prints its worst error."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import host_keep, rel_err  # noqa: E402
from test_gpu_gemm_backward_forms import PAD, PRECS, SENTINEL, TILES, bound, check, padded, rb, run_gemm  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402

PREC = {"f32": 1, "f16x3": 2, "bf16": 3}


def dev():
    return torch.device("cuda:0")


def act64(x, act):
    return F.relu(x) if act == 1 else (F.gelu(x) if act == 2 else x)


# ---------------------------------------------------------------------------------------------------------------------------
# a. the broadcast addend: A'[m] = A[m] + A_add[m % add_mod] for the columns n < add_ncols
# ---------------------------------------------------------------------------------------------------------------------------
AM, AN = 150, 192            # M ragged for the 128- and the 64-row tile
W_MAG = 0.05                 # weights at a network's magnitude: the 2^8 pre-scale is what the engine uses for them


@functools.lru_cache(maxsize=None)
def _add_case(K, add_mod):
    g = torch.Generator().manual_seed(K * 7 + add_mod)
    A = torch.randn(AM, K, generator=g)
    add = torch.randn(add_mod, K, generator=g)
    W = torch.randn(AN, K, generator=g) * W_MAG
    Aa = A + add[torch.arange(AM) % add_mod]                       # the fp32 sum the loader forms
    ref = {}
    for name, f in (("exact", lambda t: t), ("bf16", rb)):
        ref[name] = (f(Aa).double() @ f(W).double().t(), f(A).double() @ f(W).double().t())
    return A, add, W, ref


def _add_expected(ref, add_ncols):
    with_add, without = ref
    out = without.clone()
    n = min(add_ncols, AN)
    out[:, :n] = with_add[:, :n]
    return out


def _run_addend(K, add_mod, add_ncols, prec, tile, b_scale=0.0, b_split=0.0):
    A, add, W, ref = _add_case(K, add_mod)
    d = dev()
    ld = K + 4
    Wd = padded(W, ld).to(d)
    if b_split:
        Wd = ops.split16(Wd, b_split)
    out = torch.full((AM, AN + 4), SENTINEL, device=d)
    run_gemm("addend", A=padded(A, ld).to(d), lda=ld, A_add=padded(add, ld).to(d), ld_add=ld, add_mod=add_mod, add_ncols=add_ncols,
             Bw=Wd, ldb=ld, M=AM, N=AN, K=K, C=out, ldc=AN + 4, groups=1, prec=PREC[prec], tile_hint=tile,
             b_split=1 if b_split else 0, b_scale=b_split if b_split else b_scale)
    assert bool((out[:, AN:] == SENTINEL).all()), "columns beyond N were written"
    return out[:, :AN]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K", [64, 72])
def test_addend(K, prec, tile):
    """add_ncols = 64 / 128 (inside N, the second one a multiple of the wide tile), 192 (= N) and 256 (> N); add_mod = 50 (rows
    repeat) and 150 (= M); ld_add = K + 4.  K = 64 runs the unmasked f16x3 flavour (plain weights and the pre-split image), K = 72
    the masked one with a K tail.  f16x3 three ways: plain weights, b_scale = 2^8 in the loader, a pre-split image built with 2^8;
    and a pre-split image at scale 1 gives the bits of plain weights."""
    worst = 0.0
    for add_mod in (50, 150):
        ref = _add_case(K, add_mod)[3]
        for add_ncols in (64, 128, 192, 256):
            exp = _add_expected(ref["bf16" if prec == "bf16" else "exact"], add_ncols)
            exp_un = _add_expected(ref["exact"], add_ncols) if prec == "bf16" else None
            what = f"a. addend {prec} tile {tile} K={K} add_mod={add_mod} add_ncols={add_ncols}"
            plain = _run_addend(K, add_mod, add_ncols, prec, tile)
            worst = max(worst, check(what, plain, exp, bound(K), exp_un))
            if prec == "f16x3":
                worst = max(worst, check(what + " b_scale=256", _run_addend(K, add_mod, add_ncols, prec, tile, b_scale=256.0), exp,
                                         bound(K)))
                worst = max(worst, check(what + " b_split(256)", _run_addend(K, add_mod, add_ncols, prec, tile, b_split=256.0), exp,
                                         bound(K)))
                assert torch.equal(_run_addend(K, add_mod, add_ncols, prec, tile, b_split=1.0), plain), \
                    what + ": a pre-split image at scale 1 must give the bits of plain weights"
    print(f"a. addend: worst {worst:.2e}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K", [64, 72])
def test_add_ncols_narrower_than_the_tile(K, prec):
    """the decoder's K | V product at hidden_dim = 64: add_ncols = 64 with N > 64.  The addend is block-uniform in the kernel, so
    a 128-wide tile would hand it to the columns 64 .. 127 as well: the automatic choice and every hint must stay within bound (a
    hint for the 128-wide tile falls back to 128x64), and an add_ncols that no tile width divides is rejected."""
    ref = _add_case(K, 50)[3]
    exp = _add_expected(ref["bf16" if prec == "bf16" else "exact"], 64)
    exp_un = _add_expected(ref["exact"], 64) if prec == "bf16" else None
    worst = 0.0
    for tile in (0, 1, 2, 3):
        worst = max(worst, check(f"add_ncols=64 {prec} K={K} tile_hint {tile}", _run_addend(K, 50, 64, prec, tile), exp, bound(K),
                                 exp_un))
    print(f"a. add_ncols = 64 under every hint: worst {worst:.2e}")
    with pytest.raises(RuntimeError, match="add_ncols"):
        _run_addend(K, 50, 96, prec, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# b / c. the feature-complete epilogue: groups, row map, res_mod, scale / bias, ReLU -- and dropout, element by element
# ---------------------------------------------------------------------------------------------------------------------------
EG, EM, EN, ELDC, EXTRA = 2, 150, 136, 140, 11
ELDRES = 144


@functools.lru_cache(maxsize=None)
def _epi_case(K):
    g = torch.Generator().manual_seed(100 + K)
    A = torch.randn(EG, EM, K, generator=g)
    W = torch.randn(EG, EN, K, generator=g) / K ** 0.5
    scale, bias = torch.rand(EG, EN, generator=g) + 0.5, torch.randn(EG, EN, generator=g)
    res = torch.randn(EG, EM, EN, generator=g)                     # res_mod = r reads its first r rows
    rowmap = torch.randperm(EM + EXTRA, generator=g)[:EM].to(torch.int32)
    acc = torch.bmm(A.double(), W.double().transpose(1, 2))
    acc_bf = torch.bmm(rb(A).double(), rb(W).double().transpose(1, 2))
    return dict(A=A, W=W, scale=scale, bias=bias, res=res, rowmap=rowmap, acc=acc, acc_bf=acc_bf)


def _epi_launch(c, K, prec, tile, rows_out, **extra):
    """the shared geometry: groups = 2 with gA / gB / gSB / gC / gRes, ldc = 140 > N = 136, every leading dimension padded"""
    d = dev()
    ld = K + 4
    A = torch.stack([padded(c["A"][i], ld) for i in range(EG)]).to(d)
    W = torch.stack([padded(c["W"][i], ld) for i in range(EG)]).to(d)
    out = torch.full((EG, rows_out, ELDC), SENTINEL, device=d)
    kw = dict(A=A, lda=ld, Bw=W, ldb=ld, M=EM, N=EN, K=K, C=out, ldc=ELDC, groups=EG, gA=EM * ld, gB=EN * ld, gSB=EN,
              gC=rows_out * ELDC, scale=c["scale"].to(d), bias=c["bias"].to(d), prec=PREC[prec], tile_hint=tile)
    kw.update(extra)
    run_gemm("epilogue", **kw)
    return out, kw


def _res_operand(c, res_mod):
    """[G][rows][ldres] with PAD in the padding; res_mod = r > 0 keeps r rows only (a read past them would leave the tensor)"""
    rows = res_mod if res_mod else EM
    return torch.stack([padded(c["res"][i, :rows], ELDRES) for i in range(EG)]), rows


def _res64(c, res_mod):
    rows = torch.arange(EM) % res_mod if res_mod else torch.arange(EM)
    return c["res"][:, rows].double()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K", [96, 72])
def test_full_epilogue(K, prec, tile):
    """C[g][rowmap[m]][n] = relu(acc * scale[g][n] + bias[g][n] + res[g][m % res_mod][n]), res_mod 1 and 7, ReLU on and off; the
    rows the permutation does not name and the columns N .. ldc-1 keep their sentinel.  K = 96: the unmasked f16x3 loop,
    K = 72: the masked one."""
    c = _epi_case(K)
    d = dev()
    bf = prec == "bf16"
    worst = 0.0
    for res_mod in (1, 7):
        res, rows = _res_operand(c, res_mod)
        for relu in (0, 1):
            out, _ = _epi_launch(c, K, prec, tile, EM + EXTRA, rowmap=c["rowmap"].to(d), res=res.to(d), ldres=ELDRES,
                                 gRes=rows * ELDRES, res_mod=res_mod, relu=relu)

            def expected(acc):
                v = act64(acc * c["scale"].double().unsqueeze(1) + c["bias"].double().unsqueeze(1) + _res64(c, res_mod), relu)
                e = torch.full((EG, EM + EXTRA, ELDC), SENTINEL, dtype=torch.float64)
                e[:, c["rowmap"].long(), :EN] = v
                return e
            exp = expected(c["acc_bf"] if bf else c["acc"])
            what = f"b. full epilogue {prec} tile {tile} K={K} res_mod={res_mod} relu={relu}"
            owned = torch.zeros(EM + EXTRA, dtype=torch.bool)
            owned[c["rowmap"].long()] = True
            got = out.cpu()
            worst = max(worst, check(what, got[:, owned, :EN], exp[:, owned, :EN], bound(K),
                                     expected(c["acc"])[:, owned, :EN] if bf else None))
            assert bool((got[:, ~owned] == SENTINEL).all()), what + ": a row outside the row map was written"
            assert bool((got[:, :, EN:] == SENTINEL).all()), what + ": columns beyond N were written"
    print(f"b. full epilogue: worst {worst:.2e}")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("seed", [7, 2 ** 40 + 3])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_epilogue_exact(p, seed, prec, tile):
    """the keep mask is actmi_keep(seed, g * gC + orow * ldc + n, p) -- the element's offset in the OUTPUT buffer, with the group
    offset, the mapped row and ldc (not N): predicted on the host element by element.  dropout(relu(x)) (the FFN hidden layer: no
    residual) and res + dropout(x) (the projections; res_mod 0 and 1), without and with a row map.  Dropped elements are bit-equal
    to the residual (or zero), kept ones within bound of x / (1 - p) + res in float64, a second launch gives the same bits."""
    K = 96
    c = _epi_case(K)
    d = dev()
    bf = prec == "bf16"
    x64 = {name: c[name] * c["scale"].double().unsqueeze(1) + c["bias"].double().unsqueeze(1) for name in ("acc", "acc_bf")}
    worst = 0.0
    for with_map in (False, True):
        rows_out = EM + EXTRA if with_map else EM
        orow = c["rowmap"].long() if with_map else torch.arange(EM)
        gC = rows_out * ELDC
        idx = (torch.arange(EG).view(EG, 1, 1) * gC + orow.view(1, EM, 1) * ELDC + torch.arange(EN).view(1, 1, EN)).numpy()
        assert int(idx.max()) < 2 ** 32
        keep = torch.from_numpy(host_keep(seed, idx.astype(np.uint64), p))
        assert 0.6 * (1 - p) < float(keep.float().mean()) < 1 - 0.6 * p          # the mask is neither empty nor full
        for form, res_mod in (("relu", None), ("res", 0), ("res", 1)):
            extra = dict(drop_p=p, drop_seed=seed)
            if with_map:
                extra["rowmap"] = c["rowmap"].to(d)
            if form == "relu":
                extra["relu"] = 1
                r64 = torch.zeros(EG, EM, EN, dtype=torch.float64)
            else:
                res, rows = _res_operand(c, res_mod)
                extra.update(res=res.to(d), ldres=ELDRES, gRes=rows * ELDRES, res_mod=res_mod)
                r64 = _res64(c, res_mod)
            out, kw = _epi_launch(c, K, prec, tile, rows_out, **extra)

            def expected(x):
                x = F.relu(x) if form == "relu" else x
                return torch.where(keep, x / (1.0 - p), torch.zeros_like(x)) + r64
            got = out.cpu()[:, orow, :EN]
            what = f"c. dropout {form} res_mod={res_mod} rowmap={with_map} {prec} tile {tile} p={p} seed={seed}"
            worst = max(worst, check(what, got, expected(x64["acc_bf" if bf else "acc"]), bound(K),
                                     expected(x64["acc"]) if bf else None))
            assert torch.equal(got[~keep], r64.float()[~keep]), what + ": a dropped element must be exactly its residual (or 0)"
            assert bool((out[:, :, EN:] == SENTINEL).all()), what + ": columns beyond N were written"
            if with_map:
                owned = torch.zeros(rows_out, dtype=torch.bool)
                owned[orow] = True
                assert bool((out.cpu()[:, ~owned] == SENTINEL).all()), what + ": a row outside the row map was written"
            first = out.clone()
            out.fill_(SENTINEL)
            run_gemm("dropout again", **kw)
            assert torch.equal(out, first), what + ": the mask must be a pure function of (seed, element)"
    print(f"c. dropout epilogue: worst {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# d. the plain epilogue in its 16-byte-store and its scalar form
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_case():
    M, N, K = 150, 256, 96
    g = torch.Generator().manual_seed(77)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    scale, bias, res = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)

    def ref(f, act):
        return act64((f(A).double() @ f(W).double().t()) * scale.double() + bias.double() + res.double(), act)
    refs = {(name, act): ref(f, act) for name, f in (("exact", lambda t: t), ("bf16", rb)) for act in (1, 2)}
    return M, N, K, A, W, scale, bias, res, refs


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "gelu"])
def test_vector_and_scalar_plain_epilogue(act, prec, tile):
    """the same product act(acc * scale + bias + res) twice.  Aligned: N = 256 (full blocks under every tile), ldc and ldres
    multiples of 4 -- the 16-byte-store form.  Unaligned: ldc = N + 1, ldres = N + 3 and the bias pointer one float off a 16-byte
    boundary -- the scalar form everywhere.  Both within bound, the padding columns untouched."""
    M, N, K, A, W, scale, bias, res, refs = _plain_case()
    d = dev()
    bf = prec == "bf16"
    exp, exp_un = refs[("bf16" if bf else "exact", act)], refs[("exact", act)] if bf else None
    Ad, Wd, sc = padded(A, K + 4).to(d), padded(W, K + 4).to(d), scale.to(d)
    bias_buf = torch.cat([torch.full((1,), PAD), bias, torch.full((3,), PAD)]).to(d)
    worst = 0.0
    for name, ldc, ldres, bptr in (("aligned", N + 4, N + 8, bias.to(d)), ("unaligned", N + 1, N + 3, bias_buf[1:1 + N])):
        assert (bptr.data_ptr() % 16 == 0) == (name == "aligned")
        out = torch.full((M, ldc), SENTINEL, device=d)
        run_gemm(name, A=Ad, lda=K + 4, Bw=Wd, ldb=K + 4, M=M, N=N, K=K, C=out, ldc=ldc, groups=1, scale=sc, bias=bptr,
                 res=padded(res, ldres).to(d), ldres=ldres, relu=act, prec=PREC[prec], tile_hint=tile)
        what = f"d. {name} plain epilogue act={act} {prec} tile {tile}"
        worst = max(worst, check(what, out[:, :N], exp, bound(K), exp_un))
        assert bool((out[:, N:] == SENTINEL).all()), what + ": the padding columns were written"
    print(f"d. plain epilogue: worst {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# e. sliced split-K and its combine pass
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _split_case(N):
    M, K = 150, 200
    g = torch.Generator().manual_seed(N)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    scale, bias, res = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    lin = {name: (f(A).double() @ f(W).double().t()) * scale.double() + bias.double() + res.double()
           for name, f in (("exact", lambda t: t), ("bf16", rb))}
    return M, K, A, W, scale, bias, res, lin


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "gelu"])
@pytest.mark.parametrize("N", [136, 134])
def test_sliced_splitk_and_combine(N, act, prec, tile):
    """K = 200 is 7 K tiles: 3 splits own 3 / 3 / 1 of them and the K tail (200 = 6 * 32 + 8) falls into the last.  Every split
    stores its slice plainly at C + s * M * N; actmi_op_splitk_combine sums them in order and carries scale + bias + res and the
    activation: N = 136 through its 16-byte form, N = 134 through the scalar one.  Bit-repeatable, within bound of float64, and
    within 1e-5 absolute of the one-pass product with the same epilogue."""
    M, K, A, W, scale, bias, res, lin = _split_case(N)
    S = 3
    d = dev()
    bf = prec == "bf16"
    Ad, Wd = padded(A, K + 4).to(d), padded(W, K + 4).to(d)
    sc, bi, rs = scale.to(d), bias.to(d), padded(res, N + 8).to(d)
    common = dict(A=Ad, lda=K + 4, Bw=Wd, ldb=K + 4, M=M, N=N, K=K, groups=1, prec=PREC[prec], tile_hint=tile)
    ldo = N + 4
    lib = L.load()

    def split_run():
        part = torch.full((S, M, N), SENTINEL, device=d)
        run_gemm("slices", C=part, ldc=N, splitk=S, split_stride=M * N, **common)
        out = torch.full((M, ldo), SENTINEL, device=d)
        L.check(lib.actmi_op_splitk_combine(part.data_ptr(), S, M * N, N, M, N, sc.data_ptr(), bi.data_ptr(), rs.data_ptr(), N + 8,
                                            act, out.data_ptr(), ldo, L.current_stream_ptr()), None, "op_splitk_combine")
        return out
    two, again = split_run(), split_run()
    assert torch.equal(two, again)                                   # no atomics: bitwise repeatable
    one = torch.full((M, ldo), SENTINEL, device=d)
    run_gemm("one pass", C=one, ldc=ldo, scale=sc, bias=bi, res=rs, ldres=N + 8, relu=act, **common)
    what = f"e. sliced split-K N={N} act={act} {prec} tile {tile}"
    exp, exp_un = act64(lin["bf16" if bf else "exact"], act), act64(lin["exact"], act) if bf else None
    worst = max(check(what, two[:, :N], exp, bound(K), exp_un), check(what + " (one pass)", one[:, :N], exp, bound(K), exp_un))
    gap = float((two[:, :N] - one[:, :N]).abs().max())
    print(f"{what}: split against one pass {gap:.2e} absolute (bound 1.0e-05); worst {worst:.2e}")
    assert gap < 1e-5
    assert bool((two[:, N:] == SENTINEL).all()) and bool((one[:, N:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# f. the second-source convolution and the taps-inner K order under every tile (f16x3)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _second_source_case(G, B, H, W, Cc, Cx, Cout):
    """the operands and the float64 reference of test_conv2_with_downsample_as_second_source (test_gpu_kernels.py)"""
    g = torch.Generator().manual_seed(G * 100 + H)
    Hx, Wx = 2 * H - (H % 2), 2 * W - (W % 2)
    y1 = torch.randn(G, B, Cc, H, W, generator=g)
    x = torch.randn(G, B, Cx, Hx, Wx, generator=g)
    w2 = torch.randn(G, Cout, Cc, 3, 3, generator=g) / (9 * Cc) ** 0.5
    wd = torch.randn(G, Cout, Cx, 1, 1, generator=g) / Cx ** 0.5
    s2, sd = torch.rand(G, Cout, generator=g) + 0.5, torch.rand(G, Cout, generator=g) * 2 + 0.1
    b2, bd = torch.randn(G, Cout, generator=g) * 0.1, torch.randn(G, Cout, generator=g) * 0.1
    exp = torch.stack([torch.relu(F.conv2d(y1[i].double(), w2[i].double(), None, 1, 1) * s2[i].double().view(1, -1, 1, 1)
                                  + b2[i].double().view(1, -1, 1, 1)
                                  + F.conv2d(x[i].double(), wd[i].double(), None, 2, 0) * sd[i].double().view(1, -1, 1, 1)
                                  + bd[i].double().view(1, -1, 1, 1)) for i in range(G)])
    wf = torch.cat([(w2 * s2.view(G, Cout, 1, 1, 1)).permute(0, 1, 3, 4, 2).reshape(G, Cout, 9 * Cc),
                    (wd * sd.view(G, Cout, 1, 1, 1)).reshape(G, Cout, Cx)], dim=2).contiguous()
    return y1.permute(0, 1, 3, 4, 2).contiguous(), x.permute(0, 1, 3, 4, 2).contiguous(), wf, b2 + bd, exp


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("G,B,H,W,Cc,Cx,Cout,splitk", [(1, 2, 7, 9, 64, 32, 96, 2), (2, 2, 15, 20, 64, 32, 64, 0)])
def test_second_source_under_every_tile(G, B, H, W, Cc, Cx, Cout, splitk, tile):
    """the two smallest cases of test_conv2_with_downsample_as_second_source (one of them sliced split-K), in both K orders"""
    y1, x, wf, bias, exp = _second_source_case(G, B, H, W, Cc, Cx, Cout)
    d = dev()
    y1, x, wf, bias = y1.to(d), x.to(d), wf.to(d), bias.to(d)
    got = ops.conv2d_with_second_source(y1, x, ops.split16(wf, 256.0), 256.0, bias, splitk=splitk, tile_hint=tile)
    got2 = ops.conv2d_with_second_source(y1, x, ops.split16(ops.permute_conv_k(wf, 9, Cc), 256.0), 256.0, bias, splitk=splitk,
                                         k_tap_inner=True, tile_hint=tile)
    e, e2 = rel_err(got.permute(0, 1, 4, 2, 3), exp), rel_err(got2.permute(0, 1, 4, 2, 3), exp)
    print(f"f. second source {(G, B, H, W, Cc, Cx, Cout, splitk)} tile {tile}: {e:.2e}, taps inner {e2:.2e} (bound 3.0e-06)")
    assert e < 3e-6 and e2 < 3e-6


@functools.lru_cache(maxsize=None)
def _taps_inner_case(G, B, H, W, Cin, Cout, stride):
    g = torch.Generator().manual_seed(Cin + H)
    x = torch.randn(G, B, H, W, Cin, generator=g)
    w = torch.randn(G, Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
    bias = torch.randn(G, Cout, generator=g)
    exp = torch.stack([torch.relu(F.conv2d(x[i].permute(0, 3, 1, 2).double(), w[i].permute(0, 3, 1, 2).double(), bias[i].double(),
                                           stride, 1)) for i in range(G)])
    return x, w, bias, exp


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("G,B,H,W,Cin,Cout,stride", [(1, 1, 9, 11, 32, 256, 1), (2, 2, 15, 20, 64, 64, 1)])
def test_taps_inner_under_every_tile(G, B, H, W, Cin, Cout, stride, tile):
    """the two smallest cases of test_conv_k_order_taps_inner: the permuted weight rows give the convolution of the (tap, channel)
    rows under the same tile (2e-6, that test's bound), and both agree with torch's conv2d in float64 (the bound of
    test_conv_implicit_gemm)"""
    x, w, bias, exp = _taps_inner_case(G, B, H, W, Cin, Cout, stride)
    d = dev()
    x, w, bias = x.to(d), w.to(d), bias.to(d)
    kw = dict(bias=bias, relu=True, stride=stride, pad=1, prec="f16x3", b_scale=256.0, tile_hint=tile)
    ref = ops.conv2d_nhwc(x, w, **kw)
    wp = ops.permute_conv_k(w.reshape(G * Cout, 9 * Cin), 9, Cin)
    got = ops.conv2d_nhwc(x, wp.reshape(G, Cout, 3, 3, Cin), k_tap_inner=True, **kw)
    tol = 2e-6 * max(1.0, (9 * Cin / 512) ** 0.5)
    e, e_ref, e_got = rel_err(got, ref), rel_err(ref.permute(0, 1, 4, 2, 3), exp), rel_err(got.permute(0, 1, 4, 2, 3), exp)
    print(f"f. taps inner {(G, B, H, W, Cin, Cout, stride)} tile {tile}: {e:.2e} against the (tap, channel) order (bound 2.0e-06), "
          f"{e_ref:.2e} / {e_got:.2e} against float64 (bound {tol:.1e})")
    assert e < 2e-6 and e_ref < tol and e_got < tol
