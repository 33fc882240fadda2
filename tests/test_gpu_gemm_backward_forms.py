"""Kernel-level parity of the GEMM launch forms that only the training backward uses (gemm.hip through actmi_op_gemm):
transposed operands, the convolution gathers, the epilogue extensions, two-level groups with the fused attention-backward
epilogues, operand scales and the amax word -- in every precision and under every tile shape, against plain float64 on the CPU.

Bounds.  f32 and f16x3: the project's bound for these forms, 3e-6 * max(1, sqrt(K / 512)) of the reference's maximum.  bf16 is
held to the SAME bound against an emulated reference: operands rounded to bf16 (round to nearest even, after the fp32 addend
where one applies), products in float64 -- products of bf16 values are exact in fp32, so only the accumulation order differs
(fp32 accumulation against that reference: 1.2e-7 .. 1.5e-7 on the CPU at these shapes).  A bf16 result must also be MORE than
1e-4 away from the unrounded product (2e-3 .. 3e-3 here): the mode was active.  Every test prints its worst error."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import rel_err, run_gemm  # noqa: E402
from actmi import ops  # noqa: E402

PRECS = ["f32", "f16x3", "bf16"]
PREC = {"f32": 1, "f16x3": 2, "bf16": 3}
TILES = [1, 2, 3]           # 128x128, 128x64, 64x64
PAD = 7.0                   # what the padding of a leading dimension holds: finite, and wrong if it ever reached a product
SENTINEL = 123.0            # what output elements the launch does not own hold before and after


def dev():
    return torch.device("cuda:0")


def bound(K):
    return 3e-6 * max(1.0, (K / 512) ** 0.5)


def rb(x):
    """bf16 rounding as pack_bf16x4 does it (round to nearest even), back in fp32"""
    return x.float().bfloat16().float()


def up4(n):
    return (n + 3) // 4 * 4


def padded(x, ld, fill=PAD):
    """x [R][C] as the leading rows x columns of a [R][ld] matrix whose padding holds `fill`"""
    out = torch.full((x.shape[0], ld), fill, dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return out


def bits(x):
    """int32 bits of max |x|"""
    return int(x.detach().abs().max().float().cpu().view(torch.int32))


def check(what, got, exp, tol, exp_unrounded=None):
    """rel_err(got, exp) < tol; for bf16 also the distance to the unrounded product.  Returns the error."""
    e = rel_err(got, exp)
    msg = f"{what}: rel.err {e:.2e} (bound {tol:.1e})"
    if exp_unrounded is not None:
        gap = rel_err(got, exp_unrounded)
        msg += f", bf16 distance to the unrounded product {gap:.2e}"
    print(msg)
    assert e < tol, msg
    if exp_unrounded is not None:
        assert gap > 1e-4, msg + ": bf16 products cannot be this close -- the mode was not active"
    return e


# ---------------------------------------------------------------------------------------------------------------------------
# a. operand form x precision x tile shape
# ---------------------------------------------------------------------------------------------------------------------------
FORMS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0), "TT": (1, 1)}


@functools.lru_cache(maxsize=None)
def _form_operands(M, N, K, a_mag, b_mag):
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
    A = torch.randn(M, K, generator=g) * a_mag
    B = torch.randn(K, N, generator=g) * b_mag
    return A, B, A.double() @ B.double(), rb(A).double() @ rb(B).double()


def _run_form(form, prec, tile, M, N, K, a_mag=1.0, b_mag=1.0, a_dev=False, b_scale=0.0, b_dev=False):
    ta, tb = FORMS[form]
    A, B, exp, exp_bf = _form_operands(M, N, K, a_mag, b_mag)
    d = dev()
    # storage: [out][contraction] unless transposed; every leading dimension padded to a multiple of 4 (+4: ld > width), the
    # padding at the operand's own magnitude so that a measured operand scale is the operand's
    As = (padded(A.t(), up4(M) + 4, PAD * a_mag) if ta else padded(A, up4(K) + 4, PAD * a_mag)).to(d)
    Bs = (padded(B, up4(N) + 4, PAD * b_mag) if tb else padded(B.t(), up4(K) + 4, PAD * b_mag)).to(d)
    ldc = up4(N) + 4
    out = torch.full((M, ldc), SENTINEL, device=d)
    kw = dict(A=As, lda=As.shape[1], ta=ta, Bw=Bs, ldb=Bs.shape[1], tb=tb, M=M, N=N, K=K, C=out, ldc=ldc, groups=1,
              prec=PREC[prec], tile_hint=tile, b_scale=b_scale)
    if a_dev:
        kw["a_scale_dev"] = ops.pow2_scale(As[:, :M] if ta else As[:, :K])
    if b_dev:
        kw["b_scale_dev"] = ops.pow2_scale(Bs[:, :N] if tb else Bs[:, :K])
    run_gemm(f"gemm {form}", **kw)
    what = f"{form} {prec} tile {tile} ({M},{N},{K}) |A| {a_mag:g} |B| {b_mag:g}"
    e = check(what, out[:, :N], exp_bf if prec == "bf16" else exp, bound(K), exp if prec == "bf16" else None)
    assert bool((out[:, N:] == SENTINEL).all()), what + ": columns beyond N were written"
    return e


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("M,N,K", [(130, 68, 100), (300, 200, 70)])
def test_operand_forms(M, N, K, form, prec, tile):
    """ragged rows and columns under every tile, full and ragged blocks (the 16-byte-store epilogue and the scalar one), K no
    multiple of 32.  NN and TN store B contraction-contiguous, which launch_gemm accepts only with K % 4 == 0 ("ldb and K must be
    multiples of 4 for a contraction-contiguous B"): K = 70 becomes 72 for these two forms.  f16x3 runs every form again at the
    magnitudes of a gradient (A at 1e-6 with its device-side scale, B at 0.02 with the static 2^8), and NT / TT once more with B
    at 3e4 -- beyond the fp16 range unscaled -- under a device-side scale: the bound does not move, so each form's loader
    applies the scale and the epilogue undoes it exactly once."""
    if FORMS[form][1] == 0 and K % 4:
        K = up4(K)
    worst = _run_form(form, prec, tile, M, N, K)
    if prec == "f16x3":
        worst = max(worst, _run_form(form, prec, tile, M, N, K, a_mag=1e-6, b_mag=0.02, a_dev=True, b_scale=256.0))
        if FORMS[form][1] == 1:
            worst = max(worst, _run_form(form, prec, tile, M, N, K, b_mag=3e4, b_dev=True))
    print(f"a. operand forms: worst {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# b. the convolution gathers in every precision
# ---------------------------------------------------------------------------------------------------------------------------
CONVS = [(2, 2, 12, 16, 8, 16, 3, 1, 1), (1, 2, 15, 20, 16, 32, 3, 2, 1), (2, 1, 16, 24, 16, 32, 1, 2, 0),
         (1, 1, 30, 40, 64, 64, 3, 1, 1), (1, 2, 15, 21, 16, 32, 3, 2, 1)]


def _conv_grads(x, w, dy, stride, pad):
    """float64 autograd of the per-group convolution: (dx, dw) for the output gradient dy"""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    for i in range(x.shape[0]):
        F.conv2d(x[i], w[i], None, stride, pad).backward(dy[i].double())
    return x.grad, w.grad


@functools.lru_cache(maxsize=None)
def _conv_case(G, B, H, W, Cin, Cout, k, stride, pad, dy_mag):
    g = torch.Generator().manual_seed(H * 3 + Cin + W)
    x = torch.randn(G, B, Cin, H, W, generator=g)
    w = torch.randn(G, Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn(G, B, Cout, Ho, Wo, generator=g) * dy_mag
    dx, dw = _conv_grads(x, w, dy, stride, pad)
    dx_bf, _ = _conv_grads(x, rb(w), rb(dy), stride, pad)
    _, dw_bf = _conv_grads(rb(x), w, rb(dy), stride, pad)
    # epilogue operands of the data gradient, at the magnitude of dx
    dx_mag = float(dx.abs().max())
    res = torch.randn(G, B, Cin, H, W, generator=g) * (0.3 * dx_mag)
    mask = torch.randn(G, B, Cin, H, W, generator=g)
    mask[mask.abs() < 0.3] = 0.0                                  # zeros, negatives and positives
    scale = torch.rand(G, Cin, generator=g) + 0.5
    gw0 = torch.randn(G, Cout, Cin, k, k, generator=g) * (0.5 * float(dw.abs().max()))
    return dict(x=x, w=w, dy=dy, dx=dx, dw=dw, dx_bf=dx_bf, dw_bf=dw_bf, res=res, mask=mask, scale=scale, gw0=gw0, Ho=Ho, Wo=Wo)


def nhwc(t):
    return t.permute(0, 1, 3, 4, 2).contiguous().float()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("G,B,H,W,Cin,Cout,k,stride,pad", CONVS)
def test_conv_gathers(G, B, H, W, Cin, Cout, k, stride, pad, prec, tile):
    """the data gradient (mode 2) with the epilogue of conv_dgrad -- C = where(mask > 0, acc * scale[g][n] + res, 0), per-group
    strides, the amax word -- and the weight gradient (ta=1, tb=2), non-split accumulating onto a non-zero buffer through
    res = C and split in two with atomics.  f16x3 runs with dy at 1e-6 under its device-side scale (and 2^8 on the data
    gradient's weights), as the backward does."""
    c = _conv_case(G, B, H, W, Cin, Cout, k, stride, pad, 1e-6 if prec == "f16x3" else 1.0)
    d = dev()
    Ho, Wo, KK = c["Ho"], c["Wo"], k * k
    bf = prec == "bf16"
    dy = nhwc(c["dy"]).to(d)
    x = nhwc(c["x"]).to(d)
    dy_sc = ops.pow2_scale(dy.view(-1, Cout)) if prec == "f16x3" else None
    geom = dict(H=H, W=W, Cin=Cin, KH=k, KW=k, stride=stride, pad=pad, Ho=Ho, Wo=Wo, groups=G, prec=PREC[prec], tile_hint=tile,
                a_scale_dev=dy_sc)
    # ---- data gradient: weights [G][Cin][(r,s,n)]
    wd = c["w"].permute(0, 2, 3, 4, 1).contiguous().to(d)
    res, mask, scale = nhwc(c["res"]).to(d), nhwc(c["mask"]).to(d), c["scale"].to(d)
    dx = torch.full((G, B, H, W, Cin), SENTINEL, device=d)
    amax = torch.zeros(1, dtype=torch.int32, device=d)
    nx = B * H * W * Cin
    run_gemm("dgrad", mode=2, A=dy, img_stride=Ho * Wo * Cout, M=B * H * W, N=Cin, K=KK * Cout, Bw=wd, ldb=KK * Cout, C=dx,
             ldc=Cin, gA=B * Ho * Wo * Cout, gB=Cin * KK * Cout, gC=nx, res=res, ldres=Cin, gRes=nx, mask=mask, ldmask=Cin,
             gMask=nx, scale=scale, gSB=Cin, b_scale=256.0 if prec == "f16x3" else 0.0, amax_out=amax, **geom)

    def dx_ref(raw):
        v = raw * c["scale"].double().view(G, 1, Cin, 1, 1) + c["res"].double()
        return torch.where(c["mask"] > 0, v, torch.zeros_like(v))
    tag = f"{prec} tile {tile} conv {(G, B, H, W, Cin, Cout, k, stride, pad)}"
    worst = check("dgrad " + tag, dx.permute(0, 1, 4, 2, 3), dx_ref(c["dx_bf"] if bf else c["dx"]), bound(KK * Cout),
                  dx_ref(c["dx"]) if bf else None)
    assert int(amax) == bits(dx), "amax_out must hold the bits of the largest stored magnitude"
    # ---- weight gradient [G][Cout][(r,s,c)]
    wg = dict(A=dy, lda=Cout, ta=1, M=Cout, K=B * Ho * Wo, Bw=x, tb=2, N=KK * Cin, img_stride=H * W * Cin, ldc=KK * Cin,
              gA=B * Ho * Wo * Cout, gB=B * H * W * Cin, gC=Cout * KK * Cin, **geom)
    gw0 = c["gw0"].permute(0, 1, 3, 4, 2).contiguous()                                      # [G][Cout][k][k][Cin]
    exp = (c["dw_bf"] if bf else c["dw"]) + c["gw0"].double()
    exp_un = c["dw"] + c["gw0"].double() if bf else None
    gw = gw0.clone().to(d)
    run_gemm("wgrad", C=gw, res=gw, ldres=KK * Cin, gRes=Cout * KK * Cin, **wg)
    worst = max(worst, check("wgrad res=C " + tag, gw.permute(0, 1, 4, 2, 3), exp, bound(B * Ho * Wo), exp_un))
    gw = gw0.clone().to(d)
    run_gemm("wgrad splitk", C=gw, splitk=2, **wg)
    worst = max(worst, check("wgrad splitk=2 " + tag, gw.permute(0, 1, 4, 2, 3), exp, bound(B * Ho * Wo), exp_un))
    print(f"b. gathers: worst {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------------
# c. epilogue extensions, each against its formula
# ---------------------------------------------------------------------------------------------------------------------------
EPRECS = ["f32", "f16x3"]


@pytest.mark.parametrize("prec", EPRECS)
@pytest.mark.parametrize("N,ldc,ldres,ldmask", [(200, 204, 208, 212), (198, 199, 201, 203)])
def test_alpha_res_mask(N, ldc, ldres, ldmask, prec):
    """lin_dgrad: C = where(mask > 0, alpha * A @ B + res, 0) with ldmask, ldres and ldc all larger than N and all different.
    N = 200 with leading dimensions that are multiples of 4: full blocks leave through the 16-byte-store epilogue; N = 198 with
    odd leading dimensions: the scalar one everywhere.  A at 1e-4 with its device-side scale, B at 0.02 with the static 2^8."""
    M, K, alpha = 250, 96, 1.0 / 0.9
    g = torch.Generator().manual_seed(N)
    A, B = torch.randn(M, K, generator=g) * 1e-4, torch.randn(K, N, generator=g) * 0.02
    raw = alpha * (A.double() @ B.double())
    res = torch.randn(M, N, generator=g) * (0.5 * float(raw.abs().max()))
    mask = torch.randn(M, N, generator=g)
    mask[mask.abs() < 0.3] = 0.0                                   # zeros, negatives and positives
    exp = torch.where(mask > 0, raw + res.double(), torch.zeros_like(raw))
    d = dev()
    Ad, Bd = A.to(d), padded(B, up4(N), PAD * 0.02).to(d)
    out = torch.full((M, ldc), SENTINEL, device=d)
    run_gemm("lin_dgrad", A=Ad, lda=K, M=M, N=N, K=K, Bw=Bd, ldb=up4(N), tb=1, C=out, ldc=ldc, res=padded(res, ldres).to(d),
             ldres=ldres, mask=padded(mask, ldmask, 1.0).to(d), ldmask=ldmask, alpha=alpha, b_scale=256.0,
             a_scale_dev=ops.pow2_scale(Ad), prec=PREC[prec], groups=1)
    check(f"c. alpha+res+mask {prec} N={N} ld {ldc}/{ldres}/{ldmask}", out[:, :N], exp, bound(K))
    assert bool((out[:, N:] == SENTINEL).all())
    assert bool((out[:, :N].cpu()[mask <= 0] == 0).all())          # killed elements are exactly zero


@pytest.mark.parametrize("prec", EPRECS)
def test_second_output_with_mask_and_rowmap(prec):
    """the feature-complete epilogue: C[rowmap[m]][n] = v = where(mask[m][n] > 0, A @ W^T, 0) and C2[rowmap[m]][n] = v * scale2[n]"""
    M, N, K, extra = 250, 200, 96, 9
    g = torch.Generator().manual_seed(17)
    A, Wt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    mask = torch.randn(M, N, generator=g)
    mask[mask.abs() < 0.3] = 0.0
    scale2 = torch.rand(N, generator=g) + 0.5
    rowmap = torch.randperm(M + extra, generator=g)[:M].to(torch.int32)
    v = torch.where(mask > 0, A.double() @ Wt.double().t(), torch.zeros(M, N, dtype=torch.float64))
    exp = torch.full((M + extra, N), SENTINEL, dtype=torch.float64)
    exp2 = exp.clone()
    exp[rowmap.long()] = v
    exp2[rowmap.long()] = v * scale2.double()
    d = dev()
    out, out2 = torch.full((M + extra, N), SENTINEL, device=d), torch.full((M + extra, N), SENTINEL, device=d)
    run_gemm("C2", A=A.to(d), lda=K, M=M, N=N, K=K, Bw=Wt.to(d), ldb=K, C=out, ldc=N, C2=out2, scale2=scale2.to(d),
             mask=mask.to(d), ldmask=N, rowmap=rowmap.to(d), prec=PREC[prec], groups=1)
    check(f"c. C {prec}", out, exp, bound(K))
    check(f"c. C2 = C * scale2 {prec}", out2, exp2, bound(K))


@pytest.mark.parametrize("prec", EPRECS)
def test_a_rowmap_gather(prec):
    """the additional_pos_embed launch: A rows gathered through a_rowmap (repeats, out of order) from a wider matrix
    (lda > K), B stored [K][N]; f16x3 with the device-side scale of A and 2^8 on the weights"""
    M, N, K, rows, lda = 250, 200, 96, 300, 144
    g = torch.Generator().manual_seed(23)
    src = torch.randn(rows, lda, generator=g) * 1e-5
    B = torch.randn(K, N, generator=g) * 0.02
    amap = torch.randint(0, rows, (M,), generator=g).to(torch.int32)
    amap[:4] = torch.tensor([299, 0, 299, 7])
    assert len(set(amap.tolist())) < M and bool((amap[1:] < amap[:-1]).any())       # repeats, and not sorted
    exp = src[amap.long(), :K].double() @ B.double()
    d = dev()
    srcd = src.to(d)
    out = torch.zeros(M, N, device=d)
    run_gemm("a_rowmap", A=srcd, lda=lda, a_rowmap=amap.to(d), M=M, N=N, K=K, Bw=B.to(d), ldb=N, tb=1, C=out, ldc=N,
             b_scale=256.0, a_scale_dev=ops.pow2_scale(srcd[:, :K]), prec=PREC[prec], groups=1)
    check(f"c. a_rowmap {prec}", out, exp, bound(K))


@pytest.mark.parametrize("prec", EPRECS)
def test_b_addend(prec):
    """lin_wgrad with pos: both operands stored [contraction][out], B'[k][n] = B[k][n] + B_add[k % badd_mod][n], badd_mod = 36
    not dividing K = 96; f16x3 with the device-side scale of A (dY)"""
    M, N, K, mod = 250, 200, 96, 36
    g = torch.Generator().manual_seed(29)
    At = torch.randn(K, M, generator=g) * 1e-5                      # dY [rows][out]
    B, add = torch.randn(K, N, generator=g), torch.randn(mod, N, generator=g)
    exp = At.double().t() @ (B + add[torch.arange(K) % mod]).double()
    d = dev()
    Atd = padded(At, up4(M), PAD * 1e-5).to(d)
    out = torch.zeros(M, N, device=d)
    run_gemm("B_add", A=Atd, lda=up4(M), ta=1, M=M, N=N, K=K, Bw=B.to(d), ldb=N, tb=1, B_add=add.to(d), ld_badd=N, badd_mod=mod,
             C=out, ldc=N, a_scale_dev=ops.pow2_scale(Atd[:, :M]), prec=PREC[prec], groups=1)
    check(f"c. B_add {prec}", out, exp, bound(K))


@pytest.mark.parametrize("prec,b_split", [("f32", False), ("f16x3", False), ("f16x3", True)])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("N", [256, 200])
def test_a_alt(N, tile, prec, b_split):
    """the packed q | k | v projection: column blocks below alt_ncols = 128 contract A_alt, the rest contract A"""
    M, K, alt = 250, 96, 128
    g = torch.Generator().manual_seed(N)
    A, A2, Wt = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    exp = torch.cat([A2.double() @ Wt[:alt].double().t(), A.double() @ Wt[alt:].double().t()], dim=1)
    d = dev()
    Wd = Wt.to(d)
    out = torch.zeros(M, N, device=d)
    run_gemm("A_alt", A=A.to(d), A_alt=A2.to(d), alt_ncols=alt, lda=K, M=M, N=N, K=K, Bw=ops.split16(Wd) if b_split else Wd, ldb=K,
             b_split=int(b_split), C=out, ldc=N, prec=PREC[prec], tile_hint=tile, groups=1)
    check(f"c. A_alt {prec} b_split={b_split} tile {tile} N={N}", out, exp, bound(K))


@pytest.mark.parametrize("prec", EPRECS)
@pytest.mark.parametrize("N,ldc", [(200, 200), (198, 199)])
def test_amax_word(N, ldc, prec):
    """amax_out: exactly the int32 bits of max |C| over both groups, on the 16-byte-store epilogue (N = 200) and the scalar one
    (N = 198, odd ldc); a second launch with smaller values leaves the word as it is (it holds an earlier maximum)"""
    M, K, G = 250, 96, 2
    g = torch.Generator().manual_seed(N)
    A, B = torch.randn(G, M, K, generator=g), torch.randn(G, K, up4(N), generator=g)
    B[1] *= 3.0                                                      # the maximum lies in the second group
    d = dev()
    Ad, Bd = A.to(d), B.to(d)
    out = torch.zeros(G, M, ldc, device=d)
    amax = torch.zeros(1, dtype=torch.int32, device=d)
    kw = dict(lda=K, M=M, N=N, K=K, Bw=Bd, ldb=up4(N), tb=1, C=out, ldc=ldc, groups=G, gA=M * K, gB=K * up4(N), gC=M * ldc,
              amax_out=amax, prec=PREC[prec])
    run_gemm("amax", A=Ad, **kw)
    exp = torch.bmm(A.double(), B.double()[:, :, :N])
    check(f"c. amax product {prec} N={N}", out[:, :, :N], exp, bound(K))
    first = int(amax)
    assert first == bits(out[:, :, :N]) and float(out[1].abs().max()) > float(out[0].abs().max())
    run_gemm("amax again", A=Ad * 0.5, **kw)
    assert int(amax) == first and bits(out[:, :, :N]) < first


def test_finite_flag():
    """finite_flag: a finite output leaves the word alone (zero stays zero, set bits stay set); one inf in A ORs finite_bit in"""
    M, N, K = 250, 200, 96
    g = torch.Generator().manual_seed(31)
    A, Wt = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    d = dev()
    Ad, Wd = A.to(d), Wt.to(d)
    out = torch.zeros(M, N, device=d)
    flag = torch.zeros(1, dtype=torch.int32, device=d)
    kw = dict(lda=K, M=M, N=N, K=K, Bw=Wd, ldb=K, C=out, ldc=N, groups=1, finite_flag=flag, finite_bit=2, prec=PREC["f32"])
    run_gemm("finite", A=Ad, **kw)
    assert int(flag) == 0
    flag.fill_(4)
    run_gemm("finite", A=Ad, **kw)
    assert int(flag) == 4
    Ainf = Ad.clone()
    Ainf[131, 5] = float("inf")
    run_gemm("inf", A=Ainf, **kw)
    assert int(flag) == 6 and not bool(torch.isfinite(out[131]).all())
    print("c. finite_flag: 0 -> 0, 4 -> 4, 4 -> 6 with one inf in A")


# ---------------------------------------------------------------------------------------------------------------------------
# d. two-level groups and the fused attention-backward epilogues (the layout of attn_bwd in train.hip)
# ---------------------------------------------------------------------------------------------------------------------------
AB, AH, HD, NQ = 2, 3, 16, 70
AD = AH * HD
DO_MAG = 3e-7
# Nk = 50 (ldp = 52): every block is ragged, the scalar epilogue.  Nk = 130 (ldp = 132): full 64- and 128-wide blocks carry
# the same epilogues through the 16-byte-store form as well
NKS = [50, 130]


def heads(t, n):
    """[B][n][H*HD] -> [B][H][n][HD]"""
    return t.reshape(AB, n, AH, HD).permute(0, 2, 1, 3)


def unheads(t, n):
    """[B][H][n][HD] -> [B][n][H*HD]"""
    return t.permute(0, 2, 1, 3).reshape(AB, n, AD)


@functools.lru_cache(maxsize=None)
def _attn_case(NK, margin=None):
    """margin: the scores carry an attention sink (helpers.attn_sink_case): per head, component 0 of every key is zero, key 0
    (visible under both masks) is e_0 with a zero value vector, q[..., 0] = margin * sqrt(HD)"""
    g = torch.Generator().manual_seed(41 + NK)
    q = torch.randn(AB, NQ, AD, generator=g)
    kv = torch.randn(AB, NK, 2 * AD, generator=g)                   # interleaved K | V rows: k_rs = v_rs = 2 * D
    dO = torch.randn(AB, NQ, AD, generator=g) * DO_MAG
    if margin is not None:
        kv[..., :AD].view(AB, NK, AH, HD)[..., 0] = 0.0
        kv[:, 0] = 0.0
        kv[:, 0, :AD].view(AB, AH, HD)[..., 0] = 1.0
        q.view(AB, NQ, AH, HD)[..., 0] = margin * HD ** 0.5
    kpm = torch.zeros(AB, NK, dtype=torch.bool)
    kpm[0, 44:] = True                                              # the mask differs per batch
    kpm[1, 5] = True
    kpm[1, 30:37] = True
    scale = 1.0 / HD ** 0.5
    qd = q.double().requires_grad_(True)
    kvd = kv.double().requires_grad_(True)
    s = scale * heads(qd, NQ) @ heads(kvd[..., :AD], NK).transpose(-1, -2)
    s = s.masked_fill(kpm.view(AB, 1, 1, NK), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)                                # [B][H][Nq], from the masked float64 scores
    O = unheads(torch.softmax(s, dim=-1) @ heads(kvd[..., AD:], NK), NQ)
    O.backward(dO.double())
    delta = (heads(dO.double(), NQ) * heads(O.detach(), NQ)).sum(-1)                      # [B][H][Nq]
    return dict(q=q, kv=kv, dO=dO, kpm=kpm, scale=scale, lse=lse.detach().float(), delta=delta.float(),
                dq=qd.grad, dk=kvd.grad[..., :AD], dv=kvd.grad[..., AD:])


def _p_ref(c, q, k):
    """exp(scale * q k^T - lse) with the saved (fp32) log-sum-exp, killed columns exactly zero: [B][H][Nq][Nk] float64"""
    NK = k.shape[1]
    s = c["scale"] * heads(q.double(), NQ) @ heads(k.double(), NK).transpose(-1, -2)
    return torch.exp(s - c["lse"].double().unsqueeze(-1)).masked_fill(c["kpm"].view(AB, 1, 1, NK), 0.0)


def _launch_p(c, prec, tile, q, kv, P):
    """S = scale * Q K^T -> P = exp(S - lse), the first launch of attn_bwd; P is [B][H][Nq][ldp]"""
    d = dev()
    NK, ldp = kv.shape[1], P.shape[-1]
    pg = NQ * ldp
    lse, kill = c["lse"].to(d), c["kpm"].to(torch.uint8).to(d)
    run_gemm("epi 1", A=q, lda=AD, M=NQ, K=HD, Bw=kv, ldb=2 * AD, N=NK, C=P, ldc=ldp, alpha=c["scale"], groups=AB * AH,
             groups_inner=AH, gA=NQ * AD, gA2=HD, gB=NK * 2 * AD, gB2=HD, gC=pg * AH, gC2=pg, epi=1, epi_row=lse,
             gRow=AH * NQ, gRow2=NQ, epi_colkill=kill, gColkill=NK, prec=PREC[prec], tile_hint=tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("NK", NKS)
def test_epi1_probabilities(NK, prec, tile):
    """epi = 1 with two-level groups: gRow = H * Nq = 210, gRow2 = Nq = 70 and gColkill = Nk are all different, so a swapped
    stride shows; killed columns are exactly 0; the columns Nk .. ldp-1 are not the kernel's (launch_zero_cols owns them) and
    keep their sentinel"""
    c = _attn_case(NK)
    d = dev()
    P = torch.full((AB, AH, NQ, up4(NK)), SENTINEL, device=d)
    _launch_p(c, prec, tile, c["q"].to(d), c["kv"].to(d), P)
    bf = prec == "bf16"
    exp = _p_ref(c, c["q"], c["kv"][..., :AD])
    exp_bf = _p_ref(c, rb(c["q"]), rb(c["kv"][..., :AD]))
    check(f"d. epi=1 {prec} tile {tile} Nk={NK}", P[..., :NK], exp_bf if bf else exp, bound(HD), exp if bf else None)
    assert bool((P[..., :NK].cpu()[c["kpm"].view(AB, 1, 1, NK).expand(AB, AH, NQ, NK)] == 0).all())
    assert bool((P[..., NK:] == SENTINEL).all()), "the padding columns of P are not the kernel's to write"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("NK", NKS)
def test_epi2_score_gradient(NK, prec, tile):
    """epi = 2: dS = P * (dO V^T - delta) * epi_scale with res = P as a FACTOR.  P lives in a buffer of its own row stride
    (ldres = ldp + 4), so gRes / gRes2 differ from gC / gC2; dO at 3e-7 under its device-side scale; the amax word holds the
    bits of max |dS|"""
    c = _attn_case(NK)
    d = dev()
    ldp = up4(NK)
    ldr = ldp + 4
    Pref = _p_ref(c, c["q"], c["kv"][..., :AD]).float()                                   # [B][H][Nq][Nk]
    Pd = torch.zeros(AB, AH, NQ, ldr)
    Pd[..., :NK] = Pref
    Pd = Pd.to(d)
    dO, kv = c["dO"].to(d), c["kv"].to(d)
    dS = torch.full((AB, AH, NQ, ldp), SENTINEL, device=d)
    amax = torch.zeros(1, dtype=torch.int32, device=d)
    pg, pr = NQ * ldp, NQ * ldr
    run_gemm("epi 2", A=dO, lda=AD, M=NQ, K=HD, Bw=kv[..., AD:], ldb=2 * AD, N=NK, C=dS, ldc=ldp, groups=AB * AH, groups_inner=AH,
             gA=NQ * AD, gA2=HD, gB=NK * 2 * AD, gB2=HD, gC=pg * AH, gC2=pg, a_scale_dev=ops.pow2_scale(dO.view(-1, AD)),
             epi=2, epi_scale=c["scale"], epi_row=c["delta"].to(d), gRow=AH * NQ, gRow2=NQ, res=Pd, ldres=ldr, gRes=pr * AH,
             gRes2=pr, amax_out=amax, prec=PREC[prec], tile_hint=tile)

    def ref(dOx, vx):
        dP = heads(dOx.double(), NQ) @ heads(vx.double(), NK).transpose(-1, -2)
        return Pref.double() * (dP - c["delta"].double().unsqueeze(-1)) * c["scale"]
    bf = prec == "bf16"
    exp = ref(c["dO"], c["kv"][..., AD:])
    check(f"d. epi=2 {prec} tile {tile} Nk={NK}", dS[..., :NK], ref(rb(c["dO"]), rb(c["kv"][..., AD:])) if bf else exp, bound(HD),
          exp if bf else None)
    assert bool((dS[..., NK:] == SENTINEL).all())
    assert int(amax) == bits(dS[..., :NK])


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("NK", NKS)
def test_attention_backward_chain(NK, prec, tile):
    """the whole materialised chain with the descriptors of attn_bwd: P (epi 1), dV = P^T dO (ta, tb, a_scale = 2^8,
    b_scale_dev), dS (epi 2), dQ = dS K (tb, a_scale_dev) and dK = dS^T Q (ta, tb, a_scale_dev), dO at 3e-7; dQ / dK / dV land in
    packed [.][3 * D] rows as in the encoder's gQKV and raise ONE amax word.  Every product is checked against float64 (bf16:
    the emulated reference) of the operands it actually read; in f32 and f16x3 the three gradients are also compared with
    float64 autograd at 2e-5 of each tensor's maximum, the project's bound for this quantity."""
    c = _attn_case(NK)
    d = dev()
    bf = prec == "bf16"
    ldp = up4(NK)
    q, kv, dO = c["q"].to(d), c["kv"].to(d), c["dO"].to(d)
    pg = NQ * ldp
    P = torch.zeros(AB, AH, NQ, ldp, device=d)                       # zero-filled: the padding columns must be finite
    dS = torch.zeros(AB, AH, NQ, ldp, device=d)
    gq = torch.zeros(AB, NQ, 3 * AD, device=d)                       # dQ in columns [0, D)
    gkv = torch.zeros(AB, NK, 3 * AD, device=d)                      # dK in [D, 2D), dV in [2D, 3D)
    amax = torch.zeros(1, dtype=torch.int32, device=d)
    common = dict(groups=AB * AH, groups_inner=AH, prec=PREC[prec], tile_hint=tile)
    dO_sc = ops.pow2_scale(dO.view(-1, AD))
    _launch_p(c, prec, tile, q, kv, P)
    run_gemm("dV", A=P, lda=ldp, ta=1, M=NK, K=NQ, Bw=dO, ldb=AD, tb=1, N=HD, C=gkv[..., 2 * AD:], ldc=3 * AD, gA=pg * AH, gA2=pg,
             gB=NQ * AD, gB2=HD, gC=NK * 3 * AD, gC2=HD, a_scale=256.0, b_scale_dev=dO_sc, amax_out=amax, **common)
    run_gemm("dS", A=dO, lda=AD, M=NQ, K=HD, Bw=kv[..., AD:], ldb=2 * AD, N=NK, C=dS, ldc=ldp, gA=NQ * AD, gA2=HD, gB=NK * 2 * AD,
             gB2=HD, gC=pg * AH, gC2=pg, a_scale_dev=dO_sc, epi=2, epi_scale=c["scale"], epi_row=c["delta"].to(d), gRow=AH * NQ,
             gRow2=NQ, res=P, ldres=ldp, gRes=pg * AH, gRes2=pg, **common)
    dS_sc = ops.pow2_scale(dS.view(-1, ldp)[:, :NK])
    run_gemm("dQ", A=dS, lda=ldp, M=NQ, K=NK, Bw=kv, ldb=2 * AD, tb=1, N=HD, C=gq, ldc=3 * AD, gA=pg * AH, gA2=pg,
             gB=NK * 2 * AD, gB2=HD, gC=NQ * 3 * AD, gC2=HD, a_scale_dev=dS_sc, amax_out=amax, **common)
    run_gemm("dK", A=dS, lda=ldp, ta=1, M=NK, K=NQ, Bw=q, ldb=AD, tb=1, N=HD, C=gkv[..., AD:], ldc=3 * AD, gA=pg * AH, gA2=pg,
             gB=NQ * AD, gB2=HD, gC=NK * 3 * AD, gC2=HD, a_scale_dev=dS_sc, amax_out=amax, **common)
    dQ, dK, dV = gq[..., :AD], gkv[..., AD:2 * AD], gkv[..., 2 * AD:]
    assert not bool(gq[..., AD:].any()) and not bool(gkv[..., :AD].any())           # nothing outside the three column blocks
    r = rb if bf else (lambda t: t)
    Pc, dSc = P[..., :NK].cpu(), dS[..., :NK].cpu()
    Kc, Qc, dOc = c["kv"][..., :AD], c["q"], c["dO"]
    per = [("dV", dV, NQ, lambda f: unheads(f(Pc).double().transpose(-1, -2) @ heads(f(dOc).double(), NQ), NK)),
           ("dQ", dQ, NK, lambda f: unheads(f(dSc).double() @ heads(f(Kc).double(), NK), NQ)),
           ("dK", dK, NQ, lambda f: unheads(f(dSc).double().transpose(-1, -2) @ heads(f(Qc).double(), NQ), NK))]
    for name, got, K, ref in per:
        check(f"d. chain {name} {prec} tile {tile} Nk={NK}", got, ref(r), bound(K), ref(lambda t: t) if bf else None)
    assert int(amax) == max(bits(dQ), bits(dK), bits(dV)), "one amax word for the three products"
    if not bf:
        for name, got, exp in (("dQ", dQ, c["dq"]), ("dK", dK, c["dk"]), ("dV", dV, c["dv"])):
            e = rel_err(got, exp)
            print(f"d. chain {name} against float64 autograd, {prec} tile {tile} Nk={NK}: {e:.2e} (bound 2.0e-05)")
            assert e < 2e-5, (name, e)


# ---------------------------------------------------------------------------------------------------------------------------
# e. the fused epilogues are rejected, not dropped, where the kernel would take the epilogue that has none
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,match", [("rowmap", "epi.*row map"), ("C2", "epi.*C2"), ("dropout", "epi.*dropout"),
                                        ("res_mod", "epi.*res_mod"), ("atomic split-K", "epi.*split-K"),
                                        ("M*ldc", r"epi.*2\^31"), ("M*ldres", r"epi.*2\^31"), ("M*ldmask", r"epi.*2\^31")])
@pytest.mark.parametrize("epi", [1, 2])
def test_epi_is_rejected_outside_the_fast_epilogue(epi, case, match):
    """a row map, C2, dropout, res_mod, an atomic split-K and offsets at or above 2^31 send a launch to the feature-complete
    epilogue, which knows no epi: launch_gemm used to accept these and store plain products.  (M = 4 with a leading dimension of
    2^29 reaches 2^31 without the memory: the check comes before any launch.)"""
    M, N, K, big = 4, 64, 64, 1 << 29
    d = dev()
    A, Wt = torch.randn(M, K, device=d), torch.randn(N, K, device=d)
    out, out2, other = torch.zeros(M, N, device=d), torch.zeros(M, N, device=d), torch.ones(M, N, device=d)
    row, ones = torch.zeros(M, device=d), torch.ones(N, device=d)
    base = dict(A=A, lda=K, M=M, N=N, K=K, Bw=Wt, ldb=K, C=out, ldc=N, groups=1, epi=epi, epi_row=row, epi_scale=1.0, res=other,
                ldres=N, prec=PREC["f32"])
    run_gemm("epi alone", **base)                                    # accepted without the extra
    extra = {"rowmap": dict(rowmap=torch.arange(M, dtype=torch.int32, device=d)), "C2": dict(C2=out2, scale2=ones),
             "dropout": dict(drop_p=0.1, drop_seed=3), "res_mod": dict(res_mod=2), "atomic split-K": dict(splitk=2),
             "M*ldc": dict(ldc=big), "M*ldres": dict(ldres=big), "M*ldmask": dict(mask=other, ldmask=big)}[case]
    with pytest.raises(RuntimeError, match=match):
        run_gemm("epi + " + case, **{**base, **extra})
