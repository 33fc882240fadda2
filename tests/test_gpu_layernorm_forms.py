"""Kernel-level parity of LayerNorm's fused forms (layernorm.hip through actmi_op_layernorm_ex), which the engine launches and
no other op reaches: the slices of a sliced split-K product summed in the row loader (+ bias + residual), the second output
y2 = y + pos for the next block, and the action head on the row in registers with its finiteness flag.

Bounds: float64 parity at the bounds of test_layernorm (2e-6 of the result's maximum, 4e-6 with the second norm on top); the fused
loader must give the BITS of actmi_op_splitk_combine followed by actmi_op_layernorm (the promise in the kernel's comment); y2 is
one fp32 addition, so bit-equal to y + add2; the head is a D-long fp32 FMA chain, held to the project's GEMM bound(D).
D = 64 / 512 / 772 / 1284 / 2048 give 1, 2, 4 and the default 8 float4 per lane, 772 and 1284 with dead lanes in the last
iteration.  The gap between two slices holds PAD.  Every test prints its worst error."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import rel_err  # noqa: E402
from test_gpu_gemm_backward_forms import PAD, bound  # noqa: E402
from actmi import lib as L  # noqa: E402
from actmi import ops  # noqa: E402

DS = [64, 512, 772, 1284, 2048]
MS = [1, 5, 130]
MAXS = 8


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(M, D):
    g = torch.Generator().manual_seed(M * 10000 + D)
    stride = M * D + 8                                              # larger than a slice, a multiple of 4
    slices = torch.full((MAXS, stride), PAD)
    slices[:, :M * D] = torch.randn(MAXS, M * D, generator=g) * 3
    vec = {k: torch.randn(D, generator=g) for k in ("bias", "w", "b", "w2", "b2")}
    res = torch.randn(M, D, generator=g)
    add2 = torch.randn(max(M, 7), D, generator=g)
    head_w = torch.randn(64, D, generator=g) / D ** 0.5
    head_b = torch.randn(64, generator=g)
    return dict(stride=stride, slices=slices, res=res, add2=add2, head_w=head_w, head_b=head_b, **vec)


def _x64(c, M, D, nsplit, bias, res_mod):
    """float64 input row of the norm: the slices' sum (+ bias) (+ res[m % res_mod])"""
    x = c["slices"][:nsplit, :M * D].double().sum(0).view(M, D)
    if bias:
        x = x + c["bias"].double()
    if res_mod is not None:
        rows = torch.arange(M) % res_mod if res_mod else torch.arange(M)
        x = x + c["res"][rows].double()
    return x


def _ln64(x, c, D, second):
    y = F.layer_norm(x, (D,), c["w"].double(), c["b"].double(), 1e-5)
    return F.layer_norm(y, (D,), c["w2"].double(), c["b2"].double(), 1e-5) if second else y


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_fused_slices_bias_residual(D, M):
    """nsplit 1 / 2 / 3 / 8 x bias on / off x residual none / per row / res_mod = 3 x one norm / two"""
    c = _case(M, D)
    d = dev()
    dv = {k: c[k].to(d) for k in ("slices", "bias", "w", "b", "w2", "b2", "res")}
    lib = L.load()
    worst = worst2 = 0.0
    for nsplit in (1, 2, 3, 8):
        for bias in (False, True):
            for res_mod in (None, 0, 3):
                res = None if res_mod is None else (dv["res"][:3].contiguous() if res_mod else dv["res"])
                # what the unfused path computes: combine (slices in order, + bias, + res) and then the plain LayerNorm
                res_full = None if res_mod is None else (dv["res"][torch.arange(M, device=d) % 3].contiguous() if res_mod else dv["res"])
                comb = torch.empty(M, D, device=d)
                L.check(lib.actmi_op_splitk_combine(dv["slices"].data_ptr(), nsplit, c["stride"], D, M, D, None,
                                                    dv["bias"].data_ptr() if bias else None,
                                                    res_full.data_ptr() if res_full is not None else None, D, 0, comb.data_ptr(), D,
                                                    L.current_stream_ptr()), None, "op_splitk_combine")
                x64 = _x64(c, M, D, nsplit, bias, res_mod)
                for second in (False, True):
                    w2, b2 = (dv["w2"], dv["b2"]) if second else (None, None)
                    got = ops.layernorm_ex(dv["slices"], dv["w"], dv["b"], M, D, nsplit=nsplit, split_stride=c["stride"],
                                           bias=dv["bias"] if bias else None, res=res, res_mod=res_mod or 0, w2=w2, b2=b2)
                    what = f"layernorm_ex D={D} M={M} nsplit={nsplit} bias={bias} res_mod={res_mod} second={second}"
                    e = rel_err(got, _ln64(x64, c, D, second))
                    tol = 4e-6 if second else 2e-6
                    if second:
                        worst2 = max(worst2, e)
                    else:
                        worst = max(worst, e)
                    assert e < tol, f"{what}: rel.err {e:.2e} (bound {tol:.1e})"
                    unfused = ops.layernorm(comb, dv["w"], dv["b"], w2=w2, b2=b2)
                    assert torch.equal(got, unfused), what + ": the fused loader must give the bits of combine + layernorm"
    print(f"layernorm_ex D={D} M={M}: worst {worst:.2e} (bound 2.0e-06), with the second norm {worst2:.2e} (bound 4.0e-06)")


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_second_output_and_head(D, M):
    """y2 = y + add2[row % add2_mod] (add2_mod 0 and 7) bit-equal to the fp32 sum; the head (head_n 1 / 14 / 64, with and without
    head_b) within bound(D) of y_gpu @ head_w^T + head_b in float64; a flag word pre-set to another bit stays as it is.  With
    M = 1 and head_n = 1 the norm is the relative error of ONE number: 2.86e-6 of 3.0e-6 at D = 512 without head_b, where the
    512 terms (sum of magnitudes 18.6) cancel to 0.0599 -- 1.7e-7 absolute, as everywhere else."""
    c = _case(M, D)
    d = dev()
    dv = {k: c[k].to(d) for k in ("slices", "bias", "w", "b", "res", "add2", "head_w", "head_b")}
    x64 = _x64(c, M, D, 2, True, 0)
    exp = _ln64(x64, c, D, False)
    worst_y = worst_h = 0.0
    for add2_mod in (0, 7):
        add2 = dv["add2"][:7].contiguous() if add2_mod else dv["add2"][:M].contiguous()
        rows = torch.arange(M, device=d) % add2_mod if add2_mod else torch.arange(M, device=d)
        for head_n in (1, 14, 64):
            for with_b in (True, False):
                flag = torch.full((1,), 4, dtype=torch.int32, device=d)
                hw = dv["head_w"][:head_n].contiguous()
                hb = dv["head_b"][:head_n].contiguous() if with_b else None
                y, y2, head = ops.layernorm_ex(dv["slices"], dv["w"], dv["b"], M, D, nsplit=2, split_stride=c["stride"], bias=dv["bias"],
                                               res=dv["res"], add2=add2, add2_mod=add2_mod, head_w=hw, head_b=hb, flag=flag, flag_bit=1)
                what = f"layernorm_ex extras D={D} M={M} add2_mod={add2_mod} head_n={head_n} head_b={with_b}"
                e = rel_err(y, exp)
                worst_y = max(worst_y, e)
                assert e < 2e-6, f"{what}: y rel.err {e:.2e} (bound 2.0e-06)"
                assert torch.equal(y2, y + add2[rows]), what + ": y2 must be the fp32 sum y + add2[row % add2_mod]"
                hexp = y.cpu().double() @ c["head_w"][:head_n].double().t() + (c["head_b"][:head_n].double() if with_b else 0.0)
                eh = rel_err(head, hexp)
                worst_h = max(worst_h, eh)
                assert tuple(head.shape) == (M, head_n) and eh < bound(D), f"{what}: head rel.err {eh:.2e} (bound {bound(D):.1e})"
                assert int(flag) == 4, what + ": every head output is finite, the flag word must not change"
    print(f"layernorm_ex extras D={D} M={M}: y worst {worst_y:.2e} (bound 2.0e-06), head worst {worst_h:.2e} (bound {bound(D):.1e})")


@pytest.mark.parametrize("D", [64, 1284])
def test_head_finiteness_flag(D):
    """an inf in one head_w row, then a NaN in one x row: the flag word (pre-set to 4) gains exactly flag_bit"""
    M = 5
    c = _case(M, D)
    d = dev()
    x, w, b = c["slices"][0, :M * D].view(M, D).to(d), c["w"].to(d), c["b"].to(d)
    hw, hb = c["head_w"][:14].contiguous().to(d), c["head_b"][:14].contiguous().to(d)

    def run(x_, hw_, bit):
        flag = torch.full((1,), 4, dtype=torch.int32, device=d)
        _, _, head = ops.layernorm_ex(x_, w, b, M, D, head_w=hw_, head_b=hb, flag=flag, flag_bit=bit)
        return int(flag), head
    f0, head = run(x, hw, 1)
    assert f0 == 4 and bool(torch.isfinite(head).all())
    hw_inf = hw.clone()
    hw_inf[9, 3] = float("inf")
    f1, head = run(x, hw_inf, 1)
    assert f1 == 5 and not bool(torch.isfinite(head[:, 9]).all())
    x_nan = x.clone()
    x_nan[3, 1] = float("nan")
    f2, head = run(x_nan, hw, 2)
    assert f2 == 6 and bool(torch.isnan(head[3]).all()) and bool(torch.isfinite(head[[0, 1, 2, 4]]).all())
    print(f"layernorm_ex flag D={D}: 4 -> 4 finite, 4 -> 5 with an inf in head_w, 4 -> 6 with a NaN in x (flag_bit 2)")


@pytest.mark.parametrize("case,match", [("y2 without add2", "bad second output"), ("head without head_w", "bad head"),
                                        ("slice stride", "slice stride")])
def test_launcher_rejections(case, match):
    M, D = 5, 64
    c = _case(M, D)
    d = dev()
    kw = dict(nsplit=2, split_stride=c["stride"])
    if case == "y2 without add2":
        kw["want_y2"] = True
    elif case == "head without head_w":
        kw.update(want_head=True, head_n=3)
    else:
        kw["split_stride"] = M * D + 2
    with pytest.raises(RuntimeError, match=match):
        ops.layernorm_ex(c["slices"].to(d), c["w"].to(d), c["b"].to(d), M, D, **kw)
