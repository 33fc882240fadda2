"""Kernel-level parity of the training step's non-GEMM kernels (csrc/bwd.hip, the training variants of csrc/pool.hip), each
through its own actmi_op_* entry against a plain float64 reference on the CPU (torch autograd where there is one), at the
smallest shapes that reach every branch.  Elementwise kernels are held to bit equality with the fp32 formula; sums to the
project's bounds for them.  The dropout kernels are compared under the exact mask: tests/helpers.py transcribes actmi_keep,
and the first test pins that transcription against the device.  Every test prints its worst error."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import host_keep, rel_err, run_gemm  # noqa: E402
from actmi import ops  # noqa: E402
import test_gpu_gemm_backward_forms as GB  # noqa: E402  (the attention-chain helpers: one definition)

PRECS = ["f32", "f16x3"]
SENTINEL = 123.0
BIG_SEED = (0x5A17 << 32) | 0x9E3779B1           # above 2^32: the high seed word takes part


def dev():
    return torch.device("cuda:0")


def bits(x):
    """int32 bits of max |x|"""
    return int(x.detach().abs().max().float().cpu().view(torch.int32))


def word(value=0):
    return torch.full((1,), value, dtype=torch.int32, device=dev())


def mask_t(seed, shape, p):
    """keep mask of the elements 0 .. prod(shape)-1 in row-major order, as a bool tensor of that shape"""
    n = int(np.prod(shape))
    assert n < 2 ** 32
    return torch.from_numpy(host_keep(seed, np.arange(n, dtype=np.uint64), p)).view(*shape)


# ---------------------------------------------------------------------------------------------------------------------------
# 0. the host transcription of actmi_keep, pinned against the device
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [0, 987654321, BIG_SEED])
def test_host_mask_equals_the_device_mask(seed, p):
    """ops.dropout(ones) != 0 is the device's keep(seed, i, p) for i < n: element for element the host transcription (low index
    word only: see helpers.host_keep)"""
    n = 100003
    got = (ops.dropout(torch.ones(n, device=dev()), p, seed) != 0).cpu().numpy()
    exp = host_keep(seed, np.arange(n, dtype=np.uint64), p)
    diff = int((got != exp).sum())
    print(f"0. keep mask seed {seed:#x} p {p}: {diff} of {n} elements differ, kept fraction {exp.mean():.4f}")
    assert diff == 0
    assert abs(float(exp.mean()) - (1 - p)) < 0.01              # and it is a mask of the asked rate, not a constant


# ---------------------------------------------------------------------------------------------------------------------------
# 1. max pool with codes, and its backward
# ---------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 1, 1, 4, False), (2, 2, 3, 4, False), (3, 7, 9, 8, False), (2, 8, 10, 64, False), (4, 23, 31, 64, False),
              (3, 7, 9, 8, True),                      # one whole image of zeros (every window of it tied)
              (3, 260, 340, 64, False)]                # 1 060 800 float4 outputs against 4096 x 256 threads: the kernels' loops run twice


def _tie_rule_is_tested(tied, H, W):
    """at least a quarter of the windows tied, one of them in the padded first row or column (a 1 x 1 map has no tie to offer)"""
    return H * W == 1 or (float(tied.float().mean()) >= 0.25 and bool(tied[:, :, 0, :].any() or tied[:, :, :, 0].any()))


@functools.lru_cache(maxsize=None)
def _pool_case(nimg, H, W, C, zero_img):
    """the first of the seeds 0, 1, .. whose draw is tied enough (the small maps have a few dozen windows only)"""
    for k in range(20):
        c = _pool_draw(nimg, H, W, C, zero_img, 1000 * H + 10 * W + C + int(zero_img) + 7919 * k)
        if _tie_rule_is_tested(c["tied"], H, W):
            return c
    raise AssertionError("no draw with a quarter of its windows tied")


def _pool_draw(nimg, H, W, C, zero_img, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.round(2 * torch.randn(nimg, H, W, C, generator=g)) / 2)       # quantised post-ReLU map: ties everywhere
    if zero_img:
        x[1] = 0.0
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(nimg, Ho, Wo, C, generator=g)
    xn = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y, ind = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    y.backward(dy.permute(0, 3, 1, 2).double())
    # flat plane index -> window position r*3+s
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    codes = ((ind // W - (2 * ho - 1)) * 3 + (ind % W - (2 * wo - 1))).permute(0, 2, 3, 1).contiguous()
    assert int(codes.min()) >= 0 and int(codes.max()) <= 8
    y32 = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    # tie statistics: windows whose maximum is held by two or more positions
    win = F.pad(xn.detach(), (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2)         # [n][C][Ho][Wo][3][3]
    tied = (win == y.detach()[..., None, None]).sum((-1, -2)) >= 2
    # the kernel's sum: fp32, windows ho outer, wo inner; and the absolute sum of the terms
    hi = torch.arange(H).view(1, H, 1, 1)
    wi = torch.arange(W).view(1, 1, W, 1)
    dx32 = torch.zeros(nimg, H, W, C)
    dxabs = torch.zeros(nimg, H, W, C, dtype=torch.float64)
    for a in (0, 1):
        hw = (hi >> 1) + a
        okh = (hw <= ((hi + 1) >> 1)) & (hw < Ho)
        hwc = hw.clamp(max=Ho - 1).expand(1, H, W, 1)
        for b in (0, 1):
            ww = (wi >> 1) + b
            okw = (ww <= ((wi + 1) >> 1)) & (ww < Wo)
            wwc = ww.clamp(max=Wo - 1).expand(1, H, W, 1)
            me = (hi - (2 * hw - 1)) * 3 + (wi - (2 * ww - 1))
            cw = codes[:, hwc[0, :, :, 0], wwc[0, :, :, 0], :]                     # [n][H][W][C]
            gw = dy[:, hwc[0, :, :, 0], wwc[0, :, :, 0], :]
            term = torch.where((okh & okw) & (cw == me), gw, torch.zeros(()))
            dx32 = dx32 + term
            dxabs = dxabs + term.double().abs()
    return dict(x=x, dy=dy, y=y32, codes=codes.to(torch.uint8), dx64=xn.grad.permute(0, 2, 3, 1).contiguous(), dx32=dx32,
                dxabs=dxabs, tied=tied, Ho=Ho, Wo=Wo)


def test_pool_inputs_are_full_of_ties():
    """CPU-side precondition of the pool tests: at least a quarter of all windows have a tied maximum, in every case whose windows
    can hold more than one element (H * W > 1), and some window that starts in the padding (first row or column) is tied"""
    total = tied = 0
    for case in POOL_CASES:
        c = _pool_case(*case)
        t = c["tied"]
        total += t.numel()
        tied += int(t.sum())
        assert _tie_rule_is_tested(t, case[1], case[2]), (case, float(t.float().mean()))
    print(f"1. pool inputs: {tied} of {total} windows tied")
    assert tied >= total / 4


@pytest.mark.parametrize("nimg,H,W,C,zero_img", POOL_CASES)
def test_maxpool_codes_and_backward(nimg, H, W, C, zero_img):
    """forward bit-equal to F.max_pool2d, codes equal to return_indices (first maximum in scan order); dx equal to the fp32 sum of
    its (at most four) dy terms in the kernel's window order, and to float64 autograd within the rounding of three fp32 additions
    of the terms' absolute sum"""
    c = _pool_case(nimg, H, W, C, zero_img)
    t = c["tied"]
    assert _tie_rule_is_tested(t, H, W)                                  # before the GPU is used
    d = dev()
    y, codes = ops.maxpool3x3s2_idx(c["x"].to(d))
    assert torch.equal(y.cpu(), c["y"])
    wrong = int((codes.cpu() != c["codes"]).sum())
    assert wrong == 0, f"{wrong} of {codes.numel()} codes differ from ATen's first-maximum rule"
    dx = ops.maxpool3x3s2_bwd(codes, c["dy"].to(d), H, W)
    assert torch.equal(dx.cpu(), c["dx32"]), float((dx.cpu() - c["dx32"]).abs().max())
    err = (dx.cpu().double() - c["dx64"]).abs()
    room = 3 * 2.0 ** -24 * c["dxabs"]
    print(f"1. maxpool {nimg}x{H}x{W}x{C}{' zero image' if zero_img else ''}: {float(t.float().mean()):.2f} of the windows tied, "
          f"dx exact in fp32, worst |dx - float64| {float(err.max()):.2e} (room {float(room.max()):.2e})")
    assert bool((err <= room).all())
    y2, codes2 = ops.maxpool3x3s2_idx(c["x"].to(d))
    assert torch.equal(y, y2) and torch.equal(codes, codes2)
    assert torch.equal(dx, ops.maxpool3x3s2_bwd(codes, c["dy"].to(d), H, W))


@pytest.mark.parametrize("ipg", [2, 1])
@pytest.mark.parametrize("nimg,H,W,C", [(4, 23, 31, 64), (2, 8, 10, 64)])
def test_maxpool_backward_fused_relu_bn(nimg, H, W, C, ipg):
    """the fused form: dx = where(relu_x > 0, pooled gradient, 0) * scale[img // imgs_per_group][c], one fp32 product per element;
    the amax word = the bits of the largest magnitude written.  The scale table has one row per IMAGE (the kernel reads the first
    nimg / ipg of them), so a group index that forgets the division stays inside the table and reads the wrong row."""
    c = _pool_case(nimg, H, W, C, False)
    g = torch.Generator().manual_seed(77 + ipg)
    rx = torch.round(2 * torch.randn(nimg, H, W, C, generator=g)) / 2              # zeros, negatives and positives
    assert bool((rx == 0).any() and (rx < 0).any() and (rx > 0).any())
    scale = torch.rand(nimg, C, generator=g) + 0.5
    grp = torch.arange(nimg) // ipg
    exp = torch.where(rx > 0, c["dx32"], torch.zeros(())) * scale[grp].view(nimg, 1, 1, C)
    exp64 = torch.where(rx > 0, c["dx64"], torch.zeros((), dtype=torch.float64)) * scale[grp].double().view(nimg, 1, 1, C)
    d = dev()
    amax = word()
    dx = ops.maxpool3x3s2_bwd(c["codes"].to(d), c["dy"].to(d), H, W, relu_x=rx.to(d), bn_scale=scale.to(d), imgs_per_group=ipg,
                              amax_out=amax)
    e = rel_err(dx, exp64)
    print(f"1. fused pool backward {nimg}x{H}x{W}x{C} imgs_per_group {ipg}: rel.err to float64 {e:.2e}, exact in fp32: "
          f"{torch.equal(dx.cpu(), exp)}")
    assert torch.equal(dx.cpu(), exp)
    room = 4 * 2.0 ** -24 * c["dxabs"] * scale[grp].double().view(nimg, 1, 1, C)          # three additions and one product
    assert bool(((dx.cpu().double() - exp64).abs() <= room).all())
    assert int(amax) == bits(dx) == bits(exp)
    with pytest.raises(RuntimeError, match="relu_x and bn_scale come together"):
        ops.maxpool3x3s2_bwd(c["codes"].to(d), c["dy"].to(d), H, W, relu_x=rx.to(d))


def test_maxpool_entries_reject_bad_shapes():
    d = dev()
    with pytest.raises(RuntimeError):
        ops.maxpool3x3s2_idx(torch.zeros(1, 4, 4, 6, device=d))
    with pytest.raises(RuntimeError):
        ops.maxpool3x3s2_bwd(torch.zeros(1, 2, 2, 6, dtype=torch.uint8, device=d), torch.zeros(1, 2, 2, 6, device=d), 4, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. relu_bn_bwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 8])
@pytest.mark.parametrize("per_group", [64 * 4, 64 * 1234])
@pytest.mark.parametrize("G", [1, 3])
def test_relu_bn_bwd(G, per_group, C):
    """every operand combination at one shape: y_plain bit-equal to where(mask > 0, x + add, 0) in fp32, y_scaled bit-equal to
    y_plain * scale[g][i % C]; the amax word = bits of max |y_scaled|.  64 * 1234 floats per group is more than the grid holds in
    one pass (the grid-stride walk) and no multiple of the stride."""
    g = torch.Generator().manual_seed(G * 100000 + per_group + C)
    x, add = torch.randn(G, per_group, generator=g), torch.randn(G, per_group, generator=g)
    mask = torch.round(2 * torch.randn(G, per_group, generator=g)) / 2
    assert bool((mask == 0).any() and (mask < 0).any() and (mask > 0).any())
    scale = torch.rand(G, C, generator=g) + 0.5
    d = dev()
    xd, addd, maskd, scaled = x.to(d), add.to(d), mask.to(d), scale.to(d)
    sc_full = scale.view(G, 1, C).expand(G, per_group // C, C).reshape(G, per_group)
    n = 0
    for with_add in (False, True):
        for with_mask in (False, True):
            v = x + add if with_add else x.clone()
            if with_mask:
                v = torch.where(mask > 0, v, torch.zeros(()))
            vs = v * sc_full
            for plain, scaled_out in ((True, False), (False, True), (True, True)):
                amax, untouched = word(), word(0x12345678)
                yp, ys = ops.relu_bn_bwd(xd, C, add=addd if with_add else None, mask=maskd if with_mask else None, scale=scaled,
                                         want_plain=plain, want_scaled=scaled_out, amax_out=amax if scaled_out else None)
                what = f"G={G} per_group={per_group} C={C} add={with_add} mask={with_mask} plain={plain} scaled={scaled_out}"
                if plain:
                    assert torch.equal(yp.cpu(), v), what
                if scaled_out:
                    assert torch.equal(ys.cpu(), vs), what
                    assert int(amax) == bits(vs), what
                    ys2 = ops.relu_bn_bwd(xd, C, add=addd if with_add else None, mask=maskd if with_mask else None, scale=scaled,
                                          want_plain=False, want_scaled=True)[1]                  # no amax pointer
                    assert torch.equal(ys, ys2), what
                assert int(untouched) == 0x12345678, what
                n += 1
    print(f"2. relu_bn_bwd G={G} per_group={per_group} C={C}: {n} operand combinations exact in fp32 (worst error 0)")


def test_relu_bn_bwd_amax_is_a_running_maximum_and_rejects():
    d = dev()
    x = torch.full((1, 64), 0.5, device=d)
    sc = torch.ones(1, 8, device=d)
    big = word(int(torch.tensor(3.0).view(torch.int32)))
    ops.relu_bn_bwd(x, 8, scale=sc, want_plain=False, amax_out=big)
    assert int(big) == int(torch.tensor(3.0).view(torch.int32))          # an earlier, larger maximum stays
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.relu_bn_bwd(torch.zeros(1, 24, device=d), 6, scale=torch.ones(1, 6, device=d))            # C % 4
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.relu_bn_bwd(torch.zeros(1, 10, device=d), 4, scale=torch.ones(1, 4, device=d))            # per_group % 4
    with pytest.raises(RuntimeError, match="needs scale"):
        ops.relu_bn_bwd(x, 8)
    with pytest.raises(RuntimeError, match="amax_out"):
        ops.relu_bn_bwd(x, 8, want_scaled=False, amax_out=word())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. losses and their gradients
# ---------------------------------------------------------------------------------------------------------------------------
KLW = 10.0
# (B, Q, A, L, everything padded).  40 * 100 * 16 = 64000 elements are 250 blocks and B * L = 1280 is five blocks of the reparam
# kernels; the cap of l1_loss_kernel is 512 blocks * 256 threads = 131072 elements, so 90 * 100 * 16 = 144000 is the case that runs
# its grid stride
LOSS_CASES = [(1, 1, 4, 8, False), (3, 10, 14, 32, False), (8, 100, 16, 32, False), (40, 100, 16, 32, False),
              (3, 10, 14, 32, True), (90, 100, 16, 32, False)]
# Measured once on the CPU, on exactly the data of _loss_case over LOSS_CASES: torch's float32 evaluation of z = mu + exp(lv / 2) *
# eps and of autograd through sum(z * dz) + klw * kl against the float64 evaluation, worst elementwise |error| / max(1, |ref|):
# z 2.02e-07, d latent_info 2.97e-07.  The kernels' shared bound is four times the larger.
REPARAM_F32_TORCH_ERR = 2.97e-07
REPARAM_BOUND = 4 * REPARAM_F32_TORCH_ERR


@functools.lru_cache(maxsize=None)
def _loss_case(B, Q, A, L, all_pad):
    g = torch.Generator().manual_seed(B * 1000 + Q)
    a_hat, actions = torch.randn(B, Q, A, generator=g), torch.randn(B, Q, A, generator=g)
    a_hat.view(-1)[::7] = actions.view(-1)[::7]                         # exact zero differences
    is_pad = torch.zeros(B, Q, dtype=torch.bool)
    for b in range(B):
        is_pad[b, Q - (b * 3) % (Q // 2 + 1):] = (b * 3) % (Q // 2 + 1) > 0             # a padded tail of varying length
    if B >= 3:
        is_pad[B // 2] = True                                           # one sample padded from its first step
    if Q >= 10:
        is_pad[0, Q // 2] = True                                        # and a padded step in the middle of a sample
    if all_pad:
        is_pad[:] = True
    li = torch.cat([torch.randn(B, L, generator=g), 0.5 * torch.randn(B, L, generator=g)], dim=1)         # mu | logvar
    eps, dz = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    return dict(a_hat=a_hat, actions=actions, is_pad=is_pad, li=li, eps=eps, dz=dz)


def _loss_ref(c, dtype):
    """policy.py:310-320 and detr_vae.py's kl_divergence / reparametrize in `dtype`: l1, kl, loss, z, d latent_info"""
    a_hat, actions, li = c["a_hat"].to(dtype), c["actions"].to(dtype), c["li"].to(dtype).clone().requires_grad_(True)
    L = li.shape[1] // 2
    all_l1 = F.l1_loss(actions, a_hat, reduction="none")
    l1 = (all_l1 * ~c["is_pad"].unsqueeze(-1)).mean()
    mu, lv = li[:, :L], li[:, L:]
    klds = -0.5 * (1 + lv - mu.pow(2) - lv.exp())
    kl = klds.sum(1).mean(0)
    z = mu + (lv / 2).exp() * c["eps"].to(dtype)
    ((z * c["dz"].to(dtype)).sum() + KLW * kl).backward()
    return l1.detach(), kl.detach(), (l1 + KLW * kl).detach(), z.detach(), li.grad


def _elem_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())


@pytest.mark.parametrize("B,Q,A,L,all_pad", LOSS_CASES)
def test_act_losses(B, Q, A, L, all_pad):
    """l1 (mean over ALL elements, padded ones included as zeros), kl and loss against float64 at the project's bound for these
    scalars, 1e-4 of max(1, |ref|); the actual error (about 1e-7) is printed.  Sums in a fixed order: bitwise repeatable."""
    c = _loss_case(B, Q, A, L, all_pad)
    l1, kl, loss, _, _ = _loss_ref(c, torch.float64)
    d = dev()
    args = (c["a_hat"].to(d), c["actions"].to(d), c["is_pad"].to(torch.uint8).to(d))
    got = ops.act_losses(*args, latent_info=c["li"].to(d), kl_weight=KLW, L_=L).cpu().double()
    errs = [abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(got, (l1, kl, loss))]
    print(f"3. losses B={B} Q={Q} A={A} L={L}{' all padded' if all_pad else ''}: l1 {float(got[0]):.6f} kl {float(got[1]):.6f} "
          f"loss {float(got[2]):.6f}, errors {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} (bound 1e-4)")
    assert max(errs) < 1e-4
    if all_pad:
        assert float(got[0]) == 0.0
    again = ops.act_losses(*args, latent_info=c["li"].to(d), kl_weight=KLW, L_=L).cpu().double()
    assert torch.equal(got, again)
    nokl = ops.act_losses(*args).cpu().double()                          # no CVAE encoder: kl = 0, loss = l1
    assert float(nokl[0]) == float(got[0]) and float(nokl[1]) == 0.0 and float(nokl[2]) == float(got[0])
    with pytest.raises(RuntimeError, match="512 floats of block partials"):
        ops.act_losses(*args, buf=torch.empty(3 + 1 + 511, device=d))


@pytest.mark.parametrize("gscale", [1.0, 2.0 ** 10])
@pytest.mark.parametrize("B,Q,A,L,all_pad", LOSS_CASES)
def test_l1_bwd(B, Q, A, L, all_pad, gscale):
    """bit-equal to sign(a_hat - actions) * !is_pad * gscale / (B*Q*A) in fp32 (one exact product, one correctly rounded quotient):
    exactly 0 at the equal elements and at the padded ones; float64 autograd of the masked mean agrees to fp32 rounding"""
    c = _loss_case(B, Q, A, L, all_pad)
    total = B * Q * A
    sgn = torch.sign(c["a_hat"] - c["actions"]) * (~c["is_pad"]).unsqueeze(-1).float()
    exp = torch.from_numpy((sgn.numpy() * np.float32(gscale)) / np.float32(total))
    d = dev()
    got = ops.l1_bwd(c["a_hat"].to(d), c["actions"].to(d), c["is_pad"].to(torch.uint8).to(d), gscale).cpu()
    a64 = c["a_hat"].double().requires_grad_(True)
    (F.l1_loss(c["actions"].double(), a64, reduction="none") * ~c["is_pad"].unsqueeze(-1)).mean().backward()
    e = float((got.double() - a64.grad * gscale).abs().max()) / (gscale / total)
    print(f"3. l1_bwd B={B} Q={Q} A={A} gscale={gscale}: exact in fp32: {torch.equal(got, exp)}, to float64 autograd {e:.2e} of gscale/total")
    assert torch.equal(got, exp)
    assert e <= 2.0 ** -24
    assert bool((got.view(-1)[::7] == 0).all()) and bool((got[c["is_pad"]] == 0).all())


@pytest.mark.parametrize("B,Q,A,L,all_pad", [c for c in LOSS_CASES if not c[4]])
def test_reparam_and_its_backward(B, Q, A, L, all_pad):
    """z = mu + exp(logvar / 2) * eps against float64, and reparam_kl_bwd against float64 autograd of sum(z * dz) + klw * kl, under
    one bound: four times the worst elementwise error (|error| / max(1, |ref|)) that torch's own float32 CPU evaluation of the same
    formulas shows against float64 on this data -- measured once: 2.97e-07 (z 2.02e-07, d latent_info 2.97e-07), so the bound is
    1.19e-06."""
    c = _loss_case(B, Q, A, L, all_pad)
    _, _, _, z, dli = _loss_ref(c, torch.float64)
    d = dev()
    li, eps, dz = c["li"].to(d), c["eps"].to(d), c["dz"].to(d)
    gz, mu, lv = ops.reparam(li, eps, want_stats=True)
    assert torch.equal(mu.cpu(), c["li"][:, :L]) and torch.equal(lv.cpu(), c["li"][:, L:])
    gd = ops.reparam_kl_bwd(li, eps, dz, KLW)
    ez, ed = _elem_err(gz, z), _elem_err(gd, dli)
    print(f"3. reparam B={B} L={L}: z {ez:.2e}, d latent_info {ed:.2e} (bound {REPARAM_BOUND:.2e})")
    assert ez < REPARAM_BOUND and ed < REPARAM_BOUND
    assert torch.equal(gz, ops.reparam(li, eps)) and torch.equal(gd, ops.reparam_kl_bwd(li, eps, dz, KLW))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. vq_bwd and dropout_bwd
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,VC,VD", [(1, 1, 2), (3, 32, 32), (300, 8, 16)])
def test_vq_bwd(B, VC, VD):
    """softmax backward per (sample, class) against float64 autograd of sum(softmax(logits) * g), at the bound the prior-training
    test uses for its softmax gradient: 5e-6 of the tensor maximum"""
    g = torch.Generator().manual_seed(B + VC + VD)
    logits = (2 * torch.randn(B, VC, VD, generator=g, dtype=torch.float64)).requires_grad_(True)
    gr = torch.randn(B, VC, VD, generator=g)
    probs = torch.softmax(logits, -1)
    (probs * gr.double()).sum().backward()
    d = dev()
    pd, gd = probs.detach().float().to(d), gr.to(d)
    got = ops.vq_bwd(pd, gd)
    e = rel_err(got, logits.grad)
    print(f"4. vq_bwd B={B} VC={VC} VD={VD}: rel.err {e:.2e} (bound 5.0e-06)")
    assert e < 5e-6
    assert torch.equal(got, ops.vq_bwd(pd, gd))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_bwd(p):
    """bit-equal to keep * dy / (1 - p) in fp32 under the host mask -- as the kernel forms it, dy times the fp32 reciprocal of
    (1 - p); against the float64 quotient that is within two fp32 roundings"""
    n, seed = 70001, BIG_SEED + 5
    g = torch.Generator().manual_seed(9)
    dy = torch.randn(n, generator=g)
    keep = host_keep(seed, np.arange(n, dtype=np.uint64), p)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    exp = torch.from_numpy(np.where(keep, dy.numpy() * inv, np.float32(0.0)).astype(np.float32))
    got = ops.dropout_bwd(dy.to(dev()), p, seed).cpu()
    exp64 = torch.from_numpy(keep).double() * dy.double() / (1.0 - float(np.float32(p)))
    e = float(((got.double() - exp64).abs() / exp64.abs().clamp(min=1e-30)).max())
    print(f"4. dropout_bwd p={p}: exact in fp32: {torch.equal(got, exp)}, worst relative error to float64 {e:.2e}")
    assert torch.equal(got, exp)
    assert e <= 2 * 2.0 ** -24
    assert torch.equal(got, ops.dropout(dy.to(dev()), p, seed).cpu())              # the forward's mask and factor


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the engine's AdamW
# ---------------------------------------------------------------------------------------------------------------------------
ADAM = dict(lr=1e-3, lr_bb=3e-4, wd=1e-4, eps=1e-8)
# the C ABI takes the betas as float: the operation under test IS AdamW with these two values, and so is its float64 reference
BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))
# Measured once on the CPU on exactly the data of _adam_case(64 * 37): torch.optim.AdamW in float32 against float64, the update
# p_after - p_before of each of the five steps, per parameter group, as max |error| / max |update|: worst 5.80e-07.
ADAMW_F32_TORCH_ERR = 5.80e-07
ADAMW_UPDATE_BOUND = 4 * ADAMW_F32_TORCH_ERR


@functools.lru_cache(maxsize=None)
def _adam_case(n):
    g = torch.Generator().manual_seed(n)
    nslot = (n + 63) // 64
    group = (torch.arange(nslot) % 3).to(torch.uint8)                    # 0 / 1 / 2 per 64-float slot
    gel = group.repeat_interleave(64)[:n]
    p0 = torch.randn(n, generator=g) * 1e-4           # small weights: the fp32 rounding of p itself stays below the update's error
    grads = [torch.randn(n, generator=g) * 10.0 ** (1.25 * s - 3.0) for s in range(5)]            # 1e-3 .. 1e2
    return dict(group=group, gel=gel, p0=p0, grads=grads, m0=torch.randn(n, generator=g), v0=torch.rand(n, generator=g))


def _adam_torch(c, dtype):
    """five steps of torch.optim.AdamW in `dtype` with the two parameter groups: per step (p, m, v) of the elements of group 1 | 2"""
    idx = [torch.nonzero(c["gel"] == k).view(-1) for k in (1, 2)]
    ps = [c["p0"][i].to(dtype).clone().requires_grad_(True) for i in idx]
    opt = torch.optim.AdamW([dict(params=[ps[0]], lr=ADAM["lr"]), dict(params=[ps[1]], lr=ADAM["lr_bb"])], betas=BETAS,
                            eps=ADAM["eps"], weight_decay=ADAM["wd"])
    out = []
    for gr in c["grads"]:
        for pt, i in zip(ps, idx):
            pt.grad = gr[i].to(dtype)
        opt.step()
        out.append([(pt.detach().clone(), opt.state[pt]["exp_avg"].clone(), opt.state[pt]["exp_avg_sq"].clone()) for pt in ps])
    return idx, out


def _update_err(p_after, p_before, ref_after, ref_before):
    """max |update - reference update| / max |reference update|, in float64"""
    up, ur = p_after.double() - p_before.double(), ref_after.double() - ref_before.double()
    return float((up - ur).abs().max() / ur.abs().max())


@pytest.mark.parametrize("n", [64 * 37, 64 * 37 + 17])
def test_adamw_groups(n):
    """five steps of the engine's AdamW against float64 torch.optim.AdamW with two parameter groups (betas = the float values the
    C ABI carries).  Group-0 slots keep p, m, v bit for bit; m and v within 2e-6; the UPDATE p_after - p_before of every step within
    four times the error torch's own float32 CPU AdamW shows against float64 on this data (measured once: 5.80e-07 of the largest
    update, so the bound is 2.32e-06).  A partial last slot (n = 64 * 37 + 17) is allowed by the launcher: its group byte covers
    the 17 elements."""
    c = _adam_case(n)
    idx, ref = _adam_torch(c, torch.float64)
    d = dev()
    frozen = c["gel"] == 0
    m0 = torch.where(frozen, c["m0"], torch.zeros(()))                   # the untouched slots hold values that a write would change
    v0 = torch.where(frozen, c["v0"], torch.zeros(()))
    p, m, v, group = c["p0"].to(d), m0.to(d), v0.to(d), c["group"].to(d)
    worst_u = worst_m = worst_v = 0.0
    for step, gr in enumerate(c["grads"], 1):
        before = p.cpu()
        ops.adamw_groups(p, gr.to(d), m, v, group, ADAM["lr"], ADAM["lr_bb"], ADAM["wd"], step, betas=BETAS, eps=ADAM["eps"])
        after = p.cpu()
        for k in (0, 1):
            rp, rm, rv = ref[step - 1][k]
            rbefore = ref[step - 2][k][0] if step > 1 else c["p0"][idx[k]].double()
            eu = _update_err(after[idx[k]], before[idx[k]], rp, rbefore)
            em, ev = rel_err(m.cpu()[idx[k]], rm), rel_err(v.cpu()[idx[k]], rv)
            print(f"5. adamw n={n} step {step} group {k + 1}: update {eu:.2e} (bound {ADAMW_UPDATE_BOUND:.2e}), m {em:.2e}, v {ev:.2e}")
            worst_u, worst_m, worst_v = max(worst_u, eu), max(worst_m, em), max(worst_v, ev)
        assert torch.equal(after[frozen], c["p0"][frozen]) and torch.equal(m.cpu()[frozen], c["m0"][frozen])
        assert torch.equal(v.cpu()[frozen], c["v0"][frozen])
    print(f"5. adamw n={n}: worst update error {worst_u:.2e}, m {worst_m:.2e}, v {worst_v:.2e}")
    assert worst_m < 2e-6 and worst_v < 2e-6
    assert worst_u < ADAMW_UPDATE_BOUND


def test_adamw_groups_skip_flag():
    """with a masked bit of the flag word up nothing changes at all; with only an unmasked bit up the step is the plain step"""
    c = _adam_case(64 * 37)
    d = dev()
    gr, group = c["grads"][2].to(d), c["group"].to(d)

    def run(flag, mask):
        p, m, v = c["p0"].to(d), c["m0"].to(d), c["v0"].to(d)
        fw = word(flag) if flag is not None else None
        ops.adamw_groups(p, gr, m, v, group, ADAM["lr"], ADAM["lr_bb"], ADAM["wd"], 3, betas=BETAS, eps=ADAM["eps"], flags=fw,
                         skip_mask=mask)
        return p.cpu(), m.cpu(), v.cpu()
    plain = run(None, 0)
    assert not torch.equal(plain[0], c["p0"])
    skipped = run(4, 6)                                                  # ACTMI_FLAG_LOSS up, LOSS | WEIGHT masked
    assert all(torch.equal(a, b) for a, b in zip(skipped, (c["p0"], c["m0"], c["v0"])))
    for flag, mask in ((1, 6), (0, 6), (4, 0)):                          # an unmasked bit, no bit, no mask
        assert all(torch.equal(a, b) for a, b in zip(run(flag, mask), plain)), (flag, mask)
    with pytest.raises(RuntimeError, match="step counts from 1"):
        p = c["p0"].to(d)
        ops.adamw_groups(p, gr, p.clone(), p.clone(), group, 1e-3, 1e-3, 0.0, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. attention with weight dropout under the exact mask
# ---------------------------------------------------------------------------------------------------------------------------
def _attn_drop_ref(q, k, v, H, kpm, p, seed, dout=None):
    """float64: out = (softmax(s) * keep / (1 - p)) @ v, the normaliser over the un-dropped weights, keep indexed
    ((b*H + h)*Nq + q)*Nk + key; with dout also dq, dk, dv by autograd"""
    B, Nq, D = q.shape
    Nk, hd = k.shape[1], D // H
    qd, kd, vd = (t.double().requires_grad_(dout is not None) for t in (q, k, v))
    qq, kk, vv = (t.reshape(B, -1, H, hd).transpose(1, 2) for t in (qd, kd, vd))
    s = qq @ kk.transpose(-1, -2) / hd ** 0.5
    if kpm is not None:
        s = s.masked_fill(kpm.view(B, 1, 1, Nk), float("-inf"))
    keep = mask_t(seed, (B, H, Nq, Nk), p).double()
    out = ((torch.softmax(s, -1) * keep / (1.0 - p)) @ vv).transpose(1, 2).reshape(B, Nq, D)
    if dout is None:
        return out.detach()
    out.backward(dout.double())
    return out.detach(), qd.grad, kd.grad, vd.grad


def _qkv(B, H, Nq, Nk, hd, masked, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    q = torch.randn(B, Nq, D, generator=g)
    kv = torch.randn(B, Nk, 2 * D, generator=g)                          # interleaved K | V rows: the row strides take part
    kpm = None
    if masked:
        kpm = torch.zeros(B, Nk, dtype=torch.bool)
        for b in range(B):
            kpm[b, Nk - 37 - 3 * b:] = True
        kpm[0, 5] = True
    return q, kv, kpm


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,H,Nq,Nk,hd,masked", [(2, 4, 130, 200, 16, False), (1, 2, 33, 65, 32, True), (2, 8, 140, 300, 64, False)])
def test_attention_forward_with_dropout_exact(B, H, Nq, Nk, hd, masked, prec, p):
    """ops.attention with the weight dropout on against float64 under the host mask, at the bound of the no-dropout path (3e-6 of
    the output maximum); the split-KV and the one-pass kernels agree within the same bound"""
    q, kv, kpm = _qkv(B, H, Nq, Nk, hd, masked, Nq + Nk)
    D = H * hd
    seed = BIG_SEED + Nq
    exp = _attn_drop_ref(q, kv[..., :D], kv[..., D:], H, kpm, p, seed)
    d = dev()
    qd, kvd = q.to(d), kv.to(d)
    kd = kpm.to(torch.uint8).to(d) if masked else None
    outs = {}
    for split in ((True, False) if Nk == 300 else (True,)):
        outs[split] = ops.attention(qd, kvd[..., :D], kvd[..., D:], H, kpm=kd, split=split, drop_p=p, drop_seed=seed, prec=prec)
        e = rel_err(outs[split], exp)
        print(f"6. attention fwd dropout {B}x{H}x{Nq}x{Nk}x{hd} {prec} p={p} split={split}: rel.err {e:.2e} (bound 3.0e-06)")
        assert e < 3e-6
        again = ops.attention(qd, kvd[..., :D], kvd[..., D:], H, kpm=kd, split=split, drop_p=p, drop_seed=seed, prec=prec)
        assert torch.equal(outs[split], again)
    if len(outs) == 2:
        e = rel_err(outs[True], outs[False])
        print(f"6. attention fwd dropout split against one pass: {e:.2e}")
        assert e < 3e-6


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,Nq,Nk,hd,masked", [(1, 4, 260, 260, 64, False), (1, 2, 130, 257, 32, True)])
def test_attention_fused_backward_with_dropout_exact(B, H, Nq, Nk, hd, masked, p):
    """ops.attention_bwd with the weight dropout on: dq, dk, dv against float64 autograd under the host mask, at the bound of the
    no-dropout path (2e-5 of each tensor's maximum); two runs bit-identical"""
    q, kv, kpm = _qkv(B, H, Nq, Nk, hd, masked, 7 * Nq + Nk)
    D = H * hd
    seed = BIG_SEED + Nk
    g = torch.Generator().manual_seed(Nk)
    dout = torch.randn(B, Nq, D, generator=g)
    exp, dq, dk, dv = _attn_drop_ref(q, kv[..., :D], kv[..., D:], H, kpm, p, seed, dout)
    d = dev()
    qd, kvd, dod = q.to(d), kv.to(d), dout.to(d)
    kd = kpm.to(torch.uint8).to(d) if masked else None
    o, lse = ops.attention(qd, kvd[..., :D], kvd[..., D:], H, kpm=kd, want_lse=True, drop_p=p, drop_seed=seed, prec="f16x3")
    assert rel_err(o, exp) < 3e-6
    got = ops.attention_bwd(qd, kvd[..., :D], kvd[..., D:], o, lse, dod, H, kpm=kd, drop_p=p, drop_seed=seed)
    for name, a, b in zip(("dq", "dk", "dv"), got, (dq, dk, dv)):
        e = rel_err(a, b)
        print(f"6. attention fused bwd dropout {B}x{H}x{Nq}x{Nk}x{hd} p={p} {name}: rel.err {e:.2e} (bound 2.0e-05)")
        assert e < 2e-5, name
    again = ops.attention_bwd(qd, kvd[..., :D], kvd[..., D:], o, lse, dod, H, kpm=kd, drop_p=p, drop_seed=seed)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("NK", GB.NKS)
def test_attention_materialised_chain_with_dropout(NK, prec, p):
    """the chain of train.hip: attn_bwd with drop_p > 0, on the operands and descriptors of test_attention_backward_chain: P
    (epi 1), zero_cols, attn_delta, attn_drop into the dP buffer, dV = Pd^T dO, dP = dO V^T, attn_ds_drop in place, dQ, dK.  delta,
    Pd and dS against float64 under the host mask (elementwise: the project's 3e-6), dq / dk / dv against float64 autograd at that
    test's 2e-5; the pad columns Nk .. ldp-1 of both buffers, pre-filled with a sentinel, are exactly zero afterwards."""
    _chain_with_dropout(GB._attn_case(NK), NK, prec, p)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("NK", GB.NKS)
def test_attention_materialised_chain_with_dropout_at_a_sink(NK, prec, p):
    """the same chain with an attention sink in the scores (margin 10: key 0 holds all but e^-10 * Nk of every row's mass and has
    a zero value vector), same per-stage bounds"""
    _chain_with_dropout(GB._attn_case(NK, margin=10), NK, prec, p, what="chain with dropout at a sink")


def _chain_with_dropout(c, NK, prec, p, what="chain with dropout"):
    AB, AH, HD, NQ, AD = GB.AB, GB.AH, GB.HD, GB.NQ, GB.AD
    d = dev()
    tile = 3
    seed = BIG_SEED + NK
    ldp = GB.up4(NK)
    assert ldp != NK
    pg = NQ * ldp
    q, kv, dO = c["q"].to(d), c["kv"].to(d), c["dO"].to(d)
    O64, dq, dk, dv = _attn_drop_ref(c["q"], c["kv"][..., :AD], c["kv"][..., AD:], AH, c["kpm"], p, seed, c["dO"])
    keep = mask_t(seed, (AB, AH, NQ, NK), p).double()
    P = torch.full((AB, AH, NQ, ldp), SENTINEL, device=d)
    dP = torch.full((AB, AH, NQ, ldp), SENTINEL, device=d)
    common = dict(groups=AB * AH, groups_inner=AH, prec=GB.PREC[prec], tile_hint=tile)
    GB._launch_p(c, prec, tile, q, kv, P)
    assert bool((P[..., NK:] == SENTINEL).all())
    ops.zero_cols(P, NK)
    assert not bool(P[..., NK:].any())
    Pc = P[..., :NK].cpu().double()
    O = O64.float().to(d)                                                # the forward's saved output
    delta = ops.attn_delta(dO, O, AH)
    delta_ref = (GB.heads(c["dO"].double(), NQ) * GB.heads(O64.float().double(), NQ)).sum(-1)
    e_delta = rel_err(delta, delta_ref)
    ops.attn_drop(P, dP, NK, p, seed)
    assert not bool(dP[..., NK:].any()), "attn_drop leaves the pad columns of the Pd buffer zero"
    inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    e_pd = rel_err(dP[..., :NK], Pc * keep * inv)
    assert bool((dP[..., :NK].cpu()[keep == 0] == 0).all())
    dO_sc = ops.pow2_scale(dO.view(-1, AD))
    gq = torch.zeros(AB, NQ, 3 * AD, device=d)
    gkv = torch.zeros(AB, NK, 3 * AD, device=d)
    run_gemm("dV", A=dP, lda=ldp, ta=1, M=NK, K=NQ, Bw=dO, ldb=AD, tb=1, N=HD, C=gkv[..., 2 * AD:], ldc=3 * AD, gA=pg * AH, gA2=pg,
             gB=NQ * AD, gB2=HD, gC=NK * 3 * AD, gC2=HD, a_scale=256.0, b_scale_dev=dO_sc, **common)
    dP[..., NK:] = SENTINEL
    run_gemm("dP", A=dO, lda=AD, M=NQ, K=HD, Bw=kv[..., AD:], ldb=2 * AD, N=NK, C=dP, ldc=ldp, gA=NQ * AD, gA2=HD, gB=NK * 2 * AD,
             gB2=HD, gC=pg * AH, gC2=pg, a_scale_dev=dO_sc, **common)
    dPc = dP[..., :NK].cpu().double()
    ops.attn_ds_drop(P, dP, delta, c["scale"], NK, p, seed)
    assert not bool(dP[..., NK:].any()), "attn_ds_drop zeroes the pad columns of the dS buffer"
    e_ds = rel_err(dP[..., :NK], Pc * (dPc * keep * inv - delta.cpu().double().unsqueeze(-1)) * c["scale"])
    dS_sc = ops.pow2_scale(dP.view(-1, ldp)[:, :NK])
    run_gemm("dQ", A=dP, lda=ldp, M=NQ, K=NK, Bw=kv, ldb=2 * AD, tb=1, N=HD, C=gq, ldc=3 * AD, gA=pg * AH, gA2=pg,
             gB=NK * 2 * AD, gB2=HD, gC=NQ * 3 * AD, gC2=HD, a_scale_dev=dS_sc, **common)
    run_gemm("dK", A=dP, lda=ldp, ta=1, M=NK, K=NQ, Bw=q, ldb=AD, tb=1, N=HD, C=gkv[..., AD:], ldc=3 * AD, gA=pg * AH, gA2=pg,
             gB=NQ * AD, gB2=HD, gC=NK * 3 * AD, gC2=HD, a_scale_dev=dS_sc, **common)
    print(f"6. {what} Nk={NK} {prec} p={p}: delta {e_delta:.2e}, Pd {e_pd:.2e}, dS {e_ds:.2e} (bound 3.0e-06)")
    assert e_delta < 3e-6 and e_pd < 3e-6 and e_ds < 3e-6
    for name, got, exp in (("dQ", gq[..., :AD], dq), ("dK", gkv[..., AD:2 * AD], dk), ("dV", gkv[..., 2 * AD:], dv)):
        e = rel_err(got, exp)
        print(f"6. {what} Nk={NK} {prec} p={p} {name} against float64 autograd: {e:.2e} (bound 2.0e-05)")
        assert e < 2e-5, name


def test_attention_piece_entries_reject_bad_arguments():
    d = dev()
    P = torch.zeros(1, 4, 8, device=d)
    with pytest.raises(RuntimeError, match="ldp < Nk"):
        ops.attn_drop(P, P.clone(), 9, 0.1, 1)
    with pytest.raises(RuntimeError, match="ldp < Nk"):
        ops.attn_ds_drop(P, P.clone(), torch.zeros(4, device=d), 1.0, 8, 1.0, 1)               # p = 1
    with pytest.raises(RuntimeError, match="c0 <= ld"):
        ops.zero_cols(P, 9)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. LayerNorm backward at every template width
# ---------------------------------------------------------------------------------------------------------------------------
LN_CASES = [(1, 64), (3, 512), (300, 768), (300, 1024), (37, 1280), (300, 2048), (4200, 512)]


@functools.lru_cache(maxsize=None)
def _ln_case(M, D):
    g = torch.Generator().manual_seed(M + D)
    x = (torch.randn(M, D, generator=g) * 2 + 0.5).double().requires_grad_(True)
    w = (torch.rand(D, generator=g) + 0.5).double().requires_grad_(True)
    b = torch.randn(D, generator=g).double().requires_grad_(True)
    dy, add = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    F.layer_norm(x, (D,), w, b).backward(dy.double())
    return dict(x=x.detach().float(), w=w.detach().float(), dy=dy, add=add, dx=x.grad, dw=w.grad, db=b.grad,
                dw0=torch.randn(D, generator=g), db0=torch.randn(D, generator=g))


@pytest.mark.parametrize("small_ws", [False, True])
@pytest.mark.parametrize("M,D", LN_CASES)
def test_layernorm_backward_widths(M, D, small_ws):
    """ln_bwd_kernel<1, 2, 3, 4, 8> (D = 64 .. 2048; D = 1280 runs the 8-wide form with dead iterations), M < 4 and M above the
    1024-block cap, with the workspace (ordered sums: bitwise repeatable) and with one too small (the atomic path: float64
    comparison only), dx_add on and off, dw / db accumulated onto non-zero values, the dx_amax word.  dx at the project's 3e-6, dw
    and db at 3e-6 * max(1, sqrt(M / 300))."""
    c = _ln_case(M, D)
    d = dev()
    x, w, dy, add = c["x"].to(d), c["w"].to(d), c["dy"].to(d), c["add"].to(d)
    blocks = min(1024, (M + 3) // 4)
    need = blocks * 2 * D
    ws = torch.empty(need - 1 if small_ws else need, device=d)
    tol_p = 3e-6 * max(1.0, (M / 300) ** 0.5)
    for with_add in (False, True):
        dw, db, amax = c["dw0"].to(d), c["db0"].to(d), word()
        dx = ops.layernorm_bwd_ex(x, w, dy, dw, db, ws=ws, dx_add=add if with_add else None, dx_amax=amax)
        exp_dx = c["dx"] + c["add"].double() if with_add else c["dx"]
        ex, ew, eb = rel_err(dx, exp_dx), rel_err(dw, c["dw"] + c["dw0"].double()), rel_err(db, c["db"] + c["db0"].double())
        print(f"7. ln_bwd M={M} D={D} {'atomic' if small_ws else 'ordered'} dx_add={with_add}: dx {ex:.2e} (bound 3.0e-06), "
              f"dw {ew:.2e} db {eb:.2e} (bound {tol_p:.1e})")
        assert ex < 3e-6 and ew < tol_p and eb < tol_p
        assert int(amax) == bits(dx)
        dw2, db2 = c["dw0"].to(d), c["db0"].to(d)
        dx2 = ops.layernorm_bwd_ex(x, w, dy, dw2, db2, ws=ws, dx_add=add if with_add else None)              # no amax word
        assert torch.equal(dx, dx2)
        if not small_ws:
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
            dw3, db3 = c["dw0"].to(d), c["db0"].to(d)
            assert torch.equal(dx, ops.layernorm_bwd(x, w, dy, dw3, db3, ws, dx_add=add if with_add else None))
            assert torch.equal(dw, dw3) and torch.equal(db, db3)         # the entry without the amax word: the same launch


@pytest.mark.parametrize("D", [2052, 6])
def test_layernorm_backward_rejects(D):
    d = dev()
    x = torch.zeros(4, D, device=d)
    with pytest.raises(RuntimeError, match="multiple of 4 and <= 2048"):
        ops.layernorm_bwd_ex(x, torch.ones(D, device=d), x, torch.zeros(D, device=d), torch.zeros(D, device=d))


# ---------------------------------------------------------------------------------------------------------------------------
# 8. colsum paths
# ---------------------------------------------------------------------------------------------------------------------------
def _colsum_check(what, view, ref64, M, with_ws, repeatable):
    """out starts non-zero: every path of launch_colsum ACCUMULATES (out[n] += ...), as colsum_kernel and reduce_rows_kernel document"""
    d = view.device
    N = view.shape[1]
    g = torch.Generator().manual_seed(N)
    out0 = torch.randn(N, generator=g)
    ws = torch.empty(((M + 255) // 256) * N, device=d) if with_ws else None
    out = out0.to(d)
    ops.colsum(view, out, ws)
    tol = 3e-6 * max(1.0, (M / 300) ** 0.5)
    e = rel_err(out, ref64.cpu() + out0.double())
    print(f"8. colsum {what} M={M} N={N} ld={view.stride(0)} ws={with_ws}: rel.err {e:.2e} (bound {tol:.1e})")
    assert e < tol
    if repeatable:
        out2 = out0.to(d)
        ops.colsum(view, out2, ws)
        assert torch.equal(out, out2)


# (M, N, ld); N = 130 is no multiple of 4 (always the scalar kernel); N = 128 in ld = 132 takes the vectorised kernel when the
# pointer is 16-byte aligned and the scalar one when it is not
@pytest.mark.parametrize("with_ws", [True, False])
@pytest.mark.parametrize("M,N,ld", [(3, 5, 5), (300, 6, 7), (1000, 130, 132), (1000, 128, 132), (256, 64, 64), (257, 64, 64)])
def test_colsum_paths(M, N, ld, with_ws):
    """scalar and vectorised kernels, one row block and several, with the workspace (ordered: bitwise repeatable) and without
    (atomics over the row blocks: float64 only; one row block is ordered anyway); where ld > N also as a view 4 floats into the
    buffer (still 16-byte aligned) and 1 float into it (must fall back to the scalar kernel and still be right)"""
    g = torch.Generator().manual_seed(M * N)
    base = torch.randn(M * ld + 8, generator=g)
    bd = base.to(dev())
    single = M <= 256
    for off in ((0, 4, 1) if ld > N else (0,)):
        view = torch.as_strided(bd, (M, N), (ld, 1), off)
        ref = torch.as_strided(base, (M, N), (ld, 1), off).double().sum(0)
        _colsum_check(f"offset {off}", view, ref, M, with_ws, repeatable=with_ws or single)


def test_colsum_row_block_doubling():
    """N = 4096, M = 16500: 16 column blocks x 65 row blocks of 256 rows is above 1024 workgroups, so the row block doubles to
    512; built on the device, float64 reference by torch on the device"""
    d = dev()
    M, N = 16500, 4096
    assert (N // 4 + 63) // 64 * ((M + 255) // 256) > 1024
    g = torch.Generator(device=d).manual_seed(3)
    src = torch.randn(M, N, generator=g, device=d)
    ref = src.sum(0, dtype=torch.float64)
    for with_ws in (True, False):
        _colsum_check("row-block doubling", src, ref, M, with_ws, repeatable=with_ws)
