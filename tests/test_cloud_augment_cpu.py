"""No-GPU checks of the device-side point-cloud augmentation: the numpy definition (actmi.ops.cloud_augment_ref, the oracle of
actmi_op_cloud_augment) against its own properties and against the same transform written independently in float64, the draws of
actmi.ops.CloudAugment, the CLI and forward_pass's routing.

Bounds.  The identity at pivot 0 is exact ((p - 0) * 1 + 0 + 0 + 0: no operation rounds).  At a non-zero pivot (p - c) + c rounds
twice, each time to within half an ulp of a value no larger than max(|p|, |c|) in magnitude: 1 ulp of that.  The general
transform takes, per coordinate, 6 roundings one after the other that the float64 statement does not take -- the difference, a
product, the rotation's sum, the scale, and the sums with the pivot and the shift -- before the jitter is added, on values bounded
by M = |p| + |pivot| + |t| + jitter (|cos|, |sin| <= 1); the record's own fp32 fields are given to the float64 statement as they
are.  Each rounding is within half an ulp of M, so 6 make 3 ulp; the bound is 8 ulp of M, which leaves room for the rotation's
second product, the jitter's product and sum, and a scale of up to 1.05."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from actmi import lib as L
from actmi import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "actmi.h")
f32 = np.float32


def _clouds(B, P, seed, lo=-0.8, hi=0.8):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (B, P, 3)).astype(f32), rng.uniform(0, 255, (B, P, 3)).astype(f32)


def _random_records(B, seed, drop=0.3, jitter=0.002):
    rng = np.random.default_rng(seed)
    return ops.cloud_augment_records(B, angle=rng.uniform(-5, 5, B), scale=rng.uniform(0.95, 1.05, B), shift=rng.uniform(-0.01, 0.01, (B, 3)),
                                     jitter=jitter, drop=drop, order=np.arange(B) % 6, fb=rng.uniform(0.7, 1.3, B),
                                     fc=rng.uniform(0.6, 1.4, B), fs=rng.uniform(0.5, 1.5, B),
                                     seed=rng.integers(0, 1 << 64, size=B, dtype=np.uint64))


def _ulp(x):
    return np.spacing(np.abs(x).astype(f32)).astype(np.float64)


def test_record_layout_matches_the_header_struct():
    dt = ops.cloud_augment_record_dtype()
    assert dt.itemsize == 56 == C.sizeof(L.CloudAugmentRecord)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(L.CloudAugmentRecord, n).offset) for n, _ in L.CloudAugmentRecord._fields_]
    assert C.sizeof(L.CloudAugmentDesc) == 80 and L.CloudAugmentDesc.pivot.offset == 56 and L.CloudAugmentDesc.B.offset == 68
    assert "actmi_op_cloud_augment" in L.declared_symbols(HEADER)
    lib = L.load()
    assert lib.actmi_op_cloud_augment(None, None) != 0 and b"null descriptor" in lib.actmi_op_last_error()
    assert lib.actmi_version() == 110
    r = ops.cloud_augment_records(3, angle=90.0, seed=[1, 1 << 32, (1 << 64) - 1])
    assert r["cos"][0] == f32(np.cos(np.pi / 2)) and r["sin"][0] == 1
    assert list(r["seed_lo"]) == [1, 0, 0xFFFFFFFF] and list(r["seed_hi"]) == [0, 1, 0xFFFFFFFF]


def test_identity_record_at_pivot_zero_returns_the_valid_rows():
    B, P = 4, 37
    xyz, rgb = _clouds(B, P, 1)
    xyz[0, 0, 0], rgb[0, 1, 2] = -0.0, -0.0
    n = np.array([P, 1, 20, 0], np.int32)
    for order in range(6):
        ox, oc, on = ops.cloud_augment_ref(xyz, rgb, n, ops.cloud_augment_records(B, order=order, seed=order), (0, 0, 0))
        assert ox.dtype == f32 and oc.dtype == f32 and on.dtype == np.int32
        assert list(on) == [P, 1, 20, 1]                               # clamp(n, 1, P)
        for b in range(B):
            k = int(on[b])
            assert (ox[b, :k] == xyz[b, :k]).all() and (oc[b, :k] == rgb[b, :k]).all(), (order, b)
            assert not ox[b, k:].any() and not oc[b, k:].any()         # zero rows behind
    assert not np.signbit(ox[0, 0, 0]) and not np.signbit(oc[0, 1, 2])   # -0.0 comes back as +0.0


def test_identity_record_at_a_pivot_is_within_one_ulp():
    B, P = 2, 257
    xyz, rgb = _clouds(B, P, 2)
    pivot = np.array([0.31, -0.12, 0.77], f32)
    ox, oc, on = ops.cloud_augment_ref(xyz, rgb, None, ops.cloud_augment_records(B), pivot)
    assert list(on) == [P, P] and (oc == rgb).all()
    bound = _ulp(np.maximum(np.abs(xyz), np.abs(pivot)))               # (p - c) + c rounds twice
    err = np.abs(ox.astype(np.float64) - xyz.astype(np.float64))
    assert (err <= bound).all(), float((err / bound).max())
    assert err.max() > 0                                               # and the pivot really is subtracted and added


def test_ref_matches_an_independent_float64_transform():
    B, P = 6, 300
    xyz, rgb = _clouds(B, P, 3)
    n = np.array([P, 1, 150, 299, 64, 65], np.int32)
    pivot = np.array([0.2, -0.1, 0.4], f32)
    rec = _random_records(B, 4, drop=0.0)
    ox, oc, on = ops.cloud_augment_ref(xyz, rgb, n, rec, pivot)
    assert list(on) == list(n)
    worst = 0.0
    for b in range(B):
        m, r = int(n[b]), rec[b]
        p = xyz[b, :m].astype(np.float64)
        u = ops.u01_ref(int(r["seed_lo"]) | int(r["seed_hi"]) << 32, np.arange(4 * m)).reshape(m, 4).astype(np.float64)
        rot = np.array([[r["cos"], -r["sin"], 0], [r["sin"], r["cos"], 0], [0, 0, 1]], np.float64)
        t = np.array([r["tx"], r["ty"], r["tz"]], np.float64)
        q = (p - pivot) @ rot.T * float(r["scale"]) + pivot + t + (2 * u[:, :3] - 1) * float(r["jitter"])
        mag = np.abs(p) + np.abs(pivot.astype(np.float64)) + np.abs(t) + float(r["jitter"])
        bound = 8 * _ulp(mag)                                          # 8: see the module docstring
        err = np.abs(ox[b, :m].astype(np.float64) - q)
        assert (err <= bound).all(), (b, float((err / bound).max()))
        worst = max(worst, float((err / _ulp(mag)).max()))
    print(f"worst error: {worst:.2f} ulp of |p| + |pivot| + |t| + jitter")
    # the colour ops against float64, with the mean as the definition states it (an integer sum): 3 ops of 3 roundings each on
    # values of at most 255 * 1.5 -> 16 ulp of 512 is generous and still far below one grey level
    for b in range(B):
        m, r = int(n[b]), rec[b]
        c = rgb[b, :m].astype(np.float64)
        for op in ops.AUGMENT_ORDERS[int(r["order"])]:
            g = 0.2989 * c[:, 0] + 0.587 * c[:, 1] + 0.114 * c[:, 2]
            if op == 0:
                c = np.clip(float(r["fb"]) * c, 0, 255)
            elif op == 1:
                mean = np.trunc(np.clip(g.astype(f32), 0, 255)).sum() / m
                c = np.clip(float(r["fc"]) * c + (1 - float(r["fc"])) * mean, 0, 255)
            else:
                c = np.clip(float(r["fs"]) * c + (1 - float(r["fs"])) * g[:, None], 0, 255)
        assert np.abs(oc[b, :m] - c).max() <= 16 * float(np.spacing(f32(512))), b


def test_rows_behind_n_never_matter_and_kept_rows_stay_in_order():
    B, P = 5, 65
    xyz, rgb = _clouds(B, P, 5)
    n = np.array([P, 1, 32, 64, 0], np.int32)
    rec = _random_records(B, 6, drop=0.5)
    a = ops.cloud_augment_ref(xyz, rgb, n, rec, (0.1, 0.2, 0.3))
    xn, cn = xyz.copy(), rgb.copy()
    for b in range(B):
        xn[b, max(int(n[b]), 1):], cn[b, max(int(n[b]), 1):] = np.nan, np.nan
    b_ = ops.cloud_augment_ref(xn, cn, n, rec, (0.1, 0.2, 0.3))
    for x, y in zip(a, b_):
        assert x.tobytes() == y.tobytes()                              # no output bit changes
    assert np.isfinite(b_[0]).all() and np.isfinite(b_[1]).all()
    # order: with the geometry and the colours at the identity, the output is the kept subsequence of the input
    rec_id = ops.cloud_augment_records(B, drop=0.5, seed=[3, 4, 5, 6, 7])
    ox, oc, on = ops.cloud_augment_ref(xyz, rgb, None, rec_id, (0, 0, 0))
    assert 0 < on.min() and on.max() < P                               # something dropped, something kept, everywhere
    for b in range(B):
        keep = ops.u01_ref(int(rec_id["seed_lo"][b]), 4 * np.arange(P) + 3) >= f32(0.5)
        assert int(keep.sum()) == on[b] and (ox[b, :on[b]] == xyz[b][keep]).all() and (oc[b, :on[b]] == rgb[b][keep]).all()
        assert not ox[b, on[b]:].any() and not oc[b, on[b]:].any()


def test_a_draw_that_drops_everything_keeps_row_zero():
    B, P = 4, 33
    xyz, rgb = _clouds(B, P, 7)
    rec = ops.cloud_augment_records(B, angle=3.0, scale=1.02, shift=(0.01, 0, -0.01), drop=f32(0.9999999), seed=[11, 12, 13, 14])
    for b in range(B):                                                 # (no draw of these seeds reaches the top value)
        assert (ops.u01_ref(int(rec["seed_lo"][b]), 4 * np.arange(P) + 3) < f32(0.9999999)).all()
    ox, oc, on = ops.cloud_augment_ref(xyz, rgb, None, rec, (0, 0, 0))
    full = ops.cloud_augment_ref(xyz, rgb, None, ops.cloud_augment_records(B, angle=3.0, scale=1.02, shift=(0.01, 0, -0.01),
                                                                           seed=[11, 12, 13, 14]), (0, 0, 0))
    assert list(on) == [1] * B
    assert (ox[:, 0] == full[0][:, 0]).all() and (oc[:, 0] == full[1][:, 0]).all()    # exactly row 0, transformed
    assert not ox[:, 1:].any() and not oc[:, 1:].any()


def test_counts_are_clamped():
    xyz, rgb = _clouds(3, 8, 8)
    rec = ops.cloud_augment_records(3)
    _, _, on = ops.cloud_augment_ref(xyz, rgb, np.array([0, 9, -5], np.int32), rec, (0, 0, 0))
    assert list(on) == [1, 8, 1]
    _, _, on = ops.cloud_augment_ref(torch.from_numpy(xyz), torch.from_numpy(rgb), torch.tensor([1 << 30, 8, 3], dtype=torch.int32), rec, (0, 0, 0))
    assert list(on) == [8, 8, 3]
    with pytest.raises(ValueError):
        ops.cloud_augment_ref(xyz, rgb, np.array([1, 2], np.int32), rec, (0, 0, 0))
    with pytest.raises(ValueError):
        ops.cloud_augment_ref(xyz.astype(np.float64), rgb, None, rec, (0, 0, 0))


def test_u01_in_numpy_is_uniform_and_is_the_header_function():
    u = ops.u01_ref(0x0123456789ABCDEF, np.arange(1 << 20, dtype=np.uint64))
    assert u.dtype == f32 and u.min() >= 0.0 and u.max() < 1.0
    print(f"mean of 2^20 draws: {float(u.mean(dtype=np.float64)):.4f}")
    assert abs(float(u.mean(dtype=np.float64)) - 0.5) <= 0.002
    # actmi_mix32 / actmi_u01 of csrc/dropout.h in Python integers, value by value, the high index word included
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF; x ^= x >> 16
        return x
    for seed in (0, 0x0123456789ABCDEF, (1 << 64) - 1):
        idx = [0, 1, 7, (1 << 32) - 1, 1 << 32, (1 << 40) + 5]
        got = ops.u01_ref(seed, np.array(idx, dtype=np.uint64))
        for i, g in zip(idx, got):
            h = mix((i & 0xFFFFFFFF) ^ (seed & 0xFFFFFFFF))
            h = mix(h ^ (i >> 32) ^ (seed >> 32) ^ 0x9E3779B9)
            assert float(g) == (h >> 8) / 16777216.0, (seed, i)


def test_draws_stay_in_range_repeat_and_differ_by_seed(host_only):
    aug = ops.CloudAugment("cuda:0", max_points=128, max_batch=64, pivot=(0.1, 0.2, 0.3), seed=5)
    a = aug.draw_records(64)
    assert a.shape == (64,) and a.dtype == ops.cloud_augment_record_dtype()
    ang = np.degrees(np.arctan2(a["sin"].astype(np.float64), a["cos"].astype(np.float64)))
    assert np.abs(ang).max() <= 5.0 + 1e-4 and ang.min() < -2 and ang.max() > 2
    assert np.allclose(a["cos"].astype(np.float64) ** 2 + a["sin"].astype(np.float64) ** 2, 1.0, atol=1e-6)
    assert 0.95 - 1e-6 <= a["scale"].min() and a["scale"].max() <= 1.05 + 1e-6 and a["scale"].max() - a["scale"].min() > 0.05
    for k in ("tx", "ty", "tz"):
        assert np.abs(a[k]).max() <= 0.01 + 1e-8 and a[k].max() - a[k].min() > 0.01
    assert (a["jitter"] == f32(0.002)).all() and (a["drop"] == f32(0.1)).all()
    for name, x in (("fb", 0.3), ("fc", 0.4), ("fs", 0.5)):
        assert 1 - x - 1e-6 <= a[name].min() and a[name].max() <= 1 + x + 1e-6 and a[name].max() - a[name].min() > x
    assert set(a["order"]) == set(range(6))
    seeds = a["seed_lo"].astype(np.uint64) | a["seed_hi"].astype(np.uint64) << np.uint64(32)
    assert len(set(seeds.tolist())) == 64 and a["seed_hi"].max() > 1 << 24          # 64 bits, one seed per sample
    b = aug.draw_records(64)
    assert not np.array_equal(a, b)
    aug.set_seed(5)
    assert np.array_equal(aug.draw_records(64), a) and np.array_equal(aug.draw_records(64), b)
    assert not np.array_equal(ops.CloudAugment("cuda:0", 128, 64, seed=6).draw_records(64), a)
    assert len(aug.records()) == 0                                     # nothing was uploaded
    for bad in ({"drop": 1.0}, {"scale": -0.1}, {"pivot": (0, 0)}, {"pivot": (0, 0, float("nan"))}, {"max_points": 0}, {"max_batch": 70000}):
        kw = dict({"max_points": 128, "max_batch": 4}, **bad)
        with pytest.raises(ValueError):
            ops.CloudAugment("cuda:0", **kw)
    with pytest.raises(ValueError):
        ops.CloudAugment("cpu", 128, 4)


def _args(**kw):
    base = {"task_name": "sim_transfer_cube_scripted", "policy_class": "ACT", "lr": 1e-5, "chunk_size": 100, "kl_weight": 10,
            "hidden_dim": 512, "dim_feedforward": 3200, "batch_size": 8, "num_steps": 10, "eval_every": 5, "validate_every": 5,
            "save_every": 5, "ckpt_dir": "ckpt", "seed": 0, "temporal_agg": False}
    base.update(kw)
    return base


def test_cli_flag_pivot_and_refusals(monkeypatch):
    import imitate_episodes as ie
    need = ["--ckpt_dir", "c", "--policy_class", "ACT", "--task_name", "sim_transfer_cube_scripted", "--batch_size", "8", "--seed", "0",
            "--num_steps", "10", "--lr", "1e-5"]
    parser = ie.make_parser()
    plain = vars(parser.parse_args(need))
    assert plain["augment_clouds"] is False and plain["cloud_pivot"] == [0.0, 0.0, 0.0]
    got = vars(parser.parse_args(need + ["--use_pcd", "--augment_clouds", "--cloud_pivot", "0.3", "-0.1", "0.5", "--augment_images"]))
    assert got["augment_clouds"] is True and got["cloud_pivot"] == [0.3, -0.1, 0.5] and got["augment_images"] is True
    task = "sim_transfer_cube_scripted"
    monkeypatch.setitem(ie.SIM_TASK_CONFIGS, task, dict(ie.SIM_TASK_CONFIGS[task], pointcloud_names=["front"]))
    before = ie.build_config(_args(use_pcd=True))
    assert "augment_clouds" not in before and "cloud_pivot" not in before
    assert ie.build_config(_args(use_pcd=True, augment_clouds=False, cloud_pivot=[1.0, 2.0, 3.0])) == before
    cfg = ie.build_config(_args(use_pcd=True, augment_clouds=True, cloud_pivot=[0.3, -0.1, 0.5]))
    assert cfg.pop("augment_clouds") is True and cfg.pop("cloud_pivot") == [0.3, -0.1, 0.5] and cfg == before
    both = ie.build_config(_args(use_pcd=True, augment_clouds=True, augment_images=True))
    assert both["augment_clouds"] is True and both["augment_images"] is True and both["cloud_pivot"] == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="use_pcd"):
        ie.build_config(_args(augment_clouds=True))
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="Diffusion", augment_clouds=True))
    with pytest.raises(NotImplementedError):
        ie.build_config(_args(policy_class="CNNMLP", augment_clouds=True))
    with pytest.raises(ValueError, match="cloud_pivot"):
        ie.build_config(_args(use_pcd=True, augment_clouds=True, cloud_pivot=[0.0, float("inf"), 0.0]))
    assert ie.make_cloud_augment(before, None, 0) is None              # without the flag nothing is built


def test_make_cloud_augment_sizes_from_the_engine(host_only):
    import imitate_episodes as ie
    eng = type("E", (), {"cfg": object(), "device": torch.device("cuda:0"), "max_points": 96, "max_batch": 3})()
    pol = type("P", (), {"model": eng})()
    aug = ie.make_cloud_augment({"augment_clouds": True, "cloud_pivot": [0.3, -0.1, 0.5]}, pol, seed=9)
    assert isinstance(aug, ops.CloudAugment) and (aug.max_points, aug.max_batch, aug.pivot) == (96, 3, (0.3, -0.1, 0.5))
    assert np.array_equal(aug.draw_records(3), ops.CloudAugment("cuda:0", 96, 3, seed=9).draw_records(3))
    # the seed train_bc gives it differs from the image augmenter's for every run seed
    assert all((s ^ ie.CLOUD_AUGMENT_SEED_MIX) != s for s in range(64)) and ie.CLOUD_AUGMENT_SEED_MIX > 1 << 32


def test_forward_pass_routes_the_clouds_through_the_augmenter():
    import imitate_episodes as ie
    seen, calls, img_calls = {}, [], []

    class Policy:
        def __call__(self, qpos, image, actions=None, is_pad=None, **kw):
            seen.clear()
            seen.update(kw, image=image)
            return {"loss": 0.0}

    class Cloud:
        def apply(self, xyz, rgb, n=None):
            calls.append((xyz, rgb, n))
            return xyz + 1, rgb * 2, n - 1

    class Image:
        def apply(self, image_u8, depth_u16=None, B=None):
            img_calls.append(image_u8)
            return image_u8 + 1
    pol = Policy()
    pol.model = type("M", (), {"device": torch.device("cpu")})()
    img, qpos = torch.zeros(2, 1, 12, 16, 3, dtype=torch.uint8), torch.zeros(2, 14)
    act, pad = torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.bool)
    xyz, rgb, n = torch.randn(2, 5, 3), torch.rand(2, 5, 3), torch.tensor([5, 3], dtype=torch.int32)
    batch = (img, qpos, act, pad, xyz, rgb, n)
    ie.forward_pass(batch, pol, cloud_augment=Cloud())
    assert len(calls) == 1 and torch.equal(calls[0][0], xyz) and torch.equal(calls[0][1], rgb) and torch.equal(calls[0][2], n)
    pc = seen["pointcloud"]
    assert torch.equal(pc["xyz"], xyz + 1) and torch.equal(pc["rgb"], rgb * 2) and torch.equal(pc["n"], n - 1)
    assert seen["image"].data_ptr() == img.data_ptr() and not img_calls           # the image is not touched
    # both augmenters: each gets its own modality, once
    calls.clear()
    ie.forward_pass(batch, pol, Image(), Cloud())
    assert len(calls) == 1 and len(img_calls) == 1 and torch.equal(seen["image"], img + 1)
    assert torch.equal(seen["pointcloud"]["xyz"], xyz + 1)
    # without it the clouds are the batch's own, and a batch without clouds never calls it
    calls.clear()
    ie.forward_pass(batch, pol)
    assert not calls and seen["pointcloud"]["xyz"].data_ptr() == xyz.data_ptr() and torch.equal(seen["pointcloud"]["n"], n)
    ie.forward_pass((img, qpos, act, pad), pol, cloud_augment=Cloud())
    assert not calls and "pointcloud" not in seen
