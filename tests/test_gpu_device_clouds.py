"""Stored point clouds out of the device-resident episode store, on the GPU: actmi_op_gather_clouds against its numpy statement at
the sizes and addresses where its forms change, the store's 7-tuples against the host loader's from the same seed (ragged episodes,
mirror twins with a cloud rule), DeviceEpisodeReplay against EpisodeReplay, training steps and replays fed either way.  Everything is
torch.equal / np.array_equal, no tolerance: the op is copies, an exact uint8 -> f32 conversion and one fp32 subtract."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import imitate_episodes as IE  # noqa: E402
from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from test_device_clouds_cpu import CAMS, NAME, RULE, cloud_twin_dirs, write_cloud_dataset  # noqa: E402

DEV = "cuda:0"
SENT_F, SENT_I = -7.25, -77
# (rows of every item): one item and five, whole words (4, 8), rows that are none (1, 3, 5, 9, 257), 257 rows = several passes of a
# workgroup and, in the general form, more than one workgroup per item
ROW_SETS = [(4,), (3,), (257,), (8, 4, 3, 5, 1), (257, 9, 4, 1, 8)]


@functools.lru_cache(maxsize=None)
def _arena(rows, f32c, odd):
    """a random arena that holds one cloud per entry of `rows` -- at multiples of 16, or (`odd`) at addresses of every kind, one of
    them a multiple of 16 all the same -- and the item records, mirror flags mixed; computed once and left unchanged"""
    rng = np.random.default_rng(sum(rows) * 4 + 2 * f32c + odd)
    shifts = [1, 4, 0, 7, 2] if odd else [0] * 5
    parts, items, at = [], np.zeros(len(rows), dtype=ops.cloud_item_dtype()), 48
    for i, r in enumerate(rows):
        x = rng.standard_normal((r, 3)).astype(np.float32)
        x[r // 2] = 0                                                # a stored zero row
        c = rng.integers(0, 256, (r, 3), dtype=np.uint8)
        cb = c.astype(np.float32).reshape(-1).view(np.uint8) if f32c else c.reshape(-1)
        xo = at + shifts[i % 5]
        co = (xo + r * 12 + 15) // 16 * 16 + 32 + shifts[(i + 1) % 5]
        parts += [(xo, x.reshape(-1).view(np.uint8)), (co, cb)]
        items[i] = (xo, co, r, max(1, r - i), (i + len(rows)) % 2, 0)
        at = (co + cb.size + 15) // 16 * 16 + 16
    arena = rng.integers(0, 256, at + 64, dtype=np.uint8)
    for o, p in parts:
        arena[o:o + p.size] = p
    return arena, items


def _guarded(B, P, lead):
    """the three outputs in the middle of sentinel-filled buffers; lead 8 floats: 16-byte aligned, 3: only 4"""
    bx = torch.full((lead + B * P * 3 + 13,), SENT_F, dtype=torch.float32, device=DEV)
    bc = torch.full((lead + B * P * 3 + 13,), SENT_F, dtype=torch.float32, device=DEV)
    bn = torch.full((B + 8,), SENT_I, dtype=torch.int32, device=DEV)
    return (bx, bc, bn), (bx[lead:lead + B * P * 3].view(B, P, 3), bc[lead:lead + B * P * 3].view(B, P, 3), bn[4:4 + B])


def _guards_intact(bufs, B, P, lead):
    bx, bc, bn = (b.cpu() for b in bufs)
    n = B * P * 3
    return all(bool((b[:lead] == SENT_F).all()) and bool((b[lead + n:] == SENT_F).all()) for b in (bx, bc)) and \
        bool((bn[:4] == SENT_I).all()) and bool((bn[4 + B:] == SENT_I).all())


def _same(got, exp):
    """bits, not values: -0.0 and +0.0 differ"""
    return all(g.dtype == torch.from_numpy(e).dtype and tuple(g.shape) == e.shape and
               np.array_equal(g.cpu().numpy().view(np.int32), e.view(np.int32)) for g, e in zip(got, exp))


@pytest.mark.parametrize("odd", [False, True], ids=["at16", "odd"])
@pytest.mark.parametrize("f32c", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("rows", ROW_SETS, ids=[str(r) for r in ROW_SETS])
def test_gather_clouds_equals_the_numpy_statement(rows, f32c, odd):
    arena_np, items = _arena(rows, f32c, odd)
    arena = torch.from_numpy(arena_np).to(DEV)
    t_items = torch.from_numpy(items.view(np.uint8).copy()).to(DEV)
    B, top = len(rows), max(rows)
    axis, c2 = sum(rows) % 3, (0.0 if (len(rows) + odd) % 2 else 0.3)
    seen = set()
    for P in sorted({top, top + 7, (top + 3) // 4 * 4, (top + 10) // 4 * 4, max(top - 2, 1)}):    # the last: P below the largest item
        exp = ops.gather_clouds_ref(arena_np, items, P, int(f32c), mirror=(axis, c2))
        for aligned in (0, 1, 2) if P % 4 == 0 else (0,):
            lead = 8 if aligned else 3
            bufs, out = _guarded(B, P, lead)
            got = ops.gather_clouds(arena, t_items, P, int(f32c), mirror=(axis, c2), out=out, aligned=aligned)
            assert got[0].data_ptr() == out[0].data_ptr()
            assert _same(out, exp), (rows, P, aligned)
            assert _guards_intact(bufs, B, P, lead), "values around the outputs were written"
            for t in out:
                t.fill_(5)
            ops.gather_clouds(arena, t_items, P, int(f32c), mirror=(axis, c2), out=out, aligned=aligned)     # twice: the same bits
            assert _same(out, exp)
            seen.add(aligned)
    assert seen == {0, 1, 2}
    # every axis, c2 zero and not, on fresh outputs
    for ax in range(3):
        for c in (0.0, -1.75):
            P = (top + 3) // 4 * 4
            got = ops.gather_clouds(arena, t_items, P, int(f32c), mirror=(ax, c), aligned=1)
            assert _same(got, ops.gather_clouds_ref(arena_np, items, P, int(f32c), mirror=(ax, c))), (ax, c)
    if B > 1:
        assert items["flags"].min() == 0 and items["flags"].max() == 1


@pytest.mark.parametrize("f32c", [False, True], ids=["u8", "f32"])
def test_an_item_that_leaves_the_arena_is_zero_filled_and_its_neighbours_are_intact(f32c):
    arena_np, items = _arena((8, 4, 3, 5, 1), f32c, False)
    arena = torch.from_numpy(arena_np).to(DEV)
    cb = 12 if f32c else 3
    for aligned in (0, 1, 2):
        bad = np.concatenate([items, items[:1], items[:1]])            # 7 items
        bad["xyz_off"][1] = -16
        bad["rgb_off"][3] = arena_np.size - 5 * cb + 1                 # the colour range ends one byte past the arena
        bad["flags"][3] = 1
        bad["xyz_off"][5] = 1 << 40
        bad["xyz_off"][6] = arena_np.size - 8 * 12 + 16                # the xyz range ends past it, at a multiple of 16
        P = 8
        bufs, out = _guarded(7, P, 8)
        ops.gather_clouds(arena, torch.from_numpy(bad.view(np.uint8).copy()).to(DEV), P, int(f32c), mirror=(0, 0.5), out=out, aligned=aligned)
        exp = ops.gather_clouds_ref(arena_np, bad, P, int(f32c), mirror=(0, 0.5))
        assert _same(out, exp) and _guards_intact(bufs, 7, P, 8), aligned
        n = out[2].cpu().tolist()
        assert [n[i] for i in (1, 3, 5, 6)] == [0] * 4 and all(n[i] > 0 for i in (0, 2, 4))
        for i in (1, 3, 5, 6):
            assert not bool(out[0][i].any()) and not bool(out[1][i].any())
        assert all(bool(out[0][i].any()) and bool(out[1][i].any()) for i in (0, 2, 4))
    # a range that ends exactly at the arena's end is read
    last = items[:1].copy()
    last["xyz_off"], last["rows"], last["flags"] = arena_np.size - 4 * 12, 4, 0
    arena[-48:] = torch.arange(48, dtype=torch.uint8, device=DEV)    # (finite values)
    arena_np = arena.cpu().numpy()
    got = ops.gather_clouds(arena, torch.from_numpy(last.view(np.uint8).copy()).to(DEV), 4, int(f32c), aligned=1)
    assert _same(got, ops.gather_clouds_ref(arena_np, last, 4, int(f32c))) and int(got[2][0]) == int(last["n"][0])


def test_bad_arguments_are_refused():
    arena_np, items = _arena((8, 4, 3, 5, 1), False, False)
    arena = torch.from_numpy(arena_np).to(DEV)
    t_items = torch.from_numpy(items.view(np.uint8).copy()).to(DEV)
    with pytest.raises(RuntimeError, match="P % 4"):
        ops.gather_clouds(arena, t_items, 9, 0, aligned=1)
    with pytest.raises(RuntimeError, match="rgb_fmt"):
        ops.gather_clouds(arena, t_items, 8, 2)
    with pytest.raises(RuntimeError, match="mirror_axis"):
        ops.gather_clouds(arena, t_items, 8, 0, mirror=(3, 0.0))
    with pytest.raises(RuntimeError, match="P outside"):
        ops.gather_clouds(arena, t_items, 0, 0)
    with pytest.raises(ValueError, match="32-byte records"):
        ops.gather_clouds(arena, t_items[:-1], 8, 0)
    with pytest.raises(ValueError, match="out xyz"):
        ops.gather_clouds(arena, t_items, 8, 0, out=(torch.empty((5, 7, 3), device=DEV), torch.empty((5, 8, 3), device=DEV),
                                                     torch.empty(5, dtype=torch.int32, device=DEV)))
    empty = ops.gather_clouds(arena, t_items[:0], 8, 0)               # B = 0: nothing to do
    assert tuple(empty[0].shape) == (0, 8, 3)


def test_gather_clouds_offsets_beyond_4_gib():
    """an uninitialised arena of about 4.5 GiB, two clouds written, the xyz of one and the colours of the other past the 4 GiB mark:
    32-bit offset arithmetic would read the wrong place"""
    total = (9 << 29) + 4096
    arena = torch.empty(total, dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(5)
    far = (1 << 32) + 4096
    for rows, aligned, shift in ((8, 2, 0), (5, 0, 3)):
        x = [rng.standard_normal((rows, 3)).astype(np.float32) for _ in range(2)]
        c = [rng.integers(0, 256, (rows, 3), dtype=np.uint8) for _ in range(2)]
        places = [(far + 16 + shift, 1024 + shift), (2048 + shift, far + 512 + shift)]
        items = np.zeros(3, dtype=ops.cloud_item_dtype())
        for i, (xo, co) in enumerate(places):
            for o in (xo, co):
                arena[o & 0xFFFFFFFF:(o & 0xFFFFFFFF) + rows * 12] = 0                 # where a 32-bit offset would land
        for i, (xo, co) in enumerate(places):
            arena[xo:xo + rows * 12] = torch.from_numpy(x[i].reshape(-1).view(np.uint8)).to(DEV)
            arena[co:co + rows * 3] = torch.from_numpy(c[i].reshape(-1)).to(DEV)
            items[i] = (xo, co, rows, rows, i, 0)
        items[2] = items[0]
        P = 8
        got = ops.gather_clouds(arena, torch.from_numpy(items.view(np.uint8).copy()).to(DEV), P, 0, mirror=(2, 0.5), aligned=aligned)
        xyz, rgb, n = (t.cpu().numpy() for t in got)
        m = x[1].copy()
        m[:, 2] = np.float32(0.5) - m[:, 2]
        assert np.array_equal(xyz[0, :rows], x[0]) and np.array_equal(xyz[1, :rows], m) and np.array_equal(xyz[2], xyz[0])
        assert np.array_equal(rgb[0, :rows], c[0].astype(np.float32)) and np.array_equal(rgb[1, :rows], c[1].astype(np.float32))
        assert not xyz[:, rows:].any() and not rgb[:, rows:].any() and n.tolist() == [rows] * 3
    del arena
    torch.cuda.empty_cache()


# ---- the store's batches against the host loader's -------------------------------------------------------------------------------------
def _tuples_equal(d, h):
    return len(d) == len(h) and all(x.is_cuda and x.dtype == y.dtype and tuple(x.shape) == tuple(y.shape) and torch.equal(x.cpu(), y)
                                    for x, y in zip(d, h))


@pytest.mark.parametrize("rgb_u8,mask", [(True, True), (False, True), (True, False)])
def test_device_loaders_deliver_the_host_loaders_7_tuples(tmp_path, rgb_u8, mask):
    write_cloud_dataset(tmp_path / "data", Ns=(9, 8, 5, 12), rgb_u8=rgb_u8, mask=mask)
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.75, pointcloud_names=[NAME], use_pcd=True, max_points=12)
    h_tr, h_va, h_stats, _ = D.load_data(str(tmp_path / "data"), lambda n: True, list(CAMS), 5, 3, 4, rng=np.random.default_rng(3), **kw)
    d_tr, d_va, d_stats, _ = D.load_data(str(tmp_path / "data"), lambda n: True, list(CAMS), 5, 3, 4, rng=np.random.default_rng(3),
                                         device_dataset=True, device_clouds=True, device=DEV, **kw)
    store = d_tr.store
    assert store is d_va.store and store.has_clouds and store.cloud_rgb_fmt == (0 if rgb_u8 else 1) and store.cloud_n.dtype == np.int32
    assert store.device_bytes() >= store.nbytes == store.arena.numel()
    Ps = set()
    for hl, dl in ((h_tr, d_tr), (h_va, d_va)):
        hi, di = iter(hl), iter(dl)
        for _ in range(6):
            h, d = next(hi), next(di)
            assert len(d) == 7 and d[6].dtype == torch.int32 and _tuples_equal(d, h)
            Ps.add(int(d[4].shape[1]))
    assert len(Ps) > 1                                                 # ragged: the batches' P differ
    if mask:
        assert int(d[6].min()) < int(d[4].shape[1])


def test_device_loaders_with_mirror_twins_and_a_cloud_rule(tmp_path):
    plain, written = cloud_twin_dirs(tmp_path, Ns=(9, 8, 5))
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.7, pointcloud_names=[NAME], use_pcd=True, max_points=9)
    h_tr, h_va, _, _ = D.load_data(str(tmp_path / "written"), lambda n: True, list(CAMS), 5, 3, 4, rng=np.random.default_rng(8), **kw)
    d_tr, d_va, _, _ = D.load_data(str(tmp_path / "plain"), lambda n: True, list(CAMS), 5, 3, 4, rng=np.random.default_rng(8),
                                   mirror_twins=True, cloud_mirror=RULE, device_dataset=True, device_clouds=True, device=DEV, **kw)
    store = d_tr.store
    assert store.has_twins and store.has_clouds and len(store.paths) == 6 and len(store.sources) == 3
    alone = D.DeviceEpisodeStore(plain, [0, 1, 2], list(CAMS), store.norm_stats, DEV, use_pcd=True, pointcloud_names=[NAME], max_points=9)
    assert store.nbytes == alone.nbytes                                # the twins add no bytes
    for hl, dl in ((h_tr, d_tr), (h_va, d_va)):
        hi, di = iter(hl), iter(dl)
        for _ in range(6):
            assert _tuples_equal(next(di), next(hi))
    # a twin's cloud is its source's, reflected: the y of every stored row
    tw = [i for i, t in enumerate(store.twin) if t][0]
    so = [i for i, p in enumerate(store.paths) if not store.twin[i] and str(p) == store.paths[tw].source][0]
    a, b = store.gather([so], [2], 4), store.gather([tw], [2], 4)
    assert torch.equal(b[4][..., 1], np.float32(0.25) - a[4][..., 1]) and torch.equal(b[4][..., 0], a[4][..., 0])
    assert torch.equal(b[5], a[5]) and torch.equal(b[6], a[6])


def test_device_episode_replay_yields_what_episode_replay_yields(tmp_path):
    paths = write_cloud_dataset(tmp_path, Ns=(9, 8, 5))
    stats, _ = D.get_norm_stats(paths)
    kw = dict(pointcloud_names=[NAME], use_pcd=True, max_points=9)
    store = D.DeviceEpisodeStore(paths, [2, 0, 1], list(CAMS), stats, DEV, **kw)
    for eid, path in enumerate(paths):
        for batch, stride in ((4, 1), (2, 4), (64, 1), (3, 2)):
            host = D.EpisodeReplay(path, list(CAMS), stats, batch, stride=stride, **kw)
            dev = D.DeviceEpisodeReplay(store, eid, batch, stride=stride)
            hb, db = list(host), list(dev)
            assert len(hb) == len(db) == len(host) == len(dev)
            for h, d in zip(hb, db):
                assert len(d) == 5 and d[4].dtype == torch.int32 and _tuples_equal(d, h), (eid, batch, stride)


def test_a_store_without_clouds_launches_and_returns_what_it_did(tmp_path, monkeypatch):
    paths = write_cloud_dataset(tmp_path, Ns=(9, 8, 5))
    stats, lens = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, [0, 1, 2], list(CAMS), stats, DEV)
    fb = 12 * 16 * 3
    assert not store.has_clouds and store.nbytes == 9 * (-(-6 * fb // 256) * 256) and len(store.cloud_n) == 0
    calls = []
    real = {k: getattr(ops, k) for k in ("gather_frames", "gather_chunks", "gather_clouds", "gather_frames_mirror")}
    for k, fn in real.items():
        monkeypatch.setattr(ops, k, lambda *a, _k=k, _fn=fn, **kw: (calls.append(_k), _fn(*a, **kw))[1])
    out = store.gather([0, 2, 1], [5, 0, 3], 4)
    assert calls == ["gather_frames", "gather_chunks"] and len(out) == 4
    ds = D.EpisodicDataset(paths, list(CAMS), stats, [0, 1, 2], lens, 4, "ACT")
    exp = torch.utils.data.default_collate([ds[5], ds[12], ds[9]])
    assert _tuples_equal(out, exp)
    calls.clear()
    with_clouds = D.DeviceEpisodeStore(paths, [0, 1, 2], list(CAMS), stats, DEV, use_pcd=True, pointcloud_names=[NAME])
    out7 = with_clouds.gather([0, 2, 1], [5, 0, 3], 4)
    assert sorted(calls) == ["gather_chunks", "gather_clouds", "gather_frames"] and len(out7) == 7      # one more launch
    assert _tuples_equal(out7[:4], exp)


# ---- training steps and replays fed by the store against the host loader ------------------------------------------------------------------
TCAMS = ["a", "b"]
PC = {"use_pcd": True, "pcd_hidden_dim": 64, "pcd_output_dim": 64, "max_points": 48, "kl_weight": 10, "lr": 1e-4, "num_queries": 8,
      "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2, "nheads": 4, "camera_names": TCAMS, "image_h": 64,
      "image_w": 96, "base_width": 8}                                # the tiny point-cloud config of tests/test_gpu_cloud_augment.py


@pytest.fixture(scope="module")
def train_data(tmp_path_factory):
    root = tmp_path_factory.mktemp("device_clouds")
    paths = write_cloud_dataset(root / "data", Ns=(48, 37, 20), T=8, cams=TCAMS, hw=(64, 96), sims=(True, True, True))
    return root, paths


def _policy():
    from policy import ACTPolicy
    pol = ACTPolicy(dict(PC), max_batch=3)
    pol.train()
    pol.train_dropout = 0.0
    return pol


def _loaders(root, device):
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.7, pointcloud_names=[NAME], use_pcd=True, max_points=48)
    if device:
        kw.update(device_dataset=True, device_clouds=True, device=DEV)
    return D.load_data(str(root / "data"), lambda n: True, TCAMS, 3, 3, 8, rng=np.random.default_rng(7), **kw)


def _config(root, ckpt):
    return {"ckpt_dir": str(root / ckpt), "state_dim": 14, "policy_class": "ACT", "policy_config": dict(PC, max_batch=3),
            "camera_names": TCAMS, "episode_len": 8, "task_name": "sim_transfer_cube_scripted", "temporal_agg": True,
            "dataset_dir": str(root / "data"), "pointcloud_names": [NAME]}


def _two_steps(root, device, augment, replay_between=False):
    train_dl, val_dl, stats, _ = _loaders(root, device)
    pol = _policy()
    opt = pol.configure_optimizers()
    aug = IE.make_cloud_augment({"augment_clouds": True, "cloud_pivot": [0.0, 0.0, 0.0]}, pol, seed=4) if augment else None
    it, losses = iter(train_dl), []
    for step in range(2):
        opt.zero_grad()
        pol.next_eps = torch.randn(3, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
        out = IE.forward_pass(next(it), pol, cloud_augment=aug)
        out["loss"].backward()
        opt.step()
        losses.append({k: float(v) for k, v in out.items()})
        if replay_between and step == 0:
            pol.eval()
            res = IE.replay_bc(_config(root, "between"), "policy_last.ckpt", policy=pol, stats=stats, store=train_dl.store,
                               episodes=val_dl.episode_ids, verbose=False)
            assert np.isfinite(res["mae_mean"]) and pol.model.read_flags(clear=False) == 0
            pol.train()
            pol.train_dropout = 0.0
    pol.model.check_flags()
    return losses


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment_clouds"])
def test_two_training_steps_give_the_same_loss_bits_fed_by_the_store_or_the_host_loader(train_data, augment):
    root, _ = train_data
    host, dev = _two_steps(root, False, augment), _two_steps(root, True, augment)
    print(f"two steps, host loader: {host}; device store: {dev}")
    assert all(np.isfinite(v) for s in host for v in s.values())
    assert host == dev and host[0] != host[1]
    if not augment:
        assert _two_steps(root, True, False, replay_between=True) == dev      # a replay between the steps leaves them alone


def test_replay_bc_out_of_the_store_gives_the_result_bits_of_the_files(train_data, tmp_path):
    from policy import ACTPolicy
    root, paths = train_data
    stats, _ = D.get_norm_stats(paths)
    policy = ACTPolicy(dict(PC), max_batch=3, init_seed=4)
    policy.eval()
    store = D.DeviceEpisodeStore(paths, [1, 2, 0], TCAMS, stats, DEV, use_pcd=True, pointcloud_names=[NAME], max_points=48)
    bare = D.DeviceEpisodeStore(paths, [1, 2, 0], TCAMS, stats, DEV)
    with pytest.raises(NotImplementedError, match="holds no point clouds"):
        IE.replay_bc(_config(tmp_path, "bare"), "policy_last.ckpt", policy=policy, stats=stats, batch=3, verbose=False, store=bare,
                     episodes=[0, 1, 2])
    for agg in (True, False):
        cf, cs = dict(_config(tmp_path, f"files{agg}"), dataset_dir=str(root / "data"), temporal_agg=agg), \
            dict(_config(tmp_path, f"store{agg}"), dataset_dir=str(root / "data"), temporal_agg=agg)
        from_files = IE.replay_bc(cf, "policy_last.ckpt", policy=policy, stats=stats, batch=3, verbose=False)
        from_store = IE.replay_bc(cs, "policy_last.ckpt", policy=policy, stats=stats, batch=3, verbose=False, store=store, episodes=[0, 1, 2])
        for i in range(3):
            a = np.load(os.path.join(cf["ckpt_dir"], f"replay_policy_last_ep{i}.npz"))
            b = np.load(os.path.join(cs["ckpt_dir"], f"replay_policy_last_ep{i}.npz"))
            assert np.array_equal(a["target"], b["target"]) and np.array_equal(a["pred"], b["pred"]), (agg, i)
        for k in ("mae", "rmse", "max", "mae_mean", "rmse_mean", "max_max", "steps"):
            assert from_files[k] == from_store[k], (agg, k)
        assert np.isfinite(from_store["mae_mean"]) and from_store["steps"] == 24
