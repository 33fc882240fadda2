"""Mirrored twin episodes on the GPU: actmi_op_gather_frames_mirror against its numpy statement at the sizes where its forms change,
and a device-resident store that serves twins against the host loader over twin FILES (written by the restatement of
postprocess_episodes.py in tests/test_mirror_twins_cpu.py) -- batches, replays and training losses, everything with torch.equal."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from test_mirror_twins_cpu import CAMS, twin_dirs  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xCD
CAMS = list(CAMS)


# ---- the op ----------------------------------------------------------------------------------------------------------------------
def _flags(kind, n):
    return {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "alternating": (np.arange(n) % 2 == 0).astype(np.uint8)}[kind]


def _case(arena_np, arena, H, W, px, off, flip, aligned, lead):
    """one launch into the middle of a sentinel-filled buffer, compared with the numpy statement; the bytes around stay untouched"""
    n, item = len(off), H * W * px
    big = torch.full((lead + n * item + 61,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = big[lead:lead + n * item]
    got = ops.gather_frames_mirror(arena, torch.from_numpy(off).to(DEV), torch.from_numpy(flip).to(DEV), H, W, px, out=out, aligned=aligned)
    assert got.data_ptr() == out.data_ptr()
    exp = ops.gather_frames_mirror_ref(arena_np, off, flip, H, W, px)
    where = (H, W, px, n, aligned, lead, flip[:4].tolist())
    assert torch.equal(out.cpu().view(n, H, W, px), torch.from_numpy(exp)), where
    big = big.cpu()
    assert bool((big[:lead] == SENTINEL).all()) and bool((big[lead + n * item:] == SENTINEL).all()), ("bytes around out were written", where)
    return out


# px 3: W = 15 / 16 / 17 / 32 / 48 around the 16-pixel group; 64 x 96 = 18,432 bytes, two workgroup shares of 16 KiB with the cut
# inside a row; 120 x 160 four shares; 480 x 640 the real frame (57 shares).  px 2: W = 7 / 8 / 9 around the 8-pixel group
SHAPES = [(1, 1, 3), (3, 2, 3), (5, 7, 3), (2, 15, 3), (2, 16, 3), (3, 17, 3), (1, 32, 3), (2, 48, 3), (64, 96, 3), (120, 160, 3),
          (480, 640, 3), (5, 7, 2), (2, 8, 2), (3, 9, 2), (64, 96, 2)]


OP_CASES = [(s, n) for s in SHAPES for n in (1, 37) if not (s[:2] == (480, 640) and n > 1)]       # one 480 x 640 item


@pytest.mark.parametrize("shape,n", OP_CASES, ids=["x".join(map(str, s)) + f"-n{n}" for s, n in OP_CASES])
def test_gather_frames_mirror_equals_the_numpy_statement(shape, n):
    H, W, px = shape
    item = H * W * px
    rng = np.random.default_rng(item * 100 + n)
    arena_np = rng.integers(0, 256, 40 * max(item, 16) + 4096, dtype=np.uint8)
    arena = torch.from_numpy(arena_np).to(DEV)
    top = arena_np.size - item
    even = rng.integers(0, top // 16, n, dtype=np.int64) * 16
    odd = np.minimum(even + rng.integers(0, 8, n) * 2 + 1, top)
    odd[0] |= 1
    if n > 1:
        even[n // 2], odd[n // 2] = even[0], odd[0]                  # one source named twice
    fast = W % (16 if px == 3 else 8) == 0
    for kind in ("none", "all", "alternating"):
        flip = _flags(kind, n)
        _case(arena_np, arena, H, W, px, odd, flip, 0, 3)            # general form: odd sources, odd destination
        out = _case(arena_np, arena, H, W, px, even, flip, 0, 32)
        if fast:
            for aligned in (1, 2):
                out = _case(arena_np, arena, H, W, px, even, flip, aligned, 32)
            # the flag is the caller's statement; an item whose offset breaks it is still moved right (the kernel looks at it)
            broken = even.copy()
            broken[::2] += np.array([5, 8, 1, 12])[np.arange(len(broken[::2])) % 4]
            _case(arena_np, arena, H, W, px, np.minimum(broken, top), flip, 1, 32)
            _case(arena_np, arena, H, W, px, np.minimum(broken, top), flip, 2, 32)
        if kind == "none":                                           # the bytes of actmi_op_gather_frames
            plain = ops.gather_frames(arena, torch.from_numpy(even).to(DEV), item, aligned=1 if item % 16 == 0 else 0)
            assert torch.equal(out.view(n, item), plain)


def test_gather_frames_mirror_zero_fills_an_item_that_leaves_the_arena_and_refuses_bad_arguments():
    arena_np = np.arange(1, 1 + 960, dtype=np.int64).astype(np.uint8)
    arena = torch.from_numpy(arena_np).to(DEV)
    for (H, W, px), aligned, off in (((2, 16, 3), 1, [0, 880, 864, -16, 1 << 40]), ((2, 16, 3), 0, [0, 880, 864, -16, 1 << 40]),
                                     ((5, 7, 3), 0, [3, 856, 855, -1, 1 << 40]), ((3, 8, 2), 2, [16, 928, 912, -16, 1 << 40])):
        for flip in ([1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 1, 0, 1, 1]):
            fl = np.asarray(flip, dtype=np.uint8)
            got = ops.gather_frames_mirror(arena, torch.tensor(off, dtype=torch.int64, device=DEV), torch.from_numpy(fl).to(DEV), H, W, px,
                                           aligned=aligned).cpu()
            exp = torch.from_numpy(ops.gather_frames_mirror_ref(arena_np, off, fl, H, W, px))
            assert torch.equal(got, exp) and not bool(got[1].any()) and not bool(got[3].any()) and not bool(got[4].any())
            assert bool(got[0].all()) and bool(got[2].all())             # the last item that still fits is moved
    z64, z8 = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.gather_frames_mirror(arena, z64, z8, 2, 15, 3, aligned=1)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        ops.gather_frames_mirror(arena[8:], z64, z8, 2, 16, 3, aligned=1)
    with pytest.raises(RuntimeError, match="px_bytes"):
        ops.gather_frames_mirror(arena, z64, z8, 2, 16, 4)
    with pytest.raises(ValueError):
        ops.gather_frames_mirror(arena, z64, z8[:1], 2, 16, 3)
    with pytest.raises(ValueError):
        ops.gather_frames_mirror(arena, z64, z8.to(torch.int8), 2, 16, 3)


# ---- the store against the host loader over written twin files ----------------------------------------------------------------------
def _equal(d, h):
    if h.dtype == torch.uint16:
        return d.dtype == torch.uint16 and tuple(d.shape) == tuple(h.shape) and torch.equal(d.cpu().view(torch.int16), h.view(torch.int16))
    return d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape) and torch.equal(d.cpu(), h)


def _depth_kw(depth):
    return dict(depth_camera_names=CAMS, use_depth=True) if depth else {}


def test_twins_add_no_frame_bytes(tmp_path):
    plain, _ = twin_dirs(tmp_path, lengths=(6, 5, 7), cams=CAMS, base=True)
    twins = D.mirror_twin_paths(plain)
    stats, _ = D.get_norm_stats(twins)
    files_only = D.DeviceEpisodeStore(plain, range(3), CAMS, stats, DEV)
    both = D.DeviceEpisodeStore(twins, range(6), CAMS, stats, DEV)
    alone = D.DeviceEpisodeStore(twins, [4], CAMS, stats, DEV)           # a twin whose source is not listed: the source, once
    assert both.arena.numel() == files_only.arena.numel() == both.nbytes and both.has_twins and not files_only.has_twins
    assert alone.arena.numel() == -(-5 * 105 // 256) * 256 * 3 and alone.sources == [plain[1]]
    assert both.actions.shape[0] == 2 * files_only.actions.shape[0] == 36
    assert both.device_bytes() - files_only.device_bytes() == 18 * (16 + 14) * 4 + 3 * 16
    assert both.flip.tolist() == [[0, 0, 0]] * 3 + [[1, 1, 1]] * 3
    assert np.array_equal(both.block_off[3], both.block_off[0][[0, 2, 1]])


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("hw", [(5, 7), (64, 96)])                 # the general form; the 16-byte form (depth: 8-pixel groups)
def test_store_batches_with_twins_equal_the_host_loaders_over_written_files(tmp_path, hw, depth):
    twin_dirs(tmp_path, lengths=(12, 7, 6, 5), sims=(True, False, None, True), cams=CAMS, base=True, hw=hw,
              depth_cams=CAMS if depth else ())
    kw = dict(policy_class="ACT", num_workers=0, train_ratio=0.75, **_depth_kw(depth))
    host = D.load_data(str(tmp_path / "written"), lambda n: True, CAMS, 4, 3, 5, rng=np.random.default_rng(3), **kw)
    dev = D.load_data(str(tmp_path / "plain"), lambda n: True, CAMS, 4, 3, 5, rng=np.random.default_rng(3), device_dataset=True,
                      device=DEV, mirror_twins=True, **kw)
    store = dev[0].store
    assert dev[1].store is store and store.has_twins and dev[3] == host[3] and len(store.sources) == 4 and len(store.paths) == 8
    assert store.arena.numel() == sum(-(-T * hw[0] * hw[1] * px // 256) * 256 for T in (12, 7, 6, 5) for px in [3] * 3 + [2] * 3 * depth)
    for k in host[2]:
        assert np.array_equal(host[2][k], dev[2][k]), k
    assert list(dev[0].episode_ids) == list(host[0].dataset.episode_ids) and list(dev[1].episode_ids) == list(host[1].dataset.episode_ids)
    assert sum(store.twin) == 4
    h_it, d_it = [iter(host[0]), iter(host[1])], [iter(dev[0]), iter(dev[1])]
    for which in (0, 0, 1, 0, 0, 1, 0, 0):
        hb, db = next(h_it[which]), next(d_it[which])
        assert len(hb) == len(db) == (5 if depth else 4)
        for i, (h, d) in enumerate(zip(hb, db)):
            assert d.is_cuda and _equal(d, h), (which, i, d.dtype, h.dtype, tuple(d.shape), tuple(h.shape))


@pytest.mark.parametrize("hw,depth", [((5, 7), True), ((64, 96), False)])
def test_replays_of_a_twin_equal_episode_replay_on_the_written_file(tmp_path, hw, depth):
    plain, written = twin_dirs(tmp_path, lengths=(12, 7, 6), sims=(True, False, None), cams=CAMS, base=True, hw=hw,
                               depth_cams=CAMS if depth else ())
    twins = D.mirror_twin_paths(plain, depth_follows=dict(zip(CAMS, CAMS)) if depth else None)
    stats, _ = D.get_norm_stats(twins)
    store = D.DeviceEpisodeStore(twins, [5, 0, 3, 4], CAMS, stats, DEV, **_depth_kw(depth))
    assert len(store.sources) == 3
    for eid in (3, 4, 5, 0):
        for batch, stride in ((5, 1), (2, 3)):
            host = D.EpisodeReplay(written[eid], CAMS, stats, batch, stride=stride, **_depth_kw(depth))
            dev = D.DeviceEpisodeReplay(store, eid, batch, stride=stride)
            assert (dev.T, dev.steps, dev.is_sim, len(dev)) == (host.T, host.steps, host.is_sim, len(host))
            assert dev.actions.dtype == np.float32 and np.array_equal(dev.actions, host.actions)
            hb, db = list(host), list(dev)
            assert len(hb) == len(db) == len(host)
            for h, d in zip(hb, db):
                assert len(d) == len(h) == (3 if depth else 2) and all(_equal(dt, ht) for dt, ht in zip(d, h)), (eid, batch, stride)
        steps = list(range(0, int(store.T[store._local_of[eid]]), 3))
        one = next(iter(D.EpisodeReplay(written[eid], CAMS, stats, 64, stride=3, **_depth_kw(depth))))
        assert all(_equal(d, h) for d, h in zip(store.replay_batch(store._local_of[eid], steps), one))


# ---- training fed by a store with twins ---------------------------------------------------------------------------------------------
def _policy(lr=1e-5):
    from policy import ACTPolicy
    kw = {"kl_weight": 10, "lr": lr, "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2,
          "nheads": 4, "camera_names": CAMS, "image_h": 64, "image_w": 96, "base_width": 8}      # tiny_config's sizes, three cameras
    pol = ACTPolicy(kw, max_batch=4)
    pol.train()
    return pol, kw


def _steps(loaders, replay_between=False):
    import imitate_episodes as ie
    train_dl, val_dl, stats, _ = loaders
    pol, kw = _policy()
    opt = ie.make_optimizer("ACT", pol)
    it, losses, replays = iter(train_dl), [], []
    for step in range(2):
        opt.zero_grad()
        pol.next_eps = torch.randn(2, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
        out = ie.forward_pass(next(it), pol)
        out["loss"].backward()
        opt.step()
        losses.append({k: float(v) for k, v in out.items()})
        if replay_between and step == 0:
            cfg = {"ckpt_dir": replay_between, "state_dim": 14, "policy_class": "ACT", "policy_config": dict(kw, action_dim=16),
                   "camera_names": CAMS, "episode_len": 12, "task_name": "sim_transfer_cube_scripted", "temporal_agg": True}
            pol.eval()
            replays.append(ie.replay_bc(cfg, "policy_last.ckpt", policy=pol, stats=stats, store=train_dl.store,
                                        episodes=val_dl.episode_ids, verbose=False))
            pol.train()
    pol.model.check_flags()
    return losses, replays


@pytest.fixture(scope="module")
def train_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("mirror_train")
    twin_dirs(root, lengths=(12, 9, 8), sims=(True, False, None), cams=CAMS, base=True, hw=(64, 96))
    # a seed whose validation episode (the last of the permutation of 6) is a twin (ids 3..5 of the sorted list)
    seed = next(s for s in range(50) if np.random.default_rng(s).permutation(6)[5] >= 3)
    return root, seed


def _load(root, seed, mirrored):
    kw = dict(device_dataset=True, device=DEV, mirror_twins=True) if mirrored else {}
    return D.load_data(str(root / ("plain" if mirrored else "written")), lambda n: True, CAMS, 2, 2, 8, policy_class="ACT",
                       num_workers=0, rng=np.random.default_rng(seed), **kw)


def test_training_steps_fed_by_a_mirrored_store_equal_those_fed_by_the_written_files(train_dirs):
    root, seed = train_dirs
    host, _ = _steps(_load(root, seed, False))
    dev, _ = _steps(_load(root, seed, True))
    print(f"host-fed over written twin files {host}, fed by the mirrored store {dev}")
    assert all(np.isfinite(v) for s in host for v in s.values())
    assert host == dev and host[0] != host[1]


def test_a_replay_of_a_twin_between_two_steps_leaves_training_alone(train_dirs, tmp_path):
    root, seed = train_dirs
    loaders = _load(root, seed, True)
    val_ids = list(loaders[1].episode_ids)
    assert len(val_ids) == 1 and isinstance(loaders[0].store.paths[loaders[0].store._local_of[val_ids[0]]], D.MirrorTwinPath)
    plain, _ = _steps(loaders)
    with_replay, replays = _steps(_load(root, seed, True), replay_between=str(tmp_path / "between"))
    print(f"two steps {plain}; with a replay of twin {val_ids} between them {with_replay}; replay mae {replays[0]['mae_mean']:.4f}")
    assert plain == with_replay and plain[0] != plain[1]
    assert len(replays) == 1 and replays[0]["files"] == [loaders[0].store.paths[loaders[0].store._local_of[val_ids[0]]]]
    assert os.path.basename(replays[0]["files"][0]).startswith("mirror_episode_") and np.isfinite(replays[0]["mae_mean"])
