"""Device-resident episode store on the GPU: the two gather ops against their numpy statements, the store's batches against the
host loader's from the same seed, and training steps fed either way -- everything with torch.equal, no tolerance: the ops move
bytes, and every value of the chunk gather is one fp32 subtract and one correctly rounded fp32 divide, the operations torch's CPU
kernels perform."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from test_device_dataset_cpu import write_dataset  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xCD


# ---- gather_frames -----------------------------------------------------------------------------------------------------------
def _gather_case(item, n, aligned, odd, rng, arena_np=None):
    """n items of `item` bytes from a random arena into the middle of a sentinel-filled buffer -> compared with the numpy statement;
    `odd`: sources (and the destination) at odd addresses, else at multiples of 16.  One source is named twice when n > 1."""
    if arena_np is None:
        arena_np = rng.integers(0, 256, 40 * max(item, 16) + 4096, dtype=np.uint8)
    top = arena_np.size - item
    off = rng.integers(0, top // 16, n, dtype=np.int64) * 16
    if odd:
        off = np.minimum(off + rng.integers(0, 8, n) * 2 + 1, top)
        off[0] |= 1
    if n > 1:
        off[n // 2] = off[0]
    arena = torch.from_numpy(arena_np).to(DEV)
    lead = 3 if odd else 32
    big = torch.full((lead + n * item + 61,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = big[lead:lead + n * item]
    got = ops.gather_frames(arena, torch.from_numpy(off).to(DEV), item, out=out, aligned=aligned)
    assert got.data_ptr() == out.data_ptr()
    exp = torch.from_numpy(ops.gather_frames_ref(arena_np, off, item))
    assert torch.equal(out.cpu().view(n, item), exp), (item, n, aligned, odd)
    big = big.cpu()
    assert bool((big[:lead] == SENTINEL).all()) and bool((big[lead + n * item:] == SENTINEL).all()), "bytes around out were written"
    return exp


# 105 = 5 x 7 x 3 (odd), 96 (the 16-byte form), 70 = 5 x 7 uint16, 1; 69,984 and 921,600 (= 480 x 640 x 3) take the 16-byte form's
# unrolled loop over several workgroups per item, 70,001 the general form's
@pytest.mark.parametrize("item", [105, 96, 70, 1, 69984, 70001, 921600])
@pytest.mark.parametrize("n", [1, 37])
def test_gather_frames_equals_the_numpy_statement(item, n):
    if item == 921600 and n == 37:
        n = 5
    rng = np.random.default_rng(item * 100 + n)
    _gather_case(item, n, 0, True, rng)                                # general form, odd addresses
    _gather_case(item, n, 0, False, rng)
    if item % 16 == 0:
        _gather_case(item, n, 1, False, rng)                           # 16-byte loads and stores
        _gather_case(item, n, 2, False, rng)                           # the same with non-temporal loads
        # the flag is the caller's statement; an offset that breaks it is still copied right (the kernel looks at it)
        arena_np = rng.integers(0, 256, 40 * item + 4096, dtype=np.uint8)
        arena = torch.from_numpy(arena_np).to(DEV)
        off = np.array([16, 5, 32 + 9, 16][:max(1, min(n, 4))], dtype=np.int64)
        got = ops.gather_frames(arena, torch.from_numpy(off).to(DEV), item, aligned=1)
        assert torch.equal(got.cpu(), torch.from_numpy(ops.gather_frames_ref(arena_np, off, item)))


def test_gather_frames_zero_fills_an_item_that_leaves_the_arena_and_refuses_bad_arguments():
    arena_np = np.arange(1, 1 + 960, dtype=np.int64).astype(np.uint8)
    arena = torch.from_numpy(arena_np).to(DEV)
    for item, aligned, off in ((96, 1, [0, 880, 864, -16, 1 << 40]), (105, 0, [3, 856, 855, -1, 1 << 40])):
        got = ops.gather_frames(arena, torch.tensor(off, dtype=torch.int64, device=DEV), item, aligned=aligned).cpu()
        exp = torch.from_numpy(ops.gather_frames_ref(arena_np, off, item))
        assert torch.equal(got, exp) and not bool(got[3].any()) and not bool(got[4].any()) and bool(got[2].all())
    with pytest.raises(RuntimeError, match="multiples of 16"):
        ops.gather_frames(arena, torch.zeros(2, dtype=torch.int64, device=DEV), 100, aligned=1)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        ops.gather_frames(arena[8:], torch.zeros(2, dtype=torch.int64, device=DEV), 96, aligned=1)
    with pytest.raises(ValueError):
        ops.gather_frames(arena, torch.zeros(2, dtype=torch.int32, device=DEV), 96)


def test_gather_frames_offsets_beyond_4_gib():
    """an uninitialised arena of about 4.5 GiB, two frames written, one of them past the 4 GiB mark: 32-bit offset arithmetic
    would read the wrong place"""
    total = (9 << 29) + 4096
    arena = torch.empty(total, dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(5)
    for item, aligned, offs in ((96, 1, [16, (1 << 32) + 4096 + 16]), (105, 0, [(1 << 32) + 5, 7])):
        frames = [torch.from_numpy(rng.integers(0, 256, item, dtype=np.uint8)) for _ in offs]
        arena[offs[0] & 0xFFFFFFFF:(offs[0] & 0xFFFFFFFF) + item] = 0          # where a 32-bit offset would land
        arena[offs[1] & 0xFFFFFFFF:(offs[1] & 0xFFFFFFFF) + item] = 0
        for o, f in zip(offs, frames):
            arena[o:o + item] = f.to(DEV)
        got = ops.gather_frames(arena, torch.tensor(offs + offs[:1], dtype=torch.int64, device=DEV), item, aligned=aligned).cpu()
        assert torch.equal(got[0], frames[0]) and torch.equal(got[1], frames[1]) and torch.equal(got[2], frames[0])
    del arena
    torch.cuda.empty_cache()


# ---- gather_chunks -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_tables():
    """episodes of 3, 7 and 12 steps, a real one between two sim ones, 16 action columns (14 + /base_action's 2), stats whose
    means are far from zero"""
    rng = np.random.default_rng(11)
    T = [3, 7, 12]
    rec = np.zeros(3, dtype=ops.episode_rec_dtype())
    rec["row0"], rec["T"], rec["is_sim"] = [0, 3, 10], T, [1, 0, 1]
    actions = (rng.standard_normal((22, 16)) * 3 - 0.5).astype(np.float32)
    qpos = (rng.standard_normal((22, 14)) * 2 + 1).astype(np.float32)
    stats = [(rng.standard_normal(16) + 2).astype(np.float32), (rng.random(16) + 0.05).astype(np.float32),
             (rng.standard_normal(14) - 3).astype(np.float32), (rng.random(14) + 0.05).astype(np.float32)]
    samples = np.array([(e, t) for e in range(3) for t in range(T[e])] + [(1, 0), (2, 11), (0, 2)], dtype=np.int32)
    return rec, actions, qpos, stats, samples


@pytest.mark.parametrize("Q", [5, 12, 1])                      # 12: the chunk clipped to the longest episode
def test_gather_chunks_equals_the_numpy_statement_and_torch_on_the_host(chunk_tables, Q):
    rec, actions, qpos, stats, samples = chunk_tables
    dev = [torch.from_numpy(x).to(DEV) for x in (actions, qpos, rec.view(np.uint8).copy(), samples, *stats)]
    q, a, pad = ops.gather_chunks(*dev, Q)
    eq, ea, epad = ops.gather_chunks_ref(actions, qpos, rec, samples, *stats, Q)
    assert q.dtype == torch.float32 and a.dtype == torch.float32 and pad.dtype == torch.bool
    assert torch.equal(q.cpu(), torch.from_numpy(eq)) and torch.equal(a.cpu(), torch.from_numpy(ea))
    assert torch.equal(pad.cpu(), torch.from_numpy(epad))
    # the dataset's own expressions, in torch on the host, for the edge samples
    am, asd, qm, qsd = (torch.from_numpy(s) for s in stats)
    for b, (e, t) in enumerate(samples.tolist()):
        row0, T, sim = int(rec["row0"][e]), int(rec["T"][e]), bool(rec["is_sim"][e])
        s = t if sim else max(0, t - 1)
        padded = np.zeros((12, 16), dtype=np.float32)
        padded[:T - s] = actions[row0 + s:row0 + T]
        assert torch.equal(a[b].cpu(), (torch.from_numpy(padded[:Q]).float() - am) / asd), (e, t)
        assert torch.equal(q[b].cpu(), (torch.from_numpy(qpos[row0 + t]).float() - qm) / qsd), (e, t)
        assert pad[b].cpu().tolist() == [j >= T - s for j in range(Q)]
    # padded rows are -mean / std, not 0; the real episode at t = 0 starts at its row 0, at t = 1 too
    last = samples.tolist().index([2, 11])
    if Q > 1:
        assert torch.equal(a[last, 1].cpu(), (torch.zeros(16) - am) / asd) and bool((a[last, 1] != 0).all()) and bool(pad[last, 1])
    assert torch.equal(a[samples.tolist().index([1, 0])], a[samples.tolist().index([1, 1])])


def test_gather_chunks_holds_wild_table_entries_inside_the_arrays(chunk_tables):
    rec, actions, qpos, stats, _ = chunk_tables
    samples = np.array([(7, 2), (-1, 0), (1, 99), (2, -5)], dtype=np.int32)
    dev = [torch.from_numpy(x).to(DEV) for x in (actions, qpos, rec.view(np.uint8).copy(), samples, *stats)]
    q, a, pad = ops.gather_chunks(*dev, 5)
    held = np.array([(2, 2), (0, 0), (1, 6), (2, 0)], dtype=np.int32)
    eq, ea, epad = ops.gather_chunks_ref(actions, qpos, rec, held, *stats, 5)
    assert torch.equal(q.cpu(), torch.from_numpy(eq)) and torch.equal(a.cpu(), torch.from_numpy(ea)) and torch.equal(pad.cpu(), torch.from_numpy(epad))


# ---- the store against the host loader ------------------------------------------------------------------------------------------
def _both_paths(dirpath, cams, chunk, seed=3, **kw):
    host = D.load_data(str(dirpath), lambda n: True, cams, 4, 3, chunk, policy_class="ACT", num_workers=0,
                       rng=np.random.default_rng(seed), **kw)
    dev = D.load_data(str(dirpath), lambda n: True, cams, 4, 3, chunk, policy_class="ACT", num_workers=0,
                      rng=np.random.default_rng(seed), device_dataset=True, device=DEV, **kw)
    assert getattr(dev[0], "on_device", False) and getattr(dev[1], "on_device", False) and not hasattr(host[0], "on_device")
    assert dev[0].store is dev[1].store and dev[3] == host[3]
    for k in host[2]:
        assert np.array_equal(host[2][k], dev[2][k])
    return host, dev


def _compare_interleaved(host, dev, entries):
    h_it, d_it = [iter(host[0]), iter(host[1])], [iter(dev[0]), iter(dev[1])]
    for which in (0, 0, 1, 0, 0, 1, 0, 0):                            # 6 training and 2 validation batches, interleaved
        hb, db = next(h_it[which]), next(d_it[which])
        assert len(hb) == len(db) == entries
        for i, (h, d) in enumerate(zip(hb, db)):
            assert d.is_cuda and d.dtype == h.dtype and tuple(d.shape) == tuple(h.shape), (which, i, d.dtype, h.dtype, d.shape, h.shape)
            assert torch.equal(d.cpu(), h), (which, i)


@pytest.mark.parametrize("hw", [(5, 7), (4, 8)])               # 105-byte frames: the general form; 96: the 16-byte form
@pytest.mark.parametrize("chunk", [4, 50])                     # 50: clipped to each loader's longest episode
def test_store_batches_equal_the_host_loaders(tmp_path, hw, chunk):
    cams = ["top", "wrist"]
    write_dataset(tmp_path, lengths=(12, 7, 3), cams=cams, hw=hw)
    host, dev = _both_paths(tmp_path, cams, chunk)
    store = dev[0].store
    assert store.aligned == (1 if hw == (4, 8) else 0) and np.all(store.block_off % 256 == 0)
    assert store.device_bytes() >= store.nbytes == store.arena.numel()
    _compare_interleaved(host, dev, 4)


def test_store_batches_with_raw_depth_equal_the_host_loaders(tmp_path):
    cams = ["top", "wrist"]
    write_dataset(tmp_path, lengths=(12, 7, 3), cams=cams, depth_cams=cams)
    host, dev = _both_paths(tmp_path, cams, 4, depth_camera_names=cams, use_depth=True)
    _compare_interleaved(host, dev, 5)
    assert next(iter(dev[0]))[4].dtype == torch.uint16


def test_store_batches_of_a_compressed_dataset_equal_the_host_loaders(tmp_path):
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("PIL is not installed: compressed episodes cannot be written or decoded")
    cams = ["top", "wrist"]
    write_dataset(tmp_path, lengths=(6, 4, 3), cams=cams, hw=(8, 12), compress=True)
    host, dev = _both_paths(tmp_path, cams, 4)
    assert all(dev[0].store.compressed)
    _compare_interleaved(host, dev, 4)


def test_store_budget_and_membership_checks_on_the_device(tmp_path):
    cams = ["top"]
    paths = write_dataset(tmp_path, cams=cams)
    stats, lens = D.get_norm_stats(paths)
    store = D.DeviceEpisodeStore(paths, [2, 0], cams, stats, DEV)       # default budget: free memory minus the reserve
    assert store.budget_bytes > store.nbytes and store.episode_ids == [2, 0]
    with pytest.raises(ValueError, match="not in the store"):
        store.loader([1], [lens[1]], 4, iter([[0]]))
    with pytest.raises(ValueError, match="episode_len"):
        store.loader([0], [lens[0] + 1], 4, iter([[0]]))
    with pytest.raises(IndexError):
        store.gather([0], [3], 4)                                      # episode 2 has 3 steps
    ld = store.loader([0, 2], [lens[0], lens[2]], 4, iter([[0, 11, 12, 14]]))
    img, qpos, act, pad = next(ld)
    assert tuple(img.shape) == (4, 1, 5, 7, 3) and tuple(act.shape) == (4, 4, 16)
    with pytest.raises(StopIteration):
        next(ld)


# ---- training fed by the store ---------------------------------------------------------------------------------------------------
def _policy():
    from policy import ACTPolicy
    kw = {"kl_weight": 10, "lr": 1e-5, "num_queries": 8, "hidden_dim": 64, "dim_feedforward": 128, "enc_layers": 2, "dec_layers": 2,
          "nheads": 4, "camera_names": ["a", "b"], "image_h": 64, "image_w": 96, "base_width": 8}      # tiny_config's sizes
    pol = ACTPolicy(kw, max_batch=2)
    pol.train()
    return pol


@pytest.mark.parametrize("augment", [False, True])
def test_training_steps_fed_by_the_store_equal_those_fed_by_the_host_loader(tmp_path, augment):
    import imitate_episodes as ie
    cams = ["a", "b"]
    write_dataset(tmp_path, lengths=(12, 9, 8), cams=cams, hw=(64, 96))
    losses = []
    for device_dataset in (False, True):
        train_dl, _val, _stats, _ = D.load_data(str(tmp_path), lambda n: True, cams, 2, 2, 8, policy_class="ACT", num_workers=0,
                                                rng=np.random.default_rng(7), device_dataset=device_dataset,
                                                device=DEV if device_dataset else None)
        pol = _policy()
        opt = ie.make_optimizer("ACT", pol)
        aug = ie.make_augment({"augment_images": augment}, pol, seed=4)
        assert (aug is not None) == augment
        it, steps = iter(train_dl), []
        for step in range(2):
            opt.zero_grad()
            pol.next_eps = torch.randn(2, pol.model.cfg.latent_in_dim, generator=torch.Generator().manual_seed(20 + step)).to(DEV)
            out = ie.forward_pass(next(it), pol, aug)
            out["loss"].backward()
            opt.step()
            steps.append({k: float(v) for k, v in out.items()})
        pol.model.check_flags()
        losses.append(steps)
    print(f"augment={augment}: host-fed {losses[0]}, store-fed {losses[1]}")
    assert all(np.isfinite(v) for s in losses[0] for v in s.values())
    assert losses[0] == losses[1]
    assert losses[0][0] != losses[0][1]                                # two different batches, and the weights moved
