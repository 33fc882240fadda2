"""Nearest-neighbour retrieval (the VINN baseline), the parts that need no GPU: the numpy statements of the three ops against plain
float64, against the fixture made by the reference's own ``calculate_nearest_neighbors`` (tools/gen_golden_vinn.py), the
refusals, the C boundary, and replay_bc's host logic with CPU stand-ins.

Bars.  Distances of ``knn_topk_ref`` against float64: a sum of D squares in fp32 is within (D / 4 + 3) * 2^-24 relative in the
4-way order, the square root halves that, the sum of two norms adds one rounding: (D / 4 + 5) * 2^-24 relative is a bound, not a
measurement.  Against the fixture: the prediction is no further from the float64 statement than 2 x ref_vs_f64 (the gap the
reference's own fp32 torch result leaves, stored in the fixture per case; the margin covers two fp32 evaluations that differ in
their summation order only), with a floor of 1e-6 * max|target|.  Measured when the fixture was written: ref_vs_f64 between 0
(k = 1) and 4.2e-7; this path's distance 0 (k = 1) to 2.3e-7."""
import os

import numpy as np
import pytest
import torch

import imitate_episodes as IE
from actmi import lib as L
from actmi import ops
from test_replay_cpu import A, CAMS, Q, StubPolicy, _config, make_stats
from test_replay_store_cpu import HostStore, KEYS_TODAY, _args, _dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["actmi_bind_features_out", "actmi_op_knn_workspace_bytes", "actmi_op_knn_topk", "actmi_op_knn_predict",
               "actmi_op_knn_ksweep"]


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    declared = L.declared_symbols(os.path.join(ROOT, "include", "actmi.h"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert lib.actmi_op_knn_workspace_bytes(1, 16384) == 16384 * 4
    assert lib.actmi_op_knn_workspace_bytes(4000, 16384) == 1024 * 16384 * 4
    assert lib.actmi_op_knn_workspace_bytes(0, 5) == 0
    # refused at the boundary before anything could be launched
    assert lib.actmi_op_knn_topk(None, None, None, None, None, None, 1.0, 1, 1, 1, 1, 0, None, None, None, None, 0, None) != 0
    assert b"knn_topk" in lib.actmi_op_last_error()
    assert lib.actmi_op_knn_predict(None, None, None, 1, 1, None, 1, None, None, 1, 1, 1, None, None, None, None, 1, None) != 0
    assert lib.actmi_op_knn_ksweep(None, None, None, 1, None, 1, None, 1, 1, None, None, None, None, None, 1, None) != 0
    assert lib.actmi_bind_features_out(None, None, 0) != 0


# ---- the numpy statements against plain float64 -----------------------------------------------------------------------------
def _case(seed, Nq=5, Ns=60, Dv=70, S=14):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((Nq, Dv)).astype(np.float32), rng.standard_normal((Nq, S)).astype(np.float32),
            rng.standard_normal((Ns, Dv)).astype(np.float32), rng.standard_normal((Ns, S)).astype(np.float32))


def _d64(qv, qs, sv, ss, w):
    d = np.linalg.norm(qv[:, None].astype(np.float64) - sv[None].astype(np.float64), axis=2)
    if qs is not None and qs.shape[1]:
        d = d + w * np.linalg.norm(qs[:, None].astype(np.float64) - ss[None].astype(np.float64), axis=2)
    return d


@pytest.mark.parametrize("Dv,S,w", [(1, 0, 1.0), (3, 3, 0.0), (70, 14, 0.75), (512, 14, 5.0)])
def test_topk_ref_against_float64(Dv, S, w):
    qv, qs, sv, ss = _case(Dv + S, Dv=Dv, S=S)
    K = 9
    idx, dist, n = ops.knn_topk_ref(qv, qs, sv, ss, K, w)
    d = _d64(qv, qs, sv, ss, w)
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and n.dtype == np.int32 and np.all(n == K)
    bound = (max(Dv, S) / 4 + 5) * 2.0 ** -24
    for q in range(len(qv)):
        exact = d[q, idx[q]]
        assert np.all(np.abs(dist[q] - exact) <= bound * exact)
        assert np.all(np.diff(dist[q].astype(np.float64)) >= 0)
        # the set is the float64 one wherever float64 separates the K-th from the (K+1)-th by more than the bound
        order = np.argsort(d[q], kind="stable")
        if d[q, order[K]] - d[q, order[K - 1]] > 2 * bound * d[q, order[K]]:
            assert set(idx[q].tolist()) == set(order[:K].tolist())


def test_topk_ref_ties_exclusion_and_non_finite_rows():
    qv, qs, sv, ss = _case(3, Ns=40)
    sv[30:35], ss[30:35] = sv[2:7], ss[2:7]
    sv[8, 1], ss[9, 0] = np.nan, np.inf
    sep = (np.arange(40) // 10).astype(np.int32)
    exclude = np.array([1, -1, 3, -1, 0], dtype=np.int32)
    idx, dist, n = ops.knn_topk_ref(qv, qs, sv, ss, 40, 1.0, sep, exclude)
    for q in range(5):
        got = idx[q, :n[q]].tolist()
        assert 8 not in got and 9 not in got and -1 not in got
        if exclude[q] >= 0:
            assert not (set(got) & set(range(10 * exclude[q], 10 * exclude[q] + 10)))
        for s in range(2, 7):
            if s in got and s + 28 in got:
                assert got[got.index(s) + 1] == s + 28 and dist[q, got.index(s)] == dist[q, got.index(s) + 1]
        assert np.all(idx[q, n[q]:] == -1) and np.all(np.isinf(dist[q, n[q]:]))
    assert n.tolist() == [28, 38, 28, 38, 30]                    # (episode 0 holds the two non-finite rows)
    idx, dist, n = ops.knn_topk_ref(qv, qs, sv, ss, 4, 1.0, np.zeros(40, np.int32), np.zeros(5, np.int32))
    assert not n.any() and np.all(idx == -1) and np.all(np.isinf(dist))


def _rows(seed=4, Nq=6, K=7, R=50, Qn=5, An=3):
    rng = np.random.default_rng(seed)
    actions = rng.standard_normal((R, An)).astype(np.float32)
    off = rng.integers(0, R - 1, 30).astype(np.int64)
    left = np.minimum(rng.integers(1, Qn + 6, 30), R - off).astype(np.int32)
    idx = rng.integers(0, 30, (Nq, K)).astype(np.int32)
    dist = np.sort(rng.random((Nq, K)).astype(np.float32) * 4, axis=1)
    n = np.array([K, K, 3, 0, K, 1], dtype=np.int32)
    return actions, off, left, idx, dist, n, rng.standard_normal(An), rng.random(An) + 0.5


@pytest.mark.parametrize("stats", [False, True])
def test_predict_ref_against_a_plain_statement(stats):
    actions, off, left, idx, dist, n, mean, std = _rows()
    Qn = 5
    for k in (1, 4, 7):
        got, empty = ops.knn_predict_ref(idx, dist, n, k, actions, off, left, Qn, *((mean, std) if stats else (None, None)))
        assert got.dtype == np.float32 and empty == 1 and not got[3].any()
        for q in (0, 1, 2, 4, 5):
            m = min(k, n[q])
            wts = torch.softmax(-torch.from_numpy(dist[q, :m].astype(np.float64)), dim=0).numpy()
            chunk = np.zeros((Qn, actions.shape[1]))
            for i in range(m):
                s = idx[q, i]
                chunk += wts[i] * actions[off[s] + np.minimum(np.arange(Qn), left[s] - 1)].astype(np.float64)
            if stats:
                chunk = (chunk - mean) / std
            assert np.allclose(got[q], chunk, rtol=2.0 ** -23, atol=1e-12)


@pytest.mark.parametrize("stats", [False, True])
def test_ksweep_ref_is_predict_ref_at_every_k(stats):
    actions, off, left, idx, dist, n, mean, std = _rows()
    ms = (mean, std) if stats else (None, None)
    target = np.random.default_rng(9).standard_normal((6, 3)).astype(np.float32)
    sse, part = ops.knn_ksweep_ref(idx, dist, n, actions, off, target, *ms, want_partial=True)
    assert sse.shape == (7,) and part.shape == (6, 7)
    for k in range(1, 8):
        pred, _ = ops.knn_predict_ref(idx, dist, n, k, actions, off, left, 4, *ms)
        d = pred[:, 0].astype(np.float64) - target.astype(np.float64)
        want = np.zeros(6)
        for a in range(3):
            want = want + d[:, a] * d[:, a]
        assert np.array_equal(part[:, k - 1], want), k               # query by query, the same bits
        total = 0.0
        for q in range(6):
            total = total + want[q]
        assert sse[k - 1] == total


def test_pooled_features_ref():
    rng = np.random.default_rng(0)
    C_, B, fh, fw, F = 2, 3, 2, 3, 8
    m = rng.standard_normal((C_, B, fh, fw, F)).astype(np.float32)
    got = ops.pooled_features_ref(m.reshape(-1), B, C_, fh, fw)
    assert got.shape == (B, C_ * F) and got.dtype == np.float32
    want = m.astype(np.float64).mean(axis=(2, 3)).transpose(1, 0, 2).reshape(B, -1)
    assert np.allclose(got, want, rtol=0, atol=8 * 2.0 ** -24 * np.abs(m).max())


# ---- the fixture from the reference's own function ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "vinn_knn.npz"))


@pytest.mark.parametrize("wi", [0, 1])
def test_fixture_selected_sets_and_prediction(golden, wi):
    z = golden
    w = float(z["weights"][wi])
    t = f"w{wi}"
    qv, qs, sv, ss, targets = (z[f"{t}_{n}"] for n in ("qv", "qs", "sv", "ss", "targets"))
    Ns, skip, An = targets.shape
    rel = np.diff(z[f"{t}_d64"]) / z[f"{t}_d64"][1:]
    assert rel.min() >= 1e-3                                         # the fixture's own promise: the order is beyond fp32 doubt
    for k in (int(v) for v in z["ks"]):
        idx, dist, n = ops.knn_topk_ref(qv, qs, sv, ss, k, w)
        # the support rows are stored sorted, so the reference's first k rows ARE its k nearest: the selected set, in order
        assert idx.tolist() == [list(range(k))] and n.tolist() == [k]
        for form in ("flat", "chunk"):
            ref, exact, gap = z[f"{t}_k{k}_{form}_ref"], z[f"{t}_k{k}_{form}_f64"], float(z[f"{t}_k{k}_{form}_gap"])
            if form == "flat":                                       # one action per support row
                actions, off, left, Qn = targets[:, 0].copy(), np.arange(Ns), np.ones(Ns, np.int32), 1
            else:                                                    # a chunk of `skip` rows per support row
                actions, off, left, Qn = targets.reshape(Ns * skip, An), np.arange(Ns) * skip, np.full(Ns, skip, np.int32), skip
            got, empty = ops.knn_predict_ref(idx, dist, n, k, actions, off, left, Qn)
            got = got.reshape(exact.shape)
            err = float(np.abs(got.astype(np.float64) - exact).max())
            bound = max(2 * gap, 1e-6 * float(np.abs(targets).max()))
            print(f"w = {w}, k = {k}, {form}: |ours - f64| = {err:.3e}, ref_vs_f64 = {gap:.3e}, bound {bound:.3e}, "
                  f"|ours - ref| = {float(np.abs(got - ref).max()):.3e}")
            assert empty == 0 and err <= bound


# ---- refusals -------------------------------------------------------------------------------------------------------------------
class _Store:
    episode_ids = [0, 1, 2]
    _local_of = {0: 0, 1: 1, 2: 2}
    T = np.array([4, 5, 6])


def test_replay_knn_refusals_before_any_launch():
    pc = {"num_queries": Q, "action_dim": A}
    ok = IE.check_replay_knn({"k": 3}, _Store(), "ACT", pc, [2])
    assert ok["support_ids"] == [0, 1] and ok["support_rows"] == 9 and ok["state_weight"] == 1.0 and ok["exclude_self"] is False
    assert IE.check_replay_knn(3, _Store(), "ACT", pc, None)["exclude_self"] is True          # nothing beyond the replayed: all
    with pytest.raises(ValueError, match="device_dataset"):
        IE.check_replay_knn({"k": 3}, None, "ACT", pc)
    for k in (0, 513, -1, 2.5, 10):                                  # 10 > the 9 support rows
        with pytest.raises(ValueError, match="K"):
            IE.check_replay_knn({"k": k}, _Store(), "ACT", pc, [2])
    for w in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="state_weight"):
            IE.check_replay_knn({"k": 3, "state_weight": w}, _Store(), "ACT", pc, [2])
    with pytest.raises(ValueError, match="use_pcd"):
        IE.check_replay_knn({"k": 3}, _Store(), "ACT", dict(pc, use_pcd=True), [2])
    with pytest.raises(ValueError, match="Diffusion"):
        IE.check_replay_knn({"k": 3}, _Store(), "Diffusion", pc, [2])
    with pytest.raises(ValueError, match="not in the store"):
        IE.check_replay_knn({"k": 3, "support_ids": [7]}, _Store(), "ACT", pc, [2])
    with pytest.raises(ValueError, match="K"):
        IE.check_replay_knn({"k": 3, "select_k": 600}, _Store(), "ACT", pc, [2])
    # replay_bc raises them before it loads a policy or touches a file
    with pytest.raises(ValueError, match="device_dataset"):
        IE.replay_bc({"ckpt_dir": "/nonexistent", "policy_class": "ACT", "policy_config": pc}, "policy_last.ckpt", knn={"k": 3})
    with pytest.raises(ValueError, match="Diffusion"):
        IE.replay_bc({"ckpt_dir": "/nonexistent", "policy_class": "Diffusion", "policy_config": pc}, "x", knn=3, store=_Store())


def test_cli_flags_and_refusals():
    plain = IE.build_config(_args("--eval --replay"))
    assert "replay_knn" not in plain
    cfg = IE.build_config(_args("--eval --replay --device_dataset --replay_knn 5"))
    assert cfg["replay_knn"] == {"k": 5, "state_weight": 1.0}
    cfg = IE.build_config(_args("--eval --replay --device_dataset --replay_knn 5 --knn_state_weight 0 --knn_select_k 40"))
    assert cfg["replay_knn"] == {"k": 5, "state_weight": 0.0, "select_k": 40}
    for extra, what in (("--eval --replay --replay_knn 5", "device_dataset"),
                        ("--device_dataset --replay_every 10 --replay_knn 5", "replay_every"),
                        ("--device_dataset --replay_knn 5", "--eval --replay"),
                        ("--eval --replay --device_dataset --replay_knn 0", "K"),
                        ("--eval --replay --device_dataset --replay_knn 513", "K"),
                        ("--eval --replay --device_dataset --replay_knn 5 --knn_state_weight -1", "state_weight"),
                        ("--eval --replay --device_dataset --replay_knn 5 --knn_state_weight nan", "state_weight"),
                        ("--eval --replay --device_dataset --replay_knn 5 --knn_select_k 1000", "K"),
                        ("--eval --replay --device_dataset --knn_state_weight 2", "replay_knn"),
                        ("--eval --replay --device_dataset --knn_select_k 9", "replay_knn")):
        with pytest.raises(ValueError, match=what):
            IE.build_config(_args(extra))
    with pytest.raises(ValueError, match="Diffusion"):
        IE.build_config(_args("--eval --replay --device_dataset --replay_knn 5", policy_class="Diffusion"))
    from actmi.constants import SIM_TASK_CONFIGS
    SIM_TASK_CONFIGS["vinn_pcd_task"] = dict(SIM_TASK_CONFIGS["sim_transfer_cube_scripted"], pointcloud_names=["fused"])
    try:
        with pytest.raises(ValueError, match="use_pcd"):
            IE.build_config(_args("--eval --replay --device_dataset --device_clouds --use_pcd --replay_knn 5", task_name="vinn_pcd_task"))
    finally:
        del SIM_TASK_CONFIGS["vinn_pcd_task"]


# ---- replay_bc with CPU stand-ins -------------------------------------------------------------------------------------------------
class StubNeighbours(StubPolicy):
    """a stand-in for VINNPolicy: another known function of (qpos, slot), counting its empty lookups"""

    def __call__(self, qpos, image):
        return super().__call__(qpos, image) * 0.5 - 0.25

    def empty_count(self):
        return 2


@pytest.mark.parametrize("temporal_agg", [True, False])
def test_replay_bc_keeps_every_existing_bit_beside_the_baseline(tmp_path, host_only, temporal_agg, capsys):
    import json
    data, paths, eps = _dataset(tmp_path)
    stats = make_stats()

    def run(name, **kw):
        store = HostStore(paths, [2, 0, 1], stats)
        res = IE.replay_bc(_config(tmp_path / name, data, temporal_agg), "policy_last.ckpt", policy=StubPolicy(), stats=stats, batch=3,
                           episode_ensemble=ops.episode_ensemble_ref, action_error=ops.action_error_ref, store=store,
                           episodes=[0, 1], verbose=True, **kw)
        return res, capsys.readouterr().out

    plain, out_plain = run("plain")
    nb = StubNeighbours()
    both, out_both = run("knn", knn={"k": 2, "state_weight": 0.5, "policy": nb})
    assert set(plain) == KEYS_TODAY and set(both) == KEYS_TODAY | {"knn"}
    assert json.dumps({k: both[k] for k in plain}) == json.dumps(plain)          # every pre-existing key, bit for bit
    kn = both["knn"]
    assert set(kn) == {"k", "state_weight", "support_rows", "mae_mean", "rmse_mean", "max_max", "mae", "empty"}
    assert (kn["k"], kn["state_weight"], kn["support_rows"], kn["empty"]) == (2, 0.5, 9, 2)          # episode 2 of 9 steps supports
    # the baseline's figures are those of a plain replay of the stand-in
    alone = IE.replay_bc(_config(tmp_path / "alone", data, temporal_agg), "policy_last.ckpt", policy=StubNeighbours(), stats=stats,
                         batch=3, episode_ensemble=ops.episode_ensemble_ref, action_error=ops.action_error_ref,
                         store=HostStore(paths, [2, 0, 1], stats), episodes=[0, 1], verbose=False, save_episode=False)
    assert kn["mae"] == alone["mae"] and kn["mae_mean"] == alone["mae_mean"] and kn["max_max"] == alone["max_max"]
    assert kn["mae_mean"] != plain["mae_mean"]
    # files: the per-episode files are the same bytes' worth, the JSON gains the one key
    for i in range(2):
        a, b = np.load(tmp_path / "plain" / f"replay_policy_last_ep{i}.npz"), np.load(tmp_path / "knn" / f"replay_policy_last_ep{i}.npz")
        assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["target"], b["target"])
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "knn"))
    with open(tmp_path / "knn" / "replay_policy_last.json") as f:
        assert json.load(f)["knn"] == kn
    # printed: what was printed before, and one more line with the two MAEs and their ratio
    extra = [ln for ln in out_both.splitlines() if ln not in out_plain.splitlines() and "frames/s" not in ln]       # (a wall-clock rate)
    assert len(extra) == 1 and "kNN MAE" in extra[0] and "ratio" in extra[0] and f"{plain['mae_mean']:.5f}" in extra[0]


# ---- the command line's path through main() ------------------------------------------------------------------------------------
class _Loader:
    def __init__(self, store, ids):
        self.store, self.episode_ids = store, ids


def test_main_replays_the_validation_split_with_the_training_split_as_support(monkeypatch, tmp_path):
    """--eval --replay --device_dataset --replay_knn: main() loads the store training would hold, replays its validation episodes
    and names the training episodes as the support set"""
    store, stats, seen, loaded = object(), {"action_mean": [0.0]}, {}, {}

    def fake_load(args, config, task_config, dataset_dir, world, local_rank):
        loaded.update(dataset_dir=dataset_dir, device_dataset=config.get("device_dataset"))
        return _Loader(store, [4, 0, 2]), _Loader(store, [3, 1]), stats, True

    monkeypatch.setattr(IE, "_load_episode_data", fake_load)
    monkeypatch.setattr(IE, "replay_bc", lambda config, ckpt, **kw: seen.update(kw) or "done")
    data = tmp_path / "data"
    data.mkdir()
    base = "--eval --replay --device_dataset --replay_knn 3 --knn_state_weight 0.5 --knn_select_k 9"
    assert IE.main(_args(base, ckpt_dir=str(tmp_path / "ck"), dataset_dir=str(data))) == "done"
    assert loaded == {"dataset_dir": str(data), "device_dataset": True}
    assert seen["store"] is store and seen["stats"] is stats and seen["episodes"] == [3, 1] and seen["save_episode"] is True
    assert seen["knn"] == {"k": 3, "state_weight": 0.5, "select_k": 9, "support_ids": [4, 0, 2]}
    IE.main(_args(base + " --replay_episodes 1", ckpt_dir=str(tmp_path / "ck"), dataset_dir=str(data)))
    assert seen["episodes"] == [3]
    with pytest.raises(ValueError, match="dataset_dir"):
        IE.main(_args(base, ckpt_dir=str(tmp_path / "ck"), dataset_dir=str(tmp_path / "missing")))
    # without the flag main() calls the replay as it always did: no store, no knn
    seen.clear()
    IE.main(_args("--eval --replay", ckpt_dir=str(tmp_path / "ck")))
    assert "knn" not in seen and "store" not in seen


def test_load_episode_data_hands_load_data_the_runs_settings(monkeypatch, tmp_path):
    from actmi import data as D
    got = {}

    def fake(dataset_dir, name_filter, camera_names, bs_train, bs_val, chunk, skip, **kw):
        got.update(kw, dataset_dir=dataset_dir, camera_names=camera_names, chunk=chunk, bs=(bs_train, bs_val))
        return "train", "val", "stats", True

    monkeypatch.setattr(D, "load_data", fake)
    args = _args("--eval --replay --device_dataset --replay_knn 3")
    cfg = IE.build_config(args)
    from actmi.constants import SIM_TASK_CONFIGS
    out = IE._load_episode_data(args, cfg, SIM_TASK_CONFIGS[args["task_name"]], str(tmp_path), 1, 0)
    assert out == ("train", "val", "stats", True)
    assert got["device_dataset"] is True and got["policy_class"] == "ACT" and got["use_pcd"] is False and got["use_depth"] is False
    assert got["dataset_dir"] == str(tmp_path) and got["camera_names"] == cfg["camera_names"] and got["device"] is None
    assert got["bs"] == (args["batch_size"], args["batch_size"]) and got["chunk"] == args["chunk_size"]
