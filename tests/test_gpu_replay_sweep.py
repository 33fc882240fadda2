"""Replay schedule sweep on the GPU: ops.ensemble_sweep against ops.episode_ensemble on the masked table (bit for bit), the
latest-chunk schedule against the gather, both against the numpy statement; ops.sweep_error against ops.action_error per schedule
(bit for bit) and the roughness against numpy; replay_bc(sweep=...) end to end on the tiny fixture policy.

Bars.  torch.equal between an ensemble schedule (f, h, k) and episode_ensemble with weight k on the table whose dead entries
(r % f != 0 or slot >= h) are zeroed is derived, not measured: both kernels run ensemble_step_rows (csrc/ensemble_core.h), a dead
row and a zero row both get pop = false, so the same rows take the same ranks and enter the same sums in the same order.
torch.equal between rows 0-2 of sweep_error and action_error on raw[g]: the same thread shape, walk and unfused arithmetic.
1e-13 against numpy float64: the bar of tests/test_gpu_replay.py for this arithmetic on unit-scale rows (it includes the 300-row
shape).  Roughness: |got - exp| <= 1e-12 * sum |term| covers any summation order of up to 4097 float64 terms
(tests/test_gpu_replay.py).  End to end: rtol 1e-12, the summation-order bar of the pooled figures there."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import imitate_episodes as IE  # noqa: E402
from actmi import ops  # noqa: E402
from actmi.config import tiny_config  # noqa: E402

DEV = "cuda"

# (T, Q, A, len)
CASES = [(37, 10, 16, 37),                 # the base case
         (5, 10, 14, 5),                   # T < Q, every = Q larger than T
         (310, 300, 33, 301),              # second 256-row pass, per = 64, ragged
         (20, 6, 64, 0),                   # an empty episode
         (1, 4, 7, 1)]                     # a single step
IDS = [str(c) for c in CASES]


def planted_chunks(T, Q, A, seed):
    """the zeros of tests/test_gpu_replay.py for one episode: one element of the only row of t = 0 (an empty step), one element
    of a later row, a whole newest row"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((T, Q, A)).astype(np.float32)
    c[0, 0, A // 2] = 0.0
    if T > 4 and Q > 2:
        c[3, 2, A - 1] = 0.0
    if T > 2:
        c[T // 2, 0, :] = 0.0
    return c


def grid(Q):
    """every in {1, 3, Q} x horizon in {1, Q/2, Q} (horizon >= every) x k in {-0.1, 0, 0.01}, and the latest-chunk schedules"""
    return ops.make_schedules(Q, every=[1, 3, Q], horizon=[1, max(1, Q // 2), Q], k=[-0.1, 0.0, 0.01], latest=True)


@functools.lru_cache(maxsize=None)
def _case(i):
    """chunks, grid, the numpy statement, a target and its statistics of case i: computed once and left unchanged"""
    T, Q, A, n = CASES[i]
    c = planted_chunks(T, Q, A, seed=400 + i)
    S = grid(Q)
    ref, ref_empty = ops.ensemble_sweep_ref(c, S, n, want_empty=True)
    rng = np.random.default_rng(500 + i)
    target = (rng.standard_normal((T, A)) * 2).astype(np.float32)
    mean, std = rng.standard_normal(A), 0.5 + rng.random(A)
    return torch.from_numpy(c).to(DEV), S, n, ref, ref_empty, target, mean, std


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_ensemble_sweep_against_the_masked_table_and_numpy(i):
    T, Q, A, _ = CASES[i]
    cd, S, n, ref, ref_empty, *_ = _case(i)
    raw, empty = ops.ensemble_sweep(cd, S, n, want_empty=True)
    assert raw.dtype == torch.float64 and tuple(raw.shape) == (len(S), T, A) and empty.dtype == torch.int32
    assert bool(torch.isfinite(raw).all()) and not bool(raw[:, n:].any())
    for g, s in enumerate(S):
        f, h = int(s["every"]), int(s["horizon"])
        if s["mode"] == ops.SCHEDULE_ENSEMBLE:                                         # (a) the existing op on the masked table
            m = torch.zeros_like(cd)
            m[::f, :h] = cd[::f, :h]
            assert torch.equal(raw[g], ops.episode_ensemble(m[None], [n], float(s["k"]))[0]), tuple(s)
        else:                                                                          # (b) the gather
            t = torch.arange(n, device=DEV)
            exp = torch.zeros((T, A), dtype=torch.float64, device=DEV)
            exp[:n] = cd[t - t % f, t % f].to(torch.float64)
            assert torch.equal(raw[g], exp), tuple(s)
    g0 = [tuple(s) for s in S].index((1, Q, 0, 0, 0.01))                               # the un-swept op on the unmasked table
    assert torch.equal(raw[g0], ops.episode_ensemble(cd[None], [n], 0.01)[0])
    err = float(np.abs(raw.cpu().numpy() - ref).max())
    print(f"{CASES[i]}: {len(S)} schedules, max|sweep - numpy| = {err:.3e}, empty steps {ref_empty.tolist()}")
    assert err <= 1e-13                                                                # (c)
    assert np.array_equal(empty.cpu().numpy(), ref_empty)                              # (d)
    if n:
        assert ref_empty[g0] >= 1 and not bool(raw[g0, 0].any())                       # the planted empty step: zeros, no NaN
    again, empty2 = ops.ensemble_sweep(cd, S, n, want_empty=True)                      # (f) twice: the same bits
    assert torch.equal(again.view(torch.int64), raw.view(torch.int64)) and torch.equal(empty2, empty)
    sd = ops.device_schedules(S, Q, DEV)                                               # the grid uploaded once, no counts
    assert torch.equal(ops.ensemble_sweep(cd, sd, n), raw)
    for g in (g0, len(S) - 1):                                                         # G = 1
        one, e1 = ops.ensemble_sweep(cd, S[g:g + 1], n, want_empty=True)
        assert torch.equal(one[0], raw[g]) and int(e1[0]) == int(ref_empty[g])
    if n == T:
        assert torch.equal(ops.ensemble_sweep(cd, S), raw)                             # the default length


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweep_error_against_action_error_and_numpy(i):
    T, Q, A, _ = CASES[i]
    _, S, n, ref, _, target, mean, std = _case(i)
    raw = torch.from_numpy(ref).to(DEV)
    td = torch.from_numpy(target).to(DEV)
    pred, st = ops.sweep_error(raw, td, n, mean, std)
    assert tuple(st.shape) == (len(S), 4, A) and st.dtype == torch.float64 and tuple(pred.shape) == tuple(raw.shape)
    for g in range(len(S)):                                                            # (e) the un-swept op, schedule by schedule
        p1, s1 = ops.action_error(raw[g:g + 1], td[None], [n], mean, std)
        assert torch.equal(st[g, :3], s1[0]) and torch.equal(pred[g], p1[0]), g
    exp_pred, exp = ops.sweep_error_ref(ref, target, n, mean, std)
    terms = np.abs(np.diff(exp_pred[:, :n], axis=1)).sum(axis=1)
    off = np.abs(st[:, 3].cpu().numpy() - exp[:, 3])
    print(f"{CASES[i]}: roughness off numpy by at most {off.max():.3e} (sum |term| up to {terms.max():.3e})")
    assert (off <= 1e-12 * terms).all()
    if n == 0:
        assert not bool(st.any())
    pred2, st2 = ops.sweep_error(raw, td, n, mean, std)                                # (f) twice: the same bits
    assert torch.equal(st2.view(torch.int64), st.view(torch.int64)) and torch.equal(pred2, pred)
    none_pred, st3 = ops.sweep_error(raw, target, n, mean, std, want_pred=False)       # a host target, no pred
    assert none_pred is None and torch.equal(st3, st)
    one = ops.sweep_error(raw[-1:], td, n, mean, std)[1]                               # G = 1
    assert torch.equal(one[0], st[-1])


def test_sweep_refuses_what_it_cannot_hold():
    dt = ops.schedule_dtype()
    S = ops.make_schedules(3)
    with pytest.raises(ValueError, match="action_dim"):
        ops.ensemble_sweep(torch.ones((2, 3, 65), device=DEV), S)
    with pytest.raises(ValueError, match="num_queries"):
        ops.ensemble_sweep(torch.ones((1, 7681, 1), device=DEV), ops.make_schedules(7681))
    with pytest.raises(ValueError, match="horizon"):
        ops.ensemble_sweep(torch.ones((4, 3, 2), device=DEV), np.array([(3, 2, 0, 0, 0.01)], dtype=dt))          # h < f
    with pytest.raises(ValueError):
        ops.ensemble_sweep(torch.ones((4, 3, 2), device=DEV), np.zeros(0, dtype=dt))                             # an empty grid
    with pytest.raises(ValueError):
        ops.ensemble_sweep(torch.ones((4, 3, 2), device=DEV), ops.make_schedules(4))                             # a grid for longer chunks
    with pytest.raises(ValueError):
        ops.ensemble_sweep(torch.ones((4, 3, 2), dtype=torch.float64, device=DEV), S)
    with pytest.raises(ValueError):
        ops.ensemble_sweep(torch.ones((1, 4, 3, 2), device=DEV), S)
    with pytest.raises(ValueError):
        ops.sweep_error(torch.ones((2, 4, 3), dtype=torch.float64, device=DEV), torch.ones((2, 4, 3)), None, [0.0] * 3, [1.0] * 3)
    # the library's own limits, behind the wrapper's
    from actmi import lib as L
    lib = L.load()
    sd = ops.device_schedules(S, 3, DEV)
    c, raw = torch.ones((2, 3, 4), device=DEV), torch.empty((2, 2, 4), dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    for G, T, Q, A, what in ((2, 2, 3, 65, b"action_dim"), (2, 2, 7681, 4, b"num_queries"), (65536, 2, 3, 4, b"65535"), (0, 2, 3, 4, b"65535")):
        assert lib.actmi_op_ensemble_sweep(p(c), 2, p(sd), p(raw), None, G, T, Q, A, None) != 0
        assert what in lib.actmi_op_last_error(), what
    assert lib.actmi_op_ensemble_sweep(None, 2, p(sd), p(raw), None, 2, 2, 3, 4, None) != 0
    assert lib.actmi_op_sweep_error(p(raw), None, 2, None, None, None, None, 2, 2, 4, None) != 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
T_EPS = (11, 7)


def _write_episode(path, cfg, T, sim, seed):
    rng = np.random.default_rng(seed)
    ep = {"/observations/qpos": rng.standard_normal((T, 14)).astype(np.float32), "/observations/qvel": np.zeros((T, 14), np.float32),
          "/action": rng.standard_normal((T, 16)).astype(np.float32), "attrs_sim": np.array(sim)}
    for c in cfg.camera_names:
        ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, cfg.image_h, cfg.image_w, 3), dtype=np.uint8)
    np.savez(path, **ep)


def test_replay_bc_sweep_on_the_device(tmp_path):
    from policy import ACTPolicy
    cfg = tiny_config()
    pc = dict(cfg.to_dict(), max_batch=4)
    Q = cfg.num_queries
    (tmp_path / "data").mkdir()
    for i, (T, sim) in enumerate(zip(T_EPS, (True, False))):
        _write_episode(tmp_path / "data" / f"episode_{i}.npz", cfg, T, sim, seed=30 + i)
    rng = np.random.default_rng(3)
    stats = {"qpos_mean": rng.standard_normal(14).astype(np.float32), "qpos_std": (0.5 + rng.random(14)).astype(np.float32),
             "action_mean": rng.standard_normal(16).astype(np.float32), "action_std": (0.5 + rng.random(16)).astype(np.float32)}
    policy = ACTPolicy(pc, init_seed=4)

    def run(name, **kw):
        config = {"ckpt_dir": str(tmp_path / name), "state_dim": 14, "policy_class": "ACT", "policy_config": pc,
                  "camera_names": cfg.camera_names, "episode_len": 11, "task_name": "sim_transfer_cube_scripted", "temporal_agg": True,
                  "dataset_dir": str(tmp_path / "data")}
        return IE.replay_bc(config, "policy_last.ckpt", policy=policy, stats=stats, batch=4, verbose=False, **kw)

    S = IE.replay_sweep_schedules(Q, k=[-0.1, 0.0, 0.01], every=[1, 3, Q], horizon=[Q, max(1, Q // 2)])
    plain = run("plain")
    swept = run("swept", sweep=S)
    # the same call with the numpy statements, fed the tables the device held
    tables = []

    def from_device(table, schedules, length, want_empty=False):
        tables.append(table)
        return ops.ensemble_sweep_ref(table.cpu(), schedules, length, want_empty=want_empty)

    stood_in = run("ref", sweep=S, ensemble_sweep=from_device, sweep_error=ops.sweep_error_ref)
    assert [tuple(t.shape) for t in tables] == [(T, Q, 16) for T in T_EPS] and all(t.is_cuda for t in tables)
    sw, ex = swept["sweep"], stood_in["sweep"]
    assert set(sw) == {"schedules", "mae_mean", "rmse_mean", "max_max", "rough_mean", "empty", "best", "default"}
    assert sw["schedules"] == ex["schedules"] == ops.schedules_as_dicts(S) and sw["empty"] == ex["empty"]
    for key in ("mae_mean", "rmse_mean", "max_max", "rough_mean"):
        rel = np.abs(np.asarray(sw[key]) - np.asarray(ex[key])) / np.abs(ex[key])
        print(f"replay_bc sweep, {len(S)} schedules, {key}: worst relative difference to the numpy statement {rel.max():.3e}")
        assert np.allclose(sw[key], ex[key], rtol=1e-12, atol=0)
    assert sw["best"] == int(np.argmin(sw["mae_mean"])) and sw["default"] == [tuple(s) for s in S].index((1, Q, 0, 0, 0.01))
    assert np.isclose(sw["mae_mean"][sw["default"]], plain["mae_mean"], rtol=1e-12, atol=0)      # the un-swept schedule
    assert sw["max_max"][sw["default"]] == plain["max_max"]
    assert len(set(sw["mae_mean"])) > 3                                                # the schedules differ
    # every pre-existing key and file: the same bits with or without the sweep
    assert {k: v for k, v in swept.items() if k != "sweep"} == plain
    for i in range(len(T_EPS)):
        a, b = np.load(tmp_path / "plain" / f"replay_policy_last_ep{i}.npz"), np.load(tmp_path / "swept" / f"replay_policy_last_ep{i}.npz")
        assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["target"], b["target"])


def test_train_bc_logs_the_sweep_and_keeps_choosing_by_the_default_schedule(tmp_path):
    """--replay_every with --replay_sweep: the sweep's figures are logged and appended to replay_history.json, the un-swept figures
    beside them are those of the default schedule"""
    import json
    from actmi import data as D
    cfg = tiny_config()
    Q = cfg.num_queries
    for i, (T, sim) in enumerate(((12, True), (9, False), (8, False))):
        (tmp_path / "data").mkdir(exist_ok=True)
        _write_episode(tmp_path / "data" / f"episode_{i}.npz", cfg, T, sim, seed=40 + i)
    train_dl, val_dl, _, _ = D.load_data(str(tmp_path / "data"), lambda n: True, cfg.camera_names, 2, 2, Q, policy_class="ACT", num_workers=0,
                                         rng=np.random.default_rng(7), device_dataset=True, device="cuda:0")
    pc = dict(cfg.to_dict(), max_batch=2, kl_weight=10, lr=1e-5)
    config = {"ckpt_dir": str(tmp_path / "ck"), "state_dim": 14, "policy_class": "ACT", "policy_config": pc, "camera_names": cfg.camera_names,
              "episode_len": 12, "task_name": "sim_transfer_cube_scripted", "temporal_agg": True, "dataset_dir": str(tmp_path / "data"),
              "num_steps": 2, "seed": 0, "eval_every": 0, "validate_every": 2, "save_every": 1000, "replay_every": 1, "replay_episodes": 1,
              "replay_align": "train", "replay_sweep": {"k": [0.0, 0.01], "every": [1, Q], "horizon": None}}
    logged = {}
    IE.train_bc(train_dl, val_dl, config, log=lambda d, step: logged.setdefault(step, {}).update(d))
    with open(tmp_path / "ck" / "replay_history.json") as f:
        hist = json.load(f)
    assert [h["step"] for h in hist] == [1, 2]
    for h in hist:
        sw, lg = h["sweep"], logged[h["step"]]
        assert len(sw["schedules"]) == len(sw["mae_mean"]) == 2 * 3 + 3                # (1, Q), (1, Q/2), (Q, Q) x 2 weights + latest
        assert sw["best"] == int(np.argmin(sw["mae_mean"])) and sw["schedules"][sw["default"]] == {"every": 1, "horizon": Q, "mode": "ensemble", "k": 0.01}
        assert lg["replay_sweep_best"] == h["replay_sweep_best"] == sw["best"]
        assert lg["replay_sweep_best_mae"] == h["replay_sweep_best_mae"] == sw["mae_mean"][sw["best"]] <= h["replay_mae_mean"] * (1 + 1e-12)
        assert lg["replay_sweep_default_mae"] == h["replay_sweep_default_mae"] == sw["mae_mean"][sw["default"]]
        assert np.isclose(h["replay_sweep_default_mae"], h["replay_mae_mean"], rtol=1e-12, atol=0)
    assert "replay_sweep_best_mae" not in logged[0] and (tmp_path / "ck" / "policy_best_replay.ckpt").is_file()
