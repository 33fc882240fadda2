"""Train / eval entry points of the ACT path with the reference's names and CLI
(reference imitate_episodes.py: main :37, make_policy :182, make_optimizer :194, get_image :206, eval_bc :228,
forward_pass :529, train_bc :535, repeater :624, CLI :633-666), re-designed for MI355X:

* eval rollouts are BATCHED: E episodes step in lock-step, one policy query of batch E per timestep through
  libactmi, one temporal-ensemble kernel for all episodes, envs stepped by host threads (the reference runs
  episodes one after another with batch 1, :319-353);
* episodes SHARD across ranks (one process per GPU): poses are pre-drawn in the reference's RNG order, every rank
  takes a contiguous slice, a single all-gather of (episode_return, highest_reward) ends the run;
* the 10 warm-up queries per rollout and the real-time sleep (:377-382, :467-470) are off by default;
* ``replay_bc`` (``--eval --replay``) evaluates open loop on recorded episodes instead -- the one evaluation of use_depth /
  use_pcd policies and of policies trained on real-robot episodes: queries batched over TIME, one ensemble launch per episode
  (``replay_bc`` drives it; its analyses, their pooling, report and logged figures live in ``actmi.replay``);
* ``--device_dataset --replay_every N`` runs that replay on held-out episodes every N training steps, out of the device-resident
  store the batches come from (no file read); ``--replay_horizon`` adds the error along the predicted chunk;
* ``--replay_sweep`` reads a grid of execution schedules (query rate, executed horizon, ensemble weight, or the latest chunk
  alone) off the chunk tables either replay already holds: two more launches per episode, no further policy query;
* ``--eval --replay --device_dataset --replay_knn K`` replays the same validation episodes once more through a nearest-neighbour
  lookup over the training episodes (VINN with the policy's own trunk as the embedding, actmi.vinn) and prints both errors;
* ``--device_dataset --use_pcd --device_clouds`` puts the task's stored point clouds into that store as well (the batches' clouds are
  gathered on the device; ``--replay_every`` then serves point-cloud policies), and ``--mirror_twins --use_pcd --cloud_mirror_axis
  {x,y,z} [--cloud_mirror_offset C]`` gives a stored cloud the mirror rule the twins need;
* ``--device_dataset --device_decode`` decodes the JPEG frames of compressed episodes on the device as that store is loaded
  (actmi_op_jpeg_decode, bit for bit the host's PIL decode); the store holds the same bytes;
* ``--mirror_twins`` joins every episode file by its mirrored twin (postprocess_episodes.py's definition), computed as it is read:
  ``actmi.data.load_data(..., mirror_twins=True)``; with ``--device_dataset`` the twins share their sources' frames;
* ``--augment_images`` and, for the stored clouds of ``--use_pcd``, ``--augment_clouds`` augment the TRAINING batches on the
  device (actmi.ops.ImageAugment / CloudAugment), each from draws of its own.
"""
import argparse
import json
import os
import pickle
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from copy import deepcopy
from itertools import repeat

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from actmi.constants import FPS, SIM_TASK_CONFIGS  # noqa: E402
from actmi.sim_utils import compute_dict_mean, draw_episode_poses, set_seed, shard_range  # noqa: E402
from actmi import dist_utils  # noqa: E402
from actmi import ops, replay  # noqa: E402
from actmi.replay import horizon_metrics, horizon_slots, replay_metrics, replay_sweep_schedules, sweep_metrics  # noqa: E402,F401


def make_policy(policy_class, policy_config, device=None):
    """reference imitate_episodes.py:182-191 (ACT only on this path).  ``device``: the GPU this process owns
    (cuda:LOCAL_RANK under a one-process-per-GPU launcher); None = the process's current device."""
    if policy_class == "ACT":
        from policy import ACTPolicy
        return ACTPolicy(policy_config, device=device)
    if policy_class == "Diffusion":
        from policy import DiffusionPolicy
        return DiffusionPolicy(policy_config, device=device)
    raise NotImplementedError(f"policy_class {policy_class} is outside the accelerated path (SURVEY §2)")


def make_optimizer(policy_class, policy):
    """reference imitate_episodes.py:194-203."""
    if policy_class == "ACT":
        return policy.configure_optimizers()
    raise NotImplementedError


def center_crop_resize(image, ratio=0.95):
    """The Diffusion policy's eval-time image transform (reference imitate_episodes.py:214-224): the centre `ratio` crop of
    f32 [..., H, W] images, resized back to (H, W).  torchvision's ``transforms.Resize(size, antialias=True)`` on a tensor is
    ``F.interpolate(mode='bilinear', align_corners=False, antialias=True)``, which is what runs here (torchvision itself is
    not importable offline)."""
    H, W = image.shape[-2:]
    crop = image[..., int(H * (1 - ratio) / 2): int(H * (1 + ratio) / 2), int(W * (1 - ratio) / 2): int(W * (1 + ratio) / 2)]
    lead = crop.shape[:-3]
    out = torch.nn.functional.interpolate(crop.reshape(-1, *crop.shape[-3:]), size=(H, W), mode="bilinear", align_corners=False,
                                          antialias=True)
    return out.reshape(*lead, *out.shape[-3:])


def get_image(ts, camera_names, rand_crop_resize=False):
    """reference imitate_episodes.py:206-225: one timestep -> f32 [1,C,3,H,W] in [0,1] on the GPU."""
    imgs = np.stack([np.moveaxis(ts.observation["images"][c], -1, 0) for c in camera_names], axis=0)
    curr_image = torch.from_numpy(imgs / 255.0).float().cuda().unsqueeze(0)
    if rand_crop_resize:
        curr_image = center_crop_resize(curr_image)
    return curr_image


def make_post_process(policy_class, stats):
    """reference imitate_episodes.py:290-293: Diffusion policies emit actions in [-1, 1] of the dataset's min / max range,
    the others z-scored actions."""
    if policy_class == "Diffusion":
        return lambda a: ((a + 1) / 2) * (stats["action_max"] - stats["action_min"]) + stats["action_min"]
    return lambda a: a * stats["action_std"] + stats["action_mean"]


def get_image_batch_u8(ts_list, camera_names, pinned=None):
    """Fast path of the same contract: E timesteps -> u8 [E,C,H,W,3] (4x fewer H2D bytes; /255 and the ImageNet
    normalisation are fused into the conv1 loader with the reference's float arithmetic)."""
    E, C = len(ts_list), len(camera_names)
    h, w, _ = ts_list[0].observation["images"][camera_names[0]].shape
    if pinned is None or tuple(pinned.shape) != (E, C, h, w, 3):
        pinned = torch.empty((E, C, h, w, 3), dtype=torch.uint8)
        if torch.cuda.is_available():
            pinned = pinned.pin_memory()
    buf = pinned.numpy()
    for e, ts in enumerate(ts_list):
        for c, name in enumerate(camera_names):
            buf[e, c] = ts.observation["images"][name]
    return pinned


def _default_stats(state_dim, action_dim=16):
    return {"qpos_mean": np.zeros(state_dim), "qpos_std": np.ones(state_dim),
            "action_mean": np.zeros(action_dim), "action_std": np.ones(action_dim),
            "action_min": -np.ones(action_dim), "action_max": np.ones(action_dim)}


def _load_policy_and_stats(config, ckpt_name, policy, stats, dev, verbose):
    """the policy and the dataset statistics of an evaluation: a given ``policy`` / ``stats`` is used as it is, otherwise the
    checkpoint ``ckpt_name`` and ``dataset_stats.pkl`` of ``ckpt_dir`` are read (reference imitate_episodes.py:241-251)"""
    ckpt_dir = config["ckpt_dir"]
    if policy is None:
        # inference-only handle (no grad buffers), built on this rank's device
        policy = make_policy(config["policy_class"], dict(config["policy_config"], training=False), device=str(dev))
        ckpt_path = os.path.join(ckpt_dir, ckpt_name)
        if os.path.isfile(ckpt_path):
            loading_status = policy.deserialize(torch.load(ckpt_path, weights_only=True))
            if verbose:
                print(loading_status)
        elif verbose:
            print(f"no checkpoint at {ckpt_path}: evaluating the random-init policy")
        policy.cuda()
        policy.eval()
    if stats is None:
        stats_path = os.path.join(ckpt_dir, "dataset_stats.pkl")
        if os.path.isfile(stats_path):
            with open(stats_path, "rb") as f:
                stats = pickle.load(f)               # written by this program's own main()
        else:
            stats = _default_stats(config["state_dim"])
    return policy, stats


def _make_vq_sampler(policy_config, ckpt_dir, dev, rank, verbose):
    """reference imitate_episodes.py:252-262: the latent prior, weights from latent_model_last.ckpt next to the policy;
    -> ``vq_sampler(n)``, n codes [n, vq_class, vq_dim] (:393: latent_model.generate(1, temperature=1, x=None))"""
    from actmi.latent_model import LatentModelTransformer, latent_model_spec
    from actmi.weights import generate_latent_model_state_dict
    vq_dim, vq_class = policy_config["vq_dim"], policy_config["vq_class"]
    latent_model = LatentModelTransformer(vq_dim, vq_dim, vq_class, device=str(dev))
    lm_path = os.path.join(ckpt_dir, "latent_model_last.ckpt")
    if os.path.isfile(lm_path):
        latent_model.load_state_dict(torch.load(lm_path, weights_only=True))
    else:
        if verbose:
            print(f"no latent model at {lm_path}: sampling codes from a random-init prior")
        latent_model.load_state_dict(generate_latent_model_state_dict(latent_model_spec(vq_dim, vq_dim, vq_class), 0))
    draws = [0]

    def vq_sampler(n):
        draws[0] += 1
        return latent_model.generate(n, temperature=1, x=None, seed=1000 * rank + draws[0])
    return vq_sampler


def eval_bc(config, ckpt_name, save_episode=True, num_rollouts=50, policy=None, ensemble_factory=None,
            env_factory=None, stats=None, max_parallel=None, warmup_queries=0, realtime=False, verbose=True,
            trace=None, vq_sampler=None, pipeline_groups=None):
    """reference imitate_episodes.py:228-526, batched + sharded.  Returns (success_rate, avg_return).

    VQ-ACT: the reference samples the latent code from its prior model each query
    (``latent_model.generate(1, temperature=1)``, imitate_episodes.py:252-262,393-394): ``actmi.latent_model`` mirrors it
    on the library's kernels; ``vq_sampler(n) -> [n, vq_class, vq_dim]`` overrides the source of the codes."""
    set_seed(1000)
    ckpt_dir = config["ckpt_dir"]
    policy_class = config["policy_class"]
    policy_config = config["policy_config"]
    if policy_config.get("use_depth") or getattr(policy, "use_depth", False):
        # the simulators here render no depth and the reference's depth rollouts read ROS camera topics; rolling the policy out on
        # RGB alone would report the success rate of a different model
        raise NotImplementedError("eval_bc cannot roll out a use_depth policy: no environment here produces depth frames "
                                  "(train with --use_depth, evaluate on the robot's own loop or `--replay` on recorded episodes)")
    if policy_config.get("use_pcd") or getattr(policy, "use_pcd", False):
        # likewise: no simulator here produces point clouds, the fork's rollouts read the robot's fused live cloud
        raise NotImplementedError("eval_bc cannot roll out a use_pcd policy: no environment here produces point clouds "
                                  "(train with --use_pcd, evaluate on the robot's own loop or `--replay` on recorded episodes)")
    camera_names = config["camera_names"]
    max_timesteps = int(config["episode_len"])
    task_name = config["task_name"]
    temporal_agg = config["temporal_agg"]
    rank, world, local_rank = dist_utils.init_from_env()
    on_gpu = torch.cuda.is_available()
    # one process per GPU: everything of this rank (engine arena, streams, frames, ensemble ring) lives on cuda:LOCAL_RANK
    dev = torch.device("cuda", local_rank if world > 1 else torch.cuda.current_device()) if on_gpu else torch.device("cpu")

    policy, stats = _load_policy_and_stats(config, ckpt_name, policy, stats, dev, verbose)
    pre_process = lambda s_qpos: (s_qpos - stats["qpos_mean"]) / stats["qpos_std"]          # noqa: E731
    post_process = make_post_process(policy_class, stats)
    is_diffusion = policy_class == "Diffusion"

    use_vq = bool(policy_config.get("vq", False))
    if use_vq and vq_sampler is None:
        vq_sampler = _make_vq_sampler(policy_config, ckpt_dir, dev, rank, verbose)
    num_queries = policy_config["num_queries"]
    query_frequency = 1 if temporal_agg else num_queries
    action_dim = policy_config.get("action_dim", 16)
    if ensemble_factory is None:
        from actmi.ops import TemporalEnsemble
        ensemble_factory = lambda E: TemporalEnsemble(E, num_queries, action_dim, 0.01, dev)   # noqa: E731
    if env_factory is None:
        from actmi.envs import make_sim_env
        env_factory = lambda pose, idx: make_sim_env(task_name, camera_names, pose, seed=idx,   # noqa: E731
                                                     synthetic=True if config.get("synthetic_env") else None)

    # poses in the reference's draw order, then this rank's contiguous shard
    poses = draw_episode_poses(task_name, num_rollouts, seed=1000)
    lo, hi = shard_range(num_rollouts, rank, world)
    counts = [shard_range(num_rollouts, r, world)[1] - shard_range(num_rollouts, r, world)[0] for r in range(world)]
    if max_parallel is None:
        max_parallel = getattr(getattr(policy, "model", None), "max_batch", None) or (hi - lo) or 1
    pdev = getattr(getattr(policy, "model", None), "device", None)
    if on_gpu and pdev is not None and torch.device(pdev) != dev:
        raise RuntimeError(f"rank {rank}: policy engine is on {pdev} but this rank's tensors are on {dev}")
    # on-screen rendering and per-episode video dumps (imitate_episodes.py:284-287, 342-346, 516-517) need matplotlib / cv2
    # windows and files per episode: outside the accelerated path -- refused or announced, never silently dropped
    if config.get("onscreen_render"):
        raise NotImplementedError("onscreen_render is not available on the batched MI355X eval path (episodes step in "
                                  "lock-step on the GPU; there is no per-episode matplotlib window)")
    if save_episode and verbose and rank == 0:
        print("note: save_episode=True writes the result_*.txt summary only; per-episode videos are not produced here")

    local_results = []
    env_max_reward = None
    DT = 1 / FPS
    t_policy, n_queries = 0.0, 0
    pool = ThreadPoolExecutor(max_workers=min(16, max(1, max_parallel)))
    engine = getattr(policy, "model", None)
    flags_dev = engine.flags_tensor() if (on_gpu and hasattr(engine, "flags_tensor")) else None

    def _copy_frames(buf, e, ts):
        for c, name in enumerate(camera_names):
            buf[e, c] = ts.observation["images"][name]
        return ts

    for w0 in range(lo, hi, max_parallel):
        ids = list(range(w0, min(hi, w0 + max_parallel)))
        E = len(ids)
        envs = [env_factory(poses[i], i) for i in ids]
        env_max_reward = envs[0].task.max_reward
        # Two groups of episodes in ping-pong (GPU only): while the GPU runs the policy query of one group, the host steps the
        # other group's simulators, gathers their frames into pinned memory and queues that group's next query -- the H2D copy,
        # the forward and the D2H of the actions of a group are queued on the stream back to back and waited for with an event,
        # never with a device-wide synchronisation.  Episodes are independent, so each one sees exactly the steps it would see
        # alone (tests/test_gpu_rollout.py).  pipeline_groups=1 (or a CPU stand-in policy) keeps the single lock-step group.
        G = 2 if (on_gpu and E >= 2 and pipeline_groups != 1 and not realtime) else 1
        cuts = [0, E] if G == 1 else [0, (E + 1) // 2, E]
        h, w, _ = None, None, None
        groups = []
        for gi in range(G):
            sl = slice(cuts[gi], cuts[gi + 1])
            g_envs = envs[sl]
            g = {"ids": ids[sl], "envs": g_envs, "E": len(g_envs), "ens": None, "rewards": [[] for _ in g_envs], "pinned": None,
                 "all_actions": None, "ev": torch.cuda.Event() if on_gpu else None, "raw_host": None, "flag_host": None, "tq": 0.0}
            g["ens"] = ensemble_factory(g["E"]) if (temporal_agg and not is_diffusion) else None
            g["ts"] = list(pool.map(lambda e: e.reset(), g_envs))
            groups.append(g)

        def enqueue(g, t):
            """queue step t of a group: (H2D of its frames +) policy query + ensemble + D2H of the actions, then an event"""
            nonlocal n_queries
            ts_list = g["ts"]
            qpos_numpy = np.stack([np.array(ts.observation["qpos"]) for ts in ts_list])
            qpos = torch.from_numpy(pre_process(qpos_numpy)).float().to(dev, non_blocking=True)
            g["tq"] = time.time()
            if t % query_frequency == 0:
                if g["pinned"] is None or t == 0:
                    g["pinned"] = get_image_batch_u8(ts_list, camera_names, g["pinned"])
                curr_image = g["pinned"].to(dev, non_blocking=True)
                if is_diffusion:
                    # get_image(..., rand_crop_resize=True) of the reference (:214-224, :374): f32 in [0, 1], centre 0.95 crop,
                    # resized back -- on the device, for all episodes of the group at once
                    curr_image = center_crop_resize(curr_image.permute(0, 1, 4, 2, 3).float().div(255.0))
                if t == 0:
                    for _ in range(warmup_queries):
                        policy(qpos, curr_image, vq_sample=vq_sampler(qpos.shape[0])) if use_vq else policy(qpos, curr_image)
                g["all_actions"] = (policy(qpos, curr_image, vq_sample=vq_sampler(qpos.shape[0])) if use_vq
                                    else policy(qpos, curr_image))            # [E_g,Q,A]
                n_queries += g["E"]
            if g["ens"] is not None:
                raw = g["ens"].step(g["all_actions"])                        # [E_g,A] float64, like the reference
            else:
                raw = g["all_actions"][:, t % query_frequency]
            if on_gpu:
                if g["raw_host"] is None or g["raw_host"].dtype != raw.dtype:
                    g["raw_host"] = torch.empty(tuple(raw.shape), dtype=raw.dtype).pin_memory()
                    g["flag_host"] = torch.zeros(1, dtype=torch.int32).pin_memory()
                g["raw_host"].copy_(raw, non_blocking=True)
                if flags_dev is not None:
                    g["flag_host"].copy_(flags_dev, non_blocking=True)       # the range guard's word rides along: no extra sync
                g["ev"].record()
            else:
                g["raw_host"] = raw

        def finish(g, t):
            """wait for step t of a group, step its simulators (frames of the next query straight into pinned memory)"""
            nonlocal t_policy
            if on_gpu:
                g["ev"].synchronize()                                        # this group's actions are on the host
                if flags_dev is not None and int(g["flag_host"][0]) != 0:
                    engine.check_flags()                                     # raises with the reason (and clears the word)
            raw_action = g["raw_host"].numpy().copy() if on_gpu else g["raw_host"].cpu().numpy()
            if t % query_frequency == 0:
                t_policy += time.time() - g["tq"]
            if trace is not None:
                trace.append((g["ids"], t, raw_action.copy()))
            action = post_process(raw_action)
            target_qpos = action[:, :-2]
            need_frames = (t + 1) % query_frequency == 0 and g["pinned"] is not None and t + 1 < max_timesteps
            buf = g["pinned"].numpy() if need_frames else None

            def step_one(p):
                e, env, a = p
                ts = env.step(a)
                return _copy_frames(buf, e, ts) if buf is not None else ts
            g["ts"] = list(pool.map(step_one, zip(range(g["E"]), g["envs"], target_qpos)))
            for e in range(g["E"]):
                g["rewards"][e].append(g["ts"][e].reward)

        time0 = time.time()
        for g in groups:
            enqueue(g, 0)
        for t in range(max_timesteps):
            time1 = time.time()
            for g in groups:
                finish(g, t)
                if t + 1 < max_timesteps:
                    enqueue(g, t + 1)
            if realtime:
                time.sleep(max(0, DT - (time.time() - time1)))
        if verbose:
            print(f"rank {rank}: episodes {ids[0]}..{ids[-1]} avg fps {max_timesteps / (time.time() - time0):.1f} "
                  f"({E} parallel episodes{', two ping-pong groups' if G == 2 else ''})")
        for g in groups:
            for e, i in enumerate(g["ids"]):
                r = np.array(g["rewards"][e])
                episode_return = float(np.sum(r[r != None]))                  # noqa: E711  (reference :499)
                local_results.append([episode_return, float(np.max(r))])
    pool.shutdown()

    local = torch.tensor(local_results, dtype=torch.float32).reshape(-1, 2)
    allr = dist_utils.all_gather_rows(local, counts).numpy()                 # the ONE collective of the path
    episode_returns, highest_rewards = allr[:, 0], allr[:, 1]
    success_rate = float(np.mean(highest_rewards == env_max_reward))
    avg_return = float(np.mean(episode_returns))
    summary_str = f"\nSuccess rate: {success_rate}\nAverage return: {avg_return}\n\n"
    for r in range(env_max_reward + 1):
        more_or_equal_r = int((highest_rewards >= r).sum())
        summary_str += f"Reward >= {r}: {more_or_equal_r}/{num_rollouts} = {more_or_equal_r / num_rollouts * 100}%\n"
    if rank == 0:
        if verbose:
            print(summary_str)
            if n_queries:
                # issue-to-host latency summed over the queries: with two groups in flight these intervals overlap each other and the
                # simulators, so this is a latency figure, not wall time ("avg fps" above is the throughput)
                print(f"policy queries: {n_queries} on rank 0, mean issue-to-host latency {1e3 * t_policy / n_queries:.2f} ms per query group")
        os.makedirs(ckpt_dir, exist_ok=True)
        result_file_name = "result_" + ckpt_name.split(".")[0] + ".txt"
        with open(os.path.join(ckpt_dir, result_file_name), "w") as f:
            f.write(summary_str)
            f.write(repr(episode_returns.tolist()))
            f.write("\n\n")
            f.write(repr(highest_rewards.tolist()))
    return success_rate, avg_return


def _replay_query(policy, data, use_depth, use_pcd, vq_sampler):
    """one policy query on a batch of an actmi.data.EpisodeReplay: (image, qpos[, depth | xyz, rgb, n]) -> a_hat [b, Q, A]"""
    image, qpos = data[0], data[1]
    kw = {}
    if use_depth:
        kw["depth_img"] = data[2]
    if use_pcd:
        kw["pointcloud"] = {"xyz": data[2], "rgb": data[3], "n": data[4]}
    if vq_sampler is not None:
        kw["vq_sample"] = vq_sampler(qpos.shape[0])
    return policy(qpos, image, **kw)


def check_replay_knn(knn, store, policy_class, policy_config, episodes=None):
    """The refusals of ``replay_bc(knn=...)`` / ``--replay_knn``, raised before anything is launched: no store, K outside
    [1, 512] or above the support rows, a non-finite or negative state weight, use_pcd and Diffusion policies.  ``knn``: an int K
    or a dict {"k", "state_weight" (1.0), "select_k" (None: no sweep; KMAX), "support_ids" (None: the store's episodes beyond the
    replayed ones, all of them when there are none), "exclude_self" (None: True exactly when a replayed episode is a support
    episode)}; a dict may carry a ready "policy" (and "support_rows"), which is then replayed as it is.  -> the completed dict"""
    from actmi import ops, vinn
    knn = dict(knn) if isinstance(knn, dict) else {"k": knn}
    vinn.check_policy_class(policy_class, policy_config)
    if store is None:
        raise ValueError("--replay_knn looks demonstrations up in the device-resident store: it needs --device_dataset (store=...)")
    if "k" not in knn:
        raise ValueError("replay_bc(knn=...): no k")
    replayed = replay.resolve_store_episodes(store, episodes)
    if knn.get("support_ids") is None:
        rest = [i for i in store.episode_ids if i not in set(replayed)]
        knn["support_ids"] = rest or list(store.episode_ids)
    knn["support_ids"] = [int(i) for i in knn["support_ids"]]
    missing = [i for i in knn["support_ids"] if i not in store._local_of]
    if missing or not knn["support_ids"]:
        raise ValueError(f"replay_bc(knn=...): support episodes {missing} are not in the store (it holds {list(store.episode_ids)})")
    if knn.get("support_rows") is None:
        knn["support_rows"] = int(sum(int(store.T[store._local_of[i]]) for i in knn["support_ids"]))
    knn["k"], knn["state_weight"] = ops.check_knn_args(knn["k"], knn.get("state_weight", 1.0), knn["support_rows"])
    if knn.get("select_k") is not None:
        knn["select_k"], _ = ops.check_knn_args(knn["select_k"], knn["state_weight"], knn["support_rows"])
    if knn.get("exclude_self") is None:
        knn["exclude_self"] = bool(set(replayed) & set(knn["support_ids"]))
    return knn


def _replay_knn(config, ckpt_name, knn, policy, stats, store, ids, batch, episode_ensemble, action_error, align):
    """the second replay of ``replay_bc(knn=...)``: the same episodes through the nearest-neighbour policy -> result["knn"]"""
    vp = knn.get("policy")
    sel = None
    if vp is None:
        from actmi import vinn
        support = knn.get("support") or vinn.SupportSet.from_store(store, policy, knn["support_ids"], batch, align)
        vp = vinn.VINNPolicy(support, knn["k"], knn["state_weight"], getattr(policy, "model", None), exclude_self=knn["exclude_self"], stats=stats)
        if knn.get("select_k") is not None:
            sel = vinn.select_k(support, store, ids, knn["select_k"], policy, knn["state_weight"], batch)
    sub = replay_bc(config, ckpt_name, episodes=ids, policy=vp, stats=stats, batch=batch, episode_ensemble=episode_ensemble,
                    align=align, save_episode=False, verbose=False, action_error=action_error, store=store)
    out = {"k": knn["k"], "state_weight": knn["state_weight"], "support_rows": knn["support_rows"],
           "mae_mean": sub["mae_mean"], "rmse_mean": sub["rmse_mean"], "max_max": sub["max_max"], "mae": sub["mae"],
           "empty": int(vp.empty_count()) if hasattr(vp, "empty_count") else 0}
    if sel is not None:
        out["select_k"] = {"mse": sel["mse"], "best_k": sel["best_k"]}
    return out


def replay_bc(config, ckpt_name, episodes=None, policy=None, stats=None, batch=None, episode_ensemble=None, align="train",
              save_episode=True, verbose=True, action_error=None, vq_sampler=None, store=None, horizon=False, chunk_error=None,
              attention=False, attention_slots=None, attention_frames=False, sweep=None, ensemble_sweep=None, sweep_error=None,
              knn=None):
    """Open-loop replay evaluation on recorded episodes (the fork's eval_arm_gripper_depth.py:343-418 without its plots): the
    policy is queried on an episode's recorded observations, the chunks are ensembled over time (``temporal_agg``) or executed
    chunk by chunk, un-normalised, and compared with the recorded ``/action``.  Serves what ``eval_bc`` cannot roll out --
    use_depth and use_pcd policies, and policies trained on real-robot episodes.

    The observation at step t does not depend on the action at t-1, so the queries of an episode are independent: they run
    ``batch`` frames at a time (default: the engine's max_batch), the batches reach the device through ``DevicePrefetcher``, the
    chunks land in a device table [1, T, Q, A], ONE ``ops.episode_ensemble`` launch ensembles every step and ``ops.action_error``
    reduces the error on the device.  Without ``temporal_agg`` only the frames t % Q == 0 are queried and
    raw[t] = chunk[t - t % Q][t % Q] (reference :392).

    ``episodes``: None = every file ``find_all_hdf5(config["dataset_dir"])`` finds (sorted), an int n = the first n; they are
    sharded over the ranks.  ``align``: "train" compares step t with action[t] of a sim episode and action[max(0, t-1)] of a
    real one (the shift the dataset trains slot 0 on), "none" with action[t] as the fork's plot does.  ``policy``,
    ``episode_ensemble`` and ``action_error`` can be given (CPU stand-ins: ops.episode_ensemble_ref, ops.action_error_ref).

    ``store`` (an actmi.data.DeviceEpisodeStore, as ``--device_dataset`` training holds): the episodes are replayed out of device
    memory through ``DeviceEpisodeReplay`` -- no file is opened, nothing is pinned or copied from the host, the target rows are
    taken on the device from the store's action rows; everything after the queries is unchanged.  ``episodes`` may then also be a
    list of episode ids of the store (None: all it holds, an int n: the first n).

    ``horizon``: one ``ops.chunk_error`` launch per episode on the table the replay already holds (``chunk_error=``:
    ops.chunk_error_ref is the CPU stand-in) gives the error of slot j of a predicted chunk against the action j steps ahead, the
    entry the dataset trains that slot on under ``align="train"``; the rows are pooled over the episodes like the others and
    returned as ``result["horizon"] = {"mae": [Q][A], "rmse": [Q][A], "max": [Q][A], "mae_mean": [Q], "count": [Q]}``.  Without
    ``horizon`` the result and the files have no such key.
    ``attention`` (``--replay_attention``): one [batch, Q, N] buffer is bound to the policy's engine for the replay's queries
    (ACTEngine.bind_attention), so every query also leaves the decoder's cross-attention map, which is cut by the engine's token
    layout on the device (actmi.attention_maps.split_attention; ``attention_slots = (q0, q1)``: the mean over those action slots,
    default all).  Per episode i the rank that replayed it writes replay_<ckpt>_ep<i>_attn.npz -- ``rgb`` [S, K, fh, fw], ``depth``
    [S, Kd, fh, fw], ``extra`` [S, n_extra], ``share`` [S, n_sources] (float32, one row per queried step), ``steps`` [S] and
    ``sources`` (the names of share's columns) -- and ``result["attention"] = {"sources", "share_mean", "slots", "steps"}`` pools
    the share over all queried steps (sums divided by the count).  ``attention_frames``: also the queried steps' uint8 frames
    with the RGB maps laid over them (ops.heat_overlay with ops.heat_ramp) as replay_<ckpt>_ep<i>_attn_frames.npy
    [S, K, H, W, 3].  The queries, and with them every error figure, are the same bits with or without it.
    ``sweep`` (``--replay_sweep``; an ``ops.schedule_dtype()`` array, see ``ops.make_schedules``): G execution schedules -- query
    every f frames, execute the first h slots of a chunk, ensemble weight k or just the latest chunk -- read off the table the
    replay already holds, with no further policy query: per episode one ``ops.ensemble_sweep`` and one ``ops.sweep_error`` launch
    after the existing ones (``ensemble_sweep=``, ``sweep_error=``: ops.ensemble_sweep_ref and ops.sweep_error_ref are the CPU
    stand-ins).  It needs ``temporal_agg`` -- the table must hold a chunk for every frame, and the stride-Q table is not derived
    from it: a frame's a_hat is not promised to be independent of its batch mates -- else ValueError.  The rows are pooled over
    the episodes and ranks like the others into ``result["sweep"] = {"schedules": [{every, horizon, mode, k}], "mae_mean" [G],
    "rmse_mean" [G], "max_max" [G], "rough_mean" [G] (the mean |pred[t] - pred[t-1]| per step and joint: the smoothness a schedule
    gives up), "empty" [G] (steps without a populated live row), "best", "default"}`` (``sweep_metrics``), in action units.  Every
    other key, file and printed figure is the same bits with or without it.
    ``knn`` (``--replay_knn K``; ``{"k", "state_weight", "select_k", "support_ids", "exclude_self"}``, see ``check_replay_knn``):
    after the policy's replay the SAME episodes are replayed once more through ``actmi.vinn.VINNPolicy`` -- the k nearest frames of
    the store's episodes ``support_ids`` (default: those it holds beyond the replayed ones, the training split) by the policy's
    own trunk features and z-scored qpos, and the softmax-weighted mean of their action chunks -- with the same ensemble and error
    code, and ``result["knn"] = {"k", "state_weight", "support_rows", "mae_mean", "rmse_mean", "max_max", "mae", "empty"[,
    "select_k": {"mse", "best_k"}]}`` says what a lookup achieves where the policy achieved ``result["mae_mean"]``.  It needs a
    ``store`` and an ACT policy without use_pcd, else ValueError before anything is launched.  Every other key, file and printed
    figure is the same bits with or without it.
    Returns {"episodes": [...], "mae": [A], "rmse": [A], "max": [A], "mae_mean", "rmse_mean", "max_max", "steps", ...} in
    action units; with ``save_episode`` rank 0 writes replay_<ckpt>.json and per episode replay_<ckpt>_ep<i>.npz (pred, target)."""
    from actmi.data import DeviceEpisodeReplay, DevicePrefetcher, EpisodeReplay, find_all_hdf5
    ckpt_dir, policy_class, policy_config = config["ckpt_dir"], config["policy_class"], config["policy_config"]
    if knn is not None:
        knn = check_replay_knn(knn, store, policy_class, policy_config, episodes)
    if policy_class == "Diffusion":
        raise NotImplementedError("replay_bc: the Diffusion policy has no temporal ensemble and its crop-resize input path is not "
                                  "part of the replay")
    if align not in ("train", "none"):
        raise ValueError(f"align must be 'train' or 'none', got {align!r}")
    camera_names, temporal_agg = config["camera_names"], config["temporal_agg"]
    rank, world, local_rank = dist_utils.init_from_env()
    on_gpu = torch.cuda.is_available()
    dev = torch.device("cuda", local_rank if world > 1 else torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    if stats is None and store is not None:
        stats = getattr(store, "norm_stats", None)                   # the statistics the store z-scores its qpos rows with
    policy, stats = _load_policy_and_stats(config, ckpt_name, policy, stats, dev, verbose)
    if not policy_config.get("vq", False):
        vq_sampler = None
    elif vq_sampler is None:
        vq_sampler = _make_vq_sampler(policy_config, ckpt_dir, dev, rank, verbose)
    use_depth = bool(policy_config.get("use_depth") or getattr(policy, "use_depth", False))
    use_pcd = bool(policy_config.get("use_pcd") or getattr(policy, "use_pcd", False))
    Q = int(policy_config["num_queries"])
    A = int(policy_config.get("action_dim", 16))
    engine = getattr(policy, "model", None)
    batch = batch or getattr(engine, "max_batch", None) or 8
    episode_ensemble, action_error = episode_ensemble or ops.episode_ensemble, action_error or ops.action_error
    mean, std = (np.asarray(stats[k], dtype=np.float64).reshape(-1) for k in ("action_mean", "action_std"))
    if mean.shape[0] != A or std.shape[0] != A:
        raise ValueError(f"the dataset statistics hold {mean.shape[0]} action components, the policy's action_dim is {A}")
    stride = 1 if temporal_agg else Q
    # the optional analyses, in the order their rows are gathered over the ranks (every rank issues the same collectives)
    parts = []
    if horizon:
        parts.append(replay.horizon_part(chunk_error, mean, std, stride, Q, A))
    if sweep is not None:
        parts.append(replay.sweep_part(sweep, ensemble_sweep, sweep_error, temporal_agg, mean, std, Q, A, dev))
    if attention_frames and not attention:
        raise ValueError("replay_bc: attention_frames overlays the attention maps: it needs attention=True")
    dataset_dir = config.get("dataset_dir")
    if store is not None:
        if use_pcd and not getattr(store, "has_clouds", False):
            raise NotImplementedError("replay_bc: the device-resident store holds no point clouds (use_pcd); one built with "
                                      "--device_clouds does")
        ids = replay.resolve_store_episodes(store, episodes)
        files = [store.paths[store._local_of[i]] for i in ids]
    else:
        if not (dataset_dir and os.path.isdir(dataset_dir)):
            raise ValueError(f"replay_bc needs recorded episodes: config['dataset_dir'] = {dataset_dir!r} is not a directory (--dataset_dir)")
        files = find_all_hdf5(dataset_dir, bool(config.get("skip_mirrored_data", False)))
        if episodes is not None:
            if not isinstance(episodes, (int, np.integer)):
                raise ValueError("replay_bc: a list of episode ids names episodes of a store (store=...)")
            files = files[:int(episodes)]
        if not files:
            raise ValueError(f"replay_bc: no episode files under {dataset_dir}")
    spans = [shard_range(len(files), r, world) for r in range(world)]
    lo, hi = spans[rank]
    stem = "replay_" + ckpt_name.split(".")[0] if save_episode else None          # (a periodic replay saves nothing and has no name)
    local_pt, time0, n_frames = [], time.time(), 0

    def base_episode(i, ep, table, raw, target, actions, shift):
        pred, st = action_error(raw, target, None, mean, std)
        if save_episode:
            local_pt.append(torch.cat([torch.as_tensor(pred).to(torch.float64).cpu().reshape(ep.T, A),
                                       target[0].to(torch.float64).cpu()], dim=1))
        return replay.row(1 + 3 * A, float(ep.T), st)
    about = dict(align=align, temporal_agg=bool(temporal_agg), num_queries=Q,
                 files=[os.path.relpath(f, dataset_dir) if dataset_dir else f for f in files])
    parts.insert(0, replay.Part(1 + 3 * A, base_episode, lambda rows: dict(replay_metrics(rows, A), **about)))
    if attention:                                                # (last: it binds its buffer to the engine until end())
        parts.append(replay.attention_part(engine, attention_slots, attention_frames, camera_names,
                                           policy_config.get("depth_camera_names") if use_depth else None, batch, dev, ckpt_dir, stem))
    rows = [[] for _ in parts]
    for i in range(lo, hi):
        if store is not None:
            ep = DeviceEpisodeReplay(store, ids[i], batch, stride=stride)
            actions = ep.actions_device                                                              # [T, A] f32, file units
            if getattr(policy, "exclude_self", False):           # (an actmi.vinn.VINNPolicy: leave-one-episode-out)
                policy.set_exclude(ids[i])
        else:
            ep = EpisodeReplay(files[i], camera_names, stats, batch, depth_camera_names=policy_config.get("depth_camera_names"),
                               use_depth=use_depth, pointcloud_names=config.get("pointcloud_names"), use_pcd=use_pcd,
                               max_points=policy_config.get("max_points"), pcd_ignore_mask=bool(config.get("pcd_ignore_mask", False)),
                               stride=stride)
            actions = torch.from_numpy(ep.actions)
        if actions.shape[1] != A:
            raise ValueError(f"{files[i]}: the recorded actions are {actions.shape[1]} wide, the policy's action_dim is {A}")
        # the chunk of replayed step s: row s of the table (temporal_agg: s = t, every frame; else s = t // Q)
        table = torch.zeros((1, len(ep.steps), Q, A), dtype=torch.float32, device=dev)
        s0 = 0
        for data in (ep if store is not None else DevicePrefetcher(ep, device=dev if on_gpu else None)):
            a_hat = _replay_query(policy, data, use_depth, use_pcd, vq_sampler)
            table[0, s0:s0 + a_hat.shape[0]] = a_hat
            for part in parts:
                part.batch(data, a_hat.shape[0])
            s0 += a_hat.shape[0]
        n_frames += s0
        if temporal_agg:
            raw = torch.as_tensor(episode_ensemble(table, None, 0.01)).to(torch.float64)            # [1, T, A]
        else:
            raw = table.reshape(1, -1, A)[:, :ep.T].to(torch.float64)                                # reference :392
        shift = 1 if (align == "train" and not ep.is_sim) else 0                                     # utils.py:112-114
        # [1, T, A] f32, file units: row t is action[max(0, t - shift)] (taken where the rows are: on the device with a store)
        target = (torch.cat([actions[:1], actions[:ep.T - 1]], dim=0) if shift else actions)[None]
        for part, mine in zip(parts, rows):
            mine.append(part.episode(i, ep, table, raw, target, actions, shift))
        if engine is not None and hasattr(engine, "check_flags") and on_gpu:
            engine.check_flags()
        if store is not None and hasattr(store, "check_decoded"):
            store.check_decoded()                                # a compressed store: the episode's batches decoded with status 0
    for part in parts:
        part.end()
    if verbose and n_frames:
        print(f"rank {rank}: replayed episodes {lo}..{hi - 1}, {n_frames} queries in batches of {batch}, "
              f"{n_frames / max(time.time() - time0, 1e-9):.1f} frames/s")

    result = {}
    for part, mine in zip(parts, rows):
        result.update(part.pooled(replay.gathered(mine, part.width, [b - a for a, b in spans])))
    if knn is not None:
        result["knn"] = _replay_knn(config, ckpt_name, knn, policy, stats, store, ids, batch, episode_ensemble, action_error, align)
    if save_episode:
        Ts = [e["T"] for e in result["episodes"]]
        allpt = replay.gathered(local_pt, 2 * A, [sum(Ts[a:b]) for a, b in spans])
        if rank == 0:
            os.makedirs(ckpt_dir, exist_ok=True)
            for i, pt in enumerate(np.split(allpt, np.cumsum(Ts)[:-1])):
                np.savez(os.path.join(ckpt_dir, f"{stem}_ep{i}.npz"), pred=pt[:, :A], target=pt[:, A:].astype(np.float32))
            with open(os.path.join(ckpt_dir, stem + ".json"), "w") as f:
                json.dump(result, f, indent=1)
    if verbose and rank == 0:
        replay.report(result)
    return result


def _augment_frames(augment, image_data, depth_data=None):
    """the frames of a training batch through ``augment.apply`` (actmi.ops.ImageAugment): the raw u8 image batch, and with it --
    in ONE call, so that both see the same draws -- the raw uint16 depth frames of a use_depth batch"""
    if image_data.dtype != torch.uint8:
        raise NotImplementedError(f"--augment_images runs on the raw u8 [B, K, H, W, 3] frames, not on a {image_data.dtype} image "
                                  "batch (f32_images)")
    if depth_data is None:
        return augment.apply(image_data), None
    if depth_data.dtype != torch.uint16:
        raise NotImplementedError(f"--augment_images warps raw uint16 depth frames, not a {depth_data.dtype} depth batch (f32_depth)")
    return augment.apply(image_data, depth_data)


def forward_pass(data, policy, augment=None, cloud_augment=None):
    """reference imitate_episodes.py:529-532; a 5-tuple ends in the depth frames of a use_depth dataset (the fork's
    train_single_arm_gripper_all.py:568-588), a 7-tuple in the padded clouds of a use_pcd dataset and their valid counts
    (pcd_xyz, pcd_rgb, pcd_n; the fork's :576-591 passes the one fused cloud).

    ``augment`` (an actmi.ops.ImageAugment; None: nothing changes): the batch's frames go through its ``apply`` on the device
    before the policy sees them -- the reference's dataset augmentation (utils.py:141-156), one draw per sample.  The raw depth
    frames of a use_depth batch are warped with the SAME draws; the fork draws a second time for depth
    (utils_arm_gripper_all.py:180-184), which moves depth and colour apart -- the intent, registered frames, is followed here.
    The clouds of a use_pcd batch are left alone unless ``cloud_augment`` is given.

    ``cloud_augment`` (an actmi.ops.CloudAugment; None: nothing changes): the clouds and counts of a 7-tuple go through its
    ``apply`` on the device -- yaw, scale, shift, jitter, point dropout, colour jitter, one draw per sample -- and the policy gets
    what it returns: the kept points in front, zeros behind, the new counts.  It draws independently of ``augment``."""
    depth_data = None
    if len(data) == 7:
        image_data, qpos_data, action_data, is_pad, pcd_xyz, pcd_rgb, pcd_n = data
        dev = getattr(getattr(policy, "model", None), "device", None) or "cuda"
        image_data, qpos_data, action_data, is_pad, pcd_xyz, pcd_rgb, pcd_n = (
            t.to(dev, non_blocking=True) for t in (image_data, qpos_data, action_data, is_pad, pcd_xyz, pcd_rgb, pcd_n))
        if augment is not None:
            image_data, _ = _augment_frames(augment, image_data)
        if cloud_augment is not None:
            pcd_xyz, pcd_rgb, pcd_n = cloud_augment.apply(pcd_xyz.contiguous(), pcd_rgb.contiguous(), pcd_n)
        return policy(qpos_data, image_data, action_data, is_pad, pointcloud={"xyz": pcd_xyz, "rgb": pcd_rgb, "n": pcd_n})
    if len(data) == 5:
        image_data, qpos_data, action_data, is_pad, depth_data = data
    else:
        image_data, qpos_data, action_data, is_pad = data
    dev = getattr(getattr(policy, "model", None), "device", None) or "cuda"
    image_data, qpos_data, action_data, is_pad = (t.to(dev, non_blocking=True) for t in (image_data, qpos_data, action_data, is_pad))
    if depth_data is not None:
        depth_data = depth_data.to(dev, non_blocking=True)
        if augment is not None:
            image_data, depth_data = _augment_frames(augment, image_data, depth_data)
        return policy(qpos_data, image_data, action_data, is_pad, depth_img=depth_data)
    if augment is not None:
        image_data, _ = _augment_frames(augment, image_data)
    return policy(qpos_data, image_data, action_data, is_pad)


def make_augment(config, policy, seed):
    """the ImageAugment of a --augment_images run, sized from the policy's engine; None without the flag"""
    if not config.get("augment_images"):
        return None
    from actmi.ops import ImageAugment
    eng = policy.model
    cfg = eng.cfg
    return ImageAugment(eng, cfg.num_cams, cfg.image_h, cfg.image_w, eng.max_batch, seed=seed,
                        Kd=cfg.num_depth_cams)


# seed + rank of a run, mixed with a constant of its own: the cloud augmenter's generator must not repeat the image augmenter's
CLOUD_AUGMENT_SEED_MIX = 0x636C6F7564


def make_cloud_augment(config, policy, seed):
    """the CloudAugment of a --augment_clouds run, sized from the policy's engine (max_points, max_batch), about the config's
    cloud_pivot; None without the flag"""
    if not config.get("augment_clouds"):
        return None
    from actmi.ops import CloudAugment
    eng = policy.model
    return CloudAugment(eng, eng.max_points, eng.max_batch, pivot=tuple(config.get("cloud_pivot") or (0.0, 0.0, 0.0)), seed=seed)


def train_bc(train_dataloader, val_dataloader, config, log=None):
    """reference imitate_episodes.py:535-622 (wandb replaced by an optional ``log(dict, step)`` callable)."""
    num_steps = config["num_steps"]
    ckpt_dir = config["ckpt_dir"]
    seed = config["seed"]
    policy_class = config["policy_class"]
    policy_config = config["policy_config"]
    eval_every = config.get("eval_every") or 0
    if eval_every and policy_config.get("use_depth"):
        print("use_depth: no environment here produces depth frames, the periodic rollouts (--eval_every) are skipped")
        eval_every = 0
    if eval_every and policy_config.get("use_pcd"):
        print("use_pcd: no environment here produces point clouds, the periodic rollouts (--eval_every) are skipped")
        eval_every = 0
    validate_every = config["validate_every"]
    save_every = config["save_every"]
    # --replay_every: open-loop replay of validation episodes out of the device-resident store the loaders share
    replay_every = int(config.get("replay_every") or 0)
    replay_store = getattr(train_dataloader, "store", None)
    replay_ids = list(getattr(val_dataloader, "episode_ids", []))
    if replay_every:
        if replay_store is None or not replay_ids:
            raise ValueError("--replay_every replays validation episodes out of the device-resident store: it needs the loaders of "
                             "--device_dataset (load_data(..., device_dataset=True))")
        if config.get("replay_episodes") is not None:
            replay_ids = replay_ids[:int(config["replay_episodes"])]
    replay_history, best_replay = [], None
    replay_sweep = (replay_sweep_schedules(policy_config["num_queries"], **config["replay_sweep"])
                    if replay_every and config.get("replay_sweep") is not None else None)
    # data parallel (one process per GPU under torch.distributed.run): every rank builds the same initial policy on its own
    # device, draws ITS OWN batches and dropout masks (seed + rank), averages gradients over RCCL in loss.backward(); only
    # rank 0 writes checkpoints
    rank, world, local_rank = dist_utils.init_from_env()
    set_seed(seed + rank)
    dev = f"cuda:{local_rank}" if world > 1 else None
    policy = make_policy(policy_class, dict(policy_config, seed=policy_config.get("seed", seed) * world + rank), device=dev)
    if config.get("load_pretrain"):
        # reference :548-550 reads a path in its author's home directory; here: config["pretrain_ckpt_path"], else the
        # environment's ACTMI_PRETRAIN_CKPT, else that same path -- and a missing file is an error, not a silent skip
        pre = (config.get("pretrain_ckpt_path") or os.environ.get("ACTMI_PRETRAIN_CKPT") or
               os.path.join("/home/zfu/interbotix_ws/src/act/ckpts/pretrain_all", "policy_step_50000_seed_0.ckpt"))
        if not os.path.isfile(pre):
            raise FileNotFoundError(f"--load_pretrain: no checkpoint at {pre} (set --pretrain_ckpt_path or ACTMI_PRETRAIN_CKPT)")
        loading_status = policy.deserialize(torch.load(pre, weights_only=True))
        print(f"loaded! {loading_status}")
    if config.get("resume_ckpt_path"):
        loading_status = policy.deserialize(torch.load(config["resume_ckpt_path"], weights_only=True))
        print(f'Resume policy from: {config["resume_ckpt_path"]}, Status: {loading_status}')
    policy.cuda()
    optimizer = make_optimizer(policy_class, policy)
    min_val_loss = np.inf
    best_ckpt_info = None
    os.makedirs(ckpt_dir, exist_ok=True)
    from actmi.data import DevicePrefetcher
    if getattr(train_dataloader, "on_device", False):
        train_dataloader = iter(train_dataloader)        # --device_dataset: the batches are gathered on the device, nothing to pin or copy
    else:
        train_dataloader = DevicePrefetcher(repeater(train_dataloader))      # next batch's H2D copy overlaps this step
    # --augment_images: one device pass over the TRAINING batches just before the stem.  Validation stays un-augmented, so that
    # validation losses of runs with and without the flag compare (the reference's validation set is augmented too: utils.py:153)
    augment = make_augment(config, policy, seed + rank)
    # --augment_clouds: the same for the stored clouds of a use_pcd batch, training batches only for the same reason; its draws come
    # from a generator of its own (another seed), so the two streams are independent
    cloud_augment = make_cloud_augment(config, policy, (seed + rank) ^ CLOUD_AUGMENT_SEED_MIX)
    for step in range(num_steps + 1):
        if step % validate_every == 0:
            policy.eval()
            validation_dicts = []
            for batch_idx, data in enumerate(val_dataloader):
                validation_dicts.append({k: v.detach().float().cpu() for k, v in forward_pass(data, policy).items()})
                if batch_idx > 50:
                    break
            for dl in (train_dataloader, val_dataloader):       # a compressed store: every batch so far decoded with status 0
                if hasattr(getattr(dl, "store", None), "check_decoded"):
                    dl.store.check_decoded()
            validation_summary = compute_dict_mean(validation_dicts)
            epoch_val_loss = float(validation_summary["loss"])
            if epoch_val_loss < min_val_loss:
                min_val_loss = epoch_val_loss
                best_ckpt_info = (step, min_val_loss, deepcopy(policy.serialize()))
            if log:
                log({f"val_{k}": float(v) for k, v in validation_summary.items()}, step)
            print(f"Val loss:   {epoch_val_loss:.5f}")
        if eval_every and step > 0 and step % eval_every == 0:
            # reference :590-596: first save, then evaluate that checkpoint with 10 rollouts (eval_bc builds its own
            # inference-only handle from the file; under data-parallel training the rollouts shard over the ranks)
            ckpt_name = f"policy_step_{step}_seed_{seed}.ckpt"
            if rank == 0:
                torch.save(policy.serialize(), os.path.join(ckpt_dir, ckpt_name))
            dist_utils.barrier()
            success, _ = eval_bc(config, ckpt_name, save_episode=True, num_rollouts=config.get("eval_rollouts", 10),
                                 verbose=(rank == 0))
            if log:
                log({"success": success}, step)
        if replay_every and step > 0 and step % replay_every == 0:
            # every rank replays its share of the episodes and all of them pool the figures.  The queries run on the training
            # handle: its prepared weights (split images, repacked and fused convolutions, decoder constants) are rebuilt by every
            # optimizer step, so they are the weights of this step.  Nothing is drawn from the batch sampler, the dropout counter
            # or the augmenter, and replay_bc reads the range guard's flags after every episode (a raised flag is an error there).
            policy.eval()
            res = replay_bc(config, None, policy=policy, stats=replay_store.norm_stats, store=replay_store, episodes=replay_ids,
                            align=config.get("replay_align") or "train", save_episode=False, verbose=(rank == 0),
                            horizon=bool(config.get("replay_horizon")), sweep=replay_sweep)
            figures = replay.replay_figures(res)
            replay_history.append(dict(figures, step=step, steps=res["steps"], episodes=len(res["episodes"]),
                                       **({"sweep": res["sweep"]} if "sweep" in res else {})))
            if best_replay is None or res["mae_mean"] < best_replay[1]:
                best_replay = (step, res["mae_mean"], deepcopy(policy.serialize()))
            if log:
                log(figures, step)
        policy.train()
        optimizer.zero_grad()
        data = next(train_dataloader)
        forward_dict = forward_pass(data, policy, augment, cloud_augment)
        loss = forward_dict["loss"]
        loss.backward()
        optimizer.step()
        if log:
            log({k: float(v) for k, v in forward_dict.items()}, step)
        if step % save_every == 0 or step % validate_every == 0:
            policy.model.check_flags()                   # non-finite loss / weight beyond its split scale: fail loudly
        if step % save_every == 0 and rank == 0:
            torch.save(policy.serialize(), os.path.join(ckpt_dir, f"policy_step_{step}_seed_{seed}.ckpt"))
    best_step, min_val_loss, best_state_dict = best_ckpt_info
    for dl in (train_dataloader, val_dataloader):
        if hasattr(getattr(dl, "store", None), "check_decoded"):
            dl.store.check_decoded()
    if rank == 0:
        torch.save(policy.serialize(), os.path.join(ckpt_dir, "policy_last.ckpt"))
        torch.save(best_state_dict, os.path.join(ckpt_dir, f"policy_step_{best_step}_seed_{seed}.ckpt"))
        print(f"Training finished:\nSeed {seed}, val loss {min_val_loss:.6f} at step {best_step}")
        if replay_every:
            with open(os.path.join(ckpt_dir, "replay_history.json"), "w") as f:
                json.dump(replay_history, f, indent=1)
            if best_replay is not None:
                torch.save(best_replay[2], os.path.join(ckpt_dir, "policy_best_replay.ckpt"))
                print(f"Best open-loop replay: MAE {best_replay[1]:.6f} at step {best_replay[0]}")
    dist_utils.barrier()                # checkpoints are on disk before any rank goes on to read them
    return best_ckpt_info


def repeater(data_loader):
    """reference imitate_episodes.py:624-630."""
    epoch = 0
    for loader in repeat(data_loader):
        for data in loader:
            yield data
        print(f"Epoch {epoch} done")
        epoch += 1


def build_config(args):
    """The config dict of reference main() (:37-143)."""
    task_name = args["task_name"]
    task_config = SIM_TASK_CONFIGS[task_name]
    camera_names = task_config["camera_names"]
    policy_class = args["policy_class"]
    if policy_class == "ACT":                        # reference :74-94
        policy_config = {"lr": args["lr"], "num_queries": args["chunk_size"], "kl_weight": args["kl_weight"],
                         "hidden_dim": args["hidden_dim"], "dim_feedforward": args["dim_feedforward"], "lr_backbone": 1e-5,
                         "backbone": "resnet18", "enc_layers": 4, "dec_layers": 7, "nheads": 8,
                         "camera_names": camera_names, "vq": args.get("use_vq", False), "vq_class": args.get("vq_class"),
                         "vq_dim": args.get("vq_dim"), "action_dim": 16, "no_encoder": args.get("no_encoder", False),
                         "state_dim": 14, "max_batch": args.get("max_batch") or args["batch_size"]}
        if args.get("use_depth"):                    # the fork's train_single_arm_gripper_all.py:66: the names come from the task
            depth_camera_names = task_config.get("depth_camera_names")
            if not depth_camera_names:
                raise ValueError(f"--use_depth: the task config of {task_name!r} lists no depth_camera_names")
            policy_config.update(use_depth=True, depth_camera_names=list(depth_camera_names))
        if args.get("use_pcd"):                      # the fork's one fused cloud: its name comes from the task as well
            pointcloud_names = task_config.get("pointcloud_names")
            if not pointcloud_names:
                raise ValueError(f"--use_pcd: the task config of {task_name!r} lists no pointcloud_names")
            policy_config.update(use_pcd=True, max_points=int(args.get("max_points") or 4096))
    elif policy_class == "Diffusion":                # reference :95-106
        policy_config = {"lr": args["lr"], "camera_names": camera_names, "action_dim": 16, "observation_horizon": 1,
                         "action_horizon": 8, "prediction_horizon": args["chunk_size"], "num_queries": args["chunk_size"],
                         "num_inference_timesteps": 10, "ema_power": 0.75, "vq": False}
    else:
        raise NotImplementedError(f"policy_class {policy_class} is outside the accelerated path (SURVEY §2)")
    if args.get("use_depth") and policy_class != "ACT":
        raise NotImplementedError("--use_depth: depth cameras belong to the ACT policy")
    if args.get("use_pcd") and policy_class != "ACT":
        raise NotImplementedError("--use_pcd: the point-cloud token belongs to the ACT policy")
    if args.get("augment_images") and policy_class != "ACT":
        raise NotImplementedError("--augment_images: the device-side augmentation belongs to the ACT training path (Diffusion "
                                  "training is outside the accelerated path)")
    if args.get("augment_clouds"):
        if policy_class != "ACT":
            raise NotImplementedError("--augment_clouds: the point-cloud token and its augmentation belong to the ACT training path")
        if not args.get("use_pcd"):
            raise ValueError("--augment_clouds augments the stored clouds of a --use_pcd run: there are none without --use_pcd")
        pivot = args.get("cloud_pivot") or (0.0, 0.0, 0.0)
        if len(pivot) != 3 or not all(np.isfinite(float(v)) for v in pivot):
            raise ValueError(f"--cloud_pivot {pivot}: needs 3 finite numbers")
    config = {"num_steps": args["num_steps"], "eval_every": args["eval_every"], "validate_every": args["validate_every"],
            "save_every": args["save_every"], "ckpt_dir": args["ckpt_dir"], "resume_ckpt_path": args.get("resume_ckpt_path"),
            "episode_len": task_config["episode_len"], "state_dim": 14, "lr": args["lr"],
            "policy_class": args["policy_class"], "onscreen_render": args.get("onscreen_render", False),
            "policy_config": policy_config, "task_name": task_name, "seed": args["seed"],
            "temporal_agg": args["temporal_agg"], "camera_names": camera_names, "real_robot": False,
            "load_pretrain": bool(args.get("load_pretrain", False)), "pretrain_ckpt_path": args.get("pretrain_ckpt_path"),
            "synthetic_env": bool(args.get("synthetic_env", False)),
            "dataset_dir": args.get("dataset_dir") or task_config.get("dataset_dir"),
            "skip_mirrored_data": bool(args.get("skip_mirrored_data", False))}
    if args.get("use_pcd"):
        config["pointcloud_names"] = list(task_config["pointcloud_names"])
    if args.get("augment_images"):
        config["augment_images"] = True
    if args.get("augment_clouds"):
        config["augment_clouds"] = True
        config["cloud_pivot"] = [float(v) for v in (args.get("cloud_pivot") or (0.0, 0.0, 0.0))]
    if (args.get("knn_state_weight") is not None or args.get("knn_select_k") is not None) and args.get("replay_knn") is None:
        raise ValueError("--knn_state_weight and --knn_select_k belong to --replay_knn")
    if args.get("replay_knn") is not None:
        from actmi import ops, vinn
        if args.get("replay_every"):
            raise ValueError("--replay_knn with --replay_every: inside training the trunk moves and the cached support features would "
                             "be stale; evaluate with --eval --replay afterwards")
        if not (args.get("eval") and args.get("replay")):
            raise ValueError("--replay_knn replays the nearest-neighbour baseline beside an open-loop replay: it needs --eval --replay")
        vinn.check_policy_class(policy_class, {"use_pcd": bool(args.get("use_pcd"))})
        if not args.get("device_dataset"):
            raise ValueError("--replay_knn looks demonstrations up in the device-resident store: it needs --device_dataset")
        k, w = ops.check_knn_args(args["replay_knn"], 1.0 if args.get("knn_state_weight") is None else args["knn_state_weight"])
        config["replay_knn"] = {"k": k, "state_weight": w}
        if args.get("knn_select_k") is not None:
            config["replay_knn"]["select_k"] = ops.check_knn_args(args["knn_select_k"], w)[0]
    if args.get("device_dataset"):
        if policy_class != "ACT":
            raise NotImplementedError("--device_dataset: the device-resident episode store feeds the ACT training path")
        if args.get("use_pcd") and not args.get("device_clouds"):
            raise NotImplementedError("--device_dataset with --use_pcd: point clouds through the device-resident store are not "
                                      "implemented; drop --device_dataset (or put the stored clouds into the store: --device_clouds)")
        config["device_dataset"] = True
        if args.get("device_dataset_gb") is not None:
            config["device_dataset_gb"] = float(args["device_dataset_gb"])
    if args.get("device_decode"):
        if not args.get("device_dataset"):
            raise ValueError("--device_decode decodes the compressed frames of the device-resident store: it needs --device_dataset")
        config["device_decode"] = True
    if args.get("store_compressed"):
        if not (args.get("device_dataset") and args.get("device_decode")):
            raise ValueError("--store_compressed keeps the device-resident store's frames compressed and decodes every batch on the "
                             "device: it needs --device_dataset --device_decode")
        config["store_compressed"] = True
    if args.get("store_encode"):
        if not args.get("store_compressed"):
            raise ValueError("--store_encode encodes raw episodes into the store that stays compressed: it needs --store_compressed "
                             "(and --device_dataset --device_decode)")
        config["store_encode"] = True
        config["store_encode_quality"] = int(args.get("store_encode_quality") or 50)
        config["store_encode_subsampling"] = str(args.get("store_encode_subsampling") or "420")
    if args.get("store_depth_pack"):
        if not args.get("store_encode"):
            raise ValueError("--store_depth_pack packs the raw depth of episodes the store encodes as it loads them: it needs "
                             "--store_encode (and --store_compressed --device_dataset --device_decode)")
        if not args.get("use_depth"):
            raise ValueError("--store_depth_pack packs depth frames: it needs --use_depth")
        config["store_depth_pack"] = True
    if args.get("device_clouds"):
        if not (args.get("device_dataset") and args.get("use_pcd")):
            raise ValueError("--device_clouds puts the stored clouds of a --use_pcd dataset into the device-resident store: it needs "
                             "--device_dataset and --use_pcd")
        config["device_clouds"] = True
    cloud_axis = args.get("cloud_mirror_axis")
    if cloud_axis is None and args.get("cloud_mirror_offset"):
        raise ValueError("--cloud_mirror_offset is the plane of --cloud_mirror_axis")
    if cloud_axis is not None:
        if not (args.get("mirror_twins") and args.get("use_pcd")):
            raise ValueError("--cloud_mirror_axis is the mirror rule of the stored clouds of --mirror_twins with --use_pcd")
        offset = float(args.get("cloud_mirror_offset") or 0.0)
        if cloud_axis not in ("x", "y", "z") or not np.isfinite(offset) or abs(2.0 * offset) > float(np.finfo(np.float32).max):
            raise ValueError(f"--cloud_mirror_axis {cloud_axis!r} --cloud_mirror_offset {offset!r}: needs x, y or z and a finite offset")
    if args.get("mirror_twins"):
        if policy_class != "ACT":
            raise NotImplementedError("--mirror_twins: the mirrored twin episodes feed the ACT training path")
        if args.get("use_pcd") and cloud_axis is None:
            raise ValueError("--mirror_twins with --use_pcd: a stored point cloud has no mirror rule (--cloud_mirror_axis gives it one)")
        config["mirror_twins"] = True
        if cloud_axis is not None:
            config["cloud_mirror"] = ["xyz".index(cloud_axis), offset]
    if args.get("replay_every"):
        if int(args["replay_every"]) < 0:
            raise ValueError("--replay_every must not be negative")
        if policy_class != "ACT":
            raise NotImplementedError("--replay_every: the periodic open-loop replay belongs to the ACT training path")
        if args.get("use_pcd") and not args.get("device_clouds"):
            raise NotImplementedError("--replay_every with --use_pcd: the device-resident store holds no point clouds (--device_clouds "
                                      "puts them there); evaluate with --eval --replay afterwards")
        if not args.get("device_dataset"):
            raise ValueError("--replay_every replays validation episodes out of the device-resident store: it needs "
                             "--device_dataset")
        config.update(replay_every=int(args["replay_every"]), replay_episodes=args.get("replay_episodes"),
                      replay_align=args.get("replay_align") or "train", replay_horizon=bool(args.get("replay_horizon")))
    if args.get("replay_attention_slots") is not None and not args.get("replay_attention"):
        raise ValueError("--replay_attention_slots selects the action slots of --replay_attention")
    if args.get("replay_attention_frames") and not args.get("replay_attention"):
        raise ValueError("--replay_attention_frames overlays the maps of --replay_attention")
    if args.get("replay_attention"):
        if not (args.get("eval") and args.get("replay")):
            raise ValueError("--replay_attention records the attention maps of an open-loop replay: it needs --eval --replay")
        if policy_class != "ACT":
            raise NotImplementedError("--replay_attention: the cross-attention map belongs to the ACT policy's decoder")
        slots = args.get("replay_attention_slots")
        if slots is not None:
            slots = [int(s) for s in slots]
            if len(slots) != 2 or not 0 <= slots[0] < slots[1] <= int(args["chunk_size"]):
                raise ValueError(f"--replay_attention_slots {slots}: needs 0 <= Q0 < Q1 <= chunk_size {args['chunk_size']}")
        config.update(replay_attention=True, replay_attention_slots=slots,
                      replay_attention_frames=bool(args.get("replay_attention_frames")))
    sweep_lists = {key: args.get("replay_sweep_" + key) for key in ("k", "every", "horizon")}
    if any(v is not None for v in sweep_lists.values()) and not args.get("replay_sweep"):
        raise ValueError("--replay_sweep_k, --replay_sweep_every and --replay_sweep_horizon are the grid of --replay_sweep")
    if args.get("replay_sweep"):
        if not ((args.get("eval") and args.get("replay")) or args.get("replay_every")):
            raise ValueError("--replay_sweep reads execution schedules off an open-loop replay: it needs --eval --replay or --replay_every")
        if not args.get("temporal_agg"):
            raise ValueError("--replay_sweep needs --temporal_agg: the schedules are read off the table of a chunk for every frame")
        replay_sweep_schedules(int(args["chunk_size"]), **sweep_lists)          # the grid's refusals, before anything is loaded
        config["replay_sweep"] = sweep_lists
    return config


def _load_episode_data(args, config, task_config, dataset_dir, world, local_rank):
    """``load_data`` on the episode files of ``dataset_dir`` with the task's and the command line's settings: what training reads,
    and, with ``--device_dataset``, the store an ``--eval --replay --replay_knn`` run looks its neighbours up in"""
    from actmi.data import load_data
    name_filter = task_config.get("name_filter", lambda n: True)
    return load_data(dataset_dir, name_filter, config["camera_names"], args["batch_size"], args["batch_size"],
                     args.get("chunk_size") or 100, args.get("skip_mirrored_data", False),
                     policy_class=config["policy_class"], stats_dir_l=task_config.get("stats_dir"),
                     sample_weights=task_config.get("sample_weights"),
                     train_ratio=task_config.get("train_ratio", 0.99),
                     depth_camera_names=config["policy_config"].get("depth_camera_names"),
                     use_depth=bool(config["policy_config"].get("use_depth")), pointcloud_names=config.get("pointcloud_names"),
                     use_pcd=bool(config["policy_config"].get("use_pcd")), max_points=config["policy_config"].get("max_points"),
                     # --device_dataset: every rank holds its own full store on its own device
                     device_dataset=bool(config.get("device_dataset")), mirror_twins=bool(config.get("mirror_twins")),
                     device_clouds=bool(config.get("device_clouds")), device_decode=bool(config.get("device_decode")),
                     store_compressed=bool(config.get("store_compressed")), store_encode=bool(config.get("store_encode")),
                     encode_quality=config.get("store_encode_quality", 50), encode_subsampling=config.get("store_encode_subsampling", "420"),
                     depth_pack=bool(config.get("store_depth_pack")),
                     cloud_mirror=tuple(config["cloud_mirror"]) if config.get("cloud_mirror") else None,
                     device=f"cuda:{local_rank}" if world > 1 else None,     # train_bc's device
                     device_budget_bytes=(int(config["device_dataset_gb"] * 2**30)
                                          if config.get("device_dataset_gb") is not None else None))


def main(args):
    set_seed(1)
    config = build_config(args)
    rank, world, local_rank = dist_utils.init_from_env()          # one process per GPU when a launcher set WORLD_SIZE
    os.makedirs(config["ckpt_dir"], exist_ok=True)
    if rank == 0:
        with open(os.path.join(config["ckpt_dir"], "config.pkl"), "wb") as f:
            pickle.dump(config, f)
    if args["eval"] and args.get("replay"):
        # open-loop replay on recorded episodes: what a use_depth / use_pcd policy (no simulator renders its inputs) and a policy
        # trained on real-robot episodes can be evaluated with
        kw = dict(episodes=args.get("replay_episodes"))
        if config.get("replay_knn") is not None:
            # the store --device_dataset training holds (the same split from the same seed): the validation episodes are replayed,
            # the training episodes are the support set
            task_config = SIM_TASK_CONFIGS[args["task_name"]]
            dataset_dir = args.get("dataset_dir") or task_config.get("dataset_dir")
            if not (dataset_dir and os.path.isdir(dataset_dir)):
                raise ValueError("--replay_knn needs episode files (--dataset_dir)")
            train_dl, val_dl, stats, _ = _load_episode_data(args, config, task_config, dataset_dir, world, local_rank)
            kw = dict(episodes=list(val_dl.episode_ids)[:args.get("replay_episodes")], store=val_dl.store, stats=stats,
                      knn=dict(config["replay_knn"], support_ids=list(train_dl.episode_ids)))
        return replay_bc(config, "policy_last.ckpt", align=args.get("replay_align") or "train", save_episode=True,
                         horizon=bool(args.get("replay_horizon")), attention=bool(config.get("replay_attention")),
                         attention_slots=config.get("replay_attention_slots"),
                         attention_frames=bool(config.get("replay_attention_frames")),
                         sweep=(replay_sweep_schedules(config["policy_config"]["num_queries"], **config["replay_sweep"])
                                if config.get("replay_sweep") is not None else None), **kw)
    if args["eval"]:
        results = []
        for ckpt_name in ["policy_last.ckpt"]:
            success_rate, avg_return = eval_bc(config, ckpt_name, save_episode=True, num_rollouts=args["num_rollouts"])
            results.append([ckpt_name, success_rate, avg_return])
        for ckpt_name, success_rate, avg_return in results:
            print(f"{ckpt_name}: {success_rate=} {avg_return=}")
        return results
    from actmi.config import ACTConfig
    from actmi.envs import SyntheticDataset
    cfg = ACTConfig.from_policy_config(config["policy_config"])
    task_config = SIM_TASK_CONFIGS[args["task_name"]]
    camera_names, policy_class = config["camera_names"], config["policy_class"]
    dataset_dir = args.get("dataset_dir") or task_config.get("dataset_dir")
    use_depth = bool(config["policy_config"].get("use_depth"))
    if use_depth and not (dataset_dir and os.path.isdir(dataset_dir)):
        raise ValueError("--use_depth needs episode files with /observations/depth_images/<cam> (--dataset_dir): the synthetic "
                         "stand-in dataset holds no depth frames")
    use_pcd = bool(config["policy_config"].get("use_pcd"))
    if use_pcd and not (dataset_dir and os.path.isdir(dataset_dir)):
        raise ValueError("--use_pcd needs episode files with /observations/pointcloud/<name>/{xyz, rgb} (--dataset_dir): the "
                         "synthetic stand-in dataset holds no point clouds")
    device_dataset = bool(config.get("device_dataset"))
    if device_dataset and not (dataset_dir and os.path.isdir(dataset_dir)):
        raise ValueError("--device_dataset needs episode files (--dataset_dir): the synthetic stand-in dataset is generated, not stored")
    if config.get("mirror_twins") and not (dataset_dir and os.path.isdir(dataset_dir)):
        raise ValueError("--mirror_twins needs episode files (--dataset_dir): the synthetic stand-in dataset has no arms to swap")
    if dataset_dir and os.path.isdir(dataset_dir):
        # reference imitate_episodes.py:141-147: episodes on disk (HDF5 via h5py, or .npz with the same keys), z-scored
        # qpos / actions, u8 images; batches reach the device through pinned staging on a side stream
        train_dl, val_dl, stats, _ = _load_episode_data(args, config, task_config, dataset_dir, world, local_rank)
    else:
        train_dl = SyntheticDataset(cfg, args["batch_size"], 8, seed=args["seed"] * world + rank)     # disjoint per rank
        val_dl = SyntheticDataset(cfg, args["batch_size"], 2, seed=args["seed"] * world + rank + 100003)
        stats = _default_stats(14)
    if rank == 0:
        with open(os.path.join(config["ckpt_dir"], "dataset_stats.pkl"), "wb") as f:
            pickle.dump(stats, f)
    best_step, min_val_loss, best_state_dict = train_bc(train_dl, val_dl, config)
    if rank == 0:
        torch.save(best_state_dict, os.path.join(config["ckpt_dir"], "policy_best.ckpt"))
        print(f"Best ckpt, val loss {min_val_loss:.6f} @ step{best_step}")
    dist_utils.barrier()


def make_parser():
    """the CLI of reference imitate_episodes.py:633-666 and this path's additions"""
    parser = argparse.ArgumentParser()
    parser.add_argument("--eval", action="store_true")
    parser.add_argument("--onscreen_render", action="store_true")
    parser.add_argument("--ckpt_dir", action="store", type=str, required=True)
    parser.add_argument("--policy_class", action="store", type=str, required=True)
    parser.add_argument("--task_name", action="store", type=str, required=True)
    parser.add_argument("--batch_size", action="store", type=int, required=True)
    parser.add_argument("--seed", action="store", type=int, required=True)
    parser.add_argument("--num_steps", action="store", type=int, required=True)
    parser.add_argument("--lr", action="store", type=float, required=True)
    parser.add_argument("--load_pretrain", action="store_true", default=False)
    parser.add_argument("--pretrain_ckpt_path", action="store", type=str, default=None,
                        help="checkpoint --load_pretrain reads (the reference hard-codes a path in its author's home directory)")
    parser.add_argument("--eval_every", action="store", type=int, default=500)
    parser.add_argument("--validate_every", action="store", type=int, default=500)
    parser.add_argument("--save_every", action="store", type=int, default=500)
    parser.add_argument("--resume_ckpt_path", action="store", type=str)
    parser.add_argument("--skip_mirrored_data", action="store_true")
    parser.add_argument("--kl_weight", action="store", type=int)
    parser.add_argument("--chunk_size", action="store", type=int)
    parser.add_argument("--hidden_dim", action="store", type=int)
    parser.add_argument("--dim_feedforward", action="store", type=int)
    parser.add_argument("--temporal_agg", action="store_true")
    parser.add_argument("--use_vq", action="store_true")
    parser.add_argument("--vq_class", action="store", type=int)
    parser.add_argument("--vq_dim", action="store", type=int)
    parser.add_argument("--no_encoder", action="store_true")
    parser.add_argument("--use_depth", action="store_true",
                        help="ACT with one depth camera per RGB camera: the task config's depth_camera_names, raw 16-bit frames "
                             "from /observations/depth_images/<cam>")
    parser.add_argument("--use_pcd", action="store_true",
                        help="ACT with a point-cloud token: the task config's one pointcloud_names entry, ragged clouds from "
                             "/observations/pointcloud/<name>/{xyz, rgb, padding_mask}")
    parser.add_argument("--max_points", action="store", type=int, default=4096,
                        help="--use_pcd: the largest stored cloud (rows per frame) the engine's workspace is sized for")
    # additions (rollouts count hard-coded to 10 in the reference, :156)
    parser.add_argument("--num_rollouts", action="store", type=int, default=50)
    parser.add_argument("--max_batch", action="store", type=int, default=None)
    parser.add_argument("--synthetic_env", action="store_true",
                        help="evaluate on the SyntheticEnv stand-in even when a sim_env module is importable "
                             "(throughput / plumbing runs; its success rates are not task results)")
    parser.add_argument("--dataset_dir", action="store", type=str, default=None,
                        help="episode files (reference HDF5 layout, or .npz with the same keys); default: the task's dataset_dir")
    parser.add_argument("--replay", action="store_true",
                        help="with --eval: open-loop replay on the recorded episodes of --dataset_dir (replay_bc) instead of simulator "
                             "rollouts: per-joint MAE / RMSE / max of the executed against the recorded actions")
    parser.add_argument("--replay_episodes", action="store", type=int, default=None, help="--replay: only the first N episode files")
    parser.add_argument("--replay_align", action="store", type=str, default="train", choices=["train", "none"],
                        help="--replay: compare step t with the action the dataset trains slot 0 on (train: action[t-1] for "
                             "real-robot episodes) or with action[t] (none)")
    parser.add_argument("--replay_every", action="store", type=int, default=0,
                        help="ACT training with --device_dataset: every N steps replay the validation episodes (at most "
                             "--replay_episodes, aligned by --replay_align) open loop out of the device-resident store; the figures "
                             "go to replay_history.json, the weights with the lowest mean MAE to policy_best_replay.ckpt (0: off)")
    parser.add_argument("--replay_knn", action="store", type=int, default=None, metavar="K",
                        help="--eval --replay --device_dataset: after the policy's replay, replay the same (validation) episodes through "
                             "a nearest-neighbour lookup (VINN) over the training episodes -- the K nearest frames by the policy's own "
                             "trunk features and z-scored qpos, softmax-weighted mean of their action chunks -- and report both MAEs "
                             "(result['knn']); K in 1..512")
    parser.add_argument("--knn_state_weight", action="store", type=float, default=None, metavar="W",
                        help="--replay_knn: weight of the z-scored qpos distance beside the feature distance (default 1.0: a choice, "
                             "not a measurement; the reference's values are for raw qpos)")
    parser.add_argument("--knn_select_k", action="store", type=int, default=None, metavar="KMAX",
                        help="--replay_knn: also the slot-0 error of every k = 1..KMAX on the replayed episodes (vinn_select_k.py)")
    parser.add_argument("--replay_attention", action="store_true",
                        help="--eval --replay: also record the decoder's cross-attention map of every query, cut per camera and "
                             "source (replay_<ckpt>_ep<i>_attn.npz), and print / log the attention share per source")
    parser.add_argument("--replay_attention_slots", action="store", type=int, nargs=2, default=None, metavar=("Q0", "Q1"),
                        help="--replay_attention: the mean over the action slots Q0 .. Q1-1 of a chunk (default: all)")
    parser.add_argument("--replay_attention_frames", action="store_true",
                        help="--replay_attention: also write the queried frames with the maps laid over them (..._attn_frames.npy)")
    parser.add_argument("--replay_horizon", action="store_true",
                        help="--replay_every and --eval --replay: also the error of slot j of a predicted chunk against the action j "
                             "steps ahead (how the error grows along the chunk)")
    parser.add_argument("--replay_sweep", action="store_true",
                        help="--eval --replay and --replay_every, with --temporal_agg: read a grid of execution schedules (query every "
                             "F frames, execute the first H slots of a chunk, ensemble weight K or just the latest chunk) off the "
                             "chunk tables the replay already holds -- two more launches per episode, no further policy query -- and "
                             "report the error and the roughness of each.  Default grid: K in {-0.1, 0, 0.01, 0.05, 0.25}, F in "
                             "{1, Q/4, Q/2, Q}, H in {Q, Q/2}, plus the latest-chunk schedules: choices, not measurements")
    parser.add_argument("--replay_sweep_k", action="store", type=float, nargs="+", default=None, metavar="K",
                        help="--replay_sweep: the ensemble weights exp(-K * i) of the grid (K < 0 favours the newest chunk)")
    parser.add_argument("--replay_sweep_every", action="store", type=int, nargs="+", default=None, metavar="F",
                        help="--replay_sweep: the query rates of the grid (a chunk from every F-th frame)")
    parser.add_argument("--replay_sweep_horizon", action="store", type=int, nargs="+", default=None, metavar="H",
                        help="--replay_sweep: the executed slots of a chunk (F <= H <= chunk_size; pairs with H < F are left out)")
    parser.add_argument("--augment_images", action="store_true",
                        help="ACT training only, opt-in: the reference dataset's augmentation (random 0.95 crop resized back, rotation "
                             "within 5 degrees, brightness / contrast / saturation jitter) on the device, for training batches; the "
                             "reference switches it on for Diffusion alone, which is outside this path")
    parser.add_argument("--augment_clouds", action="store_true",
                        help="ACT training with --use_pcd, opt-in: augment the stored clouds of the training batches on the device "
                             "(yaw within 5 degrees about +z, 5 %% scale, 1 cm shift, 2 mm per-point jitter, a tenth of the points "
                             "dropped, the colour jitter of --augment_images); composes with --augment_images, draws of its own")
    parser.add_argument("--cloud_pivot", action="store", type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                        help="--augment_clouds: the point of the clouds' frame the yaw and the scale are taken about (default: the "
                             "base frame's origin)")
    parser.add_argument("--device_dataset", action="store_true",
                        help="ACT training from --dataset_dir, opt-in: read every episode once into device memory and gather the "
                             "training batches there (actmi.data.DeviceEpisodeStore): the same batches as the host loader, no loader "
                             "workers; every rank holds the whole dataset; with --use_pcd only together with --device_clouds")
    parser.add_argument("--device_clouds", action="store_true",
                        help="--device_dataset --use_pcd, opt-in: the task's stored point clouds go into the device-resident store "
                             "and every batch's clouds are gathered on the device; lifts the refusal of --device_dataset (and of "
                             "--replay_every) with --use_pcd")
    parser.add_argument("--device_decode", action="store_true",
                        help="--device_dataset, opt-in: the JPEG frames of compressed episodes are decoded on the device as the store "
                             "is loaded (actmi_op_jpeg_decode) instead of one by one on the host; the store holds the same bytes")
    parser.add_argument("--store_compressed", action="store_true",
                        help="--device_dataset --device_decode, opt-in: the store keeps the frames' entropy segments and per-row marks "
                             "(about 1/35 of the decoded bytes) and decodes every batch on the device (actmi_op_jpeg_decode_marked); the "
                             "batches are the same bytes")
    parser.add_argument("--store_encode", action="store_true",
                        help="--store_compressed, opt-in: raw episodes (uint8 camera frames) are encoded on the device as the store "
                             "reads them (actmi_op_jpeg_encode_marked, which also writes the marks: no index pass); raw and compressed "
                             "files may be mixed; the batches are those of compress_data.py followed by --store_compressed")
    parser.add_argument("--store_encode_quality", action="store", type=int, default=50, help="--store_encode: JPEG quality, 1..100")
    parser.add_argument("--store_encode_subsampling", action="store", type=str, choices=("420", "444"), default="420",
                        help="--store_encode: chroma subsampling")
    parser.add_argument("--store_depth_pack", action="store_true",
                        help="--store_encode --use_depth, opt-in: the raw uint16 depth frames of raw episodes, which --store_encode "
                             "alone refuses, are packed losslessly on the device as the store reads them (actmi_op_depth_pack) and "
                             "unpacked for every batch (actmi_op_depth_unpack); the depth tensors are those of the decoded store")
    parser.add_argument("--cloud_mirror_axis", action="store", type=str, choices=("x", "y", "z"), default=None,
                        help="--mirror_twins --use_pcd: the twin's stored cloud is the source's reflected across a plane normal to "
                             "this axis of the clouds' frame; lifts the refusal of --mirror_twins with --use_pcd")
    parser.add_argument("--cloud_mirror_offset", action="store", type=float, default=0.0,
                        help="--cloud_mirror_axis: where that plane lies, coordinate -> 2 * offset - coordinate (default 0)")
    parser.add_argument("--mirror_twins", action="store_true",
                        help="ACT training on episode files: join every episode by its mirrored twin (arms and wrist cameras "
                             "swapped, frames flipped, as postprocess_episodes.py defines it), computed as it is read; with "
                             "--device_dataset the twins take no frame memory; with --use_pcd only under --cloud_mirror_axis, and a directory that already "
                             "holds mirrored files needs --skip_mirrored_data")
    parser.add_argument("--device_dataset_gb", action="store", type=float, default=None,
                        help="--device_dataset: device memory the store may take, in GiB (default: what is free minus a 64 GiB reserve)")
    return parser


if __name__ == "__main__":
    main(vars(make_parser().parse_args()))
