"""VINN as a replay baseline: nearest-neighbour action retrieval on the device (the reference's vinn_cache_feature.py,
vinn_select_k.py and vinn_eval.py), with the policy's own trunk as the embedding.

Every demonstration frame of a ``DeviceEpisodeStore`` is embedded by the spatial mean of the policy's layer4 maps
(``ACTEngine.bind_features``, one forward stopped after the trunk); a query looks up its k nearest frames by
``||feature difference|| + state_weight * ||z-scored qpos difference||`` (``ops.knn_topk``) and executes the softmax(-distance)
weighted mean of their action chunks (``ops.knn_predict``), read straight out of the store's action rows.  ``VINNPolicy`` has the
policy's inference signature and returns z-scored ``[b, Q, A]`` chunks, so ``replay_bc(policy=..., store=...)`` evaluates it with
the code that evaluates the policy.

Deviations from the reference (also in README and DESIGN 5g): the features are the policy's trunk at its own resolution -- no
BYOL weights, no 120-pixel crop; qpos is z-scored, so the reference's hand-tuned state weights do not carry over and the default
1.0 is a choice, not a measurement; the weights come from the SORTED distances (the reference slices the unsorted matrix,
``pairwise_dist[:, :k]``, which its shipped k = 1 hides)."""
import numpy as np
import torch

from . import ops


def _engine_of(policy):
    eng = getattr(policy, "model", None)
    if eng is None or not hasattr(eng, "bind_features"):
        raise ValueError("VINN needs an ACT policy on the engine (policy.model.bind_features)")
    cfg = eng.cfg
    if getattr(cfg, "use_pcd", False) or getattr(policy, "use_pcd", False):
        raise ValueError("VINN: use_pcd policies are not supported (the lookup embeds camera frames)")
    return eng


def check_policy_class(policy_class, policy_config=None):
    """the policy classes the baseline refuses, before anything is built"""
    if policy_class == "Diffusion":
        raise ValueError("--replay_knn: the Diffusion policy has no ResNet trunk of this engine to embed frames with")
    if policy_config is not None and policy_config.get("use_pcd"):
        raise ValueError("--replay_knn: use_pcd policies are not supported (the lookup embeds camera frames)")


class TrunkFeatures:
    """The policy's trunk as an embedding: ``__call__(qpos, image, depth_img=None) -> [b, feature_dim]`` f32 (a view of one
    buffer that the next call overwrites).  The forward stops after the trunk and the token assembly
    (``set_forward_phase(1)``): the transformer, most of a small-batch step, is not run.  The engine's own feature binding and
    phase are put back after every call."""

    def __init__(self, engine, batch=None):
        self.engine = engine
        self.batch = int(batch or engine.max_batch)
        if not 1 <= self.batch <= engine.max_batch:
            raise ValueError(f"TrunkFeatures: batch {batch} outside [1, max_batch = {engine.max_batch}]")
        self.buf = torch.zeros((self.batch, engine.feature_dim), dtype=torch.float32, device=engine.device)
        self._a = torch.zeros((self.batch, engine.cfg.num_queries, engine.cfg.action_dim), dtype=torch.float32, device=engine.device)

    def __call__(self, qpos, image, depth_img=None):
        eng = self.engine
        b = int(qpos.shape[0])
        if b > self.batch:
            raise ValueError(f"TrunkFeatures: {b} frames for a buffer of {self.batch}")
        before, phase = eng.features_out, eng._phase
        kw = {}
        if eng.cfg.vq:                                          # (phase 1 never reads the code: any block of the right shape)
            kw["vq_sample"] = torch.zeros((b, eng.cfg.vq_class, eng.cfg.vq_dim), dtype=torch.float32, device=eng.device)
        if eng.cfg.use_depth:
            kw["depth_img"] = depth_img
        eng.bind_features(self.buf)
        eng.set_forward_phase(1)
        try:
            eng.forward_infer(qpos, image, out=self._a[:b], **kw)
        finally:
            eng.set_forward_phase(phase)
            eng.bind_features(before)
        return self.buf[:b]


class SupportSet:
    """The demonstrations a lookup searches, on the device: ``sv`` [Ns, Dv] trunk features, ``ss`` [Ns, S] the z-scored qpos rows
    the policy call receives, ``sep`` [Ns] int32 the episode id of every row (as the store was given it), ``off`` [Ns] int64 the
    row of ``store.actions`` the frame's chunk starts at and ``left`` [Ns] int32 the rows of its episode from there on."""

    def __init__(self, store, sv, ss, sep, off, left, episode_ids, align):
        self.store, self.sv, self.ss, self.sep, self.off, self.left = store, sv, ss, sep, off, left
        self.episode_ids, self.align = list(episode_ids), align

    def __len__(self):
        return int(self.sv.shape[0])

    @property
    def actions(self):
        return self.store.actions

    @classmethod
    def from_store(cls, store, policy, episode_ids=None, batch=None, align="train"):
        """Embed every frame of the store's episodes ``episode_ids`` (default: all it holds) with the policy's trunk, ``batch``
        frames at a time (default: the engine's max_batch) out of ``store.replay_batch``.  ``align``: "train" starts the chunk of
        frame t of a real-robot episode at action[max(0, t - 1)], as the dataset trains slot 0, "none" at action[t]."""
        if align not in ("train", "none"):
            raise ValueError(f"align must be 'train' or 'none', got {align!r}")
        if store is None:
            raise ValueError("VINN needs a DeviceEpisodeStore (--device_dataset): the support set is built from its frames")
        eng = _engine_of(policy)
        ids = list(store.episode_ids) if episode_ids is None else [int(i) for i in episode_ids]
        missing = [i for i in ids if i not in store._local_of]
        if not ids or missing:
            raise ValueError(f"SupportSet: episodes {missing or ids} are not in the store (it holds {list(store.episode_ids)})")
        feats = TrunkFeatures(eng, batch)
        dev = eng.device
        Ns = int(sum(int(store.T[store._local_of[i]]) for i in ids))
        sv = torch.empty((Ns, eng.feature_dim), dtype=torch.float32, device=dev)
        ss = torch.empty((Ns, int(store.qpos.shape[1])), dtype=torch.float32, device=dev)
        sep, off, left = (np.empty(Ns, dtype=dt) for dt in (np.int32, np.int64, np.int32))
        r = 0
        for i in ids:
            e = store._local_of[i]
            T, row0 = int(store.T[e]), int(store.row0[e])
            t = np.arange(T, dtype=np.int64)
            s = t if (align == "none" or bool(store.is_sim[e])) else np.maximum(t - 1, 0)
            sep[r:r + T], off[r:r + T], left[r:r + T] = i, row0 + s, T - s
            for b0 in range(0, T, feats.batch):
                data = store.replay_batch(e, t[b0:b0 + feats.batch])
                n = int(data[1].shape[0])
                sv[r + b0:r + b0 + n] = feats(data[1], data[0], data[2] if eng.cfg.use_depth else None)
                ss[r + b0:r + b0 + n] = data[1]
            r += T
        return cls(store, sv, ss, torch.from_numpy(sep).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(left).to(dev), ids,
                   align)


class VINNPolicy:
    """``__call__(qpos, image, depth_img=None) -> [b, Q, A]`` z-scored: trunk features of the frames, ``ops.knn_topk`` against
    the support set, ``ops.knn_predict`` out of the store's action rows.  ``set_exclude(episode_id)`` leaves that episode's rows
    out of every later lookup (leave-one-episode-out; None: none); ``exclude_self=True`` makes a replay do so for the episode it
    replays.  ``empty`` counts the queries that found no eligible row (a device word; ``empty_count()`` reads it)."""

    def __init__(self, support, k, state_weight=1.0, engine=None, exclude_self=False, stats=None):
        self.k, self.state_weight = ops.check_knn_args(k, state_weight, len(support))
        self.support = support
        self.model = engine if engine is not None else None
        if self.model is None or not hasattr(self.model, "bind_features"):
            raise ValueError("VINNPolicy needs the policy's engine (policy.model)")
        if self.model.cfg.use_pcd:
            raise ValueError("VINN: use_pcd policies are not supported (the lookup embeds camera frames)")
        if self.model.feature_dim != support.sv.shape[1]:
            raise ValueError(f"VINNPolicy: the engine embeds {self.model.feature_dim} values, the support rows hold {support.sv.shape[1]}")
        self.exclude_self = bool(exclude_self)
        self.use_depth, self.use_pcd = bool(self.model.cfg.use_depth), False
        self.num_queries = int(self.model.cfg.num_queries)
        stats = stats if stats is not None else getattr(support.store, "norm_stats", None)
        if stats is None:
            raise ValueError("VINNPolicy needs the action statistics (stats=, or a store that carries norm_stats)")
        self.mean = torch.as_tensor(np.asarray(stats["action_mean"], dtype=np.float64).reshape(-1), device=self.model.device)
        self.std = torch.as_tensor(np.asarray(stats["action_std"], dtype=np.float64).reshape(-1), device=self.model.device)
        self._features = TrunkFeatures(self.model)
        self._exclude = -1
        self._ex = torch.full((self._features.batch,), -1, dtype=torch.int32, device=self.model.device)
        self._ws = None
        self.empty = torch.zeros(1, dtype=torch.int32, device=self.model.device)

    def set_exclude(self, episode_id=None):
        self._exclude = -1 if episode_id is None else int(episode_id)
        self._ex.fill_(self._exclude)

    def empty_count(self):
        return int(self.empty.item())

    def neighbours(self, qpos, image, depth_img=None):
        sp = self.support
        qpos = qpos.to(torch.float32).contiguous()
        qv = self._features(qpos, image, depth_img)
        b = int(qv.shape[0])
        need = ops.knn_workspace_bytes(b, len(sp))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=qv.device)
        return ops.knn_topk(qv, qpos, sp.sv, sp.ss, self.k, self.state_weight, sp.sep, self._ex[:b] if self._exclude >= 0 else None,
                            ws=self._ws)

    def __call__(self, qpos, image, depth_img=None, **_ignored):
        sp = self.support
        idx, dist, n = self.neighbours(qpos, image, depth_img)
        chunk, _ = ops.knn_predict(idx, dist, n, self.k, sp.actions, sp.off, sp.left, self.num_queries, self.mean, self.std,
                                   empty=self.empty)
        return chunk

    def eval(self):
        return self

    def cuda(self):
        return self


def select_k(support, store, val_ids, Kmax, policy, state_weight=1.0, batch=None):
    """The device form of vinn_select_k.py: for every frame of the episodes ``val_ids`` of ``store`` (embedded like the support
    rows, the frame's own episode left out of its lookup) the ``Kmax`` nearest support rows once, then the squared error of slot
    0 of the prediction against the frame's z-scored action for every k = 1..Kmax at once (``ops.knn_ksweep``).
    -> {"mse": [Kmax] floats, "best_k": the argmin + 1, "count": frames}.  mse[k] = sse[k] / (count * A), pooled as sums and
    counts over the episodes; the reference averages per-batch means instead, which weights a ragged last batch differently."""
    Kmax, w = ops.check_knn_args(Kmax, state_weight, len(support))
    val = SupportSet.from_store(store, policy, val_ids, batch, support.align)
    A = int(store.actions.shape[1])
    mean, std = (np.asarray(store.norm_stats[k], dtype=np.float64).reshape(-1) for k in ("action_mean", "action_std"))
    m32, s32 = (torch.as_tensor(v.astype(np.float32), device=val.sv.device) for v in (mean, std))
    sse, count = np.zeros(Kmax), 0
    for i in val.episode_ids:
        rows = (val.sep == i).nonzero().reshape(-1)
        idx, dist, n = ops.knn_topk(val.sv[rows], val.ss[rows], support.sv, support.ss, Kmax, w, support.sep, val.sep[rows].contiguous())
        target = ((store.actions[val.off[rows]] - m32) / s32).contiguous()          # fp32, as the dataset z-scores its chunks
        sse = sse + ops.knn_ksweep(idx, dist, n, support.actions, support.off, target, mean, std).cpu().numpy()
        count += int(rows.numel())
    mse = sse / max(count * A, 1)
    return {"mse": mse.tolist(), "best_k": int(np.argmin(mse)) + 1, "count": count}
