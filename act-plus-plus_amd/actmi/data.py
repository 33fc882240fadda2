"""Input pipeline of the ACT training loop: the reference's ``utils.py`` dataset logic feeding the
accelerated step.

Mirrors, with the reference's names and argument meaning:
``get_norm_stats`` (utils.py:176-224), ``find_all_hdf5`` (:226-235), ``BatchSampler`` (:237-247),
``EpisodicDataset`` (:41-174; ``_locate_transition``, ``__getitem__``) and ``load_data`` (:249-301).

Differences, all on the host side of the step:
* images stay **u8 NHWC** ``[C, H, W, 3]`` (the engine's fast input format; the ``/255`` and the ImageNet normalisation are
  fused into the conv1 loader) — ``f32_images=True`` reproduces the reference contract (f32 ``[C, 3, H, W]`` in [0, 1]);
* depth frames (``use_depth``; ``/observations/depth_images/<cam>``) stay **raw uint16** ``[Cd, 1, H, W]`` when the episode
  stores an unsigned integer of at most 16 bits: the engine finds every sample's min / max on the device and fuses the
  reference's per-sample ``(d - min) / (max - min + 1e-6)`` into the depth stem's loader -- ``f32_depth=True`` (and any other
  stored dtype) reproduces the reference contract, f32 normalised on the host;
* point clouds (``use_pcd``; the fork's ``/observations/pointcloud/<name>/{xyz, rgb, padding_mask}``, one fused cloud) come
  with their **valid count**: the recorder pads every frame's cloud with zero rows up to the episode's largest, and the stored
  ``padding_mask`` (True = a point) says how many rows are points.  The fork's dataset ignores the mask, so its policy sees the
  zero rows as points; here the mask is honoured unless ``pcd_ignore_mask=True``, because the live cloud of deployment has no
  padding.  ``collate_pcd`` pads a batch's clouds with zero rows to the batch's largest stored row count and the batch becomes
  the 7-tuple ``(image, qpos, action, is_pad, pcd_xyz [B, P, 3] f32, pcd_rgb [B, P, 3] f32, pcd_n [B] int32)``; the engine
  takes the maximum over the first ``pcd_n`` rows of every sample only;
* batches are collated into **pinned** buffers and handed to the device by ``DevicePrefetcher`` on a side stream while
  the previous step computes (the reference moves 944 MB of f32 images per batch-64 step synchronously);
* episode files are opened through ``open_episode``: HDF5 via ``h5py`` when it is importable (the reference's format:
  ``/observations/qpos``, ``/observations/qvel``, ``/observations/images/<cam>``, ``/action``, optional ``/base_action``,
  attrs ``sim`` / ``compress``), or ``.npz`` files with the same keys (``attrs_sim`` / ``attrs_compress`` entries) — what
  the tests use, since neither h5py nor cv2 exists in the build container;
* compressed episodes (attr ``compress``: every frame a zero-padded JPEG byte string, utils.py:104-107) are decoded with PIL
  (libjpeg, like cv2) and flipped to the B, G, R channel order ``cv2.imdecode(buf, 1)`` returns -- **parity unpinned** against
  cv2 itself (absent here); the Diffusion-only augmentations (torchvision transforms, utils.py:141-156) are not handled.
  Everything else is checked against an independent restatement in ``tests/test_data_pipeline_cpu.py``;
* ``EpisodeReplay`` reads ONE episode in time order for the open-loop replay evaluation (``imitate_episodes.replay_bc``): the
  same tensors as ``EpisodicDataset.__getitem__`` without the action chunk, in batches of consecutive steps;
* ``DeviceEpisodeStore`` (``load_data(..., device_dataset=True)``, opt-in) reads every episode ONCE into a device arena; a
  training batch is then two device gathers (three with depth) that give the tensors of ``EpisodicDataset.__getitem__`` + the
  default collation bit for bit, with no host work, loader worker or PCIe traffic per step;
* ``DeviceEpisodeReplay`` is ``EpisodeReplay`` out of such a store (``DeviceEpisodeStore.replay_batch``): one stored episode in
  time order, the same tensors bit for bit, already on the device -- what ``--replay_every`` replays while training;
* ``load_data(..., mirror_twins=True)`` joins every episode file by its **mirrored twin** (``MirrorTwinPath``, ``MirrorSpec``): the
  episode the reference's ``postprocess_episodes.py`` writes beside it -- arms swapped with a per-joint sign vector, the base's
  turn rate negated, the wrist cameras swapped and flipped, the top camera flipped -- computed from the file as it is read
  instead of stored.  Two deviations from the reference's files: the twin is the exact mirror image (the script re-encodes every
  mirrored frame as JPEG at quality 50) and its rows are float32.  Depth cameras, which the reference does not mirror, follow
  their RGB camera.  In a ``DeviceEpisodeStore`` a twin shares its source's frames: ``actmi_op_gather_frames_mirror`` flips them
  inside the batch's gather;
* ``load_data(..., device_clouds=True)`` (with ``device_dataset`` and ``use_pcd``, opt-in) puts the stored clouds into the store as
  well: the device loaders then deliver ``collate_pcd``'s 7-tuples, the clouds gathered by ``actmi_op_gather_clouds``; and a stored
  cloud gets a **mirror rule** (``MirrorTwinPath(..., cloud_mirror=(axis, offset))``, ``load_data(..., cloud_mirror=...)``: one
  coordinate reflected across a plane of the clouds' frame), with which ``mirror_twins`` and ``use_pcd`` go together, on the host
  loader and in the store alike.

* ``compress_episode`` (``compress_data.py``) turns a raw episode into a compressed one, its frames encoded on the device
  (``episode_compress``; actmi_op_jpeg_encode writes libjpeg-turbo's bytes).

What reads an episode file (``open_episode``, the mirror views, ``find_all_hdf5``) lives in ``episode_files`` and the store with its
loaders in ``episode_store``; both are imported here by name, so ``actmi.data.<name>`` keeps resolving for every one of them."""
import numpy as np
import torch

from .episode_files import (MirrorSpec, MirrorTwinPath, _EpisodeArrays, _entry_meta, _list_hdf5, _MirrorCloud, _MirrorEpisode,  # noqa: F401
                            _MirrorFrames, _NpzEpisode, _read_action, cloud_mirror_rule, find_all_hdf5, find_all_hdf5_with_twins,
                            imdecode_bgr, mirror_cloud_xyz, mirror_twin_paths, open_episode, preprocess_base_action)
from .episode_store import (ARENA_ALIGN, DEVICE_STORE_RESERVE_BYTES, DeviceBatchLoader, DeviceEpisodeReplay,  # noqa: F401
                            DeviceEpisodeStore, arena_layout, locate_transitions, stored_cloud_counts)
from .episode_compress import compress_dataset_dir, compress_episode  # noqa: F401


def get_norm_stats(dataset_path_list):
    all_qpos, all_action, all_episode_len = [], [], []
    qpos = None
    for dataset_path in dataset_path_list:
        with open_episode(dataset_path) as root:
            qpos = np.asarray(root["/observations/qpos"][()])
            action = np.asarray(_read_action(root))
        all_qpos.append(torch.from_numpy(qpos))
        all_action.append(torch.from_numpy(action))
        all_episode_len.append(len(qpos))
    all_qpos = torch.cat(all_qpos, dim=0)
    all_action = torch.cat(all_action, dim=0)
    action_mean = all_action.mean(dim=[0]).float()
    action_std = torch.clip(all_action.std(dim=[0]).float(), 1e-2, np.inf)
    qpos_mean = all_qpos.mean(dim=[0]).float()
    qpos_std = torch.clip(all_qpos.std(dim=[0]).float(), 1e-2, np.inf)
    action_min = all_action.min(dim=0).values.float()
    action_max = all_action.max(dim=0).values.float()
    eps = 0.0001
    stats = {"action_mean": action_mean.numpy(), "action_std": action_std.numpy(),
             "action_min": action_min.numpy() - eps, "action_max": action_max.numpy() + eps,
             "qpos_mean": qpos_mean.numpy(), "qpos_std": qpos_std.numpy(), "example_qpos": qpos}
    return stats, all_episode_len


def BatchSampler(batch_size, episode_len_l, sample_weights, rng=None):
    """utils.py:237-247; ``rng`` (a ``numpy.random.Generator`` or the ``numpy.random`` module) makes it reproducible."""
    rng = rng or np.random
    sample_probs = np.array(sample_weights) / np.sum(sample_weights) if sample_weights is not None else None
    sum_dataset_len_l = np.cumsum([0] + [np.sum(episode_len) for episode_len in episode_len_l])
    randint = rng.integers if hasattr(rng, "integers") else rng.randint
    while True:
        batch = []
        for _ in range(batch_size):
            episode_idx = rng.choice(len(episode_len_l), p=sample_probs)
            batch.append(int(randint(sum_dataset_len_l[episode_idx], sum_dataset_len_l[episode_idx + 1])))
        yield batch


# ---------------------------------------------------------------------------------------------------------------------
# dataset
# ---------------------------------------------------------------------------------------------------------------------
class EpisodicDataset(torch.utils.data.Dataset):
    """utils.py:41-174.  ``__getitem__`` returns (image, qpos, action, is_pad); image is u8 ``[C,H,W,3]`` unless
    ``f32_images``.  With ``use_depth`` (the fork's depth dataset) a fifth entry follows: the frames of ``depth_camera_names``,
    raw uint16 ``[Cd,1,H,W]`` when the episode stores an unsigned integer of at most 16 bits, else (or with ``f32_depth``)
    float32 normalised by the sample's own minimum and maximum over all depth cameras.  With ``use_pcd`` (the fork's point-cloud
    dataset, utils_arm_gripper_all.py:90-99, 153-156) three entries follow the first four instead: xyz ``[N, 3]`` and rgb ``[N, 3]``
    float32 (colours stay 0..255) of the one cloud in ``pointcloud_names``, every stored row of it, and the int64 scalar ``n``, the
    number of rows that are points (the stored ``padding_mask``'s count, or N without a mask or with ``pcd_ignore_mask``); batch
    such samples with ``collate_pcd``."""

    def __init__(self, dataset_path_list, camera_names, norm_stats, episode_ids, episode_len, chunk_size, policy_class,
                 f32_images=False, depth_camera_names=None, use_depth=False, f32_depth=False, pointcloud_names=None, use_pcd=False,
                 max_points=None, pcd_ignore_mask=False):
        self.episode_ids = episode_ids
        self.dataset_path_list = dataset_path_list
        self.camera_names = camera_names
        self.norm_stats = norm_stats
        self.episode_len = episode_len
        self.chunk_size = chunk_size
        self.cumulative_len = np.cumsum(self.episode_len)
        self.max_episode_len = max(episode_len)
        self.policy_class = policy_class
        self.f32_images = f32_images
        self.use_depth = bool(use_depth)
        self.depth_camera_names = list(depth_camera_names) if depth_camera_names else []
        self.f32_depth = f32_depth
        if self.use_depth and not self.depth_camera_names:
            raise ValueError("use_depth needs depth_camera_names (the task config's list of /observations/depth_images/<cam>)")
        self.use_pcd = bool(use_pcd)
        self.pointcloud_names = list(pointcloud_names) if pointcloud_names else []
        self.max_points = None if max_points is None else int(max_points)
        self.pcd_ignore_mask = bool(pcd_ignore_mask)
        if self.use_pcd:
            if len(self.pointcloud_names) != 1:
                # the fork's training step takes the one fused cloud (train_single_arm_gripper_all.py:576-591)
                raise ValueError(f"use_pcd needs exactly one pointcloud name (/observations/pointcloud/<name>), got "
                                 f"{self.pointcloud_names}")
            if self.use_depth:
                raise NotImplementedError("use_depth together with use_pcd is not supported")
            if any(isinstance(p, MirrorTwinPath) and getattr(p, "cloud_mirror", None) is None for p in dataset_path_list):
                raise ValueError("use_pcd with mirror twins: a stored point cloud has no mirror rule (MirrorTwinPath(..., "
                                 "cloud_mirror=(axis, offset)) gives it one)")
        if policy_class == "Diffusion":
            raise NotImplementedError("the Diffusion augmentations (torchvision transforms) are outside this path")
        self._stats_t = {k: torch.as_tensor(np.asarray(norm_stats[k]), dtype=torch.float32)
                         for k in ("action_mean", "action_std", "qpos_mean", "qpos_std")}
        self.is_sim = False          # utils.py:59 (the reference overwrites what __getitem__ observed)

    def __len__(self):
        return int(self.cumulative_len[-1])

    def _locate_transition(self, index):
        assert index < self.cumulative_len[-1]
        episode_index = int(np.argmax(self.cumulative_len > index))       # first True
        start_ts = int(index - (self.cumulative_len[episode_index] - self.episode_len[episode_index]))
        return self.episode_ids[episode_index], start_ts

    def __getitem__(self, index):
        episode_id, start_ts = self._locate_transition(index)
        dataset_path = self.dataset_path_list[episode_id]
        with open_episode(dataset_path) as root:
            attrs = root.attrs
            is_sim = bool(attrs["sim"]) if "sim" in attrs else False         # legacy data lacks the attribute
            compressed = bool(attrs.get("compress", False))
            action = np.asarray(_read_action(root))
            original_action_shape = action.shape
            episode_len = original_action_shape[0]
            qpos = np.asarray(root["/observations/qpos"][start_ts])
            images = [np.asarray(root[f"/observations/images/{cam}"][start_ts]) for cam in self.camera_names]
            depths = [np.asarray(root[f"/observations/depth_images/{cam}"][start_ts]) for cam in self.depth_camera_names] \
                if self.use_depth else None
            cloud = self._read_cloud(root, start_ts, dataset_path) if self.use_pcd else None
        if compressed:                                            # utils.py:104-107
            images = [imdecode_bgr(buf) for buf in images]
            if depths is not None:                                # three equal channels of an 8-bit decode; channel 0 is kept below
                depths = [imdecode_bgr(buf) for buf in depths]
        if is_sim:
            action = action[start_ts:]
            action_len = episode_len - start_ts
        else:                                                     # "hack, to make timesteps more aligned" (utils.py:112-114)
            action = action[max(0, start_ts - 1):]
            action_len = episode_len - max(0, start_ts - 1)
        padded_action = np.zeros((self.max_episode_len, original_action_shape[1]), dtype=np.float32)
        padded_action[:action_len] = action
        is_pad = np.zeros(self.max_episode_len)
        is_pad[action_len:] = 1
        padded_action = padded_action[:self.chunk_size]
        is_pad = is_pad[:self.chunk_size]
        image_data = torch.from_numpy(np.stack(images, axis=0))                # [C,H,W,3] u8
        qpos_data = torch.from_numpy(qpos).float()
        action_data = torch.from_numpy(padded_action).float()
        is_pad = torch.from_numpy(is_pad).bool()
        if self.f32_images:
            image_data = torch.einsum("k h w c -> k c h w", image_data) / 255.0
        t = self._stats_t
        action_data = (action_data - t["action_mean"]) / t["action_std"]
        qpos_data = (qpos_data - t["qpos_mean"]) / t["qpos_std"]
        if depths is not None:
            return image_data, qpos_data, action_data, is_pad, self._depth_data(depths)
        if cloud is not None:
            return (image_data, qpos_data, action_data, is_pad) + cloud
        return image_data, qpos_data, action_data, is_pad

    def _read_cloud(self, root, start_ts, dataset_path):
        """the cloud of one sample: (xyz [N, 3] f32, rgb [N, 3] f32, n) -- every stored row, and how many of them are points"""
        base = f"/observations/pointcloud/{self.pointcloud_names[0]}"
        xyz = np.asarray(root[f"{base}/xyz"][start_ts])
        rgb = np.asarray(root[f"{base}/rgb"][start_ts])
        where = f"{dataset_path} (timestep {start_ts})"
        if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
            raise ValueError(f"{where}: point cloud xyz {xyz.shape} / rgb {rgb.shape}, expected two [N, 3] arrays")
        N = xyz.shape[0]
        n = N
        if not self.pcd_ignore_mask and f"{base}/padding_mask" in root:
            mask = np.asarray(root[f"{base}/padding_mask"][start_ts]).astype(bool).reshape(-1)
            if mask.shape[0] != N:
                raise ValueError(f"{where}: padding_mask of {mask.shape[0]} rows for a cloud of {N}")
            n = int(mask.sum())
            if not mask[:n].all():                                 # the recorder writes the points first, then the zero rows
                raise ValueError(f"{where}: padding_mask is not a prefix (True rows first): the valid points cannot be given as a count")
        if n == 0:
            raise ValueError(f"{where}: the point cloud has no valid point")
        if self.max_points is not None and N > self.max_points:
            raise ValueError(f"{where}: the point cloud stores {N} rows, more than max_points {self.max_points} (no silent truncation: "
                             "raise --max_points or down-sample the recording)")
        return (torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)),       # .float(), utils_arm_gripper_all.py:153-156
                torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.float32)), torch.tensor(n, dtype=torch.int64))

    def _depth_data(self, depths):
        """the depth frames of one sample -> [Cd, 1, H, W]: a 3-D frame keeps channel 0; raw uint16 for the device-side
        normalisation, or the reference's float32 (d - min) / (max - min + 1e-6) over all depth cameras of the sample"""
        d = np.stack([f[:, :, 0] if f.ndim == 3 else f for f in depths], axis=0)[:, None]
        if not self.f32_depth and d.dtype.kind == "u" and d.dtype.itemsize <= 2:
            return torch.from_numpy(np.ascontiguousarray(d, dtype=np.uint16))
        d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))        # torch.from_numpy(...).float(), utils_arm_gripper_all.py:147
        return (d - d.min()) / (d.max() - d.min() + 1e-6)


def collate_pcd(samples):
    """Batches the 7-entry samples of a ``use_pcd`` dataset: the first four entries as the default collation does, the clouds padded
    with ZERO rows to the batch's largest stored row count P (episodes differ in theirs) -> (image, qpos, action, is_pad,
    pcd_xyz [B, P, 3] f32, pcd_rgb [B, P, 3] f32, pcd_n [B] int32)."""
    from torch.utils.data import default_collate
    head = default_collate([s[:4] for s in samples])
    B, P = len(samples), max(int(s[4].shape[0]) for s in samples)
    xyz, rgb = torch.zeros((B, P, 3), dtype=torch.float32), torch.zeros((B, P, 3), dtype=torch.float32)
    for b, s in enumerate(samples):
        xyz[b, :s[4].shape[0]] = s[4]
        rgb[b, :s[5].shape[0]] = s[5]
    n = torch.tensor([int(s[6]) for s in samples], dtype=torch.int32)
    return tuple(head) + (xyz, rgb, n)

class EpisodeReplay:
    """One recorded episode in time order, for open-loop replay: iterating gives batches of ``batch`` consecutive replayed steps
    (the last one ragged) in the layout the policy's inference call takes, the tensors of ``EpisodicDataset.__getitem__`` for the
    same steps without the action chunk: ``(image u8 [b, K, H, W, 3], qpos f32 [b, S] z-scored)``, then with ``use_depth`` the
    depth frames ``[b, Cd, 1, H, W]`` (raw uint16 where the episode stores them so), or with ``use_pcd`` ``(xyz [b, N, 3] f32,
    rgb [b, N, 3] f32, n [b] int32)`` through ``_read_cloud``'s rules.  Compressed episodes are decoded with ``imdecode_bgr``.
    Nothing is augmented.  ``stride``: only the steps 0, stride, 2 * stride, ... are replayed (a policy without temporal
    ensembling is queried once per chunk).  ``batch`` is the caller's: the clouds of a 4096-point batch of 50 are 16 MB.

    ``.actions`` [T, A] f32 in file units (with ``/base_action`` appended as the dataset does), ``.is_sim``, ``.T``, ``.steps``."""

    def __init__(self, dataset_path, camera_names, norm_stats, batch, depth_camera_names=None, use_depth=False, f32_depth=False,
                 pointcloud_names=None, use_pcd=False, max_points=None, pcd_ignore_mask=False, stride=1):
        self.dataset_path, self.batch, self.stride = dataset_path, int(batch), int(stride)
        if self.batch < 1 or self.stride < 1:
            raise ValueError(f"batch {batch} and stride {stride} must be at least 1")
        with open_episode(dataset_path) as root:
            attrs = root.attrs
            self.is_sim = bool(attrs["sim"]) if "sim" in attrs else False
            self.compressed = bool(attrs.get("compress", False))
            self.actions = np.ascontiguousarray(_read_action(root), dtype=np.float32)
        self.T = int(self.actions.shape[0])
        self.steps = list(range(0, self.T, self.stride))
        # the switches, their checks and the per-sample depth / cloud rules are the dataset's
        self._ds = EpisodicDataset([dataset_path], camera_names, norm_stats, [0], [self.T], 1, "ACT", False, depth_camera_names,
                                   use_depth, f32_depth, pointcloud_names, use_pcd, max_points, pcd_ignore_mask)

    def __len__(self):
        return (len(self.steps) + self.batch - 1) // self.batch

    def __iter__(self):
        ds = self._ds
        t = ds._stats_t
        with open_episode(self.dataset_path) as raw:
            root = _EpisodeArrays(raw)
            for b0 in range(0, len(self.steps), self.batch):
                steps = self.steps[b0:b0 + self.batch]
                sel = slice(steps[0], steps[-1] + 1) if self.stride == 1 else steps
                qpos = torch.from_numpy(np.asarray(root["/observations/qpos"][sel])).float()
                frames = [np.asarray(root[f"/observations/images/{cam}"][sel]) for cam in ds.camera_names]
                if self.compressed:                            # utils.py:104-107, frame by frame
                    frames = [np.stack([imdecode_bgr(buf) for buf in f]) for f in frames]
                out = [torch.from_numpy(np.stack(frames, axis=1)), (qpos - t["qpos_mean"]) / t["qpos_std"]]
                if ds.use_depth:
                    depths = [np.asarray(root[f"/observations/depth_images/{cam}"][sel]) for cam in ds.depth_camera_names]
                    if self.compressed:
                        depths = [np.stack([imdecode_bgr(buf) for buf in d]) for d in depths]
                    out.append(torch.stack([ds._depth_data([d[i] for d in depths]) for i in range(len(steps))]))
                if ds.use_pcd:
                    clouds = [ds._read_cloud(root, ts, self.dataset_path) for ts in steps]
                    out += [torch.stack([c[0] for c in clouds]), torch.stack([c[1] for c in clouds]),
                            torch.tensor([int(c[2]) for c in clouds], dtype=torch.int32)]
                yield tuple(out)


def flatten_list(l):
    return [item for sublist in l for item in sublist]


def load_data(dataset_dir_l, name_filter, camera_names, batch_size_train, batch_size_val, chunk_size,
              skip_mirrored_data=False, load_pretrain=False, policy_class=None, stats_dir_l=None, sample_weights=None,
              train_ratio=0.99, num_workers=2, f32_images=False, rng=None, depth_camera_names=None, use_depth=False,
              f32_depth=False, pointcloud_names=None, use_pcd=False, max_points=None, pcd_ignore_mask=False,
              device_dataset=False, device=None, device_budget_bytes=None, mirror_twins=False, mirror_spec=None,
              device_clouds=False, cloud_mirror=None, device_decode=False,
              store_compressed=False, rows_per_mark=1, store_encode=False, encode_quality=50, encode_subsampling="420",
              depth_pack=False):
    """utils.py:249-301.  Returns (train_dataloader, val_dataloader, norm_stats, is_sim).  ``use_depth``: the batches are
    5-tuples that end in the depth frames of ``depth_camera_names`` (EpisodicDataset).  ``use_pcd``: 7-tuples that end in the
    padded clouds and their valid counts (collate_pcd).  ``device_dataset``: both loaders come from ONE ``DeviceEpisodeStore``
    on ``device`` (default: the current cuda device) that holds the train and validation episodes; the split, the norm stats
    and the samplers are built as without the flag, so the same ``rng`` gives the same episodes and the same draws, and the
    batches are the same tensors, already on the device (``loader.on_device``).  ``mirror_twins``: every episode file is joined by
    its mirrored twin (``MirrorTwinPath``; ``mirror_spec`` None: the reference's rule for the cameras each file holds), computed
    from the file as it is read -- the results are those of the same call without the flag on a directory in which the twin files
    exist (uncompressed, float32 rows): the same episode ids, stats, draws and batches.  With ``device_dataset`` the twins take no
    frame memory.  ``cloud_mirror`` ``(axis, offset)``: the mirror rule of the stored clouds (``cloud_mirror_rule``), which
    ``mirror_twins`` with ``use_pcd`` needs.  ``device_clouds``: the stored clouds of a ``use_pcd`` dataset go into the store as well
    and the device loaders deliver the 7-tuples of ``collate_pcd``, gathered by ``actmi_op_gather_clouds``.  ``device_decode``: the store
    decodes the frames of compressed episodes on the device (``DeviceEpisodeStore``); the batches are the same bytes.
    ``store_encode`` (with ``store_compressed``): raw episodes are encoded on the device as the store reads them, at
    ``encode_quality`` / ``encode_subsampling``; the batches are those of a compressed store of ``compress_dataset_dir``'s output.
    ``depth_pack`` (with ``store_encode`` and ``use_depth``): the raw uint16 depth of raw episodes is packed losslessly on the device
    and unpacked for every batch (``DeviceEpisodeStore``); the depth tensors are those of the decoded store."""
    if depth_pack and not store_encode:
        raise ValueError("depth_pack packs the raw depth of episodes the store encodes as it loads them: it needs store_encode "
                         "(and store_compressed, device_decode, device_dataset)")
    if depth_pack and not use_depth:
        raise ValueError("depth_pack packs depth frames: it needs use_depth")
    if device_decode and not device_dataset:
        raise ValueError("device_decode decodes the compressed frames of the device-resident store: it needs device_dataset")
    if store_compressed and not (device_dataset and device_decode):
        raise ValueError("store_compressed keeps the device-resident store's frames compressed and decodes every batch on the device: "
                         "it needs device_dataset and device_decode")
    if store_encode and not store_compressed:
        raise ValueError("store_encode encodes raw episodes into the store that stays compressed: it needs store_compressed (and "
                         "device_dataset, device_decode)")
    if mirror_twins and use_pcd and cloud_mirror is None:
        raise ValueError("mirror_twins with use_pcd: a stored point cloud has no mirror rule (cloud_mirror=(axis, offset) gives it one)")
    if cloud_mirror is not None:
        if not (mirror_twins and use_pcd):
            raise ValueError("cloud_mirror is the mirror rule of the stored clouds of mirror_twins with use_pcd")
        cloud_mirror = cloud_mirror_rule(cloud_mirror)[:2]
    if device_clouds and not (device_dataset and use_pcd):
        raise ValueError("device_clouds puts the stored clouds of a use_pcd dataset into the device-resident store: it needs "
                         "device_dataset and use_pcd")
    if device_dataset:                                            # refused before any file is read
        if use_pcd and not device_clouds:
            raise NotImplementedError("--device_dataset with use_pcd: point clouds through the device-resident store are not "
                                      "implemented (ragged clouds stay on the host loader); drop --device_dataset")
        if policy_class not in (None, "ACT"):
            raise NotImplementedError(f"--device_dataset: the device-resident store feeds the ACT training path, not {policy_class!r}")
        if f32_images or f32_depth:
            raise NotImplementedError("--device_dataset keeps raw u8 frames and raw uint16 depth: f32_images / f32_depth belong to "
                                      "the host loader")
    rng = rng or np.random
    if isinstance(dataset_dir_l, str):
        dataset_dir_l = [dataset_dir_l]
    if mirror_twins:
        # depth camera i shares the swap and the flip of RGB camera i (the config demands one depth camera per RGB camera)
        follows = dict(zip(depth_camera_names or [], camera_names)) if use_depth else None

        def list_files(d):
            return find_all_hdf5_with_twins(d, skip_mirrored_data, mirror_spec, follows, cloud_mirror)
    else:
        def list_files(d):
            return find_all_hdf5(d, skip_mirrored_data)
    dataset_path_list_list = [list_files(d) for d in dataset_dir_l]
    num_episodes_0 = len(dataset_path_list_list[0])
    dataset_path_list = [n for n in flatten_list(dataset_path_list_list) if name_filter(n)]
    num_episodes_l = [len(l) for l in dataset_path_list_list]
    num_episodes_cumsum = np.cumsum(num_episodes_l)
    shuffled_episode_ids_0 = rng.permutation(num_episodes_0)
    train_episode_ids_0 = shuffled_episode_ids_0[:int(train_ratio * num_episodes_0)]
    val_episode_ids_0 = shuffled_episode_ids_0[int(train_ratio * num_episodes_0):]
    train_episode_ids_l = [train_episode_ids_0] + [np.arange(n) + num_episodes_cumsum[idx]
                                                   for idx, n in enumerate(num_episodes_l[1:])]
    val_episode_ids_l = [val_episode_ids_0]
    train_episode_ids = np.concatenate(train_episode_ids_l)
    val_episode_ids = np.concatenate(val_episode_ids_l)
    print(f"\n\nData from: {dataset_dir_l}\n- Train on {[len(x) for x in train_episode_ids_l]} episodes\n"
          f"- Test on {[len(x) for x in val_episode_ids_l]} episodes\n\n")
    _, all_episode_len = get_norm_stats(dataset_path_list)
    train_episode_len_l = [[all_episode_len[i] for i in ids] for ids in train_episode_ids_l]
    val_episode_len_l = [[all_episode_len[i] for i in ids] for ids in val_episode_ids_l]
    train_episode_len = flatten_list(train_episode_len_l)
    val_episode_len = flatten_list(val_episode_len_l)
    if stats_dir_l is None:
        stats_dir_l = dataset_dir_l
    elif isinstance(stats_dir_l, str):
        stats_dir_l = [stats_dir_l]
    norm_stats, _ = get_norm_stats(flatten_list([list_files(d) for d in stats_dir_l]))
    print(f"Norm stats from: {stats_dir_l}")
    pcd_kw = dict(pointcloud_names=pointcloud_names, use_pcd=use_pcd, max_points=max_points, pcd_ignore_mask=pcd_ignore_mask)
    train_dataset = EpisodicDataset(dataset_path_list, camera_names, norm_stats, train_episode_ids, train_episode_len,
                                    chunk_size, policy_class, f32_images, depth_camera_names, use_depth, f32_depth, **pcd_kw)
    val_dataset = EpisodicDataset(dataset_path_list, camera_names, norm_stats, val_episode_ids, val_episode_len,
                                  chunk_size, policy_class, f32_images, depth_camera_names, use_depth, f32_depth, **pcd_kw)
    if device_dataset:
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        store = DeviceEpisodeStore(dataset_path_list, np.concatenate([train_episode_ids, val_episode_ids]), camera_names, norm_stats,
                                   device, depth_camera_names, use_depth, device_budget_bytes, use_pcd, policy_class,
                                   device_decode=device_decode, store_compressed=store_compressed, rows_per_mark=rows_per_mark,
                                   store_encode=store_encode, encode_quality=encode_quality, encode_subsampling=encode_subsampling,
                                   depth_pack=depth_pack,
                                   **(dict(pointcloud_names=pointcloud_names, max_points=max_points, pcd_ignore_mask=pcd_ignore_mask)
                                      if device_clouds else {}))
        train_loader = store.loader(train_episode_ids, train_episode_len, chunk_size,
                                    BatchSampler(batch_size_train, train_episode_len_l, sample_weights, rng))
        val_loader = store.loader(val_episode_ids, val_episode_len, chunk_size, BatchSampler(batch_size_val, val_episode_len_l, None, rng))
        return train_loader, val_loader, norm_stats, train_dataset.is_sim
    from torch.utils.data import DataLoader
    kw = dict(pin_memory=torch.cuda.is_available(), num_workers=num_workers)
    if num_workers > 0:
        kw["prefetch_factor"] = 2
    if use_pcd:
        kw["collate_fn"] = collate_pcd
    train_dataloader = DataLoader(train_dataset, batch_sampler=BatchSampler(batch_size_train, train_episode_len_l,
                                                                             sample_weights, rng), **kw)
    val_dataloader = DataLoader(val_dataset, batch_sampler=BatchSampler(batch_size_val, val_episode_len_l, None, rng), **kw)
    return train_dataloader, val_dataloader, norm_stats, train_dataset.is_sim


# ---------------------------------------------------------------------------------------------------------------------
# host -> device hand-off
# ---------------------------------------------------------------------------------------------------------------------
class DevicePrefetcher:
    """Wraps an iterable of host batches (tuples of tensors): batch i+1 is copied to the device on a side stream
    (from pinned memory, ``non_blocking``) while the caller computes on batch i; ``__next__`` makes the compute stream
    wait for the copy it is about to use.  On a CPU-only host it degrades to the plain iterable (tests)."""

    def __init__(self, iterable, device=None, depth=2):
        self.it = iter(iterable)
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        self.cuda = self.device is not None and self.device.type == "cuda"
        self.stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.queue = []
        self.depth = max(1, int(depth))
        for _ in range(self.depth):
            self._push()

    def _push(self):
        try:
            batch = next(self.it)
        except StopIteration:
            return
        if not self.cuda:
            self.queue.append((batch, None))
            return
        with torch.cuda.stream(self.stream):
            staged = tuple(t if t.is_pinned() else t.pin_memory() for t in batch)
            dev = tuple(t.to(self.device, non_blocking=True) for t in staged)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.queue.append((dev, ev))

    def __iter__(self):
        return self

    def __next__(self):
        if not self.queue:
            raise StopIteration
        batch, ev = self.queue.pop(0)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            for t in batch:
                t.record_stream(torch.cuda.current_stream(self.device))
        self._push()
        return batch
