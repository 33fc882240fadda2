"""compress_episode on the GPU: the files the device encoder writes are the host twin's byte for byte, and the written directory
feeds the compressed device store with the batches the host loader gives on it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import data as D  # noqa: E402
from actmi import ops  # noqa: E402
from test_device_dataset_cpu import write_dataset  # noqa: E402

DEV = "cuda:0"


def test_the_device_writes_the_host_twins_files_and_the_store_reads_them(tmp_path):
    cams, hw = ["top", "wrist"], (17, 33)
    raw = tmp_path / "raw"
    paths = write_dataset(raw, lengths=(12, 7, 3), cams=cams, hw=hw)
    dev_dir, host_dir = tmp_path / "raw_compressed", tmp_path / "host"
    os.makedirs(host_dir)
    written = D.compress_dataset_dir(str(raw), device=DEV)
    assert [os.path.basename(w) for w in written] == [os.path.basename(p) for p in paths]
    host_enc = ops.JpegHostEncoder(*hw)
    dev_enc = ops.JpegEncoder(DEV, *hw, max_frames=5)             # fewer slots than frames staged: more than one launch a piece
    for p in paths:
        name = os.path.basename(p)
        D.compress_episode(p, str(host_dir / name), encoder=host_enc)
        D.compress_episode(p, str(tmp_path / ("again_" + name)), encoder=dev_enc)
        with np.load(host_dir / name) as a, np.load(dev_dir / name) as b, np.load(tmp_path / ("again_" + name)) as c:
            assert sorted(a.files) == sorted(b.files) == sorted(c.files)
            for k in a.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (name, k)
    assert dev_enc.stats == {"frames": 2 * (12 + 7 + 3), "fallback": 0}
    kw = dict(policy_class="ACT", num_workers=0)
    host = D.load_data(str(dev_dir), lambda n: True, cams, 4, 3, 4, rng=np.random.default_rng(3), **kw)
    dev = D.load_data(str(dev_dir), lambda n: True, cams, 4, 3, 4, rng=np.random.default_rng(3), device_dataset=True, device=DEV,
                      device_decode=True, store_compressed=True, **kw)
    assert dev[0].store.store_compressed
    h_it, d_it = iter(host[0]), iter(dev[0])
    for _ in range(2):
        hb, db = next(h_it), next(d_it)
        assert len(hb) == len(db) == 4
        for h, d in zip(hb, db):
            assert d.is_cuda and torch.equal(h, d.cpu())
    dev[0].store.check_decoded()
