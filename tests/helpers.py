"""Shared helpers for the parity tests (test infrastructure)."""
import json
import os

import numpy as np
import torch

from actmi.config import ACTConfig
from actmi import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg = ACTConfig(**json.loads(str(z["config_json"]))).validate()
    return z, cfg


def regenerate(z, cfg, with_actions=True):
    """Weights and inputs are regenerated from seeds; the fixture's hashes prove they are the same bytes."""
    import hashlib
    sd = W.generate_state_dict(cfg, int(z["seed_w"]))
    inp = W.generate_inputs(cfg, int(z["batch"]), int(z["seed_in"]), with_actions=with_actions)
    for k in z.files:
        if k.startswith("sha:"):
            name = k[4:]
            a = inp[name] if name in inp else sd[name]
            assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == str(z[k]), f"regenerated {name} differs"
    return sd, inp


def sample_like(a, z):
    m = int(z["sample_max_elems"])
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return W.fixture_sample(a, m) if m else a.reshape(-1)


def torch_sd(sd_np, prefix="model."):
    return {prefix + k: torch.from_numpy(v) for k, v in sd_np.items()}


def rel_err(got, exp):
    """max |got - exp| over max |exp|, in float64 on the CPU"""
    got, exp = got.detach().cpu().double(), exp.detach().cpu().double()
    return float((got - exp).abs().max() / (exp.abs().max() + 1e-30))


def host_mix32(x):
    """actmi_mix32 of csrc/dropout.h on a uint32 array (wrap-around arithmetic)"""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def host_u01(seed, idx):
    """actmi_u01(seed, idx) for an array of element indices: float32 in [0, 1) with 24 bits"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    h = host_mix32(lo ^ np.uint32(seed & 0xFFFFFFFF))
    h = host_mix32(h ^ hi ^ np.uint32(seed >> 32) ^ np.uint32(0x9E3779B9))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def host_keep(seed, idx, p):
    """Host transcription of actmi_keep(seed, idx, p) (csrc/dropout.h): a bool array, True = the element is kept.

    Pinned against the device through actmi_op_dropout for element indices 0 .. 100002 only: that op takes no index base, so the
    comparison covers the low word of the index alone.  The `hi` word path of actmi_u01 (indices at or above 2^32) is transcribed
    here but NOT proven against the device; every test that uses this mask stays below 2^32."""
    return host_u01(seed, idx) >= np.float32(p)


def gemm_desc(**kw):
    """an actmi_gemm_desc from keyword fields; tensors become their device addresses (the caller keeps them alive)"""
    from actmi import lib as L
    d = L.GemmDesc()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def run_gemm(what, **kw):
    """actmi_op_gemm on the current stream; RuntimeError with the library's message when the launch is rejected"""
    import ctypes as C
    from actmi import lib as L
    desc = gemm_desc(**kw)
    L.check(L.load().actmi_op_gemm(C.byref(desc), L.current_stream_ptr()), None, what)
