#!/usr/bin/env python3
"""Generate tests/golden/vinn_knn.npz by running the REFERENCE's own ``calculate_nearest_neighbors`` (vinn_eval.py).

Authoring-container only: vinn_eval.py is loaded from /root/reference (read-only, never copied, never shipped) with name holders
for what it imports at module level and this path never calls (h5py, matplotlib, PIL, torchvision, einops, IPython and the
reference's own utils / sim_env / constants / imitate_episodes, which would pull in the simulator).  Only data is written.

The fixture: ONE query and 24 support rows per state weight in {0, 5}.  The support rows are stored PRE-SORTED by ascending
distance to the query: the reference weights its k nearest rows with ``pairwise_dist[:, :k]``, the distances of the FIRST k rows
rather than of the k nearest, so only on a pre-sorted support set is its output the intended algorithm for k > 1 (at its shipped
k = 1 the slip is invisible).  Neighbouring sorted distances differ by at least 1e-3 relative (checked here), so fp32 and float64
agree on the order.  Per weight w and k in {1, 3, 8}, without (``flat``) and with (``chunk``) a chunk axis:
  ref_*    the reference's fp32 torch result
  f64_*    the float64 statement: d = ||qv - sv|| + w ||qs - ss||, softmax(-d[:k]) weights, weighted sum
  gap_*    max |ref - f64|, the reference's own distance from exact arithmetic (``ref_vs_f64``)

Usage:  python tools/gen_golden_vinn.py [--check]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "vinn_knn.npz")
NS, DV, S, A, SKIP = 24, 32, 14, 4, 5
KS, WEIGHTS = (1, 3, 8), (0.0, 5.0)


def import_reference():
    holders = {"IPython": {"embed": lambda *a, **k: None}, "h5py": {}, "matplotlib": {}, "matplotlib.pyplot": {}, "PIL": {},
               "PIL.Image": {}, "torchvision": {}, "torchvision.transforms": {}, "einops": {"rearrange": None},
               "utils": {"set_seed": None, "sample_box_pose": None}, "sim_env": {"BOX_POSE": None}, "constants": {"DT": 0.02},
               "imitate_episodes": {"save_videos": None}}
    saved = {n: sys.modules.get(n) for n in holders}
    for name, attrs in holders.items():
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    try:
        spec = importlib.util.spec_from_file_location("_ref_vinn_eval", os.path.join(REF, "vinn_eval.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod.calculate_nearest_neighbors


def f64_statement(qv, qs, sv, ss, targets, k, w):
    d = np.linalg.norm(qv.astype(np.float64) - sv.astype(np.float64), axis=1) \
        + w * np.linalg.norm(qs.astype(np.float64) - ss.astype(np.float64), axis=1)
    e = np.exp(-(d[:k] - d[:k].min()))
    wts = e / e.sum()
    t = targets.astype(np.float64)
    return np.tensordot(wts, t[:k], axes=(0, 0))[None], d


def build(seed=20240):
    fn = import_reference()
    out = {"ks": np.asarray(KS, dtype=np.int32), "weights": np.asarray(WEIGHTS, dtype=np.float64)}
    for wi, w in enumerate(WEIGHTS):
        rng = np.random.default_rng(seed + wi)
        qv, qs = rng.standard_normal((1, DV)).astype(np.float32), rng.standard_normal((1, S)).astype(np.float32)
        # rows at growing distance from the query, so that the sorted distances are well apart
        radius = np.linspace(0.3, 2.5, NS)[:, None]
        sv = (qv + radius * rng.standard_normal((NS, DV)) / np.sqrt(DV)).astype(np.float32)
        ss = (qs + radius * rng.standard_normal((NS, S)) / np.sqrt(S)).astype(np.float32)
        targets = (rng.standard_normal((NS, SKIP, A)) * 2 + 0.5).astype(np.float32)
        _, d = f64_statement(qv[0], qs[0], sv, ss, targets, NS, w)
        order = np.argsort(d, kind="stable")
        sv, ss, targets, d = sv[order], ss[order], targets[order], d[order]
        rel = np.diff(d) / d[1:]
        assert rel.min() >= 1e-3, f"weight {w}: neighbouring sorted distances only {rel.min():.2e} apart; choose another seed"
        tag = f"w{wi}"
        out.update({f"{tag}_qv": qv, f"{tag}_qs": qs, f"{tag}_sv": sv, f"{tag}_ss": ss, f"{tag}_targets": targets, f"{tag}_d64": d})
        tq = (torch.from_numpy(qv), torch.from_numpy(qs))
        ts = (torch.from_numpy(sv), torch.from_numpy(ss))
        for k in KS:
            for form, tg in (("flat", targets[:, 0]), ("chunk", targets)):
                with torch.no_grad():
                    ref = fn(tq, ts, torch.from_numpy(np.ascontiguousarray(tg)), k, w).numpy()
                exact, _ = f64_statement(qv[0], qs[0], sv, ss, tg, k, w)
                assert ref.shape == exact.shape and ref.dtype == np.float32
                out[f"{tag}_k{k}_{form}_ref"] = ref
                out[f"{tag}_k{k}_{form}_f64"] = exact
                out[f"{tag}_k{k}_{form}_gap"] = np.float64(np.abs(ref.astype(np.float64) - exact).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    args = ap.parse_args()
    out = build()
    if args.check:
        z = np.load(OUT)
        assert sorted(z.files) == sorted(out), "keys differ"
        for k in z.files:
            assert np.array_equal(z[k], out[k]), k
        print("vinn_knn.npz matches")
        return
    np.savez(OUT, **out)
    for k in sorted(out):
        if k.endswith("_gap"):
            print(f"{k}: {float(out[k]):.3e}")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
