"""The decoder's cross-attention map, split by what the policy looked at.

Only decoder layer 0 reaches the action head, so the head-averaged weights ``tokens`` [B, Q, N] of its one
cross-attention are the policy's whole read of its observation: Q = num_queries action slots over the N memory tokens
``[latent, proprio, (pcl), rgb (h, cam, w) ..., depth (h, cam, w) ...]``.  The engine reports that order
(``ACTEngine.attention_layout()``, actmi_attention_layout); everything here works from the layout alone, on torch tensors
(on whatever device they live) and on numpy arrays alike.
"""
from collections import namedtuple

_Layout = namedtuple("AttentionLayout", "Q N n_extra K Kd fh fw")


class AttentionLayout(_Layout):
    """Q action slots, N tokens; n_extra tokens in front of the image tokens (2, or 3 with the point-cloud token); K RGB and
    Kd depth cameras of an fh x fw token grid each."""
    __slots__ = ()

    @staticmethod
    def from_config(cfg):
        fh, fw = cfg.feat_hw
        return AttentionLayout(cfg.num_queries, cfg.num_tokens, cfg.num_extra_tokens, cfg.num_cams, cfg.num_depth_cams, fh, fw)

    @property
    def rgb0(self):
        return self.n_extra

    @property
    def depth0(self):
        return self.n_extra + self.K * self.fh * self.fw

    def rgb_token(self, k, y, x):
        return self.rgb0 + (y * self.K + k) * self.fw + x

    def depth_token(self, k, y, x):
        return self.depth0 + (y * self.Kd + k) * self.fw + x

    @property
    def n_sources(self):
        return self.n_extra + self.K + self.Kd

    def check(self):
        if self.N != self.n_extra + (self.K + self.Kd) * self.fh * self.fw:
            raise ValueError(f"inconsistent attention layout {tuple(self)}")
        return self


def source_names(layout, camera_names=None, depth_camera_names=None):
    """one name per column of ``share``: latent, proprio, (cloud), every RGB camera, every depth camera"""
    cams = list(camera_names) if camera_names else [f"cam{k}" for k in range(layout.K)]
    dcams = list(depth_camera_names) if depth_camera_names else [f"cam{k}" for k in range(layout.Kd)]
    if len(cams) != layout.K or len(dcams) != layout.Kd:
        raise ValueError("camera names do not match the layout")
    return ["latent", "proprio"] + (["cloud"] if layout.n_extra == 3 else []) + [f"rgb:{c}" for c in cams] + \
           [f"depth:{c}" for c in dcams]


def check_slots(layout, slots):
    """(q0, q1) with 0 <= q0 < q1 <= Q; None: all slots"""
    if slots is None:
        return 0, layout.Q
    q0, q1 = (int(s) for s in slots)
    if not 0 <= q0 < q1 <= layout.Q:
        raise ValueError(f"attention slots {(q0, q1)} outside 0 <= q0 < q1 <= {layout.Q}")
    return q0, q1


def split_attention(tokens, layout, slots=None):
    """tokens [B, Q, N] -> dict(tokens, rgb [B, K, fh, fw], depth [B, Kd, fh, fw], extra [B, n_extra], share [B, n_sources]):
    the mean over the query slots [q0, q1) (default all), cut by the layout.  ``share`` is the attention mass per source --
    latent, proprio, (cloud), each RGB camera, each depth camera -- and every row of it sums to 1 (the rows of a softmax do)."""
    layout.check()
    B, Q, N = tokens.shape
    if (Q, N) != (layout.Q, layout.N):
        raise ValueError(f"tokens {tuple(tokens.shape)} do not match the layout's Q = {layout.Q}, N = {layout.N}")
    q0, q1 = check_slots(layout, slots)
    K, Kd, fh, fw, ne = layout.K, layout.Kd, layout.fh, layout.fw, layout.n_extra
    m = tokens[:, q0:q1].mean(1)                                           # [B, N]
    if hasattr(m, "permute"):                                              # torch
        import torch
        perm, cat = (lambda a: a.permute(0, 2, 1, 3)), (lambda xs: torch.cat(xs, 1))
    else:
        import numpy as np
        perm, cat = (lambda a: a.transpose(0, 2, 1, 3)), (lambda xs: np.concatenate(xs, 1))
    extra = m[:, :ne]
    rgb = perm(m[:, layout.rgb0:layout.depth0].reshape(B, fh, K, fw))      # token (y, k, x) -> [k][y][x]
    depth = perm(m[:, layout.depth0:].reshape(B, fh, Kd, fw))
    share = cat([extra, rgb.reshape(B, K, fh * fw).sum(2), depth.reshape(B, Kd, fh * fw).sum(2)])
    return {"tokens": tokens, "rgb": rgb, "depth": depth, "extra": extra, "share": share}
