"""sr_network -- the pipeline's local super-resolution backend: a compact "VGG-style" SR network (the family Real-ESRGAN
ships as ``SRVGGNetCompact``: a 3x3 head convolution, D body convolutions F -> F each followed by a per-channel
activation, a 3x3 tail convolution to 3 s^2 channels, PixelShuffle, plus the nearest-upsampled input) run by the fp32 MFMA
kernels of csrc/sr_srnet.hip.

Weights are caller-supplied: nothing is fetched and none ship with the repository.  PARITY UNPINNED: neither the Real-ESRGAN
package nor a checkpoint exists offline; the arithmetic is written out in include/sr_hip.h and held against a torch-CPU
restatement (tests/_srnet_ref.py).

Parsing a state dict is host work (no GPU, no torch); the GPU model is made on first use."""
from __future__ import annotations

import re
from typing import Dict, Mapping, Optional

import numpy as np

import _native

ACT_SLOPES = {"prelu": None, "relu": 0.0, "leakyrelu": 0.1}
_KEY = re.compile(r"^body\.(\d+)\.(weight|bias)$")


def _unwrap(state: Mapping) -> Mapping:
    """A checkpoint saved as {'params_ema': state_dict} / {'params': state_dict} -> the state dict."""
    for k in ("params_ema", "params"):
        if k in state and isinstance(state[k], Mapping):
            return state[k]
    return state


def parse_state(state: Mapping, act: str = "prelu"):
    """-> (n_feat, n_body, scale, weights[D + 2], biases[D + 2], slopes[D + 1]) as contiguous fp32 arrays.

    ``body.{i}.weight`` with 4 dimensions is a convolution (taken in index order, ``body.{i}.bias`` its bias); a
    1-dimensional ``body.{i + 1}.weight`` of F values or one value holds that convolution's PReLU slopes, otherwise the
    slopes come from ``act`` ('relu' -> 0, 'leakyrelu' -> 0.1; 'prelu' then has nothing to take them from: ValueError).
    The last convolution is the tail; its 3 s^2 outputs give the scale."""
    if act not in ACT_SLOPES:
        raise ValueError(f"act must be one of {sorted(ACT_SLOPES)}, got {act!r}")
    state = _unwrap(state)
    entries: Dict[int, Dict[str, np.ndarray]] = {}
    for key in state:
        m = _KEY.match(str(key))
        if m:
            a = state[key]
            a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
            entries.setdefault(int(m.group(1)), {})[m.group(2)] = a
    convs = [i for i in sorted(entries) if entries[i].get("weight") is not None and entries[i]["weight"].ndim == 4]
    if len(convs) < 2:
        raise ValueError("SR network state needs at least a head and a tail convolution (body.{i}.weight with 4 dimensions)")
    weights, biases, slopes = [], [], []
    for n, i in enumerate(convs):
        w = np.ascontiguousarray(entries[i]["weight"], dtype=np.float32)
        if "bias" not in entries[i]:
            raise ValueError(f"SR network state lacks body.{i}.bias")
        b = np.ascontiguousarray(entries[i]["bias"], dtype=np.float32).reshape(-1)
        if w.shape[2:] != (3, 3):
            raise ValueError(f"body.{i}.weight: only 3x3 convolutions, got {w.shape}")
        if b.shape != (w.shape[0],):
            raise ValueError(f"body.{i}.bias: expected {w.shape[0]} values, got {b.shape}")
        want_cin = 3 if n == 0 else weights[-1].shape[0]
        if w.shape[1] != want_cin:
            raise ValueError(f"body.{i}.weight takes {w.shape[1]} channels but the layer before it gives {want_cin}")
        weights.append(w)
        biases.append(b)
        if n == len(convs) - 1:
            break                                               # the tail has no activation
        F = w.shape[0]
        nxt = entries.get(i + 1, {}).get("weight")
        if nxt is not None and nxt.ndim == 1 and nxt.size in (1, F):
            slopes.append(np.ascontiguousarray(np.broadcast_to(nxt.astype(np.float32), (F,))))
        elif ACT_SLOPES[act] is None:
            raise ValueError(f"act='prelu' but the state holds no slopes body.{i + 1}.weight of {F} values or one value")
        else:
            slopes.append(np.full(F, ACT_SLOPES[act], dtype=np.float32))
    n_feat, n_body = int(weights[0].shape[0]), len(weights) - 2
    if any(w.shape[0] != n_feat for w in weights[:-1]):
        raise ValueError("every convolution before the tail must have the same number of features")
    tail_c = int(weights[-1].shape[0])
    scale = int(round((tail_c / 3.0) ** 0.5))
    if tail_c != 3 * scale * scale or scale < 1:
        raise ValueError(f"the tail convolution has {tail_c} outputs, which is not 3 s^2 for an integer scale s")
    _native.srnet_plan(1, 1, n_feat, n_body, scale)             # NotImplementedError outside the kernels' range (host only)
    return n_feat, n_body, scale, weights, biases, slopes


def load_state(path: str) -> Mapping:
    """A flat .npz through numpy (allow_pickle=False: nothing in the file is executed); .pth / .pt through
    torch.load(weights_only=True, map_location='cpu') where torch imports."""
    p = str(path)
    if p.endswith((".pth", ".pt")):
        try:
            import torch
        except ImportError as exc:
            raise RuntimeError(f"{p}: loading a .pth / .pt checkpoint needs torch; convert it to a flat .npz instead") from exc
        return torch.load(p, weights_only=True, map_location="cpu")
    with np.load(p, allow_pickle=False) as z:
        return {k: np.asarray(z[k]) for k in z.files}


class CompactSRNet:
    """The compact SR network on the GPU.  ``state``: mapping of ``body.{i}.weight`` / ``body.{i}.bias`` arrays."""

    def __init__(self, state: Mapping, act: str = "prelu", device: int = 0):
        self.n_feat, self.n_body, self.scale, self._w, self._b, self._s = parse_state(state, act)
        self.act, self.device = act, int(device)
        self._models = {}                                       # one GPU model per context (a model lives on its stream)

    @classmethod
    def from_file(cls, path: str, act: str = "prelu", device: int = 0) -> "CompactSRNet":
        return cls(load_state(path), act=act, device=device)

    def model(self, ctx: Optional["_native.Context"] = None) -> "_native.SrNetModel":
        ctx = ctx or _native.default_context(self.device)
        m = self._models.get(id(ctx))
        if m is None or m.handle is None or m.ctx is not ctx:
            m = _native.SrNetModel(ctx, self.n_feat, self.n_body, self.scale, self._w, self._b, self._s)
            self._models[id(ctx)] = m
        return m

    @staticmethod
    def _check_image_shape(shape):
        if len(shape) != 3 or int(shape[2]) != 3:
            raise ValueError(f"the SR network takes h x w x 3 u8 images, got shape {tuple(shape)}")
        return int(shape[0]), int(shape[1])

    def upscale_device(self, d_src: int, shape, d_dst: int, dst_stride: int, src_stride: Optional[int] = None, tile: int = 0,
                       ctx: Optional["_native.Context"] = None):
        """h x w x 3 u8 at d_src (dense unless src_stride is given) -> (h s) x (w s) x 3 u8 at d_dst, HBM -> HBM.
        Asynchronous on the context's stream."""
        h, w = self._check_image_shape(shape)
        self.model(ctx).upscale_u8(d_src, w * 3 if src_stride is None else src_stride, h, w, d_dst, dst_stride, tile)

    def upscale(self, image: np.ndarray, tile: int = 0) -> np.ndarray:
        """Host array in, host array out."""
        image = np.asarray(image)
        h, w = self._check_image_shape(image.shape)
        if image.dtype != np.uint8:
            raise ValueError(f"the SR network takes u8 images, got {image.dtype}")
        s = self.scale
        ctx = _native.default_context(self.device)
        d_src, d_dst = ctx.upload(image), None
        try:
            d_dst = ctx.alloc(h * s * w * s * 3)
            self.upscale_device(d_src.ptr, (h, w, 3), d_dst.ptr, w * s * 3, tile=tile, ctx=ctx)
            return ctx.download(d_dst.ptr, (h * s, w * s, 3), np.uint8)
        finally:
            ctx.sync()
            d_src.free()
            if d_dst is not None:
                d_dst.free()

    def close(self):
        for m in self._models.values():
            m.close()
        self._models = {}
