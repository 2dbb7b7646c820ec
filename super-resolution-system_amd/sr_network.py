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
    torch.load(weights_only=True, map_location='cpu') where torch imports; .safetensors through safetensors.numpy.load_file
    where safetensors imports (a local file: nothing is fetched)."""
    p = str(path)
    if p.endswith(".safetensors"):
        try:
            from safetensors.numpy import load_file
        except ImportError as exc:
            raise RuntimeError(f"{p}: loading a .safetensors checkpoint needs the safetensors package; convert it to a flat .npz instead") from exc
        return dict(load_file(p))
    if p.endswith((".pth", ".pt")):
        try:
            import torch
        except ImportError as exc:
            raise RuntimeError(f"{p}: loading a .pth / .pt checkpoint needs torch; convert it to a flat .npz instead") from exc
        return torch.load(p, weights_only=True, map_location="cpu")
    with np.load(p, allow_pickle=False) as z:
        return {k: np.asarray(z[k]) for k in z.files}


ENSEMBLE_MASKS = {1: 0x01, 2: 0x03, 4: 0x0F, 8: 0xFF}            # members of the geometric self-ensemble (include/sr_hip.h)


def ensemble_mask(ensemble) -> int:
    """``ensemble`` (1: off, 2: identity + horizontal flip, 4: the four flips, 8: all of D4) -> the mask of sr_<kind>_ens_*.
    Anything else is a ValueError."""
    if isinstance(ensemble, (bool, np.bool_)) or not isinstance(ensemble, (int, np.integer)) or int(ensemble) not in ENSEMBLE_MASKS:
        raise ValueError(f"ensemble must be one of {sorted(ENSEMBLE_MASKS)}, got {ensemble!r}")
    return ENSEMBLE_MASKS[int(ensemble)]


class CompactSRNet:
    """The compact SR network on the GPU.  ``state``: mapping of ``body.{i}.weight`` / ``body.{i}.bias`` arrays."""

    def __init__(self, state: Mapping, act: str = "prelu", device: int = 0):
        self.n_feat, self.n_body, self.scale, self._w, self._b, self._s = parse_state(state, act)
        self.act, self.device = act, int(device)
        self._models = {}                                       # one GPU model per context (a model lives on its stream)

    @classmethod
    def from_file(cls, path: str, act: str = "prelu", device: int = 0) -> "CompactSRNet":
        return cls(load_state(path), act=act, device=device)

    def _make_model(self, ctx: "_native.Context"):
        return _native.SrNetModel(ctx, self.n_feat, self.n_body, self.scale, self._w, self._b, self._s)

    def model(self, ctx: Optional["_native.Context"] = None):
        """The family's _native model on ``ctx`` (the device's default context if None), made on first use."""
        ctx = ctx or _native.default_context(self.device)
        m = self._models.get(id(ctx))
        if m is None or m.handle is None or m.ctx is not ctx:
            m = self._models[id(ctx)] = self._make_model(ctx)
        return m

    @staticmethod
    def _check_image_shape(shape):
        if len(shape) != 3 or int(shape[2]) != 3:
            raise ValueError(f"the SR network takes h x w x 3 u8 images, got shape {tuple(shape)}")
        return int(shape[0]), int(shape[1])

    def upscale_device(self, d_src: int, shape, d_dst: int, dst_stride: int, src_stride: Optional[int] = None, tile: int = 0,
                       ctx: Optional["_native.Context"] = None, ensemble: int = 1, **run):
        """h x w x 3 u8 at d_src (dense unless src_stride is given) -> (h s) x (w s) x 3 u8 at d_dst, HBM -> HBM.
        Asynchronous on the context's stream.  ``run``: what the family's forward takes beside ``tile`` (RRDBSRNet: ``tail``).
        ``ensemble``: 1 (the plain forward), or 2 / 4 / 8 members of the geometric self-ensemble (ensemble_mask)."""
        mask = ensemble_mask(ensemble)
        h, w = self._check_image_shape(shape)
        if mask == 1:
            self.model(ctx).upscale_u8(d_src, w * 3 if src_stride is None else src_stride, h, w, d_dst, dst_stride, tile, **run)
        else:
            self.model(ctx).ensemble_u8(d_src, w * 3 if src_stride is None else src_stride, h, w, d_dst, dst_stride, tile, mask=mask, **run)

    def upscale(self, image: np.ndarray, tile: int = 0, ensemble: int = 1, **run) -> np.ndarray:
        """Host array in, host array out."""
        ensemble_mask(ensemble)
        image = np.asarray(image)
        h, w = self._check_image_shape(image.shape)
        if image.dtype != np.uint8:
            raise ValueError(f"the SR network takes u8 images, got {image.dtype}")
        s = self.scale
        ctx = _native.default_context(self.device)
        d_src, d_dst = ctx.upload(image), None
        try:
            d_dst = ctx.alloc(h * s * w * s * 3)
            self.upscale_device(d_src.ptr, (h, w, 3), d_dst.ptr, w * s * 3, tile=tile, ctx=ctx, ensemble=ensemble, **run)
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


# ------------------------------------------------------------------------------------------
# The residual family: BasicSR's MSRResNet (SRResNet without batch norm) and EDSR, run by csrc/sr_resnet.hip.
# PARITY UNPINNED here too: neither the BasicSR package nor a checkpoint exists offline; the arithmetic is written out in
# include/sr_hip.h and held against a torch-CPU restatement (tests/_resnet_ref.py).
# ------------------------------------------------------------------------------------------
EDSR_RGB_MEAN = (0.4488, 0.4371, 0.4040)                        # BasicSR's defaults (DIV2K)
EDSR_IMG_RANGE = 255.0
_BLOCK_KEY = re.compile(r"^body\.(\d+)\.(conv1|conv2)\.(weight|bias)$")
_UPSAMPLE_KEY = re.compile(r"^upsample\.(\d+)\.weight$")


def _array(state: Mapping, key: str) -> np.ndarray:
    a = state[key]
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _read_conv(state: Mapping, keys, name: str, cin: int, cout, cin_text: str, refuse=None):
    """-> (weight, bias) of the 3x3 convolution ``name`` as contiguous fp32, every shape checked; a ValueError names the
    offending key.  ``cin_text`` ends the message about a wrong input width; ``refuse(w)`` may raise before that check."""
    for part in ("weight", "bias"):
        if f"{name}.{part}" not in keys:
            raise ValueError(f"{name}.{part}: not in the state")
    w = np.ascontiguousarray(_array(state, f"{name}.weight"), dtype=np.float32)
    b = np.ascontiguousarray(_array(state, f"{name}.bias"), dtype=np.float32).reshape(-1)
    if w.ndim != 4 or w.shape[2:] != (3, 3):
        raise ValueError(f"{name}.weight: only 3x3 convolutions, got shape {w.shape}")
    if refuse is not None:
        refuse(w)
    if w.shape[1] != cin:
        raise ValueError(f"{name}.weight takes {w.shape[1]} channels{cin_text.format(cin)}")
    if cout is not None and w.shape[0] != cout:
        raise ValueError(f"{name}.weight gives {w.shape[0]} channels, expected {cout}")
    if b.shape != (w.shape[0],):
        raise ValueError(f"{name}.bias: expected {w.shape[0]} values, got {b.shape}")
    return w, b


def _scalar_extras(state: Mapping, spec) -> dict:
    """The constants a .npz holds beside the state dict: ``spec`` is (key, number of values) pairs; one value comes back as
    a float, several as a tuple."""
    out = {}
    if not isinstance(state, Mapping):
        return out
    for key, size in spec:
        if key in state:
            a = np.asarray(_array(state, key), dtype=np.float64).reshape(-1)
            if a.size != size:
                raise ValueError(f"{key}: expected {size} value{'s' if size > 1 else ''}, got shape {np.shape(_array(state, key))}")
            out[key] = tuple(a.tolist()) if size > 1 else float(a[0])
    return out


def parse_residual_state(state: Mapping, res_scale: float = 1.0, img_range: float = EDSR_IMG_RANGE, rgb_mean=EDSR_RGB_MEAN):
    """-> (_native.ResNetDesc, weights, biases) in sr_resnet_create's order, contiguous fp32.

    BasicSR key names: ``conv_first``, ``body.{i}.conv1`` / ``body.{i}.conv2``, then either MSRResNet's ``upconv1`` (and
    ``upconv2`` at scale 4), ``conv_hr``, ``conv_last`` -- or EDSR's ``conv_after_body``, ``upsample.{k}``, ``conv_last``.
    ``conv_after_body.weight`` tells the two apart.  res_scale, img_range and rgb_mean are not in a state dict: they apply to
    EDSR only (MSRResNet: 1, range 1, mean 0).  Every shape is checked; a ValueError names the offending key."""
    state = _unwrap(state)
    keys = {str(k) for k in state}
    if "conv_first.weight" not in keys:
        raise ValueError("conv_first.weight: not in the state (not a residual SR network)")
    if RCAN_KEY in keys:                                         # its body.{g}.* keys would read as an EDSR of zero blocks
        raise ValueError(f"{RCAN_KEY}: this is an RCAN state (parse_rcan_state), not a residual SR network")
    if SWINIR_KEY in keys:
        raise ValueError(f"{SWINIR_KEY}: this is a SwinIR state (parse_swinir_state), not a residual SR network")
    convs = []                                                 # (key, cout or None for 'any multiple', cin)

    def conv(name: str, cin: int, cout=None):
        convs.append(_read_conv(state, keys, name, cin, cout, " but the layer before it gives {}"))
        return convs[-1][0]

    F = int(conv("conv_first", 3).shape[0])
    blocks = sorted({int(m.group(1)) for m in map(_BLOCK_KEY.match, keys) if m})
    if blocks != list(range(len(blocks))):
        raise ValueError(f"body.{len(blocks)}.conv1.weight: residual blocks must be numbered 0 .. B - 1, got {blocks}")
    for i in blocks:
        conv(f"body.{i}.conv1", F, F)
        conv(f"body.{i}.conv2", F, F)
    edsr = "conv_after_body.weight" in keys
    if edsr:
        conv("conv_after_body", F, F)
        ups = [f"upsample.{k}" for k in sorted(int(m.group(1)) for m in map(_UPSAMPLE_KEY.match, keys) if m)
               if _array(state, f"upsample.{k}.weight").ndim == 4]
    else:
        ups = [n for n in ("upconv1", "upconv2") if f"{n}.weight" in keys or f"{n}.bias" in keys]
        if ups == ["upconv2"]:
            raise ValueError("upconv1.weight: not in the state, but upconv2 is")
    if len(ups) > 2:
        raise ValueError(f"{ups[2]}.weight: at most two upsampling stages (scale 4)")
    scale = 1
    for name in ups:
        cout = int(np.shape(_array(state, f"{name}.weight"))[0]) if f"{name}.weight" in keys else 0
        r = {4 * F: 2, 9 * F: 3}.get(cout)
        if r is None or (len(ups) == 2 and r != 2):
            want = f"{4 * F}" if len(ups) == 2 else f"{4 * F} or {9 * F}"
            raise ValueError(f"{name}.weight gives {cout} channels, expected F r^2 = {want}")
        conv(name, F, cout)
        scale *= r
    if not edsr:
        conv("conv_hr", F, F)
    conv("conv_last", F, 3)
    if edsr:
        desc = _native.resnet_desc(F, len(blocks), scale, long_skip=True, res_scale=float(res_scale), mean=rgb_mean, range=float(img_range))
    else:
        desc = _native.resnet_desc(F, len(blocks), scale, conv_hr=True, bilinear_base=True, a_head=0.1, a_up=0.1, a_hr=0.1)
    _native.resnet_plan(desc, 1, 1)                              # NotImplementedError outside the kernels' range (host only)
    return desc, [w for w, _ in convs], [b for _, b in convs]


class ResidualSRNet(CompactSRNet):
    """MSRResNet / EDSR on the GPU, with CompactSRNet's surface (from_file, model, upscale, upscale_device, close).
    ``state``: a BasicSR state dict (see parse_residual_state)."""

    def __init__(self, state: Mapping, res_scale: float = 1.0, img_range: float = EDSR_IMG_RANGE, rgb_mean=EDSR_RGB_MEAN, device: int = 0):
        self.desc, self._w, self._b = parse_residual_state(state, res_scale, img_range, rgb_mean)
        self.n_feat, self.n_blocks, self.scale = self.desc.n_feat, self.desc.n_blocks, self.desc.scale
        self.preset = "edsr" if self.desc.long_skip else "msrresnet"
        self.device = int(device)
        self._models = {}

    @classmethod
    def from_file(cls, path: str, device: int = 0, **extras) -> "ResidualSRNet":
        """A .npz may hold the EDSR constants a state dict lacks as 0-d ``res_scale`` / ``img_range`` and 3-vector ``rgb_mean``
        entries; keyword arguments win over them, BasicSR's defaults stand in for the rest."""
        state = load_state(path)
        return cls(state, device=device, **{**_residual_extras(state), **extras})

    def _make_model(self, ctx: "_native.Context"):
        return _native.ResNetModel(ctx, self.desc, self._w, self._b)


def _residual_extras(state: Mapping) -> dict:
    return _scalar_extras(state, (("res_scale", 1), ("img_range", 1), ("rgb_mean", 3)))


# ------------------------------------------------------------------------------------------
# RRDBNet: BasicSR's ESRGAN / Real-ESRGAN x4 generator (RealESRGAN_x4plus: 23 blocks, RealESRGAN_x4plus_anime_6B: 6), run by
# csrc/sr_rrdb.hip.  PARITY UNPINNED here too: neither the BasicSR / Real-ESRGAN packages nor a checkpoint exist offline; the
# arithmetic is written out in include/sr_hip.h and held against a torch-CPU restatement (tests/_rrdb_ref.py).
# ------------------------------------------------------------------------------------------
RRDB_KEY = "body.0.rdb1.conv1.weight"                           # what tells an RRDBNet state from the residual family
_RRDB_BLOCK_KEY = re.compile(r"^body\.(\d+)\.rdb[123]\.conv[1-5]\.(weight|bias)$")


def parse_rrdb_state(state: Mapping, slope: float = 0.2, res_scale: float = 0.2):
    """-> (_native.RrdbDesc, weights, biases) in sr_rrdb_create's order, contiguous fp32.

    BasicSR key names: ``conv_first``, ``body.{i}.rdb{1,2,3}.conv{1..5}``, ``conv_body``, ``conv_up1``, ``conv_up2``,
    ``conv_hr``, ``conv_last``.  slope and res_scale are not in a state dict (BasicSR hard-codes 0.2 for both).  Every shape is
    checked; a ValueError names the offending key.  The x2 / x1 variants, whose ``conv_first`` takes the 12 / 48 channels of a
    pixel-unshuffle, are refused with NotImplementedError."""
    state = _unwrap(state)
    keys = {str(k) for k in state}
    if "conv_first.weight" not in keys:
        raise ValueError("conv_first.weight: not in the state (not an RRDB network)")
    convs = []

    def unshuffled(w):
        if w.shape[1] in (12, 48):
            raise NotImplementedError(f"conv_first.weight takes {w.shape[1]} channels: the x{2 if w.shape[1] == 12 else 1} RRDBNet puts a "
                                      "pixel-unshuffle in front of conv_first, which is not supported (x4 only)")

    def conv(name: str, cin: int, cout=None):
        convs.append(_read_conv(state, keys, name, cin, cout, ", expected {}", unshuffled if name == "conv_first" else None))
        return convs[-1][0]

    F = int(conv("conv_first", 3).shape[0])
    blocks = sorted({int(m.group(1)) for m in map(_RRDB_BLOCK_KEY.match, keys) if m})
    if blocks != list(range(len(blocks))):
        gap = next(i for i in range(len(blocks) + 1) if i not in blocks)
        raise ValueError(f"body.{gap}.rdb1.conv1.weight: RRDBs must be numbered 0 .. B - 1, got {blocks}")
    G = None
    for i in blocks:
        for d in (1, 2, 3):
            for k in range(1, 5):
                name = f"body.{i}.rdb{d}.conv{k}"
                if G is None:
                    if f"{name}.weight" not in keys:
                        raise ValueError(f"{name}.weight: not in the state")
                    G = int(np.shape(_array(state, f"{name}.weight"))[0])
                conv(name, F + (k - 1) * G, G)                   # every convolution 1 .. 4 has the first one's growth
            conv(f"body.{i}.rdb{d}.conv5", F + 4 * G, F)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, F, F)
    conv("conv_last", F, 3)
    desc = _native.rrdb_desc(F, 32 if G is None else G, len(blocks), 4, float(slope), float(res_scale))
    _native.rrdb_plan(desc, 1, 1)                                # NotImplementedError outside the kernels' range (host only)
    return desc, [w for w, _ in convs], [b for _, b in convs]


class RRDBSRNet(CompactSRNet):
    """RRDBNet x4 on the GPU, with CompactSRNet's surface (from_file, model, upscale, upscale_device, close) plus the tail
    phase's ``tail``.  ``state``: a BasicSR state dict (see parse_rrdb_state)."""

    def __init__(self, state: Mapping, slope: float = 0.2, res_scale: float = 0.2, device: int = 0):
        self.desc, self._w, self._b = parse_rrdb_state(state, slope, res_scale)
        self.n_feat, self.n_grow, self.n_blocks, self.scale = self.desc.n_feat, self.desc.n_grow, self.desc.n_blocks, self.desc.scale
        self.device = int(device)
        self._models = {}

    @classmethod
    def from_file(cls, path: str, device: int = 0, **extras) -> "RRDBSRNet":
        """A .npz may hold the two constants a state dict lacks as 0-d ``slope`` / ``res_scale`` entries; keyword arguments win
        over them, BasicSR's 0.2 stands in for the rest."""
        state = load_state(path)
        return cls(state, device=device, **{**_rrdb_extras(state), **extras})

    def _make_model(self, ctx: "_native.Context"):
        return _native.RrdbModel(ctx, self.desc, self._w, self._b)


def _rrdb_extras(state: Mapping) -> dict:
    return _scalar_extras(state, (("slope", 1), ("res_scale", 1)))


# ------------------------------------------------------------------------------------------
# RCAN: BasicSR's residual channel attention network (Zhang et al., ECCV 2018), run by csrc/sr_rcan.hip.  PARITY UNPINNED here
# too: neither the BasicSR package nor a checkpoint exists offline; the arithmetic is written out in include/sr_hip.h and held
# against a torch-CPU restatement (tests/_rcan_ref.py).
# ------------------------------------------------------------------------------------------
RCAN_KEY = "body.0.residual_group.0.rcab.0.weight"              # what tells an RCAN state from the residual family
_RCAN_BLOCK_KEY = re.compile(r"^body\.(\d+)\.residual_group\.(\d+)\.rcab\.")
_RCAN_GROUP_KEY = re.compile(r"^body\.(\d+)\.")


def _read_1x1(state: Mapping, keys, name: str, cout: int, cin: int):
    """-> (weight (cout, cin), bias) of the 1 x 1 convolution ``name`` as contiguous fp32; a ValueError names the offending key."""
    for part in ("weight", "bias"):
        if f"{name}.{part}" not in keys:
            raise ValueError(f"{name}.{part}: not in the state")
    w = np.ascontiguousarray(_array(state, f"{name}.weight"), dtype=np.float32)
    b = np.ascontiguousarray(_array(state, f"{name}.bias"), dtype=np.float32).reshape(-1)
    if w.shape != (cout, cin, 1, 1):
        raise ValueError(f"{name}.weight: expected the 1x1 convolution {(cout, cin, 1, 1)}, got shape {w.shape}")
    if b.shape != (cout,):
        raise ValueError(f"{name}.bias: expected {cout} values, got {b.shape}")
    return np.ascontiguousarray(w.reshape(cout, cin)), b


def parse_rcan_state(state: Mapping, res_scale: float = 1.0, img_range: float = EDSR_IMG_RANGE, rgb_mean=EDSR_RGB_MEAN):
    """-> (_native.RcanDesc, weights, biases) in sr_rcan_create's order, contiguous fp32 (the 1 x 1 layers as (out, in)).

    BasicSR key names: ``conv_first``, per group g and block b ``body.{g}.residual_group.{b}.rcab.0`` / ``.rcab.2`` (3 x 3) and
    ``.rcab.3.attention.1`` / ``.attention.3`` (1 x 1, F -> F / r -> F), ``body.{g}.conv``, then ``conv_after_body``,
    ``upsample.{k}``, ``conv_last``.  The squeeze width is read off ``attention.1``.  Groups and blocks are numbered from 0
    without gaps and every group has the same number of blocks.  res_scale, img_range and rgb_mean are not in a state dict.
    Every shape is checked; a ValueError names the offending key; what the kernels do not cover (F, more than 16 groups, x8) is
    a NotImplementedError."""
    state = _unwrap(state)
    keys = {str(k) for k in state}
    if "conv_first.weight" not in keys:
        raise ValueError("conv_first.weight: not in the state (not an RCAN)")
    tables = []

    def conv(name: str, cin: int, cout=None):
        tables.append(_read_conv(state, keys, name, cin, cout, ", expected {}"))
        return tables[-1][0]

    F = int(conv("conv_first", 3).shape[0])
    groups = sorted({int(m.group(1)) for m in map(_RCAN_GROUP_KEY.match, keys) if m})
    if not groups or groups != list(range(len(groups))):
        gap = next(i for i in range(len(groups) + 1) if i not in groups)
        raise ValueError(f"body.{gap}.conv.weight: residual groups must be numbered 0 .. G - 1, got {groups}")
    B = R = None
    for g in groups:
        blocks = sorted({int(m.group(2)) for m in map(_RCAN_BLOCK_KEY.match, keys) if m and int(m.group(1)) == g})
        if blocks != list(range(len(blocks))):
            gap = next(i for i in range(len(blocks) + 1) if i not in blocks)
            raise ValueError(f"body.{g}.residual_group.{gap}.rcab.0.weight: a group's blocks must be numbered 0 .. B - 1, got {blocks}")
        if B is None:
            B = len(blocks)
        elif len(blocks) != B:
            raise ValueError(f"body.{g}.residual_group.{min(len(blocks), B)}.rcab.0.weight: every group must have the same number of "
                             f"blocks, group 0 has {B} and group {g} has {len(blocks)}")
        for b in blocks:
            name = f"body.{g}.residual_group.{b}.rcab"
            conv(f"{name}.0", F, F)
            conv(f"{name}.2", F, F)
            if R is None:
                if f"{name}.3.attention.1.weight" not in keys:
                    raise ValueError(f"{name}.3.attention.1.weight: not in the state")
                R = int(np.shape(_array(state, f"{name}.3.attention.1.weight"))[0])
            tables.append(_read_1x1(state, keys, f"{name}.3.attention.1", R, F))
            tables.append(_read_1x1(state, keys, f"{name}.3.attention.3", F, R))
        conv(f"body.{g}.conv", F, F)
    conv("conv_after_body", F, F)
    ups = [f"upsample.{k}" for k in sorted(int(m.group(1)) for m in map(_UPSAMPLE_KEY.match, keys) if m)
           if _array(state, f"upsample.{k}.weight").ndim == 4]
    scale = 1
    for name in ups:
        cout = int(np.shape(_array(state, f"{name}.weight"))[0])
        r = {4 * F: 2, 9 * F: 3}.get(cout)
        if r is None or (len(ups) >= 2 and r != 2):
            want = f"{4 * F}" if len(ups) >= 2 else f"{4 * F} or {9 * F}"
            raise ValueError(f"{name}.weight gives {cout} channels, expected F r^2 = {want}")
        scale *= r
    if len(ups) <= 2:                                            # beyond that the plan call below refuses the scale by name
        for name in ups:
            conv(name, F, None)
        conv("conv_last", F, 3)
    desc = _native.rcan_desc(F, max(1, F // 16) if R is None else R, len(groups), B, scale, float(res_scale), rgb_mean, float(img_range))
    _native.rcan_plan(desc, 1, 1)                                # NotImplementedError outside the kernels' range (host only)
    return desc, [w for w, _ in tables], [b for _, b in tables]


class _OnePieceSRNet(CompactSRNet):
    """What RCANSRNet, SwinIRSRNet and HATSRNet share: the trunk is one piece, so there is no ``tile``, only ``tail``.
    ``_one_piece``: the family's sentence about it, with which a tile is refused."""
    _one_piece = ""

    def upscale_device(self, d_src: int, shape, d_dst: int, dst_stride: int, src_stride: Optional[int] = None, tile: int = 0,
                       ctx: Optional["_native.Context"] = None, ensemble: int = 1, tail: int = 0):
        if tile:
            raise ValueError(f"{self._one_piece}: there is no tile, got tile={tile!r}; see tail")
        # the one argument after the strides of sr_<kind>_* is tail, and CompactSRNet hands its first one on by position
        super().upscale_device(d_src, shape, d_dst, dst_stride, src_stride, tail, ctx, ensemble)


class RCANSRNet(_OnePieceSRNet):
    """RCAN on the GPU, with CompactSRNet's surface (from_file, model, upscale, upscale_device, close).  ``state``: a BasicSR
    state dict (see parse_rcan_state).

    Every RCAB pools each channel over the whole image it is given, so the image is not streamed through the trunk: there is
    no ``tile`` (anything but 0 is refused), only the ``tail`` of the upsampling phase, which changes no bit.  It also means
    that an image cut into tiles before the network (as the pipeline does with ``block_size``) pools over each tile on its own
    -- as every tiled inference of RCAN does -- so the tile size affects the values, not only the speed."""

    _one_piece = "RCAN's trunk is one piece (the channel mean is global)"

    def __init__(self, state: Mapping, res_scale: float = 1.0, img_range: float = EDSR_IMG_RANGE, rgb_mean=EDSR_RGB_MEAN, device: int = 0):
        self.desc, self._w, self._b = parse_rcan_state(state, res_scale, img_range, rgb_mean)
        d = self.desc
        self.n_feat, self.n_squeeze, self.n_groups, self.n_blocks, self.scale = d.n_feat, d.n_squeeze, d.n_groups, d.n_blocks, d.scale
        self.device = int(device)
        self._models = {}

    @classmethod
    def from_file(cls, path: str, device: int = 0, **extras) -> "RCANSRNet":
        """A .npz may hold the constants a state dict lacks as 0-d ``res_scale`` / ``img_range`` and 3-vector ``rgb_mean``
        entries; keyword arguments win over them, BasicSR's defaults (1, 255, the DIV2K mean) stand in for the rest."""
        state = load_state(path)
        return cls(state, device=device, **{**_residual_extras(state), **extras})

    def _make_model(self, ctx: "_native.Context"):
        return _native.RcanModel(ctx, self.desc, self._w, self._b)


# ------------------------------------------------------------------------------------------
# SwinIR: BasicSR's shifted-window transformer for image restoration (Liang et al., ICCVW 2021), run by csrc/sr_swinir.hip.
# PARITY UNPINNED here too: neither the BasicSR package, the official repository nor a checkpoint exists offline; the arithmetic
# is written out in include/sr_hip.h and held against a torch-CPU restatement (tests/_swinir_ref.py).
# ------------------------------------------------------------------------------------------
SWINIR_KEY = "layers.0.residual_group.blocks.0.attn.qkv.weight"  # what tells a SwinIR state from the residual family
SWINIR_RGB_MEAN = EDSR_RGB_MEAN                                  # SwinIR's defaults: the DIV2K mean, img_range 1
SWINIR_IMG_RANGE = 1.0
_SWINIR_LAYER_KEY = re.compile(r"^layers\.(\d+)\.")
_SWINIR_BLOCK_KEY = re.compile(r"^layers\.(\d+)\.residual_group\.blocks\.(\d+)\.")


def _read_dense(state: Mapping, keys, name: str, w_shape, b_shape, part_w: str = "weight"):
    """-> (weight, bias) of ``name`` as contiguous fp32 with exactly these shapes; a ValueError names the offending key."""
    out = []
    for part, shape in ((part_w, w_shape), ("bias", b_shape)):
        if shape is None:
            out.append(None)
            continue
        key = f"{name}.{part}" if part else name
        if key not in keys:
            raise ValueError(f"{key}: not in the state")
        a = np.ascontiguousarray(_array(state, key), dtype=np.float32)
        if a.shape != tuple(shape):
            raise ValueError(f"{key}: expected shape {tuple(shape)}, got {a.shape}")
        out.append(a)
    return out[0], out[1]


class _SwinStateReader:
    """What parse_swinir_state and parse_hat_state share: the tables read so far in create order, the numbering of the groups
    and of their blocks, the tables of an attention and of an MLP, and the pixelshuffle reconstruction.  The nouns of a message
    are the caller's."""

    def __init__(self, state: Mapping):
        self.state = _unwrap(state)
        self.keys = {str(k) for k in self.state}
        self.tables = []

    def refuse_half(self):
        for k in sorted(self.keys):
            name = str(getattr(self.state[k], "dtype", ""))
            if "float16" in name or "bfloat16" in name:
                raise ValueError(f"{k}: {name} weights are not supported (fp32 only)")

    def conv(self, name: str, cin: int, cout=None):
        self.tables.append(_read_conv(self.state, self.keys, name, cin, cout, ", expected {}"))
        return self.tables[-1][0]

    def dense(self, name: str, w_shape, b_shape, part_w: str = "weight"):
        self.tables.append(_read_dense(self.state, self.keys, name, w_shape, b_shape, part_w))

    def shape_of(self, key: str):
        if key not in self.keys:
            raise ValueError(f"{key}: not in the state")
        return tuple(np.shape(_array(self.state, key)))

    def groups(self, noun: str):
        groups = sorted({int(m.group(1)) for m in map(_SWINIR_LAYER_KEY.match, self.keys) if m})
        if not groups or groups != list(range(len(groups))):
            gap = next(i for i in range(len(groups) + 1) if i not in groups)
            raise ValueError(f"layers.{gap}.conv.weight: the {noun} must be numbered 0 .. L - 1, got {groups}")
        return groups

    def blocks(self, g: int, depth, a_group: str, group: str, layers: str):
        """The block numbers of group g, which has as many as the groups before it (``depth``, None for the first)."""
        blocks = sorted({int(m.group(2)) for m in map(_SWINIR_BLOCK_KEY.match, self.keys) if m and int(m.group(1)) == g})
        if not blocks or blocks != list(range(len(blocks))):
            gap = next(i for i in range(len(blocks) + 1) if i not in blocks)
            raise ValueError(f"layers.{g}.residual_group.blocks.{gap}.attn.qkv.weight: {a_group} {layers} must be numbered 0 .. D - 1, got {blocks}")
        if depth is not None and len(blocks) != depth:
            raise ValueError(f"layers.{g}.residual_group.blocks.{min(len(blocks), depth)}.attn.qkv.weight: every {group} must have the same "
                             f"depth, {group} 0 has {depth} {layers} and {group} {g} has {len(blocks)}")
        return blocks

    def attention(self, b: str, attn: str, Cn: int, rows: int, heads: int, only: str):
        """norm1, qkv, the bias table (``rows`` x heads, else ``only`` is what is supported) and proj of block b."""
        t = f"{b}.{attn}relative_position_bias_table"
        if t in self.keys and self.shape_of(t) != (rows, heads):
            got = self.shape_of(t)
            what = "every layer must have the same number of heads" if len(got) == 2 and got[0] == rows else only
            raise ValueError(f"{t}: expected shape {(rows, heads)}, got {got}: {what}")
        self.dense(f"{b}.norm1", (Cn,), (Cn,))
        self.dense(f"{b}.{attn}qkv", (3 * Cn, Cn), (3 * Cn,))
        self.dense(t, (rows, heads), None, "")
        self.dense(f"{b}.{attn}proj", (Cn, Cn), (Cn,))

    def mlp(self, b: str, Cn: int, hidden: int):
        self.dense(f"{b}.norm2", (Cn,), (Cn,))
        self.dense(f"{b}.mlp.fc1", (hidden, Cn), (hidden,))
        self.dense(f"{b}.mlp.fc2", (Cn, hidden), (Cn,))

    def shuffle_tail(self, Cn: int, not_these: str, none: str) -> int:
        """conv_before_upsample, the upsampling stages and conv_last -> the scale."""
        self.conv("conv_before_upsample.0", Cn, 64)
        ups = [f"upsample.{k}" for k in sorted(int(m.group(1)) for m in map(_UPSAMPLE_KEY.match, self.keys) if m)]
        scale = 1
        for name in ups:
            cout = int(np.shape(_array(self.state, f"{name}.weight"))[0])
            r = {256: 2, 576: 3}.get(cout)
            if r is None or (len(ups) >= 2 and r != 2) or len(ups) > 2:
                raise ValueError(f"{name}.weight gives {cout} channels in {len(ups)} stage(s), expected 64 r^2 = 256 (x2, x4) or 576 (x3){not_these}")
            scale *= r
            self.conv(name, 64, cout)
        if not ups:
            raise ValueError(f"upsample.0.weight: not in the state ({none})")
        self.conv("conv_last", 64, 3)
        return scale

    def arrays(self):
        return [w for w, _ in self.tables], [b for _, b in self.tables]


def parse_swinir_state(state: Mapping, img_range: float = SWINIR_IMG_RANGE, rgb_mean=SWINIR_RGB_MEAN):
    """-> (_native.SwinirDesc, weights, biases) in sr_swinir_create's order (_native.swinir_table_names), contiguous fp32; the
    bias entry of a relative-position table is None.

    BasicSR key names.  The whole description is read off the shapes: embed_dim from ``conv_first``, the heads from the second
    axis of ``relative_position_bias_table``, the hidden width from ``mlp.fc1``, the RSTBs and their depth from the numbering
    (from 0 without gaps, the same depth and head count everywhere), the upsampler from which keys exist
    (``conv_up1`` -> nearest+conv, ``conv_before_upsample.0`` -> pixelshuffle, ``upsample.0`` alone -> pixelshuffledirect) and
    the scale from the upsampling convolutions' widths.  The ``relative_position_index`` and ``attn_mask`` buffers are
    ignored.  A ValueError names the offending key for a wrong shape and for everything out of scope: resi_connection '3conv',
    the absolute position embedding, a window other than 8, the JPEG / denoising variants (no upsampler), Swin2SR, fp16 / bf16;
    what only the kernels' ranges exclude is a NotImplementedError."""
    rd = _SwinStateReader(state)
    state, keys, conv, dense = rd.state, rd.keys, rd.conv, rd.dense
    if SWINIR_KEY not in keys:
        raise ValueError(f"{SWINIR_KEY}: not in the state (not a SwinIR)")
    if "absolute_pos_embed" in keys:
        raise ValueError("absolute_pos_embed: the absolute position embedding (ape=True) is not supported")
    if "layers.0.conv.0.weight" in keys:
        raise ValueError("layers.0.conv.0.weight: resi_connection '3conv' is not supported (only '1conv')")
    for k in sorted(keys):
        if k.endswith((".attn.logit_scale", ".attn.cpb_mlp.0.weight", ".attn.q_bias")):
            raise ValueError(f"{k}: this is a Swin2SR state (SwinV2 attention), not a SwinIR")
    rd.refuse_half()
    Cn = int(conv("conv_first", 3).shape[0])
    dense("patch_embed.norm", (Cn,), (Cn,))
    groups = rd.groups("RSTBs")
    tkey = "layers.0.residual_group.blocks.0.attn.relative_position_bias_table"
    tshape = rd.shape_of(tkey)
    rows = (2 * _native.SWINIR_WINDOW - 1) ** 2
    if len(tshape) != 2 or tshape[0] != rows:
        raise ValueError(f"{tkey}: shape {tshape} is not a window of 8 ({rows} rows): only window_size 8 is supported")
    heads = int(tshape[1])
    hidden = int(rd.shape_of("layers.0.residual_group.blocks.0.mlp.fc1.weight")[0])
    depth = None
    for g in groups:
        blocks = rd.blocks(g, depth, "an RSTB's", "RSTB", "layers")
        depth = len(blocks)
        for j in blocks:
            b = f"layers.{g}.residual_group.blocks.{j}"
            rd.attention(b, "attn.", Cn, rows, heads, "only window_size 8 is supported")
            rd.mlp(b, Cn, hidden)
        conv(f"layers.{g}.conv", Cn, Cn)
    dense("norm", (Cn,), (Cn,))
    conv("conv_after_body", Cn, Cn)
    scale = 1
    if "conv_up1.weight" in keys:
        kind, scale = "nearest+conv", 4
        conv("conv_before_upsample.0", Cn, 64)
        for name in ("conv_up1", "conv_up2", "conv_hr"):
            conv(name, 64, 64)
        conv("conv_last", 64, 3)
    elif "conv_before_upsample.0.weight" in keys:
        kind = "pixelshuffle"
        scale = rd.shuffle_tail(Cn, "", "pixelshuffle at scale 1 has no upsampling stage and is not supported")
    elif "upsample.0.weight" in keys:
        kind = "pixelshuffledirect"
        cout = int(np.shape(_array(state, "upsample.0.weight"))[0])
        scale = {3: 1, 12: 2, 27: 3, 48: 4}.get(cout)
        if scale is None:
            raise ValueError(f"upsample.0.weight gives {cout} channels, expected 3 s^2 with s in 1 .. 4")
        conv("upsample.0", Cn, cout)
    else:
        raise ValueError("conv_last.weight: no upsampler keys (conv_before_upsample, upsample, conv_up1): the JPEG / denoising variants "
                         "of SwinIR are not supported")
    desc = _native.swinir_desc(Cn, heads, hidden, len(groups), depth, scale, kind, rgb_mean, float(img_range))
    _native.swinir_plan(desc, 1, 1)                              # NotImplementedError outside the kernels' range (host only)
    return (desc,) + rd.arrays()


class SwinIRSRNet(_OnePieceSRNet):
    """SwinIR on the GPU, with CompactSRNet's surface (from_file, model, upscale, upscale_device, close).  ``state``: a BasicSR
    state dict (see parse_swinir_state).

    Shifted windows let a pixel see farther with every layer, so the image is not streamed through the trunk: there is no
    ``tile`` (anything but 0 is refused), only the ``tail`` of the reconstruction, which changes no bit.  An image cut into
    tiles before the network (as the pipeline does with ``block_size``) is reflected, padded and windowed tile by tile -- as
    every tiled inference of SwinIR does -- so the tile size affects the values, not only the speed."""

    _one_piece = "SwinIR's trunk is one piece (shifted windows reach across any tile)"

    def __init__(self, state: Mapping, img_range: float = SWINIR_IMG_RANGE, rgb_mean=SWINIR_RGB_MEAN, device: int = 0):
        self.desc, self._w, self._b = parse_swinir_state(state, img_range, rgb_mean)
        d = self.desc
        self.n_feat, self.n_heads, self.n_hidden, self.n_groups, self.depth, self.scale = d.n_feat, d.n_heads, d.n_hidden, d.n_groups, d.depth, d.scale
        self.device = int(device)
        self._models = {}

    @classmethod
    def from_file(cls, path: str, device: int = 0, **extras) -> "SwinIRSRNet":
        """A .npz may hold the constants a state dict lacks as a 0-d ``img_range`` and a 3-vector ``rgb_mean`` entry; keyword
        arguments win over them, SwinIR's defaults (1, the DIV2K mean) stand in for the rest."""
        state = load_state(path)
        return cls(state, device=device, **{**_swinir_extras(state), **extras})

    def _make_model(self, ctx: "_native.Context"):
        return _native.SwinirModel(ctx, self.desc, self._w, self._b)


def _swinir_extras(state: Mapping) -> dict:
    return _scalar_extras(state, (("img_range", 1), ("rgb_mean", 3)))


# ------------------------------------------------------------------------------------------
# HAT: the hybrid attention transformer (Chen et al., CVPR 2023), run by csrc/sr_hat.hip: a Swin trunk with 16 x 16 windows, a
# channel-attention convolution branch (CAB) beside every window attention and an overlapping cross-attention block (OCAB) at
# the end of every group.  PARITY UNPINNED here too: neither the HAT package nor a checkpoint exists offline; the arithmetic is
# written out in include/sr_hip.h and held against a torch-CPU restatement (tests/_hat_ref.py).  The one piece restated from
# memory with the least confidence is the index of the overlapping cross-attention: a state's own
# ``relative_position_index_OCA`` buffer is used when it is there, the recalled formula only when it is not.
# ------------------------------------------------------------------------------------------
HAT_KEY = "layers.0.residual_group.overlap_attn.qkv.weight"      # what tells a HAT state from a SwinIR one
HAT_RGB_MEAN = EDSR_RGB_MEAN                                     # HAT's defaults: the DIV2K mean, img_range 1, conv_scale 0.01
HAT_IMG_RANGE = 1.0
HAT_CONV_SCALE = 0.01


def parse_hat_state(state: Mapping, img_range: float = HAT_IMG_RANGE, rgb_mean=HAT_RGB_MEAN, conv_scale: float = HAT_CONV_SCALE):
    """-> (_native.HatDesc, weights, biases, rpi_oca) in sr_hat_create's order (_native.hat_table_names), contiguous fp32; the
    bias entry of a relative-position table is None; rpi_oca is the state's ``relative_position_index_OCA`` as int32
    (256, 576) -- negative values allowed, the library wraps them -- or None where the state holds none (the default formula).

    HAT's key names.  The whole description is read off the shapes: embed_dim from ``conv_first``, the heads from the second
    axis of ``relative_position_bias_table``, window 16 from its 961 rows, the overlap window 24 from the 1521 rows of the
    OCAB's table, the hidden width from ``mlp.fc1``, the CAB's widths from ``conv_block.cab.0`` and
    ``conv_block.cab.3.attention.1``, the groups and their depth from the numbering, the scale from the upsampling
    convolutions' widths.  The two index buffers are looked for under every key that ends in their name: HAT registers them once
    on the top-level module, so a checkpoint holds the bare keys ``relative_position_index_SA`` and
    ``relative_position_index_OCA``; nested copies are read the same way.  Every ``relative_position_index_SA`` must equal the
    computed index, every ``relative_position_index_OCA`` must agree with the others and is the index used; ``attn_mask``
    buffers are ignored.  A ValueError names the offending key for a wrong shape and for everything out of scope (other
    windows, other overlap ratios, resi_connection 'identity', the absolute position embedding, upsamplers other than
    pixelshuffle, fp16 / bf16); what only the kernels' ranges exclude is a NotImplementedError."""
    rd = _SwinStateReader(state)
    state, keys, conv, dense, shape_of = rd.state, rd.keys, rd.conv, rd.dense, rd.shape_of
    if HAT_KEY not in keys:
        raise ValueError(f"{HAT_KEY}: not in the state (not a HAT)")
    if "absolute_pos_embed" in keys:
        raise ValueError("absolute_pos_embed: the absolute position embedding (ape=True) is not supported")
    if "layers.0.conv.0.weight" in keys:
        raise ValueError("layers.0.conv.0.weight: only resi_connection '1conv' is supported")
    if "layers.0.conv.weight" not in keys:
        raise ValueError("layers.0.conv.weight: not in the state (resi_connection 'identity' is not supported, only '1conv')")
    rd.refuse_half()

    def pointwise(name: str, cout: int, cin: int):              # a 1 x 1 convolution: (out, in, 1, 1) or (out, in)
        for part in ("weight", "bias"):
            if f"{name}.{part}" not in keys:
                raise ValueError(f"{name}.{part}: not in the state")
        w = np.ascontiguousarray(_array(state, f"{name}.weight"), dtype=np.float32)
        b = np.ascontiguousarray(_array(state, f"{name}.bias"), dtype=np.float32).reshape(-1)
        if w.shape not in ((cout, cin), (cout, cin, 1, 1)):
            raise ValueError(f"{name}.weight: expected shape {(cout, cin, 1, 1)}, got {w.shape}")
        if b.shape != (cout,):
            raise ValueError(f"{name}.bias: expected {cout} values, got {b.shape}")
        rd.tables.append((w.reshape(cout, cin), b))

    Cn = int(conv("conv_first", 3).shape[0])
    dense("patch_embed.norm", (Cn,), (Cn,))
    groups = rd.groups("groups")
    rows, orows = _native.HAT_REL_ROWS, _native.HAT_OCA_ROWS
    tkey = "layers.0.residual_group.blocks.0.attn.relative_position_bias_table"
    tshape = shape_of(tkey)
    if len(tshape) != 2 or tshape[0] != rows:
        raise ValueError(f"{tkey}: shape {tshape} is not a window of 16 ({rows} rows): only window_size 16 is supported")
    heads = int(tshape[1])
    okey = "layers.0.residual_group.overlap_attn.relative_position_bias_table"
    oshape = shape_of(okey)
    if len(oshape) != 2 or oshape[0] != orows:
        raise ValueError(f"{okey}: shape {oshape} is not an overlap window of 24 ({orows} rows): only overlap_ratio 0.5 of window 16 is supported")
    hidden = int(shape_of("layers.0.residual_group.blocks.0.mlp.fc1.weight")[0])
    mid = int(shape_of("layers.0.residual_group.blocks.0.conv_block.cab.0.weight")[0])
    squeeze = int(shape_of("layers.0.residual_group.blocks.0.conv_block.cab.3.attention.1.weight")[0])
    # The two index buffers, wherever the state holds them: HAT registers them once on the top-level module (the bare keys
    # ``relative_position_index_SA`` / ``relative_position_index_OCA``); a nested copy (``...attn.relative_position_index_SA``,
    # ``...overlap_attn.relative_position_index_OCA``) is read the same way.  None is ever ignored.
    rpi_oca, first = None, None
    for ikey in sorted(k for k in keys if k.endswith("relative_position_index_SA")):
        got, rel = np.asarray(_array(state, ikey)), _native.hat_rel_index()
        if got.shape != rel.shape or not np.array_equal(got, rel):
            raise ValueError(f"{ikey}: differs from the relative-position index of a 16 x 16 window that the kernels compute")
    for ikey in sorted(k for k in keys if k.endswith("relative_position_index_OCA")):
        got = _native._hat_index(np.asarray(_array(state, ikey)), ikey)
        if rpi_oca is not None and not np.array_equal(got, rpi_oca):
            raise ValueError(f"{ikey}: differs from {first} (one index serves every OCAB)")
        if rpi_oca is None:
            rpi_oca, first = got, ikey
    depth = None
    for g in groups:
        blocks = rd.blocks(g, depth, "a group's", "group", "HABs")
        depth = len(blocks)
        for j in blocks:
            b = f"layers.{g}.residual_group.blocks.{j}"
            rd.attention(b, "attn.", Cn, rows, heads, "only window_size 16 is supported")
            conv(f"{b}.conv_block.cab.0", Cn, mid)
            conv(f"{b}.conv_block.cab.2", mid, Cn)
            pointwise(f"{b}.conv_block.cab.3.attention.1", squeeze, Cn)
            pointwise(f"{b}.conv_block.cab.3.attention.3", Cn, squeeze)
            rd.mlp(b, Cn, hidden)
        o = f"layers.{g}.residual_group.overlap_attn"
        rd.attention(o, "", Cn, orows, heads, "only overlap_ratio 0.5 of window 16 is supported")
        rd.mlp(o, Cn, hidden)
        conv(f"layers.{g}.conv", Cn, Cn)
    dense("norm", (Cn,), (Cn,))
    conv("conv_after_body", Cn, Cn)
    if "conv_up1.weight" in keys:
        raise ValueError("conv_up1.weight: upsampler nearest+conv is not supported (only pixelshuffle)")
    if "conv_before_upsample.0.weight" not in keys:
        raise ValueError("conv_before_upsample.0.weight: not in the state (only upsampler pixelshuffle is supported)")
    scale = rd.shuffle_tail(Cn, ": x1 and x8 are not supported", "scale 1 is not supported")
    desc = _native.hat_desc(Cn, heads, hidden, mid, squeeze, len(groups), depth, scale, float(conv_scale), rgb_mean, float(img_range))
    _native.hat_plan(desc, 1, 1)                                 # NotImplementedError outside the kernels' range (host only)
    return (desc,) + rd.arrays() + (rpi_oca,)


class HATSRNet(_OnePieceSRNet):
    """HAT on the GPU, with CompactSRNet's surface (from_file, model, upscale, upscale_device, close).  ``state``: a HAT state
    dict (see parse_hat_state).  As SwinIRSRNet there is no ``tile`` (anything but 0 is refused), only the ``tail`` of the
    reconstruction, which changes no bit; an image cut into tiles before the network is reflected, padded, windowed -- and its
    CAB means pooled -- tile by tile."""

    _one_piece = "HAT's trunk is one piece (windows, overlaps and the CAB's mean reach across any tile)"

    def __init__(self, state: Mapping, img_range: float = HAT_IMG_RANGE, rgb_mean=HAT_RGB_MEAN, conv_scale: float = HAT_CONV_SCALE,
                 device: int = 0):
        self.desc, self._w, self._b, self._rpi = parse_hat_state(state, img_range, rgb_mean, conv_scale)
        d = self.desc
        self.n_feat, self.n_heads, self.n_hidden, self.n_groups, self.depth, self.scale = d.n_feat, d.n_heads, d.n_hidden, d.n_groups, d.depth, d.scale
        self.device = int(device)
        self._models = {}

    @classmethod
    def from_file(cls, path: str, device: int = 0, **extras) -> "HATSRNet":
        """A .npz may hold the constants a state dict lacks as 0-d ``img_range`` and ``conv_scale`` and a 3-vector ``rgb_mean``
        entry; keyword arguments win over them, HAT's defaults (1, 0.01, the DIV2K mean) stand in for the rest."""
        state = load_state(path)
        return cls(state, device=device, **{**_hat_extras(state), **extras})

    def _make_model(self, ctx: "_native.Context"):
        return _native.HatModel(ctx, self.desc, self._w, self._b, self._rpi)


def _hat_extras(state: Mapping) -> dict:
    return _scalar_extras(state, (("img_range", 1), ("rgb_mean", 3), ("conv_scale", 1)))


# ------------------------------------------------------------------------------------------
# Swin2SR: SwinV2 cosine attention with a continuous position bias, post-norm (Conde et al., ECCVW 2022), run by
# csrc/sr_swin2sr.hip.  The `transformers` package's key layout is PINNED against `transformers` 5.15.0 (random-weight float64
# goldens under tests/golden/); the official repository's layout and its -100 mask rest on the restatement
# (tests/_swin2sr_ref.py); no published checkpoint was ever run.
# ------------------------------------------------------------------------------------------
SWIN2SR_PACKAGE_KEY = "swin2sr.encoder.stages.0.layers.0.attention.self.logit_scale"   # the `transformers` layout
SWIN2SR_OFFICIAL_KEY = "layers.0.residual_group.blocks.0.attn.logit_scale"             # the official repository's layout
SWIN2SR_RGB_MEAN = EDSR_RGB_MEAN                                 # Swin2SR's defaults: the DIV2K mean, img_range 1
SWIN2SR_IMG_RANGE = 1.0
_S2_STAGE_KEY = {True: re.compile(r"^swin2sr\.encoder\.stages\.(\d+)\."), False: re.compile(r"^layers\.(\d+)\.")}
_S2_LAYER_KEY = {True: re.compile(r"^swin2sr\.encoder\.stages\.(\d+)\.layers\.(\d+)\."),
                 False: re.compile(r"^layers\.(\d+)\.residual_group\.blocks\.(\d+)\.")}


def swin2sr_layout(keys) -> Optional[str]:
    """'package', 'official' or None: which Swin2SR key layout a state's keys are."""
    keys = {str(k) for k in keys}
    return "package" if SWIN2SR_PACKAGE_KEY in keys else "official" if SWIN2SR_OFFICIAL_KEY in keys else None


def parse_swin2sr_state(state: Mapping, img_range: float = SWIN2SR_IMG_RANGE, rgb_mean=SWIN2SR_RGB_MEAN, mask_value: Optional[float] = None):
    """-> (_native.Swin2srDesc, weights, biases) in sr_swin2sr_create's order (_native.swin2sr_table_names), contiguous fp32; the
    bias entries of logit_scale and cpb_mlp.2 are None.

    Both key layouts are read: the `transformers` package's (``swin2sr.encoder.stages.{i}.layers.{j}.attention.self.{query, key,
    value, logit_scale, continuous_position_bias_mlp.0 / .2}``, ``...attention.output.dense``, ``layernorm_before / _after``,
    ``intermediate.dense``, ``output.dense``, ``stages.{i}.conv``, ``stages.{i}.patch_embed.projection``, ``upsample.*``) and the
    official repository's (``layers.{i}.residual_group.blocks.{j}.attn.{qkv.weight, q_bias, v_bias, logit_scale, cpb_mlp.*,
    proj}``, ``patch_embed.proj``, ``layers.{i}.patch_embed.proj``, ...).  query / key / value are stacked into one qkv table whose
    k bias is zero.  ``mask_value``: None takes the layout's own, -200 for the package (it adds the shifted-window mask twice),
    -100 for the official code.  The whole description is read off the shapes; the buffers ``relative_coords_table``,
    ``relative_position_index`` and ``attn_mask`` are recomputed, never read.  A ValueError names the offending key for a wrong
    shape and for everything out of scope: upsampler pixelshuffle_aux, no upsampler (JPEG / denoising), resi_connection '3conv',
    the absolute position embedding, a window other than 8, a k bias that is not zero, unequal depths or head counts between
    stages, fp16 / bf16; what only the kernels' ranges exclude is a NotImplementedError."""
    rd = _SwinStateReader(state)
    state, keys, conv, dense = rd.state, rd.keys, rd.conv, rd.dense
    layout = swin2sr_layout(keys)
    if layout is None:
        raise ValueError(f"{SWIN2SR_PACKAGE_KEY}: not in the state, nor {SWIN2SR_OFFICIAL_KEY} (not a Swin2SR)")
    pk = layout == "package"
    if mask_value is None:
        mask_value = _native.SWIN2SR_MASK_PACKAGE if pk else _native.SWIN2SR_MASK_OFFICIAL
    root = "swin2sr." if pk else ""
    up = "upsample." if pk else ""
    for k in ("swin2sr.embeddings.position_embeddings", "absolute_pos_embed"):
        if k in keys:
            raise ValueError(f"{k}: the absolute position embedding is not supported")
    c3 = "swin2sr.encoder.stages.0.conv.0.weight" if pk else "layers.0.conv.0.weight"
    if c3 in keys:
        raise ValueError(f"{c3}: resi_connection '3conv' is not supported (only '1conv')")
    aux = f"{up}conv_bicubic.weight"
    if aux in keys:
        raise ValueError(f"{aux}: upsampler pixelshuffle_aux is not supported")
    rd.refuse_half()

    def stage(i):
        return f"swin2sr.encoder.stages.{i}" if pk else f"layers.{i}"

    def block(i, j):
        return f"{stage(i)}.layers.{j}" if pk else f"{stage(i)}.residual_group.blocks.{j}"

    def pointwise(name: str, Cn: int):                           # a 1 x 1 convolution C -> C: (C, C, 1, 1) or (C, C)
        for part in ("weight", "bias"):
            if f"{name}.{part}" not in keys:
                raise ValueError(f"{name}.{part}: not in the state")
        w = np.ascontiguousarray(_array(state, f"{name}.weight"), dtype=np.float32)
        b = np.ascontiguousarray(_array(state, f"{name}.bias"), dtype=np.float32).reshape(-1)
        if w.shape not in ((Cn, Cn), (Cn, Cn, 1, 1)):
            raise ValueError(f"{name}.weight: expected shape {(Cn, Cn, 1, 1)}, got {w.shape}: only patch_size 1 is supported")
        if b.shape != (Cn,):
            raise ValueError(f"{name}.bias: expected {Cn} values, got {b.shape}")
        rd.tables.append((w.reshape(Cn, Cn), b))

    def vector(key: str, n: int, what: str = ""):
        if key not in keys:
            raise ValueError(f"{key}: not in the state")
        a = np.ascontiguousarray(_array(state, key), dtype=np.float32)
        if a.size != n or a.reshape(-1).shape != (n,):
            raise ValueError(f"{key}: expected {n} values, got shape {a.shape}{what}")
        return a.reshape(-1)

    Cn = int(conv(f"{root}first_convolution" if pk else "conv_first", 3).shape[0])
    pointwise("swin2sr.embeddings.patch_embeddings.projection" if pk else "patch_embed.proj", Cn)
    dense("swin2sr.embeddings.patch_embeddings.layernorm" if pk else "patch_embed.norm", (Cn,), (Cn,))
    stages = sorted({int(m.group(1)) for m in map(_S2_STAGE_KEY[pk].match, keys) if m})
    if not stages or stages != list(range(len(stages))):
        gap = next(i for i in range(len(stages) + 1) if i not in stages)
        raise ValueError(f"{stage(gap)}.conv.weight: the stages must be numbered 0 .. L - 1, got {stages}")
    heads = int(np.size(_array(state, SWIN2SR_PACKAGE_KEY if pk else SWIN2SR_OFFICIAL_KEY)))
    hidden = int(rd.shape_of(f"{block(0, 0)}.{'intermediate.dense' if pk else 'mlp.fc1'}.weight")[0])
    hid_cpb = _native.SWIN2SR_CPB_HIDDEN
    depth = None
    for i in stages:
        blocks = sorted({int(m.group(2)) for m in map(_S2_LAYER_KEY[pk].match, keys) if m and int(m.group(1)) == i})
        if not blocks or blocks != list(range(len(blocks))):
            gap = next(j for j in range(len(blocks) + 1) if j not in blocks)
            raise ValueError(f"{block(i, gap)}: a stage's layers must be numbered 0 .. D - 1, got {blocks}")
        if depth is not None and len(blocks) != depth:
            raise ValueError(f"{block(i, min(len(blocks), depth))}: every stage must have the same depth, stage 0 has {depth} layers and "
                             f"stage {i} has {len(blocks)}")
        depth = len(blocks)
        for j in blocks:
            b = block(i, j)
            a = f"{b}.attention.self" if pk else f"{b}.attn"
            if pk:
                if f"{a}.key.bias" in keys and np.any(np.asarray(_array(state, f"{a}.key.bias"), dtype=np.float32) != 0):
                    raise ValueError(f"{a}.key.bias: a k bias that is not zero is not supported (Swin2SR's key has none)")
                parts = [_read_dense(state, keys, f"{a}.{n}", (Cn, Cn), (Cn,) if n != "key" else None) for n in ("query", "key", "value")]
                w = np.concatenate([p[0] for p in parts])
                qb, vb = parts[0][1], parts[2][1]
            else:
                w = _read_dense(state, keys, f"{a}.qkv", (3 * Cn, Cn), None)[0]
                if f"{a}.qkv.bias" in keys:
                    full = vector(f"{a}.qkv.bias", 3 * Cn)
                    if np.any(full[Cn:2 * Cn] != 0):
                        raise ValueError(f"{a}.qkv.bias: a k bias that is not zero is not supported (Swin2SR's is q_bias, 0, v_bias)")
                    qb, vb = full[:Cn], full[2 * Cn:]
                else:
                    qb, vb = vector(f"{a}.q_bias", Cn), vector(f"{a}.v_bias", Cn)
            rd.tables.append((np.ascontiguousarray(w), np.ascontiguousarray(np.concatenate([qb, np.zeros(Cn, np.float32), vb]))))
            rd.tables.append((vector(f"{a}.logit_scale", heads, ": every layer must have the same number of heads"), None))
            mlp = f"{a}.continuous_position_bias_mlp" if pk else f"{a}.cpb_mlp"
            dense(f"{mlp}.0", (hid_cpb, 2), (hid_cpb,))
            got = rd.shape_of(f"{mlp}.2.weight")
            if got != (heads, hid_cpb):
                raise ValueError(f"{mlp}.2.weight: expected shape {(heads, hid_cpb)}, got {got}: every layer must have the same number of heads")
            dense(f"{mlp}.2", (heads, hid_cpb), None)
            dense(f"{b}.attention.output.dense" if pk else f"{a}.proj", (Cn, Cn), (Cn,))
            dense(f"{b}.layernorm_before" if pk else f"{b}.norm1", (Cn,), (Cn,))
            dense(f"{b}.intermediate.dense" if pk else f"{b}.mlp.fc1", (hidden, Cn), (hidden,))
            dense(f"{b}.output.dense" if pk else f"{b}.mlp.fc2", (Cn, hidden), (Cn,))
            dense(f"{b}.layernorm_after" if pk else f"{b}.norm2", (Cn,), (Cn,))
            for buf, want in ((f"{a}.relative_position_index", (64, 64)), (f"{a}.relative_coords_table", (1, 15, 15, 2))):
                if buf in keys and rd.shape_of(buf) != want:       # recomputed, never read -- but its shape tells the window
                    raise ValueError(f"{buf}: shape {rd.shape_of(buf)} is not a window of 8 {want}: only window_size 8 is supported")
        conv(f"{stage(i)}.conv", Cn, Cn)
        pointwise(f"{stage(i)}.patch_embed.{'projection' if pk else 'proj'}", Cn)
    dense("swin2sr.layernorm" if pk else "norm", (Cn,), (Cn,))
    conv(f"{root}conv_after_body", Cn, Cn)
    last = f"{up}final_convolution" if pk else "conv_last"
    cbu = f"{up}conv_before_upsample" if pk else "conv_before_upsample.0"
    scale = 1
    if f"{up}conv_up1.weight" in keys:
        kind, scale = "nearest+conv", 4
        conv(cbu, Cn, 64)
        for name in ("conv_up1", "conv_up2", "conv_hr"):
            conv(f"{up}{name}", 64, 64)
        conv(last, 64, 3)
    elif f"{cbu}.weight" in keys:
        kind = "pixelshuffle"
        conv(cbu, Cn, 64)
        if pk:
            ups = sorted(k[:-len(".weight")] for k in keys if k.startswith("upsample.upsample.convolution") and k.endswith(".weight"))
        else:
            ups = [f"upsample.{n}" for n in sorted(int(m.group(1)) for m in map(_UPSAMPLE_KEY.match, keys) if m)]
        if not ups:
            raise ValueError(f"{'upsample.upsample.convolution_0' if pk else 'upsample.0'}.weight: not in the state (pixelshuffle at scale 1 has no "
                             "upsampling stage and is not supported)")
        for name in ups:
            cout = int(np.shape(_array(state, f"{name}.weight"))[0])
            r = {256: 2, 576: 3}.get(cout)
            if r is None or (len(ups) >= 2 and r != 2) or len(ups) > 2:
                raise ValueError(f"{name}.weight gives {cout} channels in {len(ups)} stage(s), expected 64 r^2 = 256 (x2, x4) or 576 (x3)")
            scale *= r
            conv(name, 64, cout)
        conv(last, 64, 3)
    elif ("upsample.conv.weight" if pk else "upsample.0.weight") in keys:
        kind = "pixelshuffledirect"
        name = "upsample.conv" if pk else "upsample.0"
        cout = int(np.shape(_array(state, f"{name}.weight"))[0])
        scale = {3: 1, 12: 2, 27: 3, 48: 4}.get(cout)
        if scale is None:
            raise ValueError(f"{name}.weight gives {cout} channels, expected 3 s^2 with s in 1 .. 4")
        conv(name, Cn, cout)
    else:
        raise ValueError(f"{'final_convolution' if pk else 'conv_last'}.weight: no upsampler keys (conv_before_upsample, upsample, conv_up1): the "
                         "JPEG / denoising variants of Swin2SR are not supported")
    desc = _native.swin2sr_desc(Cn, heads, hidden, len(stages), depth, scale, kind, rgb_mean, float(img_range), float(mask_value))
    _native.swin2sr_plan(desc, 1, 1)                             # NotImplementedError outside the kernels' range (host only)
    return (desc,) + rd.arrays()


class Swin2SRNet(_OnePieceSRNet):
    """Swin2SR on the GPU, with CompactSRNet's surface (from_file, model, upscale, upscale_device, close).  ``state``: a state dict
    in the `transformers` package's or the official repository's key layout (see parse_swin2sr_state).  As SwinIRSRNet there is no
    ``tile`` (anything but 0 is refused), only the ``tail`` of the reconstruction, which changes no bit; an image cut into tiles
    before the network is reflected, padded and windowed tile by tile."""

    _one_piece = "Swin2SR's trunk is one piece (shifted windows reach across any tile)"

    def __init__(self, state: Mapping, img_range: float = SWIN2SR_IMG_RANGE, rgb_mean=SWIN2SR_RGB_MEAN, mask_value: Optional[float] = None,
                 device: int = 0):
        self.desc, self._w, self._b = parse_swin2sr_state(state, img_range, rgb_mean, mask_value)
        d = self.desc
        self.n_feat, self.n_heads, self.n_hidden, self.n_groups, self.depth, self.scale = d.n_feat, d.n_heads, d.n_hidden, d.n_groups, d.depth, d.scale
        self.mask_value = float(d.mask_value)
        self.device = int(device)
        self._models = {}

    @classmethod
    def from_file(cls, path: str, device: int = 0, **extras) -> "Swin2SRNet":
        """A .npz may hold the constants a state dict lacks as 0-d ``img_range`` and ``mask_value`` and a 3-vector ``rgb_mean``
        entry; keyword arguments win over them, Swin2SR's defaults (1, the layout's mask, the DIV2K mean) stand in for the rest."""
        state = load_state(path)
        return cls(state, device=device, **{**_swin2sr_extras(state), **extras})

    def _make_model(self, ctx: "_native.Context"):
        return _native.Swin2srModel(ctx, self.desc, self._w, self._b)


def _swin2sr_extras(state: Mapping) -> dict:
    return _scalar_extras(state, (("img_range", 1), ("rgb_mean", 3), ("mask_value", 1)))


def load_network(path: str, act: str = "prelu", device: int = 0):
    """The network a weights file holds: a ``body.0.rdb1.conv1.weight`` entry makes it an RRDBSRNet, a
    ``body.0.residual_group.0.rcab.0.weight`` entry an RCANSRNet, a ``layers.0.residual_group.overlap_attn.qkv.weight`` entry a
    HATSRNet, a ``...attention.self.logit_scale`` / ``...attn.logit_scale`` entry of layer 0 a Swin2SRNet (either key layout), a ``layers.0.residual_group.blocks.0.attn.qkv.weight`` entry a SwinIRSRNet, otherwise a ``conv_first.weight`` entry a ResidualSRNet (``act`` is ignored for these families), ``body.{i}.weight`` entries a CompactSRNet exactly as
    CompactSRNet.from_file."""
    state = load_state(path)
    if RRDB_KEY in {str(k) for k in _unwrap(state)}:
        return RRDBSRNet(state, device=device, **_rrdb_extras(state))
    if RCAN_KEY in {str(k) for k in _unwrap(state)}:
        return RCANSRNet(state, device=device, **_residual_extras(state))
    if swin2sr_layout(_unwrap(state)) is not None:                 # before SwinIR's key, which an official-layout Swin2SR state carries too
        return Swin2SRNet(state, device=device, **_swin2sr_extras(state))
    if HAT_KEY in {str(k) for k in _unwrap(state)}:                # before SwinIR's key, which a HAT state carries too
        return HATSRNet(state, device=device, **_hat_extras(state))
    if SWINIR_KEY in {str(k) for k in _unwrap(state)}:
        return SwinIRSRNet(state, device=device, **_swinir_extras(state))
    if "conv_first.weight" in {str(k) for k in _unwrap(state)}:
        return ResidualSRNet(state, device=device, **_residual_extras(state))
    return CompactSRNet(state, act=act, device=device)
