"""Torch-CPU restatement of the residual SR family's contract (include/sr_hip.h, "residual family") -- the yardstick of
tests/test_gpu_resnet.py and tests/test_resnet_host.py -- plus seeded synthetic weights under BasicSR's key names.

PARITY UNPINNED: the BasicSR package (MSRResNet, EDSR) and its checkpoints do not exist offline; this file restates the two
published forwards with torch's own operators:

    MSRResNet  f = lrelu(conv_first(x));  f = f + conv2(relu(conv1(f))) per block;  f = lrelu(pixel_shuffle(upconv(f))) per stage;
               o = conv_last(lrelu(conv_hr(f))) + interpolate(x, s, bilinear, align_corners=False)          (lrelu slope 0.1)
    EDSR       x = (x - mean) * range;  h = conv_first(x);  t = t + res_scale * conv2(relu(conv1(t))) per block;
               t = conv_after_body(t) + h;  o = conv_last(pixel_shuffle(upsample(t))) / range + mean

in float32 (what a torch user would run) and float64 (the truth the bounds are taken against).  It reads the state dict on
its own (it does not use the product's parser).  res_scale, img_range and rgb_mean ride in the state as extra entries, the
way sr_network.load_network reads them from a .npz; the fp32 values of these constants are the contract's parameters, so the
float64 forward uses those fp32 values exactly.

The two presets are two points of the C ABI's descriptor (sr_resnet_desc).  The second half of this file restates the whole
descriptor: Desc (the header's fields), conv_roles (the convolution list, restated here -- this file does not import the
product), forward_desc / chain_forward_desc (the header's eight steps in torch and in numpy fp32), synthetic_weights, the
descriptor-space list DESC_CASES, and the exact-arithmetic networks EXACT_NETS / PROBES whose every partial sum is
representable in fp32, so that any summation order gives the same bits (exact_proof is that proof)."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from _srnet_ref import _chain_conv, check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)

RGB_MEAN = (0.4488, 0.4371, 0.4040)
STAGES = {1: [], 2: [2], 3: [3], 4: [2, 2]}

# (preset, F, B, s, h, w, res_scale) of the float / u8 accuracy check
CASES = [("msr", 64, 2, 2, 45, 77, 1.0), ("msr", 64, 1, 4, 19, 37, 1.0), ("msr", 64, 1, 3, 33, 41, 1.0), ("msr", 64, 0, 1, 20, 35, 1.0),
         ("edsr", 64, 2, 2, 40, 70, 0.1), ("edsr", 128, 1, 3, 17, 40, 1.0), ("edsr", 256, 1, 4, 12, 35, 0.1),
         # the shipped depth (B = 16; EDSR at res_scale 0.1 -- at 1.0 its activations blow up and the whole output clamps), and
         # F = 192: three cout tiles in head and body, 27 tiles in the r = 3 shuffle whose groups of 9 straddle the 64-cout tiles
         ("msr", 64, 16, 2, 16, 40, 1.0), ("edsr", 64, 16, 2, 16, 40, 0.1), ("edsr", 192, 1, 3, 9, 33, 1.0), ("msr", 192, 1, 2, 9, 33, 1.0)]
# degenerate images and exact / one-past multiples of the convolution's 8 x 32 block, on one network of each preset
EDGE_SHAPES = [(1, 1), (1, 50), (50, 1), (8, 32), (9, 33)]
EDGE_CASES = [("msr", 64, 1, 2, h, w, 1.0) for h, w in EDGE_SHAPES] + [("edsr", 64, 1, 3, h, w, 0.1) for h, w in EDGE_SHAPES]


def synthetic_state(preset: str, n_feat: int, n_blocks: int, scale: int, seed: int = 20260313, res_scale: float = 1.0) -> dict:
    """Seeded weights under BasicSR's key names.  Convolutions N(0, sqrt(2 / (9 cin))), every block's conv2 and conv_last x 0.1
    (BasicSR initialises residual branches small), biases N(0, 0.01) -- conv_last's bias N(0.3, 0.2) for 'msr' so that a good
    share of the output clamps at 1.  'edsr' states also hold res_scale, img_range (255) and rgb_mean entries."""
    assert preset in ("msr", "edsr")
    rng = np.random.default_rng(seed)
    st = {}
    F = n_feat

    def conv(name, cout, cin, gain=1.0):
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * gain).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)

    conv("conv_first", F, 3)
    for i in range(n_blocks):
        conv(f"body.{i}.conv1", F, F)
        conv(f"body.{i}.conv2", F, F, 0.1 if preset == "msr" else 1.0)
    if preset == "edsr":
        conv("conv_after_body", F, F)
        for k, r in enumerate(STAGES[scale]):
            conv(f"upsample.{2 * k}", F * r * r, F)              # nn.Sequential(conv, PixelShuffle, conv, PixelShuffle)
        conv("conv_last", 3, F, 0.1)
        st["res_scale"] = np.array(res_scale, np.float32)
        st["img_range"] = np.array(255.0, np.float32)
        st["rgb_mean"] = np.array(RGB_MEAN, np.float32)
    else:
        for k, r in enumerate(STAGES[scale]):
            conv(f"upconv{k + 1}", F * r * r, F)
        conv("conv_hr", F, F)
        conv("conv_last", 3, F, 0.1)
        st["conv_last.bias"] = (0.3 + 0.2 * rng.standard_normal(3)).astype(np.float32)
    return st


def _describe(state: dict):
    """-> (preset, B, upsampling conv names, res_scale, range, mean) read off the keys."""
    edsr = "conv_after_body.weight" in state
    B = len({k.split(".")[1] for k in state if k.startswith("body.")})
    if edsr:
        ups = sorted((k[:-7] for k in state if k.startswith("upsample.") and k.endswith(".weight")), key=lambda n: int(n.split(".")[1]))
        return ("edsr", B, ups, np.float32(state.get("res_scale", 1.0)), np.float32(state.get("img_range", 255.0)),
                np.asarray(state.get("rgb_mean", RGB_MEAN), np.float32))
    ups = [n for n in ("upconv1", "upconv2") if f"{n}.weight" in state]
    return "msr", B, ups, np.float32(1.0), np.float32(1.0), np.zeros(3, np.float32)


def _r_of(state, name) -> int:
    F = np.asarray(state["conv_first.weight"]).shape[0]
    return int(round((np.asarray(state[f"{name}.weight"]).shape[0] / F) ** 0.5))


def forward(state: dict, img: np.ndarray, dtype: str = "float64") -> np.ndarray:
    """-> (h s, w s, 3) array of `dtype`, unclamped."""
    import torch
    import torch.nn.functional as Fn
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    preset, B, ups, res_scale, rng_, mean = _describe(state)

    def conv(name, y):
        return Fn.conv2d(y, torch.from_numpy(np.asarray(state[f"{name}.weight"])).to(dt),
                         torch.from_numpy(np.asarray(state[f"{name}.bias"])).to(dt), stride=1, padding=1)

    p = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None]       # a copy: cached images are read-only
    p = (p.to(torch.float32) / 255.0).to(dt)                          # the contract's fp32 division, exact in float64 afterwards
    meant = torch.from_numpy(mean).to(dt).view(1, 3, 1, 1)
    rs, rg = float(res_scale), float(rng_)                            # the fp32 constants, exactly
    with torch.no_grad():
        if preset == "msr":
            slope = float(np.float32(0.1))                            # the fp32 slope is the parameter
            t = Fn.leaky_relu(conv("conv_first", p), slope)
            for i in range(B):
                t = t + conv(f"body.{i}.conv2", Fn.relu(conv(f"body.{i}.conv1", t)))
            s = 1
            for name in ups:
                r = _r_of(state, name)
                t = Fn.leaky_relu(Fn.pixel_shuffle(conv(name, t), r), slope)
                s *= r
            o = conv("conv_last", Fn.leaky_relu(conv("conv_hr", t), slope))
            o = o + Fn.interpolate(p, scale_factor=s, mode="bilinear", align_corners=False)
        else:
            x = (p - meant) * rg
            h = conv("conv_first", x)
            t = h
            for i in range(B):
                t = t + conv(f"body.{i}.conv2", Fn.relu(conv(f"body.{i}.conv1", t))) * rs
            t = conv("conv_after_body", t) + h
            for name in ups:
                t = Fn.pixel_shuffle(conv(name, t), _r_of(state, name))
            o = conv("conv_last", t) / rg + meant
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


def _act(y: np.ndarray, a) -> np.ndarray:
    return np.where(y >= 0, y, np.float32(a) * y)


def _shuffle(v: np.ndarray, r: int) -> np.ndarray:
    """u[c, Y, X] = v[c r^2 + (Y % r) r + (X % r), Y / r, X / r]"""
    C, h, w = v.shape[0] // (r * r), v.shape[1], v.shape[2]
    c, Y, X = np.meshgrid(np.arange(C), np.arange(h * r), np.arange(w * r), indexing="ij")
    return v[c * r * r + (Y % r) * r + (X % r), Y // r, X // r]


def _fmaf(a, b, c) -> np.ndarray:
    """fp32 fmaf: the product of two fp32 values is exact in float64."""
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def bilinear_base(p: np.ndarray, s: int) -> np.ndarray:
    """The header's bilinear base in numpy fp32, in its evaluation order: p (3, h, w) fp32 -> (3, h s, w s)."""
    f = np.float32
    _, h, w = p.shape
    rscale = f(1.0 / s)

    def axis(n_out, n_in):
        src = np.maximum(rscale * (np.arange(n_out).astype(f) + f(0.5)) - f(0.5), f(0.0)).astype(f)
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        l1 = (src - i0.astype(f)).astype(f)
        return i0, i1, (f(1.0) - l1).astype(f), l1

    y0, y1, ly0, ly1 = axis(h * s, h)
    x0, x1, lx0, lx1 = axis(w * s, w)
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    top = lx0 * p[:, y0][:, :, x0] + lx1 * p[:, y0][:, :, x1]
    bot = lx0 * p[:, y1][:, :, x0] + lx1 * p[:, y1][:, :, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == f
    return out


def chain_forward(state: dict, img: np.ndarray) -> np.ndarray:
    """The forward in plain numpy fp32, summed in the order csrc/sr_resnet.hip documents (_srnet_ref._chain_conv: the head as an
    fmaf chain, every other convolution bias, channel pairs, taps, even then odd channel), the skip as one fmaf, the shuffle and
    the bilinear base written out.  No torch: a second statement of the contract beside forward().  -> float32 (h s, w s, 3)."""
    f = np.float32
    preset, B, ups, res_scale, rng_, mean = _describe(state)
    a = f(0.1) if preset == "msr" else f(1.0)

    def conv(name, y, fused=False):
        out = _chain_conv(y, np.asarray(state[f"{name}.weight"]), np.asarray(state[f"{name}.bias"]), fused=fused)
        assert out.dtype == f
        return out

    p = (np.ascontiguousarray(img).astype(f) / f(255.0)).transpose(2, 0, 1)
    x = ((p - mean[:, None, None]) * rng_).astype(f)
    h = _act(conv("conv_first", x, fused=True), a)
    t = h
    for i in range(B):
        t = _fmaf(res_scale, conv(f"body.{i}.conv2", _act(conv(f"body.{i}.conv1", t), 0.0)), t)
    if preset == "edsr":
        t = conv("conv_after_body", t) + h
    s = 1
    for name in ups:
        r = _r_of(state, name)
        t = _act(_shuffle(conv(name, t), r), a)
        s *= r
    if preset == "msr":
        t = _act(conv("conv_hr", t), a)
    y = conv("conv_last", t)
    o = y / rng_ + mean[:, None, None]
    if preset == "msr":
        o = o + bilinear_base(p, s)
    assert o.dtype == f
    return np.ascontiguousarray(o.transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def case(preset: str, F: int, B: int, s: int, h: int, w: int, res_scale: float = 1.0):
    """One shared reference per case, computed once: (state, image, float64 forward, e32 = max|float32 - float64|)."""
    state = synthetic_state(preset, F, B, s, res_scale=res_scale)
    img = make_image(h, w)
    f64 = forward(state, img, "float64")
    f32 = forward(state, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for a in (img, f64):
        a.setflags(write=False)
    return state, img, f64, e32


@functools.lru_cache(maxsize=None)
def chain_case(preset: str, F: int, B: int, s: int, h: int, w: int, res_scale: float = 1.0):
    """The second yardstick of a case, computed once: (chain_forward's output, e_chain = max|chain - float64|)."""
    state, img, f64, _ = case(preset, F, B, s, h, w, res_scale)
    chain = chain_forward(state, img)
    chain.setflags(write=False)
    return chain, float(np.max(np.abs(chain.astype(np.float64) - f64)))


def case_id(c) -> str:
    return f"{c[0]}-F{c[1]}-B{c[2]}-x{c[3]}-{c[4]}x{c[5]}"


# ---------------------------------------------------------------------------------------------------------------------------
# The whole descriptor (sr_resnet_desc of include/sr_hip.h), of which the two presets above are two points.
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Desc:
    """The header's fields under the header's names (so that _native.resnet_desc(**dataclasses.asdict(d)) builds the C struct)."""
    n_feat: int
    n_blocks: int
    scale: int
    long_skip: bool = False
    conv_hr: bool = False
    bilinear_base: bool = False
    a_head: float = 1.0
    a_up: float = 1.0
    a_hr: float = 1.0
    res_scale: float = 1.0
    mean: tuple = (0.0, 0.0, 0.0)
    range: float = 1.0                                                # noqa: A003 (the header's name)


def conv_roles(desc: Desc):
    """(role, cout, cin) of every convolution in sr_resnet_create's order, restated from the header: head, (conv1, conv2) per
    block, conv_after_body if long_skip, the upsampling stages, conv_hr if conv_hr, the last convolution."""
    F = desc.n_feat
    out = [("head", F, 3)]
    for i in range(desc.n_blocks):
        out += [(f"conv1.{i}", F, F), (f"conv2.{i}", F, F)]
    if desc.long_skip:
        out.append(("after_body", F, F))
    out += [(f"up.{k}", F * r * r, F) for k, r in enumerate(STAGES[desc.scale])]
    if desc.conv_hr:
        out.append(("hr", F, F))
    return out + [("last", 3, F)]


def desc_of_state(state: dict):
    """A preset's state dict as (Desc, weights, biases) in sr_resnet_create's order."""
    preset, B, ups, res_scale, rng_, mean = _describe(state)
    F = np.asarray(state["conv_first.weight"]).shape[0]
    s = int(np.prod([_r_of(state, n) for n in ups])) if ups else 1
    names = ["conv_first"] + [f"body.{i}.conv{j}" for i in range(B) for j in (1, 2)]
    if preset == "edsr":
        desc = Desc(F, B, s, long_skip=True, res_scale=float(res_scale), mean=tuple(float(v) for v in mean), range=float(rng_))
        names += ["conv_after_body"] + ups + ["conv_last"]
    else:
        desc = Desc(F, B, s, conv_hr=True, bilinear_base=True, a_head=0.1, a_up=0.1, a_hr=0.1)
        names += ups + ["conv_hr", "conv_last"]
    return desc, [np.asarray(state[f"{n}.weight"]) for n in names], [np.asarray(state[f"{n}.bias"]) for n in names]


def _f32c(v) -> float:
    """The fp32 value of a descriptor constant, as a Python float: the contract's parameter."""
    return float(np.float32(v))


def forward_desc(desc: Desc, weights, biases, img: np.ndarray, dtype: str = "float64", record: list | None = None) -> np.ndarray:
    """The header's eight steps with torch's operators -> (h s, w s, 3) array of `dtype`, unclamped.  The fp32 constants are
    used exactly.  record: a list that receives (role, convolution input, convolution output, stored result) per convolution
    as numpy arrays (CHW), the stored result being what follows the activation / skip add / shuffle (the last: the output)."""
    import torch
    import torch.nn.functional as Fn
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    roles = conv_roles(desc)
    assert len(weights) == len(biases) == len(roles), (len(weights), len(roles))
    k = [0]
    pending = []

    def conv(y):
        role, cout, cin = roles[k[0]]
        w, b = np.asarray(weights[k[0]]), np.asarray(biases[k[0]])
        assert w.shape == (cout, cin, 3, 3) and b.shape == (cout,), (role, w.shape, b.shape)
        k[0] += 1
        out = Fn.conv2d(y, torch.from_numpy(np.array(w)).to(dt), torch.from_numpy(np.array(b)).to(dt), stride=1, padding=1)   # copies: cached arrays are read-only
        pending.append((role, y, out))
        return out

    def stored(t):
        if record is not None:
            role, y, out = pending[-1]
            record.append((role, y[0].numpy().copy(), out[0].numpy().copy(), t[0].numpy().copy()))
        return t

    def act(y, a):
        a = _f32c(a)                                                  # the fp32 slope is the parameter; 1.0: no activation
        return y if a == 1.0 else Fn.leaky_relu(y, a)

    p = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None]       # a copy: cached images are read-only
    p = (p.to(torch.float32) / 255.0).to(dt)                          # the contract's fp32 division, exact in float64 afterwards
    meant = torch.from_numpy(np.asarray(desc.mean, np.float32)).to(dt).view(1, 3, 1, 1)
    rs, rg = _f32c(desc.res_scale), _f32c(desc.range)
    with torch.no_grad():
        x = (p - meant) * rg
        h = stored(act(conv(x), desc.a_head))
        t = h
        for _ in range(desc.n_blocks):
            u = stored(Fn.relu(conv(t)))
            t = stored(t + conv(u) * rs)
        if desc.long_skip:
            t = stored(conv(t) + h)
        for r in STAGES[desc.scale]:
            t = stored(act(Fn.pixel_shuffle(conv(t), r), desc.a_up))
        if desc.conv_hr:
            t = stored(act(conv(t), desc.a_hr))
        o = conv(t) / rg + meant
        if desc.bilinear_base:
            o = o + (p if desc.scale == 1 else Fn.interpolate(p, scale_factor=desc.scale, mode="bilinear", align_corners=False))
        stored(o)
    assert k[0] == len(roles)
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


def chain_forward_desc(desc: Desc, weights, biases, img: np.ndarray) -> np.ndarray:
    """The header's eight steps in plain numpy fp32, summed in the documented order (chain_forward, generalised).  No torch.
    -> float32 (h s, w s, 3)."""
    f = np.float32
    roles = conv_roles(desc)
    assert len(weights) == len(biases) == len(roles), (len(weights), len(roles))
    k = [0]

    def conv(y, fused=False):
        out = _chain_conv(y, np.asarray(weights[k[0]]), np.asarray(biases[k[0]]), fused=fused)
        k[0] += 1
        assert out.dtype == f
        return out

    mean, rng_, res_scale = np.asarray(desc.mean, f), f(desc.range), f(desc.res_scale)
    p = (np.ascontiguousarray(img).astype(f) / f(255.0)).transpose(2, 0, 1)
    x = ((p - mean[:, None, None]) * rng_).astype(f)
    h = _act(conv(x, fused=True), desc.a_head)
    t = h
    for _ in range(desc.n_blocks):
        t = _fmaf(res_scale, conv(_act(conv(t), 0.0)), t)
    if desc.long_skip:
        t = conv(t) + h
    for r in STAGES[desc.scale]:
        t = _act(_shuffle(conv(t), r), desc.a_up)
    if desc.conv_hr:
        t = _act(conv(t), desc.a_hr)
    y = conv(t)
    o = y / rng_ + mean[:, None, None]
    if desc.bilinear_base:
        o = o + bilinear_base(p, desc.scale)
    assert o.dtype == f and k[0] == len(roles)
    return np.ascontiguousarray(o.transpose(1, 2, 0))


def synthetic_weights(desc: Desc, seed: int = 20260313):
    """synthetic_state's distributions for any descriptor -> (weights, biases): convolutions N(0, sqrt(2 / (9 cin))), the
    convolution feeding a skip add (every conv2, conv_after_body) and the last convolution x 0.1, biases N(0, 0.01) -- the last
    convolution's N(0.3, 0.2) under a bilinear base, so that a good share of the output clamps at 1."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for role, cout, cin in conv_roles(desc):
        gain = 0.1 if role.startswith("conv2") or role in ("after_body", "last") else 1.0
        ws.append((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * gain).astype(np.float32))
        bs.append((rng.standard_normal(cout) * 0.01).astype(np.float32))
    if desc.bilinear_base:
        bs[-1] = (0.3 + 0.2 * rng.standard_normal(3)).astype(np.float32)
    return ws, bs


# The descriptor-space list: distinct non-preset values in every field, F = 64, an 11 x 37 image (one full 8 x 32 block plus a
# tail of 3 rows and 5 columns, with a pitch that is no multiple of 4).
DESC_H, DESC_W = 11, 37
_BASE = dict(a_head=0.25, a_up=0.05, a_hr=0.5, res_scale=0.5, mean=(0.45, 0.30, 0.60), range=2.0)


def _d(B, s, ls, hr, bb, **over):
    return Desc(64, B, s, bool(ls), bool(hr), bool(bb), **{**_BASE, **over})


# (id, descriptor)
DESC_CASES = ([(f"flags{ls}{hr}{bb}-B1-x2", _d(1, 2, ls, hr, bb)) for ls in (0, 1) for hr in (0, 1) for bb in (0, 1)]
              + [(f"flags111-B1-x{s}", _d(1, s, 1, 1, 1)) for s in (1, 3, 4)]
              + [("flags100-B0-x1", _d(0, 1, 1, 0, 0)), ("flags100-B0-x2", _d(0, 2, 1, 0, 0)),        # the long skip reads h twice
                 ("flags110-B3-x2", _d(3, 2, 1, 1, 0)),                                                # three rotations behind a kept h
                 ("a_up-zero", _d(1, 2, 1, 1, 1, a_up=0.0)), ("a_hr-negative", _d(1, 2, 1, 1, 1, a_hr=-0.5)),
                 ("a_head-above-1", _d(1, 2, 1, 1, 1, a_head=1.5)), ("res_scale-negative", _d(1, 2, 1, 1, 1, res_scale=-0.5)),
                 ("range-255-base", _d(1, 2, 1, 1, 1, range=255.0))])


def desc_id(c) -> str:
    return c[0]


@functools.lru_cache(maxsize=None)
def desc_case(desc: Desc, h: int = DESC_H, w: int = DESC_W, seed: int = 20260313):
    """One shared reference per descriptor, computed once: (weights, biases, image, float64 forward, e32)."""
    ws, bs = synthetic_weights(desc, seed)
    img = make_image(h, w)
    f64 = forward_desc(desc, ws, bs, img, "float64")
    f32 = forward_desc(desc, ws, bs, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for a in [img, f64] + ws + bs:
        a.setflags(write=False)
    return ws, bs, img, f64, e32


@functools.lru_cache(maxsize=None)
def desc_chain_case(desc: Desc, h: int = DESC_H, w: int = DESC_W, seed: int = 20260313):
    """The second yardstick of a descriptor, computed once: (chain_forward_desc's output, e_chain = max|chain - float64|)."""
    ws, bs, img, f64, _ = desc_case(desc, h, w, seed)
    chain = chain_forward_desc(desc, ws, bs, img)
    chain.setflags(write=False)
    return chain, float(np.max(np.abs(chain.astype(np.float64) - f64)))


# ---------------------------------------------------------------------------------------------------------------------------
# Exact-arithmetic networks: pixels in {0, 255}, dyadic mean, a power-of-two range, weights in {-1, 0, 1}, integer biases, slopes
# and res_scale powers of two or 0.  Every value is a multiple of a per-layer unit 2^-k and every partial sum of every
# convolution, in any order, stays below 2^24 units (exact_proof), so fp32 holds it exactly: the summation order and whatever the
# MFMA does inside its two-term step cannot change a bit, and the GPU must equal chain_forward_desc with zero tolerance.
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_MEAN = (0.0, 0.5, 0.25)
LAST_NNZ = 24                     # 3 couts x 24 = the 72 (cin mod 8, tap) pairs of the MFMA convolution's chunk


def exact_image(h: int, w: int, seed: int = 5) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def exact_weights(desc: Desc, nnz: int = 4, seed: int = 1):
    """Weights in {-1, 0, 1} with nnz non-zeros per output channel (the last convolution: LAST_NNZ), biases integers in
    [-2, 2].  The n-th non-zero of a convolution sits at (cin mod 8, tap) pair (n + seeded shift) mod 72 -- consecutive within
    a cout, hence distinct, and every pair is used -- in a seeded cin chunk (every chunk is used), with a seeded sign.  The
    head (3 channels) walks its 27 (cin, tap) positions the same way."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for role, cout, cin in conv_roles(desc):
        per = LAST_NNZ if role == "last" else nnz
        n = np.arange(cout * per)
        if cin == 3:
            q = (n + rng.integers(27)) % 27
            ci, tap = q % 3, q // 3
        else:
            q = (n + rng.integers(72)) % 72
            ci, tap = rng.permutation(n % (cin // 8)) * 8 + q % 8, q // 8
        w = np.zeros((cout, cin, 9), np.float32)
        w[n // per, ci, tap] = rng.choice(np.array([-1.0, 1.0], np.float32), n.size)
        ws.append(w.reshape(cout, cin, 3, 3))
        bs.append(rng.integers(-2, 3, cout).astype(np.float32))
    return ws, bs


def probe_weights(desc: Desc, role: str, tap: int, seed: int = 3):
    """A one-hot probe: convolution `role` has weight 1 at one (cin, tap) per cout, the cins a seeded permutation of the
    channels (an upsampling stage: of its F r^2 couts, modulo F; the last convolution: the first three of it); every other
    convolution is the centre-tap identity -- the head copies channel c mod 3 and adds the bias (c mod 7) - 3, so that every
    feature channel is distinct and of both signs and non-zero at the border; an upsampling stage reads channel co / r^2 (a
    nearest upsample); the last convolution sums the channels c = cout mod 3 (every channel is seen in the output).  The
    output is then a shifted, permuted copy of the head's features with zeros entering at the true image border only."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    roles = conv_roles(desc)
    assert role in [r for r, _, _ in roles] and role != "head"
    for name, cout, cin in roles:
        w = np.zeros((cout, cin, 9), np.float32)
        b = np.zeros(cout, np.float32)
        co = np.arange(cout)
        if name == role:
            w[co, (rng.permutation(max(cout, cin)) % cin)[:cout], tap] = 1.0
        elif name == "head":
            w[co, co % 3, 4] = 1.0
            b = ((co % 7) - 3).astype(np.float32)
        elif name == "last":
            ci = np.arange(cin)
            w[ci % 3, ci, 4] = 1.0
        else:
            w[co, co // (cout // cin), 4] = 1.0
        ws.append(w.reshape(cout, cin, 3, 3))
        bs.append(b)
    return ws, bs


def _dyadic_bits(v: float) -> int:
    """The least k >= 0 with v 2^k an integer."""
    k = 0
    while v * 2.0 ** k != math.floor(v * 2.0 ** k):
        k += 1
        assert k < 30, v
    return k


def _slope_bits(a: float) -> int:
    """Fraction bits a slope adds: 0 for 0, 1 and integers, j for 2^-j."""
    return _dyadic_bits(abs(a))


def exact_proof(desc: Desc, weights, biases, img: np.ndarray):
    """-> one row per convolution: (role, k, bound, units_ok, pre, stored) with 2^-k the unit of the row's values, bound the
    largest value in units of the absolute-value forward sum|w| |x| + |b| (which bounds every partial sum in any order), of the
    skip add's |res_scale y| + |skip| and of the stored result, units_ok whether input, output and stored result are whole
    multiples of the unit, pre the convolution's output and stored what follows activation / skip / shuffle / output step.
    Computed in float64, which is exact here as long as bound < 2^53.  The caller asserts units_ok and bound < 2^24."""
    assert set(np.unique(img)) <= {0, 255}
    g = math.log2(desc.range)
    assert g == int(g) and g >= 0, "range must be a power of two >= 1"
    g = int(g)
    km = max(_dyadic_bits(m) for m in desc.mean)
    rec = []
    out = forward_desc(desc, weights, biases, img, "float64", record=rec)
    base_bits = {1: 0, 2: 4, 4: 6}.get(desc.scale)                  # products of two coefficients in multiples of 1/4 (s = 2), 1/8 (s = 4)
    assert not desc.bilinear_base or base_bits is not None, "the bilinear base is exact at s in {1, 2, 4} only"
    k = max(km - g, 0)                                                # x = (p - mean) range
    k_h = k_blk = None
    rows = []
    for (role, x, pre, st), w, b in zip(rec, weights, biases):
        w, b = np.abs(np.asarray(w, np.float64)), np.abs(np.asarray(b, np.float64))
        ax = np.zeros((x.shape[0], x.shape[1] + 2, x.shape[2] + 2))
        ax[:, 1:-1, 1:-1] = np.abs(x)
        absf = b[:, None, None] + sum(np.tensordot(w[:, :, t // 3, t % 3], ax[:, t // 3:t // 3 + x.shape[1], t % 3:t % 3 + x.shape[2]], 1)
                                      for t in range(9))
        assert (absf >= np.abs(pre) - 1e-9).all()
        k_in = k
        bound = float(absf.max())
        if role == "head":
            k += _slope_bits(desc.a_head)
            k_h = k
        elif role.startswith("conv1"):
            k_blk = k_in
        elif role.startswith("conv2"):
            k = max(k_in + _slope_bits(desc.res_scale), k_blk)
            bound = max(bound, float(np.max(abs(_f32c(desc.res_scale)) * np.abs(pre) + np.abs(st - _f32c(desc.res_scale) * pre))))
        elif role == "after_body":
            k = max(k_in, k_h)
            bound = max(bound, float(np.max(np.abs(pre) + np.abs(st - pre))))
        elif role.startswith("up"):
            k += _slope_bits(desc.a_up)
        elif role == "hr":
            k += _slope_bits(desc.a_hr)
        else:                                                         # y / range + mean (+ base): every step's magnitude
            k = max(k_in + g, km, base_bits if desc.bilinear_base else 0)
            bound = max(bound, float(np.max(np.abs(pre) / desc.range + np.abs(np.asarray(desc.mean))[:, None, None] + 1.0)))
        unit = 2.0 ** -k
        whole = all(np.array_equal(a / u, np.round(a / u)) for a, u in ((x, 2.0 ** -k_in), (pre, 2.0 ** -k_in), (st, unit)))
        bound = max(bound, float(np.abs(st).max())) / unit            # in units of the finest value of the row
        rows.append((role, k, bound, whole, pre, st))
    assert np.array_equal(rows[-1][5].transpose(1, 2, 0), out)
    return rows


# (id, descriptor, h, w, non-zeros per cout): MSRResNet-like, EDSR-like (no base: at s = 3 its coefficients are not dyadic),
# every flag at once, two and four cout tiles (F = 256 at s = 3: 36 shuffle tiles, kept to 9 x 33).
EXACT_NETS = [
    ("msr-B2-x4", Desc(64, 2, 4, False, True, True, a_head=0.5, a_up=0.25, a_hr=0.0, res_scale=0.5, mean=EXACT_MEAN, range=2.0), 11, 37, 4),
    ("edsr-B2-x3", Desc(64, 2, 3, True, False, False, res_scale=0.25, mean=EXACT_MEAN, range=4.0), 11, 37, 4),
    ("flags111-x2", Desc(64, 1, 2, True, True, True, a_head=2.0, a_up=0.5, a_hr=0.25, res_scale=-0.5, mean=EXACT_MEAN, range=2.0), 11, 37, 4),
    ("F128-x2", Desc(128, 1, 2, True, False, True, a_head=0.25, a_up=0.5, res_scale=0.5, mean=EXACT_MEAN, range=1.0), 11, 37, 4),
    ("F256-x3", Desc(256, 1, 3, True, True, False, a_head=0.5, a_up=0.0, a_hr=0.5, res_scale=0.5, mean=EXACT_MEAN, range=2.0), 9, 33, 4),
]

# One-hot probes (id, descriptor, probed role, tap): every tap in both body convolutions (the slope and the in-place skip
# epilogues), one off-centre tap in a shuffle stage of r = 2 and of r = 3, and one in the last convolution.
_PROBE = dict(a_head=0.5, a_up=0.25, a_hr=0.5, res_scale=0.5, mean=EXACT_MEAN, range=2.0)
PROBES = ([(f"{role}-tap{t}", Desc(64, 1, 2, False, True, True, **_PROBE), role, t) for role in ("conv1.0", "conv2.0") for t in range(9)]
          + [("up.0-r2-tap2", Desc(64, 1, 2, True, False, True, **_PROBE), "up.0", 2),
             ("up.0-r3-tap3", Desc(64, 1, 3, True, True, False, **_PROBE), "up.0", 3),
             ("last-tap7", Desc(64, 1, 2, False, True, True, **_PROBE), "last", 7)])
PROBE_H, PROBE_W = 11, 37


@functools.lru_cache(maxsize=None)
def exact_case(name: str):
    """An exact network or probe by id, computed once: (descriptor, weights, biases, image, chain_forward_desc's output)."""
    for nid, desc, h, w, nnz in EXACT_NETS:
        if nid == name:
            ws, bs = exact_weights(desc, nnz)
            img = exact_image(h, w)
            break
    else:
        desc, role, tap = next((d, r, t) for nid, d, r, t in PROBES if nid == name)
        ws, bs = probe_weights(desc, role, tap)
        img = exact_image(PROBE_H, PROBE_W)
    chain = chain_forward_desc(desc, ws, bs, img)
    for a in [img, chain] + ws + bs:
        a.setflags(write=False)
    return desc, ws, bs, img, chain
