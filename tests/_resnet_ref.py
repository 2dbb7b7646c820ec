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
float64 forward uses those fp32 values exactly."""
from __future__ import annotations

import functools

import numpy as np

from _srnet_ref import _chain_conv, check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)

RGB_MEAN = (0.4488, 0.4371, 0.4040)
STAGES = {1: [], 2: [2], 3: [3], 4: [2, 2]}

# (preset, F, B, s, h, w, res_scale) of the float / u8 accuracy check
CASES = [("msr", 64, 2, 2, 45, 77, 1.0), ("msr", 64, 1, 4, 19, 37, 1.0), ("msr", 64, 1, 3, 33, 41, 1.0), ("msr", 64, 0, 1, 20, 35, 1.0),
         ("edsr", 64, 2, 2, 40, 70, 0.1), ("edsr", 128, 1, 3, 17, 40, 1.0), ("edsr", 256, 1, 4, 12, 35, 0.1)]
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
