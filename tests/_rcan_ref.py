"""Torch-CPU restatement of the RCAN backend's contract (include/sr_hip.h, "RCAN") -- the yardstick of tests/test_gpu_rcan.py
and tests/test_rcan_host.py -- plus seeded synthetic weights under BasicSR's key names.

PARITY UNPINNED: the BasicSR package (RCAN) and its checkpoints do not exist offline; this file restates the published forward
with torch's own operators:

    RCAB     y = conv(relu(conv(t)));  s = sigmoid(conv1x1(relu(conv1x1(adaptive_avg_pool2d(y, 1)))));  out = y * s * res_scale + t
    group    out = conv(RCAB_B(.. RCAB_1(t))) + t
    network  x = (x - mean) * range;  h = conv_first(x);  f = conv_after_body(group_G(.. group_1(h))) + h;
             o = conv_last(pixel_shuffle(upsample(f))) / range + mean

in float32 (what a torch user would run) and float64 (the truth the bounds are taken against), and a second time in plain numpy
in the documented order (chain_forward: fp32 convolution chains, the float64 channel mean through math.fsum, float64
attention).  It reads the state dict on its own (it does not use the product's parser).  res_scale, img_range and rgb_mean ride
in the state as extra entries, the way sr_network.load_network reads them from a .npz; their fp32 values are the contract's
parameters, so the float64 forward uses those fp32 values exactly.  Also here: the mutants that show what the cases can see, the
plan rule restated, the exact-arithmetic networks and the one-hot probes."""
from __future__ import annotations

import functools
import math

import numpy as np

from _resnet_ref import RGB_MEAN, STAGES, _fmaf, _shuffle, exact_image  # noqa: F401
from _srnet_ref import _chain_conv, check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)

RES_SCALE = 0.5                     # not BasicSR's 1: a forward that drops it must show

# (F, R, G, B, s, h, w) of the float / u8 accuracy check: every scale, squeeze widths 4 and 1, B = 0, F = 128 once; shapes of
# exactly one 8 x 32 block, one past it, 2 x 2 blocks with tails in both directions, 5 x 3 blocks
CASES = [(64, 4, 2, 2, 2, 40, 70), (64, 4, 1, 1, 4, 11, 37), (64, 1, 1, 2, 3, 9, 33), (64, 4, 1, 1, 1, 8, 32), (64, 4, 2, 0, 2, 11, 37),
         (128, 4, 1, 1, 2, 11, 37), (64, 1, 2, 1, 1, 40, 70)]
# degenerate images
EDGE_CASES = [(64, 4, 1, 1, 2, h, w) for h, w in [(1, 1), (1, 50), (50, 1)]]
# more than one block and at least one RCAB: where a mean over padded area, a wrong divisor, a shifted s or a dropped res_scale
# must all show
MULTI_BLOCK_CASES = [c for c in CASES if (c[5] > 8 or c[6] > 32) and c[3] > 0]


def case_id(c) -> str:
    return f"F{c[0]}-R{c[1]}-G{c[2]}-B{c[3]}-x{c[4]}-{c[5]}x{c[6]}"


def table_names(G: int, B: int, scale: int):
    """BasicSR's names of every table in sr_rcan_create's order."""
    names = ["conv_first"]
    for g in range(G):
        for b in range(B):
            r = f"body.{g}.residual_group.{b}.rcab"
            names += [f"{r}.0", f"{r}.2", f"{r}.3.attention.1", f"{r}.3.attention.3"]
        names.append(f"body.{g}.conv")
    return names + ["conv_after_body"] + [f"upsample.{2 * k}" for k in range(len(STAGES[scale]))] + ["conv_last"]


def table_shapes(F: int, R: int, G: int, B: int, scale: int):
    """(cout, cin, kernel side) of every table, in the same order."""
    group = [(F, F, 3), (F, F, 3), (R, F, 1), (F, R, 1)] * B + [(F, F, 3)]
    return [(F, 3, 3)] + group * G + [(F, F, 3)] + [(F * r * r, F, 3) for r in STAGES[scale]] + [(3, F, 3)]


def synthetic_state(F: int, R: int, G: int, B: int, scale: int, seed: int = 20260313, res_scale: float = RES_SCALE) -> dict:
    """Seeded weights under BasicSR's key names.  3 x 3 convolutions N(0, sqrt(2 / (9 cin))), conv_last x 0.1, biases N(0, 0.01).
    The attention is drawn so that s spreads over roughly 0.2 .. 0.8 and depends on the mean: b1 in [0.5, 1.5] keeps the squeeze
    layer's relu open (with R = 1 a closed relu would hide the mean altogether), w1 N(0, 0.002 / sqrt(F)) lets the channel means
    (some hundreds in size with range 255) move z1 by some tenths, w2 N(0, 0.25 / sqrt(R)) and b2 in [-1, 1] give logits of
    about +-1.5.  Also res_scale, img_range (255) and rgb_mean entries."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, (cout, cin, ks) in zip(table_names(G, B, scale), table_shapes(F, R, G, B, scale)):
        if ks == 3:
            gain = 0.1 if name == "conv_last" else 1.0
            st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * gain).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
        elif name.endswith("attention.1"):
            st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 1, 1)) * 0.002 / np.sqrt(cin)).astype(np.float32)
            st[f"{name}.bias"] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        else:
            st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 1, 1)) * 0.25 / np.sqrt(cin)).astype(np.float32)
            st[f"{name}.bias"] = rng.uniform(-1.0, 1.0, cout).astype(np.float32)
    st["res_scale"] = np.array(res_scale, np.float32)
    st["img_range"] = np.array(255.0, np.float32)
    st["rgb_mean"] = np.array(RGB_MEAN, np.float32)
    return st


def state_of(ws, bs, G: int, B: int, scale: int, res_scale: float, img_range: float, rgb_mean) -> dict:
    st = {}
    for name, w, b in zip(table_names(G, B, scale), ws, bs):
        st[f"{name}.weight"], st[f"{name}.bias"] = w, b
    st["res_scale"], st["img_range"], st["rgb_mean"] = np.array(res_scale, np.float32), np.array(img_range, np.float32), np.array(rgb_mean, np.float32)
    return st


def _dims(state: dict):
    """-> (F, R, G, B, scale) read off the keys."""
    F = np.asarray(state["conv_first.weight"]).shape[0]
    G = len({k.split(".")[1] for k in state if k.startswith("body.")})
    B = len({k.split(".")[3] for k in state if k.startswith("body.0.residual_group.")})
    R = np.asarray(state["body.0.residual_group.0.rcab.3.attention.1.weight"]).shape[0] if B else max(1, F // 16)
    ups = [k for k in state if k.startswith("upsample.") and k.endswith(".weight")]
    scale = int(np.prod([int(round((np.asarray(state[k]).shape[0] / F) ** 0.5)) for k in ups])) if ups else 1
    return F, R, G, B, scale


def _consts(state: dict):
    return (np.float32(state.get("res_scale", 1.0)), np.float32(state.get("img_range", 255.0)), np.asarray(state.get("rgb_mean", RGB_MEAN), np.float32))


def arrays(state: dict):
    """(weights, biases) in sr_rcan_create's order; the 1 x 1 layers as (out, in)."""
    F, R, G, B, s = _dims(state)
    names = table_names(G, B, s)
    ws = [np.asarray(state[f"{n}.weight"]) for n in names]
    return [w.reshape(w.shape[:2]) if w.shape[2:] == (1, 1) else w for w in ws], [np.asarray(state[f"{n}.bias"]) for n in names]


def _block8x32(h: int, w: int):
    return -(-h // 8) * 8, -(-w // 32) * 32


def forward(state: dict, img: np.ndarray, dtype: str = "float64", mutant: str = "") -> np.ndarray:
    """-> (h s, w s, 3) array of `dtype`, unclamped.  mutant (what a wrong kernel would compute, for the CPU check that the
    cases can see it): 'padded-mean' pools over the whole 8 x 32 blocks the convolution kernel works in, whose lanes beyond the
    image hold the convolution of the zero-extended input; 'divisor' pools over the image but divides by the blocks' pixel
    count; 'shift-s' scales channel c by s[c - 1]; 'no-res-scale' drops res_scale."""
    import torch
    import torch.nn.functional as Fn
    assert mutant in ("", "padded-mean", "divisor", "shift-s", "no-res-scale")
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    F, R, G, B, scale = _dims(state)
    res_scale, rng_, mean = _consts(state)
    rs, rg = (1.0 if mutant == "no-res-scale" else float(res_scale)), float(rng_)            # the fp32 constants, exactly
    hh, ww = img.shape[:2]
    ph, pw = _block8x32(hh, ww)

    def tensor(name, part):
        return torch.from_numpy(np.array(state[f"{name}.{part}"])).to(dt)

    def conv(name, y, pad=1):
        return Fn.conv2d(y, tensor(name, "weight"), tensor(name, "bias"), stride=1, padding=pad)

    p = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None]       # a copy: cached images are read-only
    p = (p.to(torch.float32) / 255.0).to(dt)                          # the contract's fp32 division, exact in float64 afterwards
    meant = torch.from_numpy(np.array(mean)).to(dt).view(1, 3, 1, 1)
    with torch.no_grad():
        h = conv("conv_first", (p - meant) * rg)
        t = h
        for g in range(G):
            gin = t
            for b in range(B):
                name = f"body.{g}.residual_group.{b}.rcab"
                y1 = Fn.relu(conv(f"{name}.0", t))
                y = conv(f"{name}.2", y1)
                if mutant == "padded-mean":
                    pooled = conv(f"{name}.2", Fn.pad(y1, (0, pw - ww, 0, ph - hh))).mean((2, 3), keepdim=True)
                elif mutant == "divisor":
                    pooled = y.sum((2, 3), keepdim=True) / (ph * pw)
                else:
                    pooled = Fn.adaptive_avg_pool2d(y, 1)
                s = torch.sigmoid(conv(f"{name}.3.attention.3", Fn.relu(conv(f"{name}.3.attention.1", pooled, 0)), 0))
                if mutant == "shift-s":
                    s = torch.roll(s, 1, 1)
                t = y * s * rs + t
            t = conv(f"body.{g}.conv", t) + gin
        t = conv("conv_after_body", t) + h
        for k, r in enumerate(STAGES[scale]):
            t = Fn.pixel_shuffle(conv(f"upsample.{2 * k}", t), r)
        o = conv("conv_last", t) / rg + meant
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


def attention(y2: np.ndarray, w1, b1, w2, b2):
    """The header's step 3 on planes y2 (F, h, w) fp32 -> (m[F] fp32, s[F] fp32, z[F] float64): the float64 mean through
    math.fsum over exactly the h w pixels, the two 1 x 1 layers in float64, index ascending, every term one rounded product and
    one rounded add, s = (float)(1 / (1 + exp(-z)))."""
    F = y2.shape[0]
    w1, w2 = np.asarray(w1, np.float32).reshape(-1, F), np.asarray(w2, np.float32).reshape(F, -1)
    R = w1.shape[0]
    n = y2.shape[1] * y2.shape[2]
    m = [np.float32(math.fsum(y2[c].astype(np.float64).ravel().tolist()) / float(n)) for c in range(F)]
    z1 = []
    for j in range(R):
        z = float(b1[j])
        for c in range(F):
            z += float(w1[j, c]) * float(m[c])
        z1.append(z if z > 0.0 else 0.0)
    zs, s = [], []
    for c in range(F):
        z = float(b2[c])
        for j in range(R):
            z += float(w2[c, j]) * z1[j]
        zs.append(z)
        s.append(np.float32(1.0 / (1.0 + math.exp(-z))))
    return np.array(m, np.float32), np.array(s, np.float32), np.array(zs, np.float64)


def chain_forward(state: dict, img: np.ndarray, record: list | None = None) -> np.ndarray:
    """The header's seven steps in plain numpy, in the documented order: every 3 x 3 convolution _srnet_ref._chain_conv (the
    head as an fmaf chain, every other one bias, channel pairs, taps, even then odd channel), relu(y) = y > 0 ? y : +0, the
    attention as attention() above, the product y2 * s[c] rounded to fp32 and then one fmaf with res_scale, the group skip and the
    long skip one add.  No torch.  record: a list that receives every s vector.  -> float32 (h s, w s, 3), unclamped."""
    f = np.float32
    F, R, G, B, scale = _dims(state)
    res_scale, rng_, mean = _consts(state)

    def conv(name, y, fused=False):
        out = _chain_conv(y, np.asarray(state[f"{name}.weight"]), np.asarray(state[f"{name}.bias"]), fused=fused)
        assert out.dtype == f
        return out

    p = (np.ascontiguousarray(img).astype(f) / f(255.0)).transpose(2, 0, 1)
    x = ((p - mean[:, None, None]) * rng_).astype(f)
    h = conv("conv_first", x, fused=True)
    t = h
    for g in range(G):
        gin = t
        for b in range(B):
            name = f"body.{g}.residual_group.{b}.rcab"
            y1 = conv(f"{name}.0", t)
            y1 = np.where(y1 > 0, y1, f(0.0))
            y2 = conv(f"{name}.2", y1)
            _, s, _ = attention(y2, state[f"{name}.3.attention.1.weight"], np.asarray(state[f"{name}.3.attention.1.bias"]),
                                state[f"{name}.3.attention.3.weight"], np.asarray(state[f"{name}.3.attention.3.bias"]))
            if record is not None:
                record.append(s)
            prod = y2 * s[:, None, None]
            assert prod.dtype == f
            t = _fmaf(res_scale, prod, t)
        t = conv(f"body.{g}.conv", t) + gin
    t = conv("conv_after_body", t) + h
    for k, r in enumerate(STAGES[scale]):
        t = _shuffle(conv(f"upsample.{2 * k}", t), r)
    o = conv("conv_last", t) / rng_ + mean[:, None, None]
    assert o.dtype == f
    return np.ascontiguousarray(o.transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def case(F: int, R: int, G: int, B: int, s: int, h: int, w: int):
    """One shared reference per case, computed once: (state, image, float64 forward, e32 = max|float32 - float64|)."""
    state = synthetic_state(F, R, G, B, s)
    img = make_image(h, w)
    f64 = forward(state, img, "float64")
    f32 = forward(state, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for a in (img, f64):
        a.setflags(write=False)
    return state, img, f64, e32


@functools.lru_cache(maxsize=None)
def chain_case(F: int, R: int, G: int, B: int, s: int, h: int, w: int):
    """The second yardstick of a case, computed once: (chain_forward's output, e_chain = max|chain - float64|, every s)."""
    state, img, f64, _ = case(F, R, G, B, s, h, w)
    rec = []
    chain = chain_forward(state, img, record=rec)
    chain.setflags(write=False)
    return chain, float(np.max(np.abs(chain.astype(np.float64) - f64))), rec


# ---------------------------------------------------------------------------------------------------------------------------
# The plan rule of include/sr_hip.h (sr_rcan_plan), restated.
# ---------------------------------------------------------------------------------------------------------------------------
TRUNK_CAP = 16 << 30
DEFAULT_TAIL = 256
TRUNK_BUFS = 5


def _pad4(v: int) -> int:
    return (v + 3) // 4 * 4


def _tail_steps(scale: int):
    """(shuffle factor behind the convolution, resolution multiplier of the convolution) of the tail phase."""
    out, m = [], 1
    for r in STAGES[scale]:
        out.append((r, m))
        m *= r
    return out + [(1, scale)]


def tail_extents(scale: int, lo: int, hi: int, length: int):
    steps = _tail_steps(scale)
    out = [None] * len(steps)
    na, nb = lo * scale, hi * scale
    for i in range(len(steps) - 1, -1, -1):
        r, m = steps[i]
        na, nb = na // r, -(-nb // r)
        out[i] = (na, nb)
        na, nb = max(na - 1, 0), min(nb + 1, length * m)
    return out


def plan(F: int, scale: int, h: int, w: int, tail: int = 0):
    """-> (the tail's halo, tail sub-pieces, workspace bytes) as the header states them."""
    steps = _tail_steps(scale)
    g = 0
    for r, _ in reversed(steps):
        g = -(-g // r) + 1
    tail = tail or DEFAULT_TAIL
    side = []
    for length in (h, w):
        big = 0
        for lo in range(0, length, tail):
            e = tail_extents(scale, lo, min(lo + tail, length), length)
            big = max([big] + [(e[i][1] - e[i][0]) * steps[i][0] for i in range(len(steps) - 1)])
        side.append(big)
    p0, p4 = h * _pad4(w), side[0] * _pad4(side[1])
    return g, -(-h // tail) * -(-w // tail), 4 * (TRUNK_BUFS * F * p0 + 2 * F * p4) + 8 * F * -(-h // 32) + 4 * F


# ---------------------------------------------------------------------------------------------------------------------------
# Exact-arithmetic networks: pixels in {0, 255}, a dyadic mean, a power-of-two range, 3 x 3 weights in {-1, 0, 1}, integer
# biases, res_scale a power of two, and an all-zero second 1 x 1 layer, so that z = 0 and s = 0.5 exactly whatever the mean.
# Every value is a multiple of a unit 2^-k and every partial sum of every convolution, in any order, stays below 2^24 units
# (exact_proof), so fp32 holds it exactly and the GPU must equal chain_forward with zero tolerance.  The channel sums are sums
# of such values below 2^53 units: exact in float64 in any order.
# ---------------------------------------------------------------------------------------------------------------------------
EXACT_MEAN = (0.0, 0.5, 0.25)
LAST_NNZ = 24


def _exact_tables(F, R, G, B, scale, nnz, seed, probe=None):
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for name, (cout, cin, ks) in zip(table_names(G, B, scale), table_shapes(F, R, G, B, scale)):
        co = np.arange(cout)
        if ks == 1:                                               # the first layer: any integers; the second: zero
            first = name.endswith("attention.1")
            ws.append((rng.integers(-2, 3, (cout, cin, 1, 1)) * first).astype(np.float32))
            bs.append((rng.integers(-2, 3, cout) * first).astype(np.float32))
            continue
        w = np.zeros((cout, cin, 9), np.float32)
        b = np.zeros(cout, np.float32)
        if probe is None:
            per = LAST_NNZ if name == "conv_last" else nnz
            n = np.arange(cout * per)
            if cin == 3:
                q = (n + rng.integers(27)) % 27
                ci, tap = q % 3, q // 3
            else:
                q = (n + rng.integers(72)) % 72
                ci, tap = rng.permutation(n % (cin // 8)) * 8 + q % 8, q // 8
            w[n // per, ci, tap] = rng.choice(np.array([-1.0, 1.0], np.float32), n.size)
            b = rng.integers(-2, 3, cout).astype(np.float32)
        elif name == probe[0]:                                    # a permutation of the channels at one tap
            w[co, (rng.permutation(max(cout, cin)) % cin)[:cout], probe[1]] = 1.0
        elif name == "conv_first":                                # every feature plane distinct, of both signs, non-zero at the border
            w[co, co % 3, 4] = 1.0 + co // 21
            b = ((co % 7) - 3).astype(np.float32)
        elif name == "conv_last":
            ci = np.arange(cin)
            w[ci % 3, ci, 4] = 1.0 - 2.0 * ((ci // 3) % 2)
        else:                                                     # centre-tap identity (an upsampling stage: a nearest upsample)
            w[co, co // (cout // cin), 4] = 1.0
        ws.append(w.reshape(cout, cin, 3, 3))
        bs.append(b)
    return ws, bs


# (id, F, R, G, B, scale, h, w, non-zeros per cout, res_scale, range)
EXACT_NETS = [
    ("F64-G2-B1-x4", 64, 4, 2, 1, 4, 11, 37, 2, 0.5, 2.0),
    ("F64-G1-B2-x3", 64, 1, 1, 2, 3, 11, 37, 2, 0.25, 4.0),
    ("F64-G2-B0-x2", 64, 4, 2, 0, 2, 9, 35, 2, 0.5, 2.0),         # groups of one convolution: the buffer rotation without RCABs
    ("F128-G1-B1-x1", 128, 8, 1, 1, 1, 9, 33, 2, 0.5, 1.0),
    ("F64-G3-B1-x2-40x70", 64, 4, 3, 1, 2, 40, 70, 1, 0.5, 2.0),  # 5 x 3 blocks, the in-place group skip twice
]
# (id, table name, tap) on F 64, R 4, G 2, B 2, x2, 11 x 37: a tap of each RCAB convolution (first block of a group: t goes to
# its own buffer; second: in place), the group convolution of the first group (h kept) and of the second (in place), one
# shuffle stage, the last convolution
PROBES = [("rcab0-conv-a-tap0", "body.0.residual_group.0.rcab.0", 0), ("rcab0-conv-b-tap8", "body.0.residual_group.0.rcab.2", 8),
          ("rcab1-conv-a-tap5", "body.1.residual_group.1.rcab.0", 5), ("rcab1-conv-b-tap1", "body.1.residual_group.1.rcab.2", 1),
          ("group0-conv-tap2", "body.0.conv", 2), ("group1-conv-tap6", "body.1.conv", 6), ("after-body-tap3", "conv_after_body", 3),
          ("up-r2-tap7", "upsample.0", 7), ("last-tap1", "conv_last", 1)]
PROBE_NET = (64, 4, 2, 2, 2, 11, 37, 0.5, 2.0)


def exact_state(name: str):
    """-> (state, image) of an exact network or probe by id."""
    for nid, F, R, G, B, s, h, w, nnz, rs, rg in EXACT_NETS:
        if nid == name:
            ws, bs = _exact_tables(F, R, G, B, s, nnz, seed=1)
            return state_of(ws, bs, G, B, s, rs, rg, EXACT_MEAN), exact_image(h, w)
    table, tap = next((t, k) for nid, t, k in PROBES if nid == name)
    F, R, G, B, s, h, w, rs, rg = PROBE_NET
    ws, bs = _exact_tables(F, R, G, B, s, 0, seed=3, probe=(table, tap))
    return state_of(ws, bs, G, B, s, rs, rg, EXACT_MEAN), exact_image(h, w)


@functools.lru_cache(maxsize=None)
def exact_case(name: str):
    """An exact network or probe by id, computed once: (state, image, chain_forward's output)."""
    state, img = exact_state(name)
    chain = chain_forward(state, img)
    for a in [img, chain] + list(state.values()):
        a.setflags(write=False)
    return state, img, chain


def exact_proof(state: dict, img: np.ndarray):
    """-> (bits, bound, float64 output): the finest unit 2^-bits of any value the network holds (inputs, convolution outputs,
    products, stored results) and the largest sum|w| |x| + |b| of any convolution -- which bounds every partial sum in any order
    -- together with every skip add's |terms|.  Computed in float64, which is exact here while bound 2^bits < 2^53.  s = 0.5 is
    asserted, not assumed.  The caller asserts bound * 2^bits < 2^24."""
    f8 = np.float64
    F, R, G, B, scale = _dims(state)
    rs32, rg32, mean32 = _consts(state)
    res_scale, rng_, mean = f8(rs32), f8(rg32), np.asarray(mean32, f8)
    seen, bound = [], [0.0]

    def conv(name, y):
        w, b = np.asarray(state[f"{name}.weight"], f8), np.asarray(state[f"{name}.bias"], f8)
        yp = np.pad(y, ((0, 0), (1, 1), (1, 1)))
        hh, ww = y.shape[1:]
        win = [yp[:, t // 3:t // 3 + hh, t % 3:t % 3 + ww] for t in range(9)]
        out = b[:, None, None] + sum(np.tensordot(w[:, :, t // 3, t % 3], win[t], 1) for t in range(9))
        ab = np.abs(b)[:, None, None] + sum(np.tensordot(np.abs(w[:, :, t // 3, t % 3]), np.abs(win[t]), 1) for t in range(9))
        bound[0] = max(bound[0], float(ab.max()))
        seen.append(out)
        return out

    def keep(v, *terms):
        seen.append(v)
        bound[0] = max(bound[0], float(np.abs(v).max()), float(sum(np.abs(t) for t in terms).max()) if terms else 0.0)
        return v

    assert set(np.unique(img)) <= {0, 255}
    x = keep((np.ascontiguousarray(img).astype(f8).transpose(2, 0, 1) / 255.0 - mean[:, None, None]) * rng_)
    h = conv("conv_first", x)
    t = h
    for g in range(G):
        gin = t
        for b in range(B):
            name = f"body.{g}.residual_group.{b}.rcab"
            y2 = conv(f"{name}.2", keep(np.maximum(conv(f"{name}.0", t), 0.0)))
            _, s, z = attention(y2.astype(np.float32), state[f"{name}.3.attention.1.weight"], np.asarray(state[f"{name}.3.attention.1.bias"]),
                                state[f"{name}.3.attention.3.weight"], np.asarray(state[f"{name}.3.attention.3.bias"]))
            assert (z == 0.0).all() and (s == np.float32(0.5)).all()
            prod = keep(y2 * 0.5)
            t = keep(res_scale * prod + t, res_scale * prod, t)
        y = conv(f"body.{g}.conv", t)
        t = keep(y + gin, y, gin)
    y = conv("conv_after_body", t)
    t = keep(y + h, y, h)
    for k, r in enumerate(STAGES[scale]):
        t = _shuffle(conv(f"upsample.{2 * k}", t), r)
    y = conv("conv_last", t)
    o = keep(keep(y / rng_) + mean[:, None, None], y / rng_, np.broadcast_to(np.abs(mean)[:, None, None], y.shape))
    bits = 0
    for arr in seen:
        while not np.array_equal(arr * 2.0 ** bits, np.round(arr * 2.0 ** bits)):
            bits += 1
            assert bits < 40
    return bits, bound[0], np.ascontiguousarray(o.transpose(1, 2, 0))
