"""Torch-CPU restatement of the RRDB backend's contract (include/sr_hip.h, "RRDBNet") -- the yardstick of tests/test_gpu_rrdb.py
and tests/test_rrdb_host.py -- plus seeded synthetic weights under BasicSR's key names.

PARITY UNPINNED: the BasicSR / Real-ESRGAN packages (RRDBNet) and their checkpoints do not exist offline; this file restates
the published forward with torch's own operators:

    dense block   x_k = lrelu(conv_k(cat(x, x_1 .. x_{k-1}))), k = 1 .. 4;  out = conv_5(cat(x, x_1 .. x_4)) * beta + x
    RRDB          out = rdb3(rdb2(rdb1(r))) * beta + r
    network       h = conv_first(x);  f = conv_body(RRDB_B(.. RRDB_1(h))) + h;
                  f = lrelu(conv_up1(interpolate(f, 2, nearest)));  f = lrelu(conv_up2(interpolate(f, 2, nearest)));
                  o = conv_last(lrelu(conv_hr(f)))                                       (lrelu slope 0.2, beta 0.2)

in float32 (what a torch user would run) and float64 (the truth the bounds are taken against), and a second time in plain
numpy fp32 in the documented summation order (chain_forward).  It reads the state dict on its own (it does not use the
product's parser).  The fp32 values of slope and beta are the contract's parameters, so the float64 forward uses those fp32
values exactly.  Also here: the plan rule restated (halo, piece counts, workspace), the exact-arithmetic networks and the
one-hot probes whose every partial sum is representable in fp32, so that any summation order gives the same bits."""
from __future__ import annotations

import functools

import numpy as np

from _srnet_ref import check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)

# (F, G, B, h, w) of the float / u8 accuracy check
CASES = [(64, 32, 1, 19, 37), (64, 32, 2, 24, 40), (128, 64, 1, 17, 40), (64, 64, 1, 9, 33), (192, 32, 1, 16, 33), (256, 64, 1, 8, 32)]
# degenerate images and exact / one-past multiples of the convolution's 8 x 32 block
EDGE_CASES = [(64, 32, 1, h, w) for h, w in [(1, 1), (1, 40), (40, 1), (8, 32), (9, 33)]]
# conv_last's bias per channel: the output is conv_last's value alone (no base image), so one channel sits at the lower clamp,
# one mid-range and one at the upper clamp.  Shares of the outputs of CASES[0] that clamp (recorded from the float64
# restatement, printed by tests/test_rrdb_host.py): 2.5 % at 0 and 12.1 % at 1.
LAST_BIAS = (0.02, 0.5, 0.98)
# ... and on the degenerate shapes.  The documented order starts every chain from its bias, so with a bias near 1 each of
# conv_last's 576 roundings is at ulp(1), about 1e-6 in all whatever the image; torch's float32 convolution adds the bias last,
# and on a one-row or one-pixel image, where two thirds of the taps are padding, its whole error is 6e-8 .. 2.5e-7.  The order
# alone then sits at 7 .. 16 e32 with LAST_BIAS (measured, eight weight seeds alike) -- the bar would measure the bias, not the
# kernels.  The edge shapes are there for their index arithmetic and are too small to clamp at both ends anyway, so they take
# small biases: e_chain / e32 is then 1.4 .. 2.7.
EDGE_LAST_BIAS = (0.0, 0.06, 0.12)


def conv_names(B: int):
    """BasicSR's names of every convolution in sr_rrdb_create's order."""
    return (["conv_first"] + [f"body.{i}.rdb{d}.conv{k}" for i in range(B) for d in (1, 2, 3) for k in range(1, 6)]
            + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"])


def conv_shapes(F: int, G: int, B: int):
    """(cout, cin) of every convolution, in the same order."""
    dense = [(G, F + k * G) for k in range(4)] + [(F, F + 4 * G)]
    return [(F, 3)] + dense * (3 * B) + [(F, F)] * 4 + [(3, F)]


def synthetic_state(F: int, G: int, B: int, seed: int = 20260313, last_bias=LAST_BIAS) -> dict:
    """Seeded weights under BasicSR's key names.  Convolutions N(0, sqrt(2 / (9 cin))), every conv5 and conv_last x 0.1, biases
    N(0, 0.01); conv_last's bias is last_bias."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, (cout, cin) in zip(conv_names(B), conv_shapes(F, G, B)):
        gain = 0.1 if name.endswith("conv5") or name == "conv_last" else 1.0
        st[f"{name}.weight"] = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * gain).astype(np.float32)
        st[f"{name}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
    st["conv_last.bias"] = np.array(last_bias, np.float32)
    return st


def state_of(ws, bs, B: int) -> dict:
    st = {}
    for name, w, b in zip(conv_names(B), ws, bs):
        st[f"{name}.weight"], st[f"{name}.bias"] = w, b
    return st


def _dims(state: dict):
    F = np.asarray(state["conv_first.weight"]).shape[0]
    B = len({k.split(".")[1] for k in state if k.startswith("body.")})
    G = np.asarray(state["body.0.rdb1.conv1.weight"]).shape[0] if B else 32
    return F, G, B


def arrays(state: dict):
    """(weights, biases) in sr_rrdb_create's order."""
    names = conv_names(_dims(state)[2])
    return [np.asarray(state[f"{n}.weight"]) for n in names], [np.asarray(state[f"{n}.bias"]) for n in names]


def forward(state: dict, img: np.ndarray, dtype: str = "float64", slope: float = 0.2, beta: float = 0.2) -> np.ndarray:
    """-> (4 h, 4 w, 3) array of `dtype`, unclamped."""
    import torch
    import torch.nn.functional as Fn
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    _, _, B = _dims(state)
    a, bt = float(np.float32(slope)), float(np.float32(beta))         # the fp32 constants, exactly

    def conv(name, y):
        return Fn.conv2d(y, torch.from_numpy(np.array(state[f"{name}.weight"])).to(dt),
                         torch.from_numpy(np.array(state[f"{name}.bias"])).to(dt), stride=1, padding=1)

    def rdb(name, x):
        feats = [x]
        for k in range(1, 5):
            feats.append(Fn.leaky_relu(conv(f"{name}.conv{k}", torch.cat(feats, 1)), a))
        return conv(f"{name}.conv5", torch.cat(feats, 1)) * bt + x

    x = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None]       # a copy: cached images are read-only
    x = (x.to(torch.float32) / 255.0).to(dt)                          # the contract's fp32 division, exact in float64 afterwards
    with torch.no_grad():
        h = conv("conv_first", x)
        t = h
        for i in range(B):
            r = t
            for d in (1, 2, 3):
                t = rdb(f"body.{i}.rdb{d}", t)
            t = t * bt + r
        f = conv("conv_body", t) + h
        f = Fn.leaky_relu(conv("conv_up1", Fn.interpolate(f, scale_factor=2, mode="nearest")), a)
        f = Fn.leaky_relu(conv("conv_up2", Fn.interpolate(f, scale_factor=2, mode="nearest")), a)
        o = conv("conv_last", Fn.leaky_relu(conv("conv_hr", f), a))
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


def _act(y: np.ndarray, a) -> np.ndarray:
    return np.where(y >= 0, y, np.float32(a) * y)


def _fmaf(a, b, c) -> np.ndarray:
    """fp32 fmaf: the product of two fp32 values is exact in float64."""
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _nearest2(v: np.ndarray) -> np.ndarray:
    """n[c, Y, X] = v[c, Y >> 1, X >> 1]"""
    Y, X = np.arange(v.shape[1] * 2) >> 1, np.arange(v.shape[2] * 2) >> 1
    return np.ascontiguousarray(v[:, Y][:, :, X])


def chain_conv(x: np.ndarray, w: np.ndarray, b: np.ndarray, fused: bool = False) -> np.ndarray:
    """3 x 3, zero padding 1, fp32, one output = one sequential chain: (cin, h, w) -> (cout, h, w); _srnet_ref._chain_conv's
    orders.  fused (the head): bias, channels ascending, taps ascending, each term one fmaf.  not fused: bias, then channel
    pairs (2p, 2p + 1) ascending, then taps ascending, then the even and the odd channel, each term one rounded fp32 multiply and
    one rounded fp32 add.  A term whose weights are zero for every cout is skipped: adding +-0 leaves a sum unchanged unless
    that sum is -0.0, which a chain that starts from a bias other than -0.0 and adds in round-to-nearest never is."""
    cout, cin = w.shape[:2]
    h, wd = x.shape[1:]
    xp = np.zeros((cin, h + 2, wd + 2), np.float32)
    xp[:, 1:-1, 1:-1] = x
    w = np.asarray(w, np.float32).reshape(cout, cin, 9)
    assert not np.signbit(np.asarray(b)[np.asarray(b) == 0]).any()
    acc = np.broadcast_to(np.asarray(b, np.float32)[:, None, None], (cout, h, wd)).copy()
    if fused:
        order = [(c, t) for c in range(cin) for t in range(9)]
    else:
        assert cin % 2 == 0
        order = [(2 * p + k, t) for p in range(cin // 2) for t in range(9) for k in (0, 1)]
    used = np.any(w != 0, axis=0)
    for c, t in order:
        if not used[c, t]:
            continue
        v = xp[c, t // 3:t // 3 + h, t % 3:t % 3 + wd][None]
        wc = w[:, c, t][:, None, None]
        if fused:
            acc = (wc.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = acc + wc * v                            # fp32 product, fp32 sum: two roundings
    assert acc.dtype == np.float32
    return acc


def chain_forward(state: dict, img: np.ndarray, slope: float = 0.2, beta: float = 0.2) -> np.ndarray:
    """The header's seven steps in plain numpy fp32, summed in the documented order over the channels of the concatenation, every
    skip one fmaf (conv_body's: one add), the third dense block's two fmafs in the header's order.  No torch.
    -> float32 (4 h, 4 w, 3), unclamped."""
    f = np.float32
    _, _, B = _dims(state)
    a, bt = f(slope), f(beta)

    def conv(name, y, fused=False):
        return chain_conv(y, np.asarray(state[f"{name}.weight"]), np.asarray(state[f"{name}.bias"]), fused=fused)

    def rdb(name, x):
        cat = x
        for k in range(1, 5):
            cat = np.concatenate([cat, _act(conv(f"{name}.conv{k}", cat), a)], 0)
        return _fmaf(bt, conv(f"{name}.conv5", cat), x)

    x = (np.ascontiguousarray(img).astype(f) / f(255.0)).transpose(2, 0, 1)
    h = conv("conv_first", x, fused=True)
    t = h
    for i in range(B):
        r = t
        for d in (1, 2, 3):
            t = rdb(f"body.{i}.rdb{d}", t)                            # the third: fmaf(beta, y, x) first ...
        t = _fmaf(bt, t, r)                                           # ... then fmaf(beta, that, r)
    v = conv("conv_body", t) + h
    v = _act(conv("conv_up1", _nearest2(v)), a)
    v = _act(conv("conv_up2", _nearest2(v)), a)
    o = conv("conv_last", _act(conv("conv_hr", v), a))
    assert o.dtype == f
    return np.ascontiguousarray(o.transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def case(F: int, G: int, B: int, h: int, w: int):
    """One shared reference per case, computed once: (state, image, float64 forward, e32 = max|float32 - float64|)."""
    state = synthetic_state(F, G, B, last_bias=last_bias_of((F, G, B, h, w)))
    img = make_image(h, w)
    f64 = forward(state, img, "float64")
    f32 = forward(state, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for arr in (img, f64):
        arr.setflags(write=False)
    return state, img, f64, e32


@functools.lru_cache(maxsize=None)
def chain_case(F: int, G: int, B: int, h: int, w: int):
    """The second yardstick of a case, computed once: (chain_forward's output, e_chain = max|chain - float64|)."""
    state, img, f64, _ = case(F, G, B, h, w)
    chain = chain_forward(state, img)
    chain.setflags(write=False)
    return chain, float(np.max(np.abs(chain.astype(np.float64) - f64)))


def last_bias_of(c):
    return EDGE_LAST_BIAS if tuple(c) in EDGE_CASES else LAST_BIAS


def case_id(c) -> str:
    return f"F{c[0]}-G{c[1]}-B{c[2]}-{c[3]}x{c[4]}"


# ---------------------------------------------------------------------------------------------------------------------------
# The plan rule of include/sr_hip.h (sr_rrdb_plan), restated.
# ---------------------------------------------------------------------------------------------------------------------------
TRUNK_CAP = 16 << 30
DEFAULT_TAIL = 256


def _rep_mult(n: int, i: int):
    """(replication factor behind convolution i, resolution multiplier of convolution i) of a network of n convolutions."""
    return (2 if i in (n - 5, n - 4) else 1), (4 if i >= n - 3 else 2 if i == n - 4 else 1)


def extents(B: int, lo: int, hi: int, length: int):
    """One axis of the backward extent rule: the piece [lo, hi) of `length` input pixels -> per convolution its half-open output
    range at its own resolution."""
    n = 15 * B + 6
    out = [None] * n
    na, nb = lo * 4, hi * 4
    for i in range(n - 1, -1, -1):
        r, m = _rep_mult(n, i)
        na, nb = na // r, -(-nb // r)
        out[i] = (na, nb)
        na, nb = max(na - 1, 0), min(nb + 1, length * m)
    return out


def halo(B: int) -> int:
    n = 15 * B + 6
    g = 0
    for i in range(n - 1, -1, -1):
        g = -(-g // _rep_mult(n, i)[0]) + 1
    return g


def _pad4(v: int) -> int:
    return (v + 3) // 4 * 4


def _trunk_bytes(F, G, B, h, w, tile):
    n = 15 * B + 6
    ey = [extents(B, lo, min(lo + tile, h), h) for lo in range(0, h, tile)]
    ex = [extents(B, lo, min(lo + tile, w), w) for lo in range(0, w, tile)]
    p0 = max(e[0][1] - e[0][0] for e in ey) * max(_pad4(e[0][1] - e[0][0]) for e in ex)
    p2 = max(2 * (e[n - 5][1] - e[n - 5][0]) for e in ey) * max(_pad4(2 * (e[n - 5][1] - e[n - 5][0])) for e in ex)
    return 4 * ((3 * (F + 4 * G) + F) * p0 + F * p2)


def plan(F: int, G: int, B: int, h: int, w: int, tile: int = 0, tail: int = 0):
    """-> (halo, trunk pieces, tail sub-pieces, workspace bytes) as the header states them."""
    n = 15 * B + 6
    if tile == 0:
        tile = next((t for t in range(2048, 32, -32) if _trunk_bytes(F, G, B, h, w, t) <= TRUNK_CAP), 32)
    tail = tail or DEFAULT_TAIL
    cnt, side = [], []
    for length in (h, w):
        subs = [(s, min(s + tail, min(lo + tile, length))) for lo in range(0, length, tile) for s in range(lo, min(lo + tile, length), tail)]
        cnt.append(len(subs))
        big = 0
        for lo, hi in subs:
            e = extents(B, lo, hi, length)
            big = max([big] + [(e[i][1] - e[i][0]) * _rep_mult(n, i)[0] for i in (n - 4, n - 3, n - 2)])
        side.append(big)
    p4 = side[0] * _pad4(side[1])
    return halo(B), -(-h // tile) * -(-w // tile), cnt[0] * cnt[1], _trunk_bytes(F, G, B, h, w, tile) + 4 * 2 * F * p4


# ---------------------------------------------------------------------------------------------------------------------------
# Exact-arithmetic networks: pixels in {0, 255}, weights in {-1, 0, 1}, integer biases, slope and beta in {0.5, 0.25}.  Every
# value is a multiple of a per-layer unit 2^-k and every partial sum of every convolution, in any order, stays below 2^24 units
# (exact_proof), so fp32 holds it exactly: no summation order, and nothing the MFMA does inside its two-term step, can change a
# bit, and the GPU must equal chain_forward with zero tolerance.
# ---------------------------------------------------------------------------------------------------------------------------
def exact_image(h: int, w: int, seed: int = 5) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def exact_state(F: int, G: int, B: int, nnz: int, chained: bool, seed: int = 1) -> dict:
    """Weights in {-1, 0, 1} with nnz non-zeros per output channel (conv_last: 24), biases integers in [-2, 2].  The n-th
    non-zero of a convolution sits at (cin mod 8, tap) pair (n + seeded shift) mod 72 -- every pair is used -- in a seeded cin
    chunk, with a seeded sign.  chained: a dense convolution k draws its chunks from the whole concatenation (x_k then depends
    on x_{k-1}: a fraction bit per activation, four deep); otherwise convolutions 1 .. 4 read x alone and only convolution 5
    reads the whole concatenation, which leaves room for the 0.25s."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for name, (cout, cin) in zip(conv_names(B), conv_shapes(F, G, B)):
        per = 24 if name == "conv_last" else nnz
        i = np.arange(cout * per)
        if cin == 3:
            q = (i + rng.integers(27)) % 27
            ci, tap = q % 3, q // 3
        else:
            q = (i + rng.integers(72)) % 72
            span = cin if chained or name.endswith("conv5") or ".rdb" not in name else F
            ci, tap = rng.permutation(i % (span // 8)) * 8 + q % 8, q // 8
        wt = np.zeros((cout, cin, 9), np.float32)
        wt[i // per, ci, tap] = rng.choice(np.array([-1.0, 1.0], np.float32), i.size)
        ws.append(wt.reshape(cout, cin, 3, 3))
        bs.append(rng.integers(-2, 3, cout).astype(np.float32))
    return state_of(ws, bs, B)


# (id, F, G, B, h, w, non-zeros per cout, chained, slope, beta); odd image sizes: the 2 x 2 replication's last row and column
EXACT_NETS = [
    ("chained-F64-G32-B1", 64, 32, 1, 11, 37, 2, True, 0.5, 0.5),
    ("F64-G64-B1-slope-quarter", 64, 64, 1, 9, 35, 2, False, 0.25, 0.5),
    ("F64-G32-B2", 64, 32, 2, 9, 35, 1, False, 0.5, 0.5),                     # the in-place rotation twice
    ("F128-G64-B1-beta-quarter", 128, 64, 1, 9, 33, 2, False, 0.5, 0.25),
    ("F64-G32-B1-both-quarter", 64, 32, 1, 9, 35, 1, False, 0.25, 0.25),
]


def exact_proof(state: dict, img: np.ndarray, slope: float, beta: float):
    """-> (bits, bound, float64 output): the finest unit 2^-bits of any value the network holds (inputs, convolution outputs, stored results) and
    the largest sum|w| |x| + |b| of any convolution -- which bounds every partial sum in any order -- together with every skip
    add's |beta y| + |skip|.  Computed in float64, which is exact here while bound 2^bits < 2^53.  The caller asserts
    bound * 2^bits < 2^24."""
    F, G, B = _dims(state)
    f8 = np.float64
    seen = []
    bound = [0.0]

    def conv(name, y):
        w, b = np.asarray(state[f"{name}.weight"], f8), np.asarray(state[f"{name}.bias"], f8)
        yp = np.pad(y, ((0, 0), (1, 1), (1, 1)))
        hh, ww = y.shape[1:]
        out = b[:, None, None] + sum(np.tensordot(w[:, :, t // 3, t % 3], yp[:, t // 3:t // 3 + hh, t % 3:t % 3 + ww], 1) for t in range(9))
        ab = np.abs(b)[:, None, None] + sum(np.tensordot(np.abs(w[:, :, t // 3, t % 3]), np.abs(yp[:, t // 3:t // 3 + hh, t % 3:t % 3 + ww]), 1)
                                            for t in range(9))
        bound[0] = max(bound[0], float(ab.max()))
        seen.append(out)
        return out

    def keep(v, *terms):
        seen.append(v)
        bound[0] = max(bound[0], float(sum(np.abs(t) for t in terms).max()) if terms else 0.0)
        return v

    def act(y):
        return keep(np.where(y >= 0, y, slope * y))

    def rdb(name, x):
        cat = x
        for k in range(1, 5):
            cat = np.concatenate([cat, act(conv(f"{name}.conv{k}", cat))], 0)
        y = conv(f"{name}.conv5", cat)
        return keep(beta * y + x, beta * y, x)

    assert set(np.unique(img)) <= {0, 255}
    x = np.ascontiguousarray(img).astype(f8).transpose(2, 0, 1) / 255.0
    h = conv("conv_first", x)
    t = h
    for i in range(B):
        r = t
        for d in (1, 2, 3):
            t = rdb(f"body.{i}.rdb{d}", t)
        t = keep(beta * t + r, beta * t, r)
    y = conv("conv_body", t)
    v = keep(y + h, y, h)
    v = act(conv("conv_up1", _nearest2(v)))
    v = act(conv("conv_up2", _nearest2(v)))
    o = conv("conv_last", act(conv("conv_hr", v)))
    bits = 0
    for arr in seen:
        while not np.array_equal(arr * 2.0 ** bits, np.round(arr * 2.0 ** bits)):
            bits += 1
            assert bits < 60
    return bits, bound[0], np.ascontiguousarray(o.transpose(1, 2, 0))


# ---------------------------------------------------------------------------------------------------------------------------
# One-hot probes on F 64, G 32, B 1.  The probed dense convolution (block d, convolution k) has a single unit weight at
# (cout co, concatenation channel j, tap t), so its output plane co is a shifted copy of plane j of the concatenation (zeros
# entering at the true image border only).  Around it: the head is (1 + c / 21) x channel c mod 3 plus the bias (c mod 7) - 3, so every
# feature plane is distinct, of both signs and non-zero at the border; every other dense convolution k <= 4 is a centre-tap copy
# of a rotated x channel (so every x_j plane is distinct too); every other conv5 is zero (its block is the identity); the probed
# block's conv5 forwards the probed plane to feature channel co mod F (k <= 4); conv_body .. conv_hr are centre-tap identities
# and conv_last sums the channels c = cout mod 3 with alternating signs.  slope 0.5, beta 0.5: every value is a small dyadic number.
# The upsampling probes put a whole permutation at one off-centre tap of conv_body, conv_up1 or conv_up2 instead: the shifted
# read crosses the 2 x 2 replication at both stages, on an image of odd size (last row / column).
# ---------------------------------------------------------------------------------------------------------------------------
PROBE_F, PROBE_G, PROBE_H, PROBE_W = 64, 32, 11, 37
PROBE_SLOPE = PROBE_BETA = 0.5


def _segment_ends(k: int):
    """First and last channel of every segment of the concatenation convolution k reads."""
    out = [0, PROBE_F - 1]
    for j in range(1, k):
        out += [PROBE_F + (j - 1) * PROBE_G, PROBE_F + j * PROBE_G - 1]
    return out


def _probe_list():
    out, n = [], 0
    for k in range(1, 6):
        for j in _segment_ends(k):
            d, t = n % 3 + 1, (n * 2 + 1) % 9
            co = (0 if n % 2 else (PROBE_G if k < 5 else PROBE_F) - 1)
            out.append((f"rdb{d}-conv{k}-cin{j}-tap{t}-cout{co}", ("dense", d, k, co, j, t)))
            n += 1
    out += [(f"{name}-tap{t}", ("perm", name, t)) for name, t in (("conv_body", 0), ("conv_up1", 8), ("conv_up1", 2), ("conv_up2", 6),
                                                                  ("conv_up2", 5), ("conv_hr", 1), ("conv_last", 7))]
    return out


PROBES = _probe_list()


def probe_state(spec, seed: int = 3) -> dict:
    F, G = PROBE_F, PROBE_G
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for name, (cout, cin) in zip(conv_names(1), conv_shapes(F, G, 1)):
        w = np.zeros((cout, cin, 9), np.float32)
        b = np.zeros(cout, np.float32)
        co = np.arange(cout)
        parts = name.split(".")
        if name == "conv_first":
            w[co, co % 3, 4] = 1.0 + co // 21
            b = ((co % 7) - 3).astype(np.float32)
        elif len(parts) == 4:                                         # body.0.rdb{d}.conv{k}
            d, k = int(parts[2][3:]), int(parts[3][4:])
            probed = spec[0] == "dense" and (d, k) == spec[1:3]
            if probed:
                w[spec[3], spec[4], spec[5]] = 1.0
            elif k < 5:
                w[co, (co + 7 * k + 3 * d) % F, 4] = 1.0
            elif spec[0] == "dense" and d == spec[1]:                 # the probed block's conv5 shows plane co of x_k
                w[spec[3] % F, F + (spec[2] - 1) * G + spec[3], 4] = 1.0
        elif name == "conv_last":
            ci = np.arange(cin)
            w[ci % 3, ci, spec[2] if spec[0] == "perm" and spec[1] == name else 4] = 1.0 - 2.0 * ((ci // 3) % 2)
        elif spec[0] == "perm" and spec[1] == name:
            w[co, rng.permutation(cin), spec[2]] = 1.0
        else:
            w[co, co, 4] = 1.0
        ws.append(w.reshape(cout, cin, 3, 3))
        bs.append(b)
    return state_of(ws, bs, 1)


@functools.lru_cache(maxsize=None)
def exact_case(name: str):
    """An exact network or probe by id, computed once: (state, image, slope, beta, chain_forward's output)."""
    for nid, F, G, B, h, w, nnz, chained, slope, beta in EXACT_NETS:
        if nid == name:
            state, img = exact_state(F, G, B, nnz, chained), exact_image(h, w)
            break
    else:
        spec = dict(PROBES)[name]
        state, img, slope, beta = probe_state(spec), exact_image(PROBE_H, PROBE_W), PROBE_SLOPE, PROBE_BETA
    chain = chain_forward(state, img, slope, beta)
    for arr in [img, chain] + list(state.values()):
        arr.setflags(write=False)
    return state, img, slope, beta, chain
