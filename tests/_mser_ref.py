"""NumPy / Python restatement of the MSER definition of include/sr_hip.h (component tree, variation, stability with ties
kept, filters, diversity against the nearest passing ancestor), a brute-force tree straight from the definition through
scipy.ndimage.label, the mutants the host test must catch, and the constructed images the host and GPU tests share.

A tree is a dict of int64 arrays in (level, seed) order: level, area, x0, y0, x1, y1, seed, parent (index into the same
order, -1 for the root).  A region is a tuple (polarity, level, area, x0, y0, x1, y1, seed, S)."""
import numpy as np

DEFAULTS = dict(delta=5, min_area=60, max_area=14400, max_variation=0.25, min_diversity=0.2)
FIELDS = ("polarity", "level", "area", "x0", "y0", "x1", "y1", "seed", "S")
TREE_FIELDS = ("level", "area", "x0", "y0", "x1", "y1", "seed", "parent")


def gray_swapped(img):
    """cv2.COLOR_BGR2GRAY applied to RGB data (15-bit rule); cn 1 is the value itself; alpha ignored."""
    img = np.asarray(img)
    if img.ndim == 2:
        return img.copy()
    if img.shape[2] == 1:
        return img[..., 0].copy()
    t = img.astype(np.int64)
    return ((t[..., 0] * 3735 + t[..., 1] * 19235 + t[..., 2] * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def _canonical(level, area, x0, y0, x1, y1, seed, par):
    n = len(level)
    order = sorted(range(n), key=lambda i: (level[i], seed[i]))
    pos = {o: i for i, o in enumerate(order)}
    pick = lambda a: np.array([a[o] for o in order], dtype=np.int64)
    return dict(level=pick(level), area=pick(area), x0=pick(x0), y0=pick(y0), x1=pick(x1), y1=pick(y1), seed=pick(seed),
                parent=np.array([pos[par[o]] if par[o] >= 0 else -1 for o in order], dtype=np.int64))


def tree(g, conn8=False):
    """Sorted-pixel sequential union-find.  Nodes of one level that meet are merged through an alias table."""
    g = np.asarray(g)
    h, w = g.shape
    flat = [int(v) for v in g.ravel()]
    order = np.argsort(g.ravel(), kind="stable")
    uf = list(range(h * w))
    active = [False] * (h * w)
    nodeof = [-1] * (h * w)
    level, area, x0, y0, x1, y1, seed, par, alias = [], [], [], [], [], [], [], [], []

    def find(p):
        while uf[p] != p:
            uf[p] = uf[uf[p]]
            p = uf[p]
        return p

    def res(n):
        while alias[n] != n:
            n = alias[n]
        return n

    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn8 else [])
    for p in order:
        p = int(p)
        t, y, x = flat[p], p // w, p % w
        n = len(level)
        level.append(t); area.append(1); x0.append(x); y0.append(y); x1.append(x); y1.append(y); seed.append(p)
        par.append(-1); alias.append(n)
        active[p] = True
        nodeof[p] = n
        for dy, dx in steps:
            yy, xx = y + dy, x + dx
            if not (0 <= yy < h and 0 <= xx < w) or not active[yy * w + xx]:
                continue
            rp, rq = find(p), find(yy * w + xx)
            if rp == rq:
                continue
            a, b = res(nodeof[rp]), res(nodeof[rq])
            if level[b] == t:
                alias[b] = a
            else:
                par[b] = a
            area[a] += area[b]
            x0[a] = min(x0[a], x0[b]); y0[a] = min(y0[a], y0[b]); x1[a] = max(x1[a], x1[b]); y1[a] = max(y1[a], y1[b])
            seed[a] = min(seed[a], seed[b])
            uf[rq] = rp
            nodeof[rp] = a
    real = [i for i in range(len(level)) if alias[i] == i]
    pos = {o: i for i, o in enumerate(real)}
    pick = lambda a: [a[o] for o in real]
    return _canonical(pick(level), pick(area), pick(x0), pick(y0), pick(x1), pick(y1), pick(seed),
                      [pos[res(par[o])] if par[o] >= 0 else -1 for o in real])


def brute(g):
    """The tree from the definition: for every t the 4-connected components of {g <= t} (scipy.ndimage.label's default
    structure), a node per component that holds a pixel of value t, parents by set inclusion."""
    from scipy import ndimage
    g = np.asarray(g)
    h, w = g.shape
    idx = np.arange(h * w).reshape(h, w)
    nodes = []                                            # (level, frozenset of pixel indices)
    for t in range(256):
        if not (g == t).any():
            continue
        lab, n = ndimage.label(g <= t)
        for c in range(1, n + 1):
            m = lab == c
            if (g[m] == t).any():
                nodes.append((t, frozenset(int(v) for v in idx[m])))
    level, area, x0, y0, x1, y1, seed, par = [], [], [], [], [], [], [], []
    for t, px in nodes:
        ys, xs = [p // w for p in px], [p % w for p in px]
        level.append(t); area.append(len(px)); x0.append(min(xs)); y0.append(min(ys)); x1.append(max(xs)); y1.append(max(ys))
        seed.append(min(px))
        best = -1
        for j, (t2, px2) in enumerate(nodes):
            if t2 > t and px <= px2 and (best < 0 or t2 < nodes[best][0]):
                best = j
        par.append(best)
    return _canonical(level, area, x0, y0, x1, y1, seed, par)


MUTANTS = ("conn8", "s_strict", "delta_off", "strict_parent", "strict_child", "area_first", "stable_ancestor", "no_bright")


def select(tr, polarity, delta=5, min_area=60, max_area=14400, max_variation=0.25, min_diversity=0.2, mutant=None):
    """The rules in the order of the definition -> regions of one polarity in (level, seed) order."""
    L, A, P = tr["level"], tr["area"], tr["parent"]
    n = len(L)
    if mutant == "delta_off":
        delta = delta + 1
    S = np.zeros(n, dtype=np.int64)
    for i in range(n):
        a = i
        while P[a] >= 0 and (L[P[a]] < L[i] + delta if mutant == "s_strict" else L[P[a]] <= L[i] + delta):
            a = P[a]
        S[i] = A[a]
    num = [int(S[i] - A[i]) for i in range(n)]
    den = [int(A[i]) for i in range(n)]
    considered = [True] * n
    if mutant == "area_first":
        considered = [min_area <= den[i] <= max_area for i in range(n)]
    stable = [True] * n
    for c in range(n):
        p = int(P[c])
        if p < 0 or not (considered[c] and considered[p]):
            continue
        vc, vp = num[c] * den[p], num[p] * den[c]        # var(c) ? var(p), cross-multiplied
        if vc > vp or (mutant == "strict_parent" and vc == vp):
            stable[c] = False
        if vp > vc or (mutant == "strict_child" and vc == vp):
            stable[p] = False
    passed = [stable[i] and considered[i] and min_area <= den[i] <= max_area
              and float(num[i]) < np.float64(max_variation) * np.float64(den[i]) for i in range(n)]
    anchor = stable if mutant == "stable_ancestor" else passed
    out = []
    for i in range(n):
        if not passed[i]:
            continue
        a = int(P[i])
        while a >= 0 and not anchor[a]:
            a = int(P[a])
        if a >= 0 and float(den[a] - den[i]) < np.float64(min_diversity) * np.float64(den[a]):
            continue
        out.append((polarity, int(L[i]), den[i], int(tr["x0"][i]), int(tr["y0"][i]), int(tr["x1"][i]), int(tr["y1"][i]),
                    int(tr["seed"][i]), int(S[i])))
    return out


def regions(g, polarity_mask=3, mutant=None, tree_fn=None, **params):
    """Dark (bit 0) then bright (bit 1) regions of the gray plane g."""
    g = np.asarray(g, dtype=np.uint8)
    build = tree_fn or (lambda a: tree(a, conn8=(mutant == "conn8")))
    out = []
    if polarity_mask & 1:
        out += select(build(g), 0, mutant=mutant, **params)
    if polarity_mask & 2 and mutant != "no_bright":
        out += select(build(255 - g), 1, mutant=mutant, **params)
    return out


def text_boxes(regs, W):
    out = []
    for r in regs:
        x, y, w, h = r[3], r[4], r[5] - r[3] + 1, r[6] - r[4] + 1
        if w > 20 and h > 10 and w < W * 0.5:
            out.append((x, y, w, h))
    return out


def trees_equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in TREE_FIELDS)


# ---- constructed images ---------------------------------------------------------------------------------------------------
def text_fixture():
    from scipy.ndimage import gaussian_filter
    img = 200.0 + 0.1 * np.arange(200, dtype=np.float64)[None, :] * np.ones((96, 1))
    for i in range(5):
        img[40:56, 12 + 36 * i:12 + 36 * i + 26] = 40.0
    img = gaussian_filter(img, 1.0) + np.random.default_rng(7).integers(-3, 4, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


TEXT_BARS = [(12 + 36 * i, 40, 26, 16) for i in range(5)]            # x, y, w, h


def nested_flat():
    g = np.full((80, 160), 230, np.uint8)
    g[10:70, 10:150] = 180
    for i in range(4):
        g[28:52, 22 + 32 * i:22 + 32 * i + 16] = 20
    return g


def corridor(n=65):
    """A 1-pixel corridor of 10 winding (boustrophedon) through an n x n field of 200."""
    g = np.full((n, n), 200, np.uint8)
    for k, y in enumerate(range(1, n - 1, 2)):
        g[y, 1:n - 1] = 10
        if y + 2 < n - 1:
            g[y + 1, n - 2 if k % 2 == 0 else 1] = 10
    return g


def spirals(n=41):
    """Two interleaved Archimedean spirals (values 30 and 60, pitch 4) on a field of 250: they join only at the last
    level."""
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    c = (n - 1) / 2.0
    r = np.hypot(yy - c, xx - c)
    turn = (np.arctan2(yy - c, xx - c) + np.pi) / (2 * np.pi)
    arm = np.floor(r - 4.0 * turn).astype(np.int64) % 4
    g = np.full((n, n), 250, np.uint8)
    g[arm == 0] = 30
    g[arm == 2] = 60
    return g


def checkerboard(h=33, w=31):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def ramp():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def noise(h=64, w=64, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w)).astype(np.uint8)


def noise3(h=127, w=129, seed=4):
    return (np.random.default_rng(seed).integers(0, 3, size=(h, w)) * 50).astype(np.uint8)


def steps(outer=10):
    """Nested flat squares of 0, 5 and `outer`: with delta 5 the ancestor at exactly level + delta decides S."""
    g = np.full((24, 24), outer, np.uint8)
    g[4:20, 4:20] = 5
    g[8:16, 8:16] = 0
    return g


def mutant_inputs():
    """mutant -> (name of the input that catches it, gray image, parameters)."""
    c = gpu_cases()
    small = dict(min_area=1)
    return {
        "conn8": ("diagonal", np.array([[0, 255], [255, 0]], np.uint8), small),
        "s_strict": ("steps", steps(10), small),
        "delta_off": ("steps6", steps(11), small),
        "strict_parent": ("nested",) + c["nested"],
        "strict_child": ("nested",) + c["nested"],
        "area_first": ("text",) + c["text"],
        "stable_ancestor": ("noise",) + c["noise"],
        "no_bright": ("nested",) + c["nested"],
    }


def baseline_source(h=720, w=1080):
    """The synthetic source of the BASELINE workload: a smooth field plus integer noise, RGB u8."""
    rng = np.random.default_rng(20260313)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 64 * np.sin(xx / 37.0 + 0.7 * c) + 48 * np.cos(yy / 23.0 + 1.3 * c) for c in range(3)], axis=-1)
    return np.clip(img + rng.integers(-12, 13, size=img.shape), 0, 255).astype(np.uint8)


def node_table(tr):
    """A tree of this module as the nine columns of sr_mser_node."""
    par = tr["parent"]
    pl = np.where(par >= 0, tr["level"][np.maximum(par, 0)], -1)
    ps = np.where(par >= 0, tr["seed"][np.maximum(par, 0)], -1)
    return np.stack([tr[k] for k in TREE_FIELDS[:7]] + [pl, ps], axis=1).astype(np.int64)


def gpu_cases():
    """name -> (gray image, parameters) of the shapes the GPU test compares; the host test holds the C restatement to the
    Python one on the same list."""
    small = dict(min_area=1)
    return {
        "1x1": (np.array([[7]], np.uint8), small),
        "1x7": (np.array([[3, 3, 9, 1, 1, 200, 9]], np.uint8), small),
        "7x1": (np.array([[3, 3, 9, 1, 1, 200, 9]], np.uint8).T.copy(), small),
        "2x2_equal": (np.full((2, 2), 5, np.uint8), small),
        "2x2_distinct": (np.array([[4, 90], [200, 13]], np.uint8), small),
        "flat64": (np.full((64, 64), 128, np.uint8), {}),
        "checkerboard": (checkerboard(), small),
        "ramp": (ramp(), small),
        "corridor": (corridor(), {}),
        "spirals": (spirals(), small),
        "noise": (noise(), small),
        "noise3": (noise3(), {}),
        "text": (text_fixture(), {}),
        "nested": (nested_flat(), {}),
    }
