"""NumPy float64 restatement of FSIM / FSIMc, written from the definition in include/sr_hip.h (the authors' FeatureSIM.m with
Kovesi's phasecong2; parity with MATLAB is unpinned).  It uses numpy.fft throughout, real(ifft2(filter)) for S2 and Sij
included, so the Parseval shortcut of the host unit is checked against the long form.

`mut` names one deliberate mistake (the mutants of tests/test_fsim_host.py): 'grid_swap' (the odd and even grid rules swapped),
'lower_median' (the lower middle value in place of the mean of the middle two), 'window_if' (a pooling window that starts at
i F), 'abs_pow' (|z|^0.03 in place of the real part of the complex power), 'no_17' (T without the division by 1.7)."""
import numpy as np

SCALES, ORIENTS = 4, 4
EPSILON, K = 1e-4, 2.0
T1, T2, T34, LAMBDA = 0.85, 160.0, 200.0, 0.03


def auto_f(h, w):
    return max(1, int(np.floor(min(h, w) / 256 + 0.5)))


def planes_int(img):
    """Y 1000, I 1000, Q 1000 as int64 planes; a gray image has Y 1000 = 1000 v and I = Q = 0 (S_i = S_q = 1)."""
    img = np.asarray(img)
    if img.ndim == 2 or img.shape[2] == 1:
        v = img.reshape(img.shape[0], img.shape[1]).astype(np.int64)
        return 1000 * v, np.zeros_like(v), np.zeros_like(v)
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return 299 * r + 587 * g + 114 * b, 596 * r - 274 * g - 322 * b, 211 * r - 523 * g + 312 * b


def pool_int(plane, F, mut=None):
    """The int64 window sums: window i of an axis covers i F + floor(F / 2) - F + 1 .. i F + floor(F / 2), zero outside."""
    h, w = plane.shape
    rows, cols = -(-h // F), -(-w // F)
    first = 0 if mut == "window_if" else F // 2 - F + 1
    pad = np.zeros((h + 2 * F, w + 2 * F), np.int64)
    pad[F:F + h, F:F + w] = plane
    out = np.zeros((rows, cols), np.int64)
    for dy in range(F):
        for dx in range(F):
            ys, xs = F + first + dy, F + first + dx
            out += pad[ys:ys + rows * F:F, xs:xs + cols * F:F][:rows, :cols]
    return out


def pooled_int(img, F, mut=None):
    return np.stack([pool_int(p, F, mut) for p in planes_int(img)])


def _axis(n, mut=None):
    odd = bool(n & 1)
    if mut == "grid_swap":
        odd = not odd
    if odd:
        return (np.arange(n) - (n - 1) / 2) / (n - 1)
    return (np.arange(n) - n // 2) / n


def filters(rows, cols, mut=None):
    """(logGabor[4], spread[4]), DC first."""
    x, y = np.meshgrid(_axis(cols, mut), _axis(rows, mut))
    r0 = np.fft.ifftshift(np.sqrt(x * x + y * y))
    theta = np.fft.ifftshift(np.arctan2(-y, x))
    radius = r0.copy()
    radius[0, 0] = 1.0
    lp = 1.0 / (1.0 + (r0 / 0.45) ** 30)
    lg = []
    for s in range(SCALES):
        fo = 1.0 / (6.0 * 2 ** s)
        g = np.exp(-(np.log(radius / fo)) ** 2 / (2.0 * np.log(0.55) ** 2)) * lp
        g[0, 0] = 0.0
        lg.append(g)
    st, ct = np.sin(theta), np.cos(theta)
    theta_sigma = np.pi / 4 / 1.2
    sp = []
    for o in range(ORIENTS):
        angl = o * np.pi / 4
        ds = st * np.cos(angl) - ct * np.sin(angl)
        dc = ct * np.cos(angl) + st * np.sin(angl)
        dt = np.abs(np.arctan2(ds, dc))
        sp.append(np.exp(-(dt * dt) / (2.0 * theta_sigma ** 2)))
    return np.stack(lg), np.stack(sp)


def noise_sums(lg, sp):
    """EM_n, S2, Sij of the four orientations, the long way: through real(ifft2(filter))."""
    rows, cols = lg.shape[1:]
    em, s2, sij = np.zeros(ORIENTS), np.zeros(ORIENTS), np.zeros(ORIENTS)
    for o in range(ORIENTS):
        em[o] = np.sum((lg[0] * sp[o]) ** 2)
        a = [np.real(np.fft.ifft2(lg[s] * sp[o])) * np.sqrt(rows * cols) for s in range(SCALES)]
        s2[o] = sum(np.sum(a[s] ** 2) for s in range(SCALES))
        sij[o] = sum(np.sum(a[s] * a[t]) for s in range(SCALES) for t in range(s + 1, SCALES))
    return em, s2, sij


def _median(v, mut=None):
    v = np.sort(np.asarray(v).ravel())
    n = v.size
    if mut == "lower_median":
        return v[(n - 1) // 2]
    return (v[(n - 1) // 2] + v[n // 2]) / 2.0


def phasecong(Y, mut=None):
    """-> {'pc', 'an_all', 'median': [4], 'T': [4]} of one float64 plane."""
    Y = np.asarray(Y, np.float64)
    rows, cols = Y.shape
    lg, sp = filters(rows, cols, mut)
    em, s2, sij = noise_sums(lg, sp)
    X = np.fft.fft2(Y)
    energy_all, an_all = np.zeros_like(Y), np.zeros_like(Y)
    med, thr = np.zeros(ORIENTS), np.zeros(ORIENTS)
    for o in range(ORIENTS):
        eo = [np.fft.ifft2(X * (lg[s] * sp[o])) for s in range(SCALES)]
        sum_e = sum_o = sum_an = 0.0
        for s in range(SCALES):
            sum_an = sum_an + np.abs(eo[s])
            sum_e = sum_e + eo[s].real
            sum_o = sum_o + eo[s].imag
        xen = np.sqrt(sum_e ** 2 + sum_o ** 2) + EPSILON
        me, mo = sum_e / xen, sum_o / xen
        energy = 0.0
        for s in range(SCALES):
            e, od = eo[s].real, eo[s].imag
            energy = energy + e * me + od * mo - np.abs(e * mo - od * me)
        med[o] = _median(np.abs(eo[0]) ** 2, mut)
        noise = (-med[o] / np.log(0.5)) / em[o]
        tau = np.sqrt((2.0 * noise * s2[o] + 4.0 * noise * sij[o]) / 2.0)
        thr[o] = tau * np.sqrt(np.pi / 2) + K * np.sqrt((2 - np.pi / 2) * tau ** 2)
        if mut != "no_17":
            thr[o] = thr[o] / 1.7
        energy_all = energy_all + np.maximum(energy - thr[o], 0.0)
        an_all = an_all + sum_an
    with np.errstate(invalid="ignore", divide="ignore"):
        pc = energy_all / an_all
    return {"pc": pc, "an_all": an_all, "median": med, "T": thr}


def _conv_same(Y, k):
    """conv2(Y, k, 'same') with a zero border, k 3 x 3."""
    h, w = Y.shape
    pad = np.zeros((h + 2, w + 2), Y.dtype)
    pad[1:-1, 1:-1] = Y
    out = np.zeros_like(Y)
    for a in range(3):
        for b in range(3):
            out = out + k[a, b] * pad[2 - a:2 - a + h, 2 - b:2 - b + w]
    return out


def gradient(Y):
    dx = np.array([[3.0, 0.0, -3.0], [10.0, 0.0, -10.0], [3.0, 0.0, -3.0]]) / 16.0
    ix, iy = _conv_same(Y, dx), _conv_same(Y, dx.T)
    return np.sqrt(ix ** 2 + iy ** 2)


def _sim(u, v, k):
    return (2.0 * u * v + k) / (u ** 2 + v ** 2 + k)


def fsim(img1, img2, F=None, mut=None):
    """-> {'fsim', 'fsimc', 'sum_s', 'sum_sc', 'sum_pcm', 'F', 'size', 'an_all_min', 'min_siq'}."""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    assert img1.shape == img2.shape
    h, w = img1.shape[:2]
    F = auto_f(h, w) if F is None else F
    unit = 1000.0 * F * F
    p1, p2 = pooled_int(img1, F, mut) / unit, pooled_int(img2, F, mut) / unit
    c1, c2 = phasecong(p1[0], mut), phasecong(p2[0], mut)
    pc1, pc2 = c1["pc"], c2["pc"]
    g1, g2 = gradient(p1[0]), gradient(p2[0])
    with np.errstate(invalid="ignore"):
        pcm = np.where(np.isnan(pc1) | np.isnan(pc2), np.nan, np.maximum(pc1, pc2))
        s = _sim(g1, g2, T2) * _sim(pc1, pc2, T1)
        z = _sim(p1[1], p2[1], T34) * _sim(p1[2], p2[2], T34)
        wgt = np.abs(z) ** LAMBDA if mut == "abs_pow" else np.real(z.astype(np.complex128) ** LAMBDA)
        sum_s, sum_sc, sum_pcm = np.sum(s * pcm), np.sum(s * wgt * pcm), np.sum(pcm)
        val, valc = (sum_s / sum_pcm, sum_sc / sum_pcm) if sum_pcm != 0 else (np.nan, np.nan)
    return {"fsim": float(val), "fsimc": float(valc), "sum_s": float(sum_s), "sum_sc": float(sum_sc), "sum_pcm": float(sum_pcm),
            "F": F, "size": p1[0].shape, "an_all_min": float(min(c1["an_all"].min(), c2["an_all"].min())),
            "min_siq": float(z.min())}


# ---- inputs the tests share ----------------------------------------------------------------------------------------------------
def structured(h, w, cn, seed):
    """A seeded image with structure at several scales (ramps, waves, blocks, a little noise), u8, h x w (x cn)."""
    rnd = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(cn):
        fx, fy, ph = rnd.uniform(0.05, 0.6), rnd.uniform(0.05, 0.6), rnd.uniform(0, 6.28)
        v = 110 + 50 * np.sin(fx * x + ph) * np.cos(fy * y) + 40 * ((x // 7 + y // 5 + c) % 2) + 0.15 * (x - y)
        v += 25 * np.sin(0.011 * x * y / max(h, w) * 8 + c) + rnd.uniform(-6, 6, (h, w))
        planes.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
    return planes[0] if cn == 1 else np.stack(planes, axis=-1)


def distorted(img, seed, amp=20, patch=True):
    """The image plus uniform integer noise in [-amp, amp], plus one flat patch."""
    rnd = np.random.default_rng(seed + 1000)
    out = np.clip(img.astype(np.int64) + rnd.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)
    if patch:
        h, w = img.shape[:2]
        out[h // 4:h // 4 + max(h // 5, 3), w // 3:w // 3 + max(w // 4, 3)] = 97
    return out


def case(h, w, cn):
    """The pair of a shape that the GPU test and the mutants of the host test share: a structured image and its distorted copy."""
    a = structured(h, w, cn, 31 * h + w + cn)
    return a, distorted(a, 31 * h + w + cn)
