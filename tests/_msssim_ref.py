"""NumPy float64 restatement of the multi-scale SSIM defined in include/sr_hip.h (sr_ms_ssim_u8), and the inputs the tests use.

Planes: level j + 1 is the 2 x 2 mean of level j, a last odd row or column dropped.  The pooling is exact: `pool_sums` keeps the
integer sums of 4^j u8 values, `planes` divides them by 4^j (a power of two: exact in float64).  Terms: explicit 11 taps
(sigma 1.5), valid convolution (axis 0, then axis 1), population covariance, l and cs per sample, S_j = mean(l cs),
CS_j = mean(cs).  Value: prod_{j < L-1} max(CS_j, 0)^w_j * max(S_{L-1}, 0)^w_{L-1}."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003
MAX_LEVELS = 5
WIN = 11


def taps():
    x = np.arange(-5, 6)
    phi = np.exp(-0.5 / (1.5 * 1.5) * x ** 2)
    return phi / phi.sum()


def gray_u8(img, shift=15):
    """cv2.cvtColor(RGB2GRAY) on u8 in fixed point (15 or 14 fractional bits); a 2-D image is gray already."""
    if img.ndim == 2:
        return img
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    if shift == 15:
        return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15).astype(np.uint8)
    return ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)


def plan(h, w, levels):
    """-> (sizes [(h_j, w_j)], counts [(h_j - 10)(w_j - 10)]); ValueError like sr_ms_ssim_plan."""
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("levels must be 1 .. 5")
    if min(h, w) < WIN << (levels - 1):
        raise ValueError(f"both sides must be at least {WIN << (levels - 1)}")
    sizes = [(h >> j, w >> j) for j in range(levels)]
    return sizes, [(a - 10) * (b - 10) for a, b in sizes]


def pool_sums(g, levels):
    """-> [s_0 .. s_{L-1}], s_j the exact integer sums (int64) of the 4^j level-0 values under each level-j pixel."""
    out = [g.astype(np.int64)]
    for _ in range(1, levels):
        s = out[-1]
        h2, w2 = s.shape[0] // 2, s.shape[1] // 2
        s = s[:2 * h2, :2 * w2]
        out.append(s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2])
    return out


def planes(g, levels):
    """The level planes in float64: sums / 4^j, exact."""
    return [s.astype(np.float64) / float(4 ** j) for j, s in enumerate(pool_sums(g, levels))]


def _valid(p, k):
    # the order of scipy.ndimage's symmetric correlate1d (centre tap, then the pairs from the outermost inwards), so that level 0
    # reproduces scikit-image to the last bit
    h, w = p.shape
    mh, mw = h - 10, w - 10
    tmp = p[5:5 + mh] * k[5]
    for j in range(5, 0, -1):
        tmp = tmp + (p[5 - j:5 - j + mh] + p[5 + j:5 + j + mh]) * k[5 - j]
    out = tmp[:, 5:5 + mw] * k[5]
    for j in range(5, 0, -1):
        out = out + (tmp[:, 5 - j:5 - j + mw] + tmp[:, 5 + j:5 + j + mw]) * k[5 - j]
    return out


def level_terms(x, y, data_range=255.0):
    """(S, CS) of two float64 planes: means of l * cs and of cs over the valid map."""
    k = taps()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy = _valid(x, k), _valid(y, k)
    uxx, uyy, uxy = _valid(x * x, k), _valid(y * y, k), _valid(x * y, k)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    a1, a2 = 2 * ux * uy + c1, 2 * vxy + c2
    b1, b2 = ux ** 2 + uy ** 2 + c1, vx + vy + c2
    s_map = (a1 * a2) / (b1 * b2)
    cs_map = a2 / b2
    return float(s_map.mean()), float(cs_map.mean())


def value(s, cs, weights=None):
    wt = WEIGHTS[:len(s)] if weights is None else tuple(weights)
    assert len(wt) == len(s) == len(cs)
    v = 1.0
    for j in range(len(s)):
        m = s[j] if j == len(s) - 1 else cs[j]
        v *= max(m, 0.0) ** wt[j]
    return v


def ms_ssim(a, b, levels=5, weights=None, data_range=255.0, shift=15):
    """-> (value, [S_j], [CS_j]) of two u8 images (2-D gray or RGB)."""
    ga, gb = gray_u8(a, shift), gray_u8(b, shift)
    plan(ga.shape[0], ga.shape[1], levels)
    pa, pb = planes(ga, levels), planes(gb, levels)
    terms = [level_terms(x, y, data_range) for x, y in zip(pa, pb)]
    s, cs = [t[0] for t in terms], [t[1] for t in terms]
    return value(s, cs, weights), s, cs


def base_image(rng, h, w, cn=1):
    """The fixture-style image: uniform noise mixed half and half with a smooth sinusoid field."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = (128 + 60 * np.sin(xx / 11.0) + 40 * np.cos(yy / 7.0))[..., None]
    a = np.clip(0.5 * rng.integers(0, 256, (h, w, cn)) + 0.5 * base, 0, 255).astype(np.uint8)
    return a if cn == 3 else a[..., 0]


def _blocks(rng, h, w, size, amp):
    g = rng.uniform(-amp, amp, (-(-h // size), -(-w // size)))
    return np.kron(g, np.ones((size, size)))[:h, :w]


def img_pair(rng, h, w, cn=1):
    """Inputs that separate the levels: b = clip(0.8 a + B16 + B4 + 6 randn + 20), with B16 / B4 random offsets (+-40 / +-30)
    constant over 16 x 16 / 4 x 4 blocks -- distortion at every scale, so CS_j stays clear of 1 and S_j of CS_j at every
    level (pure noise leaves CS_3, CS_4 at 0.999.., where mixed-up levels or swapped S / CS would pass)."""
    a = base_image(rng, h, w, cn)
    d = (_blocks(rng, h, w, 16, 40.0) + _blocks(rng, h, w, 4, 30.0))
    if cn == 3:
        d = d[..., None]
    b = np.clip(0.8 * a + d + 6.0 * rng.standard_normal(a.shape) + 20.0, 0, 255).astype(np.uint8)
    return a, b
