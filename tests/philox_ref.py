"""numpy restatement of thunder_amd/csrc/common.h's Philox stream, for the
tests that pin what a kernel draws (the resampling shuffle, the noise
background of the image mask).  A plain module: import it from a test."""
import numpy as np

MASK_STREAM = 0x6D61736B          # counter word c of k_img_mask_scale's stream


def _philox_4x32_10(seed, a, b, c, d):
    """Philox-4x32-10 as thunder_amd/csrc/common.h's Philox::next() draws it:
    counter (a, b, c, d), key = the 64-bit seed's halves; numpy uint64
    arithmetic on arrays of counters."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    m32 = np.uint64(0xFFFFFFFF)
    x = [np.asarray(v, np.uint64) & m32 for v in (a, b, c, d)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * x[0], M1 * x[2]
        x = [((p1 >> np.uint64(32)) ^ x[1] ^ np.uint64(k0)) & m32, p1 & m32,
             ((p0 >> np.uint64(32)) ^ x[3] ^ np.uint64(k1)) & m32, p0 & m32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return x


def uniform(seed, a, b, c, w):
    """Philox::uniform() of draw w (the counter's fourth word) of the stream
    (a, b, c): m = (x << 21) ^ y, 53 bits, (m + 0.5) / 2^53, in (0, 1)."""
    x = _philox_4x32_10(seed, a, b, c, w)
    m = ((x[0] << np.uint64(21)) ^ x[1]) & np.uint64((1 << 53) - 1)
    return (m.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def gauss(seed, a, b, c):
    """Philox::gauss2().x of a fresh stream (a, b, c): Box-Muller's cosine
    branch of the draws w = 0 and w = 1."""
    u1, u2 = uniform(seed, a, b, c, 0), uniform(seed, a, b, c, 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def gauss2(seed, a, b, c, w=0):
    """Philox::gauss2() of the draws w and w + 1 of the stream (a, b, c): both
    branches of Box-Muller, (r cos, r sin) with r = sqrt(-2 ln u_w) and the
    angle 2 pi u_{w+1}."""
    w = np.asarray(w, np.uint64)
    u1, u2 = uniform(seed, a, b, c, w), uniform(seed, a, b, c, w + np.uint64(1))
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def word0(seed, a, b, c, w):
    """Philox::next().x of draw w of the stream (a, b, c): the raw first word
    (the integer draws of the shuffles: (x (i + 1)) >> 32)."""
    return _philox_4x32_10(seed, a, b, c, w)[0]


def mask_draws(seed, n_img, N):
    """The standard normals k_img_mask_scale draws for a stack [n_img, N, N]:
    pixel q (flat over the whole stack, corner-origin layout) owns the stream
    (q >> 32, q & 0xffffffff, MASK_STREAM)."""
    q = np.arange(n_img * N * N, dtype=np.uint64)
    g = gauss(seed, q >> np.uint64(32), q & np.uint64(0xFFFFFFFF), MASK_STREAM)
    return g.reshape(n_img, N, N)
