"""An independent float64 restatement of the ensemble member generator for tests/test_perturb_cpu.py and
tests/test_gpu_perturb.py.  It shares no code with dlwp_amd/model/ensemble.py: its own Philox-4x32-10 (checked against Random123's
known answers by the CPU test), the Box-Muller pair in float64, float64 taps that are only rounded to float32 at the end (as the
definition says), and the smoothing as the brute-force 2-D double sum with np.roll over a field of virtual rows -- no separable
passes, no float32 accumulator."""
import math

import numpy as np

MASK = (1 << 32) - 1


def philox(c, k):
    """Philox-4x32-10 on Python integers: c four 32-bit words, k two -> four words"""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        a, b = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (b >> 32) ^ c1 ^ k0, b & MASK, (a >> 32) ^ c3 ^ k1, a & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def philox_np(c0, c1, c2, c3, k0, k1):
    """the same rounds on uint64 arrays (c0 an array, the rest integers)"""
    m = np.uint64(MASK)
    c0 = np.asarray(c0, np.uint64)
    c1, c2, c3 = (np.full(c0.shape, v, np.uint64) for v in (c1, c2, c3))
    for _ in range(10):
        a, b = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (b >> np.uint64(32)) ^ c1 ^ np.uint64(k0), b & m, (a >> np.uint64(32)) ^ c3 ^ np.uint64(k1), a & m
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def white64(seed, d, s, k, rows, width):
    """float64 z of the virtual rows `rows`: (len(rows), width)"""
    seed &= (1 << 64) - 1
    quads = (width + 3) // 4
    out = np.empty((len(rows), 4 * quads))
    for n, i in enumerate(rows):
        w = philox_np(np.arange(quads), (int(i) + 32768) + 65536 * k, d, s, seed & MASK, seed >> 32)
        for e in (0, 1):
            u1 = (2.0 * (w[2 * e] >> np.uint64(9)).astype(np.float64) + 1.0) / 16777216.0
            u2 = (w[2 * e + 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
            r = np.sqrt(-2.0 * np.log(u1))
            out[n, 2 * e::4] = r * np.cos(2.0 * math.pi * u2)
            out[n, 2 * e + 1::4] = r * np.sin(2.0 * math.pi * u2)
    return out[:, :width]


def taps64(length):
    """float64 values of the float32 taps: (R, g)"""
    radius = int(math.ceil(3.0 * length))
    a = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-a * a / (2.0 * length * length)) if radius else np.ones(1)
    return radius, (g / math.sqrt((g * g).sum())).astype(np.float32).astype(np.float64)


def zeta64(seed, d, s, k, height, width, ly, lx):
    """the brute-force double sum over a field of virtual rows: float64 (height, width)"""
    (ry, gy), (rx, gx) = taps64(ly), taps64(lx)
    z = white64(seed, d, s, k, range(-ry, height + ry), width)
    acc = np.zeros_like(z)
    for a in range(-ry, ry + 1):
        for b in range(-rx, rx + 1):
            # acc[i, j] += g_a g_b z[i + a, (j + b) mod W]; the rows that roll around are outside [ry, ry + height)
            acc += gy[a + ry] * gx[b + rx] * np.roll(np.roll(z, -a, axis=0), -b, axis=1)
    return acc[ry:ry + height]


def draw_of(g, control, antithetic):
    if control:
        if g == 0:
            return None
        g -= 1
    return (g >> 1, -1.0 if g & 1 else 1.0) if antithetic else (g, 1.0)


def perturbation64(dims, members, sigma, length, seed, control=True, antithetic=False, first_member=0):
    """p = sign sigma zeta in float64, (S, M, K, H, W); the control member's is 0"""
    s_n, k_n, h_n, w_n = dims
    ly, lx = length if isinstance(length, tuple) else (length, length)
    sigma = np.broadcast_to(np.asarray(sigma, np.float32).astype(np.float64), (k_n,))
    out = np.zeros((s_n, members, k_n, h_n, w_n))
    memo = {}
    for m in range(members):
        ds = draw_of(first_member + m, control, antithetic)
        if ds is None:
            continue
        for s in range(s_n):
            for k in range(k_n):
                if (ds[0], s, k) not in memo:
                    memo[(ds[0], s, k)] = zeta64(seed, ds[0], s, k, h_n, w_n, ly, lx)
                out[s, m, k] = ds[1] * sigma[k] * memo[(ds[0], s, k)]
    return out


def smoothing_bound(length_y, length_x):
    """float32 accumulation against the float64 double sum, per unit of max|z| <= sqrt(48 ln 2): each of the two passes adds n = 2R + 1
    rounded products into a rounded accumulator, (2 n) roundings of 2^-24 on partial sums bounded by sum |g| max|z|; the rounding of z
    itself to float32 is one more.  bound = 2^-24 (2 n_x + 2 n_y + 1) sum|g_y| sum|g_x| sqrt(48 ln 2)."""
    (ry, gy), (rx, gx) = taps64(length_y), taps64(length_x)
    return 2.0 ** -24 * (2 * (2 * rx + 1) + 2 * (2 * ry + 1) + 1) * np.abs(gy).sum() * np.abs(gx).sum() * math.sqrt(48.0 * math.log(2.0))
