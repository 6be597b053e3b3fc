"""The seeded MIND noise of include/dgtta.h restated in numpy (test infrastructure): Philox4x32-10 as published with
Random123 (Salmon et al., SC'11) and Box-Muller on 23-bit uniforms, evaluated in float64 (or any numpy float type).

    (x0,x1,x2,x3) = Philox4x32-10(counter = (v, 4*b + c/4, offset_lo, offset_hi), key = (seed_lo, seed_hi))
    u_i = ((x_i >> 9) + 0.5) * 2^-23
    c%4 == 0: sqrt(-2 ln u0) cos(2 pi u1)   1: sqrt(-2 ln u0) sin(2 pi u1)   2, 3: the same from (u2, u3)
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or ints) and two key words -> four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)])
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _LOW, p1 >> _32, p1 & _LOW
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normals(words, dtype=np.float64):
    """Four word arrays -> the four normals of a channel group, every operation in `dtype`."""
    t = np.dtype(dtype).type
    u = [((x >> np.uint64(9)).astype(dtype) + t(0.5)) * t(2.0 ** -23) for x in words]
    out = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        r, ang = np.sqrt(t(-2) * np.log(a)), t(2 * np.pi) * b
        out += [r * np.cos(ang), r * np.sin(ang)]
    return out


def mind_noise(seed, offset, b0, B, D, H, W, dtype=np.float64):
    """[B,12,D,H,W]: the field dgtta_mind3d_noise_fill writes for samples b0 .. b0+B-1."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    V = D * H * W
    vox = np.arange(V, dtype=np.uint64)
    out = np.empty((B, 12, V), dtype=dtype)
    for b in range(B):
        for g in range(3):
            words = philox4x32_10(vox, (b0 + b) * 4 + g, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
            out[b, 4 * g:4 * g + 4] = normals(words, dtype)
    return out.reshape(B, 12, D, H, W)
