"""CPU restatement of the Euler-ancestral sampler's noise and step: Philox4x32-10 in numpy (Salmon et al.; checked against the Random123
known-answer vectors), the uniforms and Box-Muller in float64, sigma_up / sigma_down and the step formula."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)

# counter / key -> output, the Random123 known-answer vectors
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> (n, 4) uint32."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def quad_bits(first_quad, n_quads, seed, step, stream):
    """The words of quads first_quad .. first_quad + n_quads - 1 as the kernels key them -> (n_quads, 4) uint32."""
    q = np.uint64(first_quad) + np.arange(n_quads, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((q & MASK32, q >> np.uint64(32), step, stream), (seed & 0xFFFFFFFF, seed >> 32))


def normals_from_bits(bits):
    """(n_quads, 4) uint32 -> (4 * n_quads,) float64: u = ((r >> 9) + 0.5) * 2^-23, Box-Muller on (u0, u1) and (u2, u3)."""
    u = ((bits >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    z = np.empty_like(u)
    for k in (0, 2):
        rad, ang = np.sqrt(-2.0 * np.log(u[:, k])), 2.0 * np.pi * u[:, k + 1]
        z[:, k], z[:, k + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z.reshape(-1)


def normals(n, seed, step, stream):
    return normals_from_bits(quad_bits(0, (n + 3) // 4, seed, step, stream))[:n]


def ancestral_sigmas(sigma_from, sigma_to, eta=1.0):
    """sigma_up = min(sigma_to, eta * sqrt(sigma_to^2 (sigma_from^2 - sigma_to^2) / sigma_from^2)), sigma_down = sqrt(sigma_to^2 - sigma_up^2)."""
    if sigma_to == 0.0:
        return 0.0, 0.0
    up = min(sigma_to, eta * np.sqrt(sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2))
    return float(up), float(np.sqrt(sigma_to ** 2 - up ** 2))


def ancestral_step(x, x0, sigma, sigma_next, noise, eta=1.0):
    """x + ((x - x0) / sigma) * (sigma_down - sigma) + noise * sigma_up, float64 numpy."""
    up, down = ancestral_sigmas(sigma, sigma_next, eta)
    return x + (x - x0) / sigma * (down - sigma) + (noise * up if up > 0 else 0.0)
