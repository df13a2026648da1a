"""numpy reference of the counter-based dropout mask (csrc/dropout.hip), written from the
definition: Philox4x32-10 of Salmon et al. ("Parallel random numbers: as easy as 1, 2, 3", SC'11),
multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two -> four uint64 arrays holding uint32 words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for r in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)      # 32 x 32 -> 64 bits: no overflow
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def threshold(p):
    """T = (uint32)((double)p * 2^32), p the FLOAT rate."""
    return int(float(np.float32(p)) * 4294967296.0)


def scale(p):
    """s = (float)(1 / (1 - (double)p))."""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_mask(n, p, seed, subseq, step, site):
    """uint8 [n]: 1 where element i is kept.  Block j = i // 4 has counter (j, subseq, site, step)
    and key (seed & 0xffffffff, seed >> 32); element 4j + k reads output word k."""
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((j, subseq, site, step), (seed & MASK, (seed >> 32) & MASK))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    return (w >= np.uint64(threshold(p))).astype(np.uint8)
