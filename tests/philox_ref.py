"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) and the engine's 53-bit uniform mapping, restated in NumPy for the
tests of the multi-trajectory imputation (include/mpstime_hip.h: mpst_impute_traj).  Vectorised over the counters."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SITE_BITS = 20


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (2,) or (..., 2) of 32-bit words -> (..., 4) uint64 holding 32-bit words."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k0, k1 = (np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1)


def uniforms(seed, row_id, K, T, trials):
    """u[n, k, j, t] of the device generator: key = the seed's two words, counter = (row id low, row id high, k, j | t << 20),
    value = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53."""
    seed = int(seed) & (2 ** 64 - 1)
    rid = np.asarray(row_id, dtype=np.int64).astype(np.uint64)
    n, k, j, t = np.meshgrid(rid, np.arange(K, dtype=np.uint64), np.arange(T, dtype=np.uint64), np.arange(trials, dtype=np.uint64),
                             indexing="ij")
    ctr = np.stack([n & MASK, n >> np.uint64(32), k, j | (t << np.uint64(SITE_BITS))], axis=-1)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    hi, lo = w[..., 0] >> np.uint64(5), w[..., 1] >> np.uint64(6)
    return ((hi << np.uint64(26)) | lo).astype(np.float64) / 9007199254740992.0
