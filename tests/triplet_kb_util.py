"""numpy restatement of the attention-dropout keep pattern of the triplet kernels for every N (csrc/triplet_common.hpp):
the hash word of element (i, k) inside a unit is (i*64 + k) >> 1 for N <= 64 -- exactly golden_util.triplet_dropout_keep --
and (i*128 + k) >> 1 for N > 64, where the stride of 64 would alias (i, k >= 64) with (i+1, k-64)."""
import numpy as np

import golden_util as gu


def row_stride(N):
    return 64 if N <= 64 else 128


def dropout_field_index(N):
    """(N, N) index of the 16-bit field element (i, k) of a unit draws its keep decision from: 2*word + (k & 1)"""
    i = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(N, dtype=np.int64)[None, :]
    return ((i * row_stride(N) + k) >> 1) * 2 + (k & 1)


def triplet_dropout_keep(seed, p, units, N):
    """keep[u, i, k] (bool) and the scale 1/(1-p); unit = ((b*2 + dir)*H + h)*N + j"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    thresh = int(min(65535, max(1, np.rint(np.float32(p) * np.float32(65536.0)))))
    units = np.asarray(units, dtype=np.uint64)
    base = (gu._mix32(np.uint64(lo) ^ gu._mix32(units)) + np.uint64(hi)) & 0xFFFFFFFF
    field = dropout_field_index(N).astype(np.uint64)
    odd = (field & 1).astype(bool)
    word = field >> 1
    keep = np.empty((len(units), N, N), dtype=bool)
    for u0 in range(0, len(units), 64):                  # in chunks: (U, N, N) uint64 temporaries are large at N = 128
        r = gu._mix32((base[u0:u0 + 64, None, None] + word[None] * 0x9e3779b9) & 0xFFFFFFFF)
        keep[u0:u0 + 64] = np.where(odd[None], r >> 16, r & 0xFFFF) >= thresh
    return keep, 1.0 / (1.0 - float(np.float32(p)))
