"""numpy restatement of ``fs2hip_cepstra`` (include/fs2hip.h) and of the table ``hip.dct_table`` builds: what the CPU and
GPU tests of the cepstral distance compare against."""
import math

import numpy as np


def table64(channels, K):
    """[K, C] float64: rows 1 .. K of the orthonormal DCT-II of length C, ``sqrt(2 / C) * cos(pi * (k + 1) * (m + 0.5) / C)``,
    every element by the host's libm in the order the formula is written."""
    scale = math.sqrt(2.0 / channels)
    return np.array([[scale * math.cos(math.pi * (k + 1) * (m + 0.5) / channels) for m in range(channels)] for k in range(K)],
                    dtype=np.float64)


def table(channels, K):
    """The table the kernel is given: float64 rounded to fp32 once."""
    return table64(channels, K).astype(np.float32)


def cepstra32(x, tab):
    """out[..., k] = (((0 + x[0] * tab[k][0]) + x[1] * tab[k][1]) + ...): an explicit loop over m on fp32 arrays, every
    product and every sum rounded to fp32 (numpy never contracts them), m ascending from 0.f."""
    x, tab = np.asarray(x, dtype=np.float32), np.asarray(tab, dtype=np.float32)
    acc = np.zeros(x.shape[:-1] + (tab.shape[0],), dtype=np.float32)
    for m in range(x.shape[-1]):
        acc = acc + x[..., m, None] * tab[:, m]
    assert acc.dtype == np.float32
    return acc


def cepstra64(x, tab):
    """The same product in float64 (of the fp32 inputs and the fp32 table)."""
    return np.asarray(x, dtype=np.float64) @ np.asarray(tab, dtype=np.float64).T


def abs_product64(x, tab):
    """sum_m |x_m * tab[k][m]| in float64: what the recursive-summation bound multiplies."""
    return np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(tab, dtype=np.float64)).T


def mel_like(rows, channels, seed):
    """[rows, C] fp32 with the scale of log-mel frames: a level per row plus a tilt over the bins plus noise."""
    g = np.random.default_rng(seed)
    level = g.normal(-4.0, 1.5, size=(rows, 1))
    tilt = np.linspace(1.0, -1.0, channels)[None] * g.normal(1.0, 0.5, size=(rows, 1))
    return (level + tilt + g.normal(0.0, 1.0, size=(rows, channels))).astype(np.float32)
