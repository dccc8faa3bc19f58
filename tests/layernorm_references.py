"""Plain references of the LayerNorm kernels (``csrc/norm.hip``) and of the stateless dropout mask (``csrc/common.h``).

``ln_fwd64`` / ``ln_bwd64`` are the LayerNorm equations in float64, written out (no ``F.layer_norm``);
``drop_factors`` is the mask's definition -- ``fs2_make_drop``, ``fs2_resolve_drop``, ``fs2_hash32``,
``fs2_drop_factor`` -- written a second time in NumPy fixed-width integers, so that the kernels are tied to a statement
on the host and not only to each other.  ``tests/test_layernorm_reference_cpu.py`` checks all three without a GPU."""
import numpy as np
import torch


def ln_fwd64(x, gamma, beta, eps):
    """x [M, C], gamma/beta [C] -> (y [M, C], mean [M], rstd [M]) in float64 (biased variance, as nn.LayerNorm)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = ((xc * xc).mean(-1) + eps) ** -0.5
    return xc * rstd[:, None] * gamma + beta, mean, rstd


def ln_bwd64(dy, x, gamma, mean, rstd):
    """The backward from SAVED statistics, as the kernel takes them: (dx [M, C], dgamma [C], dbeta [C]) in float64.
    dx = rstd * (g dy - mean_c(g dy) - xhat * mean_c(g dy xhat)), dgamma = sum_rows dy xhat, dbeta = sum_rows dy."""
    dy, x, gamma, mean, rstd = (t.double() for t in (dy, x, gamma, mean, rstd))
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = dy * gamma
    dx = rstd[:, None] * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


_U32, _U64 = np.uint32, np.uint64


def drop_seed(seed, step):
    """fs2_resolve_drop: the splitmix64 finalisation of seed + step * 0xD1B54A32D192ED03 (step None: no counter)."""
    with np.errstate(over="ignore"):
        z = np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=_U64)
        if step is not None:
            z = z + np.array([int(step) & 0xFFFFFFFFFFFFFFFF], dtype=_U64) * _U64(0xD1B54A32D192ED03)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        z = z ^ (z >> _U64(31))
    return int(z[0])


def hash32(seed, idx):
    """fs2_hash32 of a resolved 64-bit seed and a uint64 index array: the two-round multiply-xorshift mixer."""
    idx = np.asarray(idx, dtype=_U64)
    lo, hi = _U32(seed & 0xFFFFFFFF), _U32(seed >> 32)
    with np.errstate(over="ignore"):
        ih = (idx >> _U64(32)).astype(_U32)
        x = idx.astype(_U32) ^ lo ^ ((ih << _U32(13)) | (ih >> _U32(19)))
        x = x ^ (x >> _U32(16))
        x = x * _U32(0x7FEB352D)
        x = x ^ hi
        x = x ^ (x >> _U32(15))
        x = x * _U32(0x846CA68B)
        x = x ^ (x >> _U32(16))
    return x


def drop_factors(p, seed, step, n):
    """The n dropout factors of a (p, seed, step) record as a float32 tensor: 0 where the element is dropped, else
    1/(1-p) computed in fp32.  Element i is dropped iff the 16-bit field of hash32(resolved seed, i >> 1) -- the low half
    for even i, the high half for odd i -- is below the threshold uint32(p * 65536 + 0.5), p being the fp32 value."""
    p32 = np.float32(p)
    if not p32 > 0:  # fs2_make_drop: "on" only for p > 0, every factor is 1
        return torch.ones(n, dtype=torch.float32)
    t = float(p32) * 65536.0 + 0.5
    thresh = _U32(65536) if t >= 65536.0 else _U32(int(t))
    scale = np.float32(1) / (np.float32(1) - p32) if p32 < 1 else np.float32(0)
    idx = np.arange(n, dtype=_U64)
    h = hash32(drop_seed(seed, step), idx >> _U64(1))
    field = np.where((idx & _U64(1)) == 1, h >> _U32(16), h & _U32(0xFFFF))
    return torch.from_numpy(np.where(field < thresh, np.float32(0), scale).astype(np.float32))
