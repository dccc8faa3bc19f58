"""CPU: the references of the LayerNorm kernel tests (``tests/layernorm_references.py``) against ``F.layer_norm`` and its
autograd in float64, and the vectorised NumPy port of the dropout mask against the same rule in plain Python integers
-- so a mismatch on the GPU is the kernel's, not the reference's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import layernorm_references as R

M64 = 0xFFFFFFFFFFFFFFFF
M32 = 0xFFFFFFFF


@pytest.mark.parametrize("M,C", [(1, 4), (7, 252), (33, 516)])
def test_float64_layernorm_is_torchs(M, C):
    g = torch.Generator().manual_seed(M + C)
    x = (3 * torch.randn(M, C, generator=g) + 5).double().requires_grad_(True)
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).double().requires_grad_(True)
    beta = torch.randn(C, generator=g).double().requires_grad_(True)
    dy = torch.randn(M, C, generator=g).double()
    y, mean, rstd = R.ln_fwd64(x.detach().float(), gamma.detach().float(), beta.detach().float(), 1e-5)
    assert y.dtype == mean.dtype == rstd.dtype == torch.float64
    # the references upcast fp32 inputs: feed torch the same values
    xr = x.detach().float().double().requires_grad_(True)
    gr = gamma.detach().float().double().requires_grad_(True)
    br = beta.detach().float().double().requires_grad_(True)
    want = F.layer_norm(xr, (C,), gr, br, 1e-5)
    want.backward(dy)
    assert torch.allclose(y, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(mean, xr.detach().mean(-1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(rstd, (xr.detach().var(-1, unbiased=False) + 1e-5) ** -0.5, rtol=1e-12)
    dx, dgamma, dbeta = R.ln_bwd64(dy, xr.detach(), gr.detach(), mean, rstd)
    assert torch.allclose(dx, xr.grad, rtol=1e-10, atol=1e-11)
    assert torch.allclose(dgamma, gr.grad, rtol=1e-10, atol=1e-11) and torch.allclose(dbeta, br.grad, rtol=1e-12, atol=1e-12)


def _factor_scalar(p, seed, step, i):
    """The rule of csrc/common.h for ONE element, in unbounded Python integers masked by hand."""
    p32 = float(np.float32(p))
    if not p32 > 0:
        return 1.0
    t = p32 * 65536.0 + 0.5
    thresh = 65536 if t >= 65536.0 else int(t)
    z = (seed + (0 if step is None else step * 0xD1B54A32D192ED03)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    idx = i >> 1
    hi = (idx >> 32) & M32
    x = (idx & M32) ^ (z & M32) ^ (((hi << 13) | (hi >> 19)) & M32)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= z >> 32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    field = (x >> 16) if (i & 1) else (x & 0xFFFF)
    return 0.0 if field < thresh else float(np.float32(1) / (np.float32(1) - np.float32(p)))


@pytest.mark.parametrize("p,seed,step", [(0.1, 31337, None), (0.5, (1 << 40) + 12345, 7), (0.3, M64, (1 << 63) + 5),
                                         (0.0, 9, 3)])
def test_vectorised_mask_port_is_the_scalar_rule(p, seed, step):
    n = 1001
    got = R.drop_factors(p, seed, step, n)
    assert got.dtype == torch.float32 and got.shape == (n,)
    want = torch.tensor([_factor_scalar(p, seed, step, i) for i in range(n)], dtype=torch.float64)
    assert torch.equal(got.double(), want)


def test_mask_properties():
    n = 1 << 16
    a = R.drop_factors(0.25, 42, None, n)
    assert torch.equal(a, R.drop_factors(0.25, 42, 0, n))          # no counter = a counter at 0
    assert not torch.equal(a, R.drop_factors(0.25, 42, 1, n))      # the step draws a fresh mask
    assert not torch.equal(a, R.drop_factors(0.25, 43, None, n))
    assert set(a.unique().tolist()) == {0.0, float(np.float32(1) / np.float32(0.75))}
    assert abs(float((a != 0).float().mean()) - 0.75) < 0.01
    # the 64-bit index path: the high word of the pair index enters the hash
    big = np.array([5, 5 + (1 << 32)], dtype=np.uint64)
    h = R.hash32(R.drop_seed(42, None), big)
    assert h[0] != h[1]
    assert torch.equal(R.drop_factors(1.0, 1, None, 64), torch.zeros(64))
