"""CPU: the hand-written float64 references of the GST kernel tests (``tests/gst_references.py``) against
``torch.nn.GRU`` (forward and autograd) and ``oracle.fs2_oracle._GstMHA`` with identity projections, to 1e-12."""
import pytest
import torch

from oracle import fs2_oracle as O
from tests import gst_references as R

TOL = 1e-12


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _gru(I, U, seed):
    gru = torch.nn.GRU(I, U, batch_first=True).double()
    with torch.no_grad():
        for i, p in enumerate(gru.parameters()):
            p.copy_(_rnd(*p.shape, seed=seed + i) * U ** -0.5)
    return gru


def _err(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("B,I,U", [(1, 16, 128), (3, 7, 32), (2, 5, 200)])
def test_gru_step_reference_is_nn_gru(B, I, U):
    """One step from a non-zero state: h', and the gradients of x, h0 and all four parameter tensors."""
    gru = _gru(I, U, seed=10)
    x, h0, dh = _rnd(B, 1, I, seed=1), _rnd(B, U, seed=2), _rnd(B, U, seed=3)
    xa, ha = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    _, want = gru(xa, ha.unsqueeze(0))
    want[0].backward(dh)
    want_grads = [p.grad.clone() for p in gru.parameters()]
    w_ih, w_hh, b_ih, b_hh = [p.detach().clone().requires_grad_(True) for p in gru.parameters()]
    xb, hb = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    got, (r, z, n, hn) = R.gru_step_ref(xb[:, 0] @ w_ih.t() + b_ih, hb @ w_hh.t() + b_hh, hb)
    got.backward(dh)
    assert _err(got, want[0]) < TOL
    assert _err(xb.grad, xa.grad) < TOL and _err(hb.grad, ha.grad) < TOL
    for g, w in zip((w_ih, w_hh, b_ih, b_hh), want_grads):
        assert _err(g.grad, w) < TOL
    assert float(r.min()) >= 0 and float(r.max()) <= 1 and float(z.min()) >= 0 and float(z.max()) <= 1
    assert _err(hn, (h0 @ w_hh.t() + b_hh)[:, 2 * U:].detach()) < TOL and float(n.abs().max()) <= 1


@pytest.mark.parametrize("L", [1, 2, 11])
def test_gru_sequence_reference_is_nn_gru(L):
    B, I, U = 3, 24, 128
    gru = _gru(I, U, seed=20)
    x, dy = _rnd(B, L, I, seed=4), _rnd(B, U, seed=5)
    xa = x.clone().requires_grad_(True)
    _, want = gru(xa)
    (want[0] * dy).sum().backward()
    want_grads = [p.grad.clone() for p in gru.parameters()]
    ps = [p.detach().clone().requires_grad_(True) for p in gru.parameters()]
    xb = x.clone().requires_grad_(True)
    got = R.gru_sequence_ref(xb, *ps)
    (got * dy).sum().backward()
    assert _err(got, want[0]) < TOL and _err(xb.grad, xa.grad) < TOL
    for g, w in zip(ps, want_grads):
        assert _err(g.grad, w) < TOL


@pytest.mark.parametrize("B,NT,heads", [(1, 10, 4), (5, 10, 4), (3, 1, 4), (3, 32, 4), (2, 7, 1), (2, 13, 3)])
def test_attention_reference_is_the_oracle_mha(B, NT, heads):
    """``_GstMHA`` with identity projections (zero biases) is the bare attention: output = ctx, and the gradients of
    query / key / value are those of q / k / v.  The per-utterance key and value copies give dk_part / dv_part, whose
    sum over the batch is the gradient of the shared tokens."""
    F = heads * 64
    mha = O._GstMHA(F, F, F, heads, F).double()
    with torch.no_grad():
        for lin in (mha.linear_q, mha.linear_k, mha.linear_v, mha.linear_out):
            lin.weight.copy_(torch.eye(F, dtype=torch.float64))
            lin.bias.zero_()
    q, k, v, dctx = _rnd(B, F, seed=6) * 3, _rnd(NT, F, seed=7), _rnd(NT, F, seed=8), _rnd(B, F, seed=9)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    want = mha(qa.unsqueeze(1), ka.unsqueeze(0).expand(B, -1, -1), va.unsqueeze(0).expand(B, -1, -1)).squeeze(1)
    (want * dctx).sum().backward()
    qb = q.clone().requires_grad_(True)
    kb = k.unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)
    vb = v.unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)
    p, got = R.gst_attention_ref(qb, kb, vb, heads)
    (got * dctx).sum().backward()
    assert p.shape == (B, heads, NT) and float((p.sum(-1) - 1).abs().max()) < TOL
    assert _err(got, want) < TOL and _err(qb.grad, qa.grad) < TOL
    assert _err(kb.grad.sum(0), ka.grad) < TOL and _err(vb.grad.sum(0), va.grad) < TOL
    # the shared-token form (2-D k, v) is the same function
    p2, got2 = R.gst_attention_ref(q, k, v, heads)
    assert _err(got2, want.detach()) < TOL and _err(p2, p.detach()) < TOL
