"""Plain float64 references of the GST style-encoder kernels (``csrc/gst.hip``): one GRU gate step, the GRU loop,
the style-token attention.  Differentiable (autograd gives the backward), written out from the equations of
``torch.nn.GRU`` and of the reference's multi-head attention; ``tests/test_gst_reference_cpu.py`` checks them against
``torch.nn.GRU`` and ``oracle.fs2_oracle._GstMHA`` without a GPU, so a GPU mismatch is the kernel's."""
import math

import torch


def gru_step_ref(gi, gh, h):
    """One step of nn.GRU (gate order r, z, n).  gi [B, 3U] = W_ih x + b_ih, gh [B, 3U] = W_hh h + b_hh, h [B, U].
    Returns (h', (r, z, n, gh_n)) -- the second item is what ``gru_gate_fwd`` saves for its backward."""
    U = h.shape[-1]
    r = torch.sigmoid(gi[:, :U] + gh[:, :U])
    z = torch.sigmoid(gi[:, U:2 * U] + gh[:, U:2 * U])
    hn = gh[:, 2 * U:]
    n = torch.tanh(gi[:, 2 * U:] + r * hn)
    return (1 - z) * n + z * h, (r, z, n, hn)


def gru_sequence_ref(x, w_ih, w_hh, b_ih, b_hh, h0=None):
    """nn.GRU(batch_first=True), one layer: x [B, L, I] -> the last hidden state [B, U]."""
    B, L, _ = x.shape
    U = w_hh.shape[1]
    h = x.new_zeros(B, U) if h0 is None else h0
    for t in range(L):
        h, _ = gru_step_ref(x[:, t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh, h)
    return h


def gst_attention_ref(q, k, v, heads):
    """q [B, F]; k, v [NT, F] (shared) or [B, NT, F] (one copy per utterance, whose gradients are the kernel's
    ``dk_part`` / ``dv_part``); F = heads * d_k.  Returns (p [B, heads, NT], ctx [B, F]):
    p = softmax(q k^T / sqrt(d_k)) per head, ctx = p v."""
    B, F = q.shape
    dk = F // heads
    if k.dim() == 2:
        k, v = k.unsqueeze(0).expand(B, -1, -1), v.unsqueeze(0).expand(B, -1, -1)
    NT = k.shape[1]
    qh = q.view(B, heads, 1, dk)
    kh = k.reshape(B, NT, heads, dk).transpose(1, 2)   # [B, heads, NT, dk]
    vh = v.reshape(B, NT, heads, dk).transpose(1, 2)
    p = torch.softmax((qh * kh).sum(-1) / math.sqrt(dk), dim=-1)   # [B, heads, NT]
    ctx = (p.unsqueeze(-1) * vh).sum(2).reshape(B, F)
    return p, ctx
