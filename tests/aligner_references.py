"""Plain references of the learned-alignment kernels (``csrc/aligner.hip``) shared by ``tests/test_aligner_gpu.py`` and
``tests/test_aligner_shapes_gpu.py``: the restatement of fs2/attn/attention.py's distance attention (logits, attn_logprob,
attn_soft), the case builder, and the max-error-over-max-magnitude comparison.  Everything is differentiable and works
in the dtype of its inputs, so ``.double()`` inputs give the float64 reference and autograd gives the backward."""
import torch
import torch.nn.functional as F

from oracle import fs2_oracle as O


def rel_err(a, b):
    """max |a - b| over the finite entries of b, divided by max |b| (floored at 1e-6)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    fin = torch.isfinite(b)
    scale = max(float(b[fin].abs().max()), 1e-6) if bool(fin.any()) else 1e-6
    return float((a[fin] - b[fin]).abs().max()) / scale if bool(fin.any()) else 0.0


def close(a, b, tol=2e-5, msg=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    fin = torch.isfinite(b)
    assert torch.equal(torch.isfinite(a), fin), msg + ": non-finite pattern"
    scale = max(float(b[fin].abs().max()), 1e-6)
    err = float((a[fin] - b[fin]).abs().max()) / scale
    assert err < tol, f"{msg}: rel err {err:.3e}"


def make_case(B=3, T1=37, T2=11, C=80, seed=0, key_lens=None, q_lens=None, scale=3.0):
    """q [B, T1, C], k [B, T2, C] (randn * scale), ragged lengths and the beta-binomial prior, all from ``seed``."""
    g = torch.Generator().manual_seed(seed)
    q, k = torch.randn(B, T1, C, generator=g) * scale, torch.randn(B, T2, C, generator=g) * scale
    if key_lens is None:
        key_lens = [T2, max(2, T2 - 3), max(2, T2 // 2)][:B]
    if q_lens is None:
        q_lens = [T1, T1 - 5, max(T2, T1 // 2)][:B]
    key_lens = torch.tensor(list(key_lens), dtype=torch.int32)
    q_lens = torch.tensor(list(q_lens), dtype=torch.int32)
    prior = O.beta_binomial_prior(q_lens, key_lens, T1, T2)
    return q, k, key_lens, q_lens, prior


def ref_logits(q, k):
    """-0.0005 * squared distance.  float64 inputs take the Gram form (|q|^2 + |k|^2 - 2 q.k: exact to ~1e-13 there and
    it spares the (B, T1, T2, C) difference tensor at the long-text shapes); fp32 inputs the difference form."""
    if q.dtype == torch.float64:
        d = (q * q).sum(-1)[:, :, None] + (k * k).sum(-1)[:, None, :] - 2.0 * q @ k.transpose(1, 2)
    else:
        d = ((q[:, :, None, :] - k[:, None, :, :]) ** 2).sum(-1)
    return -0.0005 * d


def ref_softmax(logits, key_lens, prior):
    """(attn_logprob, attn_soft) of the logits: log_softmax + log(prior + 1e-8); softmax of that over the valid keys."""
    lp = F.log_softmax(logits, dim=2) + torch.log(prior.to(logits.dtype) + 1e-8)
    mask = torch.arange(logits.shape[2])[None, None, :] >= key_lens[:, None, None]
    soft = F.softmax(lp.masked_fill(mask, -float("inf")), dim=2)
    return lp, soft


def ref_attention(q, k, key_lens, prior):
    logits = ref_logits(q, k)
    lp, soft = ref_softmax(logits, key_lens, prior)
    return logits, lp, soft


def hard_to_idx(hard, q_lens):
    """hard [B, T1, T2] 0/1 map -> int32 [B, T1] key index of each frame, -1 on the frames at and beyond q_lens[b]."""
    idx = hard.argmax(-1).to(torch.int32)
    pad = torch.arange(hard.shape[1])[None, :] >= q_lens[:, None]
    return idx.masked_fill(pad, -1)
