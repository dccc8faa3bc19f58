"""A plain-torch restatement of LENGTH-AWARE TRAINING of the GST style encoder (``StyleEncoder.fwd_train``), written from
its definition and differentiable (autograd gives the backward).  It owns no weights: it runs on the parameters and
buffers of an ``oracle.fs2_oracle.StyleEncoder`` (``ref_enc.convs``, ``ref_enc.gru``, ``stl``), in whatever dtype that
module has -- float64 as the yardstick, float32 to measure what fp32 arithmetic alone costs.

With ``L_0 = lens`` and ``L_{l+1} = (L_l - 1) // 2 + 1`` (0 stays 0), for each of the six layers with input ``x_l``
``[B, C_l, H_l, W_l]``:

1. rows ``t >= L_l[b]`` of ``x_l`` are zero;
2. ``raw = conv3x3 stride 2 pad 1 (x_l)``;
3. train mode: BatchNorm's mean and biased variance per channel run over the positions ``(b, t, f)`` with
   ``t < L_{l+1}[b]`` only (count ``N = W_{l+1} * sum_b L_{l+1}[b]``); the running buffers move with momentum 0.1 and the
   unbiased variance ``N / (N - 1)``.  Eval mode: the running statistics, element-wise;
4. ReLU.

The GRU (gate order r, z, n; h0 = 0) runs ``L_6[b]`` steps on row b (``tests.gst_references.gru_sequence_ref``); the style
token layer is the oracle's own."""
import torch
import torch.nn.functional as F

from tests.gst_references import gru_sequence_ref


def conv_lens(lens, n=6):
    """[n + 1][B] row counts as Python ints."""
    table = [[int(v) for v in lens]]
    for _ in range(n):
        table.append([(v - 1) // 2 + 1 if v > 0 else 0 for v in table[-1]])
    return table


def row_mask(L, H, like):
    """[B, 1, H, 1]: 1 where t < L[b]."""
    t = torch.arange(H)
    return (t[None, :] < torch.tensor(L)[:, None]).to(like.dtype)[:, None, :, None]


def masked_batchnorm(raw, L, bn, training, update=True):
    """BatchNorm2d ``bn`` on ``raw`` [B, C, H, W] with training statistics over rows ``t < L[b]`` only."""
    if not training:
        mean, var = bn.running_mean, bn.running_var
    else:
        m = row_mask(L, raw.shape[2], raw)
        N = raw.shape[3] * sum(min(max(v, 0), raw.shape[2]) for v in L)
        # (where, not a product: positions beyond the lengths may hold anything, NaN included)
        kept = torch.where(m.bool(), raw, torch.zeros_like(raw))
        mean = kept.sum(dim=(0, 2, 3)) / N
        dev = torch.where(m.bool(), raw - mean[None, :, None, None], torch.zeros_like(raw))
        var = (dev * dev).sum(dim=(0, 2, 3)) / N
        if update:
            with torch.no_grad():
                unbiased = var * N / (N - 1) if N > 1 else var
                bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean.detach())
                bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * unbiased.detach())
    scale = bn.weight / torch.sqrt(var + bn.eps)
    return (raw - mean[None, :, None, None]) * scale[None, :, None, None] + bn.bias[None, :, None, None]


def style_lens_ref(enc, mel, lens, training=None):
    """The style [B, 256] of ``mel`` [B, T, n_mels] under lengths ``lens`` with the weights of ``enc`` (an
    ``oracle.fs2_oracle.StyleEncoder``); ``training`` defaults to ``enc.training``.  Train mode moves ``enc``'s running
    BatchNorm buffers."""
    training = enc.training if training is None else training
    convs, gru = enc.ref_enc.convs, enc.ref_enc.gru
    n = len(convs) // 3
    table = conv_lens(lens, n)
    x = mel.unsqueeze(1)                                       # [B, 1, T, n_mels]
    for l in range(n):
        x = x * row_mask(table[l], x.shape[2], x)
        raw = F.conv2d(x, convs[3 * l].weight, None, stride=2, padding=1)
        x = torch.relu(masked_batchnorm(raw, table[l + 1], convs[3 * l + 1], training))
    hs = x.transpose(1, 2).contiguous().view(x.shape[0], x.shape[2], -1)   # [B, L', C * F']
    rows = [gru_sequence_ref(hs[b:b + 1, :min(table[n][b], hs.shape[1])], gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
                             gru.bias_hh_l0) for b in range(hs.shape[0])]
    return enc.stl(torch.cat(rows))


class LengthAwareStyle(torch.nn.Module):
    """Drop-in for the ``gst`` of ``oracle.fs2_oracle.FastSpeech2Oracle``: the same parameters (state-dict keys
    ``ref_enc.*`` / ``stl.*``), called with the padded target mels; the lengths are set before each forward."""

    def __init__(self, enc):
        super().__init__()
        self.ref_enc, self.stl = enc.ref_enc, enc.stl
        self.lens = None

    def forward(self, mel):
        return style_lens_ref(self, mel, self.lens)

    def condition_on_gst_tokens(self, batch_size, index=0):
        raise NotImplementedError("length-aware training has no free-inference path")
