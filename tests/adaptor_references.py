"""Plain CPU references of the gather / scatter / optimizer kernels of ``csrc/misc.hip`` -- positional table, embedding,
bucketize + embedding, LengthRegulator, fused Noam / global-norm clip / AdamW -- and the input generators of their GPU
tests (``tests/test_adaptor_kernels_gpu.py``).  Every float is computed in float64; results that are a gather or a
single fp32 add are returned rounded once to fp32, which is that add.  ``tests/test_adaptor_reference_cpu.py`` checks the
references against torch's own operators and asserts the edge conditions the generated inputs are there to produce."""
import math

import numpy as np
import torch


def f32(v):
    """A Python float rounded to fp32: how a float kernel argument arrives."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------
# positional table
# ---------------------------------------------------------------------------------------------------------------------
def inv_freq(D):
    """The model's buffer: 1 / 10000^(2i / D), fp32."""
    return 1 / (10000 ** (torch.arange(0.0, D, 2.0) / D))


def posenc_angles(inv, T):
    """The fp32 product float32(t) * inv_freq[c] as [T, D / 2] (what a matmul of a column by a row gives)."""
    return torch.arange(T, dtype=torch.float32)[:, None] * inv.float()[None, :]


def posenc_table64(inv, T):
    """[T, D] float64: [sin | cos] of the fp32 angle, evaluated in float64."""
    a = posenc_angles(inv, T).double()
    return torch.cat([a.sin(), a.cos()], 1)


# ---------------------------------------------------------------------------------------------------------------------
# one fp32 add / gathers
# ---------------------------------------------------------------------------------------------------------------------
def add32(a, b):
    """a + b in float64, rounded once: the fp32 sum (exact in float64 for operands within 2^29 of each other)."""
    return (a.double() + b.double()).float()


def add_posenc(x, table, lens):
    """x [B, T, D] + table[t] where t < lens[b]; padded frames are x itself."""
    B, T, D = x.shape
    on = torch.arange(T)[None, :] < lens.long()[:, None]
    return torch.where(on[..., None], add32(x, table[:T][None]), x)


def embedding_bwd64(idx, dy, V, padding_idx=-1):
    """(dW [V, D] float64 = sum of the dy rows of each index, the rows of ``padding_idx`` dropped; the same sum over |dy|:
    the scale of every element)."""
    idx, dy = idx.reshape(-1).long(), dy.reshape(idx.numel(), -1).double()
    keep = idx != padding_idx
    dW, sc = (torch.zeros(V, dy.shape[1], dtype=torch.float64) for _ in range(2))
    dW.index_add_(0, idx[keep], dy[keep])
    sc.index_add_(0, idx[keep], dy[keep].abs())
    return dW, sc


def control_of_rows(control, ctl_idx):
    """control [B, Ts], ctl_idx [B, T] -> the control of every frame: control[b, ctl_idx[b, t]], exactly 1 where the
    index lies outside [0, Ts)."""
    Ts = control.shape[1]
    j = ctl_idx.long()
    inside = (j >= 0) & (j < Ts)
    return torch.where(inside, control.gather(1, j.clamp(0, Ts - 1)), torch.ones((), dtype=control.dtype))


def bucket_embed_add(val, control, bins, W, x):
    """(x + W[idx], idx int64, scaled) with scaled = val * control as ONE fp32 product (control: a number, taken as fp32,
    or a tensor of val's shape) and idx = torch.bucketize(scaled, bins)."""
    c = control.float() if isinstance(control, torch.Tensor) else torch.tensor(control, dtype=torch.float32)
    scaled = val.float() * c
    idx = torch.bucketize(scaled, bins)
    return add32(x.reshape(-1, x.shape[-1]), W[idx.reshape(-1)]).reshape(x.shape), idx, scaled


# ---------------------------------------------------------------------------------------------------------------------
# length regulator
# ---------------------------------------------------------------------------------------------------------------------
def length_regulate(x, dur, Tm, table=None):
    """x [B, Ts, D], dur [B, Ts] -> (out [B, Tm, D] fp32, cum [B, Ts] int32, lens [B] int32, src_idx [B, Tm] int32):
    repeat_interleave of clamp(dur, 0), truncated or zero-filled to Tm, table[t] added to the valid frames."""
    B, Ts, D = x.shape
    d = dur.long().clamp(min=0)
    cum = d.cumsum(1)
    out = torch.zeros(B, Tm, D, dtype=torch.float32)
    src = torch.full((B, Tm), -1, dtype=torch.int32)
    for b in range(B):
        rows = torch.repeat_interleave(x[b], d[b], dim=0)[:Tm]
        n = rows.shape[0]
        out[b, :n] = rows if table is None else add32(rows, table[:n])
        src[b, :n] = torch.repeat_interleave(torch.arange(Ts, dtype=torch.int32), d[b])[:Tm]
    return out, cum.int(), cum[:, -1].clamp(max=Tm).int(), src


def length_regulate_bwd64(dy, src_idx, Ts):
    """(dx [B, Ts, D] float64: the sum of dy over each token's frames; the same sum over |dy|)."""
    B, Tm, D = dy.shape
    dx, sc = (torch.zeros(B, Ts, D, dtype=torch.float64) for _ in range(2))
    for b in range(B):
        on = src_idx[b] >= 0
        j = src_idx[b][on].long()
        dx[b].index_add_(0, j, dy[b][on].double())
        sc[b].index_add_(0, j, dy[b][on].double().abs())
    return dx, sc


# ---------------------------------------------------------------------------------------------------------------------
# optimizer: Noam rate, global-norm clip, decoupled AdamW -- one step as csrc/misc.hip and fs2/noam.py define it
# ---------------------------------------------------------------------------------------------------------------------
class Optimizer64:
    """Float64 state of one parameter vector.  The hyperparameters are taken as the fp32 numbers the kernels receive."""

    def __init__(self, p0, base_lr, warmup, betas, eps, weight_decay, max_norm, grad_scale):
        self.p = p0.double().clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.base_lr, self.warmup, self.eps, self.wd = f32(base_lr), f32(warmup), f32(eps), f32(weight_decay)
        self.b1, self.b2 = f32(betas[0]), f32(betas[1])
        self.max_norm, self.grad_scale = f32(max_norm), f32(grad_scale)
        self.k = 0

    def step(self, g):
        """One step on the gradient g; returns the step record {step, lr, bc1, bc2, grad_norm, clip_coef}."""
        self.k += 1
        k, w = self.k, self.warmup
        s = max(1, k - 1)
        lr = self.base_lr * math.sqrt(w) * min(s ** -0.5, s * w ** -1.5)
        bc1, bc2 = 1.0 - self.b1 ** k, 1.0 - self.b2 ** k
        g = g.double()
        norm = math.sqrt(float((g * g).sum())) * self.grad_scale
        coef = self.grad_scale
        if self.max_norm > 0:
            coef = min(1.0, self.max_norm / (norm + 1e-6)) * self.grad_scale
        g = g * coef
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        self.p = self.p * (1 - lr * self.wd) - (lr / bc1) * self.m / (self.v.sqrt() / math.sqrt(bc2) + self.eps)
        return {"step": k, "lr": lr, "bc1": bc1, "bc2": bc2, "grad_norm": norm, "clip_coef": coef}


def noam_lr(base_lr, warmup, k):
    """fs2/noam.py at optimizer step k (1-based): last_epoch = max(1, k - 1)."""
    s = max(1, k - 1)
    return base_lr * warmup ** 0.5 * min(s ** (-0.5), s * warmup ** (-1.5))


# ---------------------------------------------------------------------------------------------------------------------
# inputs of the GPU tests (the CPU test asserts what each is there to produce)
# ---------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- optimizer
OPT = dict(base_lr=1e-3, warmup=4, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
OPT_STEPS = 12
OPT_SIZES = [1, 5, 1000, 8192 * 256 + 3]
OPT_CONFIGS = [(1.0, 1.0), (1.0, 0.25), (0.0, 0.25)]  # (max_norm, grad_scale)
OPT_ZERO_STEP = 6


def opt_params(n):
    return torch.randn(n, generator=gen(7000 + n % 1000))


def opt_grad_kind(k):
    """Step k (1-based): large and small gradients by turn, all zero once."""
    return "zero" if k == OPT_ZERO_STEP else ("large" if k % 2 else "small")


def opt_dead(n):
    """The fixed tenth of the elements whose gradient is always zero."""
    return torch.arange(n) % 10 == 3


def opt_grad(n, k):
    kind = opt_grad_kind(k)
    if kind == "zero":
        return torch.zeros(n)
    r = torch.randn(n, generator=gen(100 * k + n % 97))
    g = (r + 0.5 * torch.sign(r)) * (30.0 if kind == "large" else 1e-6)  # no element so small that n = 1 misses its kind
    g[opt_dead(n)] = 0.0
    return g


# ---- bucketize
BUCKET_M = 4099


def bucket_bins(NB):
    """Sorted edges; the 255-edge vector repeats three of its edges."""
    if NB == 1:
        return torch.tensor([0.5])
    if NB == 2:
        return torch.tensor([-1.0, 1.25])
    if NB == 255:
        b = torch.linspace(-3, 3, 255)
        b[11], b[12], b[200] = b[10], b[10], b[199]
        return b
    return torch.linspace(-2.5, 4, NB)


def bucket_specials(bins, control):
    """The values the issue lists: every edge and its two fp32 neighbours, +-inf, NaN, points beyond both ends, and for
    control != 1 the quotients edge / control."""
    inf = torch.tensor(float("inf"))
    parts = [bins, torch.nextafter(bins, inf), torch.nextafter(bins, -inf),
             torch.tensor([float("inf"), float("-inf"), float("nan"), float("nan")]),
             torch.stack([bins[0] - 1, bins[0] * 0 - 3e38, bins[-1] + 1, bins[-1] * 0 + 3e38])]
    if control != 1.0:
        parts.append(bins / torch.tensor(control, dtype=torch.float32))
    return torch.cat(parts)


def bucket_values(bins, control, M=BUCKET_M, seed=0):
    """[M] fp32: the specials at shuffled positions among random values over the edges' range and a little beyond."""
    g = gen(31 * bins.numel() + seed)
    sp = bucket_specials(bins, control)
    lo, hi = float(bins[0]) - 1, float(bins[-1]) + 1
    v = lo + (hi - lo) * torch.rand(M, generator=g)
    pos = torch.randperm(M, generator=g)[: sp.numel()]
    v[pos] = sp
    return v


# ---- embedding
def skewed_indices(M, V, seed=0):
    """int32 [M] in [0, V): index 7 owns about 40 % of the rows, V // 12 + 5 indices never occur, index 0 does."""
    g = gen(500 + M + V + seed)
    never = torch.arange(3, V, 12)[: V // 12 + 5]
    allowed = torch.tensor([v for v in range(V) if v not in set(never.tolist())])
    idx = allowed[torch.randint(0, allowed.numel(), (M,), generator=g)]
    idx[torch.rand(M, generator=g) < 0.4] = 7
    idx[M // 2] = 0
    return idx.int(), never


# ---- length regulator
LR_SHAPES = [(3, 301, 2049, 384), (70, 13, 30, 8), (1, 1, 1, 4)]
LR_LONG = 600


def lr_durations(B, Ts, Tm):
    """int32 [B, Ts].  The first shape: utterance 0 totals exactly Tm with a token of 600 frames, utterance 1 runs past Tm
    with the cut inside a token, utterance 2 is all zero; zero runs at the start, the middle and the end, and negative
    entries (they count as 0), in the first two."""
    g = gen(10007 * B + 31 * Ts + Tm)
    if (B, Ts, Tm) == LR_SHAPES[0][:3]:
        d = torch.zeros(B, Ts, dtype=torch.int32)
        for b, top in ((0, 9), (1, 22)):
            r = torch.randint(0, top, (Ts,), generator=g, dtype=torch.int32)
            r[torch.rand(Ts, generator=g) < 0.15] = 0
            r[:5], r[150:160], r[-7:] = 0, 0, 0
            r[20], r[200], r[250] = -3, -1, -7
            d[b] = r
        d[0, 100] = LR_LONG
        d[0, 101] = 0
        d[0, 101] = Tm - int(d[0].clamp(min=0).sum())
        return d
    if B == 1:
        return torch.full((1, Ts), 2, dtype=torch.int32)
    return torch.randint(-3, 6, (B, Ts), generator=g, dtype=torch.int32)
