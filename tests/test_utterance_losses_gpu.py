"""GPU: ``fs2hip_utterance_losses`` through the C ABI -- the per-utterance loss table of a teacher-forced batch.

The yardstick is a float64 computation on the CPU, written here from the formulas of include/fs2hip.h:
``weight * sum_{t < len_b, c} f(pred - tgt) / (len_b * C)`` with ``len_b = clamp(lens[b], 0, T)``, the binarisation term
over the frames below the mel length whose ``hard_idx`` is not negative, the CTC column as ``weight * nll[b]``, the total as
the sum of the columns.  The bound is the project's loss bound, ``1e-4 * max(1, |ref|)``.  Beyond values: two runs are
bit-equal, and every row of a batch is bit-equal to the same utterance scored as ``B = 1, T = len_b`` -- the order of the
additions may depend on ``len_b * C`` alone, not on the batch, the padding or the alignment of the utterance's base address.
"""
import math

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda"
COLS = 8
PITCH, ENERGY, DURATION, SPEC, POSTNET, CTC, BIN, TOTAL = range(8)
EINVAL = -22


def _call(terms, B, bin_term=None, ctc_term=None, out=None, n=None):
    """The raw entry point.  ``terms``: [(column, pred, tgt, lens, T, C, kind, weight)], kind 0 / 1, an int32 ``tgt`` is a
    duration.  Returns (code, table); the table starts as NaN so that an element nobody wrote is seen."""
    members = (hip.ScoreMember * max(len(terms), 1))()
    for m, (col, pred, tgt, lens, T, C, kind, w) in zip(members, terms):
        m.pred = None if pred is None else pred.data_ptr()
        m.lens = None if lens is None else lens.data_ptr()
        m.tgt = m.tgt_int = None
        if tgt is not None:
            if tgt.dtype == torch.int32:
                m.tgt_int = tgt.data_ptr()
            else:
                m.tgt = tgt.data_ptr()
        m.T, m.C, m.kind, m.weight, m.column = T, C, kind, w, col
    soft, hard, mel_lens, bw = bin_term if bin_term is not None else (None, None, None, 0.0)
    nll, cw = ctc_term if ctc_term is not None else (None, 0.0)
    Tm, Ts = (soft.shape[1], soft.shape[2]) if soft is not None else (0, 0)
    if out is None:
        out = torch.full((max(B, 1), COLS), float("nan"), device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    code = hip.real_lib().fs2hip_utterance_losses(members, len(terms) if n is None else n, p(soft), p(hard), p(mel_lens),
                                                  Tm, Ts, bw, p(nll), cw, out.data_ptr(), B, hip._stream())
    return code, out


def _run(terms, B, **kw):
    code, out = _call(terms, B, **kw)
    assert code == 0, code
    return out


def _ref(terms, B, bin_term=None, ctc_term=None):
    """float64 on the CPU."""
    ref = np.zeros((B, COLS))
    for col, pred, tgt, lens, T, C, kind, w in terms:
        p = pred.cpu().double().view(B, T, C)
        t = tgt.cpu().double()
        t = (torch.log(t + 1) if tgt.dtype == torch.int32 else t).view(B, T, C)
        for b, n in enumerate(lens.cpu().tolist()):
            n = min(max(n, 0), T)
            if n:
                d = p[b, :n] - t[b, :n]
                ref[b, col] = float(w) * float((d * d if kind == 0 else d.abs()).sum()) / (n * C)
    if bin_term is not None:
        soft, hard, mel_lens, w = bin_term
        s, h = soft.cpu().double(), hard.cpu()
        for b, n in enumerate(mel_lens.cpu().tolist()):
            n = min(max(n, 0), s.shape[1])
            picks = [math.log(max(float(s[b, t, int(h[b, t])]), 1e-12)) for t in range(n) if int(h[b, t]) >= 0]
            if picks:
                ref[b, BIN] = -float(w) * sum(picks) / len(picks)
    if ctc_term is not None:
        nll, w = ctc_term
        ref[:, CTC] = float(w) * nll.cpu().double().numpy()
    ref[:, TOTAL] = ref[:, :TOTAL].sum(1)
    return ref


def _check(tag, got, ref):
    g = got.cpu().double().numpy()
    assert np.isfinite(g).all(), (tag, g)
    err = np.abs(g - ref)
    tol = 1e-4 * np.maximum(1.0, np.abs(ref))
    print(f"{tag}: worst error / bound {float((err / tol).max()):.4f}")
    assert (err <= tol).all(), (tag, g, ref)
    # the total is the fp32 sum of the columns, in order
    g32 = got.cpu().numpy()
    total = np.zeros(g32.shape[0], dtype=np.float32)
    for c in range(TOTAL):
        total = (total + g32[:, c]).astype(np.float32)
    assert np.array_equal(total, g32[:, TOTAL]), (tag, total, g32[:, TOTAL])


def _lens(B, T, g):
    """A value above T (clamped to T), 0, 1 and T first, random after that."""
    fixed = [T + 3, 0, 1, T]
    rest = torch.randint(0, T + 1, (B,), generator=g).tolist()
    return torch.tensor((fixed + rest)[:B] if B > 1 else [T], dtype=torch.int32)


def _nan_tail(x, lens, B, T, C):
    """NaN in every row at and beyond the clamped length: the kernel must never read them."""
    v = x.view(B, T, C)
    for b, n in enumerate(lens.tolist()):
        v[b, min(max(n, 0), T):] = float("nan")
    return x


def _unaligned(x):
    """The same values in a view one element into a fresh buffer: a 4-byte but not 16-byte aligned base."""
    buf = torch.empty(x.numel() + 1, device=x.device, dtype=x.dtype)
    v = buf[1:]
    v.copy_(x.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def _mean_terms(B, T, C, seed):
    """MSE into spec, MAE into postnet (both [B, T, C] with NaN tails), the int-target form into duration ([B, T, 1])."""
    g = torch.Generator().manual_seed(seed)
    lens = _lens(B, T, g)
    pred = _nan_tail(torch.randn(B * T * C, generator=g) * 2, lens, B, T, C)
    pred2 = _nan_tail(torch.randn(B * T * C, generator=g), lens, B, T, C)
    tgt = _nan_tail(torch.randn(B * T * C, generator=g), lens, B, T, C)
    dlens = _lens(B, T, g)
    logd = _nan_tail(torch.randn(B * T, generator=g), dlens, B, T, 1)
    dur = torch.randint(0, 30, (B * T,), generator=g, dtype=torch.int32)
    d = lambda t: t.to(DEV)
    lens, dlens, tgt = d(lens), d(dlens), d(tgt)
    return [(SPEC, d(pred), tgt, lens, T, C, 0, 1.0), (POSTNET, d(pred2), tgt, lens, T, C, 1, 0.7),
            (DURATION, d(logd), d(dur), dlens, T, 1, 0, 1.3)]


def _alone(term, b):
    """Utterance ``b`` of a mean term as a batch of one without padding (None: it has no elements)."""
    col, pred, tgt, lens, T, C, kind, w = term
    n = min(max(int(lens[b]), 0), T)
    if n == 0:
        return None
    cut = lambda x: x.view(-1, T, C)[b, :n].contiguous().view(-1)
    return (col, cut(pred), cut(tgt), torch.tensor([n], dtype=torch.int32, device=DEV), n, C, kind, w)


def _rows_equal_alone(tag, terms, B, got, bin_term=None, ctc_term=None):
    for b in range(B):
        mine = [t for t in (_alone(term, b) for term in terms) if t is not None]
        kw = {}
        if bin_term is not None:
            soft, hard, mel_lens, w = bin_term
            n = min(max(int(mel_lens[b]), 0), soft.shape[1])
            if n:
                kw["bin_term"] = (soft[b:b + 1, :n].contiguous(), hard[b:b + 1, :n].contiguous(),
                                  torch.tensor([n], dtype=torch.int32, device=DEV), w)
        if ctc_term is not None:
            kw["ctc_term"] = (ctc_term[0][b:b + 1].contiguous(), ctc_term[1])
        if not mine and not kw:
            assert float(got[b].abs().max()) == 0.0, (tag, b)   # an utterance without a single element: all zeros
            continue
        one = _run(mine, 1, **kw)
        assert torch.equal(one[0], got[b]), (tag, b, one[0].tolist(), got[b].tolist())


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("T", [1, 5, 37])
@pytest.mark.parametrize("C", [1, 3, 80])
def test_mean_terms(C, T, B):
    tag = f"C={C} T={T} B={B}"
    terms = _mean_terms(B, T, C, seed=1000 * C + 10 * T + B)
    got = _run(terms, B)
    _check(tag, got, _ref(terms, B))
    assert float(got[:, [PITCH, ENERGY, CTC, BIN]].abs().max()) == 0.0       # absent columns are 0
    assert torch.equal(got, _run(terms, B))                                   # two runs
    _rows_equal_alone(tag, terms, B, got)
    # the same data from bases that are not 16-byte aligned: the same bits
    shifted = [(col, _unaligned(p), _unaligned(t), lens, T_, C_, k, w) for col, p, t, lens, T_, C_, k, w in terms]
    assert torch.equal(got, _run(shifted, B)), tag


def test_many_passes_of_one_workgroup():
    """T = 700, C = 80: 56 000 elements per utterance, dozens of passes of a workgroup, unrolled and not."""
    B, T, C = 3, 700, 80
    g = torch.Generator().manual_seed(5)
    lens = torch.tensor([700, 523, 41], dtype=torch.int32)
    pred = _nan_tail(torch.randn(B * T * C, generator=g) * 3, lens, B, T, C).to(DEV)
    tgt = _nan_tail(torch.randn(B * T * C, generator=g), lens, B, T, C).to(DEV)
    lens = lens.to(DEV)
    terms = [(SPEC, pred, tgt, lens, T, C, 1, 1.0), (POSTNET, pred, tgt, lens, T, C, 0, 1.0)]
    got = _run(terms, B)
    _check("T=700 C=80", got, _ref(terms, B))
    assert torch.equal(got, _run(terms, B))
    _rows_equal_alone("T=700 C=80", terms, B, got)
    shifted = [(col, _unaligned(p), _unaligned(t), lens, T, C, k, w) for col, p, t, lens, T, C, k, w in terms]
    assert torch.equal(got, _run(shifted, B))


def test_bin_and_ctc_columns():
    B, Tm, Ts = 5, 37, 11
    g = torch.Generator().manual_seed(9)
    mel_lens = torch.tensor([37, 0, 1, 40, 20], dtype=torch.int32)
    soft = torch.softmax(torch.randn(B, Tm, Ts, generator=g) * 3, -1)
    hard = torch.randint(0, Ts, (B, Tm), generator=g, dtype=torch.int32)
    hard[0, ::4] = -1                       # frames without a token
    hard[4, :20] = -1                       # an utterance whose frames all lack one: count 0 -> 0
    for t in range(0, Tm, 5):
        soft[3, t, int(hard[3, t])] = 0.0   # the clamp at 1e-12
    for b, n in enumerate(mel_lens.tolist()):
        soft[b, min(n, Tm):] = float("nan")
    nll = torch.rand(B, generator=g) * 4
    nll[1] = 0.0                            # what the CTC kernel leaves for an empty or infinite utterance
    bin_term = (soft.to(DEV), hard.to(DEV), mel_lens.to(DEV), 0.35)
    ctc_term = (nll.to(DEV), 0.1)
    terms = _mean_terms(B, 5, 3, seed=77)
    got = _run(terms, B, bin_term=bin_term, ctc_term=ctc_term)
    ref = _ref(terms, B, bin_term, ctc_term)
    _check("bin + ctc", got, ref)
    assert abs(ref[3, BIN]) > 1.0 and ref[4, BIN] == 0.0 and ref[1, BIN] == 0.0   # the clamp and the empty cases are in play
    assert float(got[:, [PITCH, ENERGY]].abs().max()) == 0.0
    assert torch.equal(got, _run(terms, B, bin_term=bin_term, ctc_term=ctc_term))
    _rows_equal_alone("bin + ctc", terms, B, got, bin_term, ctc_term)
    # the two attention terms alone (no mean term at all), and a zero binarisation weight
    only = _run([], B, bin_term=bin_term, ctc_term=ctc_term)
    _check("bin + ctc only", only, _ref([], B, bin_term, ctc_term))
    zero_w = _run([], B, bin_term=bin_term[:3] + (0.0,))
    assert float(zero_w.abs().max()) == 0.0


def test_the_binding_gives_the_same_table():
    B, T, C = 3, 5, 3
    terms = _mean_terms(B, T, C, seed=3)
    names = {SPEC: "spec", POSTNET: "postnet", DURATION: "duration"}
    got = hip.utterance_losses([(names[c], p, t, lens, T_, C_, "mse" if k == 0 else "mae", w)
                                for c, p, t, lens, T_, C_, k, w in terms], B)
    assert torch.equal(got, _run(terms, B))
    with pytest.raises(ValueError, match="named twice"):
        hip.utterance_losses([("spec",) + tuple(terms[0][1:6]) + ("mse", 1.0)] * 2, B)
    with pytest.raises(ValueError, match="pred"):
        hip.utterance_losses([("spec", terms[0][1][:-1].contiguous()) + tuple(terms[0][2:6]) + ("mse", 1.0)], B)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.utterance_losses([("spec", terms[0][1].cpu()) + tuple(terms[0][2:6]) + ("mse", 1.0)], B)


def test_argument_errors():
    B, T, C = 2, 5, 3
    x = torch.zeros(B * T * C, device=DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ok = (SPEC, x, x, lens, T, C, 0, 1.0)
    assert _call([ok], B)[0] == 0
    bad = {
        "no pred": [(SPEC, None, x, lens, T, C, 0, 1.0)],
        "no target": [(SPEC, x, None, lens, T, C, 0, 1.0)],
        "no lens": [(SPEC, x, x, None, T, C, 0, 1.0)],
        "T = 0": [(SPEC, x, x, lens, 0, C, 0, 1.0)],
        "C < 0": [(SPEC, x, x, lens, T, -1, 0, 1.0)],
        "kind": [(SPEC, x, x, lens, T, C, 2, 1.0)],
        "column = total": [(TOTAL, x, x, lens, T, C, 0, 1.0)],
        "column < 0": [(-1, x, x, lens, T, C, 0, 1.0)],
        "column twice": [ok, (SPEC, x, x, lens, T, C, 1, 1.0)],
        "too many members": [(c % 7, x, x, lens, T, C, 0, 1.0) for c in range(9)],
    }
    for tag, terms in bad.items():
        assert _call(terms, B)[0] == EINVAL, tag
    assert _call([ok], 0)[0] == EINVAL                      # B
    assert _call([ok], B, n=-1)[0] == EINVAL
    assert hip.real_lib().fs2hip_utterance_losses(None, 1, None, None, None, 0, 0, 0.0, None, 0.0, x.data_ptr(), B,
                                                  hip._stream()) == EINVAL          # members
    members = (hip.ScoreMember * 1)()
    assert hip.real_lib().fs2hip_utterance_losses(members, 0, None, None, None, 0, 0, 0.0, x.data_ptr(), 1.0, None, B,
                                                  hip._stream()) == EINVAL          # scores
    soft = torch.ones(B, T, 4, device=DEV)
    hard = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    nll = torch.zeros(B, device=DEV)
    assert _call([], B, bin_term=(soft, None, lens, 1.0))[0] == EINVAL              # soft without hard_idx
    assert _call([], B, bin_term=(soft, hard, None, 1.0))[0] == EINVAL              # ... without the lengths
    assert _call([(BIN, x, x, lens, T, C, 0, 1.0)], B, bin_term=(soft, hard, lens, 1.0))[0] == EINVAL   # column 6 twice
    assert _call([(CTC, x, x, lens, T, C, 0, 1.0)], B, ctc_term=(nll, 1.0))[0] == EINVAL                # column 5 twice
    torch.cuda.synchronize()
