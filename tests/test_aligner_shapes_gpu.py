"""GPU parity of the learned-alignment kernels (``csrc/aligner.hip``) at the shapes, ragged lengths and degenerate
lengths that ``tests/test_aligner_gpu.py`` does not reach: several 64-key tiles, texts of 129..520 tokens, the
strided state loops of the CTC recursion, every dispatch branch of the alignment search, more than one workgroup of
the binarisation loss.  Each test says (assertion or comment next to the launch condition) which branch it enters.

References: float64 CPU evaluation of the same formula (``tests/aligner_references.py``, ``oracle.fs2_oracle``) and
autograd through it.  Integer results (the alignment search, hard indices, durations) are compared bit for bit.
Floating point: ``close(..., 2e-5)`` (max error over max magnitude), except the CTC gradient and what is downstream of
it, whose bound is ``max(1e-4, 4 * e_ref)`` with ``e_ref`` the same metric between the fp32 and the float64 oracle
(torch's own fp32 ``F.ctc_loss`` gradient is that far from float64 on the same input; the factor 4 allows for a different
order of the three-way log-sum-exp and the device's expf/logf).  The bound comes from the oracle alone.

CTC-gradient cases, e_ref (fp32 oracle vs float64 oracle) and the kernel's error vs float64, as printed by the tests:

    case (Tm, Ts; L per utterance)                  e_ref     kernel    bound = max(1e-4, 4 e_ref)
    L1_and_T1      (20, 4;  1, 4, 1)                9.2e-08   3.6e-07   1.0e-04
    L12            (41, 12; 12, 9, 5)               3.8e-06   4.7e-06   1.0e-04
    L127_128_129   (300, 129; 127, 128, 129)        1.6e-04   1.6e-04   6.5e-04
    L256_300       (700, 300; 256, 300, 300, 5)     3.8e-05   3.9e-05   1.5e-04
    L300_T900      (900, 300; 300, 200)             3.4e-03   3.8e-03   1.4e-02
    T < L in a batch     (60, 40; 10, 40, 20)       3.4e-06   4.2e-06   1.0e-04
    key_len 0 in a batch (41, 12; 0, 12, 7)         9.2e-06   7.7e-06   1.0e-04
    chain (648, 128) dq / dk                        1.6e-04 / 7.9e-05   1.3e-04 / 6.9e-05   6.3e-04 / 3.1e-04
    chain (700, 300) dq / dk                        9.0e-04 / 2.8e-04   8.0e-04 / 3.0e-04   3.6e-03 / 1.1e-03

The kernel sits at the fp32 oracle's own distance from float64 everywhere (at most 1.3 x e_ref where e_ref is above the
1e-4 floor), so the factor 4 was never needed.
"""
import numpy as np
import pytest
import torch

from oracle import fs2_oracle as O
from tests.aligner_references import (close, hard_to_idx, make_case, ref_attention, ref_logits, ref_softmax, rel_err)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from fastspeech2_lightning_amd import hip
    hip.lib()
    return hip


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32)


# (B, T1, T2, C, key_lens): the benchmark; a ragged second key tile; the 64/65/129 tile edges; a long text (five key tiles,
# 16-row blocks that end beyond T1); C at both ends (16C + 64(C+1) floats of LDS: 65 216 B at C = 203, exactly 64 KB at
# C = 204, the last size the entry point takes).
# key_lens cover T2, T2 - 1, 65, 64, 2, 1 and one that is shorter than T2 by more than a wavefront (300 -> 64).
DIST_SHAPES = [
    (2, 648, 128, 80, (128, 127)),
    (3, 131, 70, 80, (70, 65, 64)),
    (2, 33, 64, 80, (64, 2)),
    (2, 33, 65, 80, (65, 1)),
    (1, 17, 129, 80, (129,)),
    (2, 700, 300, 80, (300, 64)),
    (1, 16, 9, 4, (9,)),
    (2, 5, 3, 203, (3, 2)),
    (1, 18, 66, 204, (66,)),
]
DIST_IDS = [f"{b}x{t1}x{t2}x{c}" for b, t1, t2, c, _ in DIST_SHAPES]


def _dist_case(B, T1, T2, C, key_lens, scale=3.0):
    q_lens = [T1, max(1, T1 - 5), max(1, T1 // 2)][:B]
    return make_case(B, T1, T2, C, seed=B * 1000 + T1 + T2 + C, key_lens=key_lens, q_lens=q_lens, scale=scale)


@pytest.mark.parametrize("B,T1,T2,C,key_lens", DIST_SHAPES, ids=DIST_IDS)
def test_dist_softmax_shapes(H, B, T1, T2, C, key_lens):
    q, k, key_lens, q_lens, prior = _dist_case(B, T1, T2, C, key_lens)
    logits, lp, soft = ref_attention(q.double(), k.double(), key_lens, prior)
    got = H.attn_dist(q.cuda(), k.cuda())
    close(got, logits, msg="logits")
    glp, gsoft = H.attn_softmax(got, prior.cuda(), key_lens.cuda())
    close(glp, lp, msg="logprob")
    close(gsoft, soft, msg="soft")
    gs = gsoft.cpu()
    for b in range(B):
        L = int(key_lens[b])
        assert bool((gs[b, :, L:] == 0).all()), f"soft beyond key_lens[{b}] = {L} is not exactly 0"
    rows = gs.double().sum(-1)
    assert float((rows - 1).abs().max()) < 2e-5, "a row of soft does not sum to 1"


def test_dist_refuses_channels_beyond_lds(H):
    """16C + 64(C+1) floats of LDS is exactly 64 KB at C = 204 (which runs, see DIST_SHAPES) and 65 856 B at C = 205: the
    entry point refuses that before any launch."""
    assert (16 * 204 + 64 * 205) * 4 == 64 * 1024 < (16 * 205 + 64 * 206) * 4
    q, k = torch.randn(1, 5, 205).cuda(), torch.randn(1, 3, 205).cuda()
    with pytest.raises(RuntimeError, match="attn_dist"):
        H.attn_dist(q, k)


def _ref_hard(soft, key_lens, q_lens):
    """The reference's binarisation (fp32 log, width-1 search per utterance); a one-token text, where its backtrack reads
    column -1, puts every frame on token 0."""
    out = torch.zeros(soft.shape, dtype=soft.dtype)
    for b in range(soft.shape[0]):
        t1, t2 = int(q_lens[b]), int(key_lens[b])
        if t2 == 1:
            out[b, :t1, 0] = 1
        else:
            out[b:b + 1] = O.binarize_attention(soft[b:b + 1, None], key_lens[b:b + 1], q_lens[b:b + 1])[:, 0]
    return out


def _softmax_bwd_case(H, q, k, key_lens, q_lens, prior, mode, w_bin=0.07):
    """Kernel chain dist -> softmax -> softmax_bwd against float64 autograd of (logprob . dlogprob) + w * bin loss, the
    leaf being the kernel's own logits.  hard_idx is the reference's alignment (an input of the kernel under test)."""
    B, T1, T2 = q.shape[0], q.shape[1], k.shape[1]
    glogits = H.attn_dist(q.cuda(), k.cuda())
    glp, gsoft = H.attn_softmax(glogits, prior.cuda(), key_lens.cuda())
    x = glogits.cpu().double().requires_grad_(True)
    lp, soft = ref_softmax(x, key_lens, prior)
    hard = _ref_hard(soft.detach(), key_lens, q_lens)
    idx = hard_to_idx(hard, q_lens)
    dlp = torch.randn(B, T1, T2, generator=torch.Generator().manual_seed(T1 + T2)) * 0.1
    loss = 0.0
    if mode in ("ctc", "both"):
        loss = loss + (lp * dlp.double()).sum()
    if mode in ("bin", "both"):
        loss = loss + O.attention_bin_loss(hard, soft) * w_bin
    loss.backward()
    coef = torch.tensor([-w_bin / float(hard.sum())], dtype=torch.float32).cuda()
    got = H.attn_softmax_bwd(glogits, gsoft, dlp.cuda() if mode != "bin" else None,
                             idx.cuda() if mode != "ctc" else None, coef if mode != "ctc" else None)
    return got, x.grad, soft.detach(), idx, glogits, gsoft, dlp, coef


@pytest.mark.parametrize("mode", ["ctc", "bin", "both"])  # hard_idx=None / dlogprob=None / both upstream gradients
@pytest.mark.parametrize("B,T1,T2,C,key_lens", DIST_SHAPES, ids=DIST_IDS)
def test_softmax_bwd_shapes(H, B, T1, T2, C, key_lens, mode):
    q, k, key_lens, q_lens, prior = _dist_case(B, T1, T2, C, key_lens)
    got, want, *_ = _softmax_bwd_case(H, q, k, key_lens, q_lens, prior, mode)
    print(f"softmax_bwd {B}x{T1}x{T2}x{C} {mode}: err {rel_err(got, want):.3e}")
    close(got, want, msg=f"dlogits ({mode})")


def test_softmax_bwd_clamped_rows(H):
    """Frames whose soft[row, hard] is below the 1e-12 clamp of the binarisation loss: clamp(min=1e-12) has zero slope
    there, so those rows get exactly the gradient of the CTC-only call; the others get both."""
    q, k, key_lens, q_lens, prior = make_case(2, 40, 70, 80, seed=0, scale=30.0)
    got, want, soft, idx, glogits, gsoft, dlp, coef = _softmax_bwd_case(H, q, k, key_lens, q_lens, prior, "both")
    valid = idx >= 0
    ph = torch.gather(soft, 2, idx.clamp(min=0).long()[..., None])[..., 0]
    clamped = valid & (ph < 1e-12)
    n_clamped, n_valid = int(clamped.sum()), int(valid.sum())
    print(f"clamped rows: {n_clamped} of {n_valid}; logits span {float(glogits.max() - glogits.min()):.1f} nats")
    assert 0 < n_clamped < n_valid, "the case must hold frames below the clamp and frames above it"
    # the kernel decides on its own fp32 soft: no frame may sit where fp32 and float64 disagree about the clamp
    gph = torch.gather(gsoft.cpu(), 2, idx.clamp(min=0).long()[..., None])[..., 0]
    assert torch.equal(valid & (gph <= 1e-12), clamped)
    print(f"softmax_bwd clamped case: err {rel_err(got, want):.3e}")
    close(got, want, msg="dlogits")
    ctc_only = H.attn_softmax_bwd(glogits, gsoft, dlp.cuda(), None, None)
    assert torch.equal(got.cpu()[clamped], ctc_only.cpu()[clamped])
    assert not torch.equal(got.cpu()[valid & ~clamped], ctc_only.cpu()[valid & ~clamped])


# ---------------------------------------------------------------------------------------------------------------------
# CTC.  ctc_kernel walks the S = 2L + 1 extended states 256 at a time (`s += 256`), the keys of a row 64 at a time in
# the log-sum-exp (`k += 64`) and 256 at a time in the gradient (`k += 256`).
def _ctc_logprob(B, Tm, Ts, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, Tm, Ts, generator=g) * 2, dim=2)


def _ctc_oracle(lp, key_lens, q_lens, weight, dtype):
    x = lp.detach().to(dtype).requires_grad_(True)
    v = O.attention_ctc_loss(x[:, None], key_lens, q_lens) * weight
    v.backward()
    return v.detach(), x.grad


def _ctc_check(H, name, lp, key_lens, q_lens, weight=0.1):
    v64, g64 = _ctc_oracle(lp, key_lens, q_lens, weight, torch.float64)
    _, g32 = _ctc_oracle(lp, key_lens, q_lens, weight, torch.float32)
    e_ref = rel_err(g32, g64)
    slot = torch.zeros(1, device="cuda")
    d = H.attn_ctc_loss(lp.cuda(), key_lens.cuda(), q_lens.cuda(), weight, slot)
    err = rel_err(d, g64)
    bound = max(1e-4, 4 * e_ref)
    print(f"ctc {name}: value {float(slot):.6f} (float64 {float(v64):.6f}), e_ref {e_ref:.2e}, kernel {err:.2e}, "
          f"bound {bound:.2e}")
    close(slot, v64.reshape(1), 2e-5, f"ctc value ({name})")
    dc = d.cpu()
    assert bool(torch.isfinite(dc).all()), "non-finite CTC gradient"
    assert err < bound, f"ctc grad ({name}): rel err {err:.3e}, e_ref {e_ref:.3e}, bound {bound:.3e}"
    for b in range(lp.shape[0]):  # nothing outside the utterance's own frames and keys
        T, L = int(q_lens[b]), int(key_lens[b])
        assert bool((dc[b, T:] == 0).all()) and bool((dc[b, :, L:] == 0).all()), f"gradient outside utterance {b}"
    return slot, dc, g64


CTC_CASES = {
    # name: (Tm, Ts, key_lens L, query_lens T)
    "L1_and_T1": (20, 4, (1, 4, 1), (20, 7, 1)),                 # S = 3; T = 1 with L = 1; lens far below the extents
    "L12": (41, 12, (12, 9, 5), (41, 30, 12)),
    "L127_128_129": (300, 129, (127, 128, 129), (300, 260, 129)),  # S = 255 / 257 / 259: one pass, two passes; T = L (one path)
    "L256_300": (700, 300, (256, 300, 300, 5), (700, 300, 650, 9)),  # S = 513 / 601: three passes; T = L; a short one in the padding
    "L300_T900": (900, 300, (300, 200), (900, 700)),              # keys: five 64-wide and two 256-wide strides
}


@pytest.mark.parametrize("name", list(CTC_CASES))
def test_ctc_shapes(H, name):
    Tm, Ts, key_lens, q_lens = CTC_CASES[name]
    for L in key_lens:  # which branch: number of 256-thread passes over the states
        print(f"ctc {name}: L {L} -> S {2 * L + 1} -> {(2 * L + 1 + 255) // 256} pass(es)")
    if name == "L127_128_129":
        assert [(2 * L + 1 + 255) // 256 for L in key_lens] == [1, 2, 2]
    if name == "L256_300":
        assert [(2 * L + 1 + 255) // 256 for L in key_lens] == [3, 3, 3, 1]
    _ctc_check(H, name, _ctc_logprob(len(key_lens), Tm, Ts, seed=Tm + Ts), i32(key_lens), i32(q_lens))


def test_ctc_infeasible_utterance_in_batch(H):
    """T < L has no path: zero_infinity makes its value and its gradient rows exactly 0, the batch mean is still over B,
    and the other utterances are what they are without it."""
    Tm, Ts = 60, 40
    lp = _ctc_logprob(3, Tm, Ts, seed=11)
    key_lens, q_lens = i32((10, 40, 20)), i32((60, 30, 50))
    slot, d, g64 = _ctc_check(H, "T<L in batch", lp, key_lens, q_lens)
    assert bool((d[1] == 0).all()) and bool((g64[1] == 0).all())
    keep = [0, 2]
    slot2 = torch.zeros(1, device="cuda")
    d2 = H.attn_ctc_loss(lp[keep].contiguous().cuda(), key_lens[keep].cuda(), q_lens[keep].cuda(), 0.1, slot2)
    close(slot * 3, slot2 * 2, 1e-6, "sum of the feasible utterances")
    close(d[keep] * 3, d2 * 2, 1e-6, "gradient of the feasible utterances")


def test_ctc_empty_text_in_batch(H):
    """key_lens[b] = 0: the kernel leaves early with 0; the oracle agrees (every key class masked -> the blank has
    probability 1 and the empty target costs 0).  Value 0, gradient 0, batch mean still over B."""
    lp = _ctc_logprob(3, 41, 12, seed=12)
    key_lens, q_lens = i32((0, 12, 7)), i32((41, 41, 30))
    v_alone, _ = _ctc_oracle(lp[:1], key_lens[:1], q_lens[:1], 1.0, torch.float64)
    assert float(v_alone) == 0.0
    slot, d, g64 = _ctc_check(H, "key_len 0 in batch", lp, key_lens, q_lens)
    assert bool((d[0] == 0).all()) and bool((g64[0] == 0).all())
    v12, _ = _ctc_oracle(lp[1:], key_lens[1:], q_lens[1:], 0.1, torch.float64)
    close(slot * 3, v12.reshape(1) * 2, 2e-5, "batch mean over B")


def test_ctc_value_only(H):
    """want_grad=False: the same value bit for bit, and no gradient buffer exists to be touched."""
    Tm, Ts, key_lens, q_lens = CTC_CASES["L127_128_129"]
    lp = _ctc_logprob(3, Tm, Ts, seed=Tm + Ts).cuda()
    a, b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    d = H.attn_ctc_loss(lp, i32(key_lens).cuda(), i32(q_lens).cuda(), 0.1, a)
    none = H.attn_ctc_loss(lp, i32(key_lens).cuda(), i32(q_lens).cuda(), 0.1, b, want_grad=False)
    assert d is not None and none is None
    assert torch.equal(a, b) and float(a) > 0


# ---------------------------------------------------------------------------------------------------------------------
# Binarisation loss.  fs2hip_attn_bin_loss launches min(ceil(B*Tm / 256), 256) workgroups of 256 threads, so B*Tm <= 256 is
# one workgroup, 257 two, 20 736 eighty-one, and beyond 65 536 rows the grid-stride loop runs more than once.
@pytest.mark.parametrize("B,Tm,Ts", [(1, 1, 3), (1, 255, 7), (1, 257, 7), (32, 648, 128), (70, 1000, 4)])
def test_bin_loss_shapes(H, B, Tm, Ts):
    nb = min((B * Tm + 255) // 256, 256)
    assert nb == {1: 1, 255: 1, 257: 2, 20736: 81, 70000: 256}[B * Tm]
    assert (B * Tm > nb * 256) == (B * Tm == 70000)  # the grid-stride loop repeats only in the last case
    g = torch.Generator().manual_seed(B * Tm + Ts)
    soft = torch.softmax(torch.randn(B, Tm, Ts, generator=g) * 3, dim=2)
    q_lens = torch.randint(max(1, Tm // 2), Tm + 1, (B,), generator=g)
    q_lens[0] = Tm
    idx = torch.randint(0, Ts, (B, Tm), generator=g).to(torch.int32)
    idx = idx.masked_fill(torch.arange(Tm)[None, :] >= q_lens[:, None], -1)
    valid = (idx >= 0).nonzero()
    # soft is an input of its own: a few selected entries exactly 0 and below the clamp
    for n, v in ((0, 0.0), (len(valid) // 2, 1e-13), (len(valid) - 1, 0.0)) if len(valid) > 2 else ((0, 1e-13),):
        b, t = valid[n].tolist()
        soft[b, t, idx[b, t]] = v
    hard = torch.zeros(B, Tm, Ts, dtype=torch.float64)
    hard.scatter_(2, idx.clamp(min=0).long()[..., None], (idx >= 0).double()[..., None])
    want = O.attention_bin_loss(hard, soft.double()) * 0.07
    slot = torch.zeros(1, device="cuda")
    coef = H.attn_bin_loss(soft.cuda(), idx.cuda(), 0.07, slot)
    close(slot, want.reshape(1), 2e-5, "bin value")
    close(coef, torch.tensor([-0.07 / float(hard.sum())]), 2e-5, "bin coef")


def test_bin_loss_all_padding(H):
    """Every hard_idx -1: value 0 and coef 0, no NaN (the kernel's own contract; the formula is 0/0 there)."""
    soft = torch.softmax(torch.randn(2, 300, 5, generator=torch.Generator().manual_seed(0)), dim=2)
    slot, idx = torch.ones(1, device="cuda"), torch.full((2, 300), -1, dtype=torch.int32)
    coef = H.attn_bin_loss(soft.cuda(), idx.cuda(), 0.07, slot)
    assert float(slot) == 0.0 and float(coef) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# Alignment search.  Launch conditions of fs2hip_mas, restated:
def _mas_dispatch(Tm, Ts):
    wave = Ts <= 128 and Tm * 16 <= 60 * 1024                 # mas_wave_kernel, else mas_kernel
    W = (Ts + 31) // 32
    dirs_in_lds = 2 * Ts * 4 + Tm * W * 4 <= 60 * 1024        # else the direction bits go to dirs_ws in global memory
    return "wave" if wave else ("workgroup/lds" if dirs_in_lds else "workgroup/global")


# name: (Tm, Ts, [(T1, T2) per utterance], kernel).  Inside mas_kernel an utterance with T2 > 256 takes the column loop,
# one with T2 <= 256 the register path -- chosen by its own in_lens[b].
MAS_GROUPS = {
    "Ts64": (200, 64, [(200, 64), (150, 33), (64, 64)], "wave"),
    "Ts65": (200, 65, [(200, 65), (90, 64), (10, 65)], "wave"),
    "Ts128": (648, 128, [(648, 128), (300, 127), (128, 128)], "wave"),
    "Ts129": (300, 129, [(300, 129), (200, 128), (129, 129)], "workgroup/lds"),
    "Ts256": (400, 256, [(400, 256), (300, 255), (256, 256)], "workgroup/lds"),
    "Ts257": (400, 257, [(400, 257), (300, 256), (257, 257)], "workgroup/lds"),
    "Ts300_mixed": (648, 300, [(648, 300), (500, 200), (400, 257)], "workgroup/lds"),
    "Ts520": (600, 520, [(600, 520), (560, 300), (600, 100)], "workgroup/lds"),
    "Tm2000_Ts300": (2000, 300, [(2000, 300), (1500, 200)], "workgroup/global"),
    "Tm3900_Ts100": (3900, 100, [(3900, 100), (1000, 64)], "workgroup/global"),  # <= 128 tokens, yet Tm * 16 B > 60 KB
    "ragged_wave": (300, 128, [(300, 128), (50, 120), (1, 30), (90, 2), (0, 50), (5, 128)], "wave"),
    "ragged_workgroup": (300, 300, [(300, 300), (50, 120), (1, 30), (90, 2), (0, 50), (5, 300), (1, 290)], "workgroup/lds"),
}
PAD = 3.0  # what the padding holds: log 3 > 0 would attract the search if a kernel ever read it


def _mas_reference(c):
    if c.shape[0] == 0:
        return np.zeros_like(c)
    return O.mas_width1(c.copy())


def _mas_run_and_check(H, Tm, Ts, cases, refs, is_log, pad):
    x = torch.full((len(cases), Tm, Ts), pad)
    for n, c in enumerate(cases):
        x[n, : c.shape[0], : c.shape[1]] = torch.tensor(c)
    in_lens, out_lens = i32(c.shape[1] for c in cases), i32(c.shape[0] for c in cases)
    hard, idx, dur = H.mas(x.cuda(), in_lens.cuda(), out_lens.cuda(), is_log=is_log)
    hard, idx, dur = hard.cpu().numpy(), idx.cpu().numpy(), dur.cpu().numpy()
    for n, (c, ref) in enumerate(zip(cases, refs)):
        t1, t2 = c.shape
        np.testing.assert_array_equal(hard[n, :t1, :t2], ref, err_msg=f"utterance {n} ({t1} x {t2})")
        assert hard[n].sum() == t1, f"utterance {n}: ones outside its own frames and tokens"
        np.testing.assert_array_equal(dur[n, :t2], ref.sum(0).astype(np.int32))
        assert (dur[n, t2:] == 0).all()
        if t1:
            np.testing.assert_array_equal(idx[n, :t1], ref.argmax(1))
        assert (idx[n, t1:] == -1).all()


@pytest.mark.parametrize("name", list(MAS_GROUPS))
def test_mas_branches(H, name):
    Tm, Ts, shapes, kernel = MAS_GROUPS[name]
    assert _mas_dispatch(Tm, Ts) == kernel, "the dispatch thresholds of fs2hip_mas moved: this group lost its branch"
    if kernel != "wave":
        loops = [t2 > 256 for _, t2 in shapes]  # column loop / register path, per utterance
        assert any(loops) == (Ts > 256) and not all(loops)  # past 256 tokens a launch mixes both paths
        print(f"mas {name}: column-loop utterances {loops}")
    rng = np.random.default_rng(Tm * 1000 + Ts)
    rand, ties = [], []
    for t1, t2 in shapes:
        x = rng.standard_normal((t1, t2)).astype(np.float32)
        x = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
        rand.append(x)
        ties.append(np.round(x).astype(np.float32))  # tie-heavy
    for cases in (rand, ties):
        _mas_run_and_check(H, Tm, Ts, cases, [_mas_reference(c) for c in cases], True, PAD)


@pytest.mark.parametrize("name", ["Ts128", "Ts300_mixed", "ragged_workgroup"])
def test_mas_takes_the_logarithm_itself(H, name):
    """is_log=False: inputs 2 ** -k, whose logarithm -k ln 2 is exact (correctly rounded) on any correct logf, so the
    search must agree bit for bit with the reference run on the host's logarithm; small integers k make it tie-heavy."""
    Tm, Ts, shapes, kernel = MAS_GROUPS[name]
    assert _mas_dispatch(Tm, Ts) == kernel
    rng = np.random.default_rng(Tm + Ts)
    cases = [(2.0 ** -rng.integers(0, 13, (t1, t2))).astype(np.float32) for t1, t2 in shapes]
    refs = [_mas_reference(np.log(c.astype(np.float64)).astype(np.float32)) for c in cases]
    _mas_run_and_check(H, Tm, Ts, cases, refs, False, PAD)


@pytest.mark.parametrize("Ts", [64, 200])  # wave kernel / workgroup kernel
def test_mas_single_token(H, Ts):
    """T2 = 1 is outside the bit-exact set (the reference's backtrack reads column -1 there): every frame on token 0."""
    assert _mas_dispatch(50, Ts) == ("wave" if Ts == 64 else "workgroup/lds")
    x = torch.log_softmax(torch.randn(2, 50, Ts, generator=torch.Generator().manual_seed(Ts)), dim=2)
    hard, idx, dur = H.mas(x.cuda(), i32((1, Ts)).cuda(), i32((20, 50)).cuda(), is_log=True)
    hard, idx, dur = hard.cpu(), idx.cpu(), dur.cpu()
    assert bool((idx[0, :20] == 0).all()) and bool((idx[0, 20:] == -1).all())
    assert bool((hard[0, :20, 0] == 1).all()) and float(hard[0].sum()) == 20
    assert int(dur[0, 0]) == 20 and int(dur[0].sum()) == 20
    assert float(hard[1].sum()) == 50 and int(dur[1].sum()) == 50


# ---------------------------------------------------------------------------------------------------------------------
# avg_variance: one thread per (utterance, token), 256 per workgroup -> B*Ts = 5 / 256 one workgroup, 257 two, 4 096 sixteen.
@pytest.mark.parametrize("B,Tm,Ts", [(1, 50, 5), (2, 648, 128), (1, 300, 257), (32, 648, 128)])
def test_avg_variance_shapes(H, B, Tm, Ts):
    assert (B * Ts + 255) // 256 == {5: 1, 256: 1, 257: 2, 4096: 16}[B * Ts]
    g = torch.Generator().manual_seed(B * Ts + Tm)
    var = torch.randn(B, Tm, generator=g)
    var[torch.rand(B, Tm, generator=g) < 0.3] = 0.0  # frames equal to exactly 0 are not counted
    mean = 2.0 * Tm / Ts  # totals straddle Tm: about a third of the frames' sum lands above it
    durs = torch.randint(0, int(2 * mean) + 2, (B, Ts), generator=g)
    durs[torch.rand(B, Ts, generator=g) < 0.3] = 0  # runs of zero-length tokens
    durs[:, 0] = 0
    durs[:, -1] = 0
    if B > 1:
        durs[1] = durs[1] // 4  # total below Tm
        durs[1, -1] = 3
        durs[1, 0] = 2
    durs[0, 1] += Tm // 2
    totals = durs.sum(1)
    assert bool((totals > Tm).any()) and (B == 1 or bool((totals < Tm).any()))
    cum = durs.cumsum(1).to(torch.int32)
    # frames beyond Tm do not exist: the reference sees the durations cut off at Tm
    ends = durs.cumsum(1).clamp(max=Tm)
    cut = torch.diff(ends, dim=1, prepend=torch.zeros(B, 1, dtype=ends.dtype))
    want = O.average_variance(var.double(), cut)
    got = H.avg_variance(var.cuda(), cum.cuda())
    close(got, want, 2e-5, "avg_variance")
    assert bool((got.cpu()[cut == 0] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T1,T2,C", [(2, 648, 128, 80), (2, 700, 300, 80)])
def test_aligner_chain_full_size(H, B, T1, T2, C):
    """dist -> softmax -> MAS -> CTC + bin -> softmax_bwd -> dist_bwd at the benchmark shape and at a long text against
    float64 autograd.  (648, 128): wave MAS kernel, two passes over the S = 257 CTC states, two key tiles; (700, 300):
    column loop of mas_kernel, three passes over the S = 601 CTC states, five key tiles."""
    q, k, key_lens, q_lens, prior = make_case(B, T1, T2, C, seed=T1 + T2, key_lens=(T2, T2 - 7), q_lens=(T1, T1 - 40))
    w_ctc, w_bin = 0.1, 0.07

    def oracle(dtype, hard=None):
        qr, kr = q.clone().to(dtype).requires_grad_(True), k.clone().to(dtype).requires_grad_(True)
        logits, lp, soft = ref_attention(qr, kr, key_lens, prior)
        if hard is None:
            hard = O.binarize_attention(soft.detach()[:, None], key_lens, q_lens)[:, 0]
        ctc = O.attention_ctc_loss(lp[:, None], key_lens, q_lens) * w_ctc
        binl = O.attention_bin_loss(hard.to(dtype), soft) * w_bin
        (ctc + binl).backward()
        return hard, ctc.detach(), binl.detach(), qr.grad, kr.grad

    hard, ctc, binl, dq64, dk64 = oracle(torch.float64)
    _, _, _, dq32, dk32 = oracle(torch.float32, hard)
    glogits = H.attn_dist(q.cuda(), k.cuda())
    glp, gsoft = H.attn_softmax(glogits, prior.cuda(), key_lens.cuda())
    ghard, gidx, gdur = H.mas(gsoft, key_lens.cuda(), q_lens.cuda())
    assert torch.equal(ghard.cpu().double(), hard.double()), "hard map differs from the reference's search"
    assert torch.equal(gidx.cpu(), hard_to_idx(hard, q_lens))
    slots = torch.zeros(2, device="cuda")
    dlp = H.attn_ctc_loss(glp, key_lens.cuda(), q_lens.cuda(), w_ctc, slots[0:1])
    coef = H.attn_bin_loss(gsoft, gidx, w_bin, slots[1:2])
    close(slots[0:1], ctc.reshape(1), 2e-5, "ctc value")
    close(slots[1:2], binl.reshape(1), 2e-5, "bin value")
    dlogits = H.attn_softmax_bwd(glogits, gsoft, dlp, gidx, coef)
    dq, dk = H.attn_dist_bwd(dlogits, q.cuda(), k.cuda())
    for name, got, w64, w32 in (("dq", dq, dq64, dq32), ("dk", dk, dk64, dk32)):
        e_ref, err = rel_err(w32, w64), rel_err(got, w64)
        bound = max(1e-4, 4 * e_ref)
        print(f"chain {T1}x{T2} {name}: e_ref {e_ref:.2e}, kernel {err:.2e}, bound {bound:.2e}")
        assert bool(torch.isfinite(got).all()) and err < bound, f"{name}: rel err {err:.3e}, bound {bound:.3e}"
