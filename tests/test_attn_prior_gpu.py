"""GPU: the aligner's attention prior computed from the lengths (``fs2hip_attn_prior``, ``hip.attn_prior``) and the
learned-alignment step that runs without a prior in its batch.

Kernel: the yardstick is the project's own definition, ``synthetic.beta_binomial_prior`` (scipy's ``betabinom`` in fp64,
cast to fp32).  What the aligner consumes is ``log(prior + 1e-8)``: the two sides may differ there by two fp32 ulps
relative (2.4e-7: each side rounds to fp32 once); the probabilities themselves by 2^-22 relative down to 1e-30, below
which only "tiny" is asked (whether fp32 subnormals survive the conversion is left open: nothing downstream sees them).
Padding -- rows beyond the utterance's frames, keys beyond its tokens -- is exact zero in a buffer that held NaN.

Model: a batch with ``duration = None`` computes the prior inside the step, so it must give bit for bit what the same
model gives when ``hip.attn_prior``'s tensor is fed as the batch's prior, match the scipy-fed model within the project's
loss bound, and record / replay like every other launch, bucketed geometries included."""
import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import hip as H
from fastspeech2_lightning_amd.synthetic import beta_binomial_prior
from tests.test_plan_gpu import assert_same_state, batches, build, run

pytestmark = pytest.mark.gpu

#: n = 0; a one-token text under several frames; more keys than frames; a key count past one 64-lane stride; an empty
#: utterance -- in a geometry larger than every utterance, as a bucket gives
SMALL = [(1, 1), (5, 1), (3, 7), (70, 13), (130, 67), (0, 4)]
SMALL_GEO = (136, 72)
LONG = [(1291, 200)]   # the GST configuration's extent
_REF = {}


def reference(lens, Tm, Ts, scaling=1.0):
    """``synthetic.beta_binomial_prior`` utterance by utterance (an empty one stays zero), computed once per case."""
    key = (tuple(lens), Tm, Ts, scaling)
    if key not in _REF:
        out = torch.zeros(len(lens), Tm, Ts)
        for b, (m, p) in enumerate(lens):
            if m > 0 and p > 0:
                out[b, :m, :p] = beta_binomial_prior(torch.tensor([m]), torch.tensor([p]), m, p, scaling)[0]
        _REF[key] = out
    return _REF[key]


def gpu_prior(lens, Tm, Ts, scaling=1.0):
    mel = torch.tensor([m for m, _ in lens], dtype=torch.int32, device="cuda")
    src = torch.tensor([p for _, p in lens], dtype=torch.int32, device="cuda")
    out = torch.full((len(lens), Tm, Ts), float("nan"), device="cuda")
    got = H.attn_prior(mel, src, Tm, Ts, scaling, out=out)
    assert got is out
    torch.cuda.synchronize()
    return out.cpu()


def check(lens, Tm, Ts, scaling=1.0):
    ref, got = reference(lens, Tm, Ts, scaling), gpu_prior(lens, Tm, Ts, scaling)
    assert not torch.isnan(got).any()
    valid = torch.zeros(len(lens), Tm, Ts, dtype=torch.bool)
    for b, (m, p) in enumerate(lens):
        valid[b, :min(m, Tm), :min(p, Ts)] = True
    assert (got[~valid] == 0.0).all() and (ref[~valid] == 0.0).all()
    g, r = got.double().numpy(), ref.double().numpy()
    dlog = np.abs(np.log(g + 1e-8) - np.log(r + 1e-8)).max()
    big = r >= 1e-30
    rel = (np.abs(g[big] - r[big]) / r[big]).max()
    tiny = g[~big].max() if (~big).any() else 0.0
    rows = valid.any(-1).numpy()
    sums = np.abs(g.sum(-1)[rows] - 1.0).max()
    print(f"{lens[-1]} in {(Tm, Ts)} scaling {scaling}: |d log(p + 1e-8)| {dlog:.3e}, relative {rel:.3e} "
          f"(2^-22 = {2.0 ** -22:.3e}), largest below 1e-30 {tiny:.3e}, |row sum - 1| {sums:.3e}")
    assert dlog <= 2.4e-7
    assert rel <= 2.0 ** -22
    assert tiny <= 2e-30
    assert sums <= 1e-6
    for b, (m, p) in enumerate(lens):
        if p == 1 and m > 0:
            assert (got[b, :m, 0] == 1.0).all()   # one token: every frame's whole mass
    return got


@pytest.mark.parametrize("scaling", [1.0, 0.5])
def test_small_ragged_batch_in_a_larger_geometry(scaling):
    check(SMALL, *SMALL_GEO, scaling=scaling)


def test_one_long_utterance():
    check(LONG, *LONG[0])


@pytest.mark.parametrize("form", ["0", "1"], ids=["in_place", "k_table"])
def test_the_forms_without_the_whole_number_table_give_the_same_bits(monkeypatch, form):
    """``scaling = 1`` takes every lgamma from a table of ``lgamma(j + 1)``; ``FS2_ATTN_PRIOR_TABLE`` = 0 / 1 selects the forms
    every other scaling -- or a geometry too long for the table -- takes: all lgamma calls in place / a table of the
    ``k``-only terms.  The same values summed in the same order: the same bits, and so the same bounds."""
    default = check(SMALL, *SMALL_GEO)
    default_long = gpu_prior(LONG, *LONG[0])
    monkeypatch.setenv("FS2_ATTN_PRIOR_TABLE", form)
    assert torch.equal(check(SMALL, *SMALL_GEO), default)
    assert torch.equal(gpu_prior(LONG, *LONG[0]), default_long)


def test_lengths_beyond_the_geometry_are_clamped():
    Tm, Ts = SMALL_GEO
    got = gpu_prior([(200, 67), (130, 100), (-3, 5), (7, -1)], Tm, Ts)
    want = gpu_prior([(Tm, 67), (130, Ts), (0, 5), (7, 0)], Tm, Ts)
    assert not torch.isnan(got).any() and torch.equal(got, want)
    assert (got[2:] == 0.0).all() and float(got[0, Tm - 1].sum()) > 0.99


def test_argument_errors():
    mel = torch.tensor([5, 3], dtype=torch.int32, device="cuda")
    src = torch.tensor([2, 3], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.attn_prior(mel.cpu(), src, 8, 4)
    with pytest.raises(TypeError, match="int32"):
        H.attn_prior(mel.long(), src, 8, 4)
    with pytest.raises(ValueError, match="text lengths"):
        H.attn_prior(mel, src[:1], 8, 4)
    with pytest.raises(ValueError, match="scaling"):
        H.attn_prior(mel, src, 8, 4, scaling=0.0)
    with pytest.raises(ValueError, match="geometry"):
        H.attn_prior(mel, src, 0, 4)
    with pytest.raises(ValueError, match="out is"):
        H.attn_prior(mel, src, 8, 4, out=torch.empty(2, 8, 5, device="cuda"))
    # the entry point itself: nothing is enqueued on bad arguments
    out = torch.full((2, 8, 4), float("nan"), device="cuda")
    raw = H.real_lib().fs2hip_attn_prior
    s = H._stream()
    assert raw(mel.data_ptr(), src.data_ptr(), out.data_ptr(), 2, 8, 4, 0.0, s) == -22
    assert raw(mel.data_ptr(), src.data_ptr(), out.data_ptr(), 2, 8, 4, -1.0, s) == -22
    assert raw(None, src.data_ptr(), out.data_ptr(), 2, 8, 4, 1.0, s) == -22
    assert raw(mel.data_ptr(), None, out.data_ptr(), 2, 8, 4, 1.0, s) == -22
    assert raw(mel.data_ptr(), src.data_ptr(), None, 2, 8, 4, 1.0, s) == -22
    for bad in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (-1, 8, 4)):
        assert raw(mel.data_ptr(), src.data_ptr(), out.data_ptr(), *bad, 1.0, s) == -22
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
def la_batches(config, n):
    """Learned-alignment batches of one geometry (``tests/test_plan_gpu.py``'s), their scipy prior in ``duration``."""
    return batches(config, n, learn_alignment=True)


def without_prior(b):
    return dict(b, duration=None)


def device_prior(b):
    mel_lens, src_lens = b["mel_lens"].cuda(), b["src_lens"].cuda()
    return H.attn_prior(mel_lens, src_lens, int(b["max_mel_len"]), int(b["max_src_len"]))


def one_step(model, batch):
    with torch.no_grad():
        model.training_step(batch)
    torch.cuda.synchronize()
    return model._loss_slots.clone(), dict(model.last_output), model.store.grad.clone()


def test_a_step_without_a_prior_equals_the_step_fed_the_kernels_prior_and_matches_scipys():
    computed, _, config = build(learn_alignment=True)
    fed, _, _ = build(learn_alignment=True)
    scipy_fed, _, _ = build(learn_alignment=True)
    b = la_batches(config, 1)[0]
    assert b["duration"].dim() == 3
    slots_c, out_c, grad_c = one_step(computed, without_prior(b))
    slots_f, out_f, grad_f = one_step(fed, dict(b, duration=device_prior(b)))
    assert torch.isfinite(slots_c).all() and torch.equal(slots_c, slots_f)
    assert len(out_c) == 16 and set(out_c) == set(out_f)
    for k, v in out_c.items():
        assert (v is None) == (out_f[k] is None), k
        if v is not None:
            assert torch.equal(v, out_f[k]), k
    assert out_c["attn_logprob"] is not None and torch.isfinite(out_c["attn_soft"]).all()
    assert torch.equal(grad_c, grad_f) and float(grad_c.abs().max()) > 0
    one_step(scipy_fed, dict(b))
    got, want = computed.losses_to_host(), scipy_fed.losses_to_host()
    assert set(got) == set(want) and {"attn_ctc", "attn_bin"} <= set(got)
    for k, v in want.items():
        print(f"loss {k}: computed prior {got[k]:.8f}, scipy prior {v:.8f}")
        assert abs(got[k] - v) <= 1e-4 * max(1.0, abs(v)), k


def test_list_of_none_as_collate_leaves_it_is_no_prior_either():
    computed, _, config = build(learn_alignment=True)
    listed, _, _ = build(learn_alignment=True)
    b = la_batches(config, 1)[0]
    a = one_step(computed, without_prior(b))
    c = one_step(listed, dict(b, duration=[None] * b["text"].shape[0]))
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])


def test_replayed_steps_without_a_prior_equal_eager_ones():
    eager, opt_e, config = build(plan=False, learn_alignment=True)
    planned, opt_p, _ = build(plan=True, learn_alignment=True)
    bs = [without_prior(b) for b in la_batches(config, 4)]
    want = run(eager, opt_e, bs)
    got = run(planned, opt_p, bs)
    p = planned.plans
    assert (p.eager, p.recorded, p.replayed) == (1, 1, 2) and eager.plans.recorded == 0   # the fourth step is a replay
    for i, (w, g) in enumerate(zip(want, got)):
        assert torch.isfinite(w).all() and torch.equal(w, g), (i, w.tolist(), g.tolist())
    assert_same_state(eager, planned)
    (plan,) = p.plans.values()
    assert "duration" not in plan.inputs and {"text", "mel", "mel_lens", "src_lens"} <= set(plan.inputs)
    assert H.real_lib().fs2hip_plan_op_id(b"fs2hip_attn_prior") >= 0


def test_a_bucketed_batch_without_a_prior_records_and_replays_like_the_eager_padded_step():
    eager, opt_e, config = build(plan=False, learn_alignment=True)
    planned, opt_p, _ = build(plan=True, learn_alignment=True)
    bs = [without_prior(b) for b in la_batches(config, 4)]
    Ts_b, Tm_b = int(bs[0]["max_src_len"]) + 5, int(bs[0]["max_mel_len"]) + 9
    padded = [eager.pad_batch(b, Ts_b, Tm_b) for b in bs]
    assert padded[0]["duration"] is None and padded[0]["mel"].shape[1] == Tm_b and padded[0]["text"].shape[1] == Ts_b
    want = run(eager, opt_e, padded)
    got = run(planned, opt_p, [dict(b, bucket_geometry=(Ts_b, Tm_b)) for b in bs])
    p = planned.plans
    assert (p.eager, p.recorded, p.replayed) == (1, 1, 2)
    for i, (w, g) in enumerate(zip(want, got)):
        assert torch.isfinite(w).all() and torch.equal(w, g), (i, w.tolist(), g.tolist())
    assert_same_state(eager, planned)
    (plan,) = p.plans.values()
    assert "duration" not in plan.inputs and plan.inputs["mel"].shape[1] == Tm_b
    assert planned.last_output["attn_soft"].shape[-2:] == (Tm_b, Ts_b)
