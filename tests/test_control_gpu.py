"""GPU: per-utterance and per-token inference control (a tensor in ``InferenceControl.pitch / energy / duration``,
which the reference multiplies in by plain broadcasting, fs2/variance_adaptor.py:203, :360-366).  The two kernels that
read the control from device memory against torch on the CPU, bit for bit; a constant tensor against the float path;
non-constant per-token controls against the CPU oracle.  Fresh allocations are poisoned with NaN throughout."""
import re

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import plan as PL
from fastspeech2_lightning_amd.config import InferenceControl, Stats, VarianceLevelEnum
from oracle import cases as C
from oracle import fs2_oracle as O
from tests.test_headdim_model_gpu import N_SYMBOLS, config_for

pytestmark = pytest.mark.gpu
EINVAL = -22


@pytest.fixture(autouse=True)
def poisoned_allocations():
    """``torch.empty`` / ``empty_like`` come back NaN-filled (tests/conftest.py's hunting mode, always on in this file):
    an output element a kernel did not write shows as NaN."""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned(t):
        if t.is_cuda and t.is_floating_point() and t.numel():
            t.fill_(float("nan"))
        return t
    torch.empty = lambda *a, **k: poisoned(real_empty(*a, **k))
    torch.empty_like = lambda *a, **k: poisoned(real_empty_like(*a, **k))
    allow, PL.GUARD_ALLOW = PL.GUARD_ALLOW, PL.GUARD_ALLOW | {"fill_"}
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like
        PL.GUARD_ALLOW = allow


@pytest.fixture(scope="module")
def H():
    from fastspeech2_lightning_amd import hip
    return hip


# ----------------------------------------------------------------------------------------------------------------------
# fs2hip_bucket_embed_add_ctl
# ----------------------------------------------------------------------------------------------------------------------
B_, T_, TS_ = 3, 7, 4  # M = 21 rows: not a multiple of the 4 rows per workgroup


def bucket_case(D, NB, form):
    g = torch.Generator().manual_seed(1000 * D + 10 * NB + len(form))
    bins = torch.linspace(-3, 3, NB) if NB > 1 else torch.tensor([0.25])
    W, x = torch.randn(NB + 1, D, generator=g), torch.randn(B_, T_, D, generator=g)
    val = 4 * torch.randn(B_, T_, generator=g)
    src = None
    if form == "token":
        ctl = torch.empty(B_, T_).uniform_(-2, 2, generator=g)
        ctl[0, :4] = torch.tensor([0.0, 1.0, -1.5, 1.0])
        full = ctl
    elif form == "utterance":
        ctl = torch.tensor([0.0, 1.0, -1.5])
        full = ctl[:, None].expand(B_, T_)
    else:  # a [B, Ts] control through the length regulator's source index: repeated tokens, -1 past the end
        ctl = torch.empty(B_, TS_).uniform_(-2, 2, generator=g)
        ctl[0] = torch.tensor([0.0, 1.0, -1.5, 1.0])
        ctl[1, 1] = 1.0
        src = torch.tensor([[0, 0, 1, 1, 2, 3, 3], [1, 1, 1, 0, 3, -1, -1], [2, 2, 2, 2, -1, -1, -1]], dtype=torch.int32)
        full = torch.where(src < 0, torch.ones(()), ctl.gather(1, src.clamp(min=0).long()))
    # values exactly on edges (control 1 there), below the first edge and above the last
    edges = [bins[0], bins[-1], bins[NB // 2]]
    for k, e in enumerate(edges):
        val[1, k] = e
        if form == "token":
            ctl[1, k] = 1.0
    val[2, 0], val[2, 1] = -100.0, 100.0
    return val, ctl, src, full.contiguous(), bins, W, x


@pytest.mark.parametrize("form", ["token", "utterance", "source"])
@pytest.mark.parametrize("NB", [1, 5, 255])
@pytest.mark.parametrize("D", [8, 260])
def test_bucket_embed_add_ctl_matches_torch(H, D, NB, form):
    val, ctl, src, full, bins, W, x = bucket_case(D, NB, form)
    assert (full[1, :3] == 1.0).all()  # row 1's edge values meet control 1
    want_scaled = val * full  # one fp32 multiply, as in the reference
    want_idx = torch.bucketize(want_scaled, bins)
    want_out = x + W[want_idx]
    assert {0, NB} <= set(want_idx.flatten().tolist())  # below the first edge and above the last both occur
    assert (want_scaled[1, :3] == torch.stack([bins[0], bins[-1], bins[NB // 2]])).all()  # exactly on edges
    assert (full == 0).any() and (full == 1).any() and (full < 0).any()
    out, idx, scaled = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), ctl.cuda(),
                                          ctl_idx=None if src is None else src.cuda(), scaled=True)
    assert torch.equal(idx.cpu(), want_idx.int())
    assert torch.equal(scaled.cpu(), want_scaled)
    assert torch.equal(out.cpu(), want_out)
    out2, idx2 = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), ctl.cuda(),
                                    ctl_idx=None if src is None else src.cuda())  # the scaled output is optional
    assert torch.equal(out2, out) and torch.equal(idx2, idx)


def test_bucket_embed_add_ctl_one_value_equals_the_float(H):
    val, _, _, _, bins, W, x = bucket_case(260, 5, "token")
    a = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), 0.75)
    b = H.bucket_embed_add(val.cuda(), bins.cuda(), W.cuda(), x.cuda(), torch.tensor(0.75).cuda())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------------------
# fs2hip_duration_round_ctl
# ----------------------------------------------------------------------------------------------------------------------
def duration_case(B, T, n_ctl):
    g = torch.Generator().manual_seed(B * 1000 + T)
    k = torch.randint(0, 31, (B, T), generator=g).double()
    frac = torch.empty(B, T, dtype=torch.float64).uniform_(-0.4, 0.4, generator=g)
    logd = torch.log(1 + k + frac).float()
    logd.view(-1)[0] = -50.0  # exp(logd) - 1 = -1: clamped to 0 whatever the control
    if B * T > 2:
        logd.view(-1)[1] = -0.1
    ctl = torch.randint(0, 33, (n_ctl,), generator=g).float() / 8
    if n_ctl > 2:
        ctl[1], ctl[2] = 0.0, 4.0
    return logd, ctl


@pytest.mark.parametrize("B,T,n_ctl", [(1, 1, 1), (1, 257, 257), (1, 257, 1), (3, 5, 3), (3, 5, 15)])
def test_duration_round_ctl_matches_cpu_formula(H, B, T, n_ctl):
    logd, ctl = duration_case(B, T, n_ctl)
    # the fixture is well-posed: exp(logd) - 1 at least 1e-3 from every half-integer (two fp32 exponentials may differ
    # by an ulp), controls multiples of 1/8 in [0, 4] (the product with an integer below 2^20 is exact)
    e = torch.exp(logd.double()) - 1
    assert float(((e - 0.5) - torch.round(e - 0.5)).abs().min()) >= 1e-3
    assert torch.equal(ctl * 8, torch.round(ctl * 8)) and float(ctl.min()) >= 0 and float(ctl.max()) <= 4
    full = ctl.repeat_interleave(B * T // n_ctl).view(B, T)
    want = torch.clamp(torch.round(torch.exp(logd) - 1) * full, min=0).int()
    assert int(want.view(-1)[0]) == 0
    if n_ctl > 2:
        assert int(want.max()) > 4 and (full == 0).any()
    got = H.duration_round(logd.cuda(), ctl.cuda().view(B, -1) if n_ctl == B * T else ctl.cuda())
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------------------------------------------------
# rejected arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_return_einval(H):
    M, D, NB, T = 8, 8, 5, 4
    f = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    val, ctl, bins, W, x, out, sc = f(M), f(M), f(NB), f(NB + 1, D), f(M, D), f(M, D), f(M)
    idx, src = torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    L, s = H.lib(), H._stream()

    def bucket(ctl=ctl, div=1, src=None, ctl_T=0, M=M, D=D):
        return L.fs2hip_bucket_embed_add_ctl(p(val), p(ctl), div, p(src), ctl_T, p(bins), NB, p(W), p(x), p(out), p(idx),
                                             p(sc), M, D, s)
    assert bucket() == 0 and bucket(div=T) == 0 and bucket(div=T, src=src, ctl_T=2) == 0  # the accepted forms
    assert bucket(ctl=None) == EINVAL
    assert bucket(div=0) == EINVAL and bucket(div=-1) == EINVAL
    assert bucket(div=3) == EINVAL  # M % ctl_div != 0
    assert bucket(D=6) == EINVAL  # D % 4 != 0
    assert bucket(div=T, src=src, ctl_T=0) == EINVAL and bucket(div=T, src=src, ctl_T=-1) == EINVAL

    dur = torch.zeros(M, dtype=torch.int32, device="cuda")

    def rnd(ctl=ctl, div=1, n=M):
        return L.fs2hip_duration_round_ctl(p(val), p(ctl), div, p(dur), n, s)
    assert rnd() == 0 and rnd(div=T) == 0
    assert rnd(ctl=None) == EINVAL
    assert rnd(div=0) == EINVAL and rnd(div=-2) == EINVAL
    assert rnd(div=3) == EINVAL
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="1, B or B \\* T"):
        H.duration_round(f(2, 6), f(5))
    with pytest.raises(ValueError, match="1, B or B \\* T"):
        H.bucket_embed_add(f(2, 4), bins, W, f(2, 4, D), f(3))


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
#: the seeds of the per-token controls: chosen so that the fixture is well-posed (``assert_well_posed``)
CONTROL_SEED = {"phone": 0, "frame": 152}


def build_pair(level):
    from fastspeech2_lightning_amd.model import FastSpeech2
    config = config_for(32, 2)
    config.model.variance_predictors.energy.level = VarianceLevelEnum(level)
    config.model.variance_predictors.pitch.level = VarianceLevelEnum(level)
    model = FastSpeech2(config, Stats(**C.STATS))
    oracle = O.FastSpeech2Oracle(config, Stats(**C.STATS), n_symbols=N_SYMBOLS)
    sd = O.seeded_state_dict(oracle.state_dict())
    sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([1.2])  # a useful spread of durations
    oracle.load_state_dict(sd)
    model.load_state_dict(sd)
    model.eval(); oracle.eval()
    return model, oracle


def train_batch(level="phone"):
    return O.synthetic_batch(B=2, ts_lo=6, ts_hi=12, n_symbols=N_SYMBOLS, n_mels=80, seed=7, dur_hi=5,
                             frame_level=level == "frame")


def infer_batch():
    infer = {k: v for k, v in train_batch().items() if k not in ("mel", "pitch", "energy", "duration")}
    infer.update(mel=None, mel_lens=None, max_mel_len=1_000_000, duration=None)
    return infer


def per_token_controls(seed, B, Ts):
    """Non-constant [B, Ts] controls: pitch and energy in [0.5, 2], duration multiples of 1/8 in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    pitch = torch.empty(B, Ts).uniform_(0.5, 2.0, generator=g)
    energy = torch.empty(B, Ts).uniform_(0.5, 2.0, generator=g)
    duration = torch.randint(4, 17, (B, Ts), generator=g).float() / 8
    return pitch, energy, duration


def oracle_reference(oracle, level, pitch, energy, duration):
    """The oracle's output for per-token controls and its rounded durations.  A frame-level predictor gets the [B, Tm]
    tensor: the [B, Ts] control gathered with the oracle's own durations (which do not depend on pitch / energy there)."""
    infer = infer_batch()
    with torch.no_grad():
        if level == "frame":
            first = oracle(dict(infer), InferenceControl(duration=duration), inference=True)
            dur = torch.clamp(torch.round(torch.exp(first["duration_prediction"]) - 1) * duration, min=0).long()
            Tm = int(dur.sum(1).max())
            spread = lambda c: torch.stack([  # noqa: E731
                torch.cat([c[b].repeat_interleave(dur[b]), torch.ones(Tm - int(dur[b].sum()))]) for b in range(len(c))])
            pitch, energy = spread(pitch), spread(energy)
        ref = oracle(dict(infer), InferenceControl(pitch=pitch, energy=energy, duration=duration), inference=True)
    dur = torch.clamp(torch.round(torch.exp(ref["duration_prediction"]) - 1) * duration, min=0).int()
    assert torch.equal(dur.sum(1).int(), ref["tgt_lens"].int())
    return ref, dur


def well_posed_margins(ref, duration, level):
    """(smallest relative distance of a scaled prediction of the oracle from a bin edge, smallest distance of
    exp(logd) - 1 from a half-integer), over the valid positions."""
    bins = torch.linspace(C.STATS["pitch"]["norm_min"], C.STATS["pitch"]["norm_max"], 255).double()
    mask = ref["tgt_mask"] if level == "frame" else ref["src_mask"]
    edge = float("inf")
    for k in ("pitch_prediction", "energy_prediction"):
        p = ref[k][mask].double()
        d = (p[:, None] - bins[None, :]).abs().min(1).values / p.abs().clamp(min=1.0)
        edge = min(edge, float(d.min()))
    e = (torch.exp(ref["duration_prediction"].double()) - 1)[ref["src_mask"]]
    tie = float(((e - 0.5) - torch.round(e - 0.5)).abs().min())
    return edge, tie


def run_model(model, control):
    """(output dict, rounded durations) of a free-inference forward."""
    va, seen = model.variance_adaptor, {}
    real = va.fwd

    def spy(*a, **k):
        out, ctx = real(*a, **k)
        seen.update(out)
        return out, ctx
    va.fwd = spy
    try:
        out = model(infer_batch(), control, inference=True)
    finally:
        del va.fwd
    return out, seen["duration_rounded"]


@pytest.fixture(scope="module", params=["phone", "frame"])
def case(request):
    """One model / oracle pair per predictor level."""
    return (request.param,) + build_pair(request.param)


_FLOAT_PATH = {}


def float_path(level, model):
    """The float path's output and durations: computed once (inside a test, under the suite's fixed GEMM tiles) and left
    unchanged."""
    if level not in _FLOAT_PATH:
        _FLOAT_PATH[level] = run_model(model, InferenceControl(pitch=1.25, energy=0.75, duration=1.5))
    return _FLOAT_PATH[level]


def assert_same_output(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.is_tensor(b[k]) and v.shape == b[k].shape and torch.equal(v, b[k]), k
        else:
            assert v == b[k], k


@pytest.mark.parametrize("form", ["per_token", "per_utterance", "per_utterance_column", "zero_dim", "cpu_float64"])
def test_constant_tensor_control_equals_float(case, form):
    """The new path against the float path.  For the frame-level model ``per_token`` is the [B, Ts] tensor that
    reaches the frames through the length regulator's source index."""
    level, model, _ = case
    base, base_dur = float_path(level, model)
    B, Ts = base["text_input"].shape
    assert int(base["tgt_lens"].max()) > Ts  # (so [B, Ts] cannot be taken for frames)
    shape = {"per_token": (B, Ts), "per_utterance": (B,), "per_utterance_column": (B, 1), "zero_dim": (),
             "cpu_float64": (B, Ts)}[form]
    kw = dict(dtype=torch.float64) if form == "cpu_float64" else dict(device="cuda")
    control = InferenceControl(pitch=torch.full(shape, 1.25, **kw), energy=torch.full(shape, 0.75, **kw),
                               duration=torch.full(shape, 1.5, **kw))
    out, dur = run_model(model, control)
    assert torch.equal(dur, base_dur)
    assert_same_output(out, base)
    assert np.isfinite(out["postnet_output"].cpu().numpy()).all()


def test_per_token_control_against_oracle(case):
    """Non-constant [B, Ts] controls; the bound is 1e-4 * max(1, |ref|max), as in
    tests/test_headdim_model_gpu.py::test_free_inference_against_oracle.  Measured on an MI355X, largest absolute error
    (bound): phone-level output 1.4e-6 (3.5e-4), postnet_output 4.9e-6 (3.7e-4), pitch 2.6e-6 (2.6e-4), energy 3.1e-6
    (2.1e-4); frame-level 1.2e-6, 3.6e-6, 6.7e-6, 4.1e-6 against 3.8e-4, 3.8e-4, 4.0e-4, 2.1e-4.  Durations and lengths
    are exact."""
    level, model, oracle = case
    infer = infer_batch()
    B, Ts = infer["text"].shape
    pitch, energy, duration = per_token_controls(CONTROL_SEED[level], B, Ts)
    for c in (pitch, energy, duration):
        assert float(c.min()) >= 0.5 and float(c.max()) <= 2.0 and float(c.std()) > 0.1
    assert torch.equal(duration * 8, torch.round(duration * 8))
    ref, ref_dur = oracle_reference(oracle, level, pitch, energy, duration)
    # the fixture is well-posed: no scaled prediction of the oracle within 1e-4 (relative) of a bin edge, no duration
    # within 1e-3 of a rounding tie
    edge, tie = well_posed_margins(ref, duration, level)
    print(f"{level}: bin-edge margin {edge:.3e}, rounding-tie margin {tie:.3e}")
    assert edge > 1e-4 and tie > 1e-3, (edge, tie)
    out, dur = run_model(model, InferenceControl(pitch=pitch, energy=energy, duration=duration))
    assert torch.equal(dur.cpu(), ref_dur)
    assert torch.equal(out["tgt_lens"].cpu(), ref["tgt_lens"].int())
    assert int(out["tgt_lens"].max()) > Ts
    for k in ("output", "postnet_output", "pitch_prediction", "energy_prediction"):
        a, b = out[k].cpu().numpy(), ref[k].numpy()
        assert a.shape == b.shape, k
        err, bound = np.abs(a - b).max(), 1e-4 * max(1.0, np.abs(b).max())
        print(f"{level}: {k} max abs error {err:.3e} (bound {bound:.3e})")
        assert err < bound, (k, err, bound)
    # duration_prediction stays the unscaled log-duration, as in the reference
    a, b = out["duration_prediction"].cpu().numpy(), ref["duration_prediction"].numpy()
    assert np.abs(a - b).max() < 1e-4 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", ["pitch", "energy", "duration"])
def test_shape_errors_name_the_control(case, name):
    level, model, _ = case
    base, _ = float_path(level, model)
    B, Ts = base["text_input"].shape
    assert Ts + 1 != int(base["tgt_lens"].max())
    # (a frame-level predictor's [B, Ts + 1] is neither 1, tokens nor frames: raised once the durations give the frames)
    for t in (torch.ones(B, Ts + 1), torch.ones(B + 1), torch.ones(B, Ts, 2), torch.ones(B + 1, Ts)):
        control = InferenceControl(pitch=1.25, energy=0.75, duration=1.5)
        setattr(control, name, t)
        with pytest.raises(ValueError, match=re.escape(f"InferenceControl.{name}: got a tensor of shape {list(t.shape)}")):
            model(infer_batch(), control, inference=True)


def test_training_ignores_tensor_control(case):
    level = case[0]
    model, _ = build_pair(level)  # (its own model: a training forward moves the BatchNorm running statistics)
    batch = train_batch(level)
    B, Ts = batch["text"].shape
    model.train()
    model.training_step(dict(batch))
    want = model._loss_slots.clone()
    model.training_step(dict(batch, duration_control=torch.tensor([1.5, 0.5])))
    assert torch.isfinite(want).all() and torch.equal(model._loss_slots, want)
    control = InferenceControl(pitch=torch.full((B, Ts), 2.0), energy=torch.full((B,), 0.5),
                               duration=torch.full((B, Ts), 1.5))
    plain, ctl = model(dict(batch)), model(dict(batch), control)
    assert_same_output(plain, ctl)
    a = model.loss(plain, model.prepare_batch(dict(batch)), 0)
    b = model.loss(ctl, model.prepare_batch(dict(batch)), 0)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
