"""Length-bucketed batches on the GPU: the one-launch padded feed (``fs2hip_pad_batch`` / ``hip.pad_batch``) against
``torch.nn.functional.pad``; a training step on a batch padded to a bucket geometry against the oracle fed the SAME padded
batch (padding rows count in BatchNorm statistics and loss denominators, as in the reference); launch plans on a ragged
epoch -- a full batch's geometry first eager, then recorded, then replayed, a bucket's short leftover batch always eager,
counts derived from the sampler alone --
and replayed bucketed steps bit for bit equal to eager ones.  Fresh allocations are poisoned with NaN throughout."""
import json
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd import hip as H
from fastspeech2_lightning_amd import plan as PL
from fastspeech2_lightning_amd.config import Stats
from fastspeech2_lightning_amd.synthetic import synthetic_batch, synthetic_item
from oracle import cases as C
from oracle import fs2_oracle as O
from tests.test_cli_cpu import make_project
from tests.test_plan_gpu import assert_same_state, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def poisoned_allocations():
    """``torch.empty`` / ``empty_like`` come back NaN-filled (the suite's hunting mode, always on in this file): a pad byte
    the kernel did not write, or a plan input a replay's feed missed, shows as NaN instead of as stale zeros."""
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


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------------------------------
def rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g, dtype=dtype).to(DEV)
    return torch.randint(1, 1 << 20, shape, generator=g, dtype=dtype).to(DEV)   # (never 0: a missed copy cannot pass as padding)


def garbage(shape, dtype):
    if dtype.is_floating_point:
        return torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    return torch.full(shape, -7, dtype=dtype, device=DEV)


def raw_pad(members, n=None):
    """``fs2hip_pad_batch`` itself: members = [(src ptr, dst ptr, B, src0, src1, dst0, dst1, row_bytes)]."""
    arr = (H.PadMember * max(len(members), 1))()
    for m, (src, dst, B, s0, s1, d0, d1, row) in zip(arr, members):
        m.src, m.dst, m.B, m.src0, m.src1, m.dst0, m.dst1, m.row_bytes = src, dst, B, s0, s1, d0, d1, row
    with torch.cuda.device(DEV):
        return H.lib().fs2hip_pad_batch(arr, len(members) if n is None else n, H._stream())


def member(src, dst):
    """[B, a0(, a1), inner...] -> [B, d0(, d1), inner...]: the padded axes are the ones whose extents differ, or axis 1."""
    axes = [i for i in range(1, src.dim()) if src.shape[i] != dst.shape[i]] or [1]
    assert axes in ([1], [2], [1, 2]) and src.dtype == dst.dtype
    if axes == [2]:
        axes = [1, 2]
    ext_s = [src.shape[i] for i in axes] + [1]
    ext_d = [dst.shape[i] for i in axes] + [1]
    inner = int(np.prod(src.shape[axes[-1] + 1:], dtype=np.int64))
    return (src.data_ptr(), dst.data_ptr(), src.shape[0], ext_s[0], ext_s[1], ext_d[0], ext_d[1], inner * src.element_size())


def f_pad(src, shape):
    pads = []
    for i in range(src.dim() - 1, 0, -1):
        pads += [0, shape[i] - src.shape[i]]
    return F.pad(src, pads)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64], ids=["fp32", "int32", "int64"])
@pytest.mark.parametrize("src_shape,dst_shape", [
    ((4, 37, 80), (4, 64, 80)),        # mel: one axis, 320-byte rows (16-byte units)
    ((4, 13), (4, 29)),                # text / durations / phone-level pitch: one axis, one element per row
    ((3, 41, 13), (3, 57, 20)),        # attention prior [B, Tm, Ts]: both axes
    ((3, 41, 13), (3, 41, 20)),        # only the inner of the two axes grows
    ((2, 9, 5, 3), (2, 16, 7, 3)),     # two axes in front of an inner row that is not a multiple of 16 bytes
    ((5, 21, 19), (5, 21, 19)),        # extents equal: a plain copy
    ((1, 30, 7), (1, 33, 7)),          # B = 1, 28-byte rows
    ((1, 1), (1, 1)),                  # one element
    ((6,), (6,)),                      # a length vector: no padded axis at all
], ids=["mel", "text", "prior2d", "prior_inner", "odd_row", "equal", "B1", "single", "vector"])
def test_pad_kernel_equals_functional_pad(dtype, src_shape, dst_shape):
    src = rand(src_shape, dtype, seed=len(src_shape) * 100 + src_shape[-1])
    dst = garbage(dst_shape, dtype)
    want = f_pad(src, dst_shape)
    if src.dim() == 1:
        m = (src.data_ptr(), dst.data_ptr(), src.shape[0], 1, 1, 1, 1, src.element_size())
    else:
        m = member(src, dst)
    assert raw_pad([m]) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, want)
    if src_shape != dst_shape:
        assert int((dst == 0).sum()) >= dst.numel() - src.numel()   # every pad element is zero (the garbage is gone)


def test_pad_kernel_at_unaligned_addresses_takes_narrower_units():
    """Base addresses that are only 4- or 1-byte aligned (views into a larger buffer): same result, narrower units."""
    for off, dtype in ((1, torch.int32), (3, torch.float32), (5, torch.uint8), (2, torch.int64)):
        if dtype == torch.uint8:   # odd byte addresses: 1-byte units
            big_s, big_d = rand((1024,), torch.int32, 3).view(torch.uint8), torch.full((8192,), 9, dtype=dtype, device=DEV)
        else:
            big_s, big_d = rand((4096,), dtype, 3), garbage((8192,), dtype)
        src = big_s[off:off + 3 * 11 * 8].view(3, 11, 8)
        dst = big_d[off:off + 3 * 17 * 8].view(3, 17, 8)
        before, after = big_d[:off].clone(), big_d[off + 3 * 17 * 8:].clone()
        assert raw_pad([member(src, dst)]) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst, f_pad(src, (3, 17, 8)))
        same = lambda a, b: torch.equal(a.view(torch.uint8), b.view(torch.uint8))  # noqa: E731  (NaN-proof)
        assert same(big_d[:off], before) and same(big_d[off + 3 * 17 * 8:], after)   # nothing outside the destination is touched


def test_sixteen_members_in_one_launch():
    dtypes = [torch.float32, torch.int32, torch.int64]
    srcs, dsts, wants, members = [], [], [], []
    for i in range(H.PAD_MAX_MEMBERS):
        dt = dtypes[i % 3]
        B, a0, a1, inner = 1 + i % 4, 3 + 5 * i, 2 + i, 1 + (i * 7) % 10
        shape, big = (B, a0, a1, inner), (B, a0 + (i % 5) * 3, a1 + (i % 3) * 4, inner)
        srcs.append(rand(shape, dt, seed=i))
        dsts.append(garbage(big, dt))
        wants.append(f_pad(srcs[-1], big))
        members.append((srcs[-1].data_ptr(), dsts[-1].data_ptr(), B, a0, a1, big[1], big[2], inner * srcs[-1].element_size()))
    assert raw_pad(members) == 0
    torch.cuda.synchronize()
    for i, (d, w) in enumerate(zip(dsts, wants)):
        assert torch.equal(d, w), i


def test_pad_kernel_rejects_bad_arguments():
    src, dst = rand((2, 5, 4), torch.float32, 1), garbage((2, 8, 4), torch.float32)
    keep = dst.clone()
    ok = member(src, dst)
    EINVAL = -22
    assert raw_pad([(ok[1], ok[0], 2, 8, 1, 5, 1, 16)]) == EINVAL                                  # destination smaller than the source
    assert raw_pad([(ok[0], ok[1], 2, 5, 3, 8, 2, 16)]) == EINVAL                                  # ... in the second axis
    assert raw_pad([ok] * (H.PAD_MAX_MEMBERS + 1)) == EINVAL                                       # more than 16 members
    assert raw_pad([(None, ok[1]) + ok[2:]]) == EINVAL and raw_pad([(ok[0], None) + ok[2:]]) == EINVAL   # a null pointer
    for bad in ((0, 5, 1, 8, 1, 16), (2, 0, 1, 8, 1, 16), (2, 5, 0, 8, 1, 16), (2, 5, 1, 8, 1, 0), (2, -5, 1, 8, 1, 16)):
        assert raw_pad([ok[:2] + bad]) == EINVAL, bad                                              # a non-positive extent
    assert raw_pad([ok], n=0) == EINVAL
    assert raw_pad([(ok[0], ok[0], 2, 5, 1, 8, 1, 16)]) == EINVAL                                  # padding in place would overlap
    torch.cuda.synchronize()
    same = torch.equal(dst.view(torch.int32), keep.view(torch.int32))
    assert same                                                                                   # nothing was enqueued
    assert raw_pad([(ok[0], ok[0], 2, 5, 1, 5, 1, 16)]) == 0                                       # src == dst, equal extents: nothing to do


def tight_batch(learn_alignment=False, frame_level=False, B=4, seed=21, n_mels=16):
    b = synthetic_batch(B=B, ts_lo=6, ts_hi=12, n_symbols=C.N_SYMBOLS, n_mels=n_mels, seed=seed, dur_hi=4,
                        learn_alignment=learn_alignment, frame_level=frame_level)
    return b


def cpu_padded(batch, Ts_b, Tm_b, frame_level):
    """What ``collate`` would have produced for a batch whose maxima are the bucket's: zeros behind every column."""
    out = dict(batch)
    Ts, Tm = batch["text"].shape[1], batch["mel"].shape[1]
    out["text"] = F.pad(batch["text"], (0, Ts_b - Ts))
    out["mel"] = F.pad(batch["mel"], (0, 0, 0, Tm_b - Tm))
    for k in ("pitch", "energy"):
        out[k] = F.pad(batch[k], (0, (Tm_b - Tm) if frame_level else (Ts_b - Ts)))
    if batch["duration"].dim() == 3:
        out["duration"] = F.pad(batch["duration"], (0, Ts_b - Ts, 0, Tm_b - Tm))
    else:
        out["duration"] = F.pad(batch["duration"], (0, Ts_b - Ts))
    out["max_src_len"], out["max_mel_len"] = Ts_b, Tm_b
    return out


@pytest.mark.parametrize("learn_alignment", [False, True], ids=["plain", "learn_alignment"])
def test_hip_pad_batch_pads_a_whole_device_batch_like_collate_would(learn_alignment):
    from fastspeech2_lightning_amd.model import FastSpeech2
    config = C.small_config(learn_alignment=learn_alignment)
    model = FastSpeech2(config, Stats(**C.STATS))
    batch = tight_batch(learn_alignment)
    Ts, Tm = batch["text"].shape[1], batch["mel"].shape[1]
    for Ts_b, Tm_b in ((Ts + 5, Tm + 9), (Ts, Tm + 1), (Ts + 3, Tm), (Ts, Tm)):
        want = cpu_padded(batch, Ts_b, Tm_b, learn_alignment)
        got = model.pad_batch(batch, Ts_b, Tm_b)
        assert got["max_src_len"] == Ts_b and got["max_mel_len"] == Tm_b
        for k, v in want.items():
            if torch.is_tensor(v):
                assert got[k].is_cuda and got[k].shape == v.shape, k
                assert torch.equal(got[k].cpu(), v.to(got[k].dtype)), (k, Ts_b, Tm_b)
        # the replay-side feed: every tensor of `out` -- length vectors and ids too -- written by the one launch
        dev = model.prepare_batch(batch)
        out = {k: garbage(tuple(v.shape), v.dtype) for k, v in got.items() if torch.is_tensor(v) and v.is_cuda}
        with torch.cuda.device(model.device_):
            fed = H.pad_batch(dev, Ts_b, Tm_b, out=out, frame_level=model._frame_level_targets())
        torch.cuda.synchronize()
        for k, v in out.items():
            assert fed[k] is v and torch.equal(v, got[k]), k
    with pytest.raises(ValueError, match="does not fit"):
        model.pad_batch(batch, Ts - 1, Tm)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.pad_batch(batch, Ts + 1, Tm + 1, frame_level=False)


# ----------------------------------------------------------------------------------------------------------------------
# parity: the step on a padded ragged batch is the oracle's step on the same padded batch
# ----------------------------------------------------------------------------------------------------------------------
def rel(a, b, floor=1e-6):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def regulate_to_the_padded_length(monkeypatch):
    """The reference's LengthRegulator (fs2/variance_adaptor.py:65-81) cuts its output at the longest EXPANDED utterance of
    the batch, which in every batch ``collate_method`` builds is ``max_mel_len`` itself; fed a batch whose mel padding goes
    beyond that, its own decoder input no longer matches the positional table (fs2/model.py:233-241 raises).  For the
    oracle to compute the padded batch at all, its regulator's output is continued with zero rows (mask False) up to
    ``max_mel_len`` -- what it returns whenever one utterance reaches that length.  Nothing else of the oracle changes."""
    real = O.length_regulate

    def regulate(x, durations, max_length):
        out, mask = real(x, durations, max_length)
        n = int(max_length) - out.shape[1]
        if n <= 0:
            return out, mask
        return (torch.cat([out, out.new_zeros(out.shape[0], n, out.shape[2])], 1),
                torch.cat([mask, mask.new_zeros(mask.shape[0], n)], 1))
    monkeypatch.setattr(O, "length_regulate", regulate)


@pytest.mark.parametrize("learn_alignment", [False, True], ids=["plain", "learn_alignment"])
def test_bucketed_training_step_vs_oracle_on_the_same_padded_batch(learn_alignment, monkeypatch):
    """Forward, losses and gradients of one training step on a ragged batch padded (on the GPU) to a bucket geometry well
    beyond its own maxima, against the oracle fed that padded batch.  Tolerances of the whole-path tests
    (``tests/test_model_gpu.py``): outputs and losses 1e-4 relative, gradients 2e-3 of each tensor's max."""
    from fastspeech2_lightning_amd.model import FastSpeech2
    regulate_to_the_padded_length(monkeypatch)
    config = C.small_config(learn_alignment=learn_alignment)
    batch = tight_batch(learn_alignment, B=5, seed=33)
    Ts, Tm = batch["text"].shape[1], batch["mel"].shape[1]
    Ts_b, Tm_b = Ts + 7, Tm + 19
    padded = cpu_padded(batch, Ts_b, Tm_b, learn_alignment)
    model = FastSpeech2(config, Stats(**C.STATS))
    oracle = O.FastSpeech2Oracle(config, Stats(**C.STATS), n_symbols=C.N_SYMBOLS)
    sd = O.seeded_state_dict(oracle.state_dict())
    oracle.load_state_dict(sd)
    model.load_state_dict(sd)
    model.train(); oracle.train()
    model.postnet.dropout_p = 0.0
    oracle.postnet.dropout_p = 0.0
    ref = oracle(padded)
    ref_losses = oracle.loss(ref, padded, 0)
    ref_losses["total"].backward()
    total = model.training_step(dict(batch, bucket_geometry=(Ts_b, Tm_b)))
    out = model.last_output
    for k in ("output", "postnet_output", "duration_prediction", "pitch_prediction", "energy_prediction"):
        assert (out[k] is None) == (ref[k] is None), k
        if ref[k] is None:
            continue
        assert out[k].shape == ref[k].shape, k
        r = rel(out[k].detach().cpu().numpy(), ref[k].detach().numpy())
        print(f"{k}: rel {r:.3e}")
        assert r < 1e-4, (k, r)
    assert out["output"].shape[1] == Tm_b
    got_losses = model.losses_to_host()
    assert set(got_losses) == set(ref_losses)
    for k, v in ref_losses.items():
        print(f"loss {k}: {got_losses[k]:.8f} vs {float(v):.8f}")
        assert abs(got_losses[k] - float(v)) < 1e-4 * max(1.0, abs(float(v))), k
    assert abs(float(total) - float(ref_losses["total"])) < 1e-4 * float(ref_losses["total"])
    got = model.store.grad_state_dict()
    floor = 1e-4 * max(float(p.grad.abs().max()) for p in oracle.parameters() if p.grad is not None)
    worst = ("", 0.0)
    for k, p in oracle.named_parameters():
        if p.grad is None:
            continue
        r = rel(got[k].cpu().numpy(), p.grad.numpy(), floor)
        if float(p.grad.abs().max()) < floor:   # pure-noise tensor (true gradient exactly zero), as in test_model_gpu.py
            assert r < 2e-2, (k, r)
            continue
        if r > worst[1]:
            worst = (k, r)
    print("worst gradient:", worst)
    assert worst[1] < 2e-3, worst


# ----------------------------------------------------------------------------------------------------------------------
# plans on ragged data
# ----------------------------------------------------------------------------------------------------------------------
BATCH, BUCKETS = 4, 3
#: 38 utterances of distinct mel lengths: buckets of 12 / 13 / 13 items = 3 full batches each + leftovers of 0 / 1 / 1
LENGTHS = [(5 + i % 9, 24 + 3 * i + (i * 7) % 3) for i in range(38)]


def ragged_items(config, learn_alignment=False):
    n_mels = config.preprocessing.audio.n_mels
    return [synthetic_item(t, m, n_symbols=C.N_SYMBOLS, n_mels=n_mels, seed=1000 + i, learn_alignment=learn_alignment)
            for i, (t, m) in enumerate(LENGTHS)]


def epoch_batches(items, epoch, bucketed, learn_alignment=False, seed=7):
    """The host batches of one epoch as ``fs2l train`` builds them, with and without ``--bucket-lengths``."""
    if bucketed:
        s = D.LengthBucketBatchSampler(LENGTHS, BATCH, BUCKETS, seed=seed, epoch=epoch)
        ds = D.BucketedDataset(items, s)
        return [D.collate_bucketed([ds[i] for i in b], learn_alignment=learn_alignment) for b in s], list(s)
    idx = D.random_batches(len(items), BATCH, seed + epoch)
    return [D.collate([items[i] for i in b], learn_alignment=learn_alignment) for b in idx], idx


def expected_counts(geometries):
    """A full batch's geometry: first step eager, second recorded, the rest replayed (``plan.RECORD_AFTER`` = 1).  A
    bucket's short leftover batch (another ``B``) always runs eagerly: one plan per bucket."""
    seen, eager, recorded, replayed = Counter(), 0, 0, 0
    for g in geometries:
        if g[0] != BATCH:
            eager += 1
            continue
        n = seen[g]
        seen[g] += 1
        eager, recorded, replayed = eager + (n == 0), recorded + (n == 1), replayed + (n >= 2)
    return replayed, recorded, eager


def run_epochs(model, opt, items, bucketed, epochs=2, learn_alignment=False):
    rows, kinds = [], []
    for epoch in range(epochs):
        for b in epoch_batches(items, epoch, bucketed, learn_alignment)[0]:
            before = (model.plans.replayed, model.plans.recorded, model.plans.eager)
            with torch.no_grad():
                model.training_step(b)
            after = (model.plans.replayed, model.plans.recorded, model.plans.eager)
            kinds.append(("replayed", "recorded", "eager")[[a - c for a, c in zip(after, before)].index(1)] if after != before else "off")
            rows.append(model._loss_slots.clone())
            opt.step()
    torch.cuda.synchronize()
    return rows, kinds


def test_plans_replay_on_a_ragged_epoch_with_buckets_and_never_without():
    assert PL.RECORD_AFTER == 1 and PL.MAX_PLANS >= BUCKETS
    model, opt, config = build(plan=True)
    items = ragged_items(config)
    geos = []
    for epoch in range(2):
        s = D.LengthBucketBatchSampler(LENGTHS, BATCH, BUCKETS, seed=7, epoch=epoch)
        assert [len(m) for _, m in s.buckets] == [12, 13, 13]
        geos += [(len(b),) + b.geometry for b in s]
    want = expected_counts(geos)
    assert len(geos) == 22 and want == (18 - 2 * 3, 3, 3 + 4)   # 18 full batches of 3 geometries; 4 leftover batches, all eager
    rows, kinds = run_epochs(model, opt, items, bucketed=True)
    p = model.plans
    assert (p.replayed, p.recorded, p.eager) == want, (p.replayed, p.recorded, p.eager, want)
    seen = Counter()
    for g, kind in zip(geos, kinds):                              # ... and in this order, geometry by geometry
        assert kind == ("eager" if g[0] != BATCH else ("eager", "recorded", "replayed")[min(seen[g], 2)]), (g, kind, seen[g])
        seen[g] += 1
    assert all(torch.isfinite(r).all() for r in rows)
    assert len(p.plans) == BUCKETS                                # one plan per bucket: leftovers take none
    for sig, plan in p.plans.items():                             # the plans' inputs have the buckets' geometries
        assert plan.inputs["text"].shape[0] == BATCH
        assert (plan.inputs["text"].shape[0], plan.inputs["text"].shape[1], plan.inputs["mel"].shape[1]) in set(geos)
    # the same data through the unbucketed loader: no geometry comes a third time, nothing is replayed
    plain, opt2, _ = build(plan=True)
    shapes = Counter()
    for epoch in range(2):
        for b in epoch_batches(items, epoch, bucketed=False)[0]:
            shapes[(b["text"].shape, b["mel"].shape)] += 1
    assert max(shapes.values()) < 3
    run_epochs(plain, opt2, items, bucketed=False)
    assert plain.plans.replayed == 0 and plain.plans.eager + plain.plans.recorded == 20


@pytest.mark.parametrize("variant", ["32-true", "bf16-mixed", "learn_alignment"])
def test_replayed_bucketed_steps_equal_eager_ones_bit_for_bit(variant):
    """Two models from one seed, one with plans off, over the same two bucketed epochs (dropout on): every loss term of
    every step and afterwards every weight, Adam moment, BatchNorm buffer and counter must be equal bit for bit -- the
    one-launch feed into the recorded inputs leaves nothing of the previous batch behind."""
    la = variant == "learn_alignment"
    prec = "32-true" if la else variant
    cfg = dict(learn_alignment=True) if la else {}
    eager, opt_e, config = build(prec, plan=False, **cfg)
    planned, opt_p, _ = build(prec, plan=True, **cfg)
    items = ragged_items(config, learn_alignment=la)
    want, _ = run_epochs(eager, opt_e, items, bucketed=True, learn_alignment=la)
    got, kinds = run_epochs(planned, opt_p, items, bucketed=True, learn_alignment=la)
    assert eager.plans.recorded == 0 and eager.plans.replayed == 0
    assert planned.plans.replayed == 12 and planned.plans.recorded == 3 and planned.plans.eager == 7
    for i, (w, g) in enumerate(zip(want, got)):
        assert torch.isfinite(w).all() and torch.equal(w, g), (variant, i, kinds[i], w.tolist(), g.tolist())
    assert_same_state(eager, planned)
    for k in ("output", "postnet_output", "duration_prediction", "pitch_prediction", "energy_prediction", "tgt_mask"):
        assert torch.equal(eager.last_output[k], planned.last_output[k]), k


@pytest.fixture
def host_threads_restored():
    """``fs2l train`` in this process takes the whole host for torch's intra-op pool (``parallel.apply_host_budget``):
    put the pool back as it was, or every CPU oracle of the tests that run after this file is oversubscribed."""
    before = torch.get_num_threads()
    try:
        yield
    finally:
        torch.set_num_threads(before)


def test_fs2l_train_with_bucket_lengths_replays_plans(tmp_path, host_threads_restored):
    cfg = make_project(tmp_path, n_train=24, n_val=3, write_features=True)   # batch 4, 2 buckets of 12 = 6 steps per epoch
    out = tmp_path / "run"
    assert cli.main(["train", str(cfg), "--output-dir", str(out), "--log-every", "1", "--devices", "1", "--max-steps", "12",
                     "--bucket-lengths", "2"]) == 0
    recs = [json.loads(l) for l in (out / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "training/total_loss" in r]
    assert len(train) == 12
    for r in train:
        assert r["plans_replayed"] + r["plans_recorded"] + r["plans_eager"] == r["step"]
    assert train[-1]["plans_replayed"] == 8 and train[-1]["plans_recorded"] == 2 and train[-1]["plans_eager"] == 2
    assert all(np.isfinite(r["training/total_loss"]) for r in train)
    assert (out / "lengths.json").exists()
    # without the switch the same run logs the counters too, and replays nothing on this ragged data
    out2 = tmp_path / "plain"
    assert cli.main(["train", str(cfg), "--output-dir", str(out2), "--log-every", "1", "--devices", "1", "--max-steps", "12"]) == 0
    last = [json.loads(l) for l in (out2 / "metrics.jsonl").read_text().splitlines() if "plans_replayed" in l][-1]
    assert last["plans_replayed"] + last["plans_recorded"] + last["plans_eager"] == 12 and not (out2 / "lengths.json").exists()
