"""GPU: free synthesis scored against recorded mels by DTW -- ``synthesize(..., compare=data.DtwWriter)``,
``FastSpeech2.mel_dtw`` and ``fs2l synthesize --compare-to`` -- on the small model and on-disk corpus of
tests/test_scores_gpu.py (``learn_alignment=False``, free synthesis: the model chooses its own frame counts).

Bounds.  Against the float64 definition (tests/dtw_references.py) applied to the WRITTEN spectrogram and the corpus'
recorded mel: ``|total - total64| <= (n + r + C) * 2^-23 * total64``, the end-to-end bound of tests/test_dtw_gpu.py.  Between
two batchings: the spectrograms differ by the forward's fp32 summation order; if no frame moves by more than ``d``
(Euclidean, measured here on the written files) no cost moves by more than ``d`` (triangle inequality) and the cheapest
path's total by no more than ``steps * d``, on top of the float64 bound."""
import csv

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from tests import dtw_references as R

pytestmark = pytest.mark.gpu

N_MELS = 16
_CACHE = {}


def _setup(tmp_path_factory):
    """The corpus, model, checkpoint and filelist rows, built once (inside a test: after the per-test fixtures)."""
    if "setup" not in _CACHE:
        from tests.test_scores_gpu import _corpus
        root = tmp_path_factory.mktemp("dtw")
        model, ckpt, fl, corpus, entries = _corpus(root, learn_alignment=False)
        rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
        audio = model.config.preprocessing.audio
        recorded = [torch.load(D.feature_path(corpus, "spec", e["basename"], e["speaker"], e["language"],
                                              f"spec-{audio.input_sampling_rate}-{audio.spec_type}.pt"), weights_only=True)
                    for e in entries]
        _CACHE["setup"] = (model, ckpt, fl, corpus, entries, rows, recorded)
    return _CACHE["setup"]


def _run(model, rows, corpus, out_dir, batch_size, sort, compare=True, write=True):
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, compare_dir=corpus if compare else None)
    from fastspeech2_lightning_amd.synthesis import synthesize
    writer = D.PackedSpecWriter(out_dir, model.output_key, 9, n_mels=N_MELS) if write else None
    dtw = D.DtwWriter(out_dir, 9) if compare else None
    res = synthesize(model, ds, batch_size, None, writer, sort=sort, exact_lengths=True, compare=dtw)
    return res, dtw


def _bound64(n, r, total64):
    return (n + r + N_MELS) * 2.0 ** -23 * total64


def _read(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.DictReader(f, delimiter="|"))


def _runs(tmp_path_factory):
    """Batch sizes 1, 2, 3, sorted and in input order: {tag: (records by position, spectrograms in input order)}."""
    if "runs" not in _CACHE:
        model, _, _, corpus, entries, rows, _ = _setup(tmp_path_factory)
        root = tmp_path_factory.mktemp("runs")
        runs = {}
        for batch_size in (1, 2, 3):
            for sort in (False, True):
                tag = f"b{batch_size}_{'sorted' if sort else 'input_order'}"
                res, dtw = _run(model, rows, corpus, root / tag, batch_size, sort)
                assert len(res["files"]) == len(entries) and sorted(dtw.records) == list(range(len(entries)))
                runs[tag] = (dtw.records, [torch.load(p, weights_only=True) for p in res["files"]], res["files"], dtw)
        _CACHE["runs"] = runs
    return _CACHE["runs"]


def test_totals_against_the_float64_definition_on_the_written_files(tmp_path_factory):
    _, _, _, _, entries, _, recorded = _setup(tmp_path_factory)
    records, specs, _, _ = _runs(tmp_path_factory)["b2_sorted"]
    lengths = set()
    for pos, e in enumerate(entries):
        rec, y, ref = records[pos], specs[pos].T.numpy(), recorded[pos].T.numpy()
        n, r = len(y), len(ref)
        assert rec["basename"] == e["basename"] and (rec["frames"], rec["ref_frames"]) == (n, r)
        total64, steps64 = R.dtw(R.frame_cost(y, ref))
        err, bound = abs(rec["total"] - total64), _bound64(n, r, total64)
        print(f"{e['basename']}: {n} x {r} frames, total {rec['total']!r} (float64 {total64!r}, steps {rec['steps']} / {steps64}), "
              f"error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (e["basename"], rec["total"], total64)
        assert max(n, r) <= rec["steps"] <= n + r - 1
        assert rec["mel_dtw"] == rec["total"] / rec["steps"] and rec["frame_ratio"] == n / r
        lengths.add((n, r))
    assert len(lengths) > 1 and any(n != r for n, r in lengths)     # free synthesis: not the recordings' lengths


def test_the_distance_does_not_follow_the_batch_size_or_the_sort_order(tmp_path_factory):
    _, _, _, _, entries, _, _ = _setup(tmp_path_factory)
    runs = _runs(tmp_path_factory)
    base, base_specs, _, _ = runs["b1_input_order"]
    for tag, (records, specs, _, _) in runs.items():
        worst = 0.0
        for pos in range(len(entries)):
            a, b = records[pos], base[pos]
            assert (a["frames"], a["ref_frames"]) == (b["frames"], b["ref_frames"]), (tag, pos)
            assert specs[pos].shape == base_specs[pos].shape
            d = float(((specs[pos].double() - base_specs[pos].double()) ** 2).sum(0).sqrt().max())
            bound = max(a["steps"], b["steps"]) * d + _bound64(a["frames"], a["ref_frames"], b["total"])
            worst = max(worst, abs(a["total"] - b["total"]) / bound)
            assert abs(a["total"] - b["total"]) <= bound, (tag, pos, a["total"], b["total"], d)
        print(f"{tag}: worst difference / bound {worst:.4f}")


def test_the_spectrograms_are_those_of_a_run_without_the_comparison(tmp_path, tmp_path_factory):
    model, _, _, corpus, entries, rows, _ = _setup(tmp_path_factory)
    _, _, files, _ = _runs(tmp_path_factory)["b3_sorted"]
    res, none = _run(model, rows, corpus, tmp_path / "plain", 3, True, compare=False)
    assert none is None and [p.name for p in res["files"]] == [p.name for p in files]
    for a, b in zip(res["files"], files):
        assert a.read_bytes() == b.read_bytes(), a.name
    # comparison only: no writer, the same table
    records = _runs(tmp_path_factory)["b3_sorted"][0]
    res, dtw = _run(model, rows, corpus, tmp_path / "only", 3, True, write=False)
    assert res["files"] == [] and not (tmp_path / "only").exists()
    assert {p: (r["total"], r["steps"], r["frames"]) for p, r in dtw.records.items()} == \
        {p: (r["total"], r["steps"], r["frames"]) for p, r in records.items()}


def test_mel_dtw_is_the_two_kernels_on_the_forward_s_output(tmp_path_factory):
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.synthesis import collate_items
    model, _, _, corpus, entries, rows, _ = _setup(tmp_path_factory)
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, compare_dir=corpus)
    batch = collate_items([ds[i] for i in range(3)], learn_alignment=False)
    ref, ref_lens = batch.pop("compare_mel"), batch.pop("compare_lens")
    out = model(batch, inference=True, exact_lengths=True)
    total, steps = model.mel_dtw(out, ref, ref_lens)
    assert total.dtype == torch.float32 and steps.dtype == torch.int32 and total.shape == steps.shape == (3,)
    cost = hip.frame_dist(out[model.output_key], out["tgt_lens"], ref.cuda(), ref_lens.cuda())
    t2, s2 = hip.dtw(cost, out["tgt_lens"], ref_lens.cuda())
    assert torch.equal(total, t2) and torch.equal(steps, s2)
    table = torch.full((6,), float("nan"), device="cuda")
    t3, s3 = model.mel_dtw(out, ref, ref_lens, out=table)
    assert torch.equal(table[:3], total) and torch.equal(table[3:].view(torch.int32), steps) and torch.equal(t3, total)
    assert any(name == "mel_dtw_cost" for name, _, _ in hip.persistent_buffers())
    with pytest.raises(ValueError, match="2 \\* B|6 fp32"):
        model.mel_dtw(out, ref, ref_lens, out=torch.zeros(5, device="cuda"))
    with pytest.raises(ValueError, match="ref must be"):
        model.mel_dtw(out, ref[:2], ref_lens)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.mel_dtw(out, ref, ref_lens)
    finally:
        model.eval()


def test_synthesize_refuses_what_cannot_be_compared(tmp_path, tmp_path_factory):
    from fastspeech2_lightning_amd.synthesis import synthesize
    model, _, _, corpus, _, rows, _ = _setup(tmp_path_factory)
    forced = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, teacher_forcing_dir=corpus)
    with pytest.raises(ValueError, match="teacher-forced"):
        synthesize(model, forced, 2, None, None, compare=D.DtwWriter(tmp_path, 0))
    plain = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id)
    with pytest.raises(ValueError, match="compare_dir"):
        synthesize(model, plain, 2, None, None, compare=D.DtwWriter(tmp_path, 0))


def test_the_command_writes_the_dtw_file(tmp_path, tmp_path_factory):
    model, ckpt, fl, corpus, entries, _, _ = _setup(tmp_path_factory)
    out = tmp_path / "out"
    assert cli.main(["synthesize", str(ckpt), "-f", str(fl), "--compare-to", str(corpus), "-o", str(out), "-b", "2"]) == 0
    path = out / "dtw-9.psv"
    assert path.read_text(encoding="utf8").splitlines()[0] == "|".join(D.DtwWriter.FIELDS) == (
        "basename|speaker|language|mel_dtw|total|steps|frames|ref_frames|frame_ratio|raw_text")
    got = _read(path)
    assert len(got) == len(entries) and sorted(r["basename"] for r in got) == sorted(e["basename"] for e in entries)
    scores = [float(r["mel_dtw"]) for r in got]
    assert scores == sorted(scores, reverse=True) and len(set(scores)) == len(scores)           # worst first
    by_name = {e["basename"]: e for e in entries}
    want = _runs(tmp_path_factory)["b2_sorted"][0]                                              # the same batches
    by_pos = {want[p]["basename"]: want[p] for p in want}
    for r in got:
        assert r["speaker"] == "spk0" and r["language"] == "l0" and r["raw_text"] == by_name[r["basename"]]["characters"]
        assert float(r["mel_dtw"]) == float(r["total"]) / int(r["steps"])
        assert float(r["frame_ratio"]) == int(r["frames"]) / int(r["ref_frames"])
        w = by_pos[r["basename"]]
        assert (float(r["total"]), int(r["steps"]), int(r["frames"])) == (w["total"], w["steps"], w["frames"])
    assert len(list((out / "synthesized_spec").iterdir())) == len(entries)                      # the spectrograms as before
    # scores only: the same file, no spectrogram directory
    only = tmp_path / "only"
    assert cli.main(["synthesize", str(ckpt), "-f", str(fl), "--compare-to", str(corpus), "-o", str(only), "-b", "2",
                     "--scores-only"]) == 0
    assert not (only / "synthesized_spec").exists()
    assert (only / "dtw-9.psv").read_text(encoding="utf8") == path.read_text(encoding="utf8")
