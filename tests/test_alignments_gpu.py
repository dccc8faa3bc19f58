"""GPU: ``synthesize(..., alignments=AlignmentWriter)`` and ``fs2l synthesize --write-alignments``: per-token durations,
pitch and energy beside the spectrograms.  Yardsticks: a direct ``model(batch, inference=True)`` on the batches
``synthesis_batches`` names (bit for bit), and the CPU oracle run one utterance at a time (``exact_lengths``)."""
import json
import shutil

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd import synthesis as S
from fastspeech2_lightning_amd.config import InferenceControl, TextConfig, TextProcessor
from oracle import cases as C
from oracle import fs2_oracle as O

pytestmark = pytest.mark.gpu

_MODELS = {}


def _small(level):
    from tests.test_synthesize_gpu import _build
    if level not in _MODELS:
        _MODELS[level] = _build(C.small_config(learn_alignment=False, level=level))
    return _MODELS[level]


def _forward_rows(model, ds, batch_size, sort, **kw):
    """{item index: (duration, pitch, energy, frames)} from a direct forward on the batches ``synthesis_batches`` names."""
    vp = model.config.model.variance_predictors
    want = {}
    for idx in D.synthesis_batches(ds.token_counts, batch_size, sort):
        batch = D.collate([ds[i] for i in idx], learn_alignment=model.config.model.learn_alignment)
        out = model(batch, InferenceControl(), inference=True, **kw)
        src, tgt = out["src_lens"].tolist(), out["tgt_lens"].tolist()
        for j, i in enumerate(idx):
            row = {"duration": out["duration_rounded"][j, :src[j]].cpu(), "frames": tgt[j]}
            for name in ("pitch", "energy"):
                n = src[j] if getattr(vp, name).level.value == "phone" else tgt[j]
                row[name] = out[f"{name}_prediction"][j, :n].cpu()
            want[i] = row
    return want


def _check_files(model, ds, res, want, source):
    vp = model.config.model.variance_predictors
    tp = TextProcessor(model.config.text)
    assert len(res["alignment_files"]) == len(res["files"]) == len(ds)
    for i, (apath, spath) in enumerate(zip(res["alignment_files"], res["files"])):
        rec = torch.load(apath, weights_only=True)
        assert sorted(rec) == ["duration", "duration_source", "energy", "energy_level", "frames", "pitch", "pitch_level",
                               "raw_text", "symbols", "text"]
        assert rec["duration"].dtype == torch.int32 and rec["text"].dtype == torch.int32
        assert rec["pitch"].dtype == rec["energy"].dtype == torch.float32
        assert torch.equal(rec["text"], ds.tokens[i]) and rec["symbols"] == tp.decode_tokens(rec["text"])
        assert rec["pitch_level"] == vp.pitch.level.value and rec["energy_level"] == vp.energy.level.value
        assert rec["duration_source"] == source and rec["raw_text"] == ds[i]["raw_text"]
        for k in ("duration", "pitch", "energy"):
            assert torch.equal(rec[k], want[i][k]), (i, k)
        spec = torch.load(spath, weights_only=True)
        assert int(rec["duration"].sum()) == rec["frames"] == spec.shape[1] == want[i]["frames"]


#: (depth, batch size, sort)
LOOPS = [(2, 1, True), (2, 2, True), (2, 3, True), (2, 2, False), (2, 3, False), (1, 2, True), (1, 3, False)]


@pytest.mark.parametrize("level", ["phone", "frame"])
def test_free_synthesis_files_equal_the_forward(tmp_path, level):
    from tests.test_synthesize_gpu import STEP, TEXTS, _dataset
    model = _small(level)
    symbols = TextProcessor(model.config.text).symbols
    for depth, b, sort in LOOPS:
        out = tmp_path / f"d{depth}b{b}{sort}"
        ds = _dataset(model, TEXTS)
        res = S.synthesize(model, ds, b, InferenceControl(), D.PackedSpecWriter(out, model.output_key, STEP, n_mels=16),
                           sort=sort, depth=depth, alignments=D.AlignmentWriter(out, STEP, symbols))
        assert "duration_files" not in res and not (out / "duration").exists()
        assert [p.name for p in res["alignment_files"]] == [
            f"{D.truncate_basename(D.slugify(t))}--spk0--l0--ckpt={STEP}--alignment.pt" for t in TEXTS]
        _check_files(model, ds, res, _forward_rows(model, ds, b, sort), "predicted")
    # alignments alone: no spectrogram writer
    ds = _dataset(model, TEXTS)
    res = S.synthesize(model, ds, 3, None, None, alignments=D.AlignmentWriter(tmp_path / "only", STEP, symbols))
    assert res["files"] == [] and len(res["alignment_files"]) == len(TEXTS)
    want = _forward_rows(model, ds, 3, True)
    for i, p in enumerate(res["alignment_files"]):
        assert torch.equal(torch.load(p, weights_only=True)["duration"], want[i]["duration"])
    with pytest.raises(ValueError, match="nothing to write"):
        S.synthesize(model, ds, 3, None, None)


def _corpus(tmp_path, cfg, learn_alignment, n_utts=5):
    from tests.test_data_gpu import SYMBOLS, _write_corpus
    cfg.text = TextConfig(symbols={"letters": SYMBOLS})
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    entries = _write_corpus(corpus, cfg, n_utts=n_utts, learn_alignment=learn_alignment)
    fl = tmp_path / "list.psv"
    cols = ["basename", "language", "speaker", "characters", "character_tokens"]
    fl.write_text("|".join(cols) + "\n" + "".join("|".join(e[c] for c in cols) + "\n" for e in entries), encoding="utf8")
    return corpus, entries, fl


@pytest.mark.parametrize("level", ["phone", "frame"])
def test_teacher_forced_files_equal_the_forward(tmp_path, level):
    from tests.test_synthesize_gpu import _build
    cfg = C.small_config(learn_alignment=False, level=level)
    corpus, entries, fl = _corpus(tmp_path, cfg, False)
    model = _build(cfg)
    symbols = TextProcessor(cfg.text).symbols
    rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
    for depth, b, sort in LOOPS[1:5]:
        out = tmp_path / f"d{depth}b{b}{sort}"
        ds = D.SynthesisDataset(rows, cfg, model.lang2id, model.speaker2id, teacher_forcing_dir=corpus)
        res = S.synthesize(model, ds, b, None, D.PackedSpecWriter(out, model.output_key, 9, n_mels=16), sort=sort,
                           depth=depth, alignments=D.AlignmentWriter(out, 9, symbols))
        assert "duration_files" not in res
        _check_files(model, ds, res, _forward_rows(model, ds, b, sort), "given")
        for e, p in zip(entries, res["alignment_files"]):   # given durations: the corpus's own
            stored = torch.load(D.feature_path(corpus, "duration", e["basename"], "spk0", "l0", "duration.pt"), weights_only=True)
            assert torch.equal(torch.load(p, weights_only=True)["duration"], stored.int())


def _token_dataset(model, texts):
    """A free-synthesis dataset whose items carry exactly the token ids ``texts`` (through the escaped token column)."""
    symbols = TextProcessor(model.config.text).symbols
    entries = [{"basename": f"u{k}", "characters": f"utterance {k}", "character_tokens": "/".join(symbols[int(i)] for i in t),
                "language": "l0", "speaker": "spk0", "is_last_input_chunk": True, "duration_control": 1.0}
               for k, t in enumerate(texts)]
    ds = D.SynthesisDataset(entries, model.config, model.lang2id, model.speaker2id)
    assert all(torch.equal(a, b) for a, b in zip(ds.tokens, texts))
    return ds


@pytest.mark.parametrize("level", ["phone", "frame"])
def test_exact_lengths_files_equal_the_oracle_alone(tmp_path, level):
    """The texts of the seed-21 ragged batch (tests/test_exact_lengths_gpu.py), synthesized freely as ONE batch.  With
    ``exact_lengths`` every file must be what the CPU oracle gives for the utterance alone: durations exactly, pitch and
    energy within that file's bound, 1e-4 * max(1, |ref|).  Without the flag at least one duration must differ from the
    alone-runs (on the CPU oracle itself the batch differs from them in 9 durations at the phone level and in 6 at the
    frame level; the closest duration to a rounding boundary is 7.3e-3 / 2.5e-2 * (value + 1) away)."""
    from tests.test_exact_lengths_gpu import _free_batch, _pair, _rounded
    cfg = C.small_config(learn_alignment=False, level=level)
    model, oracle = _pair(cfg)
    batch = O.synthetic_batch(**C._KW, seed=21)
    texts = [batch["text"][j, :int(batch["src_lens"][j])].clone() for j in range(3)]
    with torch.no_grad():
        alone = [oracle(_free_batch([t]), InferenceControl(), inference=True) for t in texts]
        together = oracle(_free_batch(texts), InferenceControl(), inference=True)
    v = torch.cat([torch.exp(a["duration_prediction"][0].double()) - 1 for a in alone])
    v = v[v > 0]
    assert float(((v - (torch.floor(v) + 0.5)).abs() / (v + 1)).min()) >= 1e-3
    assert any(not torch.equal(_rounded(together["duration_prediction"][j, :len(t)]), _rounded(alone[j]["duration_prediction"][0]))
               for j, t in enumerate(texts)), "the oracle's batch already equals its alone-runs: pick another seed"
    symbols = TextProcessor(cfg.text).symbols

    def run(tag, exact):
        ds = _token_dataset(model, texts)
        res = S.synthesize(model, ds, 3, InferenceControl(), D.PackedSpecWriter(tmp_path / tag, model.output_key, 1, n_mels=16),
                           exact_lengths=exact, alignments=D.AlignmentWriter(tmp_path / tag, 1, symbols))
        return [torch.load(p, weights_only=True) for p in res["alignment_files"]]

    got = run("exact", True)
    for j, (rec, ref) in enumerate(zip(got, alone)):
        want_dur = _rounded(ref["duration_prediction"][0])
        print(f"{level}: utterance {j}: durations {rec['duration'].tolist()} against alone {want_dur.tolist()}")
        assert torch.equal(rec["duration"], want_dur) and rec["frames"] == int(ref["tgt_lens"][0]) >= 1
        for k in ("pitch", "energy"):
            r = ref[f"{k}_prediction"][0]
            assert rec[k].shape == r.shape, (k, rec[k].shape, r.shape)
            err, tol = float((rec[k] - r).abs().max()), 1e-4 * max(1.0, float(r.abs().max()))
            print(f"{level}: utterance {j}: {k} error {err:.3e}, bound {tol:.3e}")
            assert err < tol, (j, k, err, tol)
    plain = run("plain", False)
    differing = sum(int((rec["duration"] != _rounded(ref["duration_prediction"][0])).sum()) for rec, ref in zip(plain, alone))
    print(f"{level}: without exact_lengths {differing} durations differ from the alone-runs")
    assert differing >= 1


def test_durations_are_clipped_to_the_frames_written(tmp_path, monkeypatch):
    """The output cut at a maximum length (the batch's ``max_mel_len``: 6 frames here): ``duration`` follows the clip rule
    and still adds up to the spectrogram's frame count."""
    from tests.test_synthesize_gpu import STEP, TEXTS, _dataset
    model = _small("frame")
    limit = 6
    monkeypatch.setattr(S, "collate", lambda *a, **k: dict(D.collate(*a, **k), max_mel_len=limit))
    ds = _dataset(model, TEXTS)
    res = S.synthesize(model, ds, 3, None, D.PackedSpecWriter(tmp_path, model.output_key, STEP, n_mels=16),
                       alignments=D.AlignmentWriter(tmp_path, STEP, TextProcessor(model.config.text).symbols))
    monkeypatch.undo()
    cut = 0
    for idx in D.synthesis_batches(ds.token_counts, 3):
        batch = dict(D.collate([ds[i] for i in idx], learn_alignment=False), max_mel_len=limit)
        out = model(batch, InferenceControl(), inference=True)
        src, tgt = out["src_lens"].tolist(), out["tgt_lens"].tolist()
        for j, i in enumerate(idx):
            full = out["duration_rounded"][j, :src[j]].cpu().long()
            rec = torch.load(res["alignment_files"][i], weights_only=True)
            spec = torch.load(res["files"][i], weights_only=True)
            ends = full.cumsum(0).clamp(max=tgt[j])
            want = torch.diff(ends, prepend=torch.zeros(1, dtype=torch.long)).int()
            assert torch.equal(rec["duration"], want)
            assert int(rec["duration"].sum()) == rec["frames"] == spec.shape[1] == tgt[j] <= limit
            assert rec["pitch"].numel() == tgt[j] and torch.equal(rec["pitch"], out["pitch_prediction"][j, :tgt[j]].cpu())
            cut += int(full.sum()) > tgt[j]
    assert cut >= 1   # at least one utterance was cut


def test_learned_aligner_durations_train_a_fixed_duration_model(tmp_path):
    from tests.test_data_gpu import _model
    from tests.test_synthesize_gpu import _build
    cfg = C.small_config(learn_alignment=True)
    corpus, entries, fl = _corpus(tmp_path, cfg, True)
    model = _build(cfg)
    rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
    ds = D.SynthesisDataset(rows, cfg, model.lang2id, model.speaker2id, teacher_forcing_dir=corpus)
    out = tmp_path / "out"
    res = S.synthesize(model, ds, 2, None, D.PackedSpecWriter(out, model.output_key, 9, n_mels=16),
                       alignments=D.AlignmentWriter(out, 9, TextProcessor(cfg.text).symbols))
    _check_files(model, ds, res, _forward_rows(model, ds, 2, True), "aligner")
    audio = cfg.preprocessing.audio
    assert [p.name for p in res["duration_files"]] == [f"{e['basename']}--spk0--l0--duration.pt" for e in
                                                        (entries[i] for b in D.synthesis_batches(ds.token_counts, 2) for i in b)]
    for e, apath in zip(entries, res["alignment_files"]):
        dur = torch.load(D.feature_path(out, "duration", e["basename"], "spk0", "l0", "duration.pt"), weights_only=True)
        mel = torch.load(D.feature_path(corpus, "spec", e["basename"], "spk0", "l0",
                                        f"spec-{audio.input_sampling_rate}-{audio.spec_type}.pt"), weights_only=True)
        assert dur.dim() == 1 and not dur.is_floating_point() and int(dur.sum()) == mel.shape[1]
        assert torch.equal(dur.int(), torch.load(apath, weights_only=True)["duration"])
    # round trip: a learn_alignment: false model (frame-level pitch / energy: the corpus's own files) trains on them
    for kind in ("spec", "pitch", "energy"):
        shutil.copytree(corpus / kind, out / kind)
    cfg2 = C.small_config(learn_alignment=False, level="frame")
    cfg2.text = cfg.text
    cfg2.preprocessing.save_dir = str(out)
    fixed = D.FeatureDataset(entries, cfg2, C.LANG2ID, C.SPEAKER2ID)
    batch = D.collate([fixed[i] for i in range(3)], learn_alignment=False)
    assert batch["duration"].shape == batch["text"].shape
    student = _model(cfg2)
    student.train()
    total = float(student.training_step(batch).detach())
    losses = student.losses_to_host()
    print("fixed-duration model trained on the exported durations:", losses)
    assert torch.isfinite(torch.tensor([total, float(losses["total"])])).all() and total > 0


def _dry_run(capsys, argv):
    capsys.readouterr()
    assert cli.main(argv + ["--dry-run"]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_the_command_writes_what_the_dry_run_names(tmp_path, capsys):
    from tests.test_synthesize_gpu import _build
    cfg = C.small_config(learn_alignment=True)
    corpus, entries, fl = _corpus(tmp_path, cfg, True)
    ckpt = tmp_path / "la.ckpt"
    _build(cfg).save_checkpoint(ckpt, global_step=9)
    base = ["synthesize", str(ckpt), "-f", str(fl), "-T", str(corpus), "-b", "2"]

    def listing(out, kind):
        return sorted(str(p) for p in (out / kind).iterdir()) if (out / kind).exists() else []

    plain, flagged, scored = tmp_path / "plain", tmp_path / "flagged", tmp_path / "scored"
    assert cli.main(base + ["-o", str(plain)]) == 0
    assert not (plain / "synthesized_alignment").exists() and not (plain / "duration").exists()
    plan = _dry_run(capsys, base + ["-o", str(flagged), "--write-alignments"])
    assert cli.main(base + ["-o", str(flagged), "--write-alignments"]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["alignment_files"] == len(entries) == len(plan["alignment_files"]) == report["files"]
    assert listing(flagged, "synthesized_alignment") == sorted(plan["alignment_files"])
    assert listing(flagged, "duration") == sorted(plan["duration_files"])
    assert listing(flagged, "synthesized_spec") == sorted(plan["files"])
    names = [p.name for p in sorted((plain / "synthesized_spec").iterdir())]
    assert names == [p.name for p in sorted((flagged / "synthesized_spec").iterdir())] and len(names) == len(entries)
    for n in names:   # the spectrogram files do not change with the flag
        assert (plain / "synthesized_spec" / n).read_bytes() == (flagged / "synthesized_spec" / n).read_bytes()
    # with scores and without spectrograms
    extra = ["-o", str(scored), "--write-alignments", "--return-scores", "--scores-only"]
    plan = _dry_run(capsys, base + extra)
    assert cli.main(base + extra) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plan["files"] == [] and report["files"] == 0 and report["alignment_files"] == len(entries)
    assert not (scored / "synthesized_spec").exists() and (scored / "scores-9.psv").exists() == (plan["scores_file"] != "")
    assert listing(scored, "synthesized_alignment") == sorted(plan["alignment_files"])
    assert listing(scored, "duration") == sorted(plan["duration_files"])
    rec = torch.load(plan["alignment_files"][0], weights_only=True)
    assert rec["duration_source"] == "aligner" and int(rec["duration"].sum()) == rec["frames"]
