"""GPU: per-utterance loss scores (``FastSpeech2.utterance_losses``, ``synthesize(..., scores=...)``, ``fs2l synthesize
--return-scores``).

The yardstick is the CPU oracle run ONE UTTERANCE AT A TIME with its own loss on top -- the reference's scorer, which runs at
batch size 1.  A ragged teacher-forced batch must reproduce those numbers row by row within the project's loss bound,
``1e-4 * max(1, |ref|)``; the batch-level ``model.loss`` must NOT (it differs from every row's total by more than 1e-2),
which keeps the inputs from becoming so benign that the comparison proves nothing.
"""
import csv

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd.config import InferenceControl, TextConfig
from fastspeech2_lightning_amd.model import LOSS_KEYS
from oracle import cases as C
from oracle import fs2_oracle as O

pytestmark = pytest.mark.gpu

_REF = {}


def _bound(ref):
    return 1e-4 * max(1.0, abs(ref))


def _oracle_alone(learn_alignment):
    """The oracle's alone-runs of the three utterances of the seed-21 batch and their losses at epochs 0 and 7: computed
    once per configuration and shared."""
    from tests.test_exact_lengths_gpu import _pair, _row
    if learn_alignment not in _REF:
        cfg = C.small_config(learn_alignment=learn_alignment)
        model, oracle = _pair(cfg)
        batch = O.synthetic_batch(**C._KW, seed=21, learn_alignment=learn_alignment)
        ref = {}
        with torch.no_grad():
            for j in range(3):
                row = _row(batch, j, learn_alignment)
                out = oracle(row, inference=True)
                for e in (0, 7):
                    ref[j, e] = {k: float(v) for k, v in oracle.loss(out, row, e).items()}
        _REF[learn_alignment] = (model, batch, ref)
    return _REF[learn_alignment]


@pytest.mark.parametrize("learn_alignment", [False, True], ids=["given_durations", "learned_alignment"])
def test_rows_of_a_batch_equal_the_oracle_alone(learn_alignment):
    model, batch, ref = _oracle_alone(learn_alignment)
    want_keys = ("duration", "spec", "postnet") + (("attn_ctc", "attn_bin") if learn_alignment else ())
    out = model(dict(batch), inference=True, exact_lengths=True)
    for e in (0, 7):
        table, keys = model.utterance_losses(out, dict(batch), current_epoch=e)
        assert keys == want_keys and tuple(table.shape) == (3, len(LOSS_KEYS) + 1) and table.is_cuda
        got = table.cpu()
        assert torch.isfinite(got).all()
        batch_total = float(model.loss(out, model.prepare_batch(dict(batch)), e)["total"])
        worst = 0.0
        for j in range(3):
            r = ref[j, e]
            assert tuple(k for k in r if k != "total") == want_keys
            row = {k: float(got[j, LOSS_KEYS.index(k)]) for k in keys}
            row["total"] = float(got[j, -1])
            print(f"learn_alignment={learn_alignment} epoch {e} utterance {j}: "
                  + ", ".join(f"{k} {row[k]:.6f} ({r[k]:.6f})" for k in row) + f"; the batch's total {batch_total:.6f}")
            for k in row:
                worst = max(worst, abs(row[k] - r[k]) / _bound(r[k]))
            for k in row:
                assert abs(row[k] - r[k]) <= _bound(r[k]), (e, j, k, row[k], r[k])
            for k in LOSS_KEYS:
                if k not in keys:
                    assert float(got[j, LOSS_KEYS.index(k)]) == 0.0
            # one number per batch is not a score of any utterance
            assert abs(batch_total - r["total"]) > 1e-2, (e, j, batch_total, r["total"])
        print(f"learn_alignment={learn_alignment} epoch {e}: worst error / bound {worst:.4f}")
    if learn_alignment:   # the binarisation weight follows the epoch: 0 at epoch 0, as under the reference's Trainer.predict
        assert all(ref[j, 0]["attn_bin"] == 0.0 and ref[j, 7]["attn_bin"] > 0.0 for j in range(3))


def test_refusals():
    model, batch, _ = _oracle_alone(False)
    out = model(dict(batch), inference=True, exact_lengths=True)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.utterance_losses(out, dict(batch))
    finally:
        model.eval()
    free = dict(batch, mel=None, mel_lens=None, duration=None, max_mel_len=1_000_000)
    with pytest.raises(ValueError, match="duration_target"):
        model.utterance_losses(model(free, InferenceControl(), inference=True), dict(batch))
    from fastspeech2_lightning_amd.synthesis import synthesize
    from tests.test_synthesize_gpu import TEXTS, _build, _dataset
    small = _build(C.small_config(learn_alignment=False))
    with pytest.raises(ValueError, match="teacher-forced"):
        synthesize(small, _dataset(small, TEXTS), 2, None, None, scores=D.ScoreWriter("unused", 0))
    with pytest.raises(ValueError, match="PackedSpecWriter"):
        synthesize(small, _dataset(small, TEXTS), 2, None, None)


def _corpus(tmp_path, learn_alignment, n_utts=5):
    """A teacher-forcing corpus, its filelist, model and checkpoint, as tests/test_synthesize_gpu.py builds its own."""
    from tests.test_data_gpu import SYMBOLS, _write_corpus
    from tests.test_synthesize_gpu import _build
    cfg = C.small_config(learn_alignment=learn_alignment)
    cfg.text = TextConfig(symbols={"letters": SYMBOLS})
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    entries = _write_corpus(corpus, cfg, n_utts=n_utts, learn_alignment=learn_alignment)
    model = _build(cfg)
    ckpt = tmp_path / "tf.ckpt"
    model.save_checkpoint(ckpt, global_step=9)
    fl = tmp_path / "list.psv"
    cols = ["basename", "language", "speaker", "characters", "character_tokens"]
    fl.write_text("|".join(cols) + "\n" + "".join("|".join(e[c] for c in cols) + "\n" for e in entries), encoding="utf8")
    return model, ckpt, fl, corpus, entries


def _read(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.DictReader(f, delimiter="|"))


def test_scores_do_not_depend_on_batch_size_or_sort_order(tmp_path):
    """Through ``synthesize(..., scores=...)`` with the learned aligner (all five columns of the file), at batch sizes 1, 2
    and 3, sorted and in input order: the same numbers within the bound and the same order in the file.  ``exact_lengths``
    is left at its default: scoring forces it."""
    from fastspeech2_lightning_amd.synthesis import synthesize
    model, _, fl, corpus, entries = _corpus(tmp_path, learn_alignment=True)
    rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
    terms = ("total", "duration", "spec", "postnet", "attn_ctc", "attn_bin")
    runs = {}
    for batch_size in (1, 2, 3):
        for sort in (False, True):
            tag = f"b{batch_size}_{'sorted' if sort else 'input_order'}"
            ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, teacher_forcing_dir=corpus)
            writer = D.PackedSpecWriter(tmp_path / tag, model.output_key, 9, n_mels=16)
            scores = D.ScoreWriter(tmp_path / tag, 9)
            res = synthesize(model, ds, batch_size, None, writer, sort=sort, scores=scores)
            assert len(res["files"]) == len(entries) and len(scores.records) == len(entries)
            path = scores.close()
            assert path == tmp_path / tag / "scores-9.psv"
            runs[tag] = _read(path)
    base = runs["b1_input_order"]
    totals = sorted(float(r["total"]) for r in base)
    print("alone: totals", totals)
    assert min(b - a for a, b in zip(totals, totals[1:])) > 1e-3      # far enough apart for the order to be the scores'
    assert [float(r["total"]) for r in base] == sorted((float(r["total"]) for r in base), reverse=True)
    for tag, got in runs.items():
        assert [r["basename"] for r in got] == [r["basename"] for r in base], tag
        worst = 0.0
        for g, w in zip(got, base):
            for k in terms:
                a, b = float(g[k]), float(w[k])
                worst = max(worst, abs(a - b) / _bound(b))
                assert abs(a - b) <= _bound(b), (tag, g["basename"], k, a, b)
            assert g["trigram_coverage_score"] == w["trigram_coverage_score"]
            assert g["phone_coverage_score"] == w["phone_coverage_score"]
        print(f"{tag}: worst difference / bound {worst:.4f}")


def test_the_command_writes_the_score_file(tmp_path):
    model, ckpt, fl, corpus, entries = _corpus(tmp_path, learn_alignment=False)
    out = tmp_path / "out"
    assert cli.main(["synthesize", str(ckpt), "-f", str(fl), "-T", str(corpus), "-o", str(out), "-b", "2",
                     "--return-scores"]) == 0
    path = out / "scores-9.psv"
    assert path.read_text(encoding="utf8").splitlines()[0] == "|".join(D.ScoreWriter.FIELDS) == (
        "basename|speaker|language|total|trigram_coverage_score|duration|spec|postnet|attn_ctc|attn_bin|raw_text|"
        "phone_coverage_score")
    got = _read(path)
    assert len(got) == len(entries) and sorted(r["basename"] for r in got) == sorted(e["basename"] for e in entries)
    totals = [float(r["total"]) for r in got]
    assert totals == sorted(totals, reverse=True) and len(set(totals)) == len(totals)       # worst first
    by_name = {e["basename"]: e for e in entries}
    for r in got:
        assert r["attn_ctc"] == "" and r["attn_bin"] == ""                                  # no aligner: empty fields
        assert r["speaker"] == "spk0" and r["language"] == "l0" and r["raw_text"] == by_name[r["basename"]]["characters"]
        parts = float(r["duration"]) + float(r["spec"]) + float(r["postnet"])
        assert abs(parts - float(r["total"])) <= 1e-5 * max(1.0, abs(parts))
        assert float(r["phone_coverage_score"]) > 0
    assert len(list((out / "synthesized_spec").iterdir())) == len(entries)                  # the spectrograms as before
    # the numbers are those of the method on the batches the command ran
    rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, teacher_forcing_dir=corpus)
    want = {}
    for idx in D.synthesis_batches(ds.token_counts, 2, True):
        batch = D.collate([ds[i] for i in idx], learn_alignment=False)
        table, _ = model.utterance_losses(model(dict(batch), inference=True, exact_lengths=True), batch)
        for j, i in enumerate(idx):
            want[entries[i]["basename"]] = float(table[j, -1])
    for r in got:
        assert float(r["total"]) == want[r["basename"]]
    # scores only: the same file, no spectrogram directory
    only = tmp_path / "only"
    assert cli.main(["synthesize", str(ckpt), "-f", str(fl), "-T", str(corpus), "-o", str(only), "-b", "2",
                     "--return-scores", "--scores-only"]) == 0
    assert not (only / "synthesized_spec").exists()
    assert (only / "scores-9.psv").read_text(encoding="utf8") == path.read_text(encoding="utf8")
