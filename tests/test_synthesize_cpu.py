"""CPU: the host side of ``fs2l synthesize`` -- parser, entries from text / filelists, the inference items of
``SynthesisDataset``, batch composition, the packed writer's input-order / chunk logic, and ``--dry-run``."""
import json
from types import SimpleNamespace

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from oracle import cases as C

FEATURE_KEYS = ["mel", "mel_style_reference", "duration", "duration_control", "pfs", "text", "raw_text", "basename",
                "speaker", "speaker_id", "language", "language_id", "energy", "pitch", "is_last_input_chunk"]


def _tables(multispeaker=False, **kw):
    cfg = C.small_config(learn_alignment=False, multispeaker=multispeaker, **kw)
    return SimpleNamespace(config=cfg, lang2id=dict(C.LANG2ID), speaker2id=dict(C.SPEAKER2ID))


def _stub_checkpoint(path, step=7, **kw):
    """A checkpoint with everything but weights: what ``--dry-run`` reads."""
    m = _tables(**kw)
    torch.save({"global_step": step, "hyper_parameters": {"config": m.config.model_checkpoint_dump(), "stats": C.STATS,
                                                          "lang2id": m.lang2id, "speaker2id": m.speaker2id}}, path)
    return path


# ---- parser ----------------------------------------------------------------------------------------------------------
def test_parser_takes_every_reference_short_option(tmp_path):
    a = cli.build_parser().parse_args(
        ["synthesize", "m.ckpt", "-t", "abc", "-t", "de", "-f", "list.psv", "-o", str(tmp_path), "-l", "l1", "-s", "spk2",
         "-D", "1.5", "--pitch-control", "0.8", "--energy-control", "1.1", "-S", "ref.pt", "-T", "tf", "-b", "3",
         "-O", "spec", "--text-representation", "phones", "--precision", "bf16-mixed", "--no-sort", "--dry-run"])
    assert a.command == "synthesize" and a.texts == ["abc", "de"] and str(a.filelist) == "list.psv"
    assert (a.language, a.speaker, a.duration_control, a.pitch_control, a.energy_control) == ("l1", "spk2", 1.5, 0.8, 1.1)
    assert str(a.style_reference) == "ref.pt" and str(a.teacher_forcing_directory) == "tf" and a.batch_size == 3
    assert a.output_type == ["spec"] and a.text_representation == "phones" and a.no_sort and a.dry_run
    d = cli.build_parser().parse_args(["synthesize", "m.ckpt", "-t", "x"])
    assert d.batch_size == 4 and d.duration_control == 1.0 and str(d.output_dir) == "synthesis_output" and not d.no_sort


@pytest.mark.parametrize("kind", ["wav", "textgrid", "readalong-xml", "readalong-html"])
def test_other_output_types_are_refused_naming_what_they_need(kind, capsys):
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["synthesize", "m.ckpt", "-t", "x", "-O", kind])
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert kind in err and ("vocoder" in err or "parent toolkit" in err)


def test_neither_text_nor_filelist_exits_with_status_1(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["synthesize", "m.ckpt"])
    assert e.value.code == 1
    assert "You must define either --text or --filelist" in capsys.readouterr().err


def test_style_reference_must_be_a_pt_file(tmp_path):
    with pytest.raises(SystemExit, match="preprocessor"):
        cli.main(["synthesize", str(tmp_path / "m.ckpt"), "-t", "abc", "-S", "ref.wav", "--dry-run"])


# ---- synthesis_entries -----------------------------------------------------------------------------------------------
def test_entries_from_a_psv_filelist(tmp_path):
    fl = tmp_path / "list.psv"
    fl.write_text("basename|characters|language|speaker\nu1|abc def|l1|spk2\n|fed cba|l0|spk0\n", encoding="utf8")
    es = D.synthesis_entries([], fl, None, None, 1.25, _tables(multispeaker=True))
    assert [e["basename"] for e in es] == ["u1", D.truncate_basename(D.slugify("fed cba"))]
    assert [(e["characters"], e["language"], e["speaker"]) for e in es] == [("abc def", "l1", "spk2"), ("fed cba", "l0", "spk0")]
    assert all(e["is_last_input_chunk"] is True and e["duration_control"] == 1.25 for e in es)
    # --language / --speaker override the rows'
    es = D.synthesis_entries(None, fl, "l0", "spk1", 1.0, _tables(multispeaker=True))
    assert {(e["language"], e["speaker"]) for e in es} == {("l0", "spk1")}


def test_entries_from_plain_text_lines(tmp_path):
    fl = tmp_path / "lines.txt"
    fl.write_text("abc def\n   padded line  \nghi\n", encoding="utf8")
    es = D.synthesis_entries([], fl, None, None, 1.0, _tables())
    assert [e["characters"] for e in es] == ["abc def", "padded line", "ghi"]
    assert [e["basename"] for e in es] == [D.truncate_basename(D.slugify(t)) for t in ("abc def", "padded line", "ghi")]
    # defaults: the first keys of the model's tables
    assert {(e["language"], e["speaker"]) for e in es} == {("l0", "spk0")}


def test_text_wins_over_filelist_with_a_note(tmp_path, capsys):
    fl = tmp_path / "lines.txt"
    fl.write_text("from the file\n", encoding="utf8")
    es = D.synthesis_entries(["from the option"], fl, None, None, 1.0, _tables())
    assert [e["characters"] for e in es] == ["from the option"]
    assert "this will only process the text" in capsys.readouterr().err


def test_unknown_speaker_on_a_multispeaker_model_is_named():
    with pytest.raises(SystemExit, match="nobody"):
        D.synthesis_entries(["abc"], None, None, "nobody", 1.0, _tables(multispeaker=True))
    with pytest.raises(SystemExit, match="l9"):
        D.synthesis_entries(["abc"], None, "l9", None, 1.0, _tables(multispeaker=True))


# ---- SynthesisDataset ------------------------------------------------------------------------------------------------
def test_items_have_the_training_items_keys_and_no_targets(capsys):
    m = _tables()
    es = D.synthesis_entries(["abc def", "w"], None, None, None, 1.5, m)
    ds = D.SynthesisDataset(es, m.config, m.lang2id, m.speaker2id)
    item = ds[0]
    assert list(item) == FEATURE_KEYS
    assert all(item[k] is None for k in ("mel", "duration", "energy", "pitch", "mel_style_reference", "pfs"))
    assert item["is_last_input_chunk"] is True and item["duration_control"] == 1.5 and item["raw_text"] == "abc def"
    assert item["text"].dtype == torch.int32 and ds.token_counts == [6, 1]   # the blank is not in the table: dropped
    assert "1 input symbol" in capsys.readouterr().err
    batch = D.collate([ds[0], ds[1]], learn_alignment=False)
    assert batch["mel_lens"] is None and batch["max_mel_len"] == 1_000_000
    assert batch["text"].shape == (2, 6) and batch["src_lens"].tolist() == [6, 1]
    assert batch["is_last_input_chunk"] == [True, True]


def test_feature_dataset_key_order_is_the_yardstick(tmp_path):
    """``FEATURE_KEYS`` above is ``FeatureDataset.__getitem__``'s key list, read from a real item."""
    cfg = C.small_config(learn_alignment=False)
    cfg.preprocessing.save_dir = str(tmp_path)
    audio = cfg.preprocessing.audio
    files = {("spec", f"spec-{audio.input_sampling_rate}-{audio.spec_type}.pt"): torch.zeros(audio.n_mels, 4),
             ("duration", "duration.pt"): torch.tensor([2, 2]), ("energy", "energy.pt"): torch.zeros(2),
             ("pitch", "pitch.pt"): torch.zeros(2)}
    for (kind, fn), t in files.items():
        p = D.feature_path(tmp_path, kind, "u", "spk0", "l0", fn)
        p.parent.mkdir(exist_ok=True)
        torch.save(t, p)
    e = {"basename": "u", "speaker": "spk0", "language": "l0", "character_tokens": "a/b", "characters": "ab"}
    assert list(D.FeatureDataset([e], cfg, C.LANG2ID, C.SPEAKER2ID)[0]) == FEATURE_KEYS
    # teacher forcing: the same files through SynthesisDataset
    item = D.SynthesisDataset([e], cfg, C.LANG2ID, C.SPEAKER2ID, teacher_forcing_dir=tmp_path)[0]
    assert list(item) == FEATURE_KEYS and item["mel"].shape == (4, audio.n_mels) and item["duration"].tolist() == [2, 2]
    assert item["energy"] is None and item["pitch"] is None


def test_token_column_and_raw_text_agree():
    m = _tables()
    a = D.SynthesisDataset([{"basename": "x", "characters": "hello", "character_tokens": "h/e/l/l/o"}], m.config, m.lang2id,
                           m.speaker2id)
    b = D.SynthesisDataset([{"basename": "x", "characters": "hello"}], m.config, m.lang2id, m.speaker2id)
    assert a[0]["text"].tolist() == b[0]["text"].tolist() and len(a[0]["text"]) == 5
    assert a.dropped == 0 and b.dropped == 0


def test_a_text_of_unknown_symbols_only_raises():
    m = _tables()
    with pytest.raises(ValueError, match="nothing-here"):
        D.SynthesisDataset([{"basename": "nothing-here", "characters": "123 !?"}], m.config, m.lang2id, m.speaker2id)


def test_style_reference_and_pfs_rules():
    m = _tables()
    with pytest.raises(ValueError, match="global style token"):
        D.SynthesisDataset([{"basename": "x", "characters": "abc"}], m.config, m.lang2id, m.speaker2id,
                           style_reference=torch.zeros(16, 9))
    g = _tables(gst=True, n_mels=80)
    ds = D.SynthesisDataset([{"basename": "x", "characters": "abc"}], g.config, g.lang2id, g.speaker2id,
                            style_reference=torch.arange(80 * 9, dtype=torch.float32).reshape(80, 9))
    ref = ds[0]["mel_style_reference"]
    assert ref.shape == (9, 80) and ref[2, 5] == 5 * 9 + 2
    with pytest.raises(ValueError, match="n_mels"):
        D.SynthesisDataset([{"basename": "x", "characters": "abc"}], g.config, g.lang2id, g.speaker2id,
                           style_reference=torch.zeros(16, 9))
    dump = m.config.model_checkpoint_dump()
    dump["model"]["target_text_representation_level"] = "phonological_features"
    from fastspeech2_lightning_amd.config import FastSpeech2Config
    with pytest.raises(ValueError, match="parent toolkit"):
        D.SynthesisDataset([{"basename": "x", "phones": "abc"}], FastSpeech2Config(**dump), m.lang2id, m.speaker2id)


# ---- synthesis_batches -----------------------------------------------------------------------------------------------
def test_batches_sorted_longest_first_and_stable():
    counts = [3, 9, 1, 9, 4, 2, 7]
    got = D.synthesis_batches(counts, 3)
    assert sorted(i for b in got for i in b) == list(range(7))
    flat = [i for b in got for i in b]
    assert flat.index(1) < flat.index(3)       # stable among the two 9s
    assert got == [[1, 3, 6], [4, 0, 5], [2]]
    assert D.synthesis_batches(counts, 3, sort=False) == [[0, 1, 2], [3, 4, 5], [6]]


# ---- PackedSpecWriter ------------------------------------------------------------------------------------------------
def test_packed_writer_restores_input_order_and_joins_chunks(tmp_path):
    n_mels = 4
    g = torch.Generator().manual_seed(3)
    frames = [5, 2, 7, 3]                       # text 0 | text 1 chunk a, chunk b | text 2
    specs = [torch.randn(n_mels, n, generator=g) for n in frames]
    texts, last = ["first text", "middle ", "part two", "last text"], [True, False, True, True]

    def packed(ids):
        offs = [0]
        for i in ids:
            offs.append(offs[-1] + n_mels * frames[i])
        buf = torch.cat([specs[i].reshape(-1) for i in ids] + [torch.full((11,), 9e9)])  # (slack behind the payload)
        batch = {"raw_text": [texts[i] for i in ids], "speaker": ["spk0"] * len(ids), "language": ["l0"] * len(ids),
                 "is_last_input_chunk": [last[i] for i in ids]}
        return buf, torch.tensor(offs), batch, ids

    w = D.PackedSpecWriter(tmp_path, "postnet_output", global_step=12, n_mels=n_mels)
    first = w.write_packed(*packed([2, 3]))    # the long chunk and the last text arrive first: nothing can be written
    assert first == [] and w.pending() == 2
    second = w.write_packed(*packed([0, 1]))
    assert w.pending() == 0
    names = [p.name for p in second]
    ref = D.SpecWriter(tmp_path, "postnet_output", global_step=12)
    assert names == [ref.filename(D.truncate_basename(D.slugify(t)), "spk0", "l0").name
                     for t in ("first text", "middle part two", "last text")]
    got = [torch.load(p, weights_only=True) for p in second]
    assert torch.equal(got[0], specs[0]) and torch.equal(got[2], specs[3])
    assert torch.equal(got[1], torch.cat([specs[1], specs[2]], -1))
    assert all(t.is_contiguous() and t.dtype == torch.float32 and t.shape[0] == n_mels for t in got)
    assert all(t.untyped_storage().nbytes() == t.numel() * 4 for t in got)   # a file holds its tensor, not the batch buffer
    with pytest.raises(ValueError, match="twice"):
        w.write_packed(*packed([0]))


# ---- --dry-run -------------------------------------------------------------------------------------------------------
def test_dry_run_prints_entries_batches_and_file_names(tmp_path, capsys):
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt", step=41)
    texts = ["abc", "abcdefghi", "a", "ihgfedcba", "abcd", "ab", "abcdefg"]
    argv = ["synthesize", str(ckpt), "-o", str(tmp_path / "out"), "-b", "3", "--dry-run"]
    for t in texts:
        argv += ["-t", t]
    assert cli.main(argv) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rep["global_step"] == 41 and rep["utterances"] == 7 and rep["token_counts"] == [3, 9, 1, 9, 4, 2, 7]
    assert rep["batches"] == [[1, 3, 6], [4, 0, 5], [2]] and rep["sort"] is True
    ref = D.SpecWriter.__new__(D.SpecWriter)
    ref.dir, ref.global_step, ref.suffix = tmp_path / "out" / "synthesized_spec", 41, "spec-pred-22050-mel-librosa.pt"
    assert rep["files"] == [str(ref.filename(D.truncate_basename(D.slugify(t)), "spk0", "l0")) for t in texts]
    assert not (tmp_path / "out").exists()      # nothing is written
    assert cli.main(argv + ["--no-sort"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["batches"] == [[0, 1, 2], [3, 4, 5], [6]]


def test_characters_model_refuses_phones(tmp_path):
    ckpt = _stub_checkpoint(tmp_path / "stub.ckpt")
    with pytest.raises(ValueError, match="incompatible"):
        cli.main(["synthesize", str(ckpt), "-t", "abc", "--text-representation", "phones", "--dry-run"])
