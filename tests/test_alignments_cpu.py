"""CPU: the host side of ``fs2l synthesize --write-alignments`` -- the parser flag, ``AlignmentWriter`` on hand-made packed
buffers (input-order release, chunk concatenation, the clip rule, the file format), ``TextProcessor.decode_tokens`` and
``--dry-run``."""
import json

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd.config import TextProcessor
from oracle import cases as C

SYMBOLS = TextProcessor(C.small_config(learn_alignment=False).text).symbols


def test_parser_flag_and_its_default():
    p = cli.build_parser()
    assert p.parse_args(["synthesize", "m.ckpt", "-t", "x"]).write_alignments is False
    a = p.parse_args(["synthesize", "m.ckpt", "-t", "x", "--write-alignments", "-T", "tf", "--return-scores", "--scores-only",
                      "--exact-lengths"])
    assert a.write_alignments and a.return_scores and a.scores_only and a.exact_lengths
    with pytest.raises(SystemExit):   # -O stays as it is: the TextGrid writer is not part of this project
        p.parse_args(["synthesize", "m.ckpt", "-t", "x", "--write-alignments", "-O", "textgrid"])


def test_decode_tokens_inverts_the_encoders():
    tp = TextProcessor(C.small_config(learn_alignment=False).text)
    ids = tp.encode_text("cab")
    assert tp.decode_tokens(ids) == ["c", "a", "b"] == tp.decode_tokens(torch.tensor(ids, dtype=torch.int32))
    assert tp.decode_tokens(tp.encode_escaped_string_sequence("w/a")) == ["w", "a"]
    assert tp.decode_tokens([]) == [] and tp.decode_tokens([0]) == [tp.symbols[0]]
    with pytest.raises(ValueError, match="symbol table"):
        tp.decode_tokens([len(tp.symbols)])
    with pytest.raises(ValueError, match="symbol table"):
        tp.decode_tokens([-1])


def _pack(utts, levels=("phone", "frame"), lead=3):
    """A packed host buffer as ``synthesize`` lays it out, by hand.  ``utts``: [(token ids, durations, frames)].  Returns
    (packed fp32, members, batch pieces, the per-utterance pitch / energy values)."""
    dur = [torch.tensor(d, dtype=torch.int32) for _, d, _ in utts]
    n_of = {"phone": [len(t) for t, _, _ in utts], "frame": [f for _, _, f in utts]}
    g = torch.Generator().manual_seed(len(utts))
    pitch = [torch.randn(n, generator=g) for n in n_of[levels[0]]]
    energy = [torch.randn(n, generator=g) for n in n_of[levels[1]]]
    parts, members, at = [torch.full((lead,), float("nan"))], {}, lead   # (members need not start at element 0)
    for name, rows, level in (("duration", dur, "phone"), ("pitch", pitch, levels[0]), ("energy", energy, levels[1])):
        offsets = [0]
        for r in rows:
            offsets.append(offsets[-1] + r.numel())
        members[name] = (at, offsets, level)
        parts += [r.view(torch.float32) if r.dtype == torch.int32 else r for r in rows]
        at += offsets[-1]
    Ts = max(len(t) for t, _, _ in utts)
    text = torch.zeros(len(utts), Ts, dtype=torch.int32)
    for b, (t, _, _) in enumerate(utts):
        text[b, :len(t)] = torch.tensor(t, dtype=torch.int32)
    return torch.cat(parts), members, text, pitch, energy


def _batch(text, raw, last=None, names=None):
    B = len(raw)
    return {"text": text, "raw_text": raw, "speaker": ["spk0"] * B, "language": ["l0"] * B,
            "is_last_input_chunk": last or [True] * B, "basename": names or [f"u{i}" for i in range(B)]}


def test_files_are_released_in_input_order_and_load_with_weights_only(tmp_path):
    w = D.AlignmentWriter(tmp_path, 11, SYMBOLS)
    assert w.dir == tmp_path / "synthesized_alignment" and w.pending() == 0
    # positions 2 and 1 arrive first (a length-sorted batch), position 0 later
    utts_a = [([3, 1, 2], [2, 0, 3], 5), ([4, 4], [1, 1], 2)]
    packed, members, text, pitch, energy = _pack(utts_a)
    sentinel = packed.clone()
    assert w.write_packed(packed, members, _batch(text, ["second text", "third text"]), [1, 2], [5, 2]) == []
    assert w.pending() == 2
    packed.fill_(123.0)   # the caller reuses its pinned buffer: every piece was cloned out of it
    with pytest.raises(ValueError, match="delivered twice"):
        w.write_packed(sentinel, members, _batch(text, ["second text", "third text"]), [2, 3], [5, 2])
    utts_b = [([5], [4], 4)]
    packed_b, members_b, text_b, pitch_b, energy_b = _pack(utts_b)
    files = w.write_packed(packed_b, members_b, _batch(text_b, ["first text"]), [0], [4])
    assert w.pending() == 0
    assert [p.name for p in files] == [f"{D.truncate_basename(D.slugify(t))}--spk0--l0--ckpt=11--alignment.pt"
                                       for t in ("first text", "second text", "third text")]
    assert all(p.parent == w.dir for p in files)
    with pytest.raises(ValueError, match="delivered twice"):
        w.write_packed(packed_b, members_b, _batch(text_b, ["first text"]), [0], [4])
    rec = torch.load(files[1], weights_only=True)
    assert sorted(rec) == ["duration", "duration_source", "energy", "energy_level", "frames", "pitch", "pitch_level",
                           "raw_text", "symbols", "text"]
    assert rec["text"].dtype == torch.int32 and rec["text"].tolist() == [3, 1, 2]
    assert rec["symbols"] == [SYMBOLS[3], SYMBOLS[1], SYMBOLS[2]]
    assert rec["duration"].dtype == torch.int32 and rec["duration"].tolist() == [2, 0, 3] and rec["frames"] == 5
    assert torch.equal(rec["pitch"], pitch[0]) and rec["pitch_level"] == "phone" and rec["pitch"].dtype == torch.float32
    assert torch.equal(rec["energy"], energy[0]) and rec["energy_level"] == "frame" and rec["energy"].numel() == 5
    assert rec["duration_source"] == "predicted" and rec["raw_text"] == "second text"
    assert torch.load(files[0], weights_only=True)["duration"].tolist() == [4]
    assert not (tmp_path / "duration").exists() and w.duration_files == []


def test_chunks_of_one_text_are_concatenated(tmp_path):
    w = D.AlignmentWriter(tmp_path, 0, TextProcessor(C.small_config(learn_alignment=False).text))   # (the processor itself)
    utts = [([1, 2], [1, 2], 3), ([3], [2], 2), ([4, 5], [1, 1], 2)]
    packed, members, text, pitch, energy = _pack(utts)
    # positions 0 + 1 are two chunks of one text; the second chunk arrives first and is held
    last = [False, True, True]
    sub = {k: (s, o[1:], lvl) for k, (s, o, lvl) in members.items()}
    sub = {k: (s + o[0], [x - o[0] for x in o], lvl) for k, (s, o, lvl) in sub.items()}
    assert w.write_packed(packed, sub, _batch(text[1:], ["b c", "tail"], last[1:]), [1, 2], [2, 2], "given") == []
    assert w.pending() == 2
    first = {k: (s, o[:2], lvl) for k, (s, o, lvl) in members.items()}
    files = w.write_packed(packed, first, _batch(text[:1], ["a "], last[:1]), [0], [3], "given")
    assert [p.name for p in files] == [f"{D.truncate_basename(D.slugify(t))}--spk0--l0--ckpt=0--alignment.pt"
                                       for t in ("a b c", "tail")] and w.pending() == 0
    rec = torch.load(files[0], weights_only=True)
    assert rec["text"].tolist() == [1, 2, 3] and rec["duration"].tolist() == [1, 2, 2] and rec["frames"] == 5
    assert rec["symbols"] == [SYMBOLS[1], SYMBOLS[2], SYMBOLS[3]] and rec["raw_text"] == "a b c"
    assert torch.equal(rec["pitch"], torch.cat(pitch[:2])) and rec["pitch"].numel() == 3      # along the tokens
    assert torch.equal(rec["energy"], torch.cat(energy[:2])) and rec["energy"].numel() == 5   # along the frames
    assert rec["duration_source"] == "given"
    # a text whose last chunk never arrives stays pending
    w2 = D.AlignmentWriter(tmp_path / "open", 0, SYMBOLS)
    assert w2.write_packed(packed, first, _batch(text[:1], ["a "], [False]), [0], [3]) == [] and w2.pending() == 1


def test_the_clip_rule(tmp_path):
    assert D.AlignmentWriter.clip(torch.tensor([3, 2, 4, 1]), 6).tolist() == [3, 2, 1, 0]
    assert D.AlignmentWriter.clip(torch.tensor([3, 2, 4, 1]), 10).tolist() == [3, 2, 4, 1]
    assert D.AlignmentWriter.clip(torch.tensor([3, 2, 4, 1]), 0).tolist() == [0, 0, 0, 0]
    assert D.AlignmentWriter.clip(torch.tensor([0, 5]), 5).dtype == torch.int32
    w = D.AlignmentWriter(tmp_path, 3, SYMBOLS)
    utts = [([1, 2, 3, 4], [3, 2, 4, 1], 6), ([5, 6], [2, 2], 4)]   # the first was cut at 6 of its 10 frames
    packed, members, text, pitch, energy = _pack(utts, levels=("frame", "phone"))
    files = w.write_packed(packed, members, _batch(text, ["cut", "whole"]), [0, 1], [6, 4])
    cut, whole = (torch.load(p, weights_only=True) for p in files)
    assert cut["duration"].tolist() == [3, 2, 1, 0] and cut["frames"] == 6 == int(cut["duration"].sum())
    assert cut["pitch"].numel() == 6 and cut["energy"].numel() == 4 and cut["text"].tolist() == [1, 2, 3, 4]
    assert whole["duration"].tolist() == [2, 2] and whole["frames"] == 4
    # more frames than the durations give is not a clip: refused
    with pytest.raises(ValueError, match="add up"):
        D.AlignmentWriter(tmp_path / "bad", 3, SYMBOLS).write_packed(packed, members, _batch(text, ["cut", "whole"]), [0, 1], [11, 4])


def test_duration_files_for_a_fixed_duration_model(tmp_path):
    w = D.AlignmentWriter(tmp_path, 3, SYMBOLS)
    utts = [([1, 2, 3], [3, 2, 4], 9), ([5, 6], [2, 2], 4)]
    packed, members, text, _, _ = _pack(utts, levels=("frame", "frame"))
    files = w.write_packed(packed, members, _batch(text, ["one", "two"], names=["LJ001", "LJ002"]), [0, 1], [9, 4],
                           duration_source="aligner", duration_files=True)
    assert [p.name for p in w.duration_files] == ["LJ001--spk0--l0--duration.pt", "LJ002--spk0--l0--duration.pt"]
    assert all(p.parent == tmp_path / "duration" for p in w.duration_files)
    assert w.duration_files[0] == D.feature_path(tmp_path, "duration", "LJ001", "spk0", "l0", "duration.pt")
    d = torch.load(w.duration_files[0], weights_only=True)
    assert d.dtype == torch.int64 and d.tolist() == [3, 2, 4]
    assert torch.load(files[0], weights_only=True)["duration_source"] == "aligner"


def test_malformed_members_are_refused(tmp_path):
    w = D.AlignmentWriter(tmp_path, 3, SYMBOLS)
    packed, members, text, _, _ = _pack([([1, 2], [1, 1], 2)])
    batch = _batch(text, ["x"])
    with pytest.raises(ValueError, match="duration_source"):
        w.write_packed(packed, members, batch, [0], [2], duration_source="guessed")
    with pytest.raises(ValueError, match="duration, pitch and energy"):
        w.write_packed(packed, {k: v for k, v in members.items() if k != "pitch"}, batch, [0], [2])
    with pytest.raises(ValueError, match="level"):
        w.write_packed(packed, dict(members, pitch=members["pitch"][:2] + ("word",)), batch, [0], [2])
    with pytest.raises(ValueError, match="frame counts"):
        w.write_packed(packed, members, batch, [0], [2, 2])
    with pytest.raises(ValueError, match="do not delimit"):
        w.write_packed(packed[:4], members, batch, [0], [2])
    with pytest.raises(ValueError, match="values at the"):   # two pitch values at the frame level need two frames
        w.write_packed(packed, dict(members, pitch=members["pitch"][:2] + ("frame",)), batch, [0], [1])
    with pytest.raises(ValueError, match="symbol table"):
        D.AlignmentWriter(tmp_path, 3, None)
    assert w.pending() == 0


def test_synthesize_needs_something_to_write():
    from fastspeech2_lightning_amd.synthesis import _Slot, synthesize
    with pytest.raises(ValueError, match="nothing to write"):
        synthesize(None, None, 2)
    # the header's earlier form is unchanged; the members' offset tables come on top
    assert _Slot.header(3) == 8 and _Slot.header(3, True) == 8 + 24 and _Slot.header(3, scored=True, members=3) == 32 + 24
    assert _Slot.header(4, members=3) == 4 * 12 and _Slot.header(4, members=3) % 4 == 0


def _stub_checkpoint(path, learn_alignment, step=7):
    cfg = C.small_config(learn_alignment=learn_alignment)
    torch.save({"global_step": step, "hyper_parameters": {"config": cfg.model_checkpoint_dump(), "stats": C.STATS,
                                                          "lang2id": dict(C.LANG2ID), "speaker2id": dict(C.SPEAKER2ID)}}, path)
    return path


def _dry(capsys, argv):
    capsys.readouterr()
    assert cli.main(argv + ["--dry-run"]) == 0
    return capsys.readouterr().out


def test_dry_run_names_the_files_only_with_the_flag(tmp_path, capsys):
    ckpt = _stub_checkpoint(tmp_path / "m.ckpt", learn_alignment=False)
    base = ["synthesize", str(ckpt), "-t", "abc", "-t", "fed cba", "-o", str(tmp_path / "out")]
    plain = json.loads(_dry(capsys, base))
    assert "alignment_files" not in plain and "duration_files" not in plain
    assert sorted(plain) == sorted(["checkpoint", "global_step", "output_dir", "utterances", "batch_size", "sort",
                                    "exact_lengths", "return_scores", "attn_prior", "token_counts", "dropped_symbols",
                                    "batches", "entries", "files"])
    flagged = json.loads(_dry(capsys, base + ["--write-alignments"]))
    assert {k: v for k, v in flagged.items() if k != "alignment_files"} == plain
    assert flagged["alignment_files"] == [
        str(tmp_path / "out" / "synthesized_alignment" / f"{D.truncate_basename(D.slugify(t))}--spk0--l0--ckpt=7--alignment.pt")
        for t in ("abc", "fed cba")]
    assert "duration_files" not in flagged   # free synthesis: nobody aligned anything


def test_dry_run_names_the_duration_files_under_teacher_forcing_with_a_learned_aligner(tmp_path, capsys):
    fl = tmp_path / "list.psv"
    fl.write_text("basename|characters|language|speaker\nLJ001|abc|l0|spk0\nLJ002|cab fed|l0|spk0\n", encoding="utf8")
    for learn_alignment in (True, False):
        ckpt = _stub_checkpoint(tmp_path / f"m{learn_alignment}.ckpt", learn_alignment)
        argv = ["synthesize", str(ckpt), "-f", str(fl), "-T", str(tmp_path / "tf"), "-o", str(tmp_path / "out"),
                "--write-alignments", "--return-scores", "--scores-only"]
        plan = json.loads(_dry(capsys, argv))
        assert plan["files"] == [] and len(plan["alignment_files"]) == 2 and plan["scores_file"].endswith("scores-7.psv")
        if learn_alignment:
            assert plan["duration_files"] == [str(tmp_path / "out" / "duration" / f"{b}--spk0--l0--duration.pt")
                                              for b in ("LJ001", "LJ002")]
        else:
            assert "duration_files" not in plan
        without = json.loads(_dry(capsys, [a for a in argv if a != "--write-alignments"]))
        assert "alignment_files" not in without and "duration_files" not in without
