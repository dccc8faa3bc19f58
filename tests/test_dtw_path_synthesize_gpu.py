"""GPU: the warping path through ``synthesize(..., compare=data.DtwWriter, paths=data.DtwPathWriter)`` and ``fs2l synthesize
--compare-to DIR --write-paths``, on the small model and on-disk corpus of tests/test_dtw_synthesize_gpu.py (shared with it:
built once), at two batch sizes.

Everything is an equality.  A path file is compared with the numpy restatement (tests/dtw_path_references.py) applied to
``hip.frame_dist`` of the WRITTEN spectrogram against the recording: the path is bit-defined by its cost matrix, the written
spectrogram is the forward's output byte for byte, and a box of ``frame_dist`` does not depend on the batch it is computed
in (tests/test_dtw_gpu.py)."""
import csv

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from tests import dtw_path_references as P
from tests.test_dtw_synthesize_gpu import N_MELS, _setup

pytestmark = pytest.mark.gpu

STEP = 9
_CACHE = {}


def _symbols(model):
    from fastspeech2_lightning_amd.config import TextProcessor
    return TextProcessor(model.config.text).symbols


def _run(model, rows, corpus, out_dir, batch_size, paths=True, write=True, alignments=False):
    from fastspeech2_lightning_amd.synthesis import synthesize
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, compare_dir=corpus)
    writer = D.PackedSpecWriter(out_dir, model.output_key, STEP, n_mels=N_MELS) if write else None
    dtw = D.DtwWriter(out_dir, STEP)
    pw = D.DtwPathWriter(out_dir, STEP, _symbols(model)) if paths else None
    aw = D.AlignmentWriter(out_dir, STEP, _symbols(model)) if alignments else None
    res = synthesize(model, ds, batch_size, None, writer, compare=dtw, paths=pw, alignments=aw)
    return res, dtw, pw


def _runs(tmp_path_factory):
    """{batch size: (result, DtwWriter, DtwPathWriter, the closed dtw file)} with spectrograms, at batch sizes 2 and 3."""
    if "runs" not in _CACHE:
        model, _, _, corpus, entries, rows, _ = _setup(tmp_path_factory)
        root = tmp_path_factory.mktemp("path_runs")
        runs = {}
        for batch_size in (2, 3):
            res, dtw, pw = _run(model, rows, corpus, root / f"b{batch_size}", batch_size)
            assert len(res["files"]) == len(res["path_files"]) == len(entries)
            runs[batch_size] = (res, dtw, pw, dtw.close())
        _CACHE["runs"] = runs
    return _CACHE["runs"]


def _restated(hip, spec, recorded):
    """The path file's contents from the written spectrogram [n_mels, n] and the recording [n_mels, r]."""
    y, ref = spec.T.contiguous(), recorded.T.contiguous()
    lens = lambda n: torch.tensor([n], dtype=torch.int32, device="cuda")  # noqa: E731
    cost = hip.frame_dist(y[None].cuda(), lens(len(y)), ref[None].cuda(), lens(len(ref)))[0].cpu().numpy()
    total, steps, dirs = P.dtw_dirs(cost, np.float32)
    return (total, steps) + P.walk(cost, dirs)


@pytest.mark.parametrize("batch_size", [2, 3])
def test_every_path_file_is_the_restatement_on_the_written_spectrogram(tmp_path_factory, batch_size):
    from fastspeech2_lightning_amd import hip
    model, _, _, _, entries, _, recorded = _setup(tmp_path_factory)
    res, dtw, _, _ = _runs(tmp_path_factory)[batch_size]
    symbols = _symbols(model)
    kinds = [0, 0, 0]
    for pos, e in enumerate(entries):
        path = res["path_files"][pos]
        assert path.name == f"{e['basename']}--spk0--l0--ckpt={STEP}--dtw-path.pt" and path.parent.name == "dtw_path"
        rec = torch.load(path, weights_only=True)
        spec = torch.load(res["files"][pos], weights_only=True)
        n, r = spec.shape[1], recorded[pos].shape[1]
        total, steps, first, last, fcost = _restated(hip, spec, recorded[pos])
        assert (rec["frames"], rec["ref_frames"]) == (n, r)
        assert rec["ref_first"].tolist() == first.tolist() and rec["ref_last"].tolist() == last.tolist(), e["basename"]
        assert rec["frame_cost"].numpy().tobytes() == fcost.tobytes(), e["basename"]
        assert np.float32(rec["total"]).tobytes() == np.float32(total).tobytes() and rec["steps"] == steps
        # ... which are the psv's
        assert (dtw.records[pos]["total"], dtw.records[pos]["steps"]) == (rec["total"], rec["steps"])
        assert int(rec["duration"].sum()) == n and rec["symbols"] == [symbols[t] for t in rec["text"].tolist()]
        assert rec["raw_text"] == e["characters"] and rec["basename"] == e["basename"]
        cells, cost, start, end = P.token_values(rec["duration"].tolist(), first, last, fcost, r)
        assert rec["token_cells"].tolist() == cells and int(rec["token_cells"].sum()) == steps
        assert rec["token_cost"].tolist() == cost
        assert rec["token_ref_start"].tolist() == start and rec["token_ref_end"].tolist() == end
        assert start[0] == 0 and max(end) == r
        step = first[1:] - last[:-1]
        kinds = [kinds[0] + int((step == 1).sum()), kinds[1] + int((step == 0).sum()), kinds[2] + int((last - first).sum())]
    print(f"batch size {batch_size}: the paths advance {kinds[0]} times with a new frame, stay {kinds[1]} times, "
          f"take {kinds[2]} left moves")


def test_the_other_files_are_those_of_a_run_without_paths(tmp_path, tmp_path_factory):
    model, _, _, corpus, entries, rows, _ = _setup(tmp_path_factory)
    res, dtw, _, dtw_file = _runs(tmp_path_factory)[3]
    plain, plain_dtw, none = _run(model, rows, corpus, tmp_path / "plain", 3, paths=False)
    assert none is None and "path_files" not in plain and not (tmp_path / "plain" / "dtw_path").exists()
    assert plain_dtw.close().read_bytes() == dtw_file.read_bytes()
    assert [p.name for p in plain["files"]] == [p.name for p in res["files"]]
    for a, b in zip(plain["files"], res["files"]):
        assert a.read_bytes() == b.read_bytes(), a.name
    # the two batch sizes agree on the lengths (the values follow the forward's summation order)
    other = _runs(tmp_path_factory)[2][1]
    assert {p: (r["frames"], r["ref_frames"]) for p, r in dtw.records.items()} == \
        {p: (r["frames"], r["ref_frames"]) for p, r in other.records.items()}


def test_with_alignments_and_without_spectrograms(tmp_path, tmp_path_factory):
    model, _, _, corpus, entries, rows, _ = _setup(tmp_path_factory)
    res, dtw, _, dtw_file = _runs(tmp_path_factory)[3]
    both, both_dtw, _ = _run(model, rows, corpus, tmp_path / "both", 3, alignments=True)
    assert both_dtw.close().read_bytes() == dtw_file.read_bytes()
    assert len(both["alignment_files"]) == len(both["path_files"]) == len(entries)
    for pos in range(len(entries)):
        a, b = torch.load(both["path_files"][pos], weights_only=True), torch.load(res["path_files"][pos], weights_only=True)
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], (pos, k)
        al = torch.load(both["alignment_files"][pos], weights_only=True)
        assert torch.equal(al["duration"], a["duration"]) and torch.equal(al["text"], a["text"]) and al["frames"] == a["frames"]
        assert both["files"][pos].read_bytes() == res["files"][pos].read_bytes()
    # comparison and paths only: no spectrogram travels, the same path files
    only, only_dtw, _ = _run(model, rows, corpus, tmp_path / "only", 3, write=False)
    assert only["files"] == [] and not (tmp_path / "only" / "synthesized_spec").exists()
    assert only_dtw.close().read_bytes() == dtw_file.read_bytes()
    for pos in range(len(entries)):
        a, b = torch.load(only["path_files"][pos], weights_only=True), torch.load(res["path_files"][pos], weights_only=True)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], (pos, k)


def test_mel_dtw_with_paths_is_the_kernels_on_the_forward_s_output(tmp_path_factory):
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.synthesis import collate_items
    model, _, _, corpus, _, rows, _ = _setup(tmp_path_factory)
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, compare_dir=corpus)
    batch = collate_items([ds[i] for i in range(3)], learn_alignment=False)
    ref, ref_lens = batch.pop("compare_mel"), batch.pop("compare_lens")
    out = model(batch, inference=True, exact_lengths=True)
    plain = model.mel_dtw(out, ref, ref_lens)
    got = model.mel_dtw_paths(out, ref, ref_lens)
    assert len(plain) == 2 and len(got) == 5
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    Tm = out[model.output_key].shape[1]
    assert [t.dtype for t in got[2:]] == [torch.int32, torch.int32, torch.float32] and all(t.shape == (3, Tm) for t in got[2:])
    cost = hip.frame_dist(out[model.output_key], out["tgt_lens"], ref.cuda(), ref_lens.cuda())
    dirs = torch.zeros(cost.shape, dtype=torch.uint8, device="cuda")
    hip.dtw_dirs(cost, out["tgt_lens"], ref_lens.cuda(), dirs)
    want = hip.dtw_path(cost, dirs, out["tgt_lens"], ref_lens.cuda())
    for u, n in enumerate(out["tgt_lens"].tolist()):
        for a, b in zip(got[2:], want):
            assert torch.equal(a[u, :n], b[u, :n])
    assert any(name == "mel_dtw_dirs" for name, _, _ in hip.persistent_buffers())


def test_the_command_writes_the_path_files_and_the_token_table(tmp_path, tmp_path_factory):
    _, ckpt, fl, corpus, entries, _, _ = _setup(tmp_path_factory)
    res, _, pw, dtw_file = _runs(tmp_path_factory)[2]
    out = tmp_path / "out"
    assert cli.main(["synthesize", str(ckpt), "-f", str(fl), "--compare-to", str(corpus), "--write-paths", "--write-alignments",
                     "-o", str(out), "-b", "2"]) == 0
    assert (out / "dtw-9.psv").read_bytes() == dtw_file.read_bytes()
    assert sorted(p.name for p in (out / "dtw_path").iterdir()) == sorted(p.name for p in res["path_files"])
    for p in res["path_files"]:                                                                 # the same batches: the same files
        a, b = torch.load(out / "dtw_path" / p.name, weights_only=True), torch.load(p, weights_only=True)
        for k in a:
            assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], (p.name, k)
    assert len(list((out / "synthesized_alignment").iterdir())) == len(entries)
    table = out / "dtw-tokens-9.psv"
    assert table.read_text(encoding="utf8") == pw.close().read_text(encoding="utf8")
    with open(table, encoding="utf8", newline="") as f:
        got = list(csv.DictReader(f, delimiter="|"))
    assert list(got[0]) == list(D.DtwPathWriter.FIELDS) and len(got) == len(entries)
    ratios = [float(r["ratio"]) for r in got]
    assert ratios == sorted(ratios, reverse=True)                                               # worst first
    by_name = {p.name.split("--")[0]: torch.load(p, weights_only=True) for p in res["path_files"]}
    for r in got:
        rec = by_name[r["basename"]]
        means = [c / n if n else -1.0 for c, n in zip(rec["token_cost"].tolist(), rec["token_cells"].tolist())]
        k = int(r["token_index"])
        assert means[k] == max(means) == float(r["token_mel_dtw"]) and means.index(max(means)) == k
        assert r["symbol"] == rec["symbols"][k] and int(r["token_frames"]) == int(rec["duration"][k])
        assert (int(r["ref_start"]), int(r["ref_end"])) == (int(rec["token_ref_start"][k]), int(rec["token_ref_end"][k]))
        assert float(r["mel_dtw"]) == rec["total"] / rec["steps"] and float(r["ratio"]) == means[k] / float(r["mel_dtw"])
        assert r["raw_text"] == rec["raw_text"]
