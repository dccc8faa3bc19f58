"""CPU: the host side of per-utterance style references -- the filelist's ``style_reference`` column
(``cli.style_references``, ``--dry-run``), per-entry references in ``SynthesisDataset``, and the ``style_reference_lens`` a
batch of ragged references carries (``synthesis.collate_items``)."""
import json
from types import SimpleNamespace

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from oracle import cases as C

N_MELS = 80


def _tables(gst=True):
    cfg = C.small_config(learn_alignment=False, gst=gst, n_mels=N_MELS if gst else 16)
    return SimpleNamespace(config=cfg, lang2id=dict(C.LANG2ID), speaker2id=dict(C.SPEAKER2ID))


def _stub_checkpoint(path, gst=True):
    m = _tables(gst)
    torch.save({"global_step": 7, "hyper_parameters": {"config": m.config.model_checkpoint_dump(), "stats": C.STATS,
                                                       "lang2id": m.lang2id, "speaker2id": m.speaker2id}}, path)
    return path


def _mel(frames, fill=0.0):
    return torch.full((N_MELS, frames), float(fill))


def _project(tmp_path, rows, frames=(31, 9)):
    """Reference files ``refs/r<i>.pt`` and a filelist whose ``style_reference`` column holds ``rows``."""
    (tmp_path / "refs").mkdir(exist_ok=True)
    for i, n in enumerate(frames):
        torch.save(_mel(n, i + 1), tmp_path / "refs" / f"r{i}.pt")
    fl = tmp_path / "texts.psv"
    texts = ["abc", "fed cba", "cab", "abcdef"]
    fl.write_text("characters|style_reference\n" + "".join(f"{t}|{r}\n" for t, r in zip(texts, rows)), encoding="utf8")
    return fl


def _entries(fl):
    return D.synthesis_entries(None, fl, None, None, 1.0, _tables())


# ---- the column ------------------------------------------------------------------------------------------------------
def test_the_column_reaches_the_entries_and_only_where_it_is_filled(tmp_path):
    fl = _project(tmp_path, ["refs/r0.pt", "", "refs/r1.pt"])
    es = _entries(fl)
    assert [e.get("style_reference") for e in es] == ["refs/r0.pt", None, "refs/r1.pt"]
    plain = tmp_path / "plain.psv"
    plain.write_text("characters\nabc\n", encoding="utf8")
    assert "style_reference" not in _entries(plain)[0]


def test_override_and_fall_back(tmp_path):
    fl = _project(tmp_path, ["refs/r0.pt", "", str(tmp_path / "refs" / "r1.pt"), "refs/r0.pt"])
    shared = tmp_path / "shared.pt"
    torch.save(_mel(5, 9), shared)
    refs, sources = cli.style_references(_entries(fl), shared, fl, N_MELS)
    assert sources == ["own file", "shared file", "own file", "own file"]
    assert [tuple(r.shape) for r in refs] == [(N_MELS, 31), (N_MELS, 5), (N_MELS, 9), (N_MELS, 31)]
    assert [float(r[0, 0]) for r in refs] == [1.0, 9.0, 2.0, 1.0]   # a row's entry wins over -S; relative and absolute paths
    assert refs[0] is refs[3]                                       # loaded once per path
    # no row names one: -S alone, as before; neither: nothing
    bare = tmp_path / "bare.psv"
    bare.write_text("characters\nabc\nfed\n", encoding="utf8")
    ref, sources = cli.style_references(_entries(bare), shared, bare, N_MELS)
    assert torch.is_tensor(ref) and tuple(ref.shape) == (N_MELS, 5) and sources == ["shared file"] * 2
    assert cli.style_references(_entries(bare), None, bare, N_MELS) == (None, [None, None])


def test_errors_name_the_row_or_the_file(tmp_path):
    fl = _project(tmp_path, ["refs/r0.pt", "", "refs/r1.pt"])
    with pytest.raises(SystemExit, match=r"row 2 \('fed-cba'\).*no style_reference"):
        cli.style_references(_entries(fl), None, fl, N_MELS)
    fl = _project(tmp_path, ["refs/r0.pt", "refs/missing.pt"])
    with pytest.raises(SystemExit, match=r"row 2 .*missing\.pt: no such file"):
        cli.style_references(_entries(fl), None, fl, N_MELS)
    fl = _project(tmp_path, ["refs/r0.pt", "refs/r1.wav"])
    with pytest.raises(SystemExit, match=r"r1\.wav: expected a \.pt file"):
        cli.style_references(_entries(fl), None, fl, N_MELS)
    torch.save(torch.zeros(16, 9), tmp_path / "refs" / "narrow.pt")
    torch.save({"mel": 1}, tmp_path / "refs" / "dict.pt")
    for name, got in (("narrow.pt", r"\[16, 9\]"), ("dict.pt", "dict")):
        fl = _project(tmp_path, ["refs/r0.pt", f"refs/{name}"])
        with pytest.raises(SystemExit, match=rf"{name}: expected a \[n_mels = 80, frames\] mel, got {got}"):
            cli.style_references(_entries(fl), None, fl, N_MELS)


def test_dry_run_reports_every_rows_style_source(tmp_path, capsys):
    ckpt = _stub_checkpoint(tmp_path / "gst.ckpt")
    fl = _project(tmp_path, ["refs/r0.pt", "", "refs/r1.pt"])
    shared = tmp_path / "shared.pt"
    torch.save(_mel(5), shared)

    def dry(*argv):
        capsys.readouterr()
        assert cli.main(["synthesize", *map(str, argv), "-o", str(tmp_path / "out"), "--dry-run"]) == 0
        return json.loads(capsys.readouterr().out)

    assert dry(ckpt, "-f", fl, "-S", shared)["style_sources"] == ["own file", "shared file", "own file"]
    assert dry(ckpt, "-t", "abc", "-t", "fed", "-S", shared)["style_sources"] == ["shared file"] * 2
    assert dry(ckpt, "-t", "abc", "-t", "fed")["style_sources"] == ["token"] * 2
    assert dry(ckpt, "-t", "abc", "-T", tmp_path / "tf", "--exact-lengths")["style_sources"] == ["target"]
    with pytest.raises(SystemExit, match="row 2"):
        dry(ckpt, "-f", fl)
    # a model without the module: no such key, and the column is refused as -S is
    plain = _stub_checkpoint(tmp_path / "plain.ckpt", gst=False)
    assert "style_sources" not in dry(plain, "-t", "abc")


# ---- SynthesisDataset ------------------------------------------------------------------------------------------------
ENTRIES = [{"basename": "u0", "characters": "abc"}, {"basename": "u1", "characters": "fed cba"},
           {"basename": "u2", "characters": "cab"}]


def _dataset(style_reference, gst=True, entries=ENTRIES):
    m = _tables(gst)
    return D.SynthesisDataset(entries, m.config, m.lang2id, m.speaker2id, style_reference=style_reference)


def test_every_item_carries_its_own_reference():
    a, b = _mel(31, 1), _mel(9, 2)
    a[5, 2] = 7.0
    ds = _dataset([a, b, a])
    refs = [ds[i]["mel_style_reference"] for i in range(3)]
    assert [tuple(r.shape) for r in refs] == [(31, N_MELS), (9, N_MELS), (31, N_MELS)]
    assert float(refs[0][2, 5]) == 7.0 and refs[0] is refs[2] and ds.style is None
    by_name = _dataset({"u2": a, "u0": b, "u1": b, "unused": a})
    assert [len(by_name[i]["mel_style_reference"]) for i in range(3)] == [9, 9, 31]
    assert [len(_dataset((a.numpy(), b.numpy(), b.numpy()))[i]["mel_style_reference"]) for i in range(3)] == [31, 9, 9]


def test_one_object_for_all_is_the_shared_reference():
    a = _mel(31, 1)
    ds, shared = _dataset([a, a, a]), _dataset(a)
    assert ds.styles is None and torch.equal(ds.style, shared.style)
    assert all(ds[i]["mel_style_reference"] is ds.style for i in range(3))


def test_per_entry_errors():
    a = _mel(31)
    with pytest.raises(ValueError, match="2 given for 3"):
        _dataset([a, a])
    with pytest.raises(ValueError, match="'u1' has none"):
        _dataset([a, None, a])
    with pytest.raises(ValueError, match=r"utterance 'u2' must be a \[n_mels = 80, frames\] mel, got \[16, 9\]"):
        _dataset([a, a, torch.zeros(16, 9)])
    with pytest.raises(ValueError, match="no entry for utterance 'u1'"):
        _dataset({"u0": a, "u2": a})
    with pytest.raises(ValueError, match="global style token"):
        _dataset([torch.zeros(16, 9)] * 3, gst=False)


# ---- the batch -------------------------------------------------------------------------------------------------------
def test_a_batch_of_ragged_references_carries_their_lengths():
    from fastspeech2_lightning_amd.synthesis import collate_items
    a, b = _mel(31, 1), _mel(9, 2)
    ds = _dataset([a, b, a])
    batch = collate_items([ds[i] for i in range(3)], learn_alignment=False)
    assert batch["style_reference_lens"].dtype == torch.int32 and batch["style_reference_lens"].tolist() == [31, 9, 31]
    ref = batch["mel_style_reference"]
    assert tuple(ref.shape) == (3, 31, N_MELS) and float(ref[1, :9].min()) == 2.0 and float(ref[1, 9:].abs().max()) == 0.0
    assert D.style_reference_lens([ds[0], ds[2]]) is None            # one object in this batch: nothing to tell apart
    # one shared reference, or none: collate's batch, key for key
    for style in (a, None):
        shared = _dataset(style)
        items = [shared[i] for i in range(3)]
        got, want = collate_items(items, learn_alignment=False), D.collate(items, learn_alignment=False)
        assert list(got) == list(want) and "style_reference_lens" not in got
