"""CPU: the host side of the computed attention prior -- ``--compute-attn-prior`` on the three commands, datasets that open
no prior file (``attn_prior="computed"``), ``collate`` and ``pad_axes`` on a batch without a prior, and what the dry runs
report.  The project directories here have no ``attn/`` folder: only the parent toolkit's preprocessor writes one."""
import json
from types import SimpleNamespace

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd import hip as H
from oracle import cases as C
from tests.test_cli_cpu import make_project


def test_the_three_commands_take_the_flag():
    ap = cli.build_parser()
    for argv in (["train", "c.yaml"], ["benchmark", "c.yaml"], ["synthesize", "m.ckpt", "-t", "abc", "-T", "tf"]):
        assert ap.parse_args(argv).compute_attn_prior is False
        assert ap.parse_args(argv + ["--compute-attn-prior"]).compute_attn_prior is True


def _dataset(tmp_path, **kw):
    cfg = make_project(tmp_path, n_train=4, n_val=1, write_features=True, learn_alignment=True)
    p = cli.plan(cli.build_parser().parse_args(["train", str(cfg)]))
    assert p["config"].model.learn_alignment and not (tmp_path / "preprocessed" / "attn").exists()
    return D.FeatureDataset(p["train_rows"], p["config"], p["lang2id"], p["speaker2id"], **kw)


def test_a_computed_prior_dataset_opens_no_prior_file_and_the_batch_carries_none(tmp_path):
    ds = _dataset(tmp_path, attn_prior="computed")
    items = [ds[i] for i in range(len(ds))]
    assert all(it["duration"] is None for it in items)
    assert all(torch.is_tensor(it[k]) for it in items for k in ("mel", "text", "pitch", "energy"))
    batch = D.collate(items, learn_alignment=True)
    assert batch["duration"] == [None] * len(items)
    assert not any(torch.is_tensor(v) and v.dim() == 3 and k != "mel" for k, v in batch.items())
    assert batch["mel"].shape[:2] == (len(items), int(batch["max_mel_len"])) and batch["mel_lens"].dtype == torch.int32
    # the padding launch of a bucketed step has no prior to pad either
    assert "duration" not in H.pad_axes(batch, frame_level=False)
    assert "duration" not in H.pad_axes(dict(batch, duration=None), frame_level=False)


def test_the_default_still_loads_the_files_and_fails_without_them(tmp_path):
    ds = _dataset(tmp_path)
    assert ds.attn_prior == "files"
    with pytest.raises(FileNotFoundError, match="attn-prior"):
        ds[0]
    with pytest.raises(ValueError, match="attn_prior"):
        D.FeatureDataset(ds.entries, ds.config, ds.lang2id, ds.speaker2id, attn_prior="table")


def _dry_run(capsys, argv):
    assert cli.main(argv + ["--dry-run"]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_train_dry_run_reports_the_prior_mode(tmp_path, capsys):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    learned = make_project(tmp_path / "a", learn_alignment=True)
    assert _dry_run(capsys, ["train", str(learned)])["attn_prior"] == "files"
    plan = _dry_run(capsys, ["train", str(learned), "--compute-attn-prior"])
    assert plan["attn_prior"] == "computed" and plan["learn_alignment"] is True and "attn_prior_note" not in plan
    given = make_project(tmp_path / "b", learn_alignment=False)
    plan = _dry_run(capsys, ["train", str(given), "--compute-attn-prior"])
    assert plan["attn_prior"] == "files" and "ignored" in plan["attn_prior_note"] and plan["learn_alignment"] is False


def _stub_checkpoint(path, learn_alignment):
    """A checkpoint with everything but weights: what ``synthesize --dry-run`` reads."""
    cfg = C.small_config(learn_alignment=learn_alignment)
    torch.save({"global_step": 7, "hyper_parameters": {"config": cfg.model_checkpoint_dump(), "stats": C.STATS,
                                                       "lang2id": dict(C.LANG2ID), "speaker2id": dict(C.SPEAKER2ID)}}, path)
    return path


def test_synthesize_dry_run_reports_the_prior_mode(tmp_path, capsys):
    learned = _stub_checkpoint(tmp_path / "la.ckpt", True)
    base = ["synthesize", str(learned), "-t", "abc def", "-T", str(tmp_path), "-o", str(tmp_path / "out")]
    assert _dry_run(capsys, base)["attn_prior"] == "files"
    plan = _dry_run(capsys, base + ["--return-scores", "--scores-only", "--compute-attn-prior"])
    assert plan["attn_prior"] == "computed" and plan["return_scores"] is True and "attn_prior_note" not in plan
    given = _stub_checkpoint(tmp_path / "dur.ckpt", False)
    plan = _dry_run(capsys, ["synthesize", str(given), "-t", "abc def", "-T", str(tmp_path), "--compute-attn-prior"])
    assert plan["attn_prior"] == "files" and "ignored" in plan["attn_prior_note"]


def test_a_teacher_forced_synthesis_item_without_a_prior(tmp_path):
    """``SynthesisDataset(attn_prior="computed")`` loads the mel from the teacher-forcing directory and nothing else."""
    cfg = make_project(tmp_path, n_train=3, n_val=1, write_features=True, learn_alignment=True)
    p = cli.plan(cli.build_parser().parse_args(["train", str(cfg)]))
    model = SimpleNamespace(config=p["config"], lang2id=p["lang2id"], speaker2id=p["speaker2id"])
    rows = D.synthesis_entries(None, tmp_path / "preprocessed" / "training_filelist.psv", None, None, 1.0, model)
    pre = tmp_path / "preprocessed"
    item = D.SynthesisDataset(rows, p["config"], p["lang2id"], p["speaker2id"], teacher_forcing_dir=pre,
                              attn_prior="computed")[0]
    assert item["duration"] is None and item["mel"].shape[1] == 16
    with pytest.raises(FileNotFoundError, match="attn-prior"):
        D.SynthesisDataset(rows, p["config"], p["lang2id"], p["speaker2id"], teacher_forcing_dir=pre)[0]
