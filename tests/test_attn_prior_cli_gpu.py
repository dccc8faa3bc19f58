"""GPU: ``--compute-attn-prior`` end to end.  A learned-alignment project directory with mels and frame-level pitch /
energy files and NO ``attn/`` folder (only the parent toolkit's preprocessor writes one) trains, benchmarks and scores;
the same commands without the flag stop at the missing prior file, as they always did.  The scores of the computed run
equal, value for value, those of a run that loads prior files holding ``hip.attn_prior``'s own per-utterance output."""
import contextlib
import csv
import json
import math

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import hip as H
from tests.test_cli_cpu import make_project

pytestmark = pytest.mark.gpu

N_TRAIN, N_VAL = 6, 2


@contextlib.contextmanager
def host_threads_kept():
    """``fs2l train`` sizes torch's intra-op pool for a training process (``parallel.apply_host_budget``: every core the
    process may run on).  Run in-process here, that setting would outlive the command and every later test of the
    session -- the CPU oracle's above all -- would compute on a pool sized for the whole host: put it back."""
    n = torch.get_num_threads()
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _name(row, fn):
    return "--".join([row["basename"], row["speaker"], row["language"], fn])


def _rows(pre):
    out = []
    for fl in ("training_filelist.psv", "validation_filelist.psv"):
        with open(pre / fl, encoding="utf8", newline="") as f:
            out += list(csv.DictReader(f, delimiter="|"))
    return out


@pytest.fixture(scope="module")
def project(tmp_path_factory):
    """The project, trained for four steps with the flag: (config, preprocessed directory, run directory)."""
    tmp = tmp_path_factory.mktemp("learned")
    cfg = make_project(tmp, n_train=N_TRAIN, n_val=N_VAL, write_features=True, learn_alignment=True)
    pre = tmp / "preprocessed"
    g = torch.Generator().manual_seed(3)
    for row in _rows(pre):   # learned alignment takes frame-level targets: one value per mel frame
        frames = torch.load(pre / "spec" / _name(row, "spec-22050-mel-librosa.pt"), weights_only=True).shape[1]
        for kind in ("pitch", "energy"):
            torch.save(torch.randn(frames, generator=g), pre / kind / _name(row, f"{kind}.pt"))
    assert not (pre / "attn").exists()
    run = tmp / "run"
    with host_threads_kept():
        assert cli.main(["train", str(cfg), "--output-dir", str(run), "--devices", "1", "--log-every", "1", "--max-steps", "4",
                         "--compute-attn-prior"]) == 0
    return cfg, pre, run


def test_train_runs_without_prior_files_and_still_fails_without_the_flag(project, tmp_path):
    cfg, pre, run = project
    ck = torch.load(run / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=False)
    assert ck["global_step"] == 4 and cli.checkpoint_tables(ck).config.model.learn_alignment is True
    recs = [json.loads(l) for l in (run / "metrics.jsonl").read_text().splitlines()]
    train = [r for r in recs if "training/total_loss" in r]
    assert [r["step"] for r in train] == [1, 2, 3, 4]
    assert all(math.isfinite(r["training/total_loss"]) and r["training/attn_ctc_loss"] > 0 for r in train)
    assert any("validation/total_loss" in r and math.isfinite(r["validation/total_loss"]) for r in recs)
    assert not (pre / "attn").exists()
    with host_threads_kept(), pytest.raises(FileNotFoundError, match="attn-prior"):
        cli.main(["train", str(cfg), "--output-dir", str(tmp_path / "files"), "--devices", "1", "--max-steps", "4"])
    assert not (tmp_path / "files" / "checkpoints" / "last.ckpt").exists()


def test_benchmark_times_the_forward_pass_without_prior_files(project, capsys):
    cfg, _, _ = project
    assert cli.main(["benchmark", str(cfg), "--compute-attn-prior", "--warmup-reps", "2", "--repetitions", "5"]) == 0
    out = capsys.readouterr().out
    assert "Average forward pass for training duration after 5 repetitions:" in out and "Standard Deviation" in out
    assert 0.0 < float(out.split("repetitions:")[1].split("ms")[0]) < 1000.0
    with pytest.raises(FileNotFoundError, match="attn-prior"):
        cli.main(["benchmark", str(cfg), "--warmup-reps", "1", "--repetitions", "1"])


def _scores(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.DictReader(f, delimiter="|"))


def test_scores_of_the_computed_prior_equal_those_of_its_own_files(project, tmp_path):
    cfg, pre, run = project
    ckpt, fl = run / "checkpoints" / "last.ckpt", pre / "training_filelist.psv"
    base = ["synthesize", str(ckpt), "-f", str(fl), "-T", str(pre), "-b", "3", "--return-scores", "--scores-only"]
    assert cli.main(base + ["-o", str(tmp_path / "computed"), "--compute-attn-prior"]) == 0
    computed = _scores(tmp_path / "computed" / "scores-4.psv")
    assert len(computed) == N_TRAIN and not (tmp_path / "computed" / "synthesized_spec").exists()
    for r in computed:
        assert all(math.isfinite(float(r[k])) for k in ("total", "duration", "spec", "postnet", "attn_ctc", "attn_bin"))
        assert float(r["attn_ctc"]) > 0
    with pytest.raises(FileNotFoundError, match="attn-prior"):
        cli.main(base + ["-o", str(tmp_path / "missing")])
    # the files the parent toolkit would have written, from the kernel's own per-utterance output
    (pre / "attn").mkdir()
    try:
        for row in _rows(pre)[:N_TRAIN]:
            frames = torch.load(pre / "spec" / _name(row, "spec-22050-mel-librosa.pt"), weights_only=True).shape[1]
            tokens = len(row["character_tokens"].split("/"))
            lens = lambda n: torch.tensor([n], dtype=torch.int32, device="cuda")  # noqa: E731
            prior = H.attn_prior(lens(frames), lens(tokens), frames, tokens)[0].cpu()
            assert tuple(prior.shape) == (frames, tokens) and abs(float(prior.sum()) - frames) < 1e-3
            torch.save(prior, pre / "attn" / _name(row, "characters-attn-prior.pt"))
        assert cli.main(base + ["-o", str(tmp_path / "files")]) == 0
    finally:
        for f in (pre / "attn").iterdir():
            f.unlink()
        (pre / "attn").rmdir()
    assert _scores(tmp_path / "files" / "scores-4.psv") == computed
