"""CPU: the command-line side of ``fs2l train --style-lengths`` (``--dry-run``, the note on a model without the style
encoder), the binding and plan-thunk entries of the new entry points, and the yardstick itself: the restatement of
``tests/style_train_references.py`` against the oracle where the two must agree (no padding at all)."""
import json
import re
from pathlib import Path

import pytest
import torch
import yaml

from fastspeech2_lightning_amd import cli
from oracle import fs2_oracle as O
from tests.style_train_references import conv_lens, style_lens_ref
from tests.test_cli_cpu import make_project

REPO = Path(__file__).resolve().parent.parent
NEW = ("fs2hip_gru_fwd_states", "fs2hip_gru_bwd_states", "fs2hip_bn_stats_lens", "fs2hip_bn_act_bwd_lens")


def _gst_project(tmp_path):
    cfg = make_project(tmp_path, n_mels=80)
    conf = yaml.safe_load(cfg.read_text())
    wide = dict(layers=1, heads=2, input_dim=256, feedforward_dim=64, conv_kernel_size=9, dropout=0.1)
    vp = dict(n_layers=1, kernel_size=3, dropout=0.1, input_dim=256, n_bins=16)
    conf["model"].update(encoder=wide, decoder=wide, use_global_style_token_module=True,
                         variance_predictors=dict(energy=vp, pitch=vp, duration=vp))
    cfg.write_text(yaml.safe_dump(conf))
    return cfg


def _dry(capsys, *argv):
    assert cli.main(["train", *map(str, argv), "--dry-run"]) == 0
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_dry_run_reports_the_flag(tmp_path, capsys):
    cfg = _gst_project(tmp_path)
    off = _dry(capsys, cfg)
    assert off["style_lengths"] is False and "style_lengths_note" not in off
    on = _dry(capsys, cfg, "--style-lengths")
    assert on["style_lengths"] is True and "style_lengths_note" not in on


def test_the_flag_is_ignored_with_a_note_on_a_model_without_the_style_encoder(tmp_path, capsys):
    cfg = make_project(tmp_path)
    rep = _dry(capsys, cfg, "--style-lengths")
    assert rep["style_lengths"] is False
    assert "ignored" in rep["style_lengths_note"] and "use_global_style_token_module" in rep["style_lengths_note"]
    assert "style_lengths_note" not in _dry(capsys, cfg)


def test_parser_takes_the_flag_for_train_and_benchmark():
    p = cli.build_parser()
    assert p.parse_args(["train", "c.yaml", "--style-lengths"]).style_lengths is True
    assert p.parse_args(["train", "c.yaml"]).style_lengths is False
    assert p.parse_args(["benchmark", "c.yaml", "--style-lengths"]).style_lengths is True


def test_bindings_and_plan_thunks_list_the_new_entry_points():
    from fastspeech2_lightning_amd import hip
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fs2hip.h").read_text(), flags=re.S)
    inc = (REPO / "fastspeech2_lightning_amd" / "csrc" / "plan_thunks.inc").read_text()
    for name in NEW:
        assert name in hip.EXPORTS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name + "(" in inc, name
    assert "fs2hip_bn_lens_parts" in hip.EXPORTS and "fs2hip_bn_lens_parts(" not in inc     # (a size query: no stream)
    for fn in ("gru_fwd_states", "gru_bwd_states", "bn_stats_lens", "bn_act_bwd_lens"):
        assert callable(getattr(hip, fn)), fn
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.gru_fwd_states(torch.zeros(1, 1, 384), torch.zeros(384, 128), torch.zeros(384), torch.ones(1, dtype=torch.int32))


def test_module_and_model_expose_the_training_path():
    from fastspeech2_lightning_amd.model import FastSpeech2
    from fastspeech2_lightning_amd.modules import StyleEncoder
    assert callable(StyleEncoder.fwd_train)
    assert isinstance(FastSpeech2.style_lengths, property) and FastSpeech2.style_lengths.fset is not None


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def _encoder(dtype, train):
    torch.manual_seed(5)
    enc = O.StyleEncoder(idim=80).to(dtype)
    with torch.no_grad():   # running statistics away from their initial 0 / 1, so that eval mode means something
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return enc.train(train)


def test_conv_lens_is_the_integer_recurrence():
    assert conv_lens([1, 2, 3, 64, 65, 257, 1291, 0])[6] == [1, 1, 1, 1, 2, 5, 21, 0]


def test_restatement_with_full_lengths_is_the_oracle_in_train_mode():
    g = torch.Generator().manual_seed(2)
    mel = torch.randn(3, 70, 80, generator=g, dtype=torch.float64)
    d = torch.randn(3, 256, generator=g, dtype=torch.float64)
    a, b = _encoder(torch.float64, True), _encoder(torch.float64, True)
    sa, sb = a(mel), style_lens_ref(b, mel, [70, 70, 70])
    assert float((sa - sb).detach().abs().max()) < 1e-12 * max(1.0, float(sa.detach().abs().max()))
    (sa * d).sum().backward(); (sb * d).sum().backward()
    top = max(float(p.grad.abs().max()) for p in a.parameters())   # (the key bias's gradient is zero but for rounding)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 1e-9 * max(float(p.grad.abs().max()), 1e-6 * top), k
    for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
        if k.endswith(("running_mean", "running_var")):
            assert float((u - v).abs().max()) < 1e-12, k


def test_restatement_in_eval_mode_gives_every_row_its_alone_run_and_train_mode_ignores_the_padded_length():
    g = torch.Generator().manual_seed(3)
    frames = [20, 64, 65, 130, 1]
    refs = [torch.randn(n, 80, generator=g, dtype=torch.float64) for n in frames]

    def padded(T, fill=0.0):
        mel = torch.full((len(refs), T, 80), fill, dtype=torch.float64)
        for b, r in enumerate(refs):
            mel[b, :len(r)] = r
        return mel

    enc = _encoder(torch.float64, False)
    with torch.no_grad():
        got = style_lens_ref(enc, padded(130), frames)
        for b, r in enumerate(refs):
            assert float((got[b] - enc(r[None])[0]).abs().max()) < 1e-12, b
    runs = []
    for T, fill in ((130, 0.0), (171, 7.0)):     # another padded length, and anything at all in the padding
        enc = _encoder(torch.float64, True)
        style = style_lens_ref(enc, padded(T, fill), frames)
        style.square().sum().backward()
        runs.append((style.detach(), [p.grad for p in enc.parameters()], [v.clone() for v in enc.state_dict().values()]))
    assert float((runs[0][0] - runs[1][0]).abs().max()) < 1e-12
    top = max(float(p.abs().max()) for p in runs[0][1])
    for p, q in zip(runs[0][1], runs[1][1]):
        assert float((p - q).abs().max()) <= 1e-9 * max(float(p.abs().max()), 1e-6 * top)
    for u, v in zip(runs[0][2], runs[1][2]):
        assert float((u.double() - v.double()).abs().max()) < 1e-12
