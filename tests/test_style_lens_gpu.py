"""GPU: length-aware GST style encoding -- ``hip.gru_last_state`` / ``hip.conv_s2_lens``, ``StyleEncoder.fwd(mel, lens)``,
the ``style_reference_lens`` batch key of ``FastSpeech2.forward`` and the ``style_reference`` filelist column of ``fs2l
synthesize``.

The yardstick is the float64 oracle run ONE REFERENCE (one utterance) AT A TIME: alone there is no padding for the strided
convolutions to read and no padded step for the GRU to run.  Bounds are those of ``tests/test_gst_module_gpu.py``
(``max(2e-5, 4 x the fp32 oracle's own error against float64)``, relative to the largest element, measured inside the
test), ``tests/test_exact_lengths_gpu.py`` (``1e-4 * max(1, |ref|.max())``) and ``tests/test_scores_gpu.py``
(``1e-4 * max(1, |ref|)``)."""
import csv
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from fastspeech2_lightning_amd.config import InferenceControl, Stats, TextConfig
from oracle import cases as C
from oracle import fs2_oracle as O
from tests.gst_references import gru_sequence_ref

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
FLOOR, FACTOR = 2e-5, 4.0
U = 128
REF_FRAMES = [20, 64, 65, 130, 257, 1, 129]
_SHARED = {}


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# ---- kernel: gru_last_state --------------------------------------------------------------------------------------------
def _gru_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    gi = torch.randn(B, T, 3 * U, generator=g)
    w_hh = torch.randn(3 * U, U, generator=g) / U ** 0.5
    b_hh = 0.1 * torch.randn(3 * U, generator=g)
    return gi, w_hh, b_hh


def _gru_ref(gi, w_hh, b_hh, steps, dtype):
    """Row b: ``gru_sequence_ref`` over the row's first ``min(steps[b], T)`` projections (fed through an identity input
    weight, which leaves them as they are)."""
    B, T, _ = gi.shape
    eye, zero = torch.eye(3 * U, dtype=dtype), torch.zeros(3 * U, dtype=dtype)
    rows = [gru_sequence_ref(gi[b:b + 1, :min(int(n), T)].to(dtype), eye, w_hh.to(dtype), zero, b_hh.to(dtype))
            for b, n in enumerate(steps)]
    return torch.cat(rows)


def _poisoned(gi, steps):
    """``gi`` with NaN in every row at and beyond its utterance's step count."""
    gi = gi.clone()
    for b, n in enumerate(steps):
        gi[b, max(int(n), 0):] = float("nan")
    return gi


GRU_CASES = {
    "ragged": (5, 6, [6, 1, 3, 0, 5]),
    "one_step": (1, 1, [1]),
    "many_rows": (70, 3, None),          # random steps in 0..3
    "clamped": (4, 3, [7, 3, 1000, 2]),   # steps above T are clamped to T
}


@pytest.mark.parametrize("name", list(GRU_CASES))
def test_gru_last_state_matches_the_float64_recurrence(name):
    from fastspeech2_lightning_amd import hip as H
    B, T, steps = GRU_CASES[name]
    gi, w_hh, b_hh = _gru_inputs(B, T, 100 + B)
    if steps is None:
        steps = torch.randint(0, T + 1, (B,), generator=torch.Generator().manual_seed(3)).tolist()
        assert {0, T} <= set(steps)
    want = _gru_ref(gi, w_hh, b_hh, steps, torch.float64)
    e32 = _rel(_gru_ref(gi, w_hh, b_hh, steps, torch.float32), want)
    got = H.gru_last_state(_poisoned(gi, steps).cuda(), w_hh.cuda(), b_hh.cuda(),
                           torch.tensor(steps, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, U) and torch.isfinite(got).all()    # (finite: the NaN rows were not read)
    err, bound = _rel(got, want), max(FLOOR, FACTOR * e32)
    print(f"gru_last_state {name}: kernel {err:.2e}, fp32 reference {e32:.2e}, bound {bound:.2e}")
    assert err < bound
    for b, n in enumerate(steps):
        if n == 0:
            assert int((got[b] != 0).sum()) == 0, (b, "a row without steps is exactly 0")
    if name == "ragged":
        assert steps[3] == 0
        for b in range(B):   # a row's result is a function of that row alone: bit-equal as a batch of one
            one = H.gru_last_state(_poisoned(gi, steps)[b:b + 1].contiguous().cuda(), w_hh.cuda(), b_hh.cuda(),
                                   torch.tensor(steps[b:b + 1], dtype=torch.int32).cuda())
            assert torch.equal(one[0], got[b]), b


def test_gru_last_state_refusals():
    from fastspeech2_lightning_amd import hip as H
    gi, w_hh, b_hh = (t.cuda() for t in _gru_inputs(2, 3, 1))
    steps = torch.tensor([1, 2], dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="only 128"):
        H.gru_last_state(torch.zeros(2, 3, 192).cuda(), torch.zeros(192, 64).cuda(), torch.zeros(192).cuda(), steps)
    with pytest.raises(ValueError, match="do not fit"):
        H.gru_last_state(gi, w_hh, b_hh[:-1].contiguous(), steps)
    with pytest.raises(ValueError, match="do not fit"):
        H.gru_last_state(gi[:, :, :-1].contiguous(), w_hh, b_hh, steps)
    with pytest.raises(ValueError, match="entries"):
        H.gru_last_state(gi, w_hh, b_hh, steps[:1].contiguous())
    with pytest.raises(ValueError, match=r"\[B, T, 3U\]"):
        H.gru_last_state(gi.view(6, 3 * U), w_hh, b_hh, steps)
    with pytest.raises(TypeError):
        H.gru_last_state(gi, w_hh, b_hh, steps.long())
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.gru_last_state(gi.cpu(), w_hh, b_hh, steps)


# ---- kernel: conv_s2_lens ----------------------------------------------------------------------------------------------
def test_conv_s2_lens_is_the_integer_recurrence():
    from fastspeech2_lightning_amd import hip as H
    lens = [1, 2, 3, 64, 65, 257, 1291, 0]
    want = [lens]
    for _ in range(6):
        want.append([(v - 1) // 2 + 1 if v > 0 else 0 for v in want[-1]])
    got = H.conv_s2_lens(torch.tensor(lens, dtype=torch.int32).cuda(), 6)
    assert got.dtype == torch.int32 and got.cpu().tolist() == want
    assert want[6] == [1, 1, 1, 1, 2, 5, 21, 0]
    with pytest.raises(ValueError, match="0 to 8"):
        H.conv_s2_lens(torch.tensor(lens, dtype=torch.int32).cuda(), 9)
    with pytest.raises(TypeError):
        H.conv_s2_lens(torch.tensor(lens).cuda(), 6)


# ---- module ------------------------------------------------------------------------------------------------------------
def _module_reference():
    """The model, the padded batch of references and the oracle's runs (float64 and fp32, alone and on the padded batch):
    computed once and shared."""
    if "module" not in _SHARED:
        from tests.test_gst_module_gpu import build
        model, sd = build(80)
        sd_gst = {k[len("gst."):]: v for k, v in sd.items() if k.startswith("gst.")}
        g = torch.Generator().manual_seed(7)
        refs = [torch.randn(n, 80, generator=g) for n in REF_FRAMES]
        mel = torch.zeros(len(refs), max(REF_FRAMES), 80)
        for b, r in enumerate(refs):
            mel[b, :len(r)] = r
        runs = {}
        for dtype in (torch.float64, torch.float32):
            enc = O.StyleEncoder(idim=80)
            enc.load_state_dict(sd_gst)
            enc = enc.to(dtype).eval()
            with torch.no_grad():
                runs[dtype] = (torch.cat([enc(r[None].to(dtype)) for r in refs]), enc(mel.to(dtype)))
        _SHARED["module"] = model, sd, mel, runs
    return _SHARED["module"]


def _eval_model():
    model, sd, mel, runs = _module_reference()
    model.load_state_dict(sd)
    return model.eval(), mel, runs


def test_style_encoder_with_lens_gives_every_reference_its_alone_run():
    model, mel, runs = _eval_model()
    alone64, padded64 = runs[torch.float64]
    alone32, padded32 = runs[torch.float32]
    lens = torch.tensor(REF_FRAMES, dtype=torch.int32).cuda()
    longest = REF_FRAMES.index(max(REF_FRAMES))
    # the discriminating half: in the oracle itself the padding moves every row but the longest ...
    for b in range(len(REF_FRAMES)):
        dev = float((padded64[b] - alone64[b]).abs().max())
        print(f"reference {b} ({REF_FRAMES[b]} frames): oracle padded against alone {dev:.2e}, largest element "
              f"{float(alone64[b].abs().max()):.2f}")
        assert (dev > 1e-3) == (b != longest), (b, dev)
    # ... and the path without lengths reproduces that padded oracle
    plain, _ = model.gst.fwd(mel.cuda())
    e, e32 = _rel(plain, padded64), _rel(padded32, padded64)
    print(f"without lens against the padded oracle: kernel {e:.2e}, fp32 oracle {e32:.2e}")
    assert e < max(FLOOR, FACTOR * e32)
    given = mel.cuda()
    style, ctx = model.gst.fwd(given, lens)
    torch.cuda.synchronize()
    assert ctx is None and tuple(style.shape) == (len(REF_FRAMES), 256)
    for b in range(len(REF_FRAMES)):
        e, e32 = _rel(style[b], alone64[b]), _rel(alone32[b], alone64[b])
        bound = max(FLOOR, FACTOR * e32)
        print(f"reference {b} ({REF_FRAMES[b]} frames): kernel {e:.2e}, fp32 oracle {e32:.2e}, bound {bound:.2e}")
        assert e < bound, (b, e, bound)


def test_full_lengths_agree_with_the_path_without_lengths():
    model, mel, runs = _eval_model()
    e32 = _rel(runs[torch.float32][1], runs[torch.float64][1])
    plain, _ = model.gst.fwd(mel.cuda())
    full = torch.full((mel.shape[0],), mel.shape[1], dtype=torch.int32).cuda()
    style, _ = model.gst.fwd(mel.cuda(), full)
    e = _rel(style, plain)
    print(f"all lengths = T_ref: with lens against without {e:.2e}, bound {max(FLOOR, FACTOR * e32):.2e}")
    assert e < max(FLOOR, FACTOR * e32)


def test_lens_in_train_mode_is_refused():
    model, mel, _ = _eval_model()
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            model.gst.fwd(mel.cuda(), torch.tensor(REF_FRAMES, dtype=torch.int32).cuda())
    finally:
        model.eval()


# ---- model -------------------------------------------------------------------------------------------------------------
def _gst_pair():
    """The GST case's model and oracle with the same weights, its ragged batch and the oracle's teacher-forced alone-runs
    with their losses: computed once and shared."""
    if "model" not in _SHARED:
        from tests.test_exact_lengths_gpu import _pair, _row
        cfg, batch, _ = C.build("e2e_gst_multispeaker_train")
        model, oracle = _pair(cfg)
        alone, losses = {}, {}
        with torch.no_grad():
            for j in range(3):
                row = _row(batch, j, False)
                alone[j] = oracle(row, inference=True)          # no reference: the utterance's own target mel
                losses[j] = {k: float(v) for k, v in oracle.loss(alone[j], row, 0).items()}
        _SHARED["model"] = cfg, model, oracle, batch, alone, losses
    return _SHARED["model"]


def _mel_close(tag, out, alone, rows):
    lens = out["tgt_lens"].cpu().tolist()
    want = [int(alone[j]["tgt_lens"][0]) for j in rows]
    print(f"{tag}: frame counts {[lens[j] for j in rows]} against alone {want}")
    assert [lens[j] for j in rows] == want
    for key in ("output", "postnet_output"):
        for j, n in zip(rows, want):
            ref = alone[j][key][0]
            got = out[key][j, :n].cpu()
            err, tol = float((got - ref).abs().max()), 1e-4 * max(1.0, float(ref.abs().max()))
            print(f"{tag}: {key} of utterance {j}: error {err:.2e}, bound {tol:.2e}")
            assert torch.isfinite(got).all() and err < tol, (tag, key, j, err, tol)


def test_teacher_forced_batch_with_its_own_mels_as_style_equals_the_oracle_alone():
    from fastspeech2_lightning_amd.model import LOSS_KEYS
    cfg, model, oracle, batch, alone, losses = _gst_pair()
    assert len(set(batch["mel_lens"].tolist())) > 1
    styled = dict(batch, mel_style_reference=batch["mel"], style_reference_lens=batch["mel_lens"])
    kept = batch["mel"].clone()
    out = model(styled, inference=True, exact_lengths=True)
    assert torch.equal(batch["mel"], kept)
    _mel_close("teacher forcing", out, alone, range(3))
    table, keys = model.utterance_losses(out, dict(batch), current_epoch=0)
    got = table.cpu()
    for j in range(3):
        r = losses[j]
        assert set(keys) | {"total"} == set(r), (keys, list(r))
        row = {k: float(got[j, LOSS_KEYS.index(k)]) for k in keys}
        row["total"] = float(got[j, -1])
        print(f"utterance {j}: " + ", ".join(f"{k} {row[k]:.6f} ({r[k]:.6f})" for k in row))
        for k in row:
            assert abs(row[k] - r[k]) <= 1e-4 * max(1.0, abs(r[k])), (j, k, row[k], r[k])


def _free_case():
    """Texts of 12, 5 and 9 tokens and references of 23, 70 and 9 frames.  Text seed 6: the first from 3 (the recipe of
    tests/test_exact_lengths_gpu.py) whose oracle alone-runs keep every duration at least 1e-3 * (value + 1) from a rounding
    boundary (1.4e-3; seeds 3 to 5 give 2.9e-6, 1.3e-4, 6.8e-4) -- chosen on the oracle, before any GPU run."""
    from tests.test_exact_lengths_gpu import _free_batch, _texts
    texts = _texts(6, [12, 5, 9])
    g = torch.Generator().manual_seed(11)
    refs = [torch.randn(n, 80, generator=g) for n in (23, 70, 9)]
    mel = torch.zeros(3, 70, 80)
    for b, r in enumerate(refs):
        mel[b, :len(r)] = r
    return texts, refs, mel, _free_batch


def test_free_inference_with_a_reference_per_row_equals_the_oracle_alone():
    cfg, model, oracle, *_ = _gst_pair()
    texts, refs, mel, _free_batch = _free_case()
    with torch.no_grad():
        alone = {j: oracle(dict(_free_batch([texts[j]]), mel_style_reference=refs[j][None]), InferenceControl(),
                           inference=True) for j in range(3)}
    v = torch.cat([torch.exp(alone[j]["duration_prediction"][0].double()) - 1 for j in range(3)])
    v = v[v > 0]
    margin = float(((v - (torch.floor(v) + 0.5)).abs() / (v + 1)).min())
    print(f"smallest distance of a duration from a half-integer / (value + 1) = {margin:.2e}")
    assert margin >= 1e-3 and min(int(alone[j]["tgt_lens"][0]) for j in range(3)) >= 1
    batch = dict(_free_batch(texts), mel_style_reference=mel, style_reference_lens=torch.tensor([23, 70, 9], dtype=torch.int32))
    out = model(batch, InferenceControl(), inference=True, exact_lengths=True)
    _mel_close("free inference", out, alone, range(3))
    # the lengths on the device, a reference on the device: the same result, and the caller's tensor is not written to
    on_dev = mel.cuda()
    on_dev[0, 23:] = 5.0
    kept = on_dev.clone()
    again = model(dict(batch, mel_style_reference=on_dev, style_reference_lens=batch["style_reference_lens"].cuda()),
                  InferenceControl(), inference=True, exact_lengths=True)
    assert torch.equal(on_dev, kept)
    _mel_close("free inference, device inputs", again, alone, range(3))


def test_model_refusals():
    cfg, model, oracle, tf_batch, *_ = _gst_pair()
    texts, refs, mel, _free_batch = _free_case()
    batch = dict(_free_batch(texts), mel_style_reference=mel)
    for bad in ([23, 71, 9], [0, 70, 9]):
        with pytest.raises(ValueError, match="1 .. T_ref"):
            model(dict(batch, style_reference_lens=torch.tensor(bad, dtype=torch.int32)), InferenceControl(), inference=True)
    with pytest.raises(ValueError, match="entries"):
        model(dict(batch, style_reference_lens=torch.tensor([23, 70], dtype=torch.int32)), InferenceControl(), inference=True)
    lens = torch.tensor([23, 70, 9], dtype=torch.int32)
    with pytest.raises(ValueError, match="mel_style_reference tensor"):
        model(dict(batch, mel_style_reference=None, style_reference_lens=lens), InferenceControl(), inference=True)
    with pytest.raises(ValueError, match="inference=True"):
        model(dict(tf_batch, mel_style_reference=tf_batch["mel"], style_reference_lens=tf_batch["mel_lens"]))
    from tests.test_exact_lengths_gpu import _pair
    plain, _ = _pair(C.small_config(learn_alignment=False))
    small = dict(_free_batch(texts), mel_style_reference=torch.zeros(3, 70, 16), style_reference_lens=lens)
    with pytest.raises(ValueError, match="global style token"):
        plain(small, InferenceControl(), inference=True)


def test_bf16_mixed_forward_with_lengths_is_finite():
    """A smoke test only: the project holds no bf16 bound for this path."""
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.model import FastSpeech2
    cfg, _, _, batch, *_ = _gst_pair()
    try:
        model = FastSpeech2(cfg, Stats(**C.STATS), lang2id=C.LANG2ID, speaker2id=C.SPEAKER2ID, precision="bf16-mixed").eval()
        out = model(dict(batch, mel_style_reference=batch["mel"], style_reference_lens=batch["mel_lens"]), inference=True,
                    exact_lengths=True)
        for j, n in enumerate(batch["mel_lens"].tolist()):
            assert torch.isfinite(out["postnet_output"][j, :n]).all() and torch.isfinite(out["output"][j, :n]).all()
    finally:
        hip.set_precision("32-true")


# ---- command line ------------------------------------------------------------------------------------------------------
def _commands(argvs):
    """``cli.main`` on every argument list, one after another, in ONE fresh child process."""
    code = ("import json, sys\nfrom fastspeech2_lightning_amd import cli\n"
            "for argv in json.loads(sys.argv[1]):\n    assert cli.main(argv) == 0, argv\n")
    r = subprocess.run([sys.executable, "-c", code, json.dumps([[str(a) for a in argv] for argv in argvs])], cwd=REPO,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _gst_checkpoint(path, symbols=None):
    """A checkpoint of the GST case's model with the oracle's seeded weights (style vectors of about 0.6, which padding
    moves by 1e-2: the module test above)."""
    from tests.test_exact_lengths_gpu import _pair
    cfg, _, _ = C.build("e2e_gst_multispeaker_train")
    if symbols is not None:
        cfg.text = TextConfig(symbols={"letters": symbols})
    model, _ = _pair(cfg)
    model.save_checkpoint(path, global_step=9)
    return cfg


def test_a_style_reference_per_row_does_not_depend_on_the_batch_size(tmp_path):
    _gst_checkpoint(tmp_path / "gst.ckpt")
    g = torch.Generator().manual_seed(5)
    (tmp_path / "refs").mkdir()
    rows = []
    for i, (text, frames) in enumerate([("abcdefghijkl", 31), ("cab", 9), ("fedcba", 64)]):
        torch.save(torch.randn(80, frames, generator=g), tmp_path / "refs" / f"r{i}.pt")
        rows.append(f"{text}|refs/r{i}.pt")
    fl = tmp_path / "texts.psv"
    fl.write_text("characters|style_reference\n" + "\n".join(rows) + "\n", encoding="utf8")
    bare = tmp_path / "bare.psv"
    bare.write_text("characters\n" + "\n".join(r.split("|")[0] for r in rows) + "\n", encoding="utf8")
    base = ["synthesize", tmp_path / "gst.ckpt", "-f", fl, "--exact-lengths"]
    _commands([base + ["-o", tmp_path / "b3", "-b", "3"], base + ["-o", tmp_path / "b1", "-b", "1", "--no-sort"],
               ["synthesize", tmp_path / "gst.ckpt", "-f", bare, "--exact-lengths", "-o", tmp_path / "token", "-b", "3"]])
    batched = sorted((tmp_path / "b3" / "synthesized_spec").iterdir())
    alone = sorted((tmp_path / "b1" / "synthesized_spec").iterdir())
    assert len(batched) == 3 and [p.name for p in batched] == [p.name for p in alone]
    for pb, pa in zip(batched, alone):
        got, want = torch.load(pb, weights_only=True), torch.load(pa, weights_only=True)
        assert got.shape == want.shape and want.shape[1] > 0, (pb.name, got.shape, want.shape)
        err, tol = float((got - want).abs().max()), 1e-4 * max(1.0, float(want.abs().max()))
        print(f"{pb.name}: {want.shape[1]} frames, -b 3 against -b 1 {err:.2e}, bound {tol:.2e}")
        assert err < tol, (pb.name, err, tol)
    # and the references reach the model: without the column (style token 0) the files are others
    moved = []
    for pb in batched:
        got, other = torch.load(pb, weights_only=True), torch.load(tmp_path / "token" / "synthesized_spec" / pb.name, weights_only=True)
        moved.append(got.shape != other.shape or float((got - other).abs().max()) > 1e-2)
    assert all(moved), moved


def test_teacher_forced_scores_of_a_gst_model_do_not_follow_the_batch_size(tmp_path):
    from tests.test_data_gpu import SYMBOLS, _write_corpus
    cfg = _gst_checkpoint(tmp_path / "gst.ckpt", SYMBOLS)
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    entries = _write_corpus(corpus, cfg, n_utts=5, learn_alignment=False)
    cols = ["basename", "language", "speaker", "characters", "character_tokens"]
    fl = tmp_path / "list.psv"
    fl.write_text("|".join(cols) + "\n" + "".join("|".join(e[c] for c in cols) + "\n" for e in entries), encoding="utf8")
    base = ["synthesize", tmp_path / "gst.ckpt", "-f", fl, "-T", corpus, "--return-scores", "--scores-only"]
    _commands([base + ["-o", tmp_path / "b1", "-b", "1"], base + ["-o", tmp_path / "b3", "-b", "3"]])

    def read(tag):
        with open(tmp_path / tag / "scores-9.psv", encoding="utf8", newline="") as f:
            return {r["basename"]: r for r in csv.DictReader(f, delimiter="|")}

    alone, batched = read("b1"), read("b3")
    assert sorted(alone) == sorted(batched) == sorted(e["basename"] for e in entries)
    for name, w in alone.items():
        for k in ("total", "duration", "spec", "postnet"):
            a, b = float(batched[name][k]), float(w[k])
            print(f"{name} {k}: -b 3 {a:.6f}, -b 1 {b:.6f}")
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (name, k, a, b)
