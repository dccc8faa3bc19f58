"""GPU: ``fs2l synthesize`` end to end.  The yardstick is ``FastSpeech2.predict_step`` (pinned by the oracle parity tests)
on the batches ``synthesis_batches`` names, collated from the same dataset: every file must equal it bit for bit."""
import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import config as cfgmod
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd.config import InferenceControl, Stats, TextConfig
from oracle import cases as C

pytestmark = pytest.mark.gpu

STEP = 4321
#: seven texts of 1 to 12 table symbols (the small configuration's table: the letters a..w)
TEXTS = ["a", "bcd", "abcdefghijkl", "cab", "fedcba", "hgfedcbai", "ab"]
_CACHE = {}


def _build(cfg):
    from fastspeech2_lightning_amd.model import FastSpeech2
    torch.manual_seed(0)
    m = FastSpeech2(cfg, Stats(**C.STATS), lang2id=C.LANG2ID, speaker2id=C.SPEAKER2ID)
    sd = m.state_dict()
    sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([1.2])  # a useful spread of durations
    m.load_state_dict(sd)
    return m.eval()


def _small(tmp_path_factory):
    """The small free-synthesis model and its checkpoint, built once (inside a test: after the per-test fixtures)."""
    if "small" not in _CACHE:
        model = _build(C.small_config(learn_alignment=False))
        path = tmp_path_factory.mktemp("ckpt") / "small.ckpt"
        model.save_checkpoint(path, global_step=STEP)
        _CACHE["small"] = (model, path)
    return _CACHE["small"]


def _dataset(model, texts, duration_control=1.0, **kw):
    entries = D.synthesis_entries(list(texts), None, None, None, duration_control, model)
    return D.SynthesisDataset(entries, model.config, model.lang2id, model.speaker2id, **kw)


def _expected(model, ds, batch_size, control=None, sort=True):
    """{item index: [n_mels, frames]} from the parent-commit forward on the batches ``synthesis_batches`` names."""
    out = {}
    for idx in D.synthesis_batches(ds.token_counts, batch_size, sort):
        batch = D.collate([ds[i] for i in idx], learn_alignment=model.config.model.learn_alignment)
        if control is None:
            res = model.predict_step(batch)
        else:
            res = model(batch, control.model_copy(), inference=True)
        lens = res["tgt_lens"].tolist()
        for j, i in enumerate(idx):
            out[i] = res[model.output_key][j, :lens[j]].T.cpu()
    return out


def _names(out_dir, texts, step=STEP):
    ref = D.SpecWriter(out_dir, "postnet_output", global_step=step)
    return [ref.filename(D.truncate_basename(D.slugify(t)), "spk0", "l0") for t in texts]


def _run_cli(ckpt, out_dir, texts, *extra):
    argv = ["synthesize", str(ckpt), "-o", str(out_dir), "-b", "3", *extra]
    for t in texts:
        argv += ["-t", t]
    assert cli.main(argv) == 0
    return sorted((out_dir / "synthesized_spec").iterdir())


def test_free_synthesis_through_the_command(tmp_path, tmp_path_factory):
    model, ckpt = _small(tmp_path_factory)
    files = _run_cli(ckpt, tmp_path, TEXTS)
    want_names = _names(tmp_path, TEXTS)
    assert len(files) == 7 and sorted(files) == sorted(want_names)
    assert all(f"ckpt={STEP}" in p.name for p in files)
    want = _expected(model, _dataset(model, TEXTS), 3)
    n_mels = model.config.preprocessing.audio.n_mels
    for i, p in enumerate(want_names):
        got = torch.load(p, weights_only=True)
        assert got.shape == want[i].shape and got.shape[0] == n_mels and got.shape[1] > 0 and got.is_contiguous()
        assert torch.equal(got, want[i]), TEXTS[i]


def test_controls_reach_the_model(tmp_path, tmp_path_factory):
    model, ckpt = _small(tmp_path_factory)
    _run_cli(ckpt, tmp_path, TEXTS, "-D", "1.5", "--pitch-control", "0.8")
    want = _expected(model, _dataset(model, TEXTS, duration_control=1.5), 3, InferenceControl(pitch=0.8, duration=1.5))
    plain = _expected(model, _dataset(model, TEXTS), 3)
    frames = []
    for i, p in enumerate(_names(tmp_path, TEXTS)):
        got = torch.load(p, weights_only=True)
        assert torch.equal(got, want[i]), TEXTS[i]
        frames.append(got.shape[1])
    assert any(f != plain[i].shape[1] for i, f in enumerate(frames))   # -D 1.5 changed at least one frame count


def test_pipelined_and_synchronous_loops_write_the_same_bytes(tmp_path, tmp_path_factory):
    from fastspeech2_lightning_amd.synthesis import synthesize
    model, _ = _small(tmp_path_factory)
    texts = [TEXTS[i % 7] + "wv"[: i // 7 + 1] for i in range(11)]     # eleven distinct texts: six batches of two
    results = {}
    for depth in (2, 1):
        ds = _dataset(model, texts)
        w = D.PackedSpecWriter(tmp_path / f"depth{depth}", model.output_key, STEP, n_mels=16)
        res = synthesize(model, ds, 2, InferenceControl(), w, sort=True, depth=depth)
        assert res["batches"] == 6 and len(res["files"]) == 11
        assert [p.name for p in res["files"]] == [p.name for p in _names(tmp_path / f"depth{depth}", texts)]  # input order
        results[depth] = [torch.load(p, weights_only=True) for p in res["files"]]
    for a, b in zip(results[2], results[1]):
        assert a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()
    want = _expected(model, _dataset(model, texts), 2)
    assert all(torch.equal(results[2][i], want[i]) for i in range(11))


def test_chunks_separated_by_sorting_are_joined_in_input_order(tmp_path, tmp_path_factory):
    from fastspeech2_lightning_amd.synthesis import synthesize
    model, _ = _small(tmp_path_factory)
    texts = ["cab", "ab", "abcdefghijkl", "fedcba", "b"]
    last = [True, False, True, True, True]                 # "ab" + "abcdefghijkl" are two chunks of one text
    entries = D.synthesis_entries(texts, None, None, None, 1.0, model)
    for e, flag in zip(entries, last):
        e["is_last_input_chunk"] = flag
    ds = D.SynthesisDataset(entries, model.config, model.lang2id, model.speaker2id)
    batches = D.synthesis_batches(ds.token_counts, 2)
    where = {i: k for k, b in enumerate(batches) for i in b}
    assert where[1] != where[2]                            # sorting did separate the chunks
    w = D.PackedSpecWriter(tmp_path / "packed", model.output_key, STEP, n_mels=16)
    res = synthesize(model, ds, 2, None, w, sort=True)
    joined = ["cab", "ababcdefghijkl", "fedcba", "b"]
    assert [p.name for p in res["files"]] == [p.name for p in _names(tmp_path / "packed", joined)]
    got = [torch.load(p, weights_only=True) for p in res["files"]]
    # the pieces are what the forward gives in the sorted batches, joined in input order
    want = _expected(model, ds, 2)
    assert torch.equal(got[1], torch.cat([want[1], want[2]], -1))
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[3]) and torch.equal(got[3], want[4])
    # and the result is what SpecWriter.write produces for the unsorted sequence
    ref = D.SpecWriter(tmp_path / "plain", model.output_key, STEP)
    paths = []
    for idx in D.synthesis_batches(ds.token_counts, 2, sort=False):
        batch = D.collate([ds[i] for i in idx], learn_alignment=False)
        paths += ref.write(model.predict_step(batch), batch)
    assert [p.name for p in paths] == [p.name for p in res["files"]]
    for p, g in zip(paths, got):
        r = torch.load(p, weights_only=True)
        print("chunks: frames", tuple(r.shape), tuple(g.shape), "max |diff|",
              float((r - g).abs().max()) if r.shape == g.shape and r.numel() else None)
        assert torch.equal(r, g)


@pytest.mark.parametrize("learn_alignment", [False, True])
def test_teacher_forcing_directory(tmp_path, learn_alignment):
    from tests.test_data_gpu import SYMBOLS, _write_corpus
    cfg = C.small_config(learn_alignment=learn_alignment)
    cfg.text = TextConfig(symbols={"letters": SYMBOLS})
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    entries = _write_corpus(corpus, cfg, n_utts=5, learn_alignment=learn_alignment)
    model = _build(cfg)
    ckpt = tmp_path / "tf.ckpt"
    model.save_checkpoint(ckpt, global_step=9)
    fl = tmp_path / "list.psv"
    cols = ["basename", "language", "speaker", "characters", "character_tokens"]
    fl.write_text("|".join(cols) + "\n" + "".join("|".join(e[c] for c in cols) + "\n" for e in entries), encoding="utf8")
    out = tmp_path / "out"
    assert cli.main(["synthesize", str(ckpt), "-f", str(fl), "-T", str(corpus), "-o", str(out), "-b", "2"]) == 0
    rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, teacher_forcing_dir=corpus)
    want = _expected(model, ds, 2)
    audio = cfg.preprocessing.audio
    for i, e in enumerate(entries):
        p = _names(out, [e["characters"]], step=9)[0]
        got = torch.load(p, weights_only=True)
        stored = torch.load(D.feature_path(corpus, "spec", e["basename"], "spk0", "l0",
                                           f"spec-{audio.input_sampling_rate}-{audio.spec_type}.pt"), weights_only=True)
        assert got.shape == stored.shape          # frame counts are the stored mel lengths
        assert torch.equal(got, want[i]), e["basename"]


def test_style_reference(tmp_path):
    cfg = C.small_config(learn_alignment=False, gst=True, n_mels=80)
    d = 256  # the style token layer emits 256 dims: the model width must match (oracle.cases.build)
    conf = dict(layers=1, heads=2, input_dim=d, feedforward_dim=64, conv_kernel_size=9, dropout=0.0)
    vp = dict(n_layers=1, kernel_size=3, dropout=0.0, input_dim=d, n_bins=16, depthwise=True)
    dump = cfg.model_checkpoint_dump()
    dump["model"].update(encoder=conf, decoder=conf,
                         variance_predictors=dict(energy=dict(vp, level="phone"), pitch=dict(vp, level="phone"), duration=vp))
    model = _build(cfgmod.FastSpeech2Config(**dump))
    ckpt = tmp_path / "gst.ckpt"
    model.save_checkpoint(ckpt, global_step=5)
    mel = torch.randn(80, 48, generator=torch.Generator().manual_seed(2))
    torch.save(mel, tmp_path / "ref.pt")
    texts = TEXTS[:4]
    _run_cli(ckpt, tmp_path / "styled", texts, "-S", str(tmp_path / "ref.pt"))
    _run_cli(ckpt, tmp_path / "token0", texts)
    styled_ds = _dataset(model, texts, style_reference=mel)
    assert styled_ds[0]["mel_style_reference"].shape == (48, 80)
    styled, token0 = _expected(model, styled_ds, 3), _expected(model, _dataset(model, texts), 3)
    differs = False
    for i, t in enumerate(texts):
        a = torch.load(_names(tmp_path / "styled", [t], step=5)[0], weights_only=True)
        b = torch.load(_names(tmp_path / "token0", [t], step=5)[0], weights_only=True)
        assert torch.equal(a, styled[i]) and torch.equal(b, token0[i])
        differs = differs or a.shape != b.shape or not torch.equal(a, b)
    assert differs


def test_style_reference_is_refused_without_the_gst_module(tmp_path, tmp_path_factory):
    _, ckpt = _small(tmp_path_factory)
    torch.save(torch.zeros(16, 8), tmp_path / "ref.pt")
    with pytest.raises(ValueError, match="global style token"):
        cli.main(["synthesize", str(ckpt), "-t", "abc", "-S", str(tmp_path / "ref.pt"), "-o", str(tmp_path / "out")])
