"""GPU: ``fs2hip_cepstra`` through the binding against the numpy restatement of its definition (tests/cepstra_references.py),
``FastSpeech2.mel_dtw(..., cepstra=K)`` and ``fs2l synthesize --compare-to DIR --cepstra K``.

The kernel's sum is bit-defined -- fp32, ascending m from 0.f, no contraction -- so every valid row is EQUAL to the
restatement, bit for bit, at every (C, K) that takes another path through the launch: K = 13 (4 coefficients per
wavefront), K = 64 (16 per wavefront), C = 5 with K = 4 (wavefronts without a coefficient of their own, an odd C).  Batches
of six utterances padded to T = 130 with the row counts of tests/dtw_references.LENGTHS -- 1, 63 / 64 / 65 around the 64-row
tile, 128 / 129 / 130 around the second -- and one with a zero and a negative length.  Padded input rows are NaN and the output
is pre-filled with NaN: nothing outside the valid rows may be read into a result or written.

``mel_dtw(..., cepstra=K)``: the mel results are bit-equal to the call without it, the cepstral ones to the three kernels
composed by hand; and since the table's rows are orthonormal (tests/test_cepstra_cpu.py: a contraction up to 1e-6) every
cepstral cost is at most the mel cost, so the cheapest cepstral path costs at most the mel path's total:
``cep_total <= total * (1 + 1e-5)``."""
import csv

import numpy as np
import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from tests import cepstra_references as CR
from tests import dtw_references as R

pytestmark = pytest.mark.gpu

T = R.T1                                                  # 130
ROWS = ([n for n, _ in R.LENGTHS],                        # 1, 1, 70, 63, 65, 130
        [min(r, T) for _, r in R.LENGTHS],                # 1, 70, 1, 64, 129, 130
        [0, 128, -3, 2, 64, 130])                         # an empty utterance, a negative length (clamped to 0)
SHAPES = ((80, 13), (80, 64), (5, 4))


@pytest.fixture(scope="module")
def hip():
    from fastspeech2_lightning_amd import hip as H
    return H


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("channels,K", SHAPES)
@pytest.mark.parametrize("rows", ROWS, ids=["first_lengths", "second_lengths", "empty_rows"])
def test_valid_rows_equal_the_restatement_and_nothing_else_is_written(hip, channels, K, rows):
    assert len(rows) == len(R.LENGTHS) == 6
    tab = CR.table(channels, K)
    x = np.full((6, T, channels), np.nan, dtype=np.float32)
    for b, n in enumerate(rows):
        if n > 0:
            x[b, :n] = CR.mel_like(n, channels, seed=100 * b + n)
    out = torch.full((6, T, K), float("nan"), device="cuda")
    got = hip.cepstra(torch.from_numpy(x).cuda(), _lens(rows), K, out=out)
    assert got is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert hip.dct_table(channels, K).cpu().numpy().tobytes() == tab.tobytes()
    assert hip.dct_table(channels, K) is hip.dct_table(channels, K)          # built once, kept
    for b, n in enumerate(rows):
        n = max(n, 0)
        want = CR.cepstra32(x[b, :n], tab)
        assert np.isfinite(got[b, :n]).all(), b
        assert got[b, :n].tobytes() == want.tobytes(), (b, n, np.max(np.abs(got[b, :n] - want)) if n else 0)
        assert np.isnan(got[b, n:]).all(), b


def test_a_row_does_not_depend_on_its_batch(hip):
    channels, K, n = 80, 13, 65
    x = CR.mel_like(n, channels, seed=9)
    alone = hip.cepstra(torch.from_numpy(x[None]).cuda(), _lens([n]), K)       # B = 1, T = n: no padding at all
    assert alone.shape == (1, n, K)
    padded = np.full((3, T, channels), np.nan, dtype=np.float32)
    padded[1, :n] = x
    padded[0, :5], padded[2, :T] = 1.0, 2.0
    both = hip.cepstra(torch.from_numpy(padded).cuda(), _lens([5, n, T]), K)
    assert both[1, :n].cpu().numpy().tobytes() == alone[0].cpu().numpy().tobytes()


def test_refusals(hip):
    f32 = dict(device="cuda", dtype=torch.float32)
    x, l2 = torch.zeros(2, 4, 80, **f32), _lens([4, 4])
    with pytest.raises(ValueError, match="K = 65"):
        hip.cepstra(x, l2, 65)
    with pytest.raises(ValueError, match="K = 80"):
        hip.cepstra(x, l2, 80)
    with pytest.raises(ValueError, match="K = 0"):
        hip.cepstra(x, l2, 0)
    with pytest.raises(ValueError, match=f"at most {hip.FRAME_DIST_MAX_C} channels"):
        hip.cepstra(torch.zeros(1, 2, 205, **f32), _lens([2]), 13)
    with pytest.raises(ValueError, match="lengths"):
        hip.cepstra(x, _lens([4]), 13)
    with pytest.raises(TypeError):
        hip.cepstra(x, l2.long(), 13)
    with pytest.raises(ValueError, match="out is"):
        hip.cepstra(x, l2, 13, out=torch.zeros(2, 4, 12, **f32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.cepstra(x.cpu(), l2, 13)
    # the C entry point refuses the same before any launch
    lib = hip.real_lib()
    out, wide = torch.zeros(2, 4, 80, **f32), torch.zeros(2, 4, 205, **f32)
    tab = torch.zeros(80, 205, **f32)
    args = lambda C, K: (2, 4, C, K, None)    # noqa: E731
    assert lib.fs2hip_cepstra(x.data_ptr(), l2.data_ptr(), tab.data_ptr(), out.data_ptr(), *args(80, 65)) == -22
    assert lib.fs2hip_cepstra(x.data_ptr(), l2.data_ptr(), tab.data_ptr(), out.data_ptr(), *args(80, 80)) == -22   # K = C
    assert lib.fs2hip_cepstra(wide.data_ptr(), l2.data_ptr(), tab.data_ptr(), out.data_ptr(), *args(205, 13)) == -22
    assert lib.fs2hip_cepstra(None, l2.data_ptr(), tab.data_ptr(), out.data_ptr(), *args(80, 13)) == -22
    assert lib.fs2hip_cepstra(x.data_ptr(), l2.data_ptr(), None, out.data_ptr(), *args(80, 13)) == -22
    assert lib.fs2hip_cepstra(x.data_ptr(), l2.data_ptr(), tab.data_ptr(), out.data_ptr(), 2, 0, 80, 13, None) == -22
    torch.cuda.synchronize()
    assert not out.any()


_CACHE = {}


def _setup(tmp_path_factory):
    if "setup" not in _CACHE:
        from tests.test_scores_gpu import _corpus
        root = tmp_path_factory.mktemp("cepstra")
        model, ckpt, fl, corpus, entries = _corpus(root, learn_alignment=False)
        rows = D.synthesis_entries(None, fl, None, None, 1.0, model)
        _CACHE["setup"] = (model, ckpt, fl, corpus, entries, rows)
    return _CACHE["setup"]


def test_mel_dtw_with_cepstra(tmp_path_factory):
    from fastspeech2_lightning_amd import hip
    from fastspeech2_lightning_amd.synthesis import collate_items
    model, _, _, corpus, entries, rows = _setup(tmp_path_factory)
    ds = D.SynthesisDataset(rows, model.config, model.lang2id, model.speaker2id, compare_dir=corpus)
    B = len(entries)
    batch = collate_items([ds[i] for i in range(B)], learn_alignment=False)
    ref, ref_lens = batch.pop("compare_mel"), batch.pop("compare_lens")
    out = model(batch, inference=True, exact_lengths=True)
    total, steps = model.mel_dtw(out, ref, ref_lens)
    res = model.mel_dtw(out, ref, ref_lens, cepstra=13)
    assert len(res) == 4 and res[2].dtype == torch.float32 and res[3].dtype == torch.int32
    assert torch.equal(res[0], total) and torch.equal(res[1], steps)
    # the three kernels by hand
    y, lens, r, rl = out[model.output_key].contiguous(), out["tgt_lens"], ref.cuda(), ref_lens.cuda()
    cost = hip.frame_dist(hip.cepstra(y, lens, 13), lens, hip.cepstra(r, rl, 13), rl)
    t2, s2 = hip.dtw(cost, lens, rl)
    assert torch.equal(res[2], t2) and torch.equal(res[3], s2)
    tot, cep, st, cst = total.tolist(), res[2].tolist(), steps.tolist(), res[3].tolist()
    print("total", tot, "cep_total", cep, "steps", st, "cep_steps", cst)
    assert all(s > 0 for s in st) and all(c > 0 for c in cep)
    for u in range(B):
        assert cep[u] <= tot[u] * (1 + 1e-5), (u, cep[u], tot[u])
        assert (cst[u] > 0) == (st[u] > 0)
    table = torch.full((4 * B,), float("nan"), device="cuda")
    again = model.mel_dtw(out, ref, ref_lens, out=table, cepstra=13)
    assert torch.equal(table[:B], total) and torch.equal(table[B:2 * B].view(torch.int32), steps)
    assert torch.equal(table[2 * B:3 * B], res[2]) and torch.equal(table[3 * B:].view(torch.int32), res[3])
    assert all(torch.equal(a, b) for a, b in zip(again, res))
    with pytest.raises(ValueError, match=f"{4 * B} fp32"):
        model.mel_dtw(out, ref, ref_lens, out=torch.zeros(2 * B, device="cuda"), cepstra=13)
    with pytest.raises(ValueError, match="cepstra = 16"):
        model.mel_dtw(out, ref, ref_lens, cepstra=16)                      # n_mels = 16: at most 15
    paths = model.mel_dtw_paths(out, ref, ref_lens, cepstra=13)
    plain = model.mel_dtw_paths(out, ref, ref_lens)
    assert len(paths) == 7 and len(plain) == 5
    assert torch.equal(paths[5], res[2]) and torch.equal(paths[6], res[3])
    n = out["tgt_lens"].tolist()
    for a, b in zip(paths[:5], plain):
        if a.dim() == 1:
            assert torch.equal(a, b)
        else:
            assert all(torch.equal(a[u, :n[u]], b[u, :n[u]]) for u in range(B))      # the path stays the mel path


def _read(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.DictReader(f, delimiter="|"))


def test_the_command_writes_the_cepstral_columns(tmp_path, tmp_path_factory):
    model, ckpt, fl, corpus, entries, _ = _setup(tmp_path_factory)
    plain, cep = tmp_path / "plain", tmp_path / "cep"
    base = ["synthesize", str(ckpt), "-f", str(fl), "--compare-to", str(corpus), "-b", "2"]
    assert cli.main(base + ["-o", str(plain)]) == 0
    assert cli.main(base + ["-o", str(cep), "--cepstra", "13"]) == 0
    a, b = _read(plain / "dtw-9.psv"), _read(cep / "dtw-9.psv")
    assert (cep / "dtw-9.psv").read_text(encoding="utf8").splitlines()[0] == (
        "basename|speaker|language|mel_dtw|total|steps|cep_dtw|cep_total|cep_steps|frames|ref_frames|frame_ratio|raw_text")
    assert len(a) == len(b) == len(entries)
    for ra, rb in zip(a, b):
        assert float(rb["cep_dtw"]) == float(rb["cep_total"]) / int(rb["cep_steps"]) > 0
        assert float(rb["cep_total"]) <= float(rb["total"]) * (1 + 1e-5)
        assert {k: v for k, v in rb.items() if not k.startswith("cep_")} == ra     # every other column, the same text
    files_a, files_b = sorted((plain / "synthesized_spec").iterdir()), sorted((cep / "synthesized_spec").iterdir())
    assert [p.name for p in files_a] == [p.name for p in files_b] and len(files_a) == len(entries)
    for pa, pb in zip(files_a, files_b):
        assert pa.read_bytes() == pb.read_bytes(), pa.name
