"""Length-bucketed batches, host side (``data.LengthBucketBatchSampler``, ``FeatureDataset.lengths``, ``collate_bucketed``,
``fs2l train --bucket-lengths --dry-run``): every item once per epoch, an order that depends only on (seed, epoch,
world), equal batch counts over the ranks, at most ``2 * n_buckets`` batch geometries per epoch, and no more padded mel
rows than random batches padded to their own maxima."""
import json
import subprocess
import sys
from collections import Counter
from pathlib import Path

import pytest
import torch

from fastspeech2_lightning_amd import cli
from fastspeech2_lightning_amd import data as D
from fastspeech2_lightning_amd import plan as PL
from fastspeech2_lightning_amd.synthetic import synthetic_item, synthetic_lengths
from tests.test_cli_cpu import make_project

REPO = Path(__file__).resolve().parent.parent

#: (name, lengths, batch size, buckets): LJSpeech-shaped, fewer items than buckets, all lengths equal, one item
CASES = [
    ("ljspeech", synthetic_lengths(1000, seed=3), 32, 8),
    ("ljspeech_b64", synthetic_lengths(1300, seed=4), 64, 8),
    ("odd_sizes", synthetic_lengths(517, seed=5), 7, 5),
    ("fewer_items_than_buckets", synthetic_lengths(5, seed=6), 4, 8),
    ("all_equal", [(30, 150)] * 100, 8, 8),
    ("one_item", [(12, 40)], 4, 8),
]
IDS = [c[0] for c in CASES]


def sampler(lengths, bs, nb, **kw):
    return D.LengthBucketBatchSampler(lengths, bs, nb, **{"seed": 11, **kw})


@pytest.mark.parametrize("name,lengths,bs,nb", CASES, ids=IDS)
def test_every_item_once_per_epoch_and_every_item_fits_its_geometry(name, lengths, bs, nb):
    s = sampler(lengths, bs, nb)
    batches = list(s)
    assert len(batches) == len(s)
    seen = Counter(i for b in batches for i in b)
    assert sorted(seen) == list(range(len(lengths))) and set(seen.values()) == {1}
    for b in batches:
        assert 1 <= len(b) <= bs
        Ts_b, Tm_b = b.geometry
        assert all(lengths[i][0] <= Ts_b and lengths[i][1] <= Tm_b for i in b)
        assert all(s.geometry_of(i) == b.geometry for i in b)
    geos = {(len(b),) + b.geometry for b in batches}
    assert len(geos) <= 2 * nb, (len(geos), nb)          # full + leftover per bucket
    assert len(s.buckets) <= nb
    # a bucket's geometry is the maxima over its members, buckets are contiguous in mel length
    tops = []
    for geo, members in s.buckets:
        assert geo == (max(lengths[i][0] for i in members), max(lengths[i][1] for i in members))
        tops.append((min(lengths[i][1] for i in members), geo[1]))
    assert all(a[1] <= b[0] for a, b in zip(tops, tops[1:]))


def test_buckets_hold_about_equally_many_items_and_round_up_to_the_step():
    lengths = synthetic_lengths(1000, seed=3)
    s = sampler(lengths, 32, 8)
    sizes = [len(m) for _, m in s.buckets]
    assert len(sizes) == 8 and max(sizes) - min(sizes) <= 1
    r = sampler(lengths, 32, 8, step=16)
    for (geo, members), (geo1, members1) in zip(r.buckets, s.buckets):
        assert members == members1
        assert geo[0] % 16 == 0 and geo[1] % 16 == 0 and 0 <= geo[0] - geo1[0] < 16 and 0 <= geo[1] - geo1[1] < 16
    assert D.LengthBucketBatchSampler(lengths, 32).n_buckets == PL.MAX_PLANS   # the default bucket count is the plan limit


def test_the_order_depends_only_on_seed_epoch_and_world():
    lengths = synthetic_lengths(400, seed=8)
    a = [list(b) for b in sampler(lengths, 16, 6, epoch=3)]
    b = [list(b) for b in sampler(lengths, 16, 6, epoch=3)]
    c = [list(b) for b in sampler(lengths, 16, 6, epoch=4)]
    d = [list(b) for b in sampler(lengths, 16, 6, epoch=3, seed=12)]
    assert a == b and a != c and a != d
    s = sampler(lengths, 16, 6, epoch=0)
    s.set_epoch(3)
    assert [list(x) for x in s] == a
    # the full batches of all buckets are shuffled together: the epoch does not walk through the buckets in order
    order = [x.bucket for x in sampler(lengths, 16, 6, epoch=3)]
    assert order != sorted(order)


@pytest.mark.parametrize("skip", [0, 1, 7, 10 ** 6])
def test_skip_batches_gives_the_tail_of_the_same_order(skip):
    lengths = synthetic_lengths(300, seed=9)
    for world, rank in ((1, 0), (3, 1)):
        whole = [list(b) for b in sampler(lengths, 8, 5, epoch=2, world=world, rank=rank)]
        tail = sampler(lengths, 8, 5, epoch=2, world=world, rank=rank, skip_batches=skip)
        assert [list(b) for b in tail] == whole[skip:] and len(tail) == len(whole[skip:])


@pytest.mark.parametrize("name,lengths,bs,nb", CASES, ids=IDS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_ranks_get_equal_counts_disjoint_batches_and_fewer_than_world_repeats(name, lengths, bs, nb, world):
    per_rank = [list(sampler(lengths, bs, nb, epoch=1, world=world, rank=r)) for r in range(world)]
    assert len({len(x) for x in per_rank}) == 1                      # the per-bucket all-reduce needs equal step counts
    every = [b for x in per_rank for b in x]
    unique = {tuple(b): b for b in every}
    assert len(every) - len(unique) < world                          # the evening-out repeats
    seen = Counter(i for b in unique.values() for i in b)
    assert sorted(seen) == list(range(len(lengths))) and set(seen.values()) == {1}   # disjoint, nothing dropped
    rows = sampler(lengths, bs, nb, epoch=1, world=world).rows()
    assert [[list(b) for b in row] for row in rows] == [[list(per_rank[r][i]) for r in range(world)] for i in range(len(rows))]
    # the batches of one global position share a geometry where possible: every bucket's full batches fill whole rows
    # as far as they go, so at most (world - 1) full batches per bucket sit in a mixed row
    mixed = Counter()
    for row in rows:
        if len({(len(b),) + b.geometry for b in row}) > 1:
            mixed.update(b.bucket for b in {tuple(b): b for b in row}.values() if len(b) == bs)   # (repeats count once)
    assert all(n < world for n in mixed.values()), mixed


@pytest.mark.parametrize("bs", [32, 64])
def test_bucketing_never_pads_more_mel_rows_than_random_batches(bs):
    """A condition, not a measurement: with the default bucket count on LJSpeech-shaped lengths, the epoch's padded mel
    rows are at most those of ``RandomSampler`` + ``BatchSampler`` (what ``fs2l train`` draws without the switch) on the
    same lengths and seed."""
    for seed in (0, 1, 2):
        lengths = synthetic_lengths(2000, seed=20 + seed)
        s = D.LengthBucketBatchSampler(lengths, bs, seed=seed, epoch=0)
        rand = D.random_batches(len(lengths), bs, seed)
        assert sorted(i for b in rand for i in b) == list(range(len(lengths)))
        plain = sum(len(b) * max(lengths[i][1] for i in b) for b in rand)
        bucketed = sum(len(b) * b.geometry[1] for b in s)
        real = sum(m for _, m in lengths)
        assert real <= bucketed <= plain, (real, bucketed, plain)
        assert bucketed == s.padded_mel_rows()
        d = s.describe()
        assert d["padded_frame_share_bucketed"] <= d["padded_frame_share_unbucketed"]
        assert d["distinct_geometries"] <= 2 * PL.MAX_PLANS


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        D.LengthBucketBatchSampler([(1, 2)], 0)
    with pytest.raises(ValueError):
        D.LengthBucketBatchSampler([(1, 2)], 4, world=2, rank=2)
    assert list(D.LengthBucketBatchSampler([], 4)) == []


def test_collate_bucketed_keeps_collate_and_adds_the_geometry():
    lengths = [(5, 20), (7, 31), (6, 25), (9, 44), (8, 40)]
    s = sampler(lengths, 2, 2)
    items = [synthetic_item(t, m, n_mels=8, seed=i) for i, (t, m) in enumerate(lengths)]
    ds = D.BucketedDataset(items, s)
    for b in s:
        got = D.collate_bucketed([ds[i] for i in b], learn_alignment=False)
        want = D.collate([items[i] for i in b], learn_alignment=False)
        assert got.pop("bucket_geometry") == b.geometry
        assert got.pop("bucket_leftover") is (len(b) != 2)   # a bucket's short last batch: run eagerly, never recorded
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k
        assert int(got["max_src_len"]) <= b.geometry[0] and int(got["max_mel_len"]) <= b.geometry[1]
    with pytest.raises(ValueError, match="different buckets"):
        D.collate_bucketed([ds[0], ds[3]], learn_alignment=False)


def dataset(tmp_path, **kw):
    cfg = make_project(tmp_path, write_features=True, **kw)
    p = cli.plan(cli.build_parser().parse_args(["train", str(cfg)]))
    return D.FeatureDataset(p["train_rows"], p["config"], p["lang2id"], p["speaker2id"]), p


def test_lengths_cache_round_trips_and_a_changed_filelist_invalidates_it(tmp_path, monkeypatch):
    ds, p = dataset(tmp_path, n_train=6, n_val=2)
    cache = tmp_path / "run" / "lengths.json"
    got = ds.lengths(cache)
    assert got == [(len(ds[i]["text"]), ds[i]["mel"].shape[0]) for i in range(len(ds))]
    stored = json.loads(cache.read_text())
    assert stored["n"] == 6 and sorted(stored["lengths"]) == sorted(f"{e['basename']}--{e['speaker']}--{e['language']}" for e in ds.entries)
    # a second dataset reads the cache: no feature file is opened
    def no_load(self, *a):
        raise AssertionError(f"feature file read despite the cache: {a}")
    monkeypatch.setattr(D.FeatureDataset, "_load", no_load)
    again = D.FeatureDataset(ds.entries, ds.config, ds.lang2id, ds.speaker2id)
    assert again.lengths(cache) == got and again.lengths(cache) is again.lengths()
    monkeypatch.undo()
    # another filelist length, or other names of the same count: measured again and rewritten
    fewer = D.FeatureDataset(ds.entries[:4], ds.config, ds.lang2id, ds.speaker2id)
    assert fewer.lengths(cache) == got[:4] and json.loads(cache.read_text())["n"] == 4
    other = D.FeatureDataset(ds.entries[2:6], ds.config, ds.lang2id, ds.speaker2id)
    assert other.lengths(cache) == got[2:6]
    assert sorted(json.loads(cache.read_text())["lengths"]) == sorted(f"{e['basename']}--{e['speaker']}--{e['language']}" for e in ds.entries[2:6])
    # a cache written for another text representation (its lengths count other tokens) is not trusted
    stored = json.loads(cache.read_text())
    assert stored["text"].startswith(("phones/", "characters/"))
    stored["text"] = ("characters" if stored["text"].startswith("phones") else "phones") + "/" + stored["text"].split("/")[1]
    stored["lengths"] = {k: [v[0] + 3, v[1]] for k, v in stored["lengths"].items()}
    cache.write_text(json.dumps(stored))
    fresh = D.FeatureDataset(ds.entries[2:6], ds.config, ds.lang2id, ds.speaker2id)
    assert fresh.lengths(cache) == got[2:6] and json.loads(cache.read_text())["text"] != stored["text"]
    # an unreadable cache is measured again; write=False leaves the file alone
    cache.write_text("{not json")
    ro = D.FeatureDataset(ds.entries, ds.config, ds.lang2id, ds.speaker2id)
    assert ro.lengths(cache, write=False) == got and cache.read_text() == "{not json"


def test_dry_run_prints_the_bucket_table_without_a_gpu(tmp_path):
    cfg = make_project(tmp_path, n_train=23, n_val=2, write_features=True)
    env_cmd = [sys.executable, str(REPO / "fs2l"), "train", str(cfg), "--bucket-lengths", "3", "--dry-run", "--seed", "5"]
    r = subprocess.run(env_cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plan = json.loads(r.stdout.strip().splitlines()[-1])
    rep = plan["bucket_lengths"]
    assert rep["n_buckets"] == len(rep["buckets"]) <= 3
    assert sum(b["items"] for b in rep["buckets"]) == 23 and plan["train_utterances"] == 23
    for b in rep["buckets"]:
        assert b["batches_per_epoch"] == -(-b["items"] // 4) and b["Ts"] > 0 and b["Tm"] >= b["Ts"]
    assert rep["batches_per_epoch_per_rank"] == sum(b["batches_per_epoch"] for b in rep["buckets"])
    assert 0.0 <= rep["padded_frame_share_bucketed"] <= rep["padded_frame_share_unbucketed"] < 1.0
    assert (tmp_path / "logs" / "exp" / "v0" / "lengths.json").exists()
    # without a value the bucket count is the plan limit; without the switch the plan is what it was
    args = cli.build_parser().parse_args(["train", str(cfg), "--bucket-lengths"])
    assert cli.bucket_count(args) == PL.MAX_PLANS
    assert cli.bucket_count(cli.build_parser().parse_args(["train", str(cfg)])) is None
    r = subprocess.run([sys.executable, str(REPO / "fs2l"), "train", str(cfg), "--dry-run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bucket_lengths" not in json.loads(r.stdout.strip().splitlines()[-1])


def test_more_buckets_than_plans_warns_once_and_keeps_the_limit(tmp_path, capsys):
    cfg = make_project(tmp_path)
    args = cli.build_parser().parse_args(["train", str(cfg), "--bucket-lengths", str(PL.MAX_PLANS + 4)])
    limit = PL.MAX_PLANS
    assert cli.bucket_count(args) == limit + 4
    err = capsys.readouterr().err
    assert err.count("warning") == 1 and "FS2_PLAN_MAX" in err
    assert PL.MAX_PLANS == limit
