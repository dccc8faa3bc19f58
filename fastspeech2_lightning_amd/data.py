"""Batch producer for the hot path: per-utterance feature files -> collated
batch dict -> pinned, asynchronously prefetched device batches; spectrogram writers; validation loop; and the data
side of ``fs2l synthesize``: text -> inference items -> length-sorted batches (``synthesis_entries``, ``SynthesisDataset``,
``synthesis_batches``, ``PackedSpecWriter``).

Restates, without the parent toolkit, the parts of the reference that sit directly either side of the step:
  * on-disk layout ``<save_dir>/<kind>/<basename>--<speaker>--<language>--<suffix>.pt`` and the item dict of
    ``FastSpeechDataset.__getitem__`` (reference ``fs2/dataset.py:53-57``, ``:99-224``);
  * ``collate_method`` (reference ``fs2/dataset.py:257-293``) -- the input contract of ``FastSpeech2.forward``;
  * the ``.pt`` spectrogram output ``[n_mels, frames]`` trimmed by ``tgt_lens`` with chunk concatenation
    (reference ``fs2/prediction_writing_callback.py:257-277``);
  * ``validation_step`` + ``log_dict(sync_dist=True)`` (reference ``fs2/model.py:515-528``).
Host code only: the device work stays in ``FastSpeech2``.
"""
from __future__ import annotations

import threading
from pathlib import Path
from typing import Iterable, Iterator, Optional

import numpy as np
import torch

SEP = "--"


def feature_path(save_dir, kind: str, basename: str, speaker: str, language: str, suffix: str) -> Path:
    return Path(save_dir) / kind / SEP.join([basename, speaker, language, suffix])


ATTN_PRIOR_MODES = ("files", "computed")


def _attn_prior_mode(mode: str) -> str:
    if mode not in ATTN_PRIOR_MODES:
        raise ValueError(f"attn_prior must be one of {ATTN_PRIOR_MODES}, got {mode!r}")
    return mode


class FeatureDataset(torch.utils.data.Dataset):
    """Training / teacher-forcing items of ``FastSpeechDataset`` (the inference branch: ``SynthesisDataset``).

    ``attn_prior`` (a model that learns its alignment): ``"files"`` loads every item's ``attn/...-attn-prior.pt`` as the
    reference does; ``"computed"`` opens no prior file and leaves the item's ``duration`` None -- the model computes the
    prior on the GPU from the batch's lengths (``hip.attn_prior``)."""

    def __init__(self, entries: list[dict], config, lang2id: dict, speaker2id: dict, text_processor=None,
                 attn_prior: str = "files"):
        from .config import TextProcessor

        self.attn_prior = _attn_prior_mode(attn_prior)
        self.entries, self.config = entries, config
        self.lang2id, self.speaker2id = lang2id, speaker2id
        self.text_processor = text_processor or TextProcessor(config.text)
        self.save_dir = Path(config.preprocessing.save_dir)
        audio = config.preprocessing.audio
        self.sampling_rate = audio.input_sampling_rate
        self.spec_type = getattr(audio, "spec_type", "mel-librosa")

    def _load(self, bn, spk, lang, kind, fn):
        return torch.load(feature_path(self.save_dir, kind, bn, spk, lang, fn), weights_only=True)

    def __len__(self):
        return len(self.entries)

    def _names(self) -> list:
        return [SEP.join([e["basename"], e.get("speaker", "default"), e.get("language", "default")]) for e in self.entries]

    def lengths(self, cache=None, write: bool = True) -> list:
        """``[(text_len, mel_len), ...]`` of every item, for ``LengthBucketBatchSampler``.  The text length is the encoded
        token count of the filelist row; the mel length is read from the item's spectrogram file -- once: the result is
        kept on the dataset and, with ``cache`` (``<run dir>/lengths.json``), on disk as JSON keyed by
        ``basename--speaker--language``.  A cache written for another filelist (another item count, or a name it does
        not hold) or for another text representation (characters / phones, symbol count) is ignored and rewritten (``write=False``: only read -- the ranks other than the first)."""
        import json

        from .config import TargetTrainingTextRepresentationLevel as L
        if getattr(self, "_lengths", None) is not None and len(self._lengths) == len(self.entries):
            return self._lengths
        names = self._names()
        chars = self.config.model.target_text_representation_level == L.characters
        level = ("characters" if chars else "phones") + f"/{len(self.text_processor.symbols)}"  # what the text lengths count
        cache = Path(cache) if cache is not None else None
        if cache is not None and cache.exists():
            try:
                with open(cache, encoding="utf8") as f:
                    stored = json.load(f)
                table = stored["lengths"]
                if stored["n"] == len(names) and stored.get("text") == level and all(n in table for n in names):
                    self._lengths = [(int(table[n][0]), int(table[n][1])) for n in names]
                    return self._lengths
            except (ValueError, KeyError, TypeError, IndexError):
                pass  # unreadable: measured again below
        spec = f"spec-{self.sampling_rate}-{self.spec_type}.pt"
        out = []
        for e in self.entries:
            tokens = e["character_tokens" if chars else "phone_tokens"]
            n_text = len(self.text_processor.encode_escaped_string_sequence(tokens))
            mel = self._load(e["basename"], e.get("speaker", "default"), e.get("language", "default"), "spec", spec)
            out.append((int(n_text), int(mel.shape[1])))
        self._lengths = out
        if cache is not None and write:
            cache.parent.mkdir(parents=True, exist_ok=True)
            tmp = cache.with_suffix(".tmp")
            with open(tmp, "w", encoding="utf8") as f:
                json.dump({"n": len(names), "text": level, "lengths": {n: list(l) for n, l in zip(names, out)}}, f)
            tmp.replace(cache)
        return out

    def __getitem__(self, index):
        from .config import TargetTrainingTextRepresentationLevel as L

        item = self.entries[index]
        speaker, language = item.get("speaker", "default"), item.get("language", "default")
        bn = item["basename"]
        m = self.config.model
        mel = self._load(bn, speaker, language, "spec", f"spec-{self.sampling_rate}-{self.spec_type}.pt").transpose(0, 1)
        chars = m.target_text_representation_level == L.characters
        if m.learn_alignment:
            duration = None
            if self.attn_prior == "files":
                duration = self._load(bn, speaker, language, "attn", ("characters" if chars else "phones") + "-attn-prior.pt")
        else:
            try:
                duration = self._load(bn, speaker, language, "duration", "duration.pt")
            except FileNotFoundError as e:
                raise ValueError("model.learn_alignment = false requires text/audio alignments in "
                                 "'preprocessed/duration' (fs2/dataset.py:144-151)") from e
        tokens = item["character_tokens" if chars else "phone_tokens"]
        text = torch.IntTensor(self.text_processor.encode_escaped_string_sequence(tokens))
        pfs = None
        if m.target_text_representation_level == L.phonological_features:
            pfs = self._load(bn, speaker, language, "pfs", "pfs.pt")
        return {
            "mel": mel, "mel_style_reference": None, "duration": duration,
            "duration_control": item.get("duration_control", 1.0), "pfs": pfs, "text": text,
            "raw_text": item.get("characters", item.get("phones", "text")), "basename": bn,
            "speaker": speaker, "speaker_id": self.speaker2id[speaker], "language": language,
            "language_id": self.lang2id[language],
            "energy": self._load(bn, speaker, language, "energy", "energy.pt"),
            "pitch": self._load(bn, speaker, language, "pitch", "pitch.pt"),
            "is_last_input_chunk": None,
        }


def _padded(seqs: list, shape_tail_max: tuple, pin: bool) -> torch.Tensor:
    """One zero-initialised [B, *max extents] buffer (pinned when the prefetcher asked for it) with every sequence
    written into its top-left corner -- the batch tensor is built in the memory the H2D copy will read."""
    first = seqs[0]
    out = torch.zeros((len(seqs),) + shape_tail_max, dtype=first.dtype, pin_memory=pin)
    for row, seq in zip(out, seqs):
        row[tuple(slice(0, n) for n in seq.shape)] = seq
    return out


def collate(items: list[dict], learn_alignment: bool = True, pin_memory: bool = False) -> dict:
    """Batch contract of the reference's ``FastSpeech2DataModule.collate_method`` (fs2/dataset.py:257-293), produced
    column by column: every key of the items becomes a list; tensor / ndarray columns become one zero-padded tensor
    (ragged in time -- and, for the attention prior of a learned-alignment model, in tokens too: it is padded to
    (max_mel_len, max_src_len) even when no utterance reaches both); int columns become int32 vectors; anything else
    (names, raw text, None placeholders) stays a list.  ``src_lens`` / ``mel_lens`` are int32, the two maxima are
    0-dim int32 tensors, and a batch without mels (inference) gets ``mel_lens = None, max_mel_len = 1_000_000``.
    ``pin_memory``: allocate the padded tensors in pinned host memory (``DevicePrefetcher`` copies from them)."""
    columns = {key: [item[key] for item in items] for key in items[0]}
    src_lens = torch.tensor([len(t) for t in columns["text"]], dtype=torch.int32)
    has_mel = columns["mel"][0] is not None
    mel_lens = torch.tensor([len(m) for m in columns["mel"]], dtype=torch.int32) if has_mel else None
    max_src = src_lens.max()
    max_mel = mel_lens.max() if has_mel else 1_000_000
    batch = {}
    for key, col in columns.items():
        head = col[0]
        if isinstance(head, np.ndarray):
            col, head = [torch.from_numpy(np.ascontiguousarray(x)) for x in col], torch.from_numpy(head)
        if torch.is_tensor(head):
            if key == "duration" and learn_alignment:
                extents = (int(max_mel), int(max_src))
            else:
                extents = tuple(max(x.shape[d] for x in col) for d in range(head.dim()))
            batch[key] = _padded(col, extents, pin_memory)
        elif isinstance(head, int) and not isinstance(head, bool):
            batch[key] = torch.tensor(col, dtype=torch.int32)
        else:
            batch[key] = col
    batch.update(src_lens=src_lens, max_src_len=max_src, mel_lens=mel_lens, max_mel_len=max_mel)
    return batch


# ----------------------------------------------------------------------------------------------------------------------
# length-bucketed batches: few batch geometries per epoch, so that training steps replay their launch plans (plan.py)
# ----------------------------------------------------------------------------------------------------------------------
class BucketBatch(list):
    """The item indices of one batch, with the ``(Ts_b, Tm_b)`` it is padded to and the index of its bucket."""

    def __init__(self, indices, geometry, bucket):
        super().__init__(indices)
        self.geometry, self.bucket = tuple(geometry), int(bucket)


class LengthBucketBatchSampler:
    """Batches of items of similar length, each padded to its BUCKET's geometry instead of to its own maxima.

    ``lengths``: every item's ``(text_len, mel_len)``.  The items sorted by mel length are cut into ``n_buckets``
    contiguous ranges at the quantiles (about equally many items each; neighbours that end up with one geometry are
    merged); a bucket's geometry ``(Ts_b, Tm_b)`` is the maxima over its members, rounded up to ``step``.  Every epoch a
    bucket's members are shuffled and cut into batches of ``batch_size`` -- the leftover items form one short batch, no
    item is dropped -- and the batches of all buckets are shuffled together.  An epoch therefore shows at most
    ``2 * n_buckets`` distinct ``(B, Ts_b, Tm_b)``, where random batches padded to their own maxima show nearly as many
    as there are batches.

    The order depends only on ``(seed, epoch, world)``.  With ``world > 1`` the batches are laid out in rows of
    ``world``, one batch per rank: rows are filled with full batches of ONE bucket as far as they go (the ranks of a
    row then run the same geometry), the remaining batches share rows, and the last row is completed by repeating its
    own batches (fewer than ``world`` repeats), so that every rank takes the same number of steps -- the per-bucket
    gradient exchange would deadlock otherwise.  ``skip_batches`` drops the first batches of this rank's list (a resumed
    epoch).  Iterating yields ``BucketBatch`` lists; ``geometry_of(index)`` is what ``BucketedDataset`` attaches to items.
    """

    def __init__(self, lengths, batch_size: int, n_buckets: Optional[int] = None, seed: int = 0, epoch: int = 0,
                 world: int = 1, rank: int = 0, step: int = 1, skip_batches: int = 0):
        if n_buckets is None:
            from .plan import MAX_PLANS
            n_buckets = MAX_PLANS
        if batch_size < 1 or n_buckets < 1 or step < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("LengthBucketBatchSampler: batch_size, n_buckets, step >= 1 and 0 <= rank < world")
        self.lengths = [(int(t), int(m)) for t, m in lengths]
        self.batch_size, self.n_buckets, self.step = int(batch_size), int(n_buckets), int(step)
        self.seed, self.epoch, self.world, self.rank, self.skip_batches = int(seed), int(epoch), int(world), int(rank), int(skip_batches)
        n = len(self.lengths)
        order = sorted(range(n), key=lambda i: (self.lengths[i][1], self.lengths[i][0], i))
        up = lambda v: -(-v // self.step) * self.step  # noqa: E731
        self.buckets = []   # [(geometry, [item indices])], shortest first
        for k in range(self.n_buckets):
            members = order[k * n // self.n_buckets:(k + 1) * n // self.n_buckets]
            if not members:
                continue
            geo = (up(max(self.lengths[i][0] for i in members)), up(max(self.lengths[i][1] for i in members)))
            if self.buckets and self.buckets[-1][0] == geo:
                self.buckets[-1][1].extend(members)
            else:
                self.buckets.append((geo, list(members)))
        self._geometry = [None] * n
        for geo, members in self.buckets:
            for i in members:
                self._geometry[i] = geo

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def geometry_of(self, index: int) -> tuple:
        return self._geometry[index]

    def rows(self) -> list:
        """The epoch as rows of ``world`` batches (row i, column r = rank r's i-th batch)."""
        g = torch.Generator().manual_seed(self.seed + self.epoch)
        W, rows, loose = self.world, [], []
        for b, (geo, members) in enumerate(self.buckets):
            perm = [members[j] for j in torch.randperm(len(members), generator=g).tolist()]
            batches = [BucketBatch(perm[i:i + self.batch_size], geo, b) for i in range(0, len(perm), self.batch_size)]
            full = [x for x in batches if len(x) == self.batch_size]
            whole = len(full) // W * W
            rows += [full[i:i + W] for i in range(0, whole, W)]
            loose += full[whole:] + [x for x in batches if len(x) != self.batch_size]
        tail = None
        for i in range(0, len(loose), W):
            row = loose[i:i + W]
            if len(row) < W:
                tail = row + [row[j % len(row)] for j in range(W - len(row))]   # the evening-out repeats
            else:
                rows.append(row)
        rows = [rows[j] for j in torch.randperm(len(rows), generator=g).tolist()]
        if tail is not None:
            rows.append(tail)
        return rows

    def batches(self) -> list:
        """This rank's batches of the epoch, ``skip_batches`` dropped."""
        return [row[self.rank] for row in self.rows()][self.skip_batches:]

    def __iter__(self):
        return iter(self.batches())

    def __len__(self):
        return max(len(self.rows()) - self.skip_batches, 0)

    # -- what ``fs2l train --dry-run`` prints -------------------------------------------------------------------------
    def padded_mel_rows(self) -> int:
        """Mel rows (frames, padding included) of the epoch's batches over all ranks, evening-out repeats left out."""
        seen, total = set(), 0
        for row in self.rows():
            for b in row:
                if id(b) not in seen:
                    seen.add(id(b))
                    total += len(b) * b.geometry[1]
        return total

    def describe(self) -> dict:
        real = sum(m for _, m in self.lengths)
        table = [dict(Ts=geo[0], Tm=geo[1], items=len(members), full_batches=len(members) // self.batch_size,
                      leftover_items=len(members) % self.batch_size,
                      batches_per_epoch=-(-len(members) // self.batch_size)) for geo, members in self.buckets]
        rand = random_batches(len(self.lengths), self.batch_size, self.seed + self.epoch)
        plain = sum(len(b) * max(self.lengths[i][1] for i in b) for b in rand)
        share = lambda padded: round(1.0 - real / padded, 4) if padded else 0.0  # noqa: E731
        rows = self.rows()
        return dict(n_buckets=len(self.buckets), buckets=table, batches_per_epoch_per_rank=len(rows),
                    distinct_geometries=len({(len(b),) + b.geometry for row in rows for b in row}),
                    padded_frame_share_bucketed=share(self.padded_mel_rows()),
                    padded_frame_share_unbucketed=share(plain))


def random_batches(n: int, batch_size: int, seed: int) -> list:
    """The batches ``fs2l train`` draws without bucketing on one GPU (``RandomSampler`` + ``BatchSampler``)."""
    sampler = torch.utils.data.RandomSampler(range(n), generator=torch.Generator().manual_seed(seed))
    return list(torch.utils.data.BatchSampler(sampler, batch_size, drop_last=False))


class BucketedDataset(torch.utils.data.Dataset):
    """``dataset`` with every item tagged with its bucket's geometry (``collate_bucketed`` turns the tags of a batch into
    the batch's ``bucket_geometry``): survives DataLoader workers, which only see indices."""

    def __init__(self, dataset, sampler: LengthBucketBatchSampler):
        self.dataset, self.sampler = dataset, sampler

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, index):
        item = dict(self.dataset[index])
        item["bucket_geometry"] = self.sampler.geometry_of(index) + (self.sampler.batch_size,)
        return item


def collate_bucketed(items: list[dict], learn_alignment: bool = True, pin_memory: bool = False) -> dict:
    """``collate`` -- unchanged: the batch is padded to its own maxima on the host -- plus ``bucket_geometry = (Ts_b,
    Tm_b)``: the training step pads the device batch to it (``FastSpeech2.pad_batch``, one launch) -- and
    ``bucket_leftover``: True for a bucket's short last batch, which the step runs eagerly and never records (one plan
    per bucket: the leftovers of N buckets do not compete with the N full geometries for the plan cache)."""
    batch = collate(items, learn_alignment=learn_alignment, pin_memory=pin_memory)
    geos = batch.pop("bucket_geometry")
    if any(tuple(g) != tuple(geos[0]) for g in geos):
        raise ValueError("collate_bucketed: the items of a batch belong to different buckets")
    batch["bucket_geometry"] = (int(geos[0][0]), int(geos[0][1]))
    batch["bucket_leftover"] = len(items) != int(geos[0][2])
    return batch


class DevicePrefetcher:
    """Keeps one batch ahead of the training step: the collated CPU batch is pinned and copied to the GPU on a
    side stream while the previous step computes; ``__next__`` only makes the compute stream wait for that copy's
    event.  ``prepare`` is ``FastSpeech2.prepare_batch`` (dtype conversion + placement)."""

    def __init__(self, batches: Iterable[dict], prepare, device):
        self.it: Iterator[dict] = iter(batches)
        self.prepare, self.device = prepare, torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self._next = None
        self._preload()

    @staticmethod
    def _pin(batch):
        out = {}
        for k, v in batch.items():
            out[k] = v.pin_memory() if torch.is_tensor(v) and v.dim() > 0 and not v.is_cuda else v
        return out

    def _preload(self):
        try:
            cpu = next(self.it)
        except StopIteration:
            self._next = None
            return
        with torch.cuda.stream(self.stream):
            dev = self.prepare(self._pin(cpu))
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._next = (dev, ev)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next is None:
            raise StopIteration
        dev, ev = self._next
        torch.cuda.current_stream(self.device).wait_event(ev)
        for v in dev.values():  # the compute stream owns the tensors from here on
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(torch.cuda.current_stream(self.device))
        self._preload()
        return dev


class SpecWriter:
    """``.pt`` spectrogram writer of the reference's prediction callback: ``[n_mels, frames]`` trimmed by
    ``tgt_lens``; consecutive chunks of one utterance are concatenated until ``is_last_input_chunk``."""

    def __init__(self, out_dir, output_key: str, global_step: int = 0, sampling_rate: int = 22050,
                 spec_type: str = "mel-librosa"):
        self.dir = Path(out_dir) / "synthesized_spec"
        self.dir.mkdir(parents=True, exist_ok=True)
        self.output_key, self.global_step = output_key, global_step
        self.suffix = f"spec-pred-{sampling_rate}-{spec_type}.pt"
        self._spec, self._text = torch.tensor(()), ""

    def filename(self, basename, speaker, language) -> Path:
        return self.dir / SEP.join([basename, speaker, language, f"ckpt={self.global_step}", self.suffix])

    def write(self, outputs: dict, batch: dict) -> list[Path]:
        written = []
        lens = [int(n) for n in outputs["tgt_lens"]]
        last = batch.get("is_last_input_chunk") or [True] * len(lens)
        for i, data in enumerate(outputs[self.output_key]):
            self._spec = torch.cat((self._spec, data[: lens[i]].cpu().transpose(0, 1)), -1)
            self._text += batch["raw_text"][i]
            if last[i] is None or last[i]:
                path = self.filename(truncate_basename(slugify(self._text)), batch["speaker"][i], batch["language"][i])
                torch.save(self._spec, path)
                written.append(path)
                self._spec, self._text = torch.tensor(()), ""
        return written


class PackedSpecWriter(SpecWriter):
    """``SpecWriter`` for batches that left the GPU packed (``hip.pack_spec``): same directory, file names and suffix, one
    contiguous ``[n_mels, frames]`` fp32 tensor per file.  ``write_packed`` takes a batch's packed HOST tensor, its
    offsets, the batch (for ``raw_text`` / ``speaker`` / ``language`` / ``is_last_input_chunk``) and the items' positions
    in the input.  Files are written in INPUT order whatever order the batches come in: a piece is held (as a copy of its
    own: the caller reuses the packed buffer) until every earlier position has arrived, and consecutive chunks of one
    text are concatenated along frames until ``is_last_input_chunk`` -- also when sorting by length has put the chunks
    into different batches."""

    def __init__(self, out_dir, output_key: str, global_step: int = 0, sampling_rate: int = 22050,
                 spec_type: str = "mel-librosa", n_mels: int = 80):
        super().__init__(out_dir, output_key, global_step, sampling_rate, spec_type)
        self.n_mels = int(n_mels)
        self._held, self._next, self._chunks = {}, 0, []

    def write_packed(self, packed: torch.Tensor, offsets, batch: dict, positions) -> list[Path]:
        offsets = [int(o) for o in offsets]
        last = batch.get("is_last_input_chunk") or [True] * len(positions)
        if len(offsets) != len(positions) + 1:
            raise ValueError(f"PackedSpecWriter: {len(offsets)} offsets for {len(positions)} utterances")
        for i, pos in enumerate(positions):
            lo, hi = offsets[i], offsets[i + 1]
            if hi < lo or (hi - lo) % self.n_mels or hi > packed.numel():
                raise ValueError(f"PackedSpecWriter: offsets {lo}..{hi} do not delimit a [{self.n_mels}, frames] block")
            if int(pos) in self._held or int(pos) < self._next:
                raise ValueError(f"PackedSpecWriter: position {int(pos)} delivered twice")
            spec = packed[lo:hi].reshape(self.n_mels, (hi - lo) // self.n_mels).clone()
            self._held[int(pos)] = (spec, batch["raw_text"][i], batch["speaker"][i], batch["language"][i],
                                    last[i] is None or bool(last[i]))
        written = []
        while self._next in self._held:
            spec, text, speaker, language, is_last = self._held.pop(self._next)
            self._next += 1
            self._chunks.append(spec)
            self._text += text
            if is_last:
                path = self.filename(truncate_basename(slugify(self._text)), speaker, language)
                torch.save(torch.cat(self._chunks, -1) if len(self._chunks) > 1 else self._chunks[0], path)
                written.append(path)
                self._chunks, self._text = [], ""
        return written

    def pending(self) -> int:
        """Pieces held back: positions not yet reached, plus chunks of a text whose last chunk has not arrived."""
        return len(self._held) + len(self._chunks)


class AlignmentWriter:
    """Per-token durations, pitch and energy beside the spectrograms ``PackedSpecWriter`` writes: which frames belong to
    which token -- what the reference's TextGrid / ReadAlong writers are built on (fs2/prediction_writing_callback.py:
    331-392) -- as data, one ``.pt`` file per text:

        ``OUT/synthesized_alignment/<basename>--<speaker>--<language>--ckpt=<step>--alignment.pt``

    with ``PackedSpecWriter``'s basename rule (``truncate_basename(slugify(text))``), input-order release and chunk
    concatenation.  The file is a dict of tensors, strings, ints and lists of strings (``torch.load(...,
    weights_only=True)`` reads it): ``text`` int32 [n] token ids, ``symbols`` their n strings, ``duration`` int32 [n] in
    frames, ``frames`` = ``duration.sum()`` = the frame count of the spectrogram file, ``pitch`` / ``energy`` fp32 ([n]
    for a ``"phone"``-level predictor, [frames] for a ``"frame"``-level one: ``pitch_level`` / ``energy_level``),
    ``duration_source`` -- ``"predicted"`` (free synthesis), ``"given"`` (teacher forcing on stored durations) or
    ``"aligner"`` (teacher forcing through a learned aligner: its MAS durations) -- and ``raw_text``.  No time in
    seconds: frames times the hop size over the sampling rate is the reader's business.

    ``duration`` describes the spectrogram actually written: where the model's ``max_length`` cut the output (fewer
    frames than the durations add up to), the cumulative ends are clipped to the frame count, ``d'[j] = min(cum_j, frames)
    - min(cum_{j-1}, frames)``, so trailing tokens shrink to what is left of them (possibly 0).

    ``symbols``: the model's symbol table (``TextProcessor(config.text).symbols``) or the ``TextProcessor`` itself.

    ``write_packed`` takes a batch's packed HOST buffer (fp32; int32 members are read through a view), the members'
    places in it, the batch, the items' positions in the input and every utterance's frame count; each piece is cloned
    out of the buffer (the caller reuses it).  With ``duration_files=True`` every utterance's durations also go to
    ``OUT/duration/<basename>--<speaker>--<language>--duration.pt`` under the FILELIST's basename (``batch["basename"]``), a
    1-D int64 tensor: the layout ``FeatureDataset`` loads for a ``learn_alignment: false`` model, so that a corpus aligned
    by a trained ``learn_alignment`` model can train a fixed-duration one."""

    LEVELS = ("phone", "frame")
    SOURCES = ("predicted", "given", "aligner")

    def __init__(self, out_dir, global_step: int = 0, symbols=None):
        self.out_dir = Path(out_dir)
        self.dir = self.out_dir / "synthesized_alignment"
        self.duration_dir = self.out_dir / "duration"
        self.dir.mkdir(parents=True, exist_ok=True)
        self.global_step = int(global_step)
        table = getattr(symbols, "symbols", symbols)
        if table is None:
            raise ValueError("AlignmentWriter: the model's symbol table is required (TextProcessor(config.text).symbols)")
        self.symbols = list(table)
        self.duration_files = []
        self._held, self._next, self._chunks = {}, 0, []

    def filename(self, basename, speaker, language) -> Path:
        return self.dir / SEP.join([basename, speaker, language, f"ckpt={self.global_step}", "alignment.pt"])

    def duration_filename(self, basename, speaker, language) -> Path:
        return feature_path(self.out_dir, "duration", basename, speaker, language, "duration.pt")

    @staticmethod
    def clip(duration: torch.Tensor, frames: int) -> torch.Tensor:
        """``duration`` [n] with its cumulative ends clipped to ``frames`` (see the class): sums to ``frames``."""
        cum = duration.to(torch.int64).cumsum(0).clamp(max=int(frames))
        return torch.diff(cum, prepend=cum.new_zeros(1)).to(torch.int32)

    def write_packed(self, packed: torch.Tensor, members: dict, batch: dict, positions, frames,
                     duration_source: str = "predicted", duration_files: bool = False) -> list[Path]:
        """``members``: ``{"duration" | "pitch" | "energy": (start, offsets, level)}`` -- the member's first element in
        ``packed``, its B + 1 element offsets from there (``hip.pack_rows``'s), and ``"phone"`` / ``"frame"``.
        ``frames``: every utterance's frame count in the written spectrogram (``tgt_lens``)."""
        if duration_source not in self.SOURCES:
            raise ValueError(f"AlignmentWriter: duration_source must be one of {self.SOURCES}, got {duration_source!r}")
        if sorted(members) != ["duration", "energy", "pitch"]:
            raise ValueError(f"AlignmentWriter: members must be duration, pitch and energy, got {sorted(members)}")
        B = len(positions)
        frames = [int(f) for f in frames]
        if len(frames) != B:
            raise ValueError(f"AlignmentWriter: {len(frames)} frame counts for {B} utterances")
        table = {}
        for name, (start, offsets, level) in members.items():
            offsets = [int(o) for o in offsets]
            if level not in self.LEVELS or (name == "duration" and level != "phone"):
                raise ValueError(f"AlignmentWriter: {name} cannot be at level {level!r}")
            if len(offsets) != B + 1:
                raise ValueError(f"AlignmentWriter: {len(offsets)} {name} offsets for {B} utterances")
            if offsets[0] != 0 or any(b < a for a, b in zip(offsets, offsets[1:])) or start < 0 \
                    or start + offsets[-1] > packed.numel():
                raise ValueError(f"AlignmentWriter: the {name} offsets {offsets} from element {start} do not delimit rows "
                                 f"of a buffer of {packed.numel()} elements")
            table[name] = (int(start), offsets, level)
        last = batch.get("is_last_input_chunk") or [True] * B
        ints = packed.view(torch.int32)
        written_durations = []
        for i, pos in enumerate(positions):
            pos = int(pos)
            if pos in self._held or pos < self._next:
                raise ValueError(f"AlignmentWriter: position {pos} delivered twice")
            start, off, _ = table["duration"]
            dur = ints[start + off[i]:start + off[i + 1]].clone()
            n = dur.numel()
            total = int(dur.sum())
            if frames[i] > total or frames[i] < 0:
                raise ValueError(f"AlignmentWriter: utterance {pos} has {frames[i]} frames but durations that add up to {total}")
            piece = {"duration": self.clip(dur, frames[i]) if total != frames[i] else dur, "frames": frames[i]}
            for name in ("pitch", "energy"):
                start, off, level = table[name]
                want = n if level == "phone" else frames[i]
                if off[i + 1] - off[i] != want:
                    raise ValueError(f"AlignmentWriter: utterance {pos}: {off[i + 1] - off[i]} {name} values at the {level} "
                                     f"level, where it has {n} tokens and {frames[i]} frames")
                piece[name] = packed[start + off[i]:start + off[i + 1]].clone()
                piece[name + "_level"] = level
            text = torch.as_tensor(batch["text"][i]).reshape(-1)
            if text.numel() < n:
                raise ValueError(f"AlignmentWriter: utterance {pos} has {n} durations for {text.numel()} tokens")
            piece["text"] = text[:n].to(torch.int32).clone()
            piece["raw_text"], piece["duration_source"] = batch["raw_text"][i], duration_source
            speaker, language = batch["speaker"][i], batch["language"][i]
            if duration_files:
                path = self.duration_filename(batch["basename"][i], speaker, language)
                path.parent.mkdir(parents=True, exist_ok=True)
                torch.save(piece["duration"].to(torch.int64), path)
                written_durations.append(path)
            self._held[pos] = (piece, speaker, language, last[i] is None or bool(last[i]))
        self.duration_files.extend(written_durations)
        written = []
        while self._next in self._held:
            piece, speaker, language, is_last = self._held.pop(self._next)
            self._next += 1
            self._chunks.append(piece)
            if is_last:
                written.append(self._save(self._chunks, speaker, language))
                self._chunks = []
        return written

    def _save(self, chunks, speaker, language) -> Path:
        first = chunks[0]
        for c in chunks[1:]:
            for k in ("pitch_level", "energy_level", "duration_source"):
                if c[k] != first[k]:
                    raise ValueError(f"AlignmentWriter: the chunks of one text disagree on {k}: {first[k]!r}, {c[k]!r}")
        cat = lambda k: torch.cat([c[k] for c in chunks]) if len(chunks) > 1 else first[k]  # noqa: E731
        raw_text = "".join(c["raw_text"] for c in chunks)
        text = cat("text")
        symbols = [self.symbols[i] for i in text.tolist()]
        record = {"text": text, "symbols": symbols, "duration": cat("duration"), "frames": sum(c["frames"] for c in chunks),
                  "pitch": cat("pitch"), "energy": cat("energy"), "pitch_level": first["pitch_level"],
                  "energy_level": first["energy_level"], "duration_source": first["duration_source"], "raw_text": raw_text}
        path = self.filename(truncate_basename(slugify(raw_text)), speaker, language)
        torch.save(record, path)
        return path

    def pending(self) -> int:
        """Pieces held back: positions not yet reached, plus chunks of a text whose last chunk has not arrived."""
        return len(self._held) + len(self._chunks)


def coverage_scores(token_lists) -> list[dict]:
    """The two coverage scores the reference attaches to every row when it scores a corpus (fs2/cli/synthesize.py:389-409,
    there with nltk's ``ngrams``): ``[{"phone_coverage_score": x, "trigram_coverage_score": y}]``, one per entry.

    Counts are taken over the whole list: how often every token occurs, and how often every trigram of consecutive
    tokens occurs in the entries framed by ``<BOS>`` and ``<EOS>``.  An entry's phone coverage is the sum of 1 / count over
    its tokens; its trigram coverage is the sum of 1 / count over its trigrams WITHOUT the boundary symbols -- the
    reference scores it that way -- so an entry of fewer than three tokens gets 0.  Rare tokens and rare contexts weigh
    more: among utterances with the same loss the file lists the least informative first.

    ``token_lists``: one sequence of hashable tokens per entry -- the ids in ``SynthesisDataset.tokens``.  Symbols the
    model's table does not hold have already been dropped there (``TextProcessor`` drops them), so they count neither as
    tokens nor inside a trigram, where the reference counts the filelist's token column as it stands."""
    from collections import Counter
    lists = [[t.item() if hasattr(t, "item") else t for t in tokens] for tokens in token_lists]
    token_counter, trigram_counter = Counter(), Counter()
    for tokens in lists:
        token_counter.update(tokens)
        framed = ["<BOS>"] + tokens + ["<EOS>"]
        trigram_counter.update(zip(framed, framed[1:], framed[2:]))
    return [{"phone_coverage_score": sum(1 / token_counter[t] for t in tokens),
             "trigram_coverage_score": sum(1 / trigram_counter[n] for n in zip(tokens, tokens[1:], tokens[2:]))}
            for tokens in lists]


class ScoreWriter:
    """The score file of the reference's ``ScorerCallback`` (fs2/prediction_writing_callback.py:138-211):
    ``<output_dir>/scores-<global_step>.psv``, '|'-separated, one row per dataset entry, worst first -- sorted by
    ``(-total, trigram_coverage_score)``, entries that tie staying in input order.  ``add`` collects a record (in any
    order: ``position`` is the entry's place in the input); ``close`` sorts, writes and returns the path.  A loss term
    the model does not have (``attn_ctc`` without the learned aligner) is an empty field."""

    FIELDS = ("basename", "speaker", "language", "total", "trigram_coverage_score", "duration", "spec", "postnet",
              "attn_ctc", "attn_bin", "raw_text", "phone_coverage_score")

    def __init__(self, output_dir, global_step: int = 0):
        self.dir, self.global_step = Path(output_dir), int(global_step)
        self.records = {}

    @property
    def path(self) -> Path:
        return self.dir / f"scores-{self.global_step}.psv"

    def add(self, position: int, record: dict):
        """``record``: basename, speaker, language, raw_text, the two coverage scores, ``total`` and the loss terms that are
        present (floats); keys that are not columns of the file (``pitch``, ``energy``) are kept but not written."""
        position = int(position)
        if position in self.records:
            raise ValueError(f"ScoreWriter: position {position} delivered twice")
        missing = [k for k in ("basename", "total", "trigram_coverage_score") if k not in record]
        if missing:
            raise ValueError(f"ScoreWriter: the record of position {position} lacks {missing}")
        self.records[position] = dict(record)

    def sorted_records(self) -> list[dict]:
        rows = [self.records[p] for p in sorted(self.records)]
        rows.sort(key=lambda r: (-r["total"], r["trigram_coverage_score"]))
        return rows

    def close(self) -> Path:
        import csv
        self.dir.mkdir(parents=True, exist_ok=True)
        with open(self.path, "w", encoding="utf8", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(self.FIELDS), delimiter="|", restval="", extrasaction="ignore",
                               lineterminator="\n")
            w.writeheader()
            for r in self.sorted_records():
                w.writerow({k: (repr(float(v)) if isinstance(v, (int, float)) and not isinstance(v, bool) else v)
                            for k, v in r.items() if v is not None})
        return self.path


class DtwWriter:
    """``<output_dir>/dtw-<global_step>.psv``: how far free synthesis is from the recording, one '|'-separated row per
    dataset entry, worst first.  ``total`` and ``steps`` are what ``FastSpeech2.mel_dtw`` gives for the entry (the
    accumulated frame distance along the cheapest warping path and the cells on it), ``mel_dtw = total / steps`` the
    mean distance per aligned frame pair, ``frames`` / ``ref_frames`` the synthesized and recorded lengths and
    ``frame_ratio`` their quotient.  ``mel_dtw`` and ``frame_ratio`` are empty fields when ``steps`` or ``ref_frames`` is 0.
    Rows are sorted by ``-mel_dtw``, rows without one last, ties in input order.  ``add`` collects a record in any order
    (``position``: the entry's place in the input); ``close`` sorts, writes and returns the path.

    ``cepstra=K`` (``fs2l synthesize --compare-to DIR --cepstra K``): the file gains the columns ``cep_dtw``, ``cep_total`` and
    ``cep_steps`` behind ``steps`` -- ``FastSpeech2.mel_dtw(..., cepstra=K)``'s distance on the cepstral coefficients 1 .. K
    along ITS cheapest path, ``cep_dtw = cep_total / cep_steps`` (empty without steps): the plain Euclidean distance on
    c1 .. cK of the model's own log-mel features (for natural-log mels, ``10 * sqrt(2) / ln(10)`` times it is the
    conventional figure in dB).  Records must then carry ``cep_total`` and ``cep_steps``.  The sort key stays ``mel_dtw``;
    without ``cepstra`` the file is what it always was (``fields`` is ``FIELDS``)."""

    FIELDS = ("basename", "speaker", "language", "mel_dtw", "total", "steps", "frames", "ref_frames", "frame_ratio", "raw_text")
    CEPSTRA_FIELDS = ("cep_dtw", "cep_total", "cep_steps")

    def __init__(self, output_dir, global_step: int = 0, cepstra=None):
        self.dir, self.global_step = Path(output_dir), int(global_step)
        self.records = {}
        self.cepstra = None if cepstra is None else int(cepstra)
        at = self.FIELDS.index("steps") + 1
        self.fields = self.FIELDS if self.cepstra is None else self.FIELDS[:at] + self.CEPSTRA_FIELDS + self.FIELDS[at:]

    @property
    def path(self) -> Path:
        return self.dir / f"dtw-{self.global_step}.psv"

    def add(self, position: int, record: dict):
        """``record``: basename, speaker, language, raw_text, ``total`` (float), ``steps``, ``frames``, ``ref_frames``
        (ints); ``mel_dtw`` and ``frame_ratio`` are derived here."""
        position = int(position)
        if position in self.records:
            raise ValueError(f"DtwWriter: position {position} delivered twice")
        need = ("basename", "total", "steps", "frames", "ref_frames") + (("cep_total", "cep_steps") if self.cepstra else ())
        missing = [k for k in need if k not in record]
        if missing:
            raise ValueError(f"DtwWriter: the record of position {position} lacks {missing}")
        rec = dict(record)
        if self.cepstra is not None:
            rec["cep_total"], rec["cep_steps"] = float(rec["cep_total"]), int(rec["cep_steps"])
            rec["cep_dtw"] = rec["cep_total"] / rec["cep_steps"] if rec["cep_steps"] > 0 else None
        for k in ("steps", "frames", "ref_frames"):
            rec[k] = int(rec[k])
        rec["total"] = float(rec["total"])
        rec["mel_dtw"] = rec["total"] / rec["steps"] if rec["steps"] > 0 else None
        rec["frame_ratio"] = rec["frames"] / rec["ref_frames"] if rec["ref_frames"] > 0 else None
        self.records[position] = rec

    def sorted_records(self) -> list[dict]:
        rows = [self.records[p] for p in sorted(self.records)]
        rows.sort(key=lambda r: (r["mel_dtw"] is None, -r["mel_dtw"] if r["mel_dtw"] is not None else 0.0))
        return rows

    def close(self) -> Path:
        import csv
        self.dir.mkdir(parents=True, exist_ok=True)
        with open(self.path, "w", encoding="utf8", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(self.fields), delimiter="|", restval="", extrasaction="ignore",
                               lineterminator="\n")
            w.writeheader()
            for r in self.sorted_records():
                w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in r.items() if v is not None})
        return self.path


class DtwPathWriter:
    """Where free synthesis is far from the recording: the warping path of ``FastSpeech2.mel_dtw_paths`` cut
    into the model's own tokens, one ``.pt`` file per dataset entry under the FILELIST's basename (as ``DtwWriter``'s rows
    are):

        ``OUT/dtw_path/<basename>--<speaker>--<language>--ckpt=<step>--dtw-path.pt``

    a dict of tensors, numbers, strings and lists of strings (``torch.load(..., weights_only=True)`` reads it):

    * per synthesized frame ``i``: ``ref_first`` / ``ref_last`` int32 [frames], the first and last recorded frame the path
      pairs it with, and ``frame_cost`` fp32 [frames], the sum of those pairs' distances (``fs2hip_dtw_path``);
    * ``frames``, ``ref_frames``, ``total``, ``steps``: as in ``dtw-<step>.psv``;
    * ``text`` int32 [n], ``symbols`` (n strings), ``duration`` int32 [n]: the durations as rendered -- through
      ``AlignmentWriter.clip`` when the model's ``max_length`` cut the output -- so they add up to ``frames``;
    * per token ``k``, which owns frames ``[s_k, e_k)`` of the cumulative durations: ``token_cells`` int64 [n] = the sum of
      ``ref_last[i] - ref_first[i] + 1`` over its frames, ``token_cost`` float64 [n] = the sum of their ``frame_cost``
      (exactly rounded, ``math.fsum``: no summation order to agree on), ``token_ref_start`` = ``ref_first[s_k]`` and
      ``token_ref_end`` = ``ref_last[e_k - 1] + 1`` (exclusive), int32 [n]: the token's boundaries in the RECORDING.  A token
      without frames has 0 cells, 0 cost, and start = end = the start of the next token that has frames
      (``ref_frames`` when there is none).  Two neighbouring tokens may share one recorded frame: when the path goes up
      across their boundary, the last frame of one and the first frame of the next are paired with the same recorded
      frame, so ``token_ref_end[k] = token_ref_start[k + 1] + 1`` and ``token_cells`` adds up to ``steps``, not to
      ``ref_frames``;
    * ``basename``, ``speaker``, ``language``, ``raw_text``.

    An entry without a path (no frames on either side: ``steps == 0``) gets empty per-frame tensors and tokens without
    cells.  What must hold for a path is checked, ``ValueError`` otherwise: ``ref_first[0] == 0``, ``ref_last[-1] ==
    ref_frames - 1``, ``ref_first[i]`` is ``ref_last[i-1]`` or ``ref_last[i-1] + 1``, ``ref_first <= ref_last``, and the
    cells add up to ``steps``.

    ``close()`` writes ``OUT/dtw-tokens-<step>.psv``, one '|'-separated row per entry: its worst token -- the largest
    ``token_cost / token_cells`` over tokens with cells (the first of equals), ``token_mel_dtw`` -- beside the entry's
    own mean ``mel_dtw = total / steps`` and their quotient ``ratio``.  Rows are sorted by ``-ratio``, entries without
    one (no path, or a mean of 0) last, ties in input order.

    ``write_packed`` takes a batch's packed HOST buffer (fp32; int32 members are read through a view) and the members'
    places in it; every piece is cloned out of the buffer (the caller reuses it)."""

    MEMBERS = ("duration", "ref_first", "ref_last", "frame_cost")
    FIELDS = ("basename", "speaker", "language", "token_index", "symbol", "token_frames", "ref_start", "ref_end",
              "token_mel_dtw", "mel_dtw", "ratio", "raw_text")

    def __init__(self, out_dir, global_step: int = 0, symbols=None):
        self.out_dir = Path(out_dir)
        self.dir = self.out_dir / "dtw_path"
        self.global_step = int(global_step)
        table = getattr(symbols, "symbols", symbols)
        if table is None:
            raise ValueError("DtwPathWriter: the model's symbol table is required (TextProcessor(config.text).symbols)")
        self.symbols = list(table)
        self.records = {}

    @property
    def path(self) -> Path:
        return self.out_dir / f"dtw-tokens-{self.global_step}.psv"

    def filename(self, basename, speaker, language) -> Path:
        return self.dir / SEP.join([basename, speaker, language, f"ckpt={self.global_step}", "dtw-path.pt"])

    @staticmethod
    def tokens(duration, ref_first, ref_last, frame_cost, ref_frames: int) -> dict:
        """The per-token values of the class docstring from one utterance's (clipped) durations and per-frame path."""
        import math
        dur = duration.to(torch.int64)
        ends = dur.cumsum(0).tolist()
        n = len(ends)
        span = (ref_last.to(torch.int64) - ref_first.to(torch.int64) + 1).cumsum(0).tolist()
        first, last, costs = ref_first.tolist(), ref_last.tolist(), frame_cost.tolist()
        cells, cost, start, end = [0] * n, [0.0] * n, [0] * n, [0] * n
        nxt = int(ref_frames)
        for k in range(n - 1, -1, -1):
            e = ends[k]
            s = ends[k - 1] if k else 0
            if e > s:
                cells[k] = span[e - 1] - (span[s - 1] if s else 0)
                cost[k] = math.fsum(costs[s:e])
                start[k], end[k] = first[s], last[e - 1] + 1
                nxt = start[k]
            else:
                start[k] = end[k] = nxt
        return {"token_cells": torch.tensor(cells, dtype=torch.int64), "token_cost": torch.tensor(cost, dtype=torch.float64),
                "token_ref_start": torch.tensor(start, dtype=torch.int32), "token_ref_end": torch.tensor(end, dtype=torch.int32)}

    @staticmethod
    def check(name, ref_first, ref_last, ref_frames: int, steps: int):
        """Raises ``ValueError`` unless the per-frame rows describe one monotone path over all ``ref_frames`` recorded
        frames with ``steps`` cells."""
        first, last = ref_first.to(torch.int64), ref_last.to(torch.int64)
        if first.numel() == 0:
            raise ValueError(f"DtwPathWriter: {name!r} has no frames, but the recursion counted {steps} cells")
        if int(first[0]) != 0 or int(last[-1]) != ref_frames - 1:
            raise ValueError(f"DtwPathWriter: the path of {name!r} runs from recorded frame {int(first[0])} to "
                             f"{int(last[-1])}, not from 0 to {ref_frames - 1}")
        if bool((first > last).any()):
            raise ValueError(f"DtwPathWriter: the path of {name!r} has a frame whose first recorded frame lies behind its last")
        step = first[1:] - last[:-1]
        if bool(((step != 0) & (step != 1)).any()):
            i = int(torch.nonzero((step != 0) & (step != 1))[0]) + 1
            raise ValueError(f"DtwPathWriter: the path of {name!r} is not connected at frame {i}: it starts at recorded frame "
                             f"{int(first[i])} where frame {i - 1} ended at {int(last[i - 1])}")
        cells = int((last - first + 1).sum())
        if cells != steps:
            raise ValueError(f"DtwPathWriter: the path of {name!r} has {cells} cells where the recursion counted {steps}")

    def write_packed(self, packed: torch.Tensor, members: dict, batch: dict, positions, frames, ref_frames, totals,
                     steps) -> list[Path]:
        """``members``: ``{"duration" | "ref_first" | "ref_last" | "frame_cost": (start, offsets)}`` -- the member's first
        element in ``packed`` and its B + 1 element offsets from there (``hip.pack_rows``'s): ``duration`` per token, the
        others per synthesized frame.  ``frames`` / ``ref_frames`` / ``totals`` / ``steps``: every utterance's frame count
        in the written spectrogram, in its recording, and its DTW total and cell count."""
        if sorted(members) != sorted(self.MEMBERS):
            raise ValueError(f"DtwPathWriter: members must be {', '.join(self.MEMBERS)}, got {sorted(members)}")
        B = len(positions)
        for what, values in (("frame counts", frames), ("recorded frame counts", ref_frames), ("totals", totals),
                             ("step counts", steps)):
            if len(values) != B:
                raise ValueError(f"DtwPathWriter: {len(values)} {what} for {B} utterances")
        table = {}
        for name, (start, offsets) in members.items():
            offsets = [int(o) for o in offsets]
            if len(offsets) != B + 1:
                raise ValueError(f"DtwPathWriter: {len(offsets)} {name} offsets for {B} utterances")
            if offsets[0] != 0 or any(b < a for a, b in zip(offsets, offsets[1:])) or start < 0 \
                    or start + offsets[-1] > packed.numel():
                raise ValueError(f"DtwPathWriter: the {name} offsets {offsets} from element {start} do not delimit rows of a "
                                 f"buffer of {packed.numel()} elements")
            table[name] = (int(start), offsets)
        ints = packed.view(torch.int32)
        written = []
        for i, pos in enumerate(positions):
            pos = int(pos)
            if pos in self.records:
                raise ValueError(f"DtwPathWriter: position {pos} delivered twice")
            name, n_frames, n_ref, n_steps = batch["basename"][i], int(frames[i]), int(ref_frames[i]), int(steps[i])

            def piece(member, source):
                start, off = table[member]
                return source[start + off[i]:start + off[i + 1]].clone()

            dur = piece("duration", ints)
            summed = int(dur.sum())
            if n_frames > summed or n_frames < 0:
                raise ValueError(f"DtwPathWriter: utterance {name!r} has {n_frames} frames but durations that add up to {summed}")
            if summed != n_frames:
                dur = AlignmentWriter.clip(dur, n_frames)
            text = torch.as_tensor(batch["text"][i]).reshape(-1)
            if text.numel() < dur.numel():
                raise ValueError(f"DtwPathWriter: utterance {name!r} has {dur.numel()} durations for {text.numel()} tokens")
            text = text[:dur.numel()].to(torch.int32).clone()
            first, last, cost = piece("ref_first", ints), piece("ref_last", ints), piece("frame_cost", packed)
            for member, t in (("ref_first", first), ("ref_last", last), ("frame_cost", cost)):
                if t.numel() != n_frames:
                    raise ValueError(f"DtwPathWriter: utterance {name!r}: {t.numel()} {member} values for {n_frames} frames")
            owned = dur
            if n_steps > 0:
                self.check(name, first, last, n_ref, n_steps)
            else:   # no frames on one side: nothing of the path is defined, and no token owns a piece of it
                first, last, cost, owned = first[:0], last[:0], cost[:0], torch.zeros_like(dur)
            tokens = self.tokens(owned, first, last, cost, n_ref)
            symbols = [self.symbols[t] for t in text.tolist()]
            speaker, language, raw_text = batch["speaker"][i], batch["language"][i], batch["raw_text"][i]
            record = {"ref_first": first, "ref_last": last, "frame_cost": cost, "frames": n_frames, "ref_frames": n_ref,
                      "total": float(totals[i]), "steps": n_steps, "text": text, "symbols": symbols, "duration": dur,
                      **tokens, "basename": name, "speaker": speaker, "language": language, "raw_text": raw_text}
            path = self.filename(name, speaker, language)
            path.parent.mkdir(parents=True, exist_ok=True)
            torch.save(record, path)
            written.append(path)
            self.records[pos] = self.worst_token(record)
        return written

    @staticmethod
    def worst_token(record: dict) -> dict:
        """The entry's row of ``dtw-tokens-<step>.psv``."""
        row = {k: record[k] for k in ("basename", "speaker", "language", "raw_text")}
        row.update(token_index=None, symbol=None, token_frames=None, ref_start=None, ref_end=None, token_mel_dtw=None,
                   ratio=None)
        row["mel_dtw"] = record["total"] / record["steps"] if record["steps"] > 0 else None
        cells, cost = record["token_cells"].tolist(), record["token_cost"].tolist()
        best = None
        for k, (n, c) in enumerate(zip(cells, cost)):
            if n > 0 and (best is None or c / n > best[0]):
                best = (c / n, k)
        if best is not None:
            k = best[1]
            row.update(token_index=k, symbol=record["symbols"][k], token_frames=int(record["duration"][k]),
                       ref_start=int(record["token_ref_start"][k]), ref_end=int(record["token_ref_end"][k]),
                       token_mel_dtw=best[0])
            if row["mel_dtw"]:
                row["ratio"] = best[0] / row["mel_dtw"]
        return row

    def sorted_records(self) -> list[dict]:
        rows = [self.records[p] for p in sorted(self.records)]
        rows.sort(key=lambda r: (r["ratio"] is None, -r["ratio"] if r["ratio"] is not None else 0.0))
        return rows

    def close(self) -> Path:
        import csv
        self.out_dir.mkdir(parents=True, exist_ok=True)
        with open(self.path, "w", encoding="utf8", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(self.FIELDS), delimiter="|", restval="", extrasaction="ignore",
                               lineterminator="\n")
            w.writeheader()
            for r in self.sorted_records():
                w.writerow({k: (repr(v) if isinstance(v, float) else v) for k, v in r.items() if v is not None})
        return self.path


# ----------------------------------------------------------------------------------------------------------------------
# synthesis: text -> inference items -> batches (reference fs2/cli/synthesize.py:136-319, fs2/dataset.py:88-224)
# ----------------------------------------------------------------------------------------------------------------------
def _check_keys(data_keys: set, model_keys: set, key: str, multi: bool):
    """In the spirit of the reference's ``validate_data_keys_with_model_keys`` (fs2/cli/synthesize.py:27-72): a speaker /
    language the model has no embedding row for ends the command with a message that names it."""
    extras = sorted(str(k) for k in data_keys - model_keys - {None})
    if not extras:
        return
    if multi:
        raise SystemExit(f"You provided {extras} which {'is not a' if len(extras) == 1 else 'are not'} {key}"
                         f"{'' if len(extras) == 1 else 's'} supported by the model {sorted(model_keys)}.")
    raise SystemExit(f"The current model doesn't support multiple {key}s but your data has {key}s {extras}.\n"
                     f"Please retrain your model with multi{'lingual' if key == 'language' else key} set to True.")


def _filelist_rows(path, text_key: str):
    """Rows of a '|'-separated filelist whose header names the text column, else None (a plain-text file)."""
    import csv
    with open(path, encoding="utf8", newline="") as f:
        header = f.readline().rstrip("\r\n").split("|")
    if text_key not in header:
        return None
    if "basename" in header:
        from .cli import read_filelist
        return read_filelist(path)
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.DictReader(f, delimiter="|", quoting=csv.QUOTE_NONE))


def synthesis_entries(texts, filelist, language, speaker, duration_control, model,
                      text_representation: str = "characters") -> list[dict]:
    """The reference's ``prepare_data`` / ``load_data_from_filelist`` (fs2/cli/synthesize.py:136-319) without text
    chunking (the parent toolkit's ``chunk_text``): every text is one entry with ``is_last_input_chunk = True``.

    ``texts`` wins over ``filelist`` (with the reference's note on stderr).  A filelist is the preprocessor's
    '|'-separated format with a header (``basename|characters|language|speaker``; token columns are kept when present)
    or, when its first line does not name the text column, plain text with one utterance per line (blanks around a line
    and empty lines dropped).  A row without a basename gets ``truncate_basename(slugify(text))``.  ``language`` /
    ``speaker`` override the rows'; the defaults are the first keys of the model's look-up tables.  ``model`` only needs
    ``lang2id``, ``speaker2id`` and ``config.model.multilingual`` / ``multispeaker``."""
    import sys
    key = text_representation
    default_language = next(iter(model.lang2id), None)
    default_speaker = next(iter(model.speaker2id), None)
    data = []
    if texts:
        if filelist:
            print("Got arguments for both text and a filelist - this will only process the text."
                  " Please re-run without providing text if you want to run batch synthesis on the provided file.",
                  file=sys.stderr)
        for text in texts:
            data.append({"basename": truncate_basename(slugify(text)), key: text,
                         "language": language or default_language, "speaker": speaker or default_speaker})
    else:
        if filelist is None:
            raise ValueError("Filelist must be provided when texts is empty or None")
        rows = _filelist_rows(filelist, key)
        if rows is not None:
            for r in rows:
                text = r.get(key) or ""
                e = {"basename": r.get("basename") or truncate_basename(slugify(text)), key: text,
                     "language": language or r.get("language") or default_language,
                     "speaker": speaker or r.get("speaker") or default_speaker}
                for col in ("character_tokens", "phone_tokens", "style_reference"):
                    if r.get(col):
                        e[col] = r[col]
                data.append(e)
        else:
            with open(filelist, encoding="utf8") as f:
                for line in f:
                    text = line.strip()
                    if text:
                        data.append({"basename": truncate_basename(slugify(text)), key: text,
                                     "language": language or default_language, "speaker": speaker or default_speaker})
    if not data:
        raise SystemExit("Nothing to synthesize: no text was given")
    m = model.config.model
    _check_keys({d["language"] for d in data}, set(model.lang2id), "language", m.multilingual)
    _check_keys({d["speaker"] for d in data}, set(model.speaker2id), "speaker", m.multispeaker)
    for d in data:
        d["is_last_input_chunk"] = True
        d["duration_control"] = duration_control if duration_control else 1.0
    return data


def _style_mel(ref, n_mels: int, what: str) -> torch.Tensor:
    """A ``[n_mels, frames]`` mel (the preprocessor's layout; a leading axis of 1 is dropped) as ``[frames, n_mels]`` fp32."""
    ref = torch.as_tensor(ref, dtype=torch.float32)
    ref = ref.squeeze(0) if ref.dim() == 3 else ref
    if ref.dim() != 2 or ref.shape[0] != n_mels or ref.shape[1] < 1:
        raise ValueError(f"{what} must be a [n_mels = {n_mels}, frames] mel, got {list(ref.shape)}")
    return ref.transpose(0, 1).contiguous()


def style_reference_lens(items: list[dict]) -> Optional[torch.Tensor]:
    """[B] int32, every item's own style-reference frame count, when the items' references are not all one object (they are
    then zero-padded to the longest by ``collate``); None for one shared reference or none."""
    refs = [item.get("mel_style_reference") for item in items]
    if torch.is_tensor(refs[0]) and any(r is not refs[0] for r in refs):
        return torch.tensor([len(r) for r in refs], dtype=torch.int32)
    return None


def synthesis_batches(token_counts, batch_size: int, sort: bool = True) -> list[list[int]]:
    """Batch composition of ``synthesize``: item indices sorted by token count, longest first (a stable sort: equal counts
    keep their input order), cut into consecutive groups of ``batch_size``; ``sort=False``: input order."""
    if batch_size < 1:
        raise ValueError("synthesis_batches: batch_size >= 1")
    order = list(range(len(token_counts)))
    if sort:
        order.sort(key=lambda i: -int(token_counts[i]))
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


class SynthesisDataset(torch.utils.data.Dataset):
    """The inference branch of the reference's ``FastSpeechDataset.__getitem__`` (fs2/dataset.py:88-98, :109-110,
    :153-154, :192-194, :212-214): the 15 keys of ``FeatureDataset``'s items in the same order, with ``mel`` /
    ``duration`` / ``energy`` / ``pitch`` None in free synthesis, ``is_last_input_chunk`` (default True) and
    ``duration_control`` from the entry.  With ``teacher_forcing_dir`` the mel and the durations (the attention prior of
    a model that learns its alignment) are loaded from that directory exactly as ``FeatureDataset`` loads them
    (``attn_prior="computed"``: no prior file is opened, ``duration`` stays None and the model computes the prior).

    Tokens: the entry's ``character_tokens`` / ``phone_tokens`` column through ``encode_escaped_string_sequence`` when
    present, else its raw ``characters`` / ``phones`` text through ``TextProcessor.encode_text``.  There is no G2P, no
    text cleaning and no chunking here: those belong to the parent toolkit, which is not part of the reference
    repository -- so a phone model needs phones, and a ``phonological_features`` model, whose feature vectors only the
    parent toolkit computes, is refused in free synthesis (with a teacher-forcing directory ``pfs.pt`` is loaded as in
    training).  Symbols the table does not hold are dropped as ``TextProcessor`` drops them; how many is reported once
    on stderr, and an utterance left without a token is an error that names it.

    ``style_reference``: a ``[n_mels, frames]`` mel (the preprocessor's spectrogram layout), attached to every item as
    ``mel_style_reference`` ``[frames, n_mels]``; refused by a model without the GST module.  It may also be one such mel
    per entry -- a sequence in entry order, or a mapping by basename: every item then carries its own reference, and a
    batch of them carries their frame counts (``style_reference_lens``).  Entries given the same object share
    it; when all do, this is the single shared reference again.  Every text is encoded in the constructor:
    ``token_counts`` is what ``synthesis_batches`` takes.

    ``compare_dir`` (free synthesis only): every item also carries ``compare_mel`` ``[frames, n_mels]``, the entry's
    recorded mel from ``<compare_dir>/spec`` -- the file ``teacher_forcing_dir`` would load, found by the same
    ``feature_path`` rule -- for ``synthesize(..., compare=DtwWriter)``.  A missing file is an error that names the
    utterance.  The unit is the filelist row: its basename names the recording."""

    def __init__(self, entries: list[dict], config, lang2id: dict, speaker2id: dict, teacher_forcing_dir=None,
                 style_reference=None, text_processor=None, attn_prior: str = "files", compare_dir=None):
        import sys

        from .config import TargetTrainingTextRepresentationLevel as L
        from .config import TextProcessor

        self.attn_prior = _attn_prior_mode(attn_prior)
        self.entries, self.config = entries, config
        self.lang2id, self.speaker2id = lang2id, speaker2id
        self.text_processor = text_processor or TextProcessor(config.text)
        m, audio = config.model, config.preprocessing.audio
        self.teacher_forcing = teacher_forcing_dir is not None
        self.save_dir = Path(teacher_forcing_dir) if self.teacher_forcing else None
        if compare_dir is not None and self.teacher_forcing:
            raise ValueError("compare_dir cannot be combined with teacher_forcing_dir: a teacher-forced spectrogram has the "
                             "recording's own length, and the losses against it already exist (ScoreWriter)")
        self.compare_dir = Path(compare_dir) if compare_dir is not None else None
        self.sampling_rate = audio.input_sampling_rate
        self.spec_type = getattr(audio, "spec_type", "mel-librosa")
        self.chars = m.target_text_representation_level == L.characters
        self.use_pfs = m.target_text_representation_level == L.phonological_features
        if self.use_pfs and not self.teacher_forcing:
            raise ValueError("a phonological_features model needs feature vectors that only the parent toolkit computes: "
                             "free synthesis is not possible here (teacher forcing loads the stored pfs.pt)")
        self.style, self.styles = None, None
        if style_reference is not None:
            if not m.use_global_style_token_module:
                raise ValueError("a style reference needs a model trained with the global style token module "
                                 "(model.use_global_style_token_module)")
            if isinstance(style_reference, dict) or (isinstance(style_reference, (list, tuple)) and all(
                    r is None or torch.is_tensor(r) or isinstance(r, np.ndarray) for r in style_reference)):
                self.styles = self._per_entry_styles(style_reference, entries, audio.n_mels)
                if all(s is self.styles[0] for s in self.styles):
                    self.style, self.styles = self.styles[0], None   # one object for all: the shared reference's path
            else:
                self.style = _style_mel(style_reference, audio.n_mels, "style reference")
        tok_key, raw_key = ("character_tokens", "characters") if self.chars else ("phone_tokens", "phones")
        self.tokens, dropped = [], 0
        for e in entries:
            if e.get(tok_key):
                ids = self.text_processor.encode_escaped_string_sequence(e[tok_key])
                seq = e[tok_key]
                n_in = len(seq) if not isinstance(seq, str) else 1 + sum(
                    1 for i, ch in enumerate(seq) if ch == "/" and (i == 0 or seq[i - 1] != "\\"))
                dropped += n_in - len(ids)
            elif e.get(raw_key) is not None:
                ids = self.text_processor.encode_text(e[raw_key])
                dropped += len(e[raw_key]) - sum(len(self.text_processor.symbols[i]) for i in ids)
            else:
                raise ValueError(f"utterance {e.get('basename')!r} has neither {tok_key!r} nor {raw_key!r}: the model reads "
                                 f"{raw_key} (turning characters into phones is the parent toolkit's G2P)")
            if not ids:
                raise ValueError(f"utterance {e.get('basename')!r} ({e.get(raw_key, e.get(tok_key))!r}) has no symbol of the "
                                 "model's symbol table: nothing to synthesize")
            self.tokens.append(torch.IntTensor(ids))
        self.dropped = dropped
        if dropped:
            print(f"{dropped} input symbol(s) are not in the model's symbol table and were dropped", file=sys.stderr)

    _load = FeatureDataset._load

    @staticmethod
    def _per_entry_styles(refs, entries, n_mels) -> list:
        """One ``[frames, n_mels]`` reference per entry from a sequence (in entry order) or a mapping by basename.  Entries
        given the same object share one converted tensor, so "all one object" survives the conversion."""
        if isinstance(refs, dict):
            missing = [e.get("basename") for e in entries if e.get("basename") not in refs]
            if missing:
                raise ValueError(f"style references: no entry for utterance {missing[0]!r}"
                                 + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
            refs = [refs[e["basename"]] for e in entries]
        if len(refs) != len(entries):
            raise ValueError(f"style references: {len(refs)} given for {len(entries)} utterances")
        done, out = {}, []
        for e, ref in zip(entries, refs):
            if ref is None:
                raise ValueError(f"style references: utterance {e.get('basename')!r} has none (every utterance needs one "
                                 "when any has its own)")
            if id(ref) not in done:
                done[id(ref)] = _style_mel(ref, n_mels, f"style reference of utterance {e.get('basename')!r}")
            out.append(done[id(ref)])
        return out

    def __len__(self):
        return len(self.entries)

    @property
    def token_counts(self) -> list:
        return [len(t) for t in self.tokens]

    def __getitem__(self, index):
        item = self.entries[index]
        speaker, language = item.get("speaker") or "default", item.get("language") or "default"
        bn = item["basename"]
        m = self.config.model
        mel = duration = pfs = None
        if self.teacher_forcing:
            mel = self._load(bn, speaker, language, "spec", f"spec-{self.sampling_rate}-{self.spec_type}.pt").transpose(0, 1)
            if m.learn_alignment:
                if self.attn_prior == "files":
                    duration = self._load(bn, speaker, language, "attn",
                                          ("characters" if self.chars else "phones") + "-attn-prior.pt")
            else:
                try:
                    duration = self._load(bn, speaker, language, "duration", "duration.pt")
                except FileNotFoundError as e:
                    raise ValueError("model.learn_alignment = false requires text/audio alignments in "
                                     "'<teacher forcing directory>/duration' (fs2/dataset.py:144-151)") from e
            if self.use_pfs:
                pfs = self._load(bn, speaker, language, "pfs", "pfs.pt")
        last = item.get("is_last_input_chunk")
        out = {
            "mel": mel, "mel_style_reference": self.style if self.styles is None else self.styles[index],
            "duration": duration,
            "duration_control": item.get("duration_control", 1.0), "pfs": pfs, "text": self.tokens[index],
            "raw_text": item.get("characters", item.get("phones", "text")), "basename": bn,
            "speaker": speaker, "speaker_id": self.speaker2id.get(speaker, 0) if not m.multispeaker else self.speaker2id[speaker],
            "language": language, "language_id": self.lang2id.get(language, 0) if not m.multilingual else self.lang2id[language],
            "energy": None, "pitch": None,
            "is_last_input_chunk": True if last is None else bool(last),
        }
        if self.compare_dir is not None:
            path = feature_path(self.compare_dir, "spec", bn, speaker, language, f"spec-{self.sampling_rate}-{self.spec_type}.pt")
            try:
                ref = torch.load(path, weights_only=True)
            except FileNotFoundError:
                raise FileNotFoundError(f"utterance {bn!r} has no recorded mel to compare to: {path} does not exist") from None
            out["compare_mel"] = _style_mel(ref, self.config.preprocessing.audio.n_mels, f"recorded mel of utterance {bn!r}")
        return out


def slugify(text: str) -> str:
    """File-name-safe form of a text (the parent toolkit's ``everyvoice.utils.slugify``: NFKC, lower case,
    non-word characters dropped, runs of blanks / dashes collapsed)."""
    import re
    import unicodedata
    text = unicodedata.normalize("NFKC", str(text))
    text = re.sub(r"[^\w\s-]", "", text.lower())
    return re.sub(r"[-\s]+", "-", text).strip("-_")


def truncate_basename(basename: str, max_length: int = 20) -> str:
    """reference ``fs2/utils/__init__.py:8-20``: slug cut to 20 characters + 8 hex digits of the sha1 of the
    full name, so that utterances sharing a prefix do not overwrite each other."""
    import hashlib
    cleaned = slugify(basename)
    if len(cleaned) <= max_length:
        return cleaned
    return cleaned[:max_length] + "-" + hashlib.sha1(bytes(basename, encoding="UTF-8")).hexdigest()[:8]


class SynthesisValidation:
    """Options of ``validate(..., synthesis=...)`` (``fs2l train --val-synthesis [--val-cepstra K]``): ``cepstra`` = K adds the
    cepstral distance (``FastSpeech2.mel_dtw(..., cepstra=K)``), None leaves the mel distance alone."""

    def __init__(self, cepstra=None):
        self.cepstra = None if cepstra is None else int(cepstra)
        self.sums = None   # the six SYNTHESIS_SUMS of the last pass (after the ranks' exchange), for whoever wants the counts


#: what a free forward must not see: their absence is what turns teacher forcing off
_TARGET_KEYS = ("mel_lens", "mel", "duration", "pitch", "energy")
#: the sums ``synthesis_metrics`` returns, in order (all-reduced across ranks as ``validate`` reduces its loss sums)
SYNTHESIS_SUMS = ("mel_dtw_sum", "cep_dtw_sum", "scored", "empty", "frames", "ref_frames")


def free_batch(model, batch: dict) -> dict:
    """The validation ``batch`` as free inference takes it: without the targets, ``max_mel_len`` = the cap
    ``config.model.max_length``, and -- a GST model -- every utterance's own recording at its own length as its style
    (what ``fs2l synthesize -T --exact-lengths`` feeds)."""
    free = {k: v for k, v in batch.items() if k not in _TARGET_KEYS}
    free.update({k: None for k in _TARGET_KEYS})   # (a collated inference batch carries the keys as None)
    free["max_mel_len"] = int(model.config.model.max_length)
    if getattr(model, "gst", None) is not None:
        free["mel_style_reference"] = batch["mel"]
        free["style_reference_lens"] = batch["mel_lens"]
    return free


def synthesis_metrics_from_sums(sums, cepstra: bool) -> dict:
    """The validation metrics of free synthesis from the six ``SYNTHESIS_SUMS`` (float64 on the host).  A mean over no
    utterance and a ratio to no frame are reported as 0.0: ``validation/synth_scored`` says how many the mean stands for."""
    mel, cep, scored, empty, frames, ref_frames = (float(v) for v in sums)
    out = {"validation/mel_dtw": mel / scored if scored > 0 else 0.0}
    if cepstra:
        out["validation/cep_dtw"] = cep / scored if scored > 0 else 0.0
    out["validation/frame_ratio"] = frames / ref_frames if ref_frames > 0 else 0.0
    out["validation/synth_scored"] = int(scored)
    out["validation/synth_empty"] = int(empty)
    return out


def synthesis_metrics(total, steps, frames, ref_frames, cep_total=None, cep_steps=None) -> tuple:
    """``(metrics, sums)`` of free synthesis over the validation utterances, from ``FastSpeech2.mel_dtw``'s per-utterance
    results and the frame counts (sequences or arrays, one entry per utterance; float64 arithmetic on the host):

        validation/mel_dtw       mean over the utterances with ``steps > 0`` of ``total / steps``
        validation/cep_dtw       the same mean of ``cep_total / cep_steps`` (only when those are given)
        validation/frame_ratio   sum of synthesized frames / sum of recorded frames
        validation/synth_scored  utterances with ``steps > 0``
        validation/synth_empty   the others: a model that predicts no frame for an utterance gives (0, 0), which is
                                 counted, not averaged

    ``sums``: the six ``SYNTHESIS_SUMS`` the metrics are quotients of -- what ranks add up before
    ``synthesis_metrics_from_sums`` divides."""
    total = np.asarray(total, dtype=np.float64).reshape(-1)
    steps = np.asarray(steps, dtype=np.int64).reshape(-1)
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    ref_frames = np.asarray(ref_frames, dtype=np.int64).reshape(-1)
    if not (len(total) == len(steps) == len(frames) == len(ref_frames)):
        raise ValueError("synthesis_metrics: total, steps, frames and ref_frames differ in length")
    scored = steps > 0
    mel = float(np.sum(total[scored] / steps[scored])) if scored.any() else 0.0
    cep = 0.0
    if cep_total is not None:
        cep_total = np.asarray(cep_total, dtype=np.float64).reshape(-1)
        cep_steps = np.asarray(cep_steps, dtype=np.int64).reshape(-1)
        if len(cep_total) != len(total) or len(cep_steps) != len(total):
            raise ValueError("synthesis_metrics: cep_total / cep_steps differ in length from total")
        if not np.array_equal(cep_steps > 0, scored):
            raise ValueError("synthesis_metrics: the cepstral and the mel distance disagree on which utterances have a path")
        cep = float(np.sum(cep_total[scored] / cep_steps[scored])) if scored.any() else 0.0
    sums = [mel, cep, float(scored.sum()), float(len(steps) - scored.sum()), float(frames.sum()), float(ref_frames.sum())]
    return synthesis_metrics_from_sums(sums, cep_total is not None), sums


def validate(model, batches: Iterable[dict], process_group=None, synthesis=None) -> dict:
    """Mean of every loss term over the validation batches and over the ranks (what
    ``log_dict(..., sync_dist=True)`` reports and checkpoint selection monitors as ``validation/total_loss``).

    ``synthesis`` (a ``SynthesisValidation``; None: exactly the above): every batch is used twice in the one pass -- after
    the teacher-forced ``validation_step``, ``forward(free_batch(model, batch), inference=True, exact_lengths=True)`` in
    eval mode runs the model on its own durations, pitch and energy, and ``FastSpeech2.mel_dtw`` scores the result against
    the batch's recorded mel.  The per-utterance results stay in GPU memory and are read back once, after the last batch
    (the free forward's own read of the frame totals is the only other synchronisation); ``synthesis_metrics`` turns them
    into ``validation/mel_dtw``, ``validation/cep_dtw`` (with ``cepstra``), ``validation/frame_ratio``,
    ``validation/synth_scored`` and ``validation/synth_empty``, in the same dict as the losses.  No training state is
    touched: eval mode, no plan, no BatchNorm buffer, no dropout counter."""
    import torch.distributed as dist

    total, n = None, 0
    keys = None
    kept = []   # per batch: the int32 rows [total bits, steps, frames, ref_frames (, cep_total bits, cep_steps)] on the device
    for batch in batches:
        losses = model.validation_step(batch)
        keys = keys or list(losses)
        vec = torch.stack([losses[k].detach().float() for k in keys])
        total = vec if total is None else total + vec
        n += 1
        if synthesis is not None:
            kept.append(_free_synthesis_rows(model, batch, synthesis.cepstra))
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1
    synth = _synthesis_summary(model, kept, synthesis, distributed, process_group) if synthesis is not None else {}
    if total is None and not distributed:
        return {}
    if distributed:
        # a rank whose shard is empty still takes part in the exchange (with zero sums) -- and learns the keys from it
        box = [keys]
        gathered = [None] * dist.get_world_size(process_group)
        dist.all_gather_object(gathered, box[0], group=process_group)
        keys = next((k for k in gathered if k), None)
        if keys is None:
            return {}
        if total is None:
            total = torch.zeros(len(keys), device=model.device_, dtype=torch.float32)
    stat = torch.cat([total, total.new_tensor([float(n)])])
    if distributed:
        dist.all_reduce(stat, group=process_group)
    mean = (stat[:-1] / stat[-1]).cpu()
    return {**{f"validation/{k}_loss": float(v) for k, v in zip(keys, mean)}, **synth}


def _free_synthesis_rows(model, batch: dict, cepstra) -> torch.Tensor:
    """One validation batch through free inference and ``mel_dtw``: ``[4 or 6, B]`` int32 in GPU memory (fp32 rows as bit
    patterns), nothing read back beyond the forward's own frame totals."""
    was = model.training
    model.eval()
    try:
        out = model(free_batch(model, batch), inference=True, exact_lengths=True)
        res = model.mel_dtw(out, batch["mel"], batch["mel_lens"], cepstra=cepstra)
        Tm = out[model.output_key].shape[1]
        rows = [res[0].view(torch.int32), res[1], out["tgt_lens"].clamp(0, Tm).to(torch.int32),
                batch["mel_lens"].to(torch.int32)]
        if cepstra is not None:
            rows += [res[2].view(torch.int32), res[3]]
        return torch.stack(rows)
    finally:
        model.train(was)


def _synthesis_summary(model, kept: list, synthesis, distributed: bool, process_group) -> dict:
    import torch.distributed as dist
    cep = synthesis.cepstra is not None
    sums = [0.0] * len(SYNTHESIS_SUMS)
    if kept:
        host = torch.cat(kept, dim=1).cpu()   # the one read of the pass
        f32 = lambda row: host[row].view(torch.float32).double().numpy()   # noqa: E731
        _, sums = synthesis_metrics(f32(0), host[1].numpy(), host[2].numpy(), host[3].numpy(),
                                    f32(4) if cep else None, host[5].numpy() if cep else None)
    if distributed:
        box = torch.tensor(sums, device=model.device_, dtype=torch.float64)
        dist.all_reduce(box, group=process_group)
        sums = box.cpu().tolist()
    elif not kept:
        return {}
    synthesis.sums = list(sums)
    return synthesis_metrics_from_sums(sums, cep)
