"""Bulk synthesis: ``synthesize`` runs free (or teacher-forced) inference batch by batch and hands every batch's
spectrograms to a ``PackedSpecWriter`` -- what ``fs2l synthesize`` runs (reference ``fs2/cli/synthesize.py:333-462``,
whose Trainer.predict + prediction-writing callback read every utterance back on its own).

A batch leaves the GPU through one kernel and one copy: ``hip.pack_spec`` trims, transposes and packs the batch's
``[B, Tm, n_mels]`` output into one device buffer (the offsets in front of the payload), and ONE ``non_blocking``
device-to-host copy on a copy stream brings offsets and payload into pinned memory.  The copy's size is known without
asking the GPU again: free inference already reads the frame totals once per batch for the output length
(``VarianceAdaptor.host_totals``), a teacher-forced batch has ``mel_lens`` on the host.  The host waits for a batch's
copy event only after the NEXT batch's forward has been enqueued (``depth`` device / pinned buffer pairs in rotation;
``depth = 1`` is the fully synchronous form and writes identical files).

By default a file is what ``forward(inference=True)`` gives for the utterance IN THE BATCH ``data.synthesis_batches`` puts
it in: the network's padded rows are not zero and its convolutions read them into an utterance's last frames, so the
values -- and, through the duration predictor, the frame count -- follow the batch, as they do in the reference;
``sort=False`` with ``batch_size = 1`` reproduces the reference's one-by-one behaviour.  ``exact_lengths=True``
(``fs2l synthesize --exact-lengths``) removes the dependence: every file is what the utterance gives when it is synthesized
alone, whatever the batch size and the sort order (``FastSpeech2.forward(exact_lengths=True)``: the padded rows are zeroed
on the device in front of every convolution over time).  What is left is rounding: the GEMMs' tile choice follows the
row count, so two batchings agree to fp32 summation order, not bit for bit.

``scores`` (a ``data.ScoreWriter``; ``fs2l synthesize -T DIR --return-scores``) adds the reference's ``return_scores``
(fs2/prediction_writing_callback.py:138-211, there at batch size 1): after each teacher-forced forward
``FastSpeech2.utterance_losses`` writes the batch's ``[B, 8]`` table of per-utterance losses into the slot's header, behind
the offsets, so it leaves the GPU inside the copy that carries the spectrograms -- same copy stream, same single wait.
``exact_lengths`` is forced on: a score must not follow ``-b`` or the sort order.  Without a spectrogram writer (scores
only) nothing is packed and the copy is the header alone.

Style references of a GST model: one shared reference is encoded as the reference encodes it (the batch carries no
lengths); per-entry references (``SynthesisDataset(style_reference=[...])``, the filelist's ``style_reference`` column) are
padded to the batch's longest and travel with ``style_reference_lens``, so every row's style is what its own reference gives
alone (``StyleEncoder.fwd(mel, lens)``).  A teacher-forced dataset without any reference, run with exact lengths (given or
forced by scores), feeds every utterance's own target mel at its own length -- what the reference does at batch size 1.

``alignments`` (a ``data.AlignmentWriter``; ``fs2l synthesize --write-alignments``) adds what says which frames belong to
which token: ``duration_rounded`` and the pitch and energy predictions, cut to every utterance's own lengths on the device
by ONE ``hip.pack_rows`` call (two small launches) into an alignment block between the header and the spectrograms --
token-level members by ``src_lens``, frame-level ones by ``tgt_lens``, their offset tables in the header.  The block's size
comes from lengths the host already has (the collated ``src_lens``, the frame totals above), so the batch still leaves in
the one copy and is waited for once; the device's offsets are checked against the host's, as the spectrograms' are.
Without ``alignments`` not one launch, allocation or header byte changes.

``compare`` (a ``data.DtwWriter``; ``fs2l synthesize --compare-to DIR``) scores FREE synthesis against the recordings: the
dataset (``SynthesisDataset(..., compare_dir=DIR)``) attaches every entry's recorded mel, the batch's references go up
with one non-blocking copy, and ``FastSpeech2.mel_dtw`` writes every utterance's dynamic-time-warping distance to its
recording -- ``B`` totals and ``B`` step counts -- where the score table would be, at the end of the slot header (the two
never occur together: scores need teacher forcing, which fixes the lengths and makes warping pointless).  So the batch
still leaves in the one copy and is waited for once.  ``exact_lengths`` is forced on, as for scores.  The unit is the
dataset entry, i.e. the filelist row.  A ``DtwWriter(..., cepstra=K)`` (``--cepstra K``) also asks for the distance on the
cepstral coefficients 1 .. K (``mel_dtw(..., cepstra=K)``): the table grows to ``4 * B`` values, the cepstral totals and step
counts behind the others, and nothing else of the slot moves.  Without ``compare`` not one launch, allocation or header byte changes.

``paths`` (a ``data.DtwPathWriter``, only with ``compare``; ``fs2l synthesize --compare-to DIR --write-paths``) adds WHERE an
utterance is far from its recording: ``FastSpeech2.mel_dtw_paths`` also walks the warping path back, and ONE
more ``hip.pack_rows`` call cuts four members to every utterance's own lengths into a path block behind the alignment
block -- ``duration_rounded`` by ``src_lens``, and per synthesized frame the first and last recorded frame the path pairs it
with and the sum of those pairs' distances, by ``tgt_lens``.  The block follows the alignment block's rules: its own offset
tables in the header (behind the alignment block's), sizes from lengths the host already has, 16-byte alignment, the
device's offsets checked against the host's, and the batch still leaves in the one copy and is waited for once.  The DTW
totals stay where they are.  Without ``paths`` not one launch, allocation or header byte changes.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import hip as H
from .data import collate, coverage_scores, style_reference_lens, synthesis_batches
from .model import LOSS_KEYS


class _Slot:
    """One device buffer + its pinned host twin, both float32: [header | alignment block | path block | payload].  The header
    holds the batch's B + 1 int64 offsets (2 floats each, rounded up to 4 floats so that what follows starts 16-byte
    aligned), then -- when alignments are written -- one such table per member of the alignment block, then -- when warping
    paths are written -- one per member of the path block, and, when the batch is scored,
    its [B, 8] table of per-utterance losses last -- or, when the batch is compared to recordings, its B DTW totals and B
    step counts there instead.  The alignment block (only with alignments) and the path block (only with paths) each hold
    their members' packed rows back to back and are rounded up to 4 floats, so the payload starts 16-byte aligned with or
    without them."""

    def __init__(self, device):
        self.device, self.dev, self.host = device, None, None

    @staticmethod
    def table(B: int) -> int:
        return -(-2 * (B + 1) // 4) * 4

    @staticmethod
    def header(B: int, scored: bool = False, members: int = 0, compared: bool = False, cepstra: bool = False) -> int:
        return ((1 + members) * _Slot.table(B) + (_COLS * B if scored else 0)
                + (_Slot.dtw_table(B, cepstra) if compared else 0))

    @staticmethod
    def dtw_table(B: int, cepstra: bool = False) -> int:
        """B totals then B step counts (int32 bit patterns) -- with a cepstral distance, B more of each behind them --
        rounded up to 4 floats like every part of the header."""
        return -(-(4 if cepstra else 2) * B // 4) * 4

    def reserve(self, floats: int):
        if self.dev is None or self.dev.numel() < floats:
            n = max(floats, 1 << 16)
            self.dev = torch.empty(n, device=self.device, dtype=torch.float32)
            self.host = torch.empty(n, dtype=torch.float32).pin_memory()


_COLS = len(LOSS_KEYS) + 1   # columns of the score table: the loss terms and the total


def synthesize(model, dataset, batch_size: int, control=None, writer=None, sort: bool = True, depth: int = 2,
               exact_lengths: bool = False, scores=None, alignments=None, compare=None, paths=None) -> dict:
    """Synthesizes every item of ``dataset`` (``data.SynthesisDataset``) and writes the spectrograms through ``writer``
    (``data.PackedSpecWriter``), in input order.  Returns ``{"files": [paths], "utterances": n, "frames": n, "batches": n}``.
    Per batch the host reads the GPU once inside the forward pass (the frame totals; nothing for a teacher-forced batch)
    and waits once, for the copy event.  ``exact_lengths``: see the module's docstring.  ``scores`` (``data.ScoreWriter``):
    every entry's per-utterance losses and coverage scores are added to it (the caller closes it); the dataset must be
    teacher-forced, ``exact_lengths`` is forced on, and ``writer`` may be None (scores only).  ``alignments``
    (``data.AlignmentWriter``): every text's durations, pitch and energy are written through it (the result gains
    ``"alignment_files"``, and ``"duration_files"`` for a teacher-forced dataset of a model that learns its alignment);
    ``writer`` may be None here too.  ``compare`` (``data.DtwWriter``): every entry's DTW distance between its free
    synthesis and its recorded mel is added to it (the caller closes it); the dataset must carry the recordings
    (``SynthesisDataset(..., compare_dir=...)``, so it is not teacher-forced), ``exact_lengths`` is forced on, and
    ``writer`` may be None (comparison only).  ``paths`` (``data.DtwPathWriter``, only together with ``compare``): every
    entry's warping path and per-token distances are written through it (the result gains ``"path_files"``; the caller
    closes it, which writes the per-token table).  At least one of writer, scores, alignments and compare is required."""
    if depth < 1:
        raise ValueError("synthesize: depth >= 1")
    if paths is not None and compare is None:
        raise ValueError("synthesize: paths= (a DtwPathWriter) goes with compare= (a DtwWriter): the path is the one the "
                         "comparison's recursion chose")
    if writer is None and scores is None and alignments is None and compare is None:
        raise ValueError("synthesize: a PackedSpecWriter is required (or a ScoreWriter as scores=, or an AlignmentWriter as "
                         "alignments=): there is nothing to write")
    scored = scores is not None
    compared = compare is not None
    pathed = paths is not None
    cep = getattr(compare, "cepstra", None) if compared else None   # (DtwWriter(..., cepstra=K): the cepstral distance too)
    if compared:
        if getattr(dataset, "teacher_forcing", False):
            raise ValueError("synthesize: compare= scores free synthesis; a teacher-forced dataset already has the "
                             "recording's lengths, and its losses are what scores= writes")
        if getattr(dataset, "compare_dir", None) is None:
            raise ValueError("synthesize: compare= needs a dataset that carries the recorded mels "
                             "(SynthesisDataset(..., compare_dir=...))")
        exact_lengths = True
    if scored:
        if not getattr(dataset, "teacher_forcing", False):
            raise ValueError("synthesize: scores need a teacher-forced dataset (SynthesisDataset(..., teacher_forcing_dir=...)): "
                             "free inference has no targets to take a loss against")
        exact_lengths = True
        coverage = coverage_scores(dataset.tokens)
    device = model.device_
    n_mels = model.config.preprocessing.audio.n_mels
    learn_alignment = model.config.model.learn_alignment
    batches = synthesis_batches(dataset.token_counts, batch_size, sort)
    # a GST model teacher-forced with exact lengths and no style reference: every utterance's own target mel at its own
    # length is its style, as the reference takes it one utterance at a time (fs2/model.py:196-203)
    own_target_style = bool(exact_lengths and getattr(dataset, "teacher_forcing", False)
                            and getattr(model, "gst", None) is not None
                            and getattr(dataset, "style", None) is None and getattr(dataset, "styles", None) is None)
    was_training = model.training
    model.eval()
    files, frames, alignment_files, path_files = [], 0, [], []
    aligned = alignments is not None
    if aligned:
        vp = model.config.model.variance_predictors
        levels = {"duration": "phone", "pitch": vp.pitch.level.value, "energy": vp.energy.level.value}
        teacher_forced = bool(getattr(dataset, "teacher_forcing", False))
        duration_source = ("aligner" if learn_alignment else "given") if teacher_forced else "predicted"
    # [(slot, copy event, header floats, total floats, expected offsets, CPU batch, positions, keys, alignment block, recorded
    #   frame counts, path block)], oldest first
    pending = []

    def finish(job):
        nonlocal frames
        slot, event, hdr, total, expect, cpu_batch, positions, keys, block, ref_frames, pathblock = job
        event.synchronize()   # the one wait of this batch
        base = hdr
        if writer is not None:
            offsets = slot.host[:2 * len(expect)].view(torch.int64)
            if offsets.tolist() != expect:
                raise RuntimeError("synthesize: the frame counts on the GPU differ from the host's (durations that do not add "
                                   f"up to the mel lengths?): offsets {offsets.tolist()} against {expect}")
        if aligned:
            ablock, members = block
            tab = _Slot.table(len(positions))
            for k, (name, (start, want, level)) in enumerate(members.items()):
                got = slot.host[(1 + k) * tab:(1 + k) * tab + 2 * len(want)].view(torch.int64).tolist()
                if got != want:
                    raise RuntimeError(f"synthesize: the {name} lengths on the GPU differ from the host's ({level} level: "
                                       f"{'token' if level == 'phone' else 'frame'} counts that do not match the batch's?): "
                                       f"offsets {got} against {want}")
            alignment_files.extend(alignments.write_packed(
                slot.host[hdr:hdr + ablock], members, cpu_batch, positions, [n // n_mels for n in _diff(expect)],
                duration_source=duration_source, duration_files=teacher_forced and learn_alignment))
            base += ablock   # (the payload lies behind the alignment block)
        if scored:
            B = len(positions)
            table = slot.host[hdr - _COLS * B:hdr].view(B, _COLS).tolist()
            for row, pos, name, speaker, language, text in zip(table, positions, cpu_batch["basename"], cpu_batch["speaker"],
                                                               cpu_batch["language"], cpu_batch["raw_text"]):
                rec = dict(basename=name, speaker=speaker, language=language, raw_text=text, total=row[-1], **coverage[pos])
                rec.update((k, row[LOSS_KEYS.index(k)]) for k in keys)
                scores.add(pos, rec)
        if compared:
            B = len(positions)
            at = hdr - _Slot.dtw_table(B, cep is not None)
            totals = slot.host[at:at + B].tolist()
            cells = slot.host[at + B:at + 2 * B].view(torch.int32).tolist()
            if cep is not None:
                cep_totals = slot.host[at + 2 * B:at + 3 * B].tolist()
                cep_cells = slot.host[at + 3 * B:at + 4 * B].view(torch.int32).tolist()
            for k, pos in enumerate(positions):
                rec = dict(basename=cpu_batch["basename"][k], speaker=cpu_batch["speaker"][k],
                           language=cpu_batch["language"][k], raw_text=cpu_batch["raw_text"][k], total=totals[k],
                           steps=cells[k], frames=(expect[k + 1] - expect[k]) // n_mels, ref_frames=ref_frames[k])
                if cep is not None:
                    rec.update(cep_total=cep_totals[k], cep_steps=cep_cells[k])
                compare.add(pos, rec)
            if pathed:
                pblock, pmembers = pathblock
                tab = _Slot.table(B)
                for name, (k, start, want, level) in pmembers.items():
                    got = slot.host[k * tab:k * tab + 2 * len(want)].view(torch.int64).tolist()
                    if got != want:
                        raise RuntimeError(f"synthesize: the warping path's {name} lengths on the GPU differ from the host's "
                                           f"({'token' if level == 'phone' else 'frame'} counts that do not match the batch's?): "
                                           f"offsets {got} against {want}")
                path_files.extend(zip(positions, paths.write_packed(
                    slot.host[base:base + pblock], {name: (start, want) for name, (_, start, want, _) in pmembers.items()},
                    cpu_batch, positions, [n // n_mels for n in _diff(expect)], ref_frames, totals, cells)))
                base += pblock   # (the payload lies behind the path block)
        frames += expect[-1] // n_mels
        if writer is not None:
            files.extend(writer.write_packed(slot.host[base:base + total], offsets, cpu_batch, positions))

    try:
        with torch.cuda.device(device):
            main = torch.cuda.current_stream(device)
            copy_stream = torch.cuda.Stream(device=device)
            slots = [_Slot(device) for _ in range(depth)]
            for i, positions in enumerate(batches):
                cpu_batch = collate_items([dataset[j] for j in positions], learn_alignment, pin_memory=True)
                if own_target_style:
                    cpu_batch["mel_style_reference"] = cpu_batch["mel"]
                    cpu_batch["style_reference_lens"] = cpu_batch["mel_lens"]
                fwd_batch, ref_frames = cpu_batch, None
                if compared:
                    # the recordings are not the forward's business: they go up on their own, in one copy
                    fwd_batch = {k: v for k, v in cpu_batch.items() if k not in ("compare_mel", "compare_lens")}
                    ref = cpu_batch["compare_mel"].to(device, non_blocking=True)
                    ref_lens = cpu_batch["compare_lens"].to(device, non_blocking=True)
                    ref_frames = cpu_batch["compare_lens"].tolist()
                out = model(fwd_batch, _copy_control(control), inference=True, exact_lengths=exact_lengths)
                y = out[model.output_key]
                B, Tm, C = y.shape
                if cpu_batch["mel_lens"] is not None:
                    lens_host = cpu_batch["mel_lens"].clamp(0, Tm)
                else:
                    lens_host = model.variance_adaptor.host_totals.clamp(0, Tm)
                expect = [0]
                for n in lens_host.tolist():
                    expect.append(expect[-1] + int(n) * C)
                hdr = _Slot.header(B, scored, (len(levels) if aligned else 0) + (len(paths.MEMBERS) if pathed else 0), compared,
                                   cep is not None)
                total = expect[-1] if writer is not None else 0   # (scores / comparison only: the header is all that travels)
                slot = slots[i % depth]   # (its previous batch, i - depth, has been finished: see the drain below)
                ablock, worst, block = 0, 0, None
                if aligned:
                    # the alignment block's layout, from lengths the host already has: token counts from the collated
                    # batch, frame counts from ``lens_host``.  On the device every member may write up to B * T elements
                    # from its start (lengths that differ from the host's: caught in ``finish``), so that much is reserved
                    rows = {"duration": out["duration_rounded"], "pitch": out["pitch_prediction"],
                            "energy": out["energy_prediction"]}
                    counts = {"phone": cpu_batch["src_lens"].tolist(), "frame": lens_host.tolist()}
                    members = {}
                    for name, level in levels.items():
                        want = [0]
                        for n in counts[level]:
                            want.append(want[-1] + int(n))
                        members[name] = (ablock, want, level)
                        worst = max(worst, ablock + rows[name].numel())
                        ablock += want[-1]
                    ablock, worst = -(-ablock // 4) * 4, -(-worst // 4) * 4
                    block = (ablock, members)
                pblock, pworst, pathblock = 0, 0, None
                if pathed:
                    # the path block, laid out like the alignment block and behind it: sizes from the same host lengths,
                    # B * T elements reserved per member.  Its tables follow the alignment block's in the header
                    pcounts = {"phone": cpu_batch["src_lens"].tolist(), "frame": lens_host.tolist()}
                    reserve = {"phone": out["duration_rounded"].numel(), "frame": B * max(Tm, 1)}
                    pmembers = {}
                    for k, name in enumerate(paths.MEMBERS):
                        level = "phone" if name == "duration" else "frame"
                        want = [0]
                        for n in pcounts[level]:
                            want.append(want[-1] + int(n))
                        pmembers[name] = (1 + (len(levels) if aligned else 0) + k, pblock, want, level)
                        pworst = max(pworst, pblock + reserve[level])
                        pblock += want[-1]
                    pblock, pworst = -(-pblock // 4) * 4, -(-pworst // 4) * 4
                    pathblock = (pblock, pmembers)
                base = hdr + ablock + pblock
                slot.reserve(hdr + max(worst, ablock + pworst) + (B * Tm * C if writer is not None else 0))
                keys = None
                if scored:
                    _, keys = model.utterance_losses(out, cpu_batch, out=slot.dev[hdr - _COLS * B:hdr].view(B, _COLS))
                if compared:
                    at = hdr - _Slot.dtw_table(B, cep is not None)
                    vals = (2 if cep is None else 4) * B
                    if pathed:
                        path_rows = dict(zip(paths.MEMBERS, (out["duration_rounded"],) + tuple(
                            model.mel_dtw_paths(out, ref, ref_lens, out=slot.dev[at:at + vals], cepstra=cep)[2:5])))
                    else:
                        model.mel_dtw(out, ref, ref_lens, out=slot.dev[at:at + vals], cepstra=cep)
                if aligned:
                    tab = _Slot.table(B)
                    H.pack_rows([(rows[name], out["src_lens" if level == "phone" else "tgt_lens"],
                                  slot.dev[hdr + start:hdr + start + rows[name].numel()],
                                  slot.dev[(1 + k) * tab:(1 + k) * tab + 2 * (B + 1)].view(torch.int64))
                                 for k, (name, (start, _, level)) in enumerate(members.items())], B)
                if pathed:
                    tab, at = _Slot.table(B), hdr + ablock
                    H.pack_rows([(path_rows[name], out["src_lens" if level == "phone" else "tgt_lens"],
                                  slot.dev[at + start:at + start + path_rows[name].numel()],
                                  slot.dev[k * tab:k * tab + 2 * (B + 1)].view(torch.int64))
                                 for name, (k, start, _, level) in pmembers.items()], B)
                if writer is not None:
                    H.pack_spec(y, out["tgt_lens"], slot.dev[base:base + B * Tm * C], slot.dev[:2 * (B + 1)].view(torch.int64))
                packed_ev = torch.cuda.Event()
                packed_ev.record(main)
                copy_stream.wait_event(packed_ev)
                with torch.cuda.stream(copy_stream):
                    slot.host[:base + total].copy_(slot.dev[:base + total], non_blocking=True)
                    copied_ev = torch.cuda.Event()
                    copied_ev.record(copy_stream)
                slot.dev.record_stream(copy_stream)
                pending.append((slot, copied_ev, hdr, total, expect, cpu_batch, positions, keys, block, ref_frames, pathblock))
                # the next batch's forward is enqueued before this batch's copy is waited for: only what exceeds
                # depth - 1 batches in flight is finished now
                while len(pending) > depth - 1:
                    finish(pending.pop(0))
            while pending:
                finish(pending.pop(0))
    finally:
        model.train(was_training)
    if writer is not None and writer.pending():
        raise RuntimeError(f"synthesize: {writer.pending()} piece(s) were never written (a text without a last chunk?)")
    res = {"files": files, "utterances": len(dataset), "frames": frames, "batches": len(batches)}
    if aligned:
        if alignments.pending():
            raise RuntimeError(f"synthesize: {alignments.pending()} alignment piece(s) were never written (a text without a "
                               "last chunk?)")
        res["alignment_files"] = alignment_files
        if teacher_forced and learn_alignment:
            res["duration_files"] = list(alignments.duration_files)
    if pathed:
        res["path_files"] = [path for _, path in sorted(path_files)]   # (one per entry, written batch by batch: input order)
    return res


def collate_items(items: list, learn_alignment: bool, pin_memory: bool = False) -> dict:
    """``collate``'s batch of ``items``; when their style references are not all one object it also carries
    ``style_reference_lens`` (``data.style_reference_lens``: every reference's own frame count in the zero-padded
    ``mel_style_reference``), which makes ``FastSpeech2.forward`` encode every row as if it were alone.  Items of a
    dataset with ``compare_dir`` carry ``compare_mel``: ``collate`` pads those to ``[B, Tr, n_mels]`` and ``compare_lens``
    [B] int32 holds every recording's own frame count (both for ``FastSpeech2.mel_dtw``, neither for ``forward``)."""
    batch = collate(items, learn_alignment=learn_alignment, pin_memory=pin_memory)
    lens = style_reference_lens(items)
    if lens is not None:
        batch["style_reference_lens"] = lens
    if "compare_mel" in items[0]:
        # ``collate`` has padded the recordings to [B, Tr, n_mels]: their own frame counts travel beside them
        batch["compare_lens"] = torch.tensor([len(item["compare_mel"]) for item in items], dtype=torch.int32,
                                             pin_memory=pin_memory)
    return batch


def _diff(cumulative: list) -> list:
    return [b - a for a, b in zip(cumulative, cumulative[1:])]


def _copy_control(control) -> Optional[object]:
    """``forward`` writes the batch's ``duration_control`` into the control it is given: every batch gets its own."""
    return None if control is None else control.model_copy()
