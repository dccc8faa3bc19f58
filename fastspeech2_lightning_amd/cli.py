"""``fs2l train`` -- the training entry of the feature-prediction path (reference ``fs2/cli/train.py:9-41``,
``fs2/cli/cli.py:46-54``; the Trainer the reference borrows from the parent toolkit's ``train_base_command`` is a
Lightning ``Trainer(gradient_clip_val=1.0, monitor="validation/total_loss", max_epochs, max_steps, ...)``).

    fs2l train CONFIG.yaml [-c training.batch_size=8 ...] [--devices N] [--resume last.ckpt]
    fs2l synthesize CKPT [-t TEXT]... [-f FILELIST] [-o OUTPUT_DIR] ...   (``synthesize_command``, synthesis.py)

What it does, in the reference's order: load the YAML/JSON config (+ ``-c key=value`` overrides), read
``<preprocessing.save_dir>/stats.json``, build the speaker / language look-up tables from the two filelists, build the
model (``lang2id``, ``speaker2id``, ``stats``), then train: ``FeatureDataset -> DataLoader(collate, pinned) ->
DevicePrefetcher -> training_step -> [bucketed gradient exchange] -> fused clip + AdamW + Noam``, validate on
``validation/total_loss``, write ``last.ckpt`` / ``best.ckpt`` in Lightning's layout (weights under the reference's
keys, optimizer state in ``torch.optim.AdamW``'s format) and resume from one.

MI355X-first: one process per GPU (``--devices N`` starts the ranks itself before any GPU call, or run under
``torch.distributed.run``), RCCL gradient buckets overlapped with the backward pass, no host synchronisation inside
a step -- losses are copied out once every ``--log-every`` steps.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time
from pathlib import Path
from typing import Optional

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before the HIP runtime initialises: see fastspeech2_lightning_amd/hip.py

import torch

MONITOR = "validation/total_loss"  # fs2/cli/train.py:37
GRADIENT_CLIP_VAL = 1.0            # fs2/cli/train.py:38


# --------------------------------------------------------------------------------------------------------------
# configuration and file plumbing (host only: exercised by the CPU tests)
# --------------------------------------------------------------------------------------------------------------
def apply_overrides(raw: dict, overrides: list) -> dict:
    """``-c training.batch_size=8``: dotted path into the config dict, value parsed as JSON when it parses."""
    for item in overrides or []:
        if "=" not in item:
            raise SystemExit(f"-c expects key=value, got {item!r}")
        key, value = item.split("=", 1)
        try:
            value = json.loads(value)
        except json.JSONDecodeError:
            pass
        node = raw
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
            if not isinstance(node, dict):
                raise SystemExit(f"-c {key}: {p!r} is not a section")
        node[parts[-1]] = value
    return raw


def load_config(path, overrides=None):
    from .config import FastSpeech2Config, _load_json_or_yaml
    path = Path(path)
    raw = apply_overrides(_load_json_or_yaml(path), overrides)
    return FastSpeech2Config.model_validate(raw, context={"config_path": path})


def read_filelist(path) -> list:
    """The preprocessor's pipe-separated filelist with a header row (``basename|language|speaker|characters|
    character_tokens|phones|phone_tokens|...``); rows become the entry dicts ``FeatureDataset`` takes."""
    with open(path, encoding="utf8", newline="") as f:
        rows = list(csv.DictReader(f, delimiter="|", quoting=csv.QUOTE_NONE))
    if not rows or "basename" not in rows[0]:
        raise ValueError(f"{path}: not a '|'-separated filelist with a 'basename' column")
    return rows


def lookup_tables(*filelists) -> tuple:
    """(lang2id, speaker2id) over the given filelists: names sorted, ids dense (the parent toolkit's
    ``lookuptables_from_config`` builds them from the training and validation filelists)."""
    langs = sorted({r.get("language") or "default" for fl in filelists for r in fl})
    speakers = sorted({r.get("speaker") or "default" for fl in filelists for r in fl})
    return {n: i for i, n in enumerate(langs)}, {n: i for i, n in enumerate(speakers)}


def filter_entries(entries: list, config) -> list:
    """Rows that carry the text representation the model trains on (the reference's
    ``filter_dataset_based_on_target_text_representation_level``)."""
    from .config import TargetTrainingTextRepresentationLevel as L
    key = "character_tokens" if config.model.target_text_representation_level == L.characters else "phone_tokens"
    kept = [e for e in entries if e.get(key)]
    if not kept:
        raise ValueError(f"no filelist row has a {key!r} column value")
    return kept


def run_dir(config, args) -> Path:
    lg = getattr(config.training, "logger", None)
    get = (lambda k, d: (lg.get(k, d) if isinstance(lg, dict) else getattr(lg, k, d))) if lg is not None else (lambda k, d: d)
    base = Path(args.output_dir) if args.output_dir else Path(get("save_dir", "logs_and_checkpoints")) / str(get("name", "FeaturePredictionExperiment")) / str(get("version", "base"))
    return base


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="fs2l", description="MI355X-native FastSpeech2 feature-prediction path")
    sub = ap.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", help="Train your Text-to-Spec model")
    tr.add_argument("config_file", type=Path)
    tr.add_argument("-c", "--config-args", action="append", default=[], metavar="KEY=VALUE")
    tr.add_argument("-d", "--devices", default="auto", help="GPUs on this node: a count or 'auto' (all visible)")
    tr.add_argument("--precision", default="32-true", choices=["32-true", "32-split", "bf16-mixed"])
    tr.add_argument("--resume", type=Path, default=None, help="checkpoint to resume from (default: <run dir>/checkpoints/last.ckpt when present)")
    tr.add_argument("--output-dir", type=Path, default=None, help="run directory (default: training.logger.save_dir/name/version)")
    tr.add_argument("--max-steps", type=int, default=None, help="overrides training.max_steps")
    tr.add_argument("--max-epochs", type=int, default=None, help="overrides training.max_epochs")
    tr.add_argument("--val-every", type=int, default=None, help="validate every N optimizer steps (default: once per epoch)")
    tr.add_argument("--ckpt-every", type=int, default=None, help="write last.ckpt every N optimizer steps (default: once per epoch)")
    tr.add_argument("--log-every", type=int, default=50)
    tr.add_argument("--seed", type=int, default=1234)
    tr.add_argument("--tune-tiles", action="store_true",
                    help="before training: the GEMM tile tuner's in-step stage on the first training batch (the runner-up "
                         "tiles of the heaviest shapes tried inside the replayed step; ~30-60 s; -1...2 %% per step).  "
                         "Weights, optimizer state and BatchNorm buffers are restored afterwards; one rank only.  Save the "
                         "table with FS2_GEMM_TILE_CACHE=<file> to reuse it")
    tr.add_argument("--bucket-lengths", type=int, nargs="?", const=0, default=None, metavar="N",
                    help="length-bucketed training batches: utterances of similar mel length share a batch, and every batch is "
                         "padded (on the GPU) to its bucket's geometry, so that steps replay their launch plans on ragged "
                         "data.  N = number of buckets (default: the launch-plan limit FS2_PLAN_MAX).  Off by default")
    tr.add_argument("--compute-attn-prior", action="store_true",
                    help="a model that learns its alignment: open no attn/*-attn-prior.pt file and compute the attention prior on the GPU "
                         "from each batch's lengths (fs2hip_attn_prior; this project's beta-binomial definition).  Ignored when "
                         "model.learn_alignment is false")
    tr.add_argument("--style-lengths", action="store_true",
                    help="a model with the global style token module: training and validation steps compute every utterance's "
                         "style from its own mel_lens frames (padded rows zeroed in front of the style encoder's convolutions, "
                         "BatchNorm statistics over the valid positions, the GRU stopped after each utterance's own steps), so "
                         "the style does not follow the batch's or the bucket's padding (FastSpeech2.style_lengths).  Ignored "
                         "when model.use_global_style_token_module is false")
    tr.add_argument("--val-synthesis", action="store_true",
                    help="every validation also runs the model FREE on each validation batch (its own durations, pitch and energy; "
                         "exact lengths) and scores the result against the batch's recorded mel by DTW (fs2hip_frame_dist + "
                         "fs2hip_dtw): validation/mel_dtw, validation/frame_ratio, validation/synth_scored and "
                         "validation/synth_empty join the losses in metrics.jsonl.  Training steps are not touched")
    tr.add_argument("--val-cepstra", type=int, default=None, metavar="K",
                    help="with --val-synthesis: also validation/cep_dtw, the DTW distance on the cepstral coefficients 1..K of "
                         "both sides along its own cheapest path (fs2hip_cepstra; MCD-DTW's distance without the dB factor)")
    tr.add_argument("--monitor", default=MONITOR, metavar="KEY",
                    help="the validation metric that selects best.ckpt, smaller is better (default: %(default)s; also the "
                         "other validation/*_loss terms of the model, validation/mel_dtw with --val-synthesis and "
                         "validation/cep_dtw with --val-cepstra).  Resuming with another key starts best over")
    tr.add_argument("--dry-run", action="store_true", help="resolve config, filelists, look-up tables and the run directory, print the plan, touch no GPU "
                                                             "(with --bucket-lengths: also reads every item's lengths once and writes the cache "
                                                             "<run dir>/lengths.json, then prints the bucket table)")
    bm = sub.add_parser("benchmark", help="Time the forward pass on one batch of the training filelist (reference fs2/cli/benchmark.py)")
    bm.add_argument("config_file", type=Path)
    bm.add_argument("-c", "--config-args", action="append", default=[], metavar="KEY=VALUE")
    bm.add_argument("--benchmark-type", choices=["training", "inference"], default="training")
    bm.add_argument("--warmup-reps", type=int, default=10)
    bm.add_argument("--repetitions", type=int, default=300)
    bm.add_argument("--precision", default="32-true", choices=["32-true", "32-split", "bf16-mixed"])
    bm.add_argument("--compute-attn-prior", action="store_true", help="as for train: the batch carries no prior, the forward computes it")
    bm.add_argument("--style-lengths", action="store_true", help="as for train (FastSpeech2.style_lengths; the training benchmark type)")
    sy = sub.add_parser("synthesize", help="Given some text and a trained model, write predicted spectrograms (reference fs2/cli/synthesize.py)")
    sy.add_argument("model_path", type=Path, help="a trained text-to-spec checkpoint")
    sy.add_argument("-t", "--text", dest="texts", action="append", default=[], help="some text to synthesize; can be repeated")
    sy.add_argument("-f", "--filelist", type=Path, default=None,
                    help="'|'-separated filelist with a header (basename|characters|language|speaker), or plain text with one utterance per line")
    sy.add_argument("-o", "--output-dir", type=Path, default=Path("synthesis_output"))
    sy.add_argument("-l", "--language", default=None, help="language of a multilingual model (default: the first of its table)")
    sy.add_argument("-s", "--speaker", default=None, help="speaker of a multispeaker model (default: the first of its table)")
    sy.add_argument("-D", "--duration-control", type=float, default=1.0, help="multiplies the durations: lower is quicker")
    sy.add_argument("--pitch-control", type=float, default=1.0, help="multiplies the predicted pitch (InferenceControl.pitch)")
    sy.add_argument("--energy-control", type=float, default=1.0, help="multiplies the predicted energy (InferenceControl.energy)")
    sy.add_argument("-S", "--style-reference", type=Path, default=None,
                    help="a .pt file holding a [n_mels, frames] mel in the preprocessor's layout (GST models only).  A filelist's "
                         "style_reference column names one per row (relative to the filelist, or absolute) and overrides this; "
                         "rows without one take this")
    sy.add_argument("-T", "--teacher-forcing-directory", type=Path, default=None,
                    help="ADVANCED. preprocessed folder with spec and duration / attn folders to teacher-force the outputs")
    sy.add_argument("-b", "--batch-size", type=int, default=4)
    sy.add_argument("-O", "--output-type", action="append", type=_output_type, default=None,
                    help="'spec': [n_mels, frames] .pt tensors (the only format written here)")
    sy.add_argument("--text-representation", choices=["characters", "phones"], default="characters")
    sy.add_argument("--precision", default="32-true", choices=["32-true", "32-split", "bf16-mixed"])
    sy.add_argument("--no-sort", action="store_true", help="batches in input order instead of sorted by length (longest first)")
    sy.add_argument("--exact-lengths", action="store_true",
                    help="every file is what the utterance gives when it is synthesized alone, whatever -b and the sort order are "
                         "(the padded rows are zeroed on the GPU in front of every convolution over time; a few dozen small launches per batch)")
    sy.add_argument("--return-scores", action="store_true",
                    help="with -T: also write OUTPUT_DIR/scores-<step>.psv, every utterance's own losses (as if it were scored alone: "
                         "implies --exact-lengths) and coverage scores, worst first (the reference's return_scores, batched)")
    sy.add_argument("--compare-to", type=Path, default=None, metavar="DIR",
                    help="with -f: also write OUTPUT_DIR/dtw-<step>.psv, every row's dynamic-time-warping distance between its "
                         "FREE synthesis and its recorded mel DIR/spec/<basename>--... (the preprocessed folder -T would read), "
                         "mean frame distance along the warping path, worst first (fs2hip_frame_dist + fs2hip_dtw; implies "
                         "--exact-lengths).  Not with -T: teacher forcing fixes the lengths, --return-scores is its measure")
    sy.add_argument("--cepstra", type=int, default=None, metavar="K",
                    help="with --compare-to: dtw-<step>.psv gains cep_dtw, cep_total and cep_steps, the same distance on the "
                         "cepstral coefficients 1..K of both sides (orthonormal DCT-II of every frame, c0 dropped: fs2hip_cepstra) "
                         "along ITS cheapest path, as MCD-DTW takes it: the plain Euclidean distance on c1..cK of the model's own "
                         "log-mel features (natural-log mels: times 10*sqrt(2)/ln(10) for the conventional dB figure)")
    sy.add_argument("--scores-only", action="store_true",
                    help="with --return-scores or --compare-to: write the score file and no spectrograms")
    sy.add_argument("--write-paths", action="store_true",
                    help="with --compare-to: also write OUTPUT_DIR/dtw_path/<basename>--...--dtw-path.pt, every row's warping path "
                         "(per synthesized frame the recorded frames it is paired with and their distance) and what it says per "
                         "token -- cells, distance and the token's boundaries in the recording -- and OUTPUT_DIR/dtw-tokens-<step>.psv, "
                         "every row's worst token against its own mean, worst first (fs2hip_dtw_dirs + fs2hip_dtw_path; the rows "
                         "leave the GPU in the copy that carries the spectrograms)")
    sy.add_argument("--write-alignments", action="store_true",
                    help="also write OUTPUT_DIR/synthesized_alignment/*--alignment.pt: every text's tokens, per-token durations in "
                         "frames, and the pitch and energy predictions (a dict of tensors; fs2hip_pack_rows packs them into the "
                         "copy that carries the spectrograms).  With -T and a model that learns its alignment the durations are the "
                         "aligner's, and OUTPUT_DIR/duration/*--duration.pt is written for training a learn_alignment: false model")
    sy.add_argument("--compute-attn-prior", action="store_true",
                    help="with -T, " + "a model that learns its alignment: open no attn/*-attn-prior.pt file and compute the attention prior on the GPU "
                         "from each batch's lengths (fs2hip_attn_prior; this project's beta-binomial definition).  Ignored when "
                         "model.learn_alignment is false")
    sy.add_argument("--dry-run", action="store_true", help="resolve entries, batches and file names, print them as JSON, touch no GPU")
    return ap


def _output_type(value: str) -> str:
    needs = {"wav": "a vocoder (spec-to-wav model)", "textgrid": "the parent toolkit's TextGrid writer",
             "readalong-xml": "the parent toolkit's ReadAlong writer",
             "readalong-html": "a vocoder and the parent toolkit's ReadAlong writer"}
    if value == "spec":
        return value
    if value in needs:
        raise argparse.ArgumentTypeError(f"output type {value!r} needs {needs[value]}, which is not part of this project: "
                                         "only 'spec' is written (feed the .pt files to your vocoder)")
    raise argparse.ArgumentTypeError(f"unknown output type {value!r}: only 'spec' is written")


def plan(args) -> dict:
    """Everything ``train`` needs that does not involve the GPU."""
    config = load_config(args.config_file, args.config_args)
    t = config.training
    if not t.training_filelist or not t.validation_filelist:
        raise SystemExit("training.training_filelist and training.validation_filelist must be set")
    base = args.config_file.parent

    def resolve(p):
        p = Path(p)
        return p if p.is_absolute() else (base / p)

    config.preprocessing.save_dir = str(resolve(config.preprocessing.save_dir))
    train_rows = filter_entries(read_filelist(resolve(t.training_filelist)), config)
    val_rows = filter_entries(read_filelist(resolve(t.validation_filelist)), config)
    lang2id, speaker2id = lookup_tables(train_rows, val_rows)
    stats_path = Path(config.preprocessing.save_dir) / "stats.json"
    with open(stats_path, encoding="utf8") as f:
        stats = json.load(f)
    out = run_dir(config, args)
    if not out.is_absolute():
        out = base / out
    ckpt_dir = out / "checkpoints"
    resume = args.resume if args.resume else (ckpt_dir / "last.ckpt" if (ckpt_dir / "last.ckpt").exists() else None)
    return dict(config=config, stats=stats, lang2id=lang2id, speaker2id=speaker2id, train_rows=train_rows,
                val_rows=val_rows, run_dir=out, ckpt_dir=ckpt_dir, resume=resume,
                max_steps=args.max_steps if args.max_steps is not None else t.max_steps,
                max_epochs=args.max_epochs if args.max_epochs is not None else t.max_epochs)


def attn_prior_mode(args, config) -> dict:
    """``--compute-attn-prior`` resolved against the model: what the datasets are built with (``attn_prior``) and what a dry
    run reports -- with a note when the flag was given to a model that has no aligner to feed."""
    asked = bool(getattr(args, "compute_attn_prior", False))
    if asked and not config.model.learn_alignment:
        return {"attn_prior": "files", "attn_prior_note": "--compute-attn-prior ignored: model.learn_alignment is false "
                                                          "(the batch carries durations, not a prior)"}
    return {"attn_prior": "computed" if asked else "files"}


def style_lengths_mode(args, config) -> dict:
    """``--style-lengths`` resolved against the model: what ``FastSpeech2.style_lengths`` is set to and what a dry run
    reports -- with a note when the flag was given to a model without the style encoder."""
    asked = bool(getattr(args, "style_lengths", False))
    if asked and not config.model.use_global_style_token_module:
        return {"style_lengths": False, "style_lengths_note": "--style-lengths ignored: model.use_global_style_token_module "
                                                              "is false (there is no style encoder)"}
    return {"style_lengths": asked}


def check_cepstra(K, n_mels: int, flag: str) -> None:
    """``--cepstra`` / ``--val-cepstra``: 1 .. min(n_mels - 1, 64) coefficients (``fs2hip_cepstra``'s limits)."""
    from .hip import CEPSTRA_MAX_K
    top = min(int(n_mels) - 1, CEPSTRA_MAX_K)
    if K is not None and not 1 <= K <= top:
        raise SystemExit(f"{flag} {K}: expected 1 .. {top} coefficients (at most n_mels - 1 = {int(n_mels) - 1} and "
                         f"{CEPSTRA_MAX_K})")


def monitor_keys(config, val_synthesis: bool = False, val_cepstra=None) -> list:
    """The metrics ``--monitor`` may name: what this run's validation produces and smaller is better for."""
    terms = ["pitch", "energy", "duration", "spec"] + (["postnet"] if config.model.use_postnet else [])
    if config.model.learn_alignment:
        terms += ["attn_ctc", "attn_bin"]
    keys = [MONITOR] + [f"validation/{k}_loss" for k in terms]
    if val_synthesis:
        keys.append("validation/mel_dtw")
        if val_cepstra is not None:
            keys.append("validation/cep_dtw")
    return keys


def val_synthesis_mode(args, config) -> dict:
    """``--val-synthesis``, ``--val-cepstra`` and ``--monitor`` resolved against the model, refusing what cannot work before
    anything is loaded: what the trainer runs with and what a dry run reports (the first two only when asked for)."""
    from .hip import DTW_MAX_T1
    asked, K = bool(getattr(args, "val_synthesis", False)), getattr(args, "val_cepstra", None)
    monitor = getattr(args, "monitor", None) or MONITOR
    if K is not None and not asked:
        raise SystemExit("--val-cepstra goes with --val-synthesis: the cepstral distance is taken on the free synthesis")
    if asked:
        check_cepstra(K, config.preprocessing.audio.n_mels, "--val-cepstra")
        if config.model.max_length > DTW_MAX_T1:
            raise SystemExit(f"--val-synthesis: model.max_length = {config.model.max_length} exceeds the DTW kernel's "
                             f"{DTW_MAX_T1} synthesized frames (fs2hip_dtw keeps 8 bytes of LDS per row)")
    offered = monitor_keys(config, asked, K)
    if monitor not in offered:
        raise SystemExit(f"--monitor {monitor}: this run does not produce it; choose from {', '.join(offered)}"
                         + ("" if asked else " (validation/mel_dtw needs --val-synthesis, validation/cep_dtw --val-cepstra)"))
    out = {"monitor": monitor}
    if asked:
        out.update(val_synthesis=True, val_cepstra=K)
    return out


def bucket_count(args) -> Optional[int]:
    """``--bucket-lengths [N]``: None = off, otherwise the number of buckets (no value: the launch-plan limit).  More
    buckets than plans are allowed but warned about once: the limit is not raised (a plan's pool is gigabytes)."""
    n = getattr(args, "bucket_lengths", None)
    if n is None:
        return None
    from .plan import MAX_PLANS
    if n < 0:
        raise SystemExit("--bucket-lengths expects a positive bucket count")
    n = n or MAX_PLANS
    if n > MAX_PLANS and int(os.environ.get("RANK", 0)) == 0:
        print(f"warning: --bucket-lengths {n} exceeds the launch-plan limit FS2_PLAN_MAX={MAX_PLANS}: the least recently "
              "used plans will be dropped and recorded again (thrashing); use fewer buckets or raise FS2_PLAN_MAX",
              file=sys.stderr, flush=True)
    return n


def bucket_report(p: dict, args, n_buckets: int) -> dict:
    """What ``--dry-run --bucket-lengths`` adds to the plan: every bucket's geometry, item count and batches per epoch, and
    the padded share of the epoch's mel frames with and without bucketing.  Reads the lengths (cached next to the run)."""
    from .data import FeatureDataset, LengthBucketBatchSampler
    ds = FeatureDataset(p["train_rows"], p["config"], p["lang2id"], p["speaker2id"])
    lengths = ds.lengths(p["run_dir"] / "lengths.json")
    sampler = LengthBucketBatchSampler(lengths, p["config"].training.batch_size, n_buckets, seed=args.seed, epoch=0)
    return sampler.describe()


# --------------------------------------------------------------------------------------------------------------
# the loop (one rank)
# --------------------------------------------------------------------------------------------------------------
class Trainer:
    def __init__(self, args, p: dict, rank: int, world: int, local_rank: int):
        from . import hip as H
        from .config import Stats
        from .data import FeatureDataset
        from .model import FastSpeech2
        from .parallel import GradSync

        self.args, self.p, self.rank, self.world = args, p, rank, world
        self.device = torch.device("cuda", local_rank)
        torch.cuda.set_device(self.device)
        config = p["config"]
        self.global_step, self.epoch = 0, 0
        ckpt = None
        if p["resume"] is not None:
            self.model, ckpt = FastSpeech2.load_from_checkpoint(p["resume"], device=str(self.device),
                                                                precision=args.precision, return_checkpoint=True)
            self.model.config.training = config.training  # schedule / filelists / batch size are this run's
            self.model.config.preprocessing.save_dir = config.preprocessing.save_dir
        else:
            self.model = FastSpeech2(config, Stats(**p["stats"]), p["lang2id"], p["speaker2id"], device=str(self.device),
                                     seed=args.seed, precision=args.precision)
            finetune = getattr(config.training, "finetune_checkpoint", None)
            if finetune:  # weights only, fresh optimizer (Lightning: load_from_checkpoint + fit without ckpt_path)
                sd = torch.load(finetune, map_location="cpu", weights_only=False)["state_dict"]
                self.model.load_state_dict(sd)
        self.model.train()
        opts, scheds = self.model.configure_optimizers()
        self.opt, self.sched = opts[0], scheds[0]["scheduler"]
        # Trainer(gradient_clip_val=1.0): Lightning passes the value through this hook before every optimizer step;
        # here it is constant, so once (the clip is part of the fused optimizer launch)
        self.model.configure_gradient_clipping(self.opt, GRADIENT_CLIP_VAL, "norm")
        if ckpt is not None:
            self.global_step, self.epoch = self.model.restore_training_state(ckpt, self.opt)
            self.sched.last_epoch = self.opt.steps_done()  # host mirror of the device-resident schedule
            self.best = ckpt.get("fs2l_best_monitor", float("inf"))
            if ckpt.get("fs2l_monitor", MONITOR) != getattr(args, "monitor", MONITOR):
                self.best = float("inf")   # best under another metric says nothing about this one: start over
            self.batches_in_epoch = int(ckpt.get("fs2l_batches_in_epoch", 0))
        else:
            self.best, self.batches_in_epoch = float("inf"), 0
        self.sync = None
        if world > 1:
            self.sync = GradSync(self.model.store)
            self.sync.broadcast_parameters(0)
            self.model.data_parallel(self.sync, rank)
            self.opt.grad_scale = self.sync.grad_scale
        self._tiles_shared = world == 1
        self.n_buckets = bucket_count(args)
        cfg = self.model.config
        mode = val_synthesis_mode(args, cfg)
        self.monitor, self.val_synthesis = mode["monitor"], None
        if mode.get("val_synthesis"):
            from .data import SynthesisValidation
            self.val_synthesis = SynthesisValidation(cepstra=mode["val_cepstra"])
        self.model.style_lengths = style_lengths_mode(args, cfg)["style_lengths"]
        prior = attn_prior_mode(args, cfg)["attn_prior"]
        self.train_set = FeatureDataset(p["train_rows"], cfg, self.model.lang2id, self.model.speaker2id, attn_prior=prior)
        self.val_set = FeatureDataset(p["val_rows"], cfg, self.model.lang2id, self.model.speaker2id, attn_prior=prior)
        self.H = H
        self.metrics = None
        if rank == 0:
            p["ckpt_dir"].mkdir(parents=True, exist_ok=True)
            self.metrics = open(p["run_dir"] / "metrics.jsonl", "a", encoding="utf8")

    # ---- data ---------------------------------------------------------------------------------------------
    def loader(self, dataset, shuffle: bool, epoch: int, workers: int, skip_batches: int = 0):
        """Batches of one epoch in an order that depends only on (seed, epoch, world): a resumed run re-derives the
        interrupted epoch's order and drops the ``skip_batches`` it had already trained on."""
        from functools import partial

        from .data import collate
        cfg = self.model.config
        if shuffle and self.n_buckets:
            return self.bucketed_loader(dataset, epoch, workers, skip_batches)
        if self.world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(dataset, self.world, self.rank, shuffle=shuffle,
                                                                      seed=self.args.seed, drop_last=False)
            sampler.set_epoch(epoch)
        elif shuffle:
            sampler = torch.utils.data.RandomSampler(dataset, generator=torch.Generator().manual_seed(self.args.seed + epoch))
        else:
            sampler = torch.utils.data.SequentialSampler(dataset)
        batches = list(torch.utils.data.BatchSampler(sampler, cfg.training.batch_size, drop_last=False))[skip_batches:]
        return torch.utils.data.DataLoader(
            dataset, batch_sampler=batches, num_workers=workers,
            collate_fn=partial(collate, learn_alignment=cfg.model.learn_alignment, pin_memory=workers == 0))

    def bucketed_loader(self, dataset, epoch: int, workers: int, skip_batches: int = 0):
        """``--bucket-lengths``: the same promise as ``loader`` (an order that depends only on (seed, epoch, world)) with
        batches of similar length; ``collate`` pads on the host as always, the batch carries its bucket's geometry and the
        training step pads it to that on the GPU."""
        from functools import partial

        from .data import BucketedDataset, LengthBucketBatchSampler, collate_bucketed
        cfg = self.model.config
        cache = self.p["run_dir"] / "lengths.json"
        lengths = dataset.lengths(cache, write=self.rank == 0)
        sampler = LengthBucketBatchSampler(lengths, cfg.training.batch_size, self.n_buckets, seed=self.args.seed, epoch=epoch,
                                           world=self.world, rank=self.rank, skip_batches=skip_batches)
        return torch.utils.data.DataLoader(
            BucketedDataset(dataset, sampler), batch_sampler=sampler.batches(), num_workers=workers,
            collate_fn=partial(collate_bucketed, learn_alignment=cfg.model.learn_alignment, pin_memory=workers == 0))

    def batches(self, dataset, shuffle, epoch, workers, skip_batches: int = 0):
        from .data import DevicePrefetcher
        return DevicePrefetcher(self.loader(dataset, shuffle, epoch, workers, skip_batches), self.model.prepare_batch,
                                self.device)

    # ---- one step -------------------------------------------------------------------------------------------
    def step(self, batch):
        self.model.current_epoch_ = self.epoch
        with torch.no_grad():  # the native loop reads the flat gradient buffer directly: no autograd node needed
            self.model.training_step(batch)
        if self.sync:
            self.sync.wait()
        self.opt.step()
        self.sched.step()  # host arithmetic only (the kernels advance the device record themselves)
        self.global_step += 1
        self.batches_in_epoch += 1
        if not self._tiles_shared:
            # every rank sums in the same order: the GEMM tiles rank 0 tuned during its first step are adopted by all
            # (shapes first seen later are tuned per rank; their tiles only change the summation order)
            from .parallel import share_tile_table
            share_tile_table(0)
            self._tiles_shared = True

    def log(self, record: dict):
        record = dict(record, step=self.global_step, epoch=self.epoch, time=round(time.time(), 3))
        if self.metrics:
            self.metrics.write(json.dumps(record) + "\n")
            self.metrics.flush()
            print(json.dumps(record), flush=True)

    def log_train(self):
        self.model.check_bad_data()  # fs2/variance_adaptor.py:289-305, read where the host synchronises anyway
        slots = self.model._loss_slots.cpu()  # the one D2H copy per log interval
        from .model import LOSS_KEYS
        rec = {f"training/{k}_loss": float(slots[i]) for i, k in enumerate(LOSS_KEYS) if k in self.model.last_losses}
        rec["training/total_loss"] = float(slots[len(LOSS_KEYS)])
        r = self.opt.record()
        rec.update(lr=r["lr"], grad_norm=r["grad_norm"])
        rec["style_lengths"] = bool(self.model.style_lengths)
        rec.update(self.model.plans.counters())  # steps replayed from / recorded into a launch plan, or run eagerly
        self.log(rec)

    def validate(self) -> float:
        from .data import validate
        cfg = self.model.config
        if self.sync is not None:
            self.sync.broadcast_buffers(0)  # DDP broadcast_buffers: every rank evaluates with rank 0's running statistics
        if self.val_synthesis is None:
            means = validate(self.model, self.batches(self.val_set, False, 0, cfg.training.val_data_workers))
        else:
            means = validate(self.model, self.batches(self.val_set, False, 0, cfg.training.val_data_workers),
                             synthesis=self.val_synthesis)
        self.model.train()
        self.log(means)
        if self.monitor in ("validation/mel_dtw", "validation/cep_dtw") and not means.get("validation/synth_scored"):
            return float("inf")   # (a mean over no utterance is logged as 0.0: it must not win)
        return means.get(self.monitor, float("inf"))

    def save(self, name: str):
        if self.rank != 0:
            return
        ckpt = self.model.checkpoint_dict(self.global_step, self.epoch, self.opt)
        ckpt["fs2l_best_monitor"] = self.best
        if self.monitor != MONITOR:
            ckpt["fs2l_monitor"] = self.monitor   # (absent: the default -- checkpoints of runs without --monitor do not change)
        ckpt["fs2l_batches_in_epoch"] = self.batches_in_epoch
        path = self.p["ckpt_dir"] / name
        tmp = path.with_suffix(".tmp")
        torch.save(ckpt, tmp)
        os.replace(tmp, path)

    def after_step(self):
        a = self.args
        if a.log_every and self.global_step % a.log_every == 0:
            self.log_train()
        if a.val_every and self.global_step % a.val_every == 0:
            self.check_validation()
        if a.ckpt_every and self.global_step % a.ckpt_every == 0:
            self.save("last.ckpt")

    def check_validation(self):
        m = self.validate()
        if m < self.best:
            self.best = m
            self.save("best.ckpt")

    def tune_tiles(self):
        """``--tune-tiles``: ``hip.refine_tiles_in_step`` on the first training batch.  The trial steps are real steps, so
        everything they touch -- weights, gradient, Adam moments, the device step record (learning-rate schedule, dropout
        masks), BatchNorm running statistics and counters -- is snapshotted first and put back afterwards: training
        starts from exactly the state it would have started from, with a better tile table."""
        if self.world > 1:
            self.log({"tune_tiles": "skipped: one rank only"})
            return
        H, model, S = self.H, self.model, self.model.store
        loader = self.loader(self.train_set, True, self.epoch, 0, 0)
        batch = model.prepare_batch(next(iter(loader)))
        snap = [t.clone() for t in (S.flat, S.grad, S.adam_m, S.adam_v, model.step_state, S.bn_counters)]
        bufs = {k: v.clone() for k, v in S.buffers.items()}

        def step():
            with torch.no_grad():
                model.training_step(batch)
            self.opt.step()

        def settle():
            for _ in range(6):
                before = model.plans.replayed
                step()
                if model.plans.replayed > before:
                    break
            torch.cuda.synchronize()

        def eager_step():
            model.plan_enabled = False
            try:
                step()
            finally:
                model.plan_enabled = True
        t0 = time.perf_counter()
        for _ in range(2):
            step()  # (first-stage tuning of this geometry's shapes)
        ms, changed = H.refine_tiles_in_step(step, rounds=8, top=32, candidates=3, settle=settle, count_step=eager_step)
        with torch.no_grad():
            for dst, src in zip((S.flat, S.grad, S.adam_m, S.adam_v, model.step_state, S.bn_counters), snap):
                dst.copy_(src)
            for k, v in bufs.items():
                S.buffers[k].copy_(v)
        S.weights_changed()
        model.plans.clear()  # (their recorded loss / output tensors belong to the tuning steps)
        if os.environ.get("FS2_GEMM_TILE_CACHE"):
            H.save_tile_cache(os.environ["FS2_GEMM_TILE_CACHE"])
        self.log({"tune_tiles": {"changed": changed, "ms_per_step": round(ms, 3), "seconds": round(time.perf_counter() - t0, 1)}})

    def fit(self):
        if getattr(self.args, "tune_tiles", False):
            self.tune_tiles()
        p, cfg = self.p, self.model.config
        max_steps, max_epochs = p["max_steps"], p["max_epochs"]
        done = lambda: 0 <= max_steps <= self.global_step  # noqa: E731  (Lightning: max_steps = -1 means no limit)
        from .data import DevicePrefetcher
        while self.epoch < max_epochs and not done():
            loader = self.loader(self.train_set, True, self.epoch, cfg.training.train_data_workers, self.batches_in_epoch)
            epoch_batches = self.batches_in_epoch + len(loader)
            for batch in DevicePrefetcher(loader, self.model.prepare_batch, self.device):
                self.step(batch)
                self.after_step()
                if done():
                    break
            if self.batches_in_epoch >= epoch_batches:  # the epoch is complete (also when max_steps fell on its last batch)
                self.epoch += 1
                self.batches_in_epoch = 0
                if not self.args.val_every:
                    self.check_validation()
                if not self.args.ckpt_every:
                    self.save("last.ckpt")
        torch.cuda.synchronize()
        self.model.check_bad_data()
        self.save("last.ckpt")
        if self.metrics:
            self.metrics.close()
        return self.global_step


def spawn_ranks(n: int, argv: list) -> int:
    """``--devices N`` without a launcher: N child processes, one per GPU, started before this process makes any GPU
    call (it never does); never an exec of a process that has touched the GPU."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-m", "fastspeech2_lightning_amd"] + argv, env=env))
    return wait_ranks(procs)


def wait_ranks(procs: list, poll_s: float = 0.2) -> int:
    """Waits for every rank; when one exits non-zero the others -- which would sit in a rendezvous or a collective
    until the process-group timeout -- are terminated, and that rank's code is returned."""
    failed = None
    while any(p.poll() is None for p in procs):
        for r, p in enumerate(procs):
            rc = p.poll()
            if rc not in (None, 0) and failed is None:
                failed = (r, rc)
                print(f"rank {r} exited with code {rc}: stopping the other ranks", file=sys.stderr, flush=True)
                for q in procs:
                    if q.poll() is None:
                        q.terminate()
        time.sleep(poll_s)
        if failed is not None:
            deadline = time.time() + 10.0
            while any(p.poll() is None for p in procs) and time.time() < deadline:
                time.sleep(poll_s)
            for q in procs:
                if q.poll() is None:
                    q.kill()
    if failed is not None:
        return abs(failed[1]) or 1
    return max((abs(p.returncode) for p in procs), default=0)


def gather_from_ranks(procs: list, queue, n: int, timeout: float = 300.0, poll_s: float = 0.5) -> list:
    """``n`` results from a queue that ``multiprocessing`` ranks feed, watching the ranks while waiting: a rank that
    dies (non-zero exit code) fails the wait in seconds -- its siblings, which would sit in a rendezvous or a
    collective, are terminated -- instead of after the queue's whole timeout (``wait_ranks`` for ``Process`` objects)."""
    import queue as _queue
    out, deadline = [], time.time() + timeout
    while len(out) < n:
        try:
            out.append(queue.get(timeout=poll_s))
            continue
        except _queue.Empty:
            pass
        dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
        # (a rank that exited cleanly has already queued its result; Empty + every rank gone = results lost)
        gone = not dead and all(p.exitcode is not None for p in procs) and queue.empty()
        if dead or gone or time.time() > deadline:
            for p in procs:
                if p.is_alive():
                    p.terminate()
            for p in procs:
                p.join(10)
                if p.is_alive():
                    p.kill()
            why = (f"rank(s) {dead} exited with an error" if dead else
                   "every rank exited without a result" if gone else f"no result within {timeout:.0f} s")
            raise RuntimeError(f"gather_from_ranks: {why} ({len(out)} of {n} results)")
    return out


def train(args, argv) -> int:
    p = plan(args)
    mode = val_synthesis_mode(args, p["config"])
    if args.dry_run:
        n_buckets = bucket_count(args)
        print(json.dumps({
            **({"bucket_lengths": bucket_report(p, args, n_buckets)} if n_buckets else {}),
            "config": str(args.config_file), "run_dir": str(p["run_dir"]), "resume": str(p["resume"]) if p["resume"] else None,
            "train_utterances": len(p["train_rows"]), "validation_utterances": len(p["val_rows"]),
            "lang2id": p["lang2id"], "speaker2id": p["speaker2id"], "batch_size": p["config"].training.batch_size,
            "max_steps": p["max_steps"], "max_epochs": p["max_epochs"], **mode,
            "gradient_clip_val": GRADIENT_CLIP_VAL, "learn_alignment": p["config"].model.learn_alignment,
            **attn_prior_mode(args, p["config"]), **style_lengths_mode(args, p["config"]),
            "stats": sorted(p["stats"])}))
        return 0
    world = int(os.environ.get("WORLD_SIZE", 0))
    if not world:
        n = torch.cuda.device_count() if args.devices == "auto" else int(args.devices)  # (device_count does not initialise the GPU)
        if n > 1:
            return spawn_ranks(n, argv)
        world = 1
    rank, local = int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    backend = os.environ.get("FS2L_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
        else:
            dist.init_process_group(backend)
    # this rank's share of the host: intra-op threads, and a cap on the DataLoader workers the config asks for
    from .parallel import apply_host_budget
    budget = apply_host_budget(int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    t = p["config"].training
    t.train_data_workers = min(int(t.train_data_workers), budget["workers"])
    t.val_data_workers = min(int(t.val_data_workers), budget["workers"])
    trainer = Trainer(args, p, rank, world, local)
    steps = trainer.fit()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"finished": True, "global_step": steps, "epoch": trainer.epoch, "best_" + trainer.monitor: trainer.best,
                          "checkpoint": str(p["ckpt_dir"] / "last.ckpt")}), flush=True)
    return 0


def benchmark(args) -> int:
    """reference ``fs2/cli/benchmark.py:14-80``: the first ``training.batch_size`` items of the training filelist,
    collated; ``warmup_reps`` untimed forward passes, then ``repetitions`` timed ones (HIP events, one sync each);
    prints mean and standard deviation in ms.  ``training`` = teacher-forced forward (targets in the batch),
    ``inference`` = ``forward(inference=True)``."""
    import numpy as np

    from .config import Stats
    from .data import FeatureDataset, collate
    from .model import FastSpeech2

    args.output_dir = args.resume = None
    args.max_steps = args.max_epochs = None
    p = plan(args)
    config = p["config"]
    model = FastSpeech2(config, Stats(**p["stats"]), p["lang2id"], p["speaker2id"], precision=args.precision)
    model.eval()
    model.style_lengths = style_lengths_mode(args, config)["style_lengths"]
    ds = FeatureDataset(p["train_rows"], config, p["lang2id"], p["speaker2id"],
                        attn_prior=attn_prior_mode(args, config)["attn_prior"])
    n = min(config.training.batch_size, len(ds))
    batch = model.prepare_batch(collate([ds[i] for i in range(n)], learn_alignment=config.model.learn_alignment))
    inference = args.benchmark_type == "inference"
    if inference:
        batch = {k: v for k, v in batch.items() if k not in ("mel", "mel_lens", "pitch", "energy", "duration")}
        batch.update(mel=None, mel_lens=None, duration=None, max_mel_len=config.model.max_length)
    for _ in range(args.warmup_reps):
        model(batch, inference=inference)
    timings = np.zeros(args.repetitions)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.repetitions):
        start.record()
        model(batch, inference=inference)
        end.record()
        torch.cuda.synchronize()
        timings[rep] = start.elapsed_time(end)
    print(f"Average forward pass for {args.benchmark_type} duration after {args.repetitions} repetitions: "
          f"{timings.mean()} ms Standard Deviation: {timings.std()}")
    return 0


def checkpoint_tables(ckpt: dict):
    """What the data side of ``synthesize`` needs of a model, from a checkpoint's ``hyper_parameters`` alone (no GPU, no
    weights): ``config``, ``lang2id``, ``speaker2id``."""
    from types import SimpleNamespace

    from .config import FastSpeech2Config
    hp = ckpt["hyper_parameters"]
    config = hp["config"]
    if not isinstance(config, FastSpeech2Config):
        config = FastSpeech2Config(**config)
    return SimpleNamespace(config=config, lang2id=dict(hp.get("lang2id") or {}), speaker2id=dict(hp.get("speaker2id") or {}))


def synthesis_file_names(dataset, out_dir, global_step: int) -> list:
    """The files ``PackedSpecWriter`` will write for ``dataset``, in input order (one per text: chunks are joined)."""
    from .data import SEP, slugify, truncate_basename
    audio = dataset.config.preprocessing.audio
    suffix = f"spec-pred-{audio.input_sampling_rate}-{getattr(audio, 'spec_type', 'mel-librosa')}.pt"
    names, text = [], ""
    for e in dataset.entries:
        text += e.get("characters", e.get("phones", "text"))  # (``raw_text`` of the item)
        if e.get("is_last_input_chunk", True):
            names.append(str(Path(out_dir) / "synthesized_spec" / SEP.join(
                [truncate_basename(slugify(text)), e.get("speaker") or "default", e.get("language") or "default",
                 f"ckpt={global_step}", suffix])))
            text = ""
    return names


def alignment_file_names(dataset, out_dir, global_step: int) -> list:
    """The files ``AlignmentWriter`` will write for ``dataset``, in input order (one per text: chunks are joined)."""
    from .data import SEP, slugify, truncate_basename
    names, text = [], ""
    for e in dataset.entries:
        text += e.get("characters", e.get("phones", "text"))  # (``raw_text`` of the item)
        if e.get("is_last_input_chunk", True):
            names.append(str(Path(out_dir) / "synthesized_alignment" / SEP.join(
                [truncate_basename(slugify(text)), e.get("speaker") or "default", e.get("language") or "default",
                 f"ckpt={global_step}", "alignment.pt"])))
            text = ""
    return names


def duration_file_names(dataset, out_dir) -> list:
    """The ``duration/`` files ``AlignmentWriter`` writes for a teacher-forced dataset of a model that learns its alignment:
    one per entry, under the filelist's basename."""
    from .data import feature_path
    return [str(feature_path(out_dir, "duration", e["basename"], e.get("speaker") or "default",
                             e.get("language") or "default", "duration.pt")) for e in dataset.entries]


def style_references(entries: list, shared, filelist, n_mels: int) -> tuple:
    """The style references of ``fs2l synthesize``: ``-S`` (``shared``, one ``.pt`` for the run) and the filelist's
    ``style_reference`` column (one ``.pt`` per row, relative to the filelist or absolute).  A row's entry overrides ``-S``;
    rows without one take ``-S``; a row without one on a run where other rows have one and there is no ``-S`` is an error
    that names it.  Files are loaded once per path and must hold a ``[n_mels, frames]`` mel.

    Returns ``(what SynthesisDataset takes as style_reference, [every row's source])``: None / the shared mel / one mel per
    entry (rows of one path share one object), and ``"own file"`` / ``"shared file"`` / None per entry."""
    cache = {}

    def load(path, what):
        path = Path(path)
        if path.suffix != ".pt":
            raise SystemExit(f"{what} {path}: expected a .pt file holding a [n_mels, frames] mel; turning audio into a mel "
                             "needs the parent toolkit's preprocessor")
        key = str(path.resolve())
        if key not in cache:
            try:
                ref = torch.load(path, map_location="cpu", weights_only=True)
            except FileNotFoundError:
                raise SystemExit(f"{what} {path}: no such file") from None
            shape = list(ref.shape) if torch.is_tensor(ref) else type(ref).__name__
            if not torch.is_tensor(ref) or ref.dim() not in (2, 3) or (ref.dim() == 3 and ref.shape[0] != 1) \
                    or ref.shape[-2] != n_mels or ref.shape[-1] < 1:
                raise SystemExit(f"{what} {path}: expected a [n_mels = {n_mels}, frames] mel, got {shape}")
            cache[key] = ref
        return cache[key]

    own = [e.get("style_reference") for e in entries]
    if not any(own):
        if shared is None:
            return None, [None] * len(entries)
        # (one reference for the run: loaded as it is, SynthesisDataset checks it)
        return torch.load(shared, map_location="cpu", weights_only=True), ["shared file"] * len(entries)
    base = Path(filelist).parent if filelist is not None else Path(".")
    shared_ref = load(shared, "--style-reference") if shared is not None else None
    refs, sources = [], []
    for i, (e, name) in enumerate(zip(entries, own)):
        if name:
            path = Path(name)
            refs.append(load(path if path.is_absolute() else base / path,
                             f"style_reference of row {i + 1} ({e.get('basename')!r})"))
            sources.append("own file")
        elif shared_ref is not None:
            refs.append(shared_ref)
            sources.append("shared file")
        else:
            raise SystemExit(f"row {i + 1} ({e.get('basename')!r}) of {filelist} has no style_reference and there is no "
                             "--style-reference (-S) to fall back on: other rows name one")
    return refs, sources


def synthesize_command(args) -> int:
    """``fs2l synthesize`` (reference ``fs2/cli/synthesize.py:466-700``): checkpoint + text -> ``.pt`` spectrograms in
    ``OUTPUT_DIR/synthesized_spec/``, one GPU.  Argument errors come before anything expensive is loaded."""
    from .config import TargetTrainingTextRepresentationLevel as L
    if not args.texts and not args.filelist:
        print("You must define either --text or --filelist", file=sys.stderr)
        raise SystemExit(1)
    if args.style_reference is not None and args.style_reference.suffix != ".pt":
        raise SystemExit(f"--style-reference {args.style_reference}: expected a .pt file holding a [n_mels, frames] mel; turning "
                         "audio into a mel needs the parent toolkit's preprocessor")
    if args.batch_size < 1:
        raise SystemExit("--batch-size must be at least 1")
    if args.return_scores and args.teacher_forcing_directory is None:
        raise SystemExit("--return-scores needs --teacher-forcing-directory (-T): a loss is taken against the recorded mel and "
                         "durations, which free synthesis does not have")
    if args.compare_to is not None and args.teacher_forcing_directory is not None:
        raise SystemExit("--compare-to scores free synthesis, whose length differs from the recording's; with "
                         "--teacher-forcing-directory (-T) the lengths are the recording's and --return-scores gives the losses")
    if args.compare_to is not None and args.texts:
        raise SystemExit("--compare-to needs --filelist (-f): the recorded mel of a row is found by its basename, and a --text "
                         "(-t) has none")
    if args.cepstra is not None and args.compare_to is None:
        raise SystemExit("--cepstra goes with --compare-to: the cepstral distance is taken between a free synthesis and its "
                         "recording")
    if args.write_paths and args.compare_to is None:
        raise SystemExit("--write-paths goes with --compare-to: the path is the one that leads to the recording")
    if args.scores_only and not (args.return_scores or args.compare_to is not None):
        raise SystemExit("--scores-only goes with --return-scores or --compare-to")
    from .data import (AlignmentWriter, DtwPathWriter, DtwWriter, PackedSpecWriter, ScoreWriter, SynthesisDataset, coverage_scores,
                       synthesis_batches, synthesis_entries)
    print(f"Loading checkpoint from {args.model_path}", file=sys.stderr)
    if args.dry_run:
        ckpt = torch.load(args.model_path, map_location="cpu", weights_only=False)
        model = checkpoint_tables(ckpt)
    else:
        from .model import FastSpeech2
        model, ckpt = FastSpeech2.load_from_checkpoint(args.model_path, precision=args.precision, return_checkpoint=True)
    global_step = int(ckpt.get("global_step", 0))
    config = model.config
    if config.model.target_text_representation_level == L.characters and args.text_representation != "characters":
        raise ValueError(f"Your model was trained on {config.model.target_text_representation_level} but you provided "
                         f"{args.text_representation} which is incompatible.")
    entries = synthesis_entries(args.texts, args.filelist, args.language, args.speaker, args.duration_control, model,
                                args.text_representation)
    style, style_sources = style_references(entries, args.style_reference, args.filelist, config.preprocessing.audio.n_mels)
    dataset = SynthesisDataset(entries, config, model.lang2id, model.speaker2id,
                               teacher_forcing_dir=args.teacher_forcing_directory, style_reference=style,
                               attn_prior=attn_prior_mode(args, config)["attn_prior"], compare_dir=args.compare_to)
    sort = not args.no_sort
    scores = ScoreWriter(args.output_dir, global_step) if args.return_scores else None
    check_cepstra(args.cepstra, config.preprocessing.audio.n_mels, "--cepstra")
    compare = None
    if args.compare_to is not None:
        compare = (DtwWriter(args.output_dir, global_step) if args.cepstra is None
                   else DtwWriter(args.output_dir, global_step, cepstra=args.cepstra))
    if args.dry_run:
        plan = {
            "checkpoint": str(args.model_path), "global_step": global_step, "output_dir": str(args.output_dir),
            "utterances": len(dataset), "batch_size": args.batch_size, "sort": sort,
            "exact_lengths": bool(args.exact_lengths or args.return_scores or compare is not None),
            "return_scores": bool(args.return_scores), **attn_prior_mode(args, config),
            "token_counts": dataset.token_counts, "dropped_symbols": dataset.dropped,
            "batches": synthesis_batches(dataset.token_counts, args.batch_size, sort),
            "entries": [{k: e.get(k) for k in ("basename", "language", "speaker", "duration_control")} for e in entries],
            "files": [] if args.scores_only else synthesis_file_names(dataset, args.output_dir, global_step)}
        if config.model.use_global_style_token_module:
            # where every row's style comes from: style token 0, the -S file, the row's own file, or (teacher forcing
            # without a reference) the row's target mel
            plan["style_sources"] = [s or ("target" if dataset.teacher_forcing else "token") for s in style_sources]
        if scores is not None:
            plan["scores_file"] = str(scores.path)
            for e, cov in zip(plan["entries"], coverage_scores(dataset.tokens)):
                e.update(cov)
        if compare is not None:
            plan["compare_to"] = str(args.compare_to)
            plan["dtw_file"] = str(compare.path)
            if args.cepstra is not None:
                plan["cepstra"] = args.cepstra
            if args.write_paths:
                paths = DtwPathWriter(args.output_dir, global_step, dataset.text_processor.symbols)
                plan["dtw_tokens_file"] = str(paths.path)
                plan["path_files"] = [str(paths.filename(e["basename"], e.get("speaker") or "default",
                                                                e.get("language") or "default")) for e in entries]
        if args.write_alignments:
            plan["alignment_files"] = alignment_file_names(dataset, args.output_dir, global_step)
            if dataset.teacher_forcing and config.model.learn_alignment:
                plan["duration_files"] = duration_file_names(dataset, args.output_dir)
        print(json.dumps(plan))
        return 0
    from .config import InferenceControl
    from .synthesis import synthesize
    audio = config.preprocessing.audio
    writer = None
    if not args.scores_only:
        writer = PackedSpecWriter(args.output_dir, model.output_key, global_step, audio.input_sampling_rate,
                                  getattr(audio, "spec_type", "mel-librosa"), n_mels=audio.n_mels)
    alignments = None
    if args.write_alignments:
        alignments = AlignmentWriter(args.output_dir, global_step, dataset.text_processor.symbols)
    paths = DtwPathWriter(args.output_dir, global_step, dataset.text_processor.symbols) if args.write_paths else None
    control = InferenceControl(pitch=args.pitch_control, energy=args.energy_control, duration=args.duration_control)
    t0 = time.perf_counter()
    res = synthesize(model, dataset, args.batch_size, control, writer, sort=sort, exact_lengths=args.exact_lengths,
                     scores=scores, alignments=alignments, compare=compare, paths=paths)
    torch.cuda.synchronize()
    report = {"finished": True, "utterances": res["utterances"], "files": len(res["files"]), "frames": res["frames"],
              "batches": res["batches"], "seconds": round(time.perf_counter() - t0, 3),
              "output_dir": str(writer.dir if writer is not None else args.output_dir)}
    if scores is not None:
        report["scores_file"] = str(scores.close())
    if compare is not None:
        report["dtw_file"] = str(compare.close())
    if paths is not None:
        report["path_files"] = len(res["path_files"])
        report["dtw_tokens_file"] = str(paths.close())
    if alignments is not None:
        report["alignment_files"] = len(res["alignment_files"])
    print(json.dumps(report), flush=True)
    return 0


def main(argv: Optional[list] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if args.command == "train":
        return train(args, argv)
    if args.command == "benchmark":
        return benchmark(args)
    if args.command == "synthesize":
        return synthesize_command(args)
    return 2


if __name__ == "__main__":
    raise SystemExit(main())
