"""The REFERENCE resumes a checkpoint written by the HIP model -- ``tests/golden/hip_written.ckpt``, produced on an MI355X
by ``python -m tests.test_ckpt_interchange_gpu`` after three training steps.  What the reference did with that file -- its
own ``on_load_checkpoint`` (fs2/model.py:353-367), strict ``load_state_dict``, ``torch.optim.AdamW.load_state_dict`` and
``NoamLR.load_state_dict``, then a fourth training step -- is recorded in ``tests/golden/hip_written_ref_resume.npz``
(``python oracle/make_golden.py resume``, where the reference's sources are at hand).  Here: that record is of this very
file, its fourth step reproduces the loss and weights the HIP run recorded for its own fourth step, and the CPU oracle
(the reference's path restated in PyTorch) takes the file the same way and reproduces the reference's step."""
import hashlib
import json

import numpy as np
import torch


def test_reference_accepts_and_resumes_a_checkpoint_written_by_the_hip_model(golden_dir):
    from fastspeech2_lightning_amd.config import FastSpeech2Config, Stats
    from fastspeech2_lightning_amd.optim import NoamLR, noam_scale
    from oracle import cases as C
    from oracle import fs2_oracle as O
    from oracle import make_golden as MG

    path = golden_dir / "hip_written.ckpt"
    rec = np.load(golden_dir / "hip_written_ref_resume.npz")
    assert str(rec["ckpt_sha256"]) == hashlib.sha256(path.read_bytes()).hexdigest(), "record of another checkpoint"
    expect = json.loads((golden_dir / "hip_written.json").read_text())
    g = np.load(golden_dir / "ckpt_interchange.npz")
    # the reference: config and schedule taken from the file, and its fourth step is the HIP run's
    assert not bool(rec["use_postnet"]) and int(rec["warmup_steps"]) == 2
    assert int(rec["last_epoch"]) == 3 and int(rec["global_step"]) == 3
    l4 = float(rec["loss_4"])
    assert abs(l4 - expect["loss_4"]) < 1e-4 * expect["loss_4"], (l4, expect["loss_4"])
    # and the weights after that step are the HIP run's (Adam moments and step count really came across)
    for k, probe in expect["after_4"].items():
        got = rec[f"sd_after_4/{k}"].reshape(-1)[:8]
        assert float(np.abs(got - np.asarray(probe)).max()) < 2e-4, (k, got.tolist(), probe)
    # the two trajectories are the same run: the reference's own three steps gave the same losses
    assert np.abs(np.asarray(expect["losses_1_3"]) - g["losses_1_3"]).max() < 2e-3 * g["losses_1_3"].max()

    # the oracle, driven the way Lightning drives the reference: hyper-parameters from the file, strict weights, AdamW
    # and NoamLR built first and then loaded with the file's state
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    hp = ckpt["hyper_parameters"]
    config, stats = FastSpeech2Config(**hp["config"]), Stats(**hp["stats"])
    assert config.model.use_postnet is False and config.training.optimizer.warmup_steps == 2
    oracle = O.FastSpeech2Oracle(config, stats, n_symbols=C.N_SYMBOLS)
    before = {k: v.clone() for k, v in ckpt["state_dict"].items()}
    oracle.load_state_dict(ckpt["state_dict"], strict=True)
    o = config.training.optimizer
    opt = torch.optim.AdamW(oracle.parameters(), o.learning_rate, betas=tuple(o.betas), eps=o.eps,
                            weight_decay=o.weight_decay)
    sched = NoamLR(opt, o.warmup_steps)
    opt.load_state_dict(ckpt["optimizer_states"][0])
    sched.load_state_dict(ckpt["lr_schedulers"][0])
    assert sched.last_epoch == 3 and ckpt["global_step"] == 3
    batch = {k[6:]: (int(g[k]) if g[k].ndim == 0 else torch.from_numpy(g[k])) for k in g.files if k.startswith("batch/")}
    oracle.train()
    _, _, (o4,) = MG.reference_train_steps(oracle, batch, 1, opt, sched)
    assert abs(o4 - l4) < 1e-5 * l4, (o4, l4)
    lr4 = o.learning_rate * noam_scale(4, o.warmup_steps)
    num = den = 0.0
    for k, v in oracle.state_dict().items():
        if not v.dtype.is_floating_point:
            continue
        want = torch.from_numpy(rec[f"sd_after_4/{k}"])
        assert float((v - want).abs().max()) <= 2.0 * lr4 * 1.01, k   # (at most an Adam sign flip on a noise-level element)
        num += float(((v - before[k]) - (want - before[k])).pow(2).sum())
        den += float((want - before[k]).pow(2).sum())
    assert (num / den) ** 0.5 < 1e-4, (num / den) ** 0.5
