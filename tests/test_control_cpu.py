"""CPU: ``InferenceControl`` takes a float or a tensor per field (the reference multiplies by plain broadcasting,
fs2/variance_adaptor.py:203, :360-366), and the CPU oracle with a constant [B, Ts] tensor equals the oracle with the
float -- what makes it the yardstick of tests/test_control_gpu.py."""
import pytest
import torch

from fastspeech2_lightning_amd.config import InferenceControl, Stats
from oracle import cases as C
from oracle import fs2_oracle as O
from tests.test_headdim_model_gpu import N_SYMBOLS, config_for


def test_inference_control_round_trips_floats():
    assert InferenceControl().model_dump() == dict(pitch=1.0, energy=1.0, duration=1.0)
    c = InferenceControl(pitch=0.9, energy=2, duration="1.5")
    assert (c.pitch, c.energy, c.duration) == (0.9, 2.0, 1.5)
    assert all(type(v) is float for v in (c.pitch, c.energy, c.duration))
    assert InferenceControl(**c.model_dump()) == c
    assert InferenceControl.model_validate_json(c.model_dump_json()) == c
    assert InferenceControl(pitch=1.0) == InferenceControl()
    with pytest.raises(ValueError):
        InferenceControl(pitch="loud")
    with pytest.raises(ValueError):
        InferenceControl(duration=[1.0, 2.0])


def test_inference_control_holds_tensors():
    p, e, d = torch.rand(2, 5), torch.tensor(1.5), torch.ones(2, dtype=torch.float64)
    c = InferenceControl(pitch=p, energy=e, duration=d)
    assert c.pitch is p and c.energy is e and c.duration is d  # kept as given: no copy, no conversion to a float
    c.pitch = 0.5
    assert c.pitch == 0.5 and c.duration is d
    assert InferenceControl(pitch=p).energy == 1.0


def test_oracle_constant_tensor_control_equals_float():
    config = config_for(32, 2)
    oracle = O.FastSpeech2Oracle(config, Stats(**C.STATS), n_symbols=N_SYMBOLS)
    sd = O.seeded_state_dict(oracle.state_dict())
    sd["variance_adaptor.duration_predictor.linear.bias"] = torch.tensor([1.2])  # a useful spread of durations
    oracle.load_state_dict(sd)
    oracle.eval()
    batch = O.synthetic_batch(B=2, ts_lo=6, ts_hi=12, n_symbols=N_SYMBOLS, n_mels=80, seed=7, dur_hi=5)
    infer = {k: v for k, v in batch.items() if k not in ("mel", "pitch", "energy", "duration")}
    infer.update(mel=None, mel_lens=None, max_mel_len=1_000_000, duration=None)
    B, Ts = infer["text"].shape
    with torch.no_grad():
        want = oracle(dict(infer), InferenceControl(pitch=1.25, energy=0.75, duration=1.5), inference=True)
        got = oracle(dict(infer), InferenceControl(pitch=torch.full((B, Ts), 1.25), energy=torch.full((B, Ts), 0.75),
                                                   duration=torch.full((B, Ts), 1.5)), inference=True)
    assert int(want["tgt_lens"].max()) > Ts
    for k, v in want.items():
        if torch.is_tensor(v):
            assert torch.equal(v, got[k]), k
        else:
            assert v == got[k], k
