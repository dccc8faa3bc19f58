"""GPU: ``fs2hip_pack_spec`` -- a batch's valid frames, transposed to [bands, frames] and packed back to back, with the
offsets computed on the device -- bit-exact against ``torch.cat([y[b, :l].T.reshape(-1) ...])`` and a host cumsum."""
import pytest
import torch

from fastspeech2_lightning_amd import hip as H

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0

#: (B, Tm, C, lens): tile edges at 31-33 and 63-65 frames, a C that is no multiple of 4, zero lengths in the middle / at the end
CASES = [
    (1, 1, 1, [1]),
    (3, 70, 80, [70, 1, 0]),
    (2, 129, 128, [64, 129]),
    (5, 65, 20, [65, 63, 64, 33, 2]),
    (4, 33, 3, [33, 32, 31, 0]),
]


def _inputs(B, Tm, C, lens, seed=0):
    y = torch.randn(B, Tm, C, generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lens):
        y[b, n:] = float("nan")   # rows at and beyond len_b must never reach the result
    return y


@pytest.mark.parametrize("B,Tm,C,lens", CASES, ids=[f"B{c[0]}-Tm{c[1]}-C{c[2]}" for c in CASES])
def test_pack_spec_matches_torch(B, Tm, C, lens):
    y = _inputs(B, Tm, C, lens)
    want = torch.cat([y[b, :n].T.reshape(-1) for b, n in enumerate(lens)])
    want_offsets = torch.tensor([0] + [C * n for n in lens]).cumsum(0)
    packed = torch.full((B * Tm * C,), SENTINEL, device="cuda")
    got, offsets = H.pack_spec(y.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"), packed)
    assert got.data_ptr() == packed.data_ptr() and offsets.dtype == torch.int64 and offsets.shape == (B + 1,)
    assert torch.equal(offsets.cpu(), want_offsets)
    total = int(want_offsets[-1])
    host = packed.cpu()
    assert torch.isfinite(host[:total]).all()
    assert torch.equal(host[:total], want)
    assert (host[total:] == SENTINEL).all()     # nothing behind the payload is touched
    # every utterance is its own [C, len] block
    for b, n in enumerate(lens):
        lo = int(want_offsets[b])
        assert torch.equal(host[lo:lo + C * n].reshape(C, n), y[b, :n].T)


def test_pack_spec_allocates_the_worst_case_and_the_offsets():
    B, Tm, C, lens = CASES[3]
    y = _inputs(B, Tm, C, lens, seed=1)
    packed, offsets = H.pack_spec(y.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"))
    assert packed.numel() == B * Tm * C and offsets.tolist() == [0, 1300, 2560, 3840, 4500, 4540]
    assert torch.equal(packed[:4540].cpu(), torch.cat([y[b, :n].T.reshape(-1) for b, n in enumerate(lens)]))


def test_rejected_arguments_raise_and_launch_nothing():
    lens = torch.tensor([2, 3], dtype=torch.int32, device="cuda")
    y = torch.randn(2, 4, 8, device="cuda")
    packed = torch.full((2 * 4 * 8,), SENTINEL, device="cuda")
    offsets = torch.full((3,), -5, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="empty"):
        H.pack_spec(torch.empty(0, 4, 8, device="cuda"), lens[:0], packed, offsets)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.pack_spec(y.cpu(), lens, packed, offsets)
    with pytest.raises(ValueError, match="contiguous"):
        H.pack_spec(torch.randn(2, 8, 4, device="cuda").transpose(1, 2), lens, packed, offsets)
    with pytest.raises(ValueError, match="worst case"):
        H.pack_spec(y, lens, packed[:40], offsets)
    with pytest.raises(ValueError, match="lens has"):
        H.pack_spec(y, lens[:1], packed, offsets)
    with pytest.raises(TypeError):
        H.pack_spec(y, lens.long(), packed, offsets)
    # the C entry point itself refuses non-positive extents and null pointers with -22
    L = H.real_lib()
    s = torch.cuda.current_stream().cuda_stream
    for args in ((0, 4, 8), (2, 0, 8), (2, 4, 0)):
        assert L.fs2hip_pack_spec(y.data_ptr(), lens.data_ptr(), packed.data_ptr(), offsets.data_ptr(), *args, s) == -22
    assert L.fs2hip_pack_spec(None, lens.data_ptr(), packed.data_ptr(), offsets.data_ptr(), 2, 4, 8, s) == -22
    assert L.fs2hip_pack_spec(y.data_ptr(), lens.data_ptr(), packed.data_ptr(), None, 2, 4, 8, s) == -22
    torch.cuda.synchronize()
    assert (packed == SENTINEL).all() and (offsets == -5).all()
