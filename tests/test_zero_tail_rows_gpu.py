"""GPU: ``hip.zero_tail_rows`` (``fs2hip_zero_tail_rows``, csrc/mask.hip), the mask of exact-length inference: rows at and
beyond an utterance's length become all-zero bytes by stores (NaN in the tail included), rows below it keep every bit.
One case per store width: 16-byte, 4-byte (a 20-byte row; a base 4 bytes into an allocation) and 2-byte (6-byte bf16 rows)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 4, 7
LENS = [0, 7, 3, 9]   # empty, full, ragged, beyond T (clamps to T)
GUARD = 64            # elements on either side of the tensor that must stay as they were


def _ints(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(cols, dtype, offset_elems=0):
    from fastspeech2_lightning_amd import hip
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    n = B * T * cols
    alloc = torch.randn(offset_elems + GUARD + n + GUARD, generator=g).to(dtype).to(dev)
    x = alloc[offset_elems + GUARD:offset_elems + GUARD + n].view(B, T, cols)
    assert x.is_contiguous() and x.data_ptr() == alloc.data_ptr() + (offset_elems + GUARD) * alloc.element_size()
    for b, n_valid in enumerate(LENS):   # NaN and Inf in some tail rows: a multiply would keep them
        if n_valid < T:
            x[b, n_valid, 0] = float("nan")
            x[b, T - 1, cols - 1] = float("inf")
    before = alloc.clone()
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    out = hip.zero_tail_rows(x, lens, B, T)
    torch.cuda.synchronize()
    assert out.data_ptr() == x.data_ptr()
    x0 = before[offset_elems + GUARD:offset_elems + GUARD + n].view(B, T, cols)
    for b, n_valid in enumerate(LENS):
        k = min(max(n_valid, 0), T)
        assert torch.equal(_ints(x[b, :k].contiguous()), _ints(x0[b, :k].contiguous())), (b, "valid rows moved")
        assert int(_ints(x[b, k:].contiguous()).abs().max() if k < T else 0) == 0, (b, "tail not all-zero bytes")
    # nothing outside the tensor was written
    lo, hi = offset_elems + GUARD, offset_elems + GUARD + n
    assert torch.equal(_ints(alloc[lo - GUARD:lo]), _ints(before[lo - GUARD:lo]))
    assert torch.equal(_ints(alloc[hi:hi + GUARD]), _ints(before[hi:hi + GUARD]))
    return x


@pytest.mark.parametrize("cols,dtype", [(5, torch.float32), (8, torch.float32), (3, torch.bfloat16)],
                         ids=["fp32x5_20B_rows", "fp32x8_vector", "bf16x3_6B_rows"])
def test_tail_rows_become_zero_and_valid_rows_keep_their_bits(cols, dtype):
    x = _run(cols, dtype)
    assert x.data_ptr() % 16 == 0
    assert (x.element_size() * cols % 16 == 0) == (cols == 8)   # only the 8-column case is on the 16-byte path


def test_base_four_bytes_into_an_allocation_takes_the_narrow_path():
    """32-byte rows from a base that is 4 mod 16: 16-byte stores would be misaligned, 4-byte stores are used."""
    x = _run(8, torch.float32, offset_elems=1)
    assert x.data_ptr() % 16 == 4


def test_shape_checks():
    from fastspeech2_lightning_amd import hip
    dev = torch.device("cuda")
    x = torch.zeros(B, T, 8, device=dev)
    lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        hip.zero_tail_rows(x, lens[:3], B, T)
    with pytest.raises(ValueError):
        hip.zero_tail_rows(x, lens, B, T + 1)       # x is [B, T, 8], not [B, T + 1, ...]
    with pytest.raises(TypeError):
        hip.zero_tail_rows(x, lens.long(), B, T)
    with pytest.raises(ValueError):
        hip.zero_tail_rows(x.to(torch.float16), lens, B, T)
