"""GPU: ``fs2hip_pack_rows`` -- several small [B, T] tensors, every row cut to its utterance's length and packed back to
back in one call, the offsets computed on the device -- bit for bit against torch slicing and a host cumsum, with
poisoned destination and offsets buffers: what the call does not own keeps its sentinel."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from fastspeech2_lightning_amd import hip as H

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SENTINEL = 0x5EA7BEEF                # an int32 bit pattern no input holds (ints are drawn below 2^20; as fp32 it is 6e18)
OFF_SENTINEL = -(1 << 40)
SLACK = 5                            # elements behind the worst case that must keep the sentinel too


def _member(B, T, lens, dtype, seed):
    """(src on the host with poison at and beyond every length, lens as given, the clamped lengths)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int32:
        src = torch.randint(0, 1 << 20, (B, T), generator=g, dtype=torch.int32)
        poison = -1
    else:
        src = torch.randn(B, T, generator=g)
        poison = float("nan")
    clamped = [min(max(int(n), 0), T) for n in lens]
    for b, n in enumerate(clamped):
        src[b, n:] = poison   # elements at and beyond len_b must never reach the result
    return src, clamped


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _run_and_check(specs, B, odd_start=False, raw=False):
    """``specs``: [(T, lens, dtype)].  Packs them in one call and checks every member."""
    table, kept = [], []
    for i, (T, lens, dtype) in enumerate(specs):
        src, clamped = _member(B, T, lens, dtype, seed=100 + i)
        base = torch.full((B * T + SLACK + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        if odd_start:
            assert base.data_ptr() % 16 == 0
            base = base[1:]   # 4-byte but not 16-byte aligned
            assert base.data_ptr() % 16 == 4
        dst = base.view(dtype) if dtype == torch.float32 else base
        offsets = torch.full((B + 3,), OFF_SENTINEL, dtype=torch.int64, device="cuda")
        lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
        table.append((src.cuda(), lens_dev, dst, offsets))
        kept.append((src, clamped, base, offsets))
    if raw:
        arr = (H.PackMember * len(table))()
        for m, (src, lens_dev, dst, offsets) in zip(arr, table):
            m.src, m.lens, m.dst, m.offsets, m.T = src.data_ptr(), lens_dev.data_ptr(), dst.data_ptr(), offsets.data_ptr(), src.shape[1]
        assert H.lib().fs2hip_pack_rows(arr, len(table), B, H._stream()) == 0
    else:
        res = H.pack_rows(table, B)
        assert [r[0].data_ptr() for r in res] == [t[2].data_ptr() for t in table]
    torch.cuda.synchronize()
    for src, clamped, base, offsets in kept:
        want_offsets = torch.tensor([0] + clamped, dtype=torch.int64).cumsum(0)
        host_off = offsets.cpu()
        assert torch.equal(host_off[:B + 1], want_offsets)
        assert (host_off[B + 1:] == OFF_SENTINEL).all()
        total = int(want_offsets[-1])
        want = torch.cat([_bits(src[b, :n]) for b, n in enumerate(clamped)]) if total else torch.empty(0, dtype=torch.int32)
        host = base.cpu()
        assert torch.equal(host[:total], want)
        assert (host[total:] == SENTINEL).all()   # every byte at or beyond the member's total keeps its sentinel


def test_one_utterance():
    _run_and_check([(7, [5], torch.int32)], 1)
    _run_and_check([(7, [7], torch.float32)], 1)


@pytest.mark.parametrize("T", [1, 9, 257, 1030], ids=lambda t: f"T{t}")
def test_lengths_at_the_edges_and_clamped(T):
    """0, 1, T, T + 3 (clamped to T) and -2 (clamped to 0); T = 1030 needs two workgroups per row."""
    for dtype in (torch.int32, torch.float32):
        _run_and_check([(T, [0, 1, T, T + 3, -2], dtype)], 5)
    if T > 1024:
        _run_and_check([(T, [1024, 1025, T, 1023, 0], torch.float32)], 5)


def test_three_hundred_utterances_exercise_the_prologues_chunking():
    g = torch.Generator().manual_seed(3)
    lens = torch.randint(-1, 14, (300,), generator=g).tolist()
    _run_and_check([(11, lens, torch.int32)], 300)
    _run_and_check([(3, [3] * 300, torch.float32)], 300)


def test_three_members_with_their_own_T_lens_and_dtype():
    B = 4
    _run_and_check([(13, [13, 4, 0, 9], torch.int32), (13, [13, 4, 0, 9], torch.float32),
                    (70, [70, 33, 1, 64], torch.float32)], B)
    _run_and_check([(13, [13, 4, 0, 9], torch.int32), (70, [70, 33, 1, 64], torch.float32),
                    (1, [1, 0, 1, 1], torch.float32)], B, raw=True)


def test_eight_members():
    B = 3
    specs = [(5 + 37 * i, [5 + 37 * i, i, (7 * i) % 5], torch.float32 if i % 2 else torch.int32) for i in range(8)]
    _run_and_check(specs, B)


def test_destination_at_an_odd_element():
    _run_and_check([(257, [257, 3, 100], torch.float32), (6, [6, 0, 5], torch.int32)], 3, odd_start=True)


def test_members_of_one_call_may_sit_back_to_back_in_one_buffer():
    """The layout ``synthesize`` uses: int32 durations and fp32 predictions in one fp32 buffer, every member starting where
    the host knows the previous one ends."""
    B, T = 3, 6
    lens = [6, 2, 5]
    dur, _ = _member(B, T, lens, torch.int32, 1)
    pit, _ = _member(B, T, lens, torch.float32, 2)
    total = sum(lens)
    buf = torch.full((2 * total + SLACK + 2 * B * T,), float("inf"), device="cuda")
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
    H.pack_rows([(dur.cuda(), lens_dev, buf[:B * T], None), (pit.cuda(), lens_dev, buf[total:total + B * T], None)], B)
    host = buf.cpu()
    assert torch.equal(host[:total].view(torch.int32), torch.cat([dur[b, :n] for b, n in enumerate(lens)]))
    assert torch.equal(host[total:2 * total], torch.cat([pit[b, :n] for b, n in enumerate(lens)]))
    assert torch.isinf(host[2 * total:]).all()


def test_rejected_arguments_return_einval_and_write_nothing():
    B, T = 2, 4
    src = torch.arange(B * T, dtype=torch.int32, device="cuda").view(B, T)
    lens = torch.tensor([4, 2], dtype=torch.int32, device="cuda")
    dst = torch.full((B * T,), SENTINEL, dtype=torch.int32, device="cuda")
    offsets = torch.full((B + 1,), OFF_SENTINEL, dtype=torch.int64, device="cuda")
    L, s = H.lib(), H._stream()

    def table(n=1, **over):
        arr = (H.PackMember * 9)()
        for m in arr:
            m.src, m.lens, m.dst, m.offsets, m.T = src.data_ptr(), lens.data_ptr(), dst.data_ptr(), offsets.data_ptr(), T
        for k, v in over.items():
            setattr(arr[n - 1], k, v)   # (the LAST member is the bad one: the ones before it must not have been launched)
        return arr

    assert L.fs2hip_pack_rows(None, 1, B, s) == -22
    for n in (0, -1, H.PACK_MAX_MEMBERS + 1):
        assert L.fs2hip_pack_rows(table(), n, B, s) == -22
    for bad_B in (0, -3):
        assert L.fs2hip_pack_rows(table(), 1, bad_B, s) == -22
    for field in ("src", "lens", "dst", "offsets"):
        assert L.fs2hip_pack_rows(table(2, **{field: None}), 2, B, s) == -22, field
    for bad_T in (0, -1):
        assert L.fs2hip_pack_rows(table(2, T=bad_T), 2, B, s) == -22
    torch.cuda.synchronize()
    assert (dst.cpu() == SENTINEL).all() and (offsets.cpu() == OFF_SENTINEL).all()
    # the wrapper's own checks
    with pytest.raises(ValueError, match="members per call"):
        H.pack_rows([], B)
    with pytest.raises(ValueError, match="members per call"):
        H.pack_rows([(src, lens, None, None)] * 9, B)
    with pytest.raises(ValueError, match="fp32 or int32"):
        H.pack_rows([(src.long(), lens, None, None)], B)
    with pytest.raises(TypeError):
        H.pack_rows([(src, lens.long(), None, None)], B)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H.pack_rows([(src.cpu(), lens, None, None)], B)
    with pytest.raises(ValueError, match="worst case"):
        H.pack_rows([(src, lens, dst[:B * T - 1], None)], B)
    with pytest.raises(ValueError, match="entries"):
        H.pack_rows([(src, lens[:1], None, None)], B)
    with pytest.raises(ValueError, match="offsets holds"):
        H.pack_rows([(src, lens, None, offsets[:B])], B)
    with pytest.raises(ValueError, match="is not"):
        H.pack_rows([(src, lens, None, None)], B + 1)
    with pytest.raises(ValueError):
        H.pack_rows([(src.t(), lens, None, None)], T)
    torch.cuda.synchronize()
    assert (dst.cpu() == SENTINEL).all() and (offsets.cpu() == OFF_SENTINEL).all()


def test_pack_struct_layout_matches_header():
    text = (REPO / "include" / "fs2hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*?)\} Fs2PackMember;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = decl.replace("*", " ").split(",")
        names.append(parts[0].split()[-1])
        names += [p.strip() for p in parts[1:]]
    assert names == [f[0] for f in H.PackMember._fields_]
    assert ctypes.sizeof(H.PackMember) == 40
    assert int(re.search(r"#define FS2_PACK_MAX_MEMBERS (\d+)", text).group(1)) == H.PACK_MAX_MEMBERS
