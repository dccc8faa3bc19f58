"""GPU: ``fs2hip_attn_softmax_own_keys`` -- the aligner's log_softmax over an utterance's OWN keys, which is what
exact-length inference needs for ``attn_logprob`` (and through it the CTC score) not to follow the batch's longest text.

Yardstick: float64 on the CPU, ``log_softmax(logits[:, :L]) + log(prior + 1e-8)`` and the softmax of that over the same
keys; bound ``1e-4 * max(1, |ref|)`` as for every loss input.  And the property that matters: a row of a padded batch equals
the utterance run alone (``T2 = L``) through the plain entry point, where there is nothing to leave out."""
import pytest
import torch

from fastspeech2_lightning_amd import hip

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,T1,T2", [(1, 5, 7), (3, 23, 12), (4, 9, 130)])
def test_rows_equal_the_utterance_alone(B, T1, T2):
    g = torch.Generator().manual_seed(100 * T2 + B)
    logits = (-torch.rand(B, T1, T2, generator=g) * 3).cuda()
    prior = (torch.rand(B, T1, T2, generator=g) + 0.05).cuda()
    lens = [T2, 1, max(1, T2 // 2), max(1, T2 - 1)][:B]
    key_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    logprob, soft = hip.attn_softmax(logits, prior, key_lens, own_keys=True)
    plain_lp, plain_soft = hip.attn_softmax(logits, prior, key_lens)
    worst = 0.0
    for b, L in enumerate(lens):
        x, p = logits[b, :, :L].cpu().double(), prior[b, :, :L].cpu().double()
        ref_lp = torch.log_softmax(x, -1) + torch.log(p + 1e-8)
        ref_soft = torch.softmax(ref_lp, -1)
        for got, ref in ((logprob[b, :, :L], ref_lp), (soft[b, :, :L], ref_soft)):
            err = (got.cpu().double() - ref).abs()
            tol = 1e-4 * ref.abs().clamp(min=1.0)
            worst = max(worst, float((err / tol).max()))
            assert bool((err <= tol).all()), (b, L)
        assert float(soft[b, :, L:].abs().sum()) == 0.0
        # alone through the plain entry point: the same bits (same code, same keys, same order)
        a_lp, a_soft = hip.attn_softmax(logits[b:b + 1, :, :L].contiguous(), prior[b:b + 1, :, :L].contiguous(),
                                        key_lens[b:b + 1].contiguous())
        assert torch.equal(a_lp[0], logprob[b, :, :L]) and torch.equal(a_soft[0], soft[b, :, :L]), (b, L)
        if L < T2:   # and the plain form on the padded batch does differ: the reason this entry point exists
            assert float((plain_lp[b, :, :L] - logprob[b, :, :L]).abs().min()) > 1e-3
        else:
            assert torch.equal(plain_lp[b], logprob[b]) and torch.equal(plain_soft[b], soft[b])
    print(f"B={B} T1={T1} T2={T2}: worst error / bound {worst:.4f}")


def test_argument_errors():
    x = torch.zeros(1, 2, 3, device="cuda")
    k = torch.ones(1, dtype=torch.int32, device="cuda")
    L = hip.real_lib()
    assert L.fs2hip_attn_softmax_own_keys(x.data_ptr(), x.data_ptr(), k.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 2, 3,
                                          hip._stream()) == -22
    assert L.fs2hip_attn_softmax_own_keys(None, x.data_ptr(), k.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 2, 3,
                                          hip._stream()) == -22
