"""The band form of attention without a GPU: the new refusals name their argument and come before the device check, valid
grouped-query and windowed calls on CPU tensors reach that check, and the yardstick of tests/attention_band_util.py agrees
with torch's own attention in float64 under an explicit boolean mask and repeat_interleave'd K / V."""
import pytest
import torch
import torch.nn.functional as F

import torchrua_amd as ta
import attention_band_util as U

LENS = torch.tensor([2, 3])


def cont(heads=4, D=32):
    return ta.C(torch.zeros(int(LENS.sum()), heads, D, dtype=torch.bfloat16), LENS)


Q, KV = cont(), cont(2)
REFUSALS = {
    'heads no multiple': (lambda: Q.attention(cont(3), cont(3)), '`k` has 3 heads, `q` 4'),
    'v unlike k': (lambda: Q.attention(KV, cont(1)), r'`v` has the hidden dimensions \(1, 32\), `k` \(2, 32\)'),
    'negative window': (lambda: Q.attention(KV, KV, window=-1), '`window` = -1'),
    'bool window': (lambda: Q.attention(KV, KV, window=True), '`window` = True'),
    'float side': (lambda: Q.attention(KV, KV, window=(1.0, None)), '`window` = '),
    'three sides': (lambda: Q.attention(KV, KV, window=(1, 2, 3)), '`window` = '),
    'causal with right': (lambda: Q.attention(KV, KV, causal=True, window=(4, 1)), '`window` = .* right = 1 and `causal`'),
    'align': (lambda: Q.attention(KV, KV, align='middle'), "`align` = 'middle'"),
    'segment align': (lambda: ta.segment_attention(Q.data, LENS, KV.data, KV.data, LENS, align=None), '`align` = None'),
    # valid calls: only the device is wrong
    'gqa': (lambda: Q.attention(KV, KV), '`q` lives on cpu'),
    'mqa, window, end': (lambda: Q.attention(cont(1), cont(1), causal=True, window=(3, None), align='end'), '`q` lives on cpu'),
    'segment window': (lambda: ta.segment_attention(Q.data, LENS, KV.data, KV.data, LENS, window=(0, 2 ** 70)), '`q` lives on cpu'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_name_their_argument(case):
    call, match = REFUSALS[case]
    with pytest.raises(ta.RuaError, match=match) as err:
        call()
    assert 'out of scope' not in str(err.value)


@pytest.mark.parametrize('mask', [('end', 2, 0), ('start', 1, 2), ('end', None, 1)])
def test_yardstick_agrees_with_torch_in_float64(mask):
    qlens, klens, H, G, D = [3, 5, 2], [4, 5, 6], 4, 2, 32     # every query has a visible key
    q, k, v, g = (U.draw(n, h, D, torch.bfloat16, s) for n, h, s in ((qlens, H, 1), (klens, H // G, 2), (klens, H // G, 3), (qlens, H, 4)))
    (out, dq, dk, dv), bounds, _ = U.reference(q, qlens, k, v, klens, g, mask, None, torch.bfloat16)
    assert all(bool((b > 0).all()) for b in bounds[:2])
    pad = lambda x, lens: torch.nn.utils.rnn.pad_sequence(x.to(U.F64).split(lens), True).transpose(1, 2)   # noqa: E731
    pq, pk, pv = pad(q, qlens).requires_grad_(), pad(k, klens).requires_grad_(), pad(v, klens).requires_grad_()
    see = torch.zeros(len(qlens), 1, max(qlens), max(klens), dtype=torch.bool)
    for b, (T, S) in enumerate(zip(qlens, klens)):
        see[b, 0, :T, :S] = ~U.hide_of(T, S, *mask)
    see[:, :, :, 0] |= ~see.any(-1)                              # padding queries: any key, their rows are dropped
    want = F.scaled_dot_product_attention(pq, pk.repeat_interleave(G, 1), pv.repeat_interleave(G, 1), attn_mask=see)
    unpad = lambda x, lens: torch.cat([x[b, :, :n].transpose(0, 1) for b, n in enumerate(lens)])           # noqa: E731
    wq, wk, wv = torch.autograd.grad(unpad(want, qlens), (pq, pk, pv), g.to(U.F64))
    for got, exp in ((out, unpad(want, qlens)), (dq, unpad(wq, qlens)), (dk, unpad(wk, klens)), (dv, unpad(wv, klens))):
        torch.testing.assert_close(got, exp.detach(), rtol=1e-12, atol=1e-12)
