"""Per-sequence attention without a GPU: every refusal names its argument (the device check comes last, so CPU tensors
reach all the others), and the yardstick of tests/attention_util.py agrees with torch's own attention in float64."""
import math

import pytest
import torch
import torch.nn.functional as F

import torchrua_amd as ta
import attention_util as U

LENS = torch.tensor([2, 3])


def cont(dtype=torch.bfloat16, hidden=(2, 32), lens=LENS, kind='C'):
    c = ta.C(torch.zeros((int(lens.sum()),) + hidden, dtype=dtype), lens)
    return c if kind == 'C' else ta.L(torch.zeros((lens.numel(), int(lens.max())) + hidden, dtype=dtype), lens)


Q = cont()
REFUSALS = {
    'q is no container': (lambda: ta.attention(Q.data, Q, Q), '`q` is a container'),
    'v is no container': (lambda: Q.attention(Q, Q.data), '`v` is a container'),
    'fp32': (lambda: cont(torch.float32).attention(Q, Q), '`q` is one of'),
    'dtypes differ': (lambda: Q.attention(cont(torch.float16), Q), '`k` has dtype'),
    'one hidden dimension': (lambda: cont(hidden=(32,)).attention(Q, Q), r'`q` has exactly the hidden dimensions \(heads, D\)'),
    'other heads': (lambda: Q.attention(Q, cont(hidden=(4, 32))), '`v` has the hidden dimensions'),
    'D = 48': (lambda: cont(hidden=(2, 48)).attention(cont(hidden=(2, 48)), cont(hidden=(2, 48))), 'D = 48'),
    'k and v types': (lambda: Q.attention(Q, cont(kind='L')), '`k` and `v` are containers of ONE type'),
    'k and v lengths': (lambda: Q.attention(Q, cont(lens=torch.tensor([3, 2]))), '`k` and `v` have the same lengths'),
    'other B': (lambda: Q.attention(*[cont(lens=torch.tensor([2, 2, 1]))] * 2), '`k` holds 3 sequences'),
    'other device': (lambda: Q.attention(ta.C(Q.data.to('meta'), LENS), Q), '`k` lives on meta'),
    'scale': (lambda: Q.attention(Q, Q, scale=math.nan), '`scale` = nan'),
    'scale type': (lambda: Q.attention(Q, Q, scale='1'), '`scale` = '),
    'cpu': (lambda: Q.attention(Q, Q), '`q` lives on cpu'),
    'segment form': (lambda: ta.segment_attention(Q.data, LENS, Q.data, Q.data[:3], LENS), '`k` and `v` have the same lengths'),
    'segment cpu': (lambda: ta.segment_attention(Q.data, LENS, Q.data, Q.data, LENS), '`q` lives on cpu'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_name_their_argument(case):
    call, match = REFUSALS[case]
    with pytest.raises(ta.RuaError, match=match):
        call()


@pytest.mark.parametrize('causal', [False, True])
def test_yardstick_agrees_with_torch_in_float64(causal):
    qlens, klens, H, D = [3, 0, 5, 2], [4, 2, 5, 1], 2, 32
    klens = qlens if causal else klens
    q, k, v, g = (U.draw(n, H, D, torch.bfloat16, s) for n, s in ((qlens, 1), (klens, 2), (klens, 3), (qlens, 4)))
    (out, dq, dk, dv), _, _ = U.reference(q, qlens, k, v, klens, g, causal, None, torch.bfloat16)
    pad = lambda x, lens: torch.nn.utils.rnn.pad_sequence(x.to(U.F64).split(lens), True).transpose(1, 2)   # noqa: E731
    pq, pk, pv = pad(q, qlens).requires_grad_(), pad(k, klens).requires_grad_(), pad(v, klens).requires_grad_()
    mask = (torch.arange(max(klens)) < torch.tensor(klens)[:, None])[:, None, None, :].expand(-1, 1, max(qlens), -1)
    if causal:
        mask = mask & torch.ones(max(qlens), max(klens), dtype=torch.bool).tril()
    want = F.scaled_dot_product_attention(pq, pk, pv, attn_mask=mask)
    unpad = lambda x, lens: torch.cat([x[b, :, :n].transpose(0, 1) for b, n in enumerate(lens)])           # noqa: E731
    wq, wk, wv = torch.autograd.grad(unpad(want, qlens), (pq, pk, pv), g.to(U.F64))
    for got, exp in ((out, unpad(want, qlens)), (dq, unpad(wq, qlens)), (dk, unpad(wk, klens)), (dv, unpad(wv, klens))):
        torch.testing.assert_close(got, exp.detach(), rtol=1e-12, atol=1e-12)
