"""attention_decode without a GPU: its refusals name their argument and come before the device check, the plan behind it
(rua_attention_decode_plan, a pure host function) keeps its promises, and the lse yardstick of
tests/attention_decode_util.py agrees with torch.logsumexp in float64."""
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _ops
import attention_band_util as U
import attention_decode_util as DU

LENS = torch.tensor([2, 3])


def cont(heads=4, D=32, lens=LENS, grad=False):
    return ta.C(torch.zeros(int(lens.sum()), heads, D, dtype=torch.bfloat16, requires_grad=grad), lens)


Q, KV = cont(), cont(2)
REFUSALS = {
    'too many queries': (lambda: cont(lens=torch.tensor([33, 1])).attention_decode(cont(2, lens=torch.tensor([33, 1])),
                                                                                   cont(2, lens=torch.tensor([33, 1]))),
                         '`q` holds a sequence of 33 queries.*`attention`'),
    'kv_chunk 0': (lambda: Q.attention_decode(KV, KV, kv_chunk=0), '`kv_chunk` = 0'),
    'kv_chunk 100': (lambda: Q.attention_decode(KV, KV, kv_chunk=100), '`kv_chunk` = 100'),
    'kv_chunk -128': (lambda: Q.attention_decode(KV, KV, kv_chunk=-128), '`kv_chunk` = -128'),
    'kv_chunk True': (lambda: Q.attention_decode(KV, KV, kv_chunk=True), '`kv_chunk` = True'),
    'requires grad': (lambda: Q.attention_decode(cont(2, grad=True), KV), '`k` requires grad.*`attention`'),
    'segment requires grad': (lambda: ta.segment_attention_decode(cont(grad=True).data, LENS, KV.data, KV.data, LENS),
                              '`q` requires grad.*`attention`'),
    # inherited from attention_args
    'heads no multiple': (lambda: Q.attention_decode(cont(3), cont(3)), '`k` has 3 heads, `q` 4'),
    'causal with right': (lambda: Q.attention_decode(KV, KV, window=(4, 1)), '`window` = .* right = 1 and `causal`'),
    # valid calls: only the device is wrong, and that refusal comes last
    'cpu': (lambda: Q.attention_decode(KV, KV, kv_chunk=256), '`q` lives on cpu'),
    'segment cpu': (lambda: ta.segment_attention_decode(Q.data, LENS, KV.data, KV.data, LENS, return_lse=True), '`q` lives on cpu'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_name_their_argument(case):
    call, match = REFUSALS[case]
    with pytest.raises(ta.RuaError, match=match):
        call()


def test_no_refusal_of_a_leaf_without_grad_mode():
    with torch.no_grad(), pytest.raises(ta.RuaError, match='`q` lives on cpu'):
        Q.attention_decode(cont(2, grad=True), KV)


@pytest.mark.parametrize('B,heads,heads_kv,T_max,S_max,chunk_in', [
    (64, 32, 8, 1, 8192, None), (4, 32, 8, 1, 32768, None), (2, 4, 1, 1, 5000, None), (1, 8, 1, 32, 128, None),
    (3, 8, 1, 7, 129, None), (5000, 3, 1, 6, 6, None), (12, 4, 2, 32, 300, 128), (2, 4, 4, 4, 1000, 384), (1, 4, 4, 1, 0, None),
])
@pytest.mark.parametrize('D', [32, 128])
def test_the_plan(B, heads, heads_kv, T_max, S_max, chunk_in, D):
    chunk, n_split, ws_bytes = _ops.attention_decode_plan(B, heads, heads_kv, D, T_max, S_max, chunk_in)
    assert chunk > 0 and chunk % 128 == 0 and n_split >= 1 and n_split * chunk >= S_max
    assert (n_split - 1) * chunk < max(S_max, 1), 'no split without a key'
    assert n_split == 1 or S_max > 128
    assert chunk_in is None or chunk == chunk_in
    ncb = -(-T_max * (heads // heads_kv) // 32)
    assert ws_bytes == (B * heads_kv * ncb * n_split * 32 * (D + 2) * 4 if n_split > 1 else 0)
    assert (chunk, n_split, ws_bytes) == _ops.attention_decode_plan(B, heads, heads_kv, D, T_max, S_max, chunk_in)
    if chunk_in is None and S_max > 128 and B * heads_kv * ncb < 2048:
        assert n_split > 1, 'an idle device and a long cache: the plan splits'


def test_lse_yardstick_agrees_with_torch_in_float64():
    qlens, klens, H, G, D, mask = [3, 1, 2], [4, 5, 1], 4, 2, 32, ('end', 2, 0)
    q, k = U.draw(qlens, H, D, torch.bfloat16, 1), U.draw(klens, H // G, D, torch.bfloat16, 2)
    lse, bound = DU.lse_reference(q, qlens, k, klens, mask, None, 1)
    rows = []
    for a, b in zip(q.to(U.F64).split(qlens), k.to(U.F64).split(klens)):
        s = D ** -0.5 * torch.einsum('thd,shd->ths', a, b.repeat_interleave(G, 1))
        rows.append(s.masked_fill(U.hide_of(a.size(0), b.size(0), *mask)[:, None, :], -float('inf')).logsumexp(-1))
    want = torch.cat(rows)
    dead = torch.isinf(want)
    assert bool(dead.any()) and torch.equal(torch.isinf(lse), dead) and bool((bound[dead] == 0).all()) and bool((bound[~dead] > 0).all())
    torch.testing.assert_close(lse[~dead], want[~dead], rtol=1e-12, atol=1e-12)
