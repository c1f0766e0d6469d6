"""attention_paged without a GPU: the three names are exported and installed, the C symbol is declared, every refusal
names its argument and comes before the device check, which a valid call — 100 queries in a sequence — reaches last."""
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

LENS = torch.tensor([100, 3])
E4M3, BF16 = torch.float8_e4m3fn, torch.bfloat16
Q = ta.C(torch.zeros(103, 4, 32, dtype=BF16), LENS)
TABLE, SIZES = torch.zeros(2, 8, dtype=torch.int32), torch.tensor([120, 7])


def pages(dtype=BF16, n=4, ps=16, heads=2, D=32):
    return torch.zeros(n, ps, heads, D, dtype=torch.bfloat16).to(dtype)


def call(k=None, v=None, table=TABLE, sizes=SIZES, q=Q, **kw):
    k = pages() if k is None else k
    return lambda: q.attention_paged(k, k.clone() if v is None else v, table, sizes, **kw)


KV8 = pages(E4M3)
REFUSALS = {
    'q no container': (lambda: ta.attention_paged(Q.data, pages(), pages(), TABLE, SIZES), '`q` is a container'),
    'q dtype': (call(q=ta.C(Q.data.float(), LENS)), '`q` is one of'),
    'q grad': (call(q=ta.C(Q.data.clone().requires_grad_(), LENS)), '`q` requires grad .*`attention` is the differentiable'),
    'k grad': (call(k=pages().requires_grad_()), '`k_pages` requires grad'),
    'k 3-D': (call(k=pages()[0]), r'`k_pages` is a tensor \[num_pages, page_size, heads_kv, D\]'),
    'v shape': (call(v=pages(n=5)), '`v_pages` has the shape'),
    'k strided': (call(k=pages(D=64)[..., :32], v=pages()), '`k_pages` is contiguous'),
    'page_size 48': (call(k=pages(ps=48)), r'`k_pages` has page_size = 48'),
    'k fp8, v not': (call(k=KV8, v=pages()), '`v_pages` has dtype torch.bfloat16, `k_pages` torch.float8_e4m3fn'),
    'v fp8, k not': (call(v=KV8), '`v_pages` has dtype torch.float8_e4m3fn, `k_pages` torch.bfloat16'),
    'scale': (call(scale=float('nan')), '`scale` = nan'),
    'window': (call(window=-1), '`window` = -1'),
    'window right, causal': (call(window=(3, 2)), r'`window` = \(3, 2\) has right = 2 and `causal` is set'),
    'align': (call(align='middle'), "`align` = 'middle'"),
    'table int64': (call(table=TABLE.long()), '`page_table` is a contiguous int32 tensor'),
    'table rows': (call(table=torch.zeros(3, 8, dtype=torch.int32)), r'`page_table` .* = \[2, max_pages\]'),
    'sizes int32': (call(sizes=SIZES.int()), '`kv_sizes` is an int64 tensor'),
    'k_scale with bf16': (call(k_scale=2.0), '`k_scale` is given'),
    'v_scale shape': (call(k=KV8, v_scale=torch.ones(4)), r'`v_scale` is a float32 tensor \[heads_kv\] = \[2\]'),
    'table too short': (call(sizes=torch.tensor([129, 7])), '`page_table` has 8 columns of 16 keys .* holds 129'),
    'no kv_chunk': (call(kv_chunk=128), 'kv_chunk'),
    'segment q': (lambda: ta.segment_attention_paged(Q, LENS, pages(), pages(), TABLE, SIZES), '`q` is a tensor'),
    # valid calls with 100 queries in a sequence: only the device is wrong, and that refusal comes last
    'cpu': (call(), '`q` lives on cpu'),
    'cpu fp8': (call(k=KV8, k_scale=0.5, v_scale=torch.ones(2), return_lse=True, causal=False, window=(3, 2)), '`q` lives on cpu'),
    'segment cpu': (lambda: ta.segment_attention_paged(Q.data, LENS, KV8, KV8, TABLE, SIZES, v_scale=3), '`q` lives on cpu'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_name_their_argument(case):
    fn, match = REFUSALS[case]
    with pytest.raises(TypeError if case == 'no kv_chunk' else ta.RuaError, match=match):
        fn()


def test_the_names_are_exported_and_installed():
    assert callable(ta.attention_paged) and callable(ta.segment_attention_paged)
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.attention_paged is ta.attention_paged
    assert 'rua_segment_attention_paged_forward' in _lib.SYMBOLS
