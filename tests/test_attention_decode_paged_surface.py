"""attention_decode_paged without a GPU: the three names are exported and installed, every refusal names its argument
and comes before the device check, which a valid call reaches last."""
import pytest
import torch

import torchrua_amd as ta

LENS = torch.tensor([2, 3])
E4M3, BF16 = torch.float8_e4m3fn, torch.bfloat16
Q = ta.C(torch.zeros(5, 4, 32, dtype=BF16), LENS)
TABLE, SIZES = torch.zeros(2, 3, dtype=torch.int32), torch.tensor([40, 7])


def pages(dtype=BF16, n=4, ps=16, heads=2, D=32):
    return torch.zeros(n, ps, heads, D, dtype=torch.bfloat16).to(dtype)


def call(k=None, v=None, table=TABLE, sizes=SIZES, q=Q, **kw):
    k = pages() if k is None else k
    return lambda: q.attention_decode_paged(k, k.clone() if v is None else v, table, sizes, **kw)


KV8 = pages(E4M3)
REFUSALS = {
    'q no container': (lambda: ta.attention_decode_paged(Q.data, pages(), pages(), TABLE, SIZES), '`q` is a container'),
    'q dtype': (call(q=ta.C(Q.data.float(), LENS)), '`q` is one of'),
    'q 33 queries': (call(q=ta.C(torch.zeros(33, 4, 32, dtype=BF16), torch.tensor([33, 0]))), '`q` holds a sequence of 33'),
    'q grad': (call(q=ta.C(Q.data.clone().requires_grad_(), LENS)), '`q` requires grad'),
    'k 3-D': (call(k=pages()[0]), r'`k_pages` is a tensor \[num_pages, page_size, heads_kv, D\]'),
    'v no tensor': (call(v=3), '`v_pages` is a tensor'),
    'v shape': (call(v=pages(n=5)), '`v_pages` has the shape'),
    'k strided': (call(k=pages(D=64)[..., :32], v=pages()), '`k_pages` is contiguous'),
    'v strided': (call(v=pages(heads=4)[:, :, ::2]), '`v_pages` is contiguous'),
    'page_size 8': (call(k=pages(ps=8)), r'`k_pages` has page_size = 8'),
    'page_size 48': (call(k=pages(ps=48)), r'`k_pages` has page_size = 48'),
    'k float32': (call(k=pages(torch.float32)), '`k_pages` is one of'),
    'k f16, q bf16': (call(k=pages(torch.float16)), '`k_pages` has dtype torch.float16, `q` torch.bfloat16'),
    'k e5m2': (call(k=pages(torch.float8_e5m2)), '`k_pages` has dtype torch.float8_e5m2.*float8_e4m3fn'),
    'k fp8, v not': (call(k=KV8, v=pages()), '`v_pages` has dtype torch.bfloat16, `k_pages` torch.float8_e4m3fn'),
    'v fp8, k not': (call(v=KV8), '`v_pages` has dtype torch.float8_e4m3fn, `k_pages` torch.bfloat16'),
    'D': (call(k=pages(D=64)), r'`k_pages` has the hidden dimensions \(2, 64\)'),
    'head ratio': (call(k=pages(heads=3)), '`k_pages` has 3 heads, `q` 4'),
    'v device': (call(v=pages().to('meta')), '`v_pages` lives on meta'),
    'scale': (call(scale=float('nan')), '`scale` = nan'),
    'window': (call(window=-1), '`window` = -1'),
    'align': (call(align='middle'), "`align` = 'middle'"),
    'table int64': (call(table=TABLE.long()), '`page_table` is a contiguous int32 tensor'),
    'table 1-D': (call(table=TABLE[0]), '`page_table` is a contiguous int32 tensor'),
    'table rows': (call(table=torch.zeros(3, 3, dtype=torch.int32)), r'`page_table` .* = \[2, max_pages\]'),
    'table strided': (call(table=torch.zeros(2, 6, dtype=torch.int32)[:, ::2]), '`page_table` is a contiguous int32 tensor'),
    'table device': (call(table=TABLE.to('meta')), '`page_table` .*on meta'),
    'table list': (call(table=[[0]]), '`page_table` .*got list'),
    'sizes int32': (call(sizes=SIZES.int()), '`kv_sizes` is an int64 tensor'),
    'sizes length': (call(sizes=torch.tensor([1, 2, 3])), r'`kv_sizes` is an int64 tensor \[B\] = \[2\]'),
    'kv_chunk': (call(kv_chunk=100), '`kv_chunk` = 100'),
    'k grad': (call(k=pages().requires_grad_()), '`k_pages` requires grad'),
    'k_scale with bf16': (call(k_scale=2.0), '`k_scale` is given'),
    'v_scale shape': (call(k=KV8, v_scale=torch.ones(4)), r'`v_scale` is a float32 tensor \[heads_kv\] = \[2\]'),
    'k_scale 0': (call(k=KV8, k_scale=0.0), '`k_scale` = 0.0'),
    'table too short': (call(sizes=torch.tensor([49, 7])), '`page_table` has 3 columns of 16 keys .* holds 49'),
    'segment q': (lambda: ta.segment_attention_decode_paged(Q, LENS, pages(), pages(), TABLE, SIZES), '`q` is a tensor'),
    'segment table': (lambda: ta.segment_attention_decode_paged(Q.data, LENS, pages(), pages(), TABLE.long(), SIZES),
                      '`page_table` is a contiguous int32 tensor'),
    # valid calls: only the device is wrong, and that refusal comes last
    'cpu': (call(sizes=torch.tensor([48, 7]), kv_chunk=128), '`q` lives on cpu'),
    'cpu fp8': (call(k=KV8, k_scale=0.5, v_scale=torch.ones(2), return_lse=True), '`q` lives on cpu'),
    'segment cpu': (lambda: ta.segment_attention_decode_paged(Q.data, LENS, KV8, KV8, TABLE, SIZES, v_scale=3), '`q` lives on cpu'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_name_their_argument(case):
    fn, match = REFUSALS[case]
    with pytest.raises(ta.RuaError, match=match):
        fn()


def test_the_names_are_exported_and_installed():
    assert callable(ta.attention_decode_paged) and callable(ta.segment_attention_decode_paged)
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.attention_decode_paged is ta.attention_decode_paged
