"""attention_decode over a float8_e4m3fn cache without a GPU: every refusal names its argument and comes before the
device check, which a valid fp8 call reaches last."""
import pytest
import torch

import torchrua_amd as ta

LENS = torch.tensor([2, 3])
E4M3 = torch.float8_e4m3fn


def cont(heads=2, dtype=E4M3, D=32):
    return ta.C(torch.zeros(int(LENS.sum()), heads, D, dtype=torch.bfloat16).to(dtype), LENS)


Q, KV, KV16 = cont(4, torch.bfloat16), cont(), cont(2, torch.bfloat16)
ONES = torch.ones(2)
REFUSALS = {
    'fp8 q': (lambda: cont(4).attention_decode(KV, KV, k_scale=1.0), '`q` is one of'),
    'k fp8, v not': (lambda: Q.attention_decode(KV, KV16), '`v` has dtype torch.bfloat16, `k` torch.float8_e4m3fn'),
    'v fp8, k not': (lambda: Q.attention_decode(KV16, KV), '`v` has dtype torch.float8_e4m3fn, `k` torch.bfloat16'),
    'e5m2': (lambda: Q.attention_decode(cont(dtype=torch.float8_e5m2), KV), '`k` has dtype torch.float8_e5m2.*float8_e4m3fn'),
    'e4m3fnuz': (lambda: Q.attention_decode(KV, cont(dtype=torch.float8_e4m3fnuz)), '`v` has dtype .*fnuz.*float8_e4m3fn'),
    'e5m2fnuz': (lambda: Q.attention_decode(cont(dtype=torch.float8_e5m2fnuz), KV), '`k` has dtype .*fnuz.*float8_e4m3fn'),
    'uint8': (lambda: Q.attention_decode(cont(dtype=torch.uint8), cont(dtype=torch.uint8)), '`k` has dtype torch.uint8.*float8_e4m3fn'),
    'k_scale with bf16': (lambda: Q.attention_decode(KV16, KV16, k_scale=2.0), '`k_scale` is given'),
    'v_scale with bf16': (lambda: Q.attention_decode(KV16, KV16, v_scale=ONES), '`v_scale` is given'),
    'scale float64': (lambda: Q.attention_decode(KV, KV, k_scale=ONES.double()), '`k_scale` is a float32 tensor'),
    'scale shape': (lambda: Q.attention_decode(KV, KV, v_scale=torch.ones(4)), r'`v_scale` is a float32 tensor \[heads_kv\] = \[2\]'),
    'scale 2-D': (lambda: Q.attention_decode(KV, KV, k_scale=torch.ones(2, 1)), '`k_scale` is a float32 tensor'),
    'scale device': (lambda: Q.attention_decode(KV, KV, k_scale=torch.ones(2, device='meta')), '`k_scale` is a float32 tensor'),
    'scale grad': (lambda: Q.attention_decode(KV, KV, v_scale=ONES.clone().requires_grad_()), '`v_scale` .*requiring grad'),
    'scale 0': (lambda: Q.attention_decode(KV, KV, k_scale=0.0), '`k_scale` = 0.0'),
    'scale negative': (lambda: Q.attention_decode(KV, KV, v_scale=-1), '`v_scale` = -1'),
    'scale inf': (lambda: Q.attention_decode(KV, KV, k_scale=float('inf')), '`k_scale` = inf'),
    'scale nan': (lambda: Q.attention_decode(KV, KV, v_scale=float('nan')), '`v_scale` = nan'),
    'scale True': (lambda: Q.attention_decode(KV, KV, k_scale=True), '`k_scale` = True'),
    'scale str': (lambda: ta.segment_attention_decode(Q.data, LENS, KV.data, KV.data, LENS, v_scale='1'), "`v_scale` = '1'"),
    # valid calls: only the device is wrong, and that refusal comes last
    'cpu': (lambda: Q.attention_decode(KV, KV, k_scale=0.5, v_scale=ONES, kv_chunk=128), '`q` lives on cpu'),
    'segment cpu': (lambda: ta.segment_attention_decode(Q.data, LENS, KV.data, KV.data, LENS, k_scale=ONES, v_scale=3),
                    '`q` lives on cpu'),
    'bf16 through the new signature': (lambda: Q.attention_decode(KV16, KV16, k_scale=None, v_scale=None), '`q` lives on cpu'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_name_their_argument(case):
    call, match = REFUSALS[case]
    with pytest.raises(ta.RuaError, match=match):
        call()
