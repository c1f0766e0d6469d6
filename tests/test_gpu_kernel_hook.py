"""The names the kernel hook reports (torchrua_amd._ops.set_kernel_hook): bench.py keys its per-kernel timings on them,
and every launch goes through ONE bracket (_ops._call) — hook(name, True), the entry point, hook(name, False).  Each
operator runs once forward and once backward on a CattedSequence of lengths [2, 0, 5] with H = 3 in fp32: the smallest
shape with an empty sequence, a narrow unaligned row and a live backward.  The recorded sequence must be exactly the
operator's own pairs, in launch order."""
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib as K
from torchrua_amd import _ops as O
from torchrua_amd.layout import describe

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LENS = [2, 0, 5]


def _c(seed=0, grad=True):
    x = torch.randn(sum(LENS), 3, generator=torch.Generator().manual_seed(seed)).to(DEV).requires_grad_(grad)
    return ta.with_host_sizes(x, torch.tensor(LENS)), x


def _record(run):
    """The hook calls of run() -> a tensor (or None: forward only) and of the backward of its sum."""
    calls = []
    O.set_kernel_hook(lambda name, opening: calls.append((name, opening)))
    try:
        y = run()
        if y is not None:
            y.sum().backward()
        torch.cuda.synchronize()
    finally:
        O.set_kernel_hook(None)
    return calls


def _pairs(*names):
    return [(n, opening) for n in names for opening in (True, False)]


def _forward_only(_result) -> None:
    return None


def _index():
    c, _ = _c(grad=False)
    return c.argmax()


CASES = {
    'reduce_sum': (lambda: ta.reduce_sum(_c()[0]), ['reduce']),          # (the backward kernel carries no name)
    'reduce_max': (lambda: ta.reduce_max(_c()[0]), ['reduce']),          # (nor does the trailing rua_fill_empty)
    'softmax': (lambda: (_c()[0].softmax().data * _c(1, False)[1]), ['softmax', 'softmax_bwd']),
    'log_softmax': (lambda: (_c()[0].log_softmax().data * _c(1, False)[1]), ['log_softmax', 'log_softmax_bwd']),
    'cumsum': (lambda: _c()[0].cumsum().data, ['cumsum', 'cumsum_rev']),
    'cumsum_rev': (lambda: _c()[0].cumsum(reverse=True).data, ['cumsum_rev', 'cumsum']),
    'linear_scan': (lambda: _c()[0].linear_scan(_c(1)[0]).data, ['linear_scan', 'linear_scan_bwd']),
    'linear_scan_rev': (lambda: _c()[0].linear_scan(_c(1)[0], reverse=True).data,
                        ['linear_scan_rev', 'linear_scan_rev_bwd']),
    'linear_scan_scalar': (lambda: _c()[0].linear_scan(0.5).data, ['linear_scan', 'linear_scan_bwd']),
    'seq_max': (lambda: _c()[0].max().values, ['seq_max', 'put']),
    'seq_min': (lambda: _c()[0].min().values, ['seq_min', 'put']),
    'argmax': (lambda: _forward_only(_c()[0].argmax()), ['argmax']),
    'argmin': (lambda: _forward_only(_c()[0].argmin()), ['argmin']),
    'softmax_pool': (lambda: _c()[0].softmax_pool(_c(1)[1]), ['softmax_pool', 'softmax_pool_bwd']),
    'var_mean': (lambda: sum(_c()[0].var_mean()), ['var_mean', 'var_mean_bwd']),
    'var': (lambda: _c()[0].var(), ['var_mean', 'var_mean_bwd']),
    'standardize': (lambda: (_c()[0].standardize().data * _c(1, False)[1]), ['standardize', 'standardize_bwd']),
    'to_left': (lambda: _c()[0].left().data, ['to_left', 'to_left_bwd']),
    'to_pack': (lambda: _c()[0].pack().data, ['to_pack', 'to_pack_bwd']),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_hook_sequence(case):
    run, names = CASES[case]
    assert _record(run) == _pairs(*names)


def test_hook_sequence_take_put():
    """take and put are each other's adjoint: the backward of one is the other's launch."""
    index = _index()
    c, x = _c()
    lay, hidden = describe(c), (3,)
    assert _record(lambda: O.take(x, index, lay, hidden)) == _pairs('take', 'put')
    src = torch.randn(3, 3, device=DEV, requires_grad=True)
    assert _record(lambda: O.put(src, index, lay, hidden, tuple(x.shape))) == _pairs('put', 'take')


def test_hook_is_restored_and_silent_when_unset():
    """No hook, no calls — and a refused launch leaves the hook where it was (the bracket does not swallow the error)."""
    calls = []
    O.set_kernel_hook(lambda name, opening: calls.append((name, opening)))
    try:
        c, _ = _c(grad=False)
        with pytest.raises(K.RuaError):
            O.launch_cumsum(describe(c), c.data.to(torch.int32), False, (3,))
        assert calls == []                                   # refused before the bracket opened
        assert O._kernel_hook is not None
    finally:
        O.set_kernel_hook(None)
    c.cumsum()
    assert calls == [] and O._kernel_hook is None
