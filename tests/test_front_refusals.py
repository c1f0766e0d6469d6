"""The Python-side refusals of the per-sequence operators that change raggedness or take a side argument, in one table:
compress, repeat_interleave, sort / argsort / reorder / topk, unique_consecutive, window_pool, join / unjoin,
softmax_pool, linear_scan and causal_conv.  No GPU: every container here lives on the host, so a call that passes its
argument checks ends in "no CPU fallback" — and every row whose message is a specific one is a double fault by
construction (a host payload AND a bad argument): the specific refusal has to win.

Each row names what the message must hold: the operator, the argument's noun and the offending value (a type name, a
dtype, a shape or a device).  Public API only.

Cells the table leaves out, because the call does not end in a RuaError there (the operator reads `sequence.data` first):
"not a container" for compress, repeat_interleave, softmax_pool, linear_scan and causal_conv.  softmax_pool and
linear_scan check the payload's device BEFORE they look at the scores / the gate; their rows pin that order.
"""
import pytest
import torch

import torchrua_amd as ta

LENS = [2, 0, 3]
HIDDEN = (2,)
NO_CPU = 'no CPU fallback'
BOOL, I32, I64, F32, F64 = torch.bool, torch.int32, torch.int64, torch.float32, torch.float64


def _containers(dtype=F32):
    """C / L / P / R over the same three sequences, built from their fields (a cast would need the device)."""
    sizes = torch.tensor(LENS)
    x = torch.arange(10).view(5, 2).to(dtype)
    s0, s2 = x[:2], x[2:]
    left, right = torch.zeros(3, 3, 2, dtype=dtype), torch.zeros(3, 3, 2, dtype=dtype)
    left[0, :2], left[2, :3] = s0, s2
    right[0, 1:], right[2, :] = s0, s2
    packed = ta.P(data=torch.stack([s2[0], s0[0], s2[1], s0[1], s2[2]]), batch_sizes=torch.tensor([2, 2, 1]),
                  sorted_indices=torch.tensor([2, 0, 1]), unsorted_indices=torch.tensor([1, 2, 0]))
    return {'C': ta.C(x, sizes), 'L': ta.L(left, sizes), 'P': packed, 'R': ta.R(right, sizes)}


def _lead(z):
    return tuple(z.data.shape[:1]) if isinstance(z, (ta.C, ta.P)) else tuple(z.data.shape[:2])


ZS = _containers()
OTHER = {'C': 'L', 'L': 'R', 'P': 'C', 'R': 'P'}
ROWS = []


def row(name, call, *needles, wins=True):
    """`call()` must raise a RuaError whose message holds every needle; wins: it is not the device refusal."""
    ROWS.append(pytest.param(call, needles, wins, id=name))


# ---- a per-token side argument: the mask of compress, the counts of repeat_interleave, the indices of reorder
for op, noun, good, bad in (('compress', 'mask', BOOL, torch.uint8), ('repeat_interleave', 'repeats', I64, I32),
                            ('reorder', 'indices', I64, I32)):
    for kind, z in ZS.items():
        f, lead = getattr(ta, op), _lead(z)
        other = ZS[OTHER[kind]]
        longer = (lead[0] + 1,) + lead[1:]
        # (reorder also takes the full storage shape, one index per element: its "too many dimensions" is another width)
        wide = lead + ((3,) if op == 'reorder' else HIDDEN)
        row(f'{op}-{kind}-type', lambda f=f, z=z: f(z, [1] * 5), op, noun, 'list')
        row(f'{op}-{kind}-dtype', lambda f=f, z=z, lead=lead, bad=bad: f(z, torch.ones(lead, dtype=bad)), op, noun, str(bad))
        row(f'{op}-{kind}-hidden', lambda f=f, z=z, wide=wide, good=good: f(z, torch.ones(wide, dtype=good)), op, noun,
            str(wide), *(() if op == 'reorder' else ('hidden dimensions',)))
        row(f'{op}-{kind}-shape', lambda f=f, z=z, longer=longer, good=good: f(z, torch.ones(longer, dtype=good)), op, noun,
            str(longer), str(lead))
        row(f'{op}-{kind}-container', lambda f=f, z=z, other=other, good=good:
            f(z, other._replace(data=torch.ones(_lead(other), dtype=good))), op, noun, type(other).__name__,
            type(z).__name__)
        row(f'{op}-{kind}-device', lambda f=f, z=z, lead=lead, good=good: f(z, torch.ones(lead, dtype=good, device='meta')),
            op, noun, 'meta')
        # the argument is fine, and so is the same argument inside a container of the same type: the device refusal
        row(f'{op}-{kind}-fits', lambda f=f, z=z, lead=lead, good=good: f(z, torch.ones(lead, dtype=good)), NO_CPU, wins=False)
        row(f'{op}-{kind}-fits-in-a-container', lambda f=f, z=z, lead=lead, good=good:
            f(z, z._replace(data=torch.ones(lead, dtype=good))), NO_CPU, wins=False)
    seg = getattr(ta, 'segment_' + op, None)
    if seg is not None:
        x, sizes = ZS['C']
        row(f'segment_{op}-dtype', lambda seg=seg, bad=bad: seg(x, torch.ones(5, dtype=bad), sizes), 'segment_' + op, noun,
            str(bad))
        row(f'segment_{op}-hidden', lambda seg=seg, good=good: seg(x, torch.ones(5, 2, dtype=good), sizes), 'segment_' + op,
            noun, '(5, 2)', 'hidden dimensions')
        row(f'segment_{op}-shape', lambda seg=seg, good=good: seg(x, torch.ones(4, dtype=good), sizes), 'segment_' + op, noun,
            '(4,)', '(5,)')
        row(f'segment_{op}-device', lambda seg=seg, good=good: seg(x, torch.ones(5, dtype=good, device='meta'), sizes),
            'segment_' + op, noun, 'meta')

for kind, z in ZS.items():
    lead = _lead(z)
    row(f'repeat_interleave-{kind}-bool', lambda z=z, lead=lead: z.repeat_interleave(torch.ones(lead, dtype=BOOL)),
        'repeat_interleave', 'repeats', 'torch.bool', 'compress(mask)')
    row(f'repeat_interleave-{kind}-negative', lambda z=z: z.repeat_interleave(-3), 'repeat_interleave', 'repeats', '-3')
    row(f'repeat_interleave-{kind}-huge', lambda z=z: z.repeat_interleave(2 ** 31), 'repeat_interleave', 'repeats', str(2 ** 31))
    row(f'repeat_interleave-{kind}-float', lambda z=z: z.repeat_interleave(1.5), 'repeat_interleave', 'repeats', 'float')
    row(f'reorder-{kind}-per-element-fits', lambda z=z: z.reorder(torch.zeros(z.data.shape, dtype=I64)), NO_CPU, wins=False)

# ---- not a container
for op, args in (('sort', ()), ('argsort', ()), ('reorder', (torch.zeros(5, dtype=I64),)), ('topk', (1,)),
                 ('unique_consecutive', ()), ('window_pool', (2,)), ('unjoin', ([1],))):
    row(f'{op}-not-a-container', lambda op=op, args=args: getattr(ta, op)([ZS['C'].data], *args), op, 'container', 'list')
    row(f'{op}-tensor-for-a-container', lambda op=op, args=args: getattr(ta, op)(ZS['C'].data, *args), op, 'container', 'Tensor')

# ---- the arguments of the operators without a per-token side argument
for kind, z in ZS.items():
    ints = _containers(I32)[kind]
    for op in ('sort', 'argsort'):
        row(f'{op}-{kind}-payload-dtype', lambda op=op, ints=ints: getattr(ta, op)(ints), op, 'torch.int32')
        row(f'{op}-{kind}-fits', lambda op=op, z=z: getattr(ta, op)(z), NO_CPU, wins=False)
    row(f'topk-{kind}-k', lambda z=z: z.topk(-1), 'topk', 'k', '-1')
    row(f'topk-{kind}-k-type', lambda z=z: z.topk(1.5), 'topk', 'k', '1.5')
    row(f'topk-{kind}-fits', lambda z=z: z.topk(1), NO_CPU, wins=False)
    row(f'unique_consecutive-{kind}-complex', lambda kind=kind: _containers(torch.complex64)[kind].unique_consecutive(),
        'unique_consecutive', 'complex', 'torch.complex64')
    row(f'unique_consecutive-{kind}-fits', lambda z=z: z.unique_consecutive(True, True), NO_CPU, wins=False)
    row(f'window_pool-{kind}-kernel', lambda z=z: z.window_pool(0), 'window_pool', 'kernel_size', '0')
    row(f'window_pool-{kind}-kernel-type', lambda z=z: z.window_pool(2.0), 'window_pool', 'kernel_size', 'float')
    row(f'window_pool-{kind}-stride', lambda z=z: z.window_pool(2, 0), 'window_pool', 'stride', '0')
    row(f'window_pool-{kind}-mode', lambda z=z: z.window_pool(2, mode='min'), 'window_pool', 'mode', "'min'")
    row(f'window_pool-{kind}-payload-dtype', lambda ints=ints: ints.window_pool(2), 'window_pool', 'torch.int32')
    row(f'window_pool-{kind}-fits', lambda z=z: z.window_pool(2), NO_CPU, wins=False)

    # join: the parts
    other = ZS[OTHER[kind]]
    row(f'join-{kind}-not-a-list', lambda z=z: ta.join(z), 'join', 'list of parts', type(z).__name__)
    row(f'join-{kind}-part-type', lambda z=z: ta.join([z, 'x']), 'join', 'part 1', 'str')
    row(f'join-{kind}-mixed', lambda z=z, other=other: z.join(other), 'join', type(z).__name__, type(other).__name__)
    row(f'join-{kind}-tensor-shape', lambda z=z: z.join(torch.zeros(3, 5)), 'join', 'part 1', '(3, 5)', '(3, 2)')
    row(f'join-{kind}-dtype', lambda z=z, ints=ints: z.join(ints), 'join', 'part 1', 'torch.int32')
    row(f'join-{kind}-device', lambda z=z: z.join(torch.zeros(3, 2, device='meta')), 'join', 'different devices', 'meta')
    row(f'join-{kind}-fits', lambda z=z: z.join(torch.zeros(3, 2), z), NO_CPU, wins=False)
    # unjoin: the sizes, one value per SEQUENCE
    row(f'unjoin-{kind}-not-a-list', lambda z=z: ta.unjoin(z, 1), 'unjoin', 'list of sizes', 'int')
    row(f'unjoin-{kind}-size-type', lambda z=z: z.unjoin('x'), 'unjoin', 'size 0', "'x'")
    row(f'unjoin-{kind}-size-dtype', lambda z=z: z.unjoin(1, torch.ones(3, dtype=I32)), 'unjoin', 'size 1', 'torch.int32')
    row(f'unjoin-{kind}-size-shape', lambda z=z: z.unjoin(torch.ones(4, dtype=I64)), 'unjoin', 'size 0', '(4,)')
    row(f'unjoin-{kind}-size-negative', lambda z=z: z.unjoin(-1), 'unjoin', 'size 0', '-1')
    row(f'unjoin-{kind}-size-device', lambda z=z: z.unjoin(torch.ones(3, dtype=I64, device='meta')), 'unjoin',
        'different devices', 'meta')
    row(f'unjoin-{kind}-fits', lambda z=z: z.unjoin(1, torch.ones(3, dtype=I64)), NO_CPU, wins=False)

    # causal_conv: the filter and the bias are checked against the payload before anything asks for a device
    row(f'causal_conv-{kind}-weight-shape', lambda z=z: z.causal_conv(torch.zeros(3, 5)), 'causal_conv', 'weight', '(3, 5)',
        '(2,)')
    row(f'causal_conv-{kind}-taps', lambda z=z: z.causal_conv(torch.zeros(9, 2)), 'causal_conv', 'K', '9')
    row(f'causal_conv-{kind}-weight-dtype', lambda z=z: z.causal_conv(torch.zeros(3, 2, dtype=F64)), 'causal_conv', 'weight',
        'torch.float64')
    row(f'causal_conv-{kind}-bias-shape', lambda z=z: z.causal_conv(torch.zeros(3, 2), torch.zeros(3)), 'causal_conv', 'bias',
        '(3,)')
    row(f'causal_conv-{kind}-bias-dtype', lambda z=z: z.causal_conv(torch.zeros(3, 2), torch.zeros(2, dtype=F64)),
        'causal_conv', 'bias', 'torch.float64')
    row(f'causal_conv-{kind}-fits', lambda z=z: z.causal_conv(torch.zeros(3, 2), torch.zeros(2)), NO_CPU, wins=False)

    # softmax_pool and linear_scan ask for the payload's device first: on a host payload that refusal wins, whatever
    # the scores / the gate are
    lead = _lead(z)
    for name, arg in (('fits', torch.zeros(lead)), ('type', [0.0] * 5), ('dtype', torch.zeros(lead, dtype=F64)),
                      ('shape', torch.zeros((lead[0] + 1,) + lead[1:])), ('device', torch.zeros(lead, device='meta')),
                      ('container', other._replace(data=torch.zeros(_lead(other))))):
        row(f'softmax_pool-{kind}-{name}', lambda z=z, arg=arg: z.softmax_pool(arg), NO_CPU, 'cpu', wins=False)
        row(f'linear_scan-{kind}-{name}', lambda z=z, arg=arg: z.linear_scan(arg), NO_CPU, 'cpu', wins=False)


@pytest.mark.parametrize('call, needles, wins', ROWS)
def test_refusal(call, needles, wins):
    with pytest.raises(ta.RuaError) as caught:
        call()
    message = str(caught.value)
    for needle in needles:
        assert needle in message, (needle, message)
    assert (NO_CPU not in message) == wins, message


def test_the_table_covers_every_operator():
    ids = {p.id.split('-')[0] for p in ROWS}
    assert ids >= {'compress', 'segment_compress', 'repeat_interleave', 'segment_repeat_interleave', 'sort', 'argsort',
                   'reorder', 'topk', 'unique_consecutive', 'window_pool', 'join', 'unjoin', 'softmax_pool', 'linear_scan',
                   'causal_conv'}
    assert len(ROWS) == len({p.id for p in ROWS})
