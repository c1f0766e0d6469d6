"""The path table of tests/test_gpu_reduce_paths.py stays complete: every reduce kernel template of rua_reduce_impl.h
is named by the expected trace of at least one case, so a kernel added without a case fails on any machine."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_SEGMENT_REDUCE = {'scatter_self_grad_kernel'}     # scatter_*'s own family


def _kernels():
    text = open(os.path.join(ROOT, 'torchrua_amd', 'csrc', 'rua_reduce_impl.h')).read()
    return set(re.findall(r'__global__[^;{]*?\bvoid\s+(\w+)', text))


def _expected_traces():
    """Every string of the `fwd` / `bwd` / `bwd_prod` fields of the Case(...) rows of PATHS, read without importing
    the GPU module."""
    tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_gpu_reduce_paths.py')).read())
    paths = next(n.value for n in tree.body if isinstance(n, ast.Assign) and any(
        isinstance(t, ast.Name) and t.id == 'PATHS' for t in n.targets))
    seen = []
    for call in paths.elts:
        assert isinstance(call, ast.Call) and call.func.id == 'Case'
        for kw in call.keywords:
            if kw.arg in ('fwd', 'bwd', 'bwd_prod'):
                seen += [e.value for e in kw.value.elts]
    return seen


def test_the_kernel_grep_finds_the_reduce_family():
    ks = _kernels()
    assert {'seg_reduce_kernel', 'seg_reduce_team_kernel', 'seg_reduce_ranks_kernel', 'seg_reduce_tail_kernel',
            'seg_reduce_combine_kernel', 'seg_backward_kernel', 'seg_backward_tail_kernel', 'seg_backward_walk_kernel',
            'seg_backward_ranks_kernel', 'seg_backward_rows_kernel', 'fill_empty_kernel',
            'scatter_self_grad_kernel'} <= ks


def test_every_reduce_kernel_has_a_path_case():
    named = {t.split()[0] for t in _expected_traces()}
    missing = sorted(_kernels() - NOT_SEGMENT_REDUCE - named)
    assert not missing, f'reduce kernels no case of test_gpu_reduce_paths.PATHS expects to reach: {missing}'
    unknown = sorted(named - _kernels())
    assert not unknown, f'expected traces name kernels rua_reduce_impl.h does not define: {unknown}'
