"""CPU tests (no kernel launched) of the three entries that guard a training step -- msmp_grads_finite_f32 with its size query,
msmp_adamw_guarded_f32, msmp_status_poison_f32: the header declares them at the ABI version the library and the binding report, null
pointers, bad counts and a short workspace are refused by return value with msmp_last_error naming the entry, and the optimizer's
`skip_nonfinite` option is refused without `capturable`."""
import ctypes
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINITE, GUARDED, POISON, QUERY = 'msmp_grads_finite_f32', 'msmp_adamw_guarded_f32', 'msmp_status_poison_f32', 'msmp_grads_finite_workspace_bytes'
N = 3
NUMEL = (1, 5000, 12345)          # 1 + 2 + 4 chunks of 4096 elements


def table(values):
    """a host array of pointers (fake, never dereferenced: every case is refused before a launch); None stays NULL"""
    return (ctypes.c_void_p * len(values))(*values)


def numel(values=NUMEL):
    return (ctypes.c_int64 * len(values))(*values)


def finite(L, **kw):
    d = dict(n=N, grads=table([4096 * (i + 1) for i in range(N)]), numel=numel(), n_scalars=1, scalars=table([65536]), verdict=69632, ws=73728, stream=None)
    d.update(kw)
    if 'ws_bytes' not in d:
        d['ws_bytes'] = L.msmp_grads_finite_workspace_bytes(N, numel()) + d.pop('ws_delta', 0)
    return L.msmp_grads_finite_f32(d['n'], d['grads'], d['numel'], d['n_scalars'], d['scalars'], d['verdict'], d['ws'], d['ws_bytes'], d['stream'])


GUARDED_ORDER = ('n', 'params', 'grads', 'exp_avg', 'exp_avg_sq', 'numel', 'lr', 'beta1', 'beta2', 'eps', 'wd', 'step', 'verdict', 'skipped', 'stream')


def guarded(L, **kw):
    d = dict(n=N, numel=numel(), lr=1 << 20, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, step=(1 << 20) + 256, verdict=(1 << 20) + 512, skipped=(1 << 20) + 768,
             stream=None)
    for j, k in enumerate(('params', 'grads', 'exp_avg', 'exp_avg_sq')):
        d[k] = table([65536 * (j + 1) + 4096 * i for i in range(N)])
    d.update(kw)
    return L.msmp_adamw_guarded_f32(*[d[k] for k in GUARDED_ORDER])


def refused(L, rc, name, word, code=-1):
    assert rc == code, (rc, L.msmp_last_error())
    assert name.encode() in L.msmp_last_error() and word in L.msmp_last_error(), L.msmp_last_error()


def test_header_declares_and_library_exports_the_entries(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in (FINITE, GUARDED, POISON):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert re.search(r'\bsize_t\s+' + QUERY + r'\s*\(', header) and getattr(L, QUERY) is not None
    assert abi_versions_agree(header, L)
    import msmp_pde_amd._lib as B
    assert int(re.search(r'#define\s+MSMP_ABI_VERSION\s+(\d+)', header).group(1)) == B.MSMP_ABI_VERSION == L.msmp_version()
    assert re.search(r'#define\s+MSMP_NONFINITE_GRAD\s+1\b', header) and re.search(r'#define\s+MSMP_NONFINITE_SCALAR\s+2\b', header)
    # each prototype cites the reference's loop / optimizer, as its neighbours do
    for name in (FINITE, GUARDED, POISON):
        comment = header[:header.index('int ' + name)].rsplit('/*', 1)[1]
        assert 'experiments/train_helper.py:125-141' in comment or 'experiments/train.py:410' in comment, name


@pytest.mark.parametrize('pointer', ['grads', 'numel', 'scalars', 'verdict', 'ws'])
def test_finite_check_refuses_null_pointers(L, pointer):
    refused(L, finite(L, **{pointer: None}), FINITE, b'null')


def test_finite_check_refuses_null_entries_of_its_tables(L):
    refused(L, finite(L, grads=table([4096, None, 12288])), FINITE, b'null')
    refused(L, finite(L, scalars=table([None])), FINITE, b'null')


def test_finite_check_refuses_bad_counts(L):
    for kw in (dict(n=-1), dict(n_scalars=-1), dict(n_scalars=5)):
        refused(L, finite(L, **kw), FINITE, b'bad counts')
    for bad in (-1, 1 << 31, 1 << 40):
        refused(L, finite(L, numel=numel((1, bad, 12345)), ws_bytes=1 << 40), FINITE, b'element count')


def test_finite_check_takes_no_tensors_and_no_scalars_by_null(L):
    """nothing to read: NULL tables are fine then, and the refusal that is left is the workspace's"""
    refused(L, finite(L, n=0, grads=None, numel=None, n_scalars=0, scalars=None, ws_bytes=0), FINITE, b'workspace', code=-3)


def test_finite_check_refuses_a_workspace_one_byte_short(L):
    refused(L, finite(L, ws_delta=-1), FINITE, b'workspace', code=-3)
    refused(L, finite(L, ws_bytes=0), FINITE, b'workspace', code=-3)


def test_the_size_query(L):
    q = L.msmp_grads_finite_workspace_bytes
    assert q(N, numel()) == 4 * (1 + 2 + 4)                   # one int32 word per 4096-element block
    assert q(2, numel((4096, 4097))) == 4 * (1 + 2)
    assert q(1, numel((0,))) == 4 and q(0, None) == 4           # never an empty workspace: the entry wants a pointer
    assert q(-1, numel()) == 0 and q(1, None) == 0 and q(1, numel((-1,))) == 0 and q(1, numel((1 << 31,))) == 0


@pytest.mark.parametrize('pointer', ['params', 'grads', 'exp_avg', 'exp_avg_sq', 'numel', 'lr', 'step', 'verdict', 'skipped'])
def test_guarded_adamw_refuses_null_pointers(L, pointer):
    refused(L, guarded(L, **{pointer: None}), GUARDED, b'null')


def test_guarded_adamw_refuses_null_entries_bad_counts_and_bad_betas(L):
    for k in ('params', 'grads', 'exp_avg', 'exp_avg_sq'):
        refused(L, guarded(L, **{k: table([4096, 8192, None])}), GUARDED, b'null')
    refused(L, guarded(L, n=-1), GUARDED, b'null pointer')
    for bad in (-1, 1 << 31):
        refused(L, guarded(L, numel=numel((1, 5000, bad))), GUARDED, b'element count')
    for kw in (dict(beta1=1.0), dict(beta2=-0.1)):
        refused(L, guarded(L, **kw), GUARDED, b'hyper-parameters')


def test_status_poison_refuses_a_null_pointer(L):
    refused(L, L.msmp_status_poison_f32(None, None), POISON, b'null')


def test_the_existing_adamw_entries_keep_their_prototypes():
    import msmp_pde_amd._lib as B
    c = ctypes
    assert B.SIGNATURES['msmp_adamw_capturable_f32'] == (c.c_int, [c.c_int] + [c.c_void_p] * 6 + [c.c_float] * 4 + [c.c_void_p] * 2)
    assert B.SIGNATURES['msmp_adamw_guarded_f32'] == (c.c_int, [c.c_int] + [c.c_void_p] * 6 + [c.c_float] * 4 + [c.c_void_p] * 4)


def test_skip_nonfinite_needs_capturable():
    import torch
    import msmp_pde_amd as mp
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match='capturable'):
        mp.optim.AdamW([p], skip_nonfinite=True)
    opt = mp.optim.AdamW([p], capturable=True, skip_nonfinite=True)
    assert opt.skip_nonfinite and opt.skipped_steps == 0 and 'skip_nonfinite' not in opt.state_dict()['param_groups'][0]
    assert not mp.optim.AdamW([p]).skip_nonfinite
    with pytest.raises(ValueError, match='single-element'):
        opt.watch(torch.zeros(2))


def test_a_range_policy_needs_skip_nonfinite():
    import torch
    import msmp_pde_amd as mp
    from msmp_pde_amd import train as T
    p = torch.nn.Parameter(torch.zeros(3))
    plain = mp.optim.AdamW([p], capturable=True)
    for policy in ('auto', 'sync'):
        with pytest.raises(ValueError, match='skip_nonfinite'):
            T._check_policy(policy, plain)
        T._check_policy(policy, mp.optim.AdamW([p], capturable=True, skip_nonfinite=True))
    T._check_policy(None, plain)
    with pytest.raises(ValueError, match='range_policy'):
        T._check_policy('warn', plain)
