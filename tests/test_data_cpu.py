"""CPU tests of msmp_pde_amd.data: the downprojection against what the reference's HDF5Dataset.__getitem__ returned
(tests/golden/dataset_*.npz, written by tests/golden/gen_golden_dataset.py), the thin HDF5 reader on a fake mapping, the epoch
loader, the start steps and the host range checks of DeviceDataset.batch.  No kernel is launched and no device is needed."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import load

S, NT, NX, NX_SUPER = 3, 12, 10, 20
VARS = {'CE': ('alpha', 'beta', 'gamma'), 'KF': ('r', 'D'), 'KS': (), 'WE': ('bc_left', 'bc_right', 'c'), 'AD': ('a', 'b')}


@pytest.fixture(scope='module')
def D():
    from msmp_pde_amd import data
    return data


class Pde(object):
    """f'{pde}', grid_size, tmin / tmax and untructured_grid are all the data path reads of a PDE object."""

    def __init__(self, name, unstructured=False, nt=NT, nx=NX):
        self.name, self.untructured_grid = name, unstructured
        self.tmin, self.tmax, self.grid_size, self.L = 0.0, 4.0, [nt, nx], 16.0

    def __repr__(self):
        return self.name


def pde_of(tag, **kw):
    return Pde('AD' if tag in ('AD', 'ADu') else tag, unstructured=(tag == 'ADu'), **kw)


# ---- downproject against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['CE', 'KF', 'KS', 'WE'])
def test_downproject_matches_the_reference_to_rounding(D, tag):
    """|delta| <= 8 * 2^-52 * max|u_super|: each side makes at most six roundings of relative 2^-53 (five products or sums of taps
    and the scaling) on sums bounded by max|u|, so two sides give 6 * 2^-52, and 8 leaves slack for the order of summation."""
    d = load(f'dataset_{tag}.npz')
    u, x = D.downproject(pde_of(tag), torch.tensor(d['in_super']), int(d['ratio_nt']), int(d['ratio_nx']),
                         x_super=torch.tensor(d['in_x_super']))
    assert u.dtype == torch.float64 and tuple(u.shape) == (S, NT, NX)
    bound = 8 * 2.0 ** -52 * np.abs(d['in_super']).max()
    err = np.abs(u.numpy() - d['u_super']).max()
    print(f'{tag}: max|delta| = {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    if tag == 'WE':           # the grid goes through the same filter (common/utils.py:229-230)
        assert np.abs(x.numpy() - d['x'][0]).max() <= 8 * 2.0 ** -52 * np.abs(d['in_x_super']).max()


@pytest.mark.parametrize('tag', ['AD', 'ADu'])
def test_downproject_of_the_two_component_layout_is_exact(D, tag):
    d = load(f'dataset_{tag}.npz')
    src = d['in_base'] if tag == 'ADu' else d['in_super']          # the unstructured experiments train on the base array
    u, _ = D.downproject(pde_of(tag), src, int(d['ratio_nt']), int(d['ratio_nx']))
    assert tuple(u.shape) == (S, NT, 2, NX)
    assert np.array_equal(u.numpy(), d['u_super'])


def test_downproject_of_ad_refuses_a_time_ratio(D):
    with pytest.raises(ValueError, match='ratio_nt == 1'):
        D.downproject(pde_of('AD'), np.zeros((2, 2, 8, 8)), 2, 2)


def test_downproject_at_ratio_4_and_time_ratio_2_against_a_loop(D):
    rng = np.random.default_rng(7)
    u = rng.standard_normal((2, 10, 24))
    rt, rx = 2, 4
    for name in ('CE', 'KF', 'WE'):
        if name == 'WE':
            padded = u[:, ::rt]
            taps, w = rx, 1. / rx
        else:
            v = u[:, ::rt]
            left, right = (np.zeros_like(v[..., :2]),) * 2 if name == 'KF' else (v[..., -3:-1], v[..., 1:3])
            padded = np.concatenate((left, v, right), -1)
            taps, w = 5, 0.2
        n_out = (padded.shape[-1] - taps) // rx + 1
        want = np.zeros(padded.shape[:2] + (n_out,))
        for s in range(padded.shape[0]):
            for t in range(padded.shape[1]):
                for i in range(n_out):
                    acc = 0.0
                    for j in range(taps):
                        acc = acc + w * padded[s, t, i * rx + j]
                    want[s, t, i] = acc
        got, _ = D.downproject(Pde(name), u, rt, rx)
        assert tuple(got.shape) == want.shape == (2, 5, 6)
        assert np.abs(got.numpy() - want).max() <= 8 * 2.0 ** -52 * np.abs(u).max(), name


# ---- the dataset object ---------------------------------------------------------------------------------------------------------
def dataset_of(D, tag, device='cpu'):
    d = load(f'dataset_{tag}.npz')
    name = 'AD' if tag in ('AD', 'ADu') else tag
    variables = {v: d['in_' + v] for v in VARS[name]}
    ds = D.DeviceDataset.from_arrays(pde_of(tag), d['in_super'], d['in_x_super'] if tag == 'WE' else d['in_x'], variables, (NT, NX),
                                     (NT, NX_SUPER), device, u_base=d['in_base'])
    return ds, d


@pytest.mark.parametrize('tag', ['CE', 'KF', 'KS', 'WE', 'AD', 'ADu'])
def test_from_arrays_keeps_the_reference_sample_layout_in_float32(D, tag):
    ds, d = dataset_of(D, tag)
    comps = 2 if tag in ('AD', 'ADu') else 1
    assert ds.store.dtype == torch.float32 and tuple(ds.store.shape) == (S, NT, comps, NX) and ds.store.is_contiguous()
    want = torch.tensor(d['u_super']).reshape(S, NT, comps, NX)
    # float32 roundings of two float64 values a few 2^-52 apart are the same number or neighbours: one float32 ulp, 2^-23 relative
    assert (ds.store.double() - want.float().double()).abs().max() <= 2.0 ** -23 * want.abs().max()
    if comps == 2:
        assert torch.equal(ds.store, want.float())
    assert ds.x.dtype == torch.float64 and ds.x32.dtype == torch.float32
    assert np.abs(ds.x.numpy() - d['x'][0]).max() <= 8 * 2.0 ** -52 * 16
    assert torch.equal(ds.t, torch.linspace(0.0, 4.0, NT, dtype=torch.float64)) and torch.equal(ds.t32, ds.t.float())
    name = 'AD' if comps == 2 else tag
    assert tuple(ds.var_table.shape) == (S, len(VARS[name])) and ds.var_table.dtype == torch.float32
    for v, key in enumerate(VARS[name]):
        sign = -1.0 if (name, key) == ('CE', 'beta') else 1.0          # common/utils.py:392
        assert torch.equal(ds.var_table[:, v], torch.tensor(sign * d['var_' + key]).float())
    assert len(ds) == S and ds.u_base is not None


def test_from_arrays_refuses_a_store_that_does_not_fit_the_pde(D):
    d = load('dataset_CE.npz')
    variables = {v: d['in_' + v] for v in VARS['CE']}
    with pytest.raises(ValueError, match='time steps'):
        D.DeviceDataset.from_arrays(pde_of('CE', nt=NT + 1), d['in_super'], d['in_x'], variables, (NT, NX), (NT, NX_SUPER), 'cpu')
    with pytest.raises(ValueError, match='grid has'):
        D.DeviceDataset.from_arrays(pde_of('CE'), d['in_super'], d['in_x'][:-1], variables, (NT, NX), (NT, NX_SUPER), 'cpu')
    with pytest.raises(ValueError, match='entries for'):
        D.DeviceDataset.from_arrays(pde_of('CE'), d['in_super'], d['in_x'], dict(variables, beta=d['in_beta'][:2]), (NT, NX),
                                    (NT, NX_SUPER), 'cpu')


class FakeDataset(np.ndarray):
    """An array with `.attrs`, like an h5py dataset."""

    def __new__(cls, a, **attrs):
        obj = np.asarray(a).view(cls)
        obj.attrs = attrs
        return obj

    def __array_finalize__(self, obj):
        self.attrs = getattr(obj, 'attrs', {})


@pytest.mark.parametrize('tag', ['CE', 'WE', 'AD'])
def test_from_hdf5_reads_an_open_mapping_under_the_reference_names(D, tag):
    ds_arrays, d = dataset_of(D, tag)
    name = 'AD' if tag == 'AD' else tag
    group = {f'pde_{NT}-{NX}': FakeDataset(d['in_base'], x=d['in_x']), f'pde_{NT}-{NX_SUPER}': FakeDataset(d['in_super'], x=d['in_x_super'])}
    for v in VARS[name]:
        group[v] = d['in_' + v]
    ds = D.DeviceDataset.from_hdf5({'train': group, 'valid': {}}, pde_of(tag), 'train', (NT, NX), (NT, NX_SUPER), 'cpu')
    assert torch.equal(ds.store, ds_arrays.store) and torch.equal(ds.x, ds_arrays.x) and torch.equal(ds.var_table, ds_arrays.var_table)
    assert np.array_equal(np.asarray(ds.u_base), d['in_base'])


def test_from_hdf5_on_a_path_says_that_h5py_is_missing(D):
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match='needs h5py, which is not installed'):
            D.DeviceDataset.from_hdf5('/nonexistent/CE_train_E2.h5', pde_of('CE'), 'train', device='cpu')
    else:
        with pytest.raises(OSError):
            D.DeviceDataset.from_hdf5('/nonexistent/CE_train_E2.h5', pde_of('CE'), 'train', device='cpu')


# ---- loader and start steps -----------------------------------------------------------------------------------------------------
def big_dataset(D, n=23):
    rng = np.random.default_rng(3)
    return D.DeviceDataset.from_arrays(pde_of('KS'), rng.standard_normal((n, NT, NX_SUPER)), np.linspace(0, 16, NX), {}, (NT, NX),
                                       (NT, NX_SUPER), 'cpu')


def test_loader_epochs_are_seeded_permutations(D):
    ds = big_dataset(D)
    gen = lambda: torch.Generator().manual_seed(11)
    full = D.DeviceDataset.loader(ds, 4, drop_last=False, generator=gen())
    epoch = list(full)
    assert len(epoch) == len(full) == 6 and [len(b) for b in epoch] == [4] * 5 + [3]
    assert sorted(i for b in epoch for i in b) == list(range(23))
    dropped = ds.loader(4, generator=gen())
    assert list(dropped) == epoch[:5] and len(dropped) == 5
    a, b = ds.loader(4, generator=gen()), ds.loader(4, generator=gen())
    first, second = list(a), list(a)
    assert first != second                                         # a new permutation every epoch ...
    assert [list(b), list(b)] == [first, second]                   # ... and the same ones under the same seed
    assert [i for bt in ds.loader(5, shuffle=False, drop_last=False) for i in bt] == list(range(23))


def test_loader_shards_are_disjoint_and_cover_each_global_batch(D):
    ds = big_dataset(D)
    gen = lambda: torch.Generator().manual_seed(5)
    whole = list(ds.loader(5, drop_last=False, generator=gen()))
    r0 = list(ds.loader(5, drop_last=False, generator=gen(), rank=0, world=2))
    r1 = list(ds.loader(5, drop_last=False, generator=gen(), rank=1, world=2))
    assert len(whole) == len(r0) == len(r1) == 5
    for g, a, b in zip(whole, r0, r1):
        assert a + b == g and not set(a) & set(b)
        assert len(a) - len(b) in (0, 1)
    with pytest.raises(ValueError):
        ds.loader(4, rank=2, world=2)


@pytest.mark.parametrize('unrolled', [0, 1, 2])
def test_random_steps_stay_inside_the_reference_range(D, unrolled):
    creator = SimpleNamespace(tw=5, t_res=40)
    draws = D.random_steps(creator, 4000, unrolled, random.Random(0))
    lo, hi = 5, 40 - 5 * (1 + unrolled)
    assert len(draws) == 4000 and min(draws) == lo and max(draws) == hi          # 4000 draws from at most 31 values reach both ends
    assert D.random_steps(creator, 8, unrolled, random.Random(1)) == D.random_steps(creator, 8, unrolled, random.Random(1))
    with pytest.raises(ValueError):
        D.random_steps(SimpleNamespace(tw=5, t_res=14), 4, 1)


# ---- host range checks of batch ---------------------------------------------------------------------------------------------------
def test_batch_refuses_bad_lists_before_any_library_call(D, monkeypatch):
    from msmp_pde_amd import _lib

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'lib', no_library)
    ds, _ = dataset_of(D, 'CE')
    creator = SimpleNamespace(pde=pde_of('CE'), tw=3, n=2, t_res=NT)
    with pytest.raises(IndexError, match='sample index 3'):
        ds.batch(creator, [0, 3], [3, 3])
    with pytest.raises(IndexError, match='sample index -1'):
        ds.batch(creator, [-1, 0], [3, 3])
    with pytest.raises(ValueError, match='step 2 outside 3 .. 9'):
        ds.batch(creator, [0, 1], [3, 2])
    with pytest.raises(ValueError, match='step 10 outside 3 .. 9'):
        ds.batch(creator, [0, 1], [10, 3])
    with pytest.raises(ValueError, match='2 sample indices for 1 steps'):
        ds.batch(creator, [0, 1], [3])
    with pytest.raises(TypeError):
        ds.batch(creator, [0, 1], torch.tensor([3, 3]))
    with pytest.raises(ValueError, match='GraphCreator on a CE dataset'):
        ds.batch(SimpleNamespace(pde=pde_of('WE'), tw=3, n=2), [0], [3])
