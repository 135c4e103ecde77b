#!/usr/bin/env python3
"""Generate tests/golden/dataset_{CE,KF,KS,WE,AD,ADu}.npz from the REFERENCE's own HDF5Dataset.__getitem__ (common/utils.py:156-264).

Runs only where the reference tree is present (like gen_golden.py, whose stand-ins for the third-party modules it reuses):

    python tests/golden/gen_golden_dataset.py

There is no HDF5 file and no h5py: the dataset object is made with object.__new__, its `data` is a dict of seeded in-memory arrays
(the reference's load_all mode holds a dict as well), and the arrays that need `.attrs` (WE reads the super-resolution grid from them)
are an ndarray subclass carrying them.  Each fixture holds 3 samples with nt = 12 and nx_super = 20 -> nx = 10: the inputs
(`in_super`, `in_base`, `in_x`, `in_x_super`, `in_<variable>`) and what __getitem__ returned per sample, stacked (`u_super`, `u_base`,
`x`, `var_<variable>`).  Data only, a few KB each."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
if not os.path.isdir(REF):
    sys.exit('reference tree not present: golden vectors can only be regenerated in the build container')
sys.path.insert(0, os.path.join(HERE, 'standins'))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import common.utils as U  # noqa: E402
from equations.PDEs import CE, WE, AD  # noqa: E402

assert torch.get_default_dtype() == torch.float64  # side effect of temporal/solvers.py:10

S, NT, NX, NX_SUPER = 3, 12, 10, 20
VARIABLES = {'CE': ('alpha', 'beta', 'gamma'), 'KF': ('r', 'D'), 'KS': (), 'WE': ('bc_left', 'bc_right', 'c'), 'AD': ('a', 'b')}


class WithAttrs(np.ndarray):
    """An array with the `.attrs` of an h5py dataset."""

    def __new__(cls, a, attrs):
        obj = np.asarray(a).view(cls)
        obj.attrs = dict(attrs)
        return obj

    def __array_finalize__(self, obj):
        self.attrs = getattr(obj, 'attrs', {})


class Named(object):
    """The reference dispatches on f'{pde}' and, for AD, reads `untructured_grid`."""

    def __init__(self, name, unstructured=False):
        self.name, self.untructured_grid = name, unstructured

    def __repr__(self):
        return self.name


def make(tag, seed):
    name = 'AD' if tag in ('AD', 'ADu') else tag
    rng = np.random.default_rng(seed)
    x_base = np.linspace(0., 16., NX)
    x_super = np.sort(rng.uniform(-8., 8., NX_SUPER)) if name == 'WE' else np.linspace(0., 16., NX_SUPER)
    shape_s, shape_b = ((S, 2, NT, NX_SUPER), (S, 2, NT, NX)) if name == 'AD' else ((S, NT, NX_SUPER), (S, NT, NX))
    u_s, u_b = rng.standard_normal(shape_s), rng.standard_normal(shape_b)
    ds = object.__new__(U.HDF5Dataset)
    ds.pde = Named(name, unstructured=(tag == 'ADu'))
    ds.mode, ds.dtype = 'train', torch.float64
    ds.base_resolution, ds.super_resolution = (NT, NX), (NT, NX_SUPER)
    ds.dataset_base, ds.dataset_super = f'pde_{NT}-{NX}', f'pde_{NT}-{NX_SUPER}'
    ds.data = {ds.dataset_base: WithAttrs(u_b, {'x': x_base}), ds.dataset_super: WithAttrs(u_s, {'x': x_super})}
    for v in VARIABLES[name]:
        ds.data[v] = rng.uniform(0.1, 2.0, S)
    # the ratios as HDF5Dataset.__init__ computes them (:133-138): for the AD layout [S, 2, nt, nx] they compare axes 1 and 2
    ds.ratio_nt = int(ds.data[ds.dataset_super].shape[1] / ds.data[ds.dataset_base].shape[1])
    ds.ratio_nx = int(ds.data[ds.dataset_super].shape[2] / ds.data[ds.dataset_base].shape[2])
    ds.x = x_base
    if name == 'KF':
        # The KF branch calls F.conv1d on the 4-D [1, 1, nt, nx + 4] tensor with a 4-D weight and a 2-D stride (:195), which the torch
        # of this image refuses ("Expected 2D (unbatched) or 3D (batched) input to conv1d").  With those arguments the call can only
        # mean the 2-D convolution its CE and KS siblings spell F.conv2d (:174, :213), so for this branch alone the name is bound to it.
        conv1d, U.F.conv1d = U.F.conv1d, U.F.conv2d
        try:
            items = [ds[i] for i in range(S)]
        finally:
            U.F.conv1d = conv1d
    else:
        items = [ds[i] for i in range(S)]
    out = {'in_super': u_s, 'in_base': u_b, 'in_x': x_base, 'in_x_super': x_super,
           'u_base': np.stack([np.asarray(it[0]) for it in items]), 'u_super': np.stack([np.asarray(it[1]) for it in items]),
           'x': np.stack([np.asarray(it[2]) for it in items]), 'ratio_nt': np.int64(ds.ratio_nt), 'ratio_nx': np.int64(ds.ratio_nx)}
    for v in VARIABLES[name]:
        out['in_' + v] = ds.data[v]
        out['var_' + v] = np.stack([np.asarray(it[3][v]) for it in items])
    assert out['u_super'].dtype == np.float64
    path = os.path.join(HERE, f'dataset_{tag}.npz')
    np.savez(path, **out)
    print(path, out['u_super'].shape, out['x'].shape, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    for k, tag in enumerate(('CE', 'KF', 'KS', 'WE', 'AD', 'ADu')):
        make(tag, 1000 + k)
