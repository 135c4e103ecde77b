"""Device-resident dataset: a whole split lives on the GPU, downprojected once, and a training batch is ONE kernel launch.

Reference: HDF5Dataset (common/utils.py:101-265) + torch DataLoader read a [250, 200] float64 trajectory from HDF5 per sample, run
F.conv2d on the CPU to downproject it (every epoch again), collate and copy to the device; GraphCreator.create_data / create_graph
(:300-428) then gather, permute, repeat and concatenate the batch, with one blocking host-to-device copy per equation parameter.  An
E2 training split is 2048 x 250 x 100 floats = 205 MB at base resolution, so here:

    downproject(...)        the reference's downprojection formulas, vectorised over the sample axis, float64, run once;
    DeviceDataset           the float32 store [S, nt, comps, nx], grid, time axis and parameter table on the device;
    DeviceDataset.batch     node rows, labels, positions and parameter columns of a batch from (sample indices, time steps) by one
                            msmp_batch_assemble_f32 launch (csrc/batch_assemble_kernel.hip), no host read-back;
    DeviceDataset.advance   create_next_graph (:431-471): labels and pos[:, 0] of the next unrolling step by a mode-1 launch;
    DeviceDataset.loader    epoch iterator of index lists, sharded over ranks like dist.shard_range;
    random_steps            the start steps of experiments/train_helper.py:94-97.

Datasets larger than device memory and background prefetch are out of scope.  There is no CPU fallback: `batch` needs the library."""
import random as _random

import numpy as np
import torch

from . import _lib
from .dist import shard_range
from .graph import Data, GraphStructure, torch_time_axis

_CHUNK = 128                # samples per downprojection step: bounds the float64 temporaries (128 x 250 x 204 x 8 B = 52 MB)

# parameter columns in the order of GraphCreator.create_graph (common/utils.py:388-426), with the sign each is stored with (:392)
VARIABLES = {
    'CE': (('alpha', 1.0), ('beta', -1.0), ('gamma', 1.0)),
    'KF': (('r', 1.0), ('D', 1.0)),
    'KS': (),
    'WE': (('bc_left', 1.0), ('bc_right', 1.0), ('c', 1.0)),
    'AD': (('a', 1.0), ('b', 1.0)),
}


def _tensor(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def _taps(padded, taps, weight, stride):
    """sum_j weight * padded[..., j + stride * i]: F.conv2d with a [1, taps] kernel of equal weights and stride (1, stride)."""
    n_out = (padded.shape[-1] - taps) // stride + 1
    span = (n_out - 1) * stride + 1
    out = weight * padded[..., 0:span:stride]
    for j in range(1, taps):
        out = out + weight * padded[..., j:j + span:stride]
    return out


def _downproject_chunk(name, unstructured, u, ratio_nt, ratio_nx):
    """One chunk of samples, float64.  HDF5Dataset.__getitem__ (common/utils.py:167-261) without the sample loop."""
    if name in ('CE', 'KS', 'KF'):
        u = u[:, ::ratio_nt]
        if name == 'KF':                    # zero padding (:191-193)
            pad = torch.zeros_like(u[..., :2])
            padded = torch.cat((pad, u, pad), -1)
        else:                               # periodic padding u[..., -3:-1] | u | u[..., 1:3] (:170-172, :209-211)
            padded = torch.cat((u[..., -3:-1], u, u[..., 1:3]), -1)
        return _taps(padded, 5, 0.2, ratio_nx)
    if name == 'WE':                        # box filter, no padding (:224-226)
        return _taps(u[:, ::ratio_nt], ratio_nx, 1. / ratio_nx, ratio_nx)
    if name == 'AD':                        # [S, 2, nt, nx_super] -> [S, nt, 2, nx] (:244-261)
        if not unstructured:
            u = u[..., 0:-1:2]
        return u.transpose(1, 2)
    raise ValueError(f'unknown pde {name}')


def downproject(pde, u_super, ratio_nt, ratio_nx, x_super=None):
    """(u, x): the training trajectories HDF5Dataset.__getitem__ returns as `u_super`, for all samples at once, in float64 on the
    device of the input.  u_super: [S, nt_super, nx_super] (AD: the file layout [S, 2, nt, nx_super]; with `pde.untructured_grid` the
    BASE array, which the reference returns in place of a downprojection, :253-255).  Returns u [S, nt, nx] (AD: [S, nt, 2, nx]) and
    the grid: for WE `x_super` under the same box filter (:229-230), otherwise `x_super` as it came (the other experiments read the
    base grid from the file's attributes).  AD needs ratio_nt == 1: the reference's `[::ratio_nt]` slices the component axis there."""
    name = f'{pde}'
    ratio_nt, ratio_nx = int(ratio_nt), int(ratio_nx)
    if ratio_nt < 1 or ratio_nx < 1:
        raise ValueError(f'downproject: ratios must be positive integers, not {ratio_nt}, {ratio_nx}')
    if name not in VARIABLES:
        raise ValueError(f'unknown pde {name}')
    unstructured = bool(getattr(pde, 'untructured_grid', False))
    if name == 'AD' and ratio_nt != 1:
        raise ValueError('downproject: AD needs ratio_nt == 1 (the reference slices the component axis with [::ratio_nt], common/utils.py:244)')
    u_super = _tensor(u_super)
    if u_super.dim() != (4 if name == 'AD' else 3):
        raise ValueError(f'downproject: {name} trajectories must have {4 if name == "AD" else 3} dimensions, not {tuple(u_super.shape)}')
    out = None
    for s0 in range(0, u_super.shape[0], _CHUNK):
        piece = _downproject_chunk(name, unstructured, u_super[s0:s0 + _CHUNK].to(torch.float64), ratio_nt, ratio_nx)
        if out is None:
            out = torch.empty((u_super.shape[0],) + tuple(piece.shape[1:]), dtype=torch.float64, device=u_super.device)
        out[s0:s0 + _CHUNK] = piece
    x = x_super
    if name == 'WE' and x_super is not None:
        x = _taps(_tensor(x_super).to(torch.float64), ratio_nx, 1. / ratio_nx, ratio_nx)
    return out, x


def random_steps(creator, batch_size, unrolled_graphs, rng=None):
    """`batch_size` start steps drawn like experiments/train_helper.py:94-97: uniformly from
    tw .. t_res - tw - tw * unrolled_graphs.  rng: a random.Random (default: the module `random`, as the reference)."""
    steps = range(creator.tw, creator.t_res - creator.tw - creator.tw * unrolled_graphs + 1)
    if len(steps) == 0:
        raise ValueError(f'random_steps: no start step leaves room for {unrolled_graphs} unrolled windows of {creator.tw} in {creator.t_res} steps')
    return (rng or _random).choices(steps, k=batch_size)


class _Loader(object):
    """Epoch iterator of DeviceDataset.loader: every `iter()` is one epoch of index lists."""

    def __init__(self, n_samples, batch_size, shuffle, drop_last, generator, rank, world):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f'loader: bad batch_size={batch_size}, rank={rank}, world={world}')
        self.n, self.bs, self.shuffle, self.drop_last = int(n_samples), int(batch_size), shuffle, drop_last
        self.generator, self.rank, self.world = generator, rank, world

    def __len__(self):
        return self.n // self.bs if self.drop_last else -(-self.n // self.bs)

    def __iter__(self):
        order = (torch.randperm(self.n, generator=self.generator) if self.shuffle else torch.arange(self.n)).tolist()
        for i in range(0, self.n, self.bs):
            glob = order[i:i + self.bs]
            if len(glob) < self.bs and self.drop_last:
                return
            g0, g1 = shard_range(len(glob), self.rank, self.world)
            yield glob[g0:g1]


class DeviceDataset(object):
    """One split of a dataset on the device (module docstring).  Attributes: store float32 [S, nt, comps, nx]; x, x32 the [nx] grid in
    float64 and float32; t, t32 the time axis (graph.torch_time_axis: the reference's CPU linspace, so pos[:, 0] has its values);
    var_table float32 [S, n_vars] in the column order of GraphCreator.create_graph, CE's beta negated (common/utils.py:392); variables
    (the dict as given, for the reference's evaluation loops); u_base if given."""

    def __init__(self, pde, store, x, variables, device, u_base=None):
        name = f'{pde}'
        if name not in VARIABLES:
            raise ValueError(f'unknown pde {name}')
        self.pde, self.name = pde, name
        self.device = torch.device(device)
        if store.dim() != 4 or store.shape[2] != (2 if name == 'AD' else 1):
            raise ValueError(f'DeviceDataset: the store must be [S, nt, {2 if name == "AD" else 1}, nx], not {tuple(store.shape)}')
        if store.shape[1] != int(pde.grid_size[0]):
            raise ValueError(f'DeviceDataset: {store.shape[1]} time steps after the downprojection, pde.grid_size[0] = {pde.grid_size[0]}')
        self.store = store.to(self.device, torch.float32).contiguous()
        self.device = self.store.device                          # 'cuda' -> 'cuda:0': index tensors are compared against it
        self.n_samples, self.nt, self.comps, self.nx = (int(v) for v in self.store.shape)
        x = _tensor(x).detach().to(torch.float64).reshape(-1)
        if x.shape[0] != self.nx:
            raise ValueError(f'DeviceDataset: the grid has {x.shape[0]} points, the trajectories {self.nx}')
        self.x_host = x.cpu().contiguous()                       # build_edge_index evaluates the grid on the CPU
        self.x = x.to(self.device)
        self.x32 = self.x.to(torch.float32)
        t = torch_time_axis(pde)
        self.t = t.to(self.device)
        self.t32 = self.t.to(torch.float32)
        self.variables = dict(variables)
        cols = []
        for key, sign in VARIABLES[name]:
            v = _tensor(variables[key]).detach().reshape(-1)
            if v.shape[0] != self.n_samples:
                raise ValueError(f'DeviceDataset: variables[{key!r}] has {v.shape[0]} entries for {self.n_samples} samples')
            cols.append(sign * v.to(self.device))
        self.n_vars = len(cols)
        self.var_table = (torch.stack(cols, 1).to(torch.float32).contiguous() if cols
                          else torch.zeros(self.n_samples, 0, dtype=torch.float32, device=self.device))
        self.u_base = u_base
        self._structs = {}           # (batch size, neighbours) -> (edge_index, batch vector, GraphStructure): the same objects for every batch
        self._work = {}              # (batch size, time window, neighbours) -> the Data of working_batch
        self._scratch = {}         # node count -> [n_vars, N] columns for an `out=` whose columns are scattered in memory
        self._index_dev = {}       # batch size -> [2, B] int32 device buffer the host lists are copied into

    def __len__(self):
        return self.n_samples

    # -- construction --------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, pde, u_super, x, variables, base_resolution, super_resolution, device, u_base=None):
        """u_super: [S, nt_super, nx_super] (AD: [S, 2, nt, nx_super]; with pde.untructured_grid the reference trains on `u_base`, which
        must then be given), numpy or torch, host or device.  x: the [nx] grid of the base resolution; for WE the grid of the super
        resolution also works (it goes through the box filter, common/utils.py:229-230).  variables: dict of [S] arrays under the
        reference's names.  Downprojects once, chunk by chunk on `device`, and keeps the result in float32."""
        name = f'{pde}'
        device = torch.device(device)
        rt, rx = super_resolution[0] / base_resolution[0], super_resolution[1] / base_resolution[1]
        if not (float(rt).is_integer() and float(rx).is_integer()):
            raise ValueError(f'DeviceDataset: super_resolution {tuple(super_resolution)} is no integer multiple of base_resolution {tuple(base_resolution)}')
        rt, rx = int(rt), int(rx)
        if name == 'AD' and getattr(pde, 'untructured_grid', False):
            if u_base is None:
                raise ValueError('DeviceDataset: the unstructured AD experiments train on u_base (common/utils.py:253-255): pass it')
            src = u_base
        else:
            src = u_super
        store = None
        for s0 in range(0, src.shape[0], _CHUNK):          # sliced before it is converted: an HDF5 dataset is read chunk by chunk
            piece, _ = downproject(pde, _tensor(src[s0:s0 + _CHUNK]).to(device), rt, rx)
            if piece.dim() == 3:
                piece = piece[:, :, None, :]
            if store is None:
                store = torch.empty((src.shape[0],) + tuple(piece.shape[1:]), dtype=torch.float32, device=device)
            store[s0:s0 + _CHUNK] = piece
        if store is None:
            raise ValueError('DeviceDataset: no samples')
        x = _tensor(x).detach().to(torch.float64).reshape(-1)
        if name == 'WE' and x.shape[0] != store.shape[-1]:
            x = _taps(x, rx, 1. / rx, rx)
        return cls(pde, store, x, variables, device, u_base=u_base)

    @classmethod
    def from_hdf5(cls, file_or_path, pde, mode, base_resolution=None, super_resolution=None, device='cuda'):
        """The split `mode` ('train', 'valid', 'test') of a file written by the reference's generator, under the dataset and attribute
        names HDF5Dataset.__init__ reads (common/utils.py:123-145): `pde_{nt}-{nx}` at both resolutions, the base dataset's attribute
        `x` (WE: the super dataset's, downprojected), and one [S] dataset per equation parameter.  file_or_path: a path (needs h5py,
        imported only then) or an open mapping mode -> name -> array whose arrays carry `.attrs`."""
        name = f'{pde}'
        base_resolution = (250, 100) if base_resolution is None else base_resolution
        super_resolution = (250, 200) if super_resolution is None else super_resolution
        close = None
        if isinstance(file_or_path, (str, bytes)) or hasattr(file_or_path, '__fspath__'):
            try:
                import h5py
            except ImportError as exc:
                raise ImportError(f'DeviceDataset.from_hdf5({file_or_path!r}): reading a file from a path needs h5py, which is not installed; '
                                  'install it, or pass an open mapping mode -> name -> array (or use DeviceDataset.from_arrays)') from exc
            file_or_path = close = h5py.File(file_or_path, 'r')
        try:
            group = file_or_path[mode]
            base = group[f'pde_{base_resolution[0]}-{base_resolution[1]}']
            sup = group[f'pde_{super_resolution[0]}-{super_resolution[1]}']
            x = np.asarray(sup.attrs['x'] if name == 'WE' else base.attrs['x'])
            variables = {key: np.asarray(group[key][:]) for key, _ in VARIABLES[name]}
            u_base = np.asarray(base[:])
            ds = cls.from_arrays(pde, sup, x, variables, base_resolution, super_resolution, device, u_base=u_base)
        finally:
            if close is not None:
                close.close()
        return ds

    # -- epochs ----------------------------------------------------------------------------------------------------------------
    def loader(self, batch_size, shuffle=True, drop_last=True, generator=None, rank=0, world=1):
        """Epoch iterator of index lists: a host-side permutation (torch.randperm under `generator`; every rank must seed it alike),
        cut into global batches of `batch_size`, of which rank r gets the contiguous shard dist.shard_range(len, r, world)."""
        return _Loader(self.n_samples, batch_size, shuffle, drop_last, generator, rank, world)

    # -- batches ---------------------------------------------------------------------------------------------------------------
    def _indices(self, tw, indices, steps):
        """[2, B] -> (sample_idx, steps) int32 on the device.  Lists are range-checked here and go up in one pinned asynchronous copy;
        device tensors are used as they are (int32) or cast on the device, unchecked: the kernel answers a bad one with NaN rows."""
        if torch.is_tensor(indices) != torch.is_tensor(steps):
            raise TypeError('DeviceDataset.batch: give indices and steps both as lists or both as tensors')
        if torch.is_tensor(indices):
            if indices.dim() != 1 or indices.shape != steps.shape or indices.is_floating_point() or steps.is_floating_point():
                raise ValueError('DeviceDataset.batch: index tensors must be 1-D integer tensors of one length')
            if indices.device != self.device or steps.device != self.device:
                raise ValueError(f'DeviceDataset.batch: index tensors must be on {self.device} (lists are copied for you)')
            return indices.to(torch.int32).contiguous(), steps.to(torch.int32).contiguous()
        if len(indices) != len(steps) or not len(indices):
            raise ValueError(f'DeviceDataset.batch: {len(indices)} sample indices for {len(steps)} steps')
        if min(indices) < 0 or max(indices) >= self.n_samples:
            bad = next(i for i in indices if not 0 <= i < self.n_samples)
            raise IndexError(f'DeviceDataset.batch: sample index {bad} outside 0 .. {self.n_samples - 1}')
        if min(steps) < tw or max(steps) > self.nt - tw:
            bad = next(s for s in steps if not tw <= s <= self.nt - tw)
            raise ValueError(f'DeviceDataset.batch: step {bad} outside {tw} .. {self.nt - tw} (a window of {tw} steps on either side)')
        host = torch.tensor([indices, steps], dtype=torch.int32).pin_memory()      # pinned blocks are recycled only after the copy ran
        dev = self._index_dev.get(len(indices))
        if dev is None:
            dev = self._index_dev[len(indices)] = torch.empty(2, len(indices), dtype=torch.int32, device=self.device)
        dev.copy_(host, non_blocking=True)
        return dev[0], dev[1]

    def _structure(self, creator, bsz):
        key = (bsz, creator.n)
        st = self._structs.get(key)
        if st is None:
            # once per batch size (device builders + one CSR build, with their read-backs); every later batch reuses the objects
            edge_index = creator.build_edge_index(self.x_host, bsz, self.device)
            batch = torch.arange(bsz, device=self.device).repeat_interleave(self.nx)
            st = self._structs[key] = (edge_index, batch, GraphStructure(edge_index, batch, bsz * self.nx))
        return st

    def _check_creator(self, creator):
        if f'{creator.pde}' != self.name:
            raise ValueError(f'DeviceDataset: a {creator.pde} GraphCreator on a {self.name} dataset')
        if int(creator.pde.grid_size[0]) != self.nt or int(creator.pde.grid_size[1]) != self.nx:
            raise ValueError(f'DeviceDataset: the creator\'s grid {list(creator.pde.grid_size)} is not the dataset\'s [{self.nt}, {self.nx}]')

    def _column_names(self):
        return [key for key, _ in VARIABLES[self.name]]

    def batch(self, creator, indices, steps, out=None):
        """The graph batch GraphCreator.create_graph(*create_data(u, steps), x, variables, steps) makes of the samples `indices` at the
        start steps `steps` (common/utils.py:300-428), all float32: x, y [N, comps * tw], pos [N, 2], the experiment's [N, 1] columns,
        plus `batch` and `edge_index` (the same tensor objects for every batch of one size, with their GraphStructure attached, so
        nothing structural is rebuilt).  ONE msmp_batch_assemble_f32 launch; lists add one pinned asynchronous [2, B] int32 copy.
        out: a Data of the same batch size whose float32 tensors are written in place, without an allocation (columns that do not
        lie behind one another in memory, like the separately cloned ones of CapturedTrainStep.data, are filled by one small
        device copy each from a scratch buffer of the dataset)."""
        self._check_creator(creator)
        tw, nx, comps = creator.tw, self.nx, self.comps
        idx, stp = self._indices(tw, indices, steps)
        bsz = int(idx.shape[0])
        n = bsz * nx
        names = self._column_names()
        scatter = None
        if out is None:
            edge_index, batch, gs = self._structure(creator, bsz)
            x = torch.empty(n, comps * tw, dtype=torch.float32, device=self.device)
            y = torch.empty(n, comps * tw, dtype=torch.float32, device=self.device)
            pos = torch.empty(n, 2, dtype=torch.float32, device=self.device)
            out = Data(x=x, edge_index=edge_index, y=y, pos=pos, batch=batch)
            vars_ptr = None
            if self.n_vars:
                cols = torch.empty(self.n_vars, n, dtype=torch.float32, device=self.device)
                for v, key in enumerate(names):
                    setattr(out, key, cols[v].view(n, 1))
                vars_ptr = cols.data_ptr()
            out._msmp_structure = gs
        else:
            x, y, pos = out.x, out.y, out.pos
            for t, shape in ((x, (n, comps * tw)), (y, (n, comps * tw)), (pos, (n, 2))):
                if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == self.device and tuple(t.shape) == shape and t.is_contiguous()):
                    raise ValueError(f'DeviceDataset.batch(out=): x, y and pos must be contiguous float32 tensors on {self.device} of shapes '
                                     f'{(n, comps * tw)}, {(n, comps * tw)}, {(n, 2)}')
            targets = [getattr(out, key) for key in names]
            for t in targets:
                if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == self.device and t.numel() == n and t.is_contiguous()):
                    raise ValueError(f'DeviceDataset.batch(out=): every parameter column must be a contiguous float32 tensor of {n} values')
            if all(t.data_ptr() == targets[0].data_ptr() + 4 * n * v for v, t in enumerate(targets)):
                vars_ptr = targets[0].data_ptr() if targets else None
            else:
                scratch = self._scratch.get(n)
                if scratch is None:
                    scratch = self._scratch[n] =torch.empty(self.n_vars, n, dtype=torch.float32, device=self.device)
                vars_ptr, scatter = scratch.data_ptr(), (scratch, targets)
        L = _lib.lib()
        _lib.check(L.msmp_batch_assemble_f32(self.store.data_ptr(), self.n_samples, self.nt, comps, nx, idx.data_ptr(), stp.data_ptr(), bsz, tw,
                                             self.t32.data_ptr(), self.x32.data_ptr(), self.var_table.data_ptr() if self.n_vars else None,
                                             self.n_vars, 0, x.data_ptr(), y.data_ptr(), pos.data_ptr(), vars_ptr if self.n_vars else None,
                                             _lib.current_stream()), 'msmp_batch_assemble_f32')
        if scatter is not None:
            for v, t in enumerate(scatter[1]):
                t.view(-1).copy_(scatter[0][v])
        return out

    def working_batch(self, creator, indices, steps):
        """`batch` into a Data the dataset keeps per (batch size, time window) and overwrites at the next call: no allocation from the
        second batch on (train.dataset_training_step)."""
        key = (len(indices), creator.tw, creator.n)
        work = self._work.get(key)
        if work is None:
            work = self._work[key] = self.batch(creator, indices, steps)
            return work
        return self.batch(creator, indices, steps, out=work)

    def advance(self, graph, pred, indices, steps):
        """GraphCreator.create_next_graph (common/utils.py:431-471) for a graph made by `batch`: x becomes the prediction (the last
        comps * tw columns of cat(x, pred)), and the labels of the windows starting at `steps` and pos[:, 0] = t[steps] are written
        into graph.y / graph.pos by one mode-1 msmp_batch_assemble_f32 launch.  pos[:, 1], the parameter columns, batch and
        edge_index stay as they are."""
        tw = graph.y.shape[1] // self.comps
        keep = self.comps * tw
        n = graph.y.shape[0]
        for t, shape in ((graph.y, (n, keep)), (graph.pos, (n, 2))):
            if not (t.dtype == torch.float32 and t.device == self.device and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError('DeviceDataset.advance: graph.y and graph.pos must be the contiguous float32 tensors `batch` made')
        idx, stp = self._indices(tw, indices, steps)
        bsz = int(idx.shape[0])
        if bsz * self.nx != n:
            raise ValueError(f'DeviceDataset.advance: {bsz} indices for a graph of {n} nodes ({self.nx} per sample)')
        if pred.shape[1] == keep and graph.x.shape[1] == keep:
            graph.x = pred.to(graph.x.dtype)         # cat(x, pred)[:, keep:] == pred
        else:
            graph.x = torch.cat((graph.x, pred.to(graph.x.dtype)), 1)[:, keep:]
        L = _lib.lib()
        _lib.check(L.msmp_batch_assemble_f32(self.store.data_ptr(), self.n_samples, self.nt, self.comps, self.nx, idx.data_ptr(), stp.data_ptr(),
                                             bsz, tw, self.t32.data_ptr(), None, None, 0, 1, None, graph.y.data_ptr(),
                                             graph.pos.data_ptr(), None, _lib.current_stream()), 'msmp_batch_assemble_f32')
        return graph
